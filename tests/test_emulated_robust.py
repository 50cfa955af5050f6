"""CPU-emulated run (tests/emu) of the robustness analysis calls (tfft_channel_batch[_dev], tfft_robustness_batch[_dev]): the AWGN and
JPEG-quantisation channels against their fp64 restatements in numpy, every form of the calls against each other, the robustness counts
against the composition of public calls that defines them, and the error codes.  Not the product path (see test_emulated.py);
tests/test_gpu_robust.py is the gate on the MI355X."""
import os
import subprocess

import pytest

import robust_cases as RC
from parity_cases import HostBufs
from steganosaurus_amd import binding as B

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")

# W, H not multiples of 8 (edge blocks), 3W mod 4 = 3 (101: every row has another byte shift), one and several strips of blocks
SHAPES = [(48, 40), (100, 30), (101, 37), (64, 64), (256, 256)]


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


@pytest.mark.parametrize("w,h", SHAPES)
def test_awgn_against_the_reference(emu, w, h):
    RC.check_awgn_shape(emu, HostBufs, w, h)


@pytest.mark.parametrize("w,h", SHAPES)
def test_jpeg_against_the_reference(emu, w, h):
    RC.check_jpeg_shape(emu, HostBufs, w, h)


def test_jpeg_wider_than_one_strip(emu):
    # 300 columns: a full strip of 32 blocks, then a partial one whose last block is completed from column 299
    RC.check_jpeg_shape(emu, HostBufs, 300, 9, n=2, qualities=(75,))


def test_channel_errors(emu):
    RC.check_channel_errors(emu, HostBufs)


def test_channel_calls_leave_the_slots_alone(emu):
    RC.check_channel_leaves_slots(emu, HostBufs)


# 256^2 with a 12 + 16-byte payload, 3 images in 2 slots and in 1: plain list / sorted list + bit index, without / with jitter + adaptive alpha
@pytest.mark.parametrize("sort,phase", [(False, False), (True, False), (False, True), (True, True)])
def test_robustness_equals_the_composition_256(emu, sort, phase):
    case = RC.make_case(emu, HostBufs, 256, 256, 3, 28, sort, phase)
    RC.check_robustness(emu, HostBufs, case)


def test_robustness_centred_128(emu):
    # 128^2, centred, a header and an empty message (16-byte tag); the list no longer than the stream (64^2 cannot hold 912 + 56*16 positions)
    case = RC.make_case(emu, HostBufs, 128, 128, 3, 16, True, False, center=True, extra_bins=0)
    RC.check_robustness(emu, HostBufs, case)


def test_coarser_quantiser_costs_more_raw_bits(emu):
    RC.check_jpeg_order(emu, HostBufs, RC.make_case(emu, HostBufs, 256, 256, 2, 28, True, False))


def test_robustness_errors(emu):
    RC.check_robust_errors(emu, HostBufs, RC.make_case(emu, HostBufs, 128, 128, 2, 16, False, False, extra_bins=40))
