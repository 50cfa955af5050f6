"""CPU-emulated run (tests/emu) of the exact batched capacities (tfft_set_batch_exact): usable_out of the batched embeds equals the
reference's integer (the oracle, bit-identical to the reference, and the reference-made golden vectors), the stego bytes those of mode
OFF.  Not the product path (see test_emulated.py); tests/test_gpu_exact_batch.py is the gate on the MI355X."""
import os
import subprocess

import pytest

import exact_batch_cases as XC
from parity_cases import HostBufs
from steganosaurus_amd import binding as B

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


# 96 x 64 x 3 in 2 slots (two chunks) and the golden geometries, uncentred and centred, with the four (rmin, rmax, magmin) cases
@pytest.mark.parametrize("w,h", [(48, 40), (100, 30), (64, 64)])
@pytest.mark.parametrize("center", [0, 1])
def test_all_mode_is_the_reference_integer(emu, orc, golden_dir, w, h, center):
    XC.check_geometry(emu, orc, HostBufs, golden_dir, w, h, center)


@pytest.mark.parametrize("center", [0, 1])
def test_all_mode_two_chunks(emu, orc, center):
    covers = XC.np.stack([XC.cover_rgb(96, 64, 30 + i) for i in range(3)])
    XC.check_all_dev(emu, HostBufs, XC.oracle_want(orc, covers, center, emu), covers, center, slots=2)


def test_host_stream_form(emu, orc):
    XC.check_host_stream(emu, orc, 96, 64, 0)


def test_walks_and_fit(emu, orc):
    XC.check_walks_and_fit(emu, orc, HostBufs, 100, 120)


def test_near_mode(emu, orc):
    XC.check_near(emu, HostBufs, orc, 64, 48)


def test_off_mode_one_pixel_wide_and_errors(emu):
    XC.check_off_and_errors(emu, HostBufs, 48, 40)
