"""CPU-emulated run (tests/emu) of the SPAM co-occurrence counts (tfft_spam_batch[_dev]): counts == the numpy
restatement of the definition, exactly, through the host and the _dev form.  Not the product path (see test_emulated.py);
tests/test_gpu_spam.py is the gate on the MI355X."""
import os
import subprocess

import numpy as np
import pytest

import spam_cases as SC
from parity_cases import HostBufs
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


# 1x1, 3x9, 9x3: empty directions; 4x4: one triple per diagonal; 47x5, 50x6, 101x37, 100x30: 3w mod 4 = 1, 2, 3, 0; 300x9; 64x64.
# The kernel's tile is SC.TILE_COLS = 256 pixel columns by SC.TILE_ROWS = 13 rows (a band of rows is a multiple of 13): w 1, 2, 3 past 256 and
# h 1, 2, 3 past 13 and past 26, so that the 3-pixel halo crosses a tile edge every possible way, in both dimensions
SHAPES = [(1, 1), (3, 9), (9, 3), (4, 4), (47, 5), (50, 6), (101, 37), (100, 30), (300, 9), (64, 64),
          (257, 14), (258, 15), (259, 16), (257, 29), (258, 27), (259, 28)]


def test_the_shapes_cross_the_tile_every_way():
    assert sorted({w - SC.TILE_COLS for (w, h) in SHAPES if w > SC.TILE_COLS and w < 300}) == [1, 2, 3]
    assert sorted({h % SC.TILE_ROWS for (w, h) in SHAPES if w > SC.TILE_COLS and w < 300}) == [1, 2, 3]
    assert sorted({(3 * w) % 4 for (w, h) in SHAPES[4:8]}) == [0, 1, 2, 3]


@pytest.mark.parametrize("w,h", SHAPES)
def test_counts_equal_the_definition(emu, w, h):
    SC.check_shape(emu, HostBufs, w, h, t=3, seed=w + h)


@pytest.mark.parametrize("t", [1, 2, 4])
def test_other_truncations(emu, t):
    SC.check_shape(emu, HostBufs, 101, 37, t=t, seed=t)


@pytest.mark.parametrize("slots", [1, 2])
def test_batch_equals_single_calls(emu, slots):
    imgs = np.stack([cover_rgb(101, 37, 30 + i) for i in range(3)])      # images 1 and 2 start at odd, unaligned bytes
    assert (101 * 37 * 3) % 4 != 0 and (2 * 101 * 37 * 3) % 4 != 0
    SC.check_batch_equals_singles(emu, HostBufs, imgs, slots)


def test_repeated_calls_return_identical_bytes(emu):
    SC.check_images(emu, HostBufs, np.stack([cover_rgb(50, 6, 1), SC.flat(50, 6)]), slots=1, repeat=True)


def test_errors(emu):
    SC.check_errors(emu)


@pytest.mark.parametrize("slots", [1, 2])
def test_resident_image_survives_the_call(emu, slots):
    SC.check_slots_after_spam(emu, HostBufs, slots=slots)
