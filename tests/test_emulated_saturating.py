"""CPU-emulated run (tests/emu) of the quality and channel kernels where they clamp and where tiles end (tests/saturating_cases.py): AWGN
and JPEG on contents that reach 0 and 255, SSE / SSIM on pairs of such contents, an SSE beyond 2^32, and SSIM at shapes that end inside a
tile at a bar that sees one row of windows.  Not the product path (see test_emulated.py); tests/test_gpu_saturating.py is the gate on the
MI355X."""
import os
import subprocess

import pytest

import saturating_cases as SC
from parity_cases import HostBufs
from steganosaurus_amd import binding as B

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


@pytest.mark.parametrize("w,h", SC.SATURATING_SHAPES)
@pytest.mark.parametrize("kind", ["full", "sat", "edges", "white", "black"])
def test_awgn_on_saturating_content(emu, kind, w, h):
    SC.check_awgn_saturating(emu, HostBufs, kind, w, h)


@pytest.mark.parametrize("w,h", SC.SATURATING_SHAPES)
@pytest.mark.parametrize("kind", SC.SATURATING)
def test_jpeg_on_saturating_content(emu, kind, w, h):
    SC.check_jpeg_saturating(emu, HostBufs, kind, w, h)


# one window (11 x 11) and a second tile column and row holding one window column / row (75 x 43)
@pytest.mark.parametrize("kind", SC.SATURATING_PAIRS)
@pytest.mark.parametrize("w,h", [(11, 11), (75, 43)])
def test_quality_saturating(emu, w, h, kind):
    a, b = SC.saturating_pair(kind, w, h)
    SC.check_quality_pair(emu, HostBufs, a, b, slots=2)


def test_quality_sse_beyond_32_bits(emu):
    SC.check_quality_sse_wide(emu)


@pytest.mark.parametrize("w,h", SC.TILE_SHAPES)
def test_quality_tile_edges(emu, w, h):
    SC.check_quality_tiles(emu, HostBufs, w, h)
