"""The quality and channel kernels on the MI355X where they clamp and where tiles end (tests/saturating_cases.py): AWGN and JPEG on
contents that reach 0 and 255 at 101x37, 259x17 and 5x3, SSE / SSIM on pairs of such contents at 11x11 and 75x43, an SSE beyond 2^32, and
SSIM at 74x42, 75x43, 85x53 and 139x75 -- 1080p and 4K are multiples of the 64-window tile, so a partial tile in x, and a bar that sees one
row of windows, run on the device only here."""
import pytest

import saturating_cases as SC
from parity_cases import TorchBufs
from steganosaurus_amd import binding as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    # torch's HIP runtime first: initialised after the library's in the same process it finds no device
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")


@pytest.fixture(scope="module")
def lib():
    return B.load()


@pytest.mark.parametrize("w,h", SC.SATURATING_SHAPES)
@pytest.mark.parametrize("kind", ["full", "sat", "edges", "white", "black"])
def test_awgn_on_saturating_content(lib, kind, w, h):
    SC.check_awgn_saturating(lib, TorchBufs, kind, w, h)


@pytest.mark.parametrize("w,h", SC.SATURATING_SHAPES)
@pytest.mark.parametrize("kind", SC.SATURATING)
def test_jpeg_on_saturating_content(lib, kind, w, h):
    SC.check_jpeg_saturating(lib, TorchBufs, kind, w, h)


@pytest.mark.parametrize("kind", SC.SATURATING_PAIRS)
@pytest.mark.parametrize("w,h", [(11, 11), (75, 43)])
def test_quality_saturating(lib, w, h, kind):
    a, b = SC.saturating_pair(kind, w, h)
    SC.check_quality_pair(lib, TorchBufs, a, b, slots=2)


def test_quality_sse_beyond_32_bits(lib):
    SC.check_quality_sse_wide(lib)


@pytest.mark.parametrize("w,h", SC.TILE_SHAPES)
def test_quality_tile_edges(lib, w, h):
    SC.check_quality_tiles(lib, TorchBufs, w, h)
