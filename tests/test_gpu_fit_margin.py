"""What the fitted embed promises about its margin, its counts and its frozen images, on a real MI355X, against an fp64 restatement of
DESIGN.md section 10 (tests/fit_margin_cases.py): the cases of tests/test_emulated_fit_margin.py through the product library."""
import pytest

import fit_margin_cases as MC
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


@pytest.mark.parametrize("margin", [0.25, 0.5, 1.0])
@pytest.mark.parametrize("combo", list(MC.COMBOS))
def test_margin_holds_where_convergence_is_reported(lib, orc, combo, margin):
    MC.check_margin(lib, orc, TorchBufs, combo, margin)


@pytest.mark.parametrize("max_iters", [0, 1, 2])
@pytest.mark.parametrize("combo", list(MC.COMBOS))
def test_counts_mid_flight(lib, orc, combo, max_iters):
    # the host form beside the device form once: 100 x 300 after one correction
    MC.check_counts(lib, orc, TorchBufs, combo, max_iters, host=(combo, max_iters) == ("100x300", 1))


@pytest.mark.parametrize("margin_bins,max_iters", [(301, 1), (301, 32), (0, 1), (0, 32)])
def test_partition_with_a_remainder(lib, orc, margin_bins, max_iters):
    n_bins, nblk, per = MC.check_partition(lib, orc, TorchBufs, 120, 200, margin_bins, max_iters)
    assert (n_bins, nblk, per) == ((2557, 3, 853) if margin_bins else (2256, 3, 752))


@pytest.mark.parametrize("margin_bins", [2, 301])
def test_partition_counts_every_entry(lib, orc, margin_bins):
    # the one-shot bytes of six images: a sixth of each stream reads wrong, and wrong_out is the fp64 count only if no entry is left out
    n_bins, nblk, per = MC.check_partition(lib, orc, TorchBufs, 120, 200, margin_bins, 0, nimg=6)
    assert n_bins % nblk != 0


@pytest.mark.parametrize("max_iters", [1, 16])
def test_partition_at_the_cap(lib, orc, max_iters):
    n_bins, nblk, per = MC.check_partition(lib, orc, TorchBufs, 300, 400, 66001 - 2256, max_iters)
    assert (n_bins, nblk, per, n_bins - 63 * per) == (66001, 64, 1032, 985)


def test_converged_images_are_frozen(lib, orc):
    MC.check_freezing(lib, orc, TorchBufs)


def test_permuted_batch(lib, orc):
    MC.check_permutation(lib, orc, TorchBufs)


def test_images_alone(lib, orc):
    MC.check_singles(lib, orc, TorchBufs)


def test_floor_bound_cover(lib, orc):
    MC.check_floor_bound(lib, orc, TorchBufs)


@pytest.mark.parametrize("max_iters", [0, 2, 12])
def test_clamping_covers(lib, orc, max_iters):
    MC.check_clamping(lib, orc, TorchBufs, max_iters)
