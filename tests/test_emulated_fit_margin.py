"""CPU-emulated run (tests/emu) of what the fitted embed promises about its margin, its counts and its frozen images, against an fp64
restatement of DESIGN.md section 10 (tests/fit_margin_cases.py).  Not the product path (see test_emulated.py);
tests/test_gpu_fit_margin.py is the gate on the MI355X."""
import os
import subprocess

import pytest

import fit_margin_cases as MC
from parity_cases import HostBufs
from steganosaurus_amd import binding as B

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


@pytest.mark.parametrize("margin", [0.25, 0.5, 1.0])
@pytest.mark.parametrize("combo", list(MC.COMBOS))
def test_margin_holds_where_convergence_is_reported(emu, orc, combo, margin):
    MC.check_margin(emu, orc, HostBufs, combo, margin)


@pytest.mark.parametrize("max_iters", [0, 1, 2])
@pytest.mark.parametrize("combo", list(MC.COMBOS))
def test_counts_mid_flight(emu, orc, combo, max_iters):
    # the host form beside the device form once: 100 x 300 after one correction
    MC.check_counts(emu, orc, HostBufs, combo, max_iters, host=(combo, max_iters) == ("100x300", 1))


@pytest.mark.parametrize("margin_bins,max_iters", [(301, 1), (301, 32), (0, 1), (0, 32)])
def test_partition_with_a_remainder(emu, orc, margin_bins, max_iters):
    n_bins, nblk, per = MC.check_partition(emu, orc, HostBufs, 120, 200, margin_bins, max_iters)
    assert (n_bins, nblk, per) == ((2557, 3, 853) if margin_bins else (2256, 3, 752))


@pytest.mark.parametrize("margin_bins", [2, 301])
def test_partition_counts_every_entry(emu, orc, margin_bins):
    # the one-shot bytes of six images: a sixth of each stream reads wrong, and wrong_out is the fp64 count only if no entry is left out
    n_bins, nblk, per = MC.check_partition(emu, orc, HostBufs, 120, 200, margin_bins, 0, nimg=6)
    assert n_bins % nblk != 0


@pytest.mark.parametrize("max_iters", [1, 16])
def test_partition_at_the_cap(emu, orc, max_iters):
    n_bins, nblk, per = MC.check_partition(emu, orc, HostBufs, 300, 400, 66001 - 2256, max_iters)
    assert (n_bins, nblk, per, n_bins - 63 * per) == (66001, 64, 1032, 985)


def test_converged_images_are_frozen(emu, orc):
    MC.check_freezing(emu, orc, HostBufs)


def test_permuted_batch(emu, orc):
    MC.check_permutation(emu, orc, HostBufs)


def test_images_alone(emu, orc):
    MC.check_singles(emu, orc, HostBufs)


def test_floor_bound_cover(emu, orc):
    MC.check_floor_bound(emu, orc, HostBufs)


@pytest.mark.parametrize("max_iters", [0, 2, 12])
def test_clamping_covers(emu, orc, max_iters):
    MC.check_clamping(emu, orc, HostBufs, max_iters)
