"""CPU-emulated run (tests/emu) of the batched pipelines' phase options, tfft_set_phase_options: jitter and adaptive alpha in the
delta embed, the tile-resident read and the generic paths, against the fp64 reference.  Not the product path (see test_emulated.py);
tests/test_gpu_phase_batch.py is the gate on the MI355X."""
import os
import subprocess

import numpy as np
import pytest

import phase_cases as PH
from _checkers import Params
from parity_cases import HostBufs
from steganosaurus_amd import binding as B

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


@pytest.mark.parametrize("kw", [dict(jitter=0.05), dict(jitter=0.0, adaptive=True), dict(jitter=0.05, adaptive=True, center=True)])
def test_batch_phase_options_sorted_two_chunks(emu, orc, kw):
    PH.check_phase_batch(emu, orc, HostBufs, 64, 64, 300, nimg=3, slots=2, sort=True, envs=({}, {"TFFT_MEDIAN_FALLBACK": "1"},
                                                                                           {"TFFT_STATS_FUSED": "0"}), lsb_frac=0.05, **kw)


def test_batch_phase_options_unsorted_two_step_columns(emu, orc):
    # PH = 512: two-step column plan (buckets per row group); the in-kernel statistics (TFFT_STATS_TILE=2) run on it
    PH.check_phase_batch(emu, orc, HostBufs, 100, 300, 300, nimg=2, slots=1, sort=False, jitter=0.05, adaptive=True,
                         envs=({}, {"TFFT_STATS_TILE": "2"}, {"TFFT_STATS_TILE": "0"}), lsb_frac=0.05)


def test_batch_phase_options_buckets_longer_than_the_registers(emu, orc):
    # 1500 bins on a 64 x 64 grid, annulus out to 0.95: buckets hold more entries than travel in registers (NE per thread), so the
    # first inverse step fetches the rest -- and their jitter phasors -- in place, and the read does the same
    PH.check_phase_batch(emu, orc, HostBufs, 64, 64, 1500, nimg=3, slots=2, sort=True, jitter=0.05, adaptive=True, rmax=0.95,
                         envs=({},), lsb_frac=0.05)


def test_stream_batch_phase_options(emu, orc):
    PH.check_phase_stream(emu, orc, HostBufs, 128, 128, secret=8, nimg=3, slots=2, jitter=0.05, adaptive=True)


def test_phase_options_arguments(emu):
    ctx = B.Context(16, 16, lib=emu)
    jit = np.zeros(5, np.float32)
    assert emu.tfft_set_phase_options(ctx.h, jit.ctypes.data, 0, 0) == -1          # a jitter array of no length
    assert emu.tfft_set_phase_options(None, None, 0, 0) == -1
    ctx.set_phase_options(jit, True)
    ctx.set_phase_options()
    ctx.close()


def test_adaptive_read_needs_no_medians_below_half_pi(orc):
    """read_bit_from_bin (S:734-746) with adaptive alpha: for alpha < pi/2 every a = alpha*clamp(|F|/med, 0.5, 2) lies in (0, pi), the
    targets j +- a are symmetric about j and j + pi, and the bit is the side of that line -- the same as with adaptive off."""
    rng = np.random.default_rng(4)
    n = 4000
    spec = np.zeros((3, 64, 64), np.complex128)
    bins = np.stack([rng.integers(0, 3, n), rng.integers(1, 32, n), rng.integers(1, 32, n)], axis=1).astype(np.int32)
    for alpha in (0.1, 0.5, 1.0, 1.5):
        theta = rng.uniform(-np.pi, np.pi, n)
        jit = rng.uniform(-0.5, 0.5, n)
        mag = np.exp(rng.uniform(-3, 3, n))
        med = np.exp(rng.uniform(-1, 1, 3))
        # one bin per draw: write it, read it alone
        got_on, got_off = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        for i in range(n):
            p, y, x = bins[i]
            spec[p, y, x] = mag[i] * np.exp(1j * theta[i])
            b = bins[i:i + 1]
            got_on[i] = orc.read_bins(spec, b, alpha, jit[i:i + 1], True, med)[0]
            got_off[i] = orc.read_bins(spec, b, alpha, jit[i:i + 1], False, med)[0]
        assert np.array_equal(got_on, got_off), alpha
    # alpha >= pi/2: a = alpha*clamp(..) can pass pi, and then +a lies on the other side of the line: the bit depends on |F|/med
    alpha, med = 2.0, np.ones(3)
    spec[:] = 0
    p, y, x = 0, 3, 5       # |F| = 2 med: adaptive a = 4.0 > pi against the fixed 2.0
    diffs = 0
    for theta in np.linspace(-np.pi, np.pi, 721):
        spec[p, y, x] = 2.0 * np.exp(1j * theta)
        b = np.array([[p, y, x]], np.int32)
        on = orc.read_bins(spec, b, alpha, np.zeros(1), True, med)[0]
        off = orc.read_bins(spec, b, alpha, np.zeros(1), False, med)[0]
        diffs += int(on != off)
    assert diffs > 0, "with alpha >= pi/2 the medians change the bit: the batched extraction refuses adaptive there"
