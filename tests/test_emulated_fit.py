"""CPU-emulated run (tests/emu) of the fitted embed (tfft_embed_stream_batch_fit[_dev]) on covers whose sides are not powers of two:
every stream bit of every fitted stego reads right in the fp64 reference reader and the library's walks reader, where the one-shot
walks embed loses images.  Not the product path (see test_emulated.py); tests/test_gpu_fit.py is the gate on the MI355X."""
import os
import subprocess

import pytest

import fit_cases as FC
from parity_cases import HostBufs
from steganosaurus_amd import binding as B
from walks_cases import WALK_ENVS

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


# 100 x 300 pads to 128 x 512 (two-step columns); 120 x 200 and 65 x 130 have odd row byte counts (the delta row kernel's unaligned
# cover reads); three images in two slots: two chunks.  The MSE bound is 3x the one-shot embed's, 3.5x on 65 x 130: a quarter of the
# padded grid survives the crop there and the fit measured 3.06x with adaptive alpha
@pytest.mark.parametrize("w,h,nimg,jitter,adaptive,center,mse_ratio", [
    (100, 300, 2, 0.05, True, False, 3.0),
    (100, 300, 3, 0.0, False, True, 3.0),
    (120, 200, 3, 0.05, False, False, 3.0),
    (120, 200, 2, 0.0, True, True, 3.0),
    (65, 130, 3, 0.0, False, False, 3.5),
    (65, 130, 2, 0.05, True, True, 3.5),
])
def test_fitted_stego_reads_back(emu, orc, w, h, nimg, jitter, adaptive, center, mse_ratio):
    FC.check_fit(emu, orc, HostBufs, w, h, nimg, slots=2, jitter=jitter, adaptive=adaptive, center=center, mse_ratio=mse_ratio)


def test_zero_iterations_are_the_walks_embed(emu, orc):
    FC.check_zero_iters(emu, orc, HostBufs, 120, 200, nimg=3, slots=2, jitter=0.05, adaptive=True, center=False, envs=WALK_ENVS)


def test_zero_iterations_two_step_columns(emu, orc):
    FC.check_zero_iters(emu, orc, HostBufs, 100, 300, nimg=2, slots=2, jitter=0.0, adaptive=False, center=True,
                        envs=({}, {"TFFT_STATS_TILE": "2"}, {"TFFT_EMBED_DELTA": "0"}))


def test_fitted_under_the_spectrum_embed(emu, orc):
    # TFFT_EMBED_DELTA=0 writes F' into the spectrum: the fit builds its buckets and F0 itself and ends in the same place
    b = FC.make_batch(orc, 120, 200, 2, jitter=0.05, seed=5, lib=emu)
    s, _, it, wr = FC.run_fit(emu, HostBufs, b, 2, False, False, env={"TFFT_EMBED_DELTA": "0"})
    assert (it >= 0).all() and (wr == 0).all(), (it, wr)
    FC.oracle_bits_ok(orc, b, s, False, False)


def test_errors(emu, orc):
    FC.check_fit_errors(emu, orc, HostBufs)
