"""CPU-emulated run (tests/emu) of the stego analysis calls (tfft_phase_hist_batch[_dev], tfft_quality_batch[_dev]): annulus phase
histograms against the fp64 oracle spectrum, SSE / SSIM against numpy, chunking, errors and the phase-histogram detector on a one-shot
stego.  Not the product path (see test_emulated.py); tests/test_gpu_analysis.py is the gate on the MI355X."""
import os
import subprocess

import numpy as np
import pytest

import analysis_cases as AC
from parity_cases import HostBufs
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


# 48x40 and 100x30 (non-square, non-power-of-two), 64x64 uncentred and centred (rmax 0.7 crosses x = PW/2 into mirrored stored bins),
# a 256^2 synthetic cover; nbins 8 / 256 / 4096, both radii, no threshold and 0.01 x the oracle median
@pytest.mark.parametrize("w,h,center", [(48, 40, 0), (100, 30, 0), (64, 64, 0), (64, 64, 1), (256, 256, 0)])
def test_histograms_against_the_oracle(emu, orc, w, h, center):
    rgb = cover_rgb(w, h, 3)
    spec, _ = orc.forward_rgb8(rgb, center)
    assert np.abs(spec - AC.np_spectrum(rgb, center)).max() <= 1e-6 * np.abs(spec).max()
    AC.check_hist_image(emu, HostBufs, rgb, center, spec)


def test_histogram_chunks_match_single_calls(emu):
    covers = np.stack([cover_rgb(64, 48, 10 + i) for i in range(3)])
    for nbins in (8, 4096):
        AC.check_hist_chunks(emu, HostBufs, covers, nbins=nbins, slots=2, rmax=0.7)


@pytest.mark.parametrize("w,h", [(11, 11), (12, 40), (65, 130)])
def test_quality(emu, w, h):
    a = np.stack([cover_rgb(w, h, 20 + i) for i in range(3)])
    b = np.stack([AC.perturbed(a[i], i) for i in range(3)])
    b[1] = a[1]                           # one identical pair in the batch: SSE 0, SSIM exactly 1
    sse, ssim = AC.check_quality(emu, HostBufs, a, b, slots=2)
    assert (sse[1] == 0).all() and (ssim[1] == 1.0).all()


def test_errors(emu):
    AC.check_errors(emu)


@pytest.mark.parametrize("slots", [1, 2])
def test_resident_image_survives_a_quality_call(emu, slots):
    AC.check_slots_after_calls(emu, slots=slots)


def test_peak_excess_on_a_one_shot_stego(emu):
    ratio = AC.check_peak_excess(emu, HostBufs, cover_rgb(256, 256, 0), payload_len=100)
    assert (ratio > 0.5).all()
