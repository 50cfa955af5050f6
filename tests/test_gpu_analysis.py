"""Stego analysis on the MI355X (tfft_phase_hist_batch[_dev], tfft_quality_batch[_dev], `turtlefft embed --report 1`): the checks of
tests/analysis_cases.py on 1080p, 4K, the fused 4096-column plan, 640x360 and 2048^2 batches (fp64 oracle spectrum: np.fft with the
reference's sign convention), the quality figures at 1080p and 4K, the +-alpha excess of a one-shot stego and the CLI report line."""
import os
import re
import subprocess

import numpy as np
import pytest

import analysis_cases as AC
from parity_cases import TorchBufs
from steganosaurus_amd import analysis as A
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb, gradient_cover

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "steganosaurus_amd", "turtlefft")


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    # torch's HIP runtime first: initialised after the library's in the same process it finds no device
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")


@pytest.fixture(scope="module")
def lib():
    return B.load()


def covers_of(w, h, n, seed=0):
    return np.stack([cover_rgb(w, h, seed + i) if i % 2 == 0 else gradient_cover(w, h, seed + i) for i in range(n)])


# (w, h, n, slots, center, fused plan expected); 256^2 at rmax 0.7 reaches x > PW/2, the mirrored stored bins
BATCHES = [(1920, 1080, 4, 3, 0, True), (3840, 2160, 2, 2, 1, True), (4096, 2048, 2, 2, 0, True), (640, 360, 1, 1, 0, False),
           (2048, 2048, 1, 1, 0, True), (256, 256, 2, 2, 1, False)]


def test_batches_cover_fused_and_unfused_plans(lib):
    ctx = B.Context(4096, 2160, lib=lib)
    try:
        fused = [ctx.plan_info(w, h, min(n, slots))["fused"] for (w, h, n, slots, _, _) in BATCHES]
    finally:
        ctx.close()
    assert fused == [b[5] for b in BATCHES]
    assert any(fused) and not all(fused)


@pytest.mark.parametrize("w,h,n,slots,center,fused", BATCHES)
def test_histograms_against_the_oracle(lib, w, h, n, slots, center, fused):
    covers = covers_of(w, h, n)
    ctx = B.Context(w, h, slots=slots, lib=lib)
    try:
        radii = AC.RADII if w * h <= 640 * 360 else AC.RADII[:1]
        if w == h == 256:
            assert (AC.annulus(256, 256, *AC.RADII[1])[1] > 128).any()      # the mirrored branch is exercised
        for nbins in (256, 4096):
            for (rmin, rmax) in radii:
                got = AC.hist_dev(lib, TorchBufs, ctx, covers, nbins, center, rmin, rmax)
                host = ctx.phase_hist_batch_host(covers, nbins=nbins, center=center, rmin=rmin, rmax=rmax)
                assert np.array_equal(got, host)
                for i in range(n):
                    spec = AC.np_spectrum(covers[i], center)
                    AC.check_hist(got[i], spec, rmin, rmax, nbins, None, (w, h, i, nbins, rmin, rmax))
                    if nbins == 256 and (rmin, rmax) == AC.RADII[0]:
                        thr = 0.01 * np.array([AC.median_abs(spec[p]) for p in range(3)])
                        one = ctx.phase_hist_batch_host(covers[i:i + 1], nbins=nbins, center=center, rmin=rmin, rmax=rmax, thr=thr)
                        AC.check_hist(one[0], spec, rmin, rmax, nbins, thr, (w, h, i, "thr"))
                    del spec
    finally:
        ctx.close()


def test_resident_image_survives_a_quality_call(lib):
    AC.check_slots_after_calls(lib, 512, 512, slots=2)


def test_chunks_match_single_calls_1080p(lib):
    AC.check_hist_chunks(lib, TorchBufs, covers_of(1920, 1080, 4, 7), nbins=256, slots=3)


@pytest.mark.parametrize("w,h,n", [(1920, 1080, 4), (3840, 2160, 2)])
def test_quality(lib, w, h, n):
    a = covers_of(w, h, n, 3)
    b = np.stack([AC.perturbed(a[i], i, amp=1 + i) for i in range(n)])
    b[-1] = a[-1]
    sse, ssim = AC.check_quality(lib, TorchBufs, a, b, slots=2)
    assert (sse[-1] == 0).all() and (ssim[-1] == 1.0).all()
    assert (A.psnr_db(sse[:-1], w, h) > 40).all()


def test_peak_excess_2048(lib):
    ratio = AC.check_peak_excess(lib, TorchBufs, cover_rgb(2048, 2048, 0), payload_len=4096)
    assert (ratio > 0.5).all()


def test_cli_report(tmp_path):
    import ctypes as C
    host = C.CDLL(os.path.join(ROOT, "steganosaurus_amd", "libtfhost.so"))
    cover = cover_rgb(512, 512, 0)
    cp, sp = str(tmp_path / "cover.png"), str(tmp_path / "stego.png")
    assert host.tfh_png_write(cp.encode(), cover.ctypes.data_as(C.c_void_p), 512, 512) == 0
    secret = "report: the quick brown fox"
    args = ["embed", "--in", cp, "--out", sp, "--secret", secret, "--pass", "pw", "--pbkdf2_iter", "1000"]
    r = subprocess.run([CLI, *args, "--report", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Embedded %d bits into %s (payload %d bytes, ver=2, salt/nonce in header)\n" % (912 + 56 * (len(secret) + 16), sp, len(secret))
    lines = r.stderr.splitlines()
    assert len(lines) == 1 and lines[0].startswith("Report: "), r.stderr
    stego = AC.png_read_rgb8(sp)
    m = re.search(r"PSNR\(dB\) R=(\S+) G=(\S+) B=(\S+); SSIM R=(\S+) G=(\S+) B=(\S+); KL\(stego\|\|cover\) R=(\S+) G=(\S+) B=(\S+)$", lines[0])
    assert m, lines[0]
    vals = [float(v) for v in m.groups()]
    d = cover.astype(np.int64) - stego.astype(np.int64)
    sse = (d * d).sum(axis=(0, 1))
    assert np.allclose(vals[:3], A.psnr_db(sse, 512, 512), rtol=0, atol=2e-6)
    for p in range(3):
        assert abs(vals[3 + p] - AC.ssim_ref(cover[:, :, p], stego[:, :, p])) <= 1e-4
    ctx = B.Context(512, 512, slots=2, lib=B.load())
    try:
        hist = ctx.phase_hist_batch_host(np.stack([cover, stego]), nbins=256)
    finally:
        ctx.close()
    assert np.allclose(vals[6:], A.kl_divergence(hist[1], hist[0]), rtol=0, atol=2e-8)
    # stdout and the stego do not depend on the flag (the salt is random: compare the form, and the stego still extracts)
    r = subprocess.run([CLI, "extract", "--in", sp, "--pass", "pw", "--pbkdf2_iter", "1000"], capture_output=True, text=True)
    assert (r.returncode, r.stdout) == (0, secret + "\n"), r.stderr
