"""The fitted embed on a real MI355X: the CLI's --fit_crop writes stego of covers whose sides are not powers of two that the REFERENCE CLI
reads (test_gpu_cli.py's test_nonpow2_behaves_like_the_reference shows the one-shot stego it cannot), and 1080p / 4K batches with
distinct keys converge and decode through the library's unmodified reader."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fit_cases as FC
from _checkers import REF_CLI, have_ref
from parity_cases import TorchBufs
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "steganosaurus_amd", "turtlefft")
IT = ["--pbkdf2_iter", "1000"]


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    # torch's HIP runtime first: initialised after the library's in the same process it finds no device
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")


@pytest.fixture(scope="module")
def covers(tmp_path_factory):
    d = tmp_path_factory.mktemp("fitcovers")
    host = C.CDLL(os.path.join(ROOT, "steganosaurus_amd", "libtfhost.so"))
    out = {}
    for name, img in (("np600", cover_rgb(600, 400, 0)), ("vga", cover_rgb(640, 480, 1)), ("hd", cover_rgb(1920, 1080, 2)),
                      ("hdgrad", FC.gradient_rgb(1920, 1080, 3))):
        p = str(d / (name + ".png"))
        assert host.tfh_png_write(p.encode(), img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0]) == 0
        out[name] = p
    out["dir"] = str(d)
    return out


@pytest.mark.skipif(not have_ref(), reason="reference CLI not present")
@pytest.mark.parametrize("cover,extra", [("np600", []), ("vga", ["--jitter", "0.05"]), ("hd", ["--adaptive_alpha", "1", "--center", "1"]),
                                         ("hdgrad", [])])
def test_cli_fit_crop_is_read_by_the_reference(covers, cover, extra):
    a = os.path.join(covers["dir"], cover + "_fit.png")
    secret = "fitted: %s survives the crop" % cover
    r = run(CLI, "embed", "--in", covers[cover], "--out", a, "--secret", secret, "--pass", "pw", "--fit_crop", "1", *IT, *extra)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr            # (no convergence warning)
    r = run(REF_CLI, "extract", "--in", a, "--pass", "pw", *IT, *extra)
    assert (r.returncode, r.stdout) == (0, secret + "\n"), r.stderr
    r = run(CLI, "extract", "--in", a, "--pass", "pw", *IT, *extra)
    assert (r.returncode, r.stdout) == (0, secret + "\n"), r.stderr


@pytest.mark.parametrize("w,h,nimg,slots,jitter,adaptive", [(1920, 1080, 8, 8, 0.05, False), (3840, 2160, 4, 4, 0.0, True)])
def test_batches_converge_and_decode(orc, w, h, nimg, slots, jitter, adaptive):
    lib = B.load()
    # half of the images synthetic photo-like, half smooth gradients
    covers = np.stack([cover_rgb(w, h, 40 + i) if i % 2 == 0 else FC.gradient_rgb(w, h, 40 + i) for i in range(nimg)])
    b = FC.make_batch(orc, w, h, nimg, secret=200, jitter=jitter, seed=3, lib=lib, covers=covers)
    s, u, it, wr = FC.run_fit(lib, TorchBufs, b, slots, adaptive, False, max_iters=16)
    assert (it >= 0).all() and (wr == 0).all(), (it, wr)
    ho, po, so, _ = FC.extract_walks(lib, TorchBufs, b, slots, adaptive, False, s)
    assert list(so) == [b["secret"]] * nimg, so
    assert np.array_equal(ho, b["headers"]) and np.array_equal(po, b["payloads"])
    FC.oracle_bits_ok(orc, b, s, adaptive, False, images=(0, 1))
    ws, wu = FC.run_walks(lib, TorchBufs, b, slots, adaptive, False)
    assert np.array_equal(u, wu)
    _, _, wso, _ = FC.extract_walks(lib, TorchBufs, b, slots, adaptive, False, ws)
    assert (wso == -1).any(), wso


def test_zero_iterations_are_the_walks_embed(orc):
    lib = B.load()
    FC.check_zero_iters(lib, orc, TorchBufs, 1920, 1080, nimg=5, slots=4, jitter=0.05, adaptive=True, center=False,
                        envs=({}, {"TFFT_STREAMS": "2"}, {"TFFT_EMBED_DELTA": "0"}))


def test_fitted_small_batch_and_host_form(orc):
    lib = B.load()
    FC.check_fit(lib, orc, TorchBufs, 600, 400, nimg=3, slots=2, jitter=0.05, adaptive=False, center=False)
