"""SPAM co-occurrence counts on the MI355X (tfft_spam_batch[_dev], `turtlefft spam`): the checks of
tests/spam_cases.py -- counts == the numpy restatement of the definition, exactly -- on 640x360, 1919x1081, 1080p, 256^2 batches and a flat
2048^2 image (every triple in one counter), repeated calls, and the CLI's feature lines."""
import os
import subprocess

import numpy as np
import pytest

import spam_cases as SC
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


# (w, h, n, slots): 1919x1081 images start at odd bytes and end in a half-empty tile; 1080p x 3 in 2 slots is two chunks of the host form
@pytest.mark.parametrize("w,h,n,slots", [(640, 360, 1, 1), (1919, 1081, 2, 2), (1920, 1080, 3, 2), (256, 256, 2, 2)])
def test_counts_equal_the_definition(lib, w, h, n, slots):
    imgs = covers_of(w, h, n, seed=w % 7)
    got = SC.check_images(lib, TorchBufs, imgs, t=3, slots=slots, tag=(w, h, n, slots), repeat=True)
    one = B.Context(w, h, slots=1, lib=lib)
    try:
        single = one.spam_batch_host(imgs[n - 1:n])
    finally:
        one.close()
    assert single[0].tobytes() == got[n - 1].tobytes()      # the last image alone, one slot: the same bytes


def test_flat_2048_is_exact_under_maximal_contention(lib):
    imgs = SC.flat(2048, 2048)[None]
    ctx = B.Context(2048, 2048, slots=1, lib=lib)
    try:
        host = ctx.spam_batch_host(imgs)
        dev = SC.spam_dev(TorchBufs, ctx, imgs)
    finally:
        ctx.close()
    assert host.tobytes() == dev.tobytes()
    centre = (3 * 7 + 3) * 7 + 3
    want = np.zeros((1, 3, 4, 343), np.int64)
    want[0, :, :, centre] = SC.dir_totals(2048, 2048)
    assert np.array_equal(host.astype(np.int64), want)


@pytest.mark.parametrize("t", [1, 2, 4])
def test_other_truncations(lib, t):
    SC.check_images(lib, TorchBufs, covers_of(301, 67, 2, seed=t), t=t, slots=1, tag=("t", t))


def test_patterns_and_tile_edges(lib):
    SC.check_shape(lib, TorchBufs, 259, 29)
    SC.check_shape(lib, TorchBufs, 4, 4)
    SC.check_shape(lib, TorchBufs, 3, 9)


def test_resident_image_survives_the_call(lib):
    SC.check_slots_after_spam(lib, TorchBufs, 512, 512, slots=2)


def test_cli_spam(tmp_path, lib):
    import ctypes as C
    host = C.CDLL(os.path.join(ROOT, "steganosaurus_amd", "libtfhost.so"))
    img = cover_rgb(512, 512, 0)
    path = str(tmp_path / "image.png")
    assert host.tfh_png_write(path.encode(), img.ctypes.data_as(C.c_void_p), 512, 512) == 0
    r = subprocess.run([CLI, "spam", "--in", path], capture_output=True, text=True)
    assert (r.returncode, r.stderr) == (0, ""), r.stderr
    lines = r.stdout.splitlines()
    assert [ln.split(" ", 1)[0] for ln in lines] == ["R", "G", "B"]
    ctx = B.Context(512, 512, slots=1, lib=lib)
    try:
        want = A.spam_features(ctx.spam_batch_host(img[None]))[0]
    finally:
        ctx.close()
    assert want.shape == (3, 686)
    for p in range(3):
        fields = lines[p].split(" ")[1:]
        assert len(fields) == 686
        got = np.array([float(v) for v in fields])
        # %.9e rounds to 5e-10 relative
        assert (np.abs(got - want[p]) <= 1e-9 * np.maximum(np.abs(want[p]), 1e-300)).all(), p
