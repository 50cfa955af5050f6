"""Exact capacities of the batched embeds on a real MI355X (tfft_set_batch_exact): in ALL mode every image's
usable_out equals a second context's single-image tfft_capacity(magmin * tfft_medians) -- the reference's integer -- through every batched
embed form, the stego bytes are those of mode OFF, and NEAR mode takes the reference's "Message too large" decisions."""
import ctypes as C
import os

import numpy as np
import pytest

import exact_batch_cases as XC
from parity_cases import TorchBufs
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb, gradient_cover

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}       # largest |fp32 - exact| per geometry (printed at the end, bounded by guard / 8)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")
    yield
    if WORST:
        print("\nlargest |fp32 - exact| capacity per geometry:", WORST)


def _all_vs_single(covers, center, cases, slots, orc=None, orc_images=()):
    n, h, w = covers.shape[:3]

    def want(rmin, rmax, magmin):
        caps = XC.single_capacities(None, covers, center, rmin, rmax, magmin)
        for i in orc_images:      # (not with magmin = 1: the median bins tie with the threshold, see exact_batch_cases.oracle_want)
            if orc is not None and magmin != 1.0:
                cap, _ = orc.capacity_rgb8(covers[i], XC.Params(rmin=rmin, rmax=rmax, magmin=magmin, center=center))
                assert cap == caps[i], (i, cap, caps[i])
        return caps
    worst = XC.check_all_dev(None, TorchBufs, want, covers, center, slots=slots, cases=cases, inplace=False)
    WORST[(w, h, center, n)] = max(worst, WORST.get((w, h, center, n), 0))
    assert worst <= XC.GUARD // 8, worst


def test_1080p_32_images(orc):
    covers = np.stack([cover_rgb(1920, 1080, i) if i % 2 else gradient_cover(1920, 1080, i) for i in range(32)])
    _all_vs_single(covers, 0, ((0.05, 0.45, 0.01), (0.1, 0.6, 1.0)), slots=16, orc=orc, orc_images=(0, 31))


def test_4k_centred_threshold_at_median(orc):
    covers = np.stack([cover_rgb(3840, 2160, 10 + i) if i % 2 else gradient_cover(3840, 2160, 10 + i) for i in range(8)])
    _all_vs_single(covers, 1, ((0.05, 0.45, 0.01), (0.05, 0.45, 1.0)), slots=8, orc=orc, orc_images=(0,))


@pytest.mark.parametrize("w,h,n", [(2048, 2048, 2), (640, 360, 5)])
def test_other_geometries(w, h, n):
    covers = np.stack([cover_rgb(w, h, 20 + i) for i in range(n)])
    _all_vs_single(covers, 0, XC.CASES, slots=2)


def test_512_golden_pair(golden_dir):
    covers = np.stack([cover_rgb(512, 512, 0), gradient_cover(512, 512, 1)])
    want = np.array([int(np.load(os.path.join(golden_dir, f"fft_512_{k}.npz"))["capacity"]) for k in ("lcg", "grad")], np.int64)
    XC.check_all_dev(None, TorchBufs, lambda *a: want, covers, 0, slots=2, cases=((0.05, 0.45, 0.01),))


def test_host_stream_walks_fit(orc):
    XC.check_host_stream(None, orc, 640, 360, 0, nimg=5, slots=4, cases=((0.05, 0.45, 0.01), (0.1, 0.6, 1.0)))
    XC.check_walks_and_fit(None, orc, TorchBufs, 600, 400, nimg=3, slots=2)


def test_png_batch(tmp_path):
    host = C.CDLL(os.path.join(ROOT, "steganosaurus_amd", "libtfhost.so"))
    w, h, n, plen = 640, 360, 5, 4
    covers = np.stack([cover_rgb(w, h, 50 + i) for i in range(n)])
    ins, outs = [], []
    for i in range(n):
        p = str(tmp_path / ("c%d.png" % i))
        assert host.tfh_png_write(p.encode(), covers[i].ctypes.data_as(C.c_void_p), w, h) == 0
        ins.append(p); outs.append(str(tmp_path / ("s%d.png" % i)))
    bins = B.Walk(bytes(range(32)), 512, 1024, 0.05, 0.45, 0.7).next(912 + 56 * plen)
    headers = np.random.default_rng(1).integers(0, 256, (n, 38)).astype(np.uint8)
    payloads = np.random.default_rng(2).integers(0, 256, (n, plen)).astype(np.uint8)
    caps = XC.single_capacities(None, covers, 0, 0.05, 0.45, 0.01)
    res = {}
    for mode in (XC.OFF, XC.ALL):
        ctx = XC.make_ctx(None, w, h, 4, mode)
        try:
            outs_m = [o + str(mode) for o in outs]
            usable, _ = B.embed_png_batch(ctx, ins, outs_m, w, h, bins, headers, payloads, chunk=n, threads=2, png_level=1)
            res[mode] = (np.asarray(usable, np.int64), [open(o, "rb").read() for o in outs_m], ctx.batch_exact_info(n))
        finally:
            ctx.close()
    assert np.array_equal(res[XC.ALL][0], caps) and (res[XC.ALL][2] == 1).all(), (res[XC.ALL][0], caps, res[XC.ALL][2])
    assert res[XC.ALL][1] == res[XC.OFF][1]


def test_near_decisions_match_the_reference(orc):
    """n_bits in {cap-1, cap, cap+1}: "Message too large" (n_bits > usable, S:1009-1012) exactly where the reference raises it"""
    w, h = 640, 360
    covers = np.stack([cover_rgb(w, h, 60 + i) for i in range(4)])
    cap = orc.capacity_rgb8(covers[0])[0]
    walk = B.Walk(bytes(range(32)), 512, 1024, 0.05, 0.45, 0.7).next(cap + 1)
    for n in (cap - 1, cap, cap + 1):
        _, u, st = XC.embed_dev(None, TorchBufs, covers, walk[:n], np.ones((4, n), np.uint8), 2, XC.NEAR)
        assert st[0] == 1 and u[0] == cap, (n, st, u, cap)
        assert (n > u[0]) == (n > cap)
    XC.check_near(None, TorchBufs, orc, w, h)


def test_off_one_pixel_wide_and_errors():
    XC.check_off_and_errors(None, TorchBufs, 640, 360)
