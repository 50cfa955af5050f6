"""Checks of the fitted embed (tfft_embed_stream_batch_fit[_dev]): stego of covers whose sides are not powers of two that reads back.
Shared by the emulated run (tests/test_emulated_fit.py, HostBufs) and the MI355X run (tests/test_gpu_fit.py, TorchBufs)."""
import numpy as np
import pytest

import walks_cases as WC
from _checkers import Params
from parity_cases import _ctx_with_env, rep_stream
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb


def gradient_rgb(w, h, seed):
    """a smooth cover: two linear ramps and a little noise (most of its spectrum is small away from the axes)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 40 + 150 * (x / max(w - 1, 1)) * 0.6 + 150 * (y / max(h - 1, 1)) * 0.4
    img = np.stack([base + 10 * c for c in range(3)], axis=-1) + rng.normal(0, 2, (h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def make_batch(orc, w, h, nimg, secret=8, jitter=0.05, tag=b"fit", seed=0, margin_bins=300, n_threads=4, lib=None, covers=None):
    """distinct keys, their walks and jitter, covers and frames: what one fitted call takes"""
    plen = secret + 16
    n_bins = 912 + 56 * plen + margin_bins
    ph, pw = orc.next_pow2(h), orc.next_pow2(w)
    pks, keys = WC.image_keys(orc, nimg, tag)
    bins, jit, st = B.walks_build(keys, ph, pw, n_bins, max_jitter=jitter if jitter else None, n_threads=n_threads, lib=lib)
    assert (st == 0).all()
    if covers is None:
        covers = np.stack([cover_rgb(w, h, 700 + seed + i) for i in range(nimg)])
    headers, payloads = WC._frames(nimg, secret, 90 + seed)
    return dict(w=w, h=h, pks=pks, bins=bins, jit=jit if jitter else None, covers=covers, headers=headers, payloads=payloads, secret=secret,
                jitter=jitter)


def run_fit(lib, bufs, b, slots, adaptive, center, max_iters=32, margin=0.5, env=None, host=False, inplace=False):
    """one fitted embed of the batch: (stego, usable_out, iters_out, wrong_out)"""
    nimg = len(b["covers"])
    w, h = b["w"], b["h"]
    bins, jit = b["bins"], b["jit"]
    n_bins = bins.shape[1]
    plen = b["payloads"].shape[1]
    ctx = _ctx_with_env(env or {}, w, h, slots=slots, lib=lib)
    try:
        if host:
            out = np.zeros_like(b["covers"]); us = np.zeros(nimg, np.uint64)
            it = np.full(nimg, -7, np.int32); wr = np.full(nimg, 7, np.uint32)
            ctx.embed_stream_batch_fit_host(b["covers"], bins, b["headers"], b["payloads"], out, jitter=jit, adaptive=adaptive, usable=us,
                                            iters=it, wrong=wr, center=center, max_iters=max_iters, margin=margin)
            return out, us, it, wr
        kb, pb = bufs.put(np.ascontiguousarray(bins).view(np.uint8).reshape(-1, 8))
        jb, pj = bufs.put(jit) if jit is not None else (None, None)
        cb, pc = bufs.put(b["covers"]); hb, phd = bufs.put(b["headers"]); yb, py = bufs.put(b["payloads"])
        ob, po = (cb, pc) if inplace else bufs.put(np.zeros_like(b["covers"]))
        ub, pu = bufs.put(np.zeros(nimg, np.uint64))
        ib, pi = bufs.put(np.full(nimg, -7, np.int32)); wb, pw_ = bufs.put(np.full(nimg, 7, np.uint32))
        ctx.embed_stream_batch_fit_dev(nimg, pc, w, h, pb, pj, n_bins, phd, py, plen, po, adaptive=adaptive, center=center, usable_ptr=pu,
                                       iters_ptr=pi, wrong_ptr=pw_, max_iters=max_iters, margin=margin)
        ctx.sync()
        return bufs.get(ob).copy(), bufs.get(ub).copy(), bufs.get(ib).copy(), bufs.get(wb).copy()
    finally:
        ctx.close()


def run_walks(lib, bufs, b, slots, adaptive, center, env=None):
    """the one-shot walks embed of the same batch: (stego, usable_out)"""
    return WC._run(lib, bufs, env or {}, b["w"], b["h"], slots, b["covers"], b["bins"], b["jit"], adaptive, b["headers"], b["payloads"], center,
                   walks=True)


def extract_walks(lib, bufs, b, slots, adaptive, center, stego):
    """the library's unmodified reader: (headers, payloads, statuses, raw bits)"""
    return WC._run(lib, bufs, {}, b["w"], b["h"], slots, b["covers"], b["bins"], b["jit"], adaptive, b["headers"], b["payloads"], center,
                   walks=True, extract_src=stego)


def oracle_bits_ok(orc, b, stego, adaptive, center, images=None):
    """the fp64 reference reader returns every stream bit of the given images right"""
    P = Params(jitter=b["jitter"], adaptive_alpha=int(adaptive), center=int(center))
    for i in (range(len(stego)) if images is None else images):
        want = rep_stream(b["headers"][i], b["payloads"][i])
        got = orc.extract_bits(stego[i], b["pks"][i], len(want), P)
        assert np.array_equal(got, want), ("fp64 reader", i, int((got != want).sum()))


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def check_fit(lib, orc, bufs, w, h, nimg, slots, jitter, adaptive, center, max_iters=32, mse_ratio=3.0, host=True, seed=0):
    """every image of a fitted batch reads back (fp64 reference reader, the library's walks reader); the one-shot embed of the same batch
    loses at least one; max_iters = 0 is the walks embed; the host form gives the bytes of the device form; the distortion stays bounded"""
    b = make_batch(orc, w, h, nimg, jitter=jitter, seed=seed, lib=lib)
    s, u, it, wr = run_fit(lib, bufs, b, slots, adaptive, center, max_iters=max_iters)
    # every bit reads right; the margin may still be settling on the smallest covers (iters_out -1: some entries below mu/2)
    assert (wr == 0).all() and (it >= -1).all() and (it >= 0).any(), (it, wr)
    oracle_bits_ok(orc, b, s, adaptive, center)
    ho, po, so, _ = extract_walks(lib, bufs, b, slots, adaptive, center, s)
    assert list(so) == [b["secret"]] * nimg, so
    assert np.array_equal(ho, b["headers"]) and np.array_equal(po, b["payloads"])
    ws, wu = run_walks(lib, bufs, b, slots, adaptive, center)
    assert np.array_equal(u, wu), ("usable_out", u, wu)
    _, _, wso, _ = extract_walks(lib, bufs, b, slots, adaptive, center, ws)
    assert (wso == -1).any(), ("the one-shot embed read back everywhere: not a case the fit is needed for", wso)
    m_fit = np.mean([mse(s[i], b["covers"][i]) for i in range(nimg)])
    m_one = np.mean([mse(ws[i], b["covers"][i]) for i in range(nimg)])
    assert m_fit <= mse_ratio * m_one, ("MSE fitted / one-shot", m_fit, m_one)
    if host:
        hs, hu, hit, hwr = run_fit(lib, bufs, b, slots, adaptive, center, max_iters=max_iters, host=True)
        assert np.array_equal(hs, s) and np.array_equal(hu, u) and np.array_equal(hit, it) and np.array_equal(hwr, wr)
    return s, it, m_fit, m_one


def check_zero_iters(lib, orc, bufs, w, h, nimg, slots, jitter, adaptive, center, envs=({},)):
    """max_iters = 0: the bytes and usable_out of the walks embed, under every variant in `envs`; iters_out says who converged, and
    wrong_out counts the stream bits the library's reader gets wrong from those bytes"""
    b = make_batch(orc, w, h, nimg, jitter=jitter, seed=11, lib=lib)
    for env in envs:
        s, u, it, wr = run_fit(lib, bufs, b, slots, adaptive, center, max_iters=0, env=env)
        ws, wu = run_walks(lib, bufs, b, slots, adaptive, center, env=env)
        assert np.array_equal(s, ws), ("stego", env, int((s != ws).sum()))
        assert np.array_equal(u, wu), ("usable_out", env)
        assert set(it.tolist()) <= {0, -1}, it
        _, _, _, raw = extract_walks(lib, bufs, b, slots, adaptive, center, ws)
        for i in range(nimg):
            want = rep_stream(b["headers"][i], b["payloads"][i])
            assert int(wr[i]) == int((raw[i, :len(want)] != want).sum()), ("wrong_out", env, i)
            if it[i] == 0:
                assert wr[i] == 0
    # in place: the covers are copied before the first write
    ws, _ = run_walks(lib, bufs, b, slots, adaptive, center)
    s2, _, _, _ = run_fit(lib, bufs, b, slots, adaptive, center, max_iters=0, inplace=True)
    s3, _, _, _ = run_fit(lib, bufs, b, slots, adaptive, center, max_iters=4, inplace=True)
    s4, _, _, _ = run_fit(lib, bufs, b, slots, adaptive, center, max_iters=4)
    assert np.array_equal(s2, ws) and np.array_equal(s3, s4)


def check_fit_errors(lib, orc, bufs, w=100, h=120):
    """alpha outside (0, pi/2), negative max_iters, margin <= 0 -> TFFT_E_INVALID; a bit index set -> TFFT_E_STATE; a bin on an excluded
    axis in one image's list -> TFFT_E_BIN_RANGE (device and host forms), and the flag does not stick"""
    b = make_batch(orc, w, h, 2, secret=0, jitter=0.05, tag=b"fit-errors", margin_bins=50, lib=lib)
    nimg, n_bins, plen = 2, b["bins"].shape[1], b["payloads"].shape[1]
    kb, pb = bufs.put(b["bins"].view(np.uint8).reshape(-1, 8)); cb, pc = bufs.put(b["covers"])
    hb, phd = bufs.put(b["headers"]); yb, py = bufs.put(b["payloads"]); ob, po = bufs.put(np.zeros_like(b["covers"]))
    ctx = B.Context(w, h, slots=2, lib=lib)
    try:
        for kw in ({"alpha": np.pi / 2}, {"alpha": 1.6}, {"alpha": 0.0}, {"alpha": -0.5}, {"max_iters": -1}, {"margin": 0.0}):
            with pytest.raises(B.TfftError) as ei:
                ctx.embed_stream_batch_fit_dev(nimg, pc, w, h, pb, None, n_bins, phd, py, plen, po, **kw)
            assert ei.value.status == -1, kw
            with pytest.raises(B.TfftError) as ei:
                ctx.embed_stream_batch_fit_host(b["covers"], b["bins"], b["headers"], b["payloads"], np.zeros_like(b["covers"]), **kw)
            assert ei.value.status == -1, kw
        ctx.set_bit_index(np.arange(n_bins, dtype=np.uint32))
        with pytest.raises(B.TfftError) as ei:
            ctx.embed_stream_batch_fit_dev(nimg, pc, w, h, pb, None, n_bins, phd, py, plen, po)
        assert ei.value.status == -6
        ctx.set_bit_index(None)
        bad = b["bins"].copy()
        bad[1, 17]["y"] = 0
        kb2, pb2 = bufs.put(bad.view(np.uint8).reshape(-1, 8))
        with pytest.raises(B.TfftError) as ei:
            ctx.embed_stream_batch_fit_dev(nimg, pc, w, h, pb2, None, n_bins, phd, py, plen, po)
        assert ei.value.status == -8
        with pytest.raises(B.TfftError) as ei:
            ctx.embed_stream_batch_fit_host(b["covers"], bad, b["headers"], b["payloads"], np.zeros_like(b["covers"]))
        assert ei.value.status == -8
        ctx.embed_stream_batch_fit_dev(nimg, pc, w, h, pb, None, n_bins, phd, py, plen, po, max_iters=1)
        ctx.sync()
    finally:
        ctx.close()
