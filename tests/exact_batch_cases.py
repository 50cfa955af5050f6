"""Exact capacities of the batched embeds (tfft_set_batch_exact), written once and run twice: on the CPU-emulated
build of the kernel sources (tests/test_emulated_exact_batch.py) and on the MI355X (tests/test_gpu_exact_batch.py, -m gpu).

What every check holds: with the mode on, usable_out is the reference's integer (the oracle's capacity_rgb8, or a single-image
tfft_capacity(magmin * tfft_medians) of a second context), the per-image states say so, and the stego bytes are those of mode OFF."""
import os

import numpy as np

import fit_cases as FC
from _checkers import Params
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

OFF, ALL, NEAR = 0, 1, 2
GUARD = 64
CASES = ((0.05, 0.45, 0.01), (0.0, 1.5, 0.3), (0.1, 0.6, 1.0), (0.05, 0.45, 0.0))


def p2(v):
    return 1 << (int(v) - 1).bit_length()


def make_ctx(lib, w, h, slots, mode=None, guard=GUARD):
    ctx = B.Context(w, h, slots=slots, lib=lib)
    if mode is not None:
        ctx.set_batch_exact(mode, guard)
    return ctx


def shared_bins(lib, w, h, n=16):
    return B.Walk(bytes(range(32)), p2(h), p2(w), 0.05, 0.45, 0.7, lib=lib).next(n)


def embed_dev(lib, bufs, covers, bins, bits, slots, mode, center=False, rmin=0.05, rmax=0.45, magmin=0.01, inplace=False, guard=GUARD):
    """one tfft_embed_batch_dev: (stego, usable_out, states); mode None: a context that never called the setter"""
    n, h, w = covers.shape[:3]
    ctx = make_ctx(lib, w, h, slots, mode, guard)
    try:
        ki, kp = bufs.put(np.ascontiguousarray(bins).view(np.uint8).reshape(-1, 8))
        bi, bp = bufs.put(bits)
        ii, ip = bufs.put(covers)
        oi, op = (ii, ip) if inplace else bufs.put(np.zeros_like(covers))
        ui, up = bufs.put(np.full(n, -1, np.int64))
        ctx.embed_batch_dev(n, ip, w, h, kp, bp, bits.shape[1], op, center=center, rmin=rmin, rmax=rmax, magmin=magmin, usable_ptr=up)
        ctx.sync()
        return bufs.get(oi).copy(), bufs.get(ui).astype(np.int64), ctx.batch_exact_info(n)
    finally:
        ctx.close()


def single_capacities(lib, covers, center, rmin, rmax, magmin):
    """tfft_capacity(magmin * tfft_medians) of each image alone: the exact single-image path"""
    n, h, w = covers.shape[:3]
    one = B.Context(w, h, lib=lib)
    try:
        caps = []
        for i in range(n):
            one.forward_rgb8(covers[i], center)
            caps.append(one.capacity(magmin * one.medians(), rmin, rmax))
        return np.array(caps, np.int64)
    finally:
        one.close()


def check_all_dev(lib, bufs, want_fn, covers, center, slots=2, cases=CASES, inplace=True):
    """ALL mode through tfft_embed_batch_dev: usable == want_fn(rmin, rmax, magmin) for every image, states 1, bytes of mode OFF (and the
    same again when the stego is written over the covers).  Returns the largest |fp32 - exact| seen."""
    n, h, w = covers.shape[:3]
    bins = shared_bins(lib, w, h)
    bits = (np.arange(n * len(bins)).reshape(n, -1) % 3 == 0).astype(np.uint8)
    worst = 0
    for (rmin, rmax, magmin) in cases:
        kw = dict(center=center, rmin=rmin, rmax=rmax, magmin=magmin)
        s_off, u_off, st_off = embed_dev(lib, bufs, covers, bins, bits, slots, OFF, **kw)
        s_all, u_all, st_all = embed_dev(lib, bufs, covers, bins, bits, slots, ALL, **kw)
        want = want_fn(rmin, rmax, magmin)
        assert (st_off == 0).all(), st_off
        assert (st_all == 1).all(), ((w, h, center, rmin, rmax, magmin), st_all)
        assert np.array_equal(u_all, want), ((w, h, center, rmin, rmax, magmin), u_all, want, u_off)
        assert np.array_equal(s_all, s_off), "stego bytes differ from mode OFF"
        worst = max(worst, int(np.abs(u_off - want).max()))
        if inplace:
            s_in, u_in, st_in = embed_dev(lib, bufs, covers, bins, bits, slots, ALL, inplace=True, **kw)
            assert np.array_equal(u_in, want) and (st_in == 1).all() and np.array_equal(s_in, s_off), "in-place embed"
    return worst


def oracle_want(orc, covers, center, lib=None):
    """the reference's integers.  With magmin = 1 the threshold IS the median: the median bin and its mirror tie with it, and whether the
    reference counts the mirror depends on the last ulp its own FFT gives the mirror (no other fp64 evaluation reproduces that; covers
    with symmetric spectra tie several bins).  There the answer is the single-image exact call's."""
    def want(rmin, rmax, magmin):
        ref = np.array([orc.capacity_rgb8(c, Params(rmin=rmin, rmax=rmax, magmin=magmin, center=center))[0] for c in covers], np.int64)
        if magmin != 1.0:
            return ref
        return single_capacities(lib, covers, center, rmin, rmax, magmin)
    return want


def golden_covers(golden_dir, w, h, center, nimg):
    """image 0 is the golden vector's cover (its reference-made `capacity` at default parameters), the others synthetic"""
    g = np.load(os.path.join(golden_dir, f"fft_{w}x{h}_c{center}.npz"))
    covers = np.stack([cover_rgb(w, h, int(g["cover_index"]))] + [cover_rgb(w, h, 80 + i) for i in range(nimg - 1)])
    return covers, int(g["capacity"])


def check_geometry(lib, orc, bufs, golden_dir, w, h, center, nimg=3, slots=2):
    covers, gcap = golden_covers(golden_dir, w, h, center, nimg)
    want = oracle_want(orc, covers, center, lib)
    assert want(0.05, 0.45, 0.01)[0] == gcap
    return check_all_dev(lib, bufs, want, covers, center, slots=slots)


def check_host_stream(lib, orc, w, h, center, nimg=3, slots=2, cases=CASES):
    """the host stream form (three-stream ring): exact usable, states 1, bytes of mode OFF"""
    covers = np.stack([cover_rgb(w, h, 90 + i) for i in range(nimg)])
    ph, pw = p2(h), p2(w)
    plen = 2
    n_bins = 912 + 56 * plen
    bins = B.Walk(bytes(range(32)), ph, pw, 0.0, 1.5, 0.9, lib=lib).next(n_bins)
    hdr = np.random.default_rng(3).integers(0, 256, (nimg, 38)).astype(np.uint8)
    pay = np.random.default_rng(4).integers(0, 256, (nimg, plen)).astype(np.uint8)
    want = oracle_want(orc, covers, center, lib)
    for (rmin, rmax, magmin) in cases:
        res = {}
        for mode in (OFF, ALL):
            ctx = make_ctx(lib, w, h, slots, mode)
            try:
                out = np.zeros_like(covers)
                us = np.zeros(nimg, np.uint64)
                ctx.embed_stream_batch_host(covers, bins, hdr, pay, out, usable=us, center=center, rmin=rmin, rmax=rmax, magmin=magmin)
                res[mode] = (out, us.astype(np.int64), ctx.batch_exact_info(nimg))
            finally:
                ctx.close()
        assert (res[ALL][2] == 1).all() and (res[OFF][2] == 0).all(), (res[ALL][2], res[OFF][2])
        assert np.array_equal(res[ALL][1], want(rmin, rmax, magmin)), (rmin, rmax, magmin, res[ALL][1], want(rmin, rmax, magmin))
        assert np.array_equal(res[ALL][0], res[OFF][0])


def check_near(lib, bufs, orc, w, h, center=False, nimg=2, slots=2):
    """NEAR: n_bits in {cap-1, cap, cap+1} of image 0 settles it (state 1, exact); n_bits far below leaves the fp32 count (state 0)"""
    covers = np.stack([cover_rgb(w, h, 60 + i) for i in range(nimg)])
    want = oracle_want(orc, covers, center)(0.05, 0.45, 0.01)
    ph, pw = p2(h), p2(w)
    cap = int(want[0])
    walk = B.Walk(bytes(range(32)), ph, pw, 0.05, 0.45, 0.7, lib=lib).next(cap + 1)
    s_off, u_off, _ = embed_dev(lib, bufs, covers, walk[:8], np.ones((nimg, 8), np.uint8), slots, OFF, center=center)
    for n in (cap - 1, cap, cap + 1):
        bits = np.ones((nimg, n), np.uint8)
        _, u, st = embed_dev(lib, bufs, covers, walk[:n], bits, slots, NEAR, center=center)
        assert st[0] == 1 and u[0] == cap, (n, st, u, cap)
        for i in range(nimg):
            assert (st[i] == 1 and u[i] == want[i]) or (st[i] == 0 and abs(int(u_off[i]) - n) > GUARD and u[i] == u_off[i]), (i, st, u)
    s, u, st = embed_dev(lib, bufs, covers, walk[:8], np.ones((nimg, 8), np.uint8), slots, NEAR, center=center, guard=4)
    assert (st == 0).all() and np.array_equal(u, u_off) and np.array_equal(s, s_off), (st, u, u_off)


def check_off_and_errors(lib, bufs, w, h):
    """OFF: states 0 and usable of a context that never called the setter; 1-pixel-wide covers: state -1 with the fp32 count; bad
    arguments: TFFT_E_INVALID"""
    covers = np.stack([cover_rgb(w, h, 40 + i) for i in range(3)])
    bins = shared_bins(lib, w, h)
    bits = np.ones((3, len(bins)), np.uint8)
    s0, u0, _ = embed_dev(lib, bufs, covers, bins, bits, 2, None)
    s1, u1, st1 = embed_dev(lib, bufs, covers, bins, bits, 2, OFF)
    assert np.array_equal(u0, u1) and np.array_equal(s0, s1) and (st1 == 0).all()
    thin = np.stack([cover_rgb(1, 64, 5 + i) for i in range(2)])
    tb = np.zeros(0, B.BIN_DTYPE)                         # (no bins: only the statistics matter here)
    s_off, u_off, _ = embed_dev(lib, bufs, thin, tb, np.zeros((2, 0), np.uint8), 2, OFF, rmax=1.5, rmin=0.0)
    s_all, u_all, st = embed_dev(lib, bufs, thin, tb, np.zeros((2, 0), np.uint8), 2, ALL, rmax=1.5, rmin=0.0)
    assert (st == -1).all() and np.array_equal(u_all, u_off) and np.array_equal(s_all, s_off), (st, u_all, u_off)
    ctx = B.Context(w, h, slots=2, lib=lib)
    try:
        for bad in (-1, 3):
            assert ctx.lib.tfft_set_batch_exact(ctx.h, bad, 64) == -1
        assert ctx.lib.tfft_batch_exact_info(ctx.h, 1, B._ptr(np.zeros(1, np.int32))) == -1      # no call yet
        ctx.set_batch_exact(ALL)
        ki, kp = bufs.put(np.ascontiguousarray(bins).view(np.uint8).reshape(-1, 8)); bi, bp = bufs.put(bits)
        ii, ip = bufs.put(covers); oi, op = bufs.put(np.zeros_like(covers)); ui, up = bufs.put(np.zeros(3, np.int64))
        ctx.embed_batch_dev(3, ip, w, h, kp, bp, len(bins), op, usable_ptr=up)
        ctx.sync()
        assert (ctx.batch_exact_info(3) == 1).all()
        assert ctx.lib.tfft_batch_exact_info(ctx.h, 4, B._ptr(np.zeros(4, np.int32))) == -1
    finally:
        ctx.close()


def check_walks_and_fit(lib, orc, bufs, w, h, nimg=3, slots=2, center=False):
    """the walks and fitted embeds: exact usable (the cover's capacity), states 1, bytes of mode OFF (fit with 0 and > 0 iterations)"""
    b = FC.make_batch(orc, w, h, nimg, jitter=0.05, seed=11, lib=lib)
    want = oracle_want(orc, b["covers"], center)(0.05, 0.45, 0.01)
    res = {}
    for mode in (OFF, ALL):
        res[("walks", mode)] = _walks_dev(lib, bufs, b, slots, center, mode)
        for iters in (0, 4):
            res[("fit", iters, mode)] = _fit_dev(lib, bufs, b, slots, center, mode, iters)
    for key in [("walks",)] + [("fit", i) for i in (0, 4)]:
        s_off, u_off, st_off = res[key + (OFF,)]
        s_all, u_all, st_all = res[key + (ALL,)]
        assert (st_off == 0).all() and (st_all == 1).all(), (key, st_off, st_all)
        assert np.array_equal(u_all, want), (key, u_all, want)
        assert np.array_equal(s_all, s_off), key


def _walks_dev(lib, bufs, b, slots, center, mode):
    nimg = len(b["covers"])
    w, h = b["w"], b["h"]
    ctx = make_ctx(lib, w, h, slots, mode)
    try:
        kb, pb = bufs.put(np.ascontiguousarray(b["bins"]).view(np.uint8).reshape(-1, 8))
        jb, pj = bufs.put(b["jit"])
        cb, pc = bufs.put(b["covers"]); hb, phd = bufs.put(b["headers"]); yb, py = bufs.put(b["payloads"])
        ob, po = cb, pc                                   # in place
        ub, pu = bufs.put(np.zeros(nimg, np.int64))
        ctx.embed_stream_batch_walks_dev(nimg, pc, w, h, pb, pj, b["bins"].shape[1], phd, py, b["payloads"].shape[1], po, center=center,
                                         usable_ptr=pu)
        ctx.sync()
        return bufs.get(ob).copy(), bufs.get(ub).astype(np.int64), ctx.batch_exact_info(nimg)
    finally:
        ctx.close()


def _fit_dev(lib, bufs, b, slots, center, mode, iters):
    nimg = len(b["covers"])
    w, h = b["w"], b["h"]
    ctx = make_ctx(lib, w, h, slots, mode)
    try:
        kb, pb = bufs.put(np.ascontiguousarray(b["bins"]).view(np.uint8).reshape(-1, 8))
        jb, pj = bufs.put(b["jit"])
        cb, pc = bufs.put(b["covers"]); hb, phd = bufs.put(b["headers"]); yb, py = bufs.put(b["payloads"])
        ob, po = bufs.put(np.zeros_like(b["covers"]))
        ub, pu = bufs.put(np.zeros(nimg, np.int64))
        ctx.embed_stream_batch_fit_dev(nimg, pc, w, h, pb, pj, b["bins"].shape[1], phd, py, b["payloads"].shape[1], po, center=center,
                                       usable_ptr=pu, max_iters=iters)
        ctx.sync()
        return bufs.get(ob).copy(), bufs.get(ub).astype(np.int64), ctx.batch_exact_info(nimg)
    finally:
        ctx.close()
