"""Checks of the batched stream pipelines with one walk per image (tfft_*_stream_batch_walks[_dev], tfft_walks_build,
tfft_lowfreq_mag_batch_dev), shared by the emulated run (tests/test_emulated_walks.py, HostBufs) and the MI355X run
(tests/test_gpu_walks_batch.py, TorchBufs)."""
import hashlib

import numpy as np
import pytest

from _checkers import Params
from parity_cases import PK, _ctx_with_env, cover_of, host_cover_hash, load_cover_hash_cases, make_header, rep_stream
from phase_cases import STATS_ENVS, _phase_near_boundary
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

# how the per-image pipelines may be cut and run: every variant must give the bytes of the shared-list call
WALK_ENVS = STATS_ENVS + ({"TFFT_TILE_READ": "0"}, {"TFFT_TILE_READ": "3"}, {"TFFT_EMBED_DELTA": "0"}, {"TFFT_STREAMS": "2"})


def image_keys(orc, n, tag=b"walks"):
    """n distinct path keys and their subkeys (walk | r | g | b), as n users with their own passphrase would have"""
    pks = [hashlib.sha256(tag + b"#%d" % i).digest() for i in range(n)]
    return pks, b"".join(b"".join(orc.subkeys(pk)) for pk in pks)


def _frames(nimg, secret, seed):
    plen = secret + 16
    rng = np.random.default_rng(seed)
    headers = np.stack([make_header(secret, seed + i) for i in range(nimg)])
    payloads = np.stack([rng.integers(0, 256, plen).astype(np.uint8) for _ in range(nimg)])
    return headers, payloads


def _run(lib, bufs, env, w, h, slots, covers, bins, jit, adaptive, headers, payloads, center, walks, extract_src=None, host=False):
    """one embed (or, with extract_src, one extraction) through the shared-list call (walks False: `bins` is ONE list, jitter and adaptive
    set as phase options) or the per-image call (walks True: bins (n, n_bins), jitter (n, n_bins) or None)"""
    nimg = len(covers)
    n_bins = bins.shape[-1]
    plen = payloads.shape[1]
    ctx = _ctx_with_env(env, w, h, slots=slots, lib=lib)
    try:
        if not walks:
            ctx.set_phase_options(jit, adaptive)
        if host:
            if extract_src is None:
                out = np.zeros_like(covers); us = np.zeros(nimg, np.uint64)
                if walks:
                    ctx.embed_stream_batch_walks_host(covers, bins, headers, payloads, out, jitter=jit, adaptive=adaptive, usable=us, center=center)
                else:
                    ctx.embed_stream_batch_host(covers, bins, headers, payloads, out, usable=us, center=center)
                return out, us
            ho = np.zeros((nimg, 38), np.uint8); po = np.zeros((nimg, plen), np.uint8); so = np.zeros(nimg, np.int32)
            ro = np.zeros((nimg, n_bins), np.uint8)
            if walks:
                ctx.extract_stream_batch_walks_host(extract_src, bins, ho, po, so, ro, jitter=jit, adaptive=adaptive, center=center)
            else:
                ctx.extract_stream_batch_host(extract_src, bins, ho, po, so, ro, center=center)
            po[so < 0] = 0          # (no payload is defined for an image whose header was not found)
            return ho, po, so, ro
        kb, pb = bufs.put(np.ascontiguousarray(bins).view(np.uint8).reshape(-1, 8))
        jb, pj = bufs.put(jit) if (walks and jit is not None) else (None, None)
        if extract_src is None:
            cb, pc = bufs.put(covers); hb, ph_ = bufs.put(headers); yb, py = bufs.put(payloads)
            ob, po = bufs.put(np.zeros_like(covers)); ub, pu = bufs.put(np.zeros(nimg, np.uint64))
            if walks:
                ctx.embed_stream_batch_walks_dev(nimg, pc, w, h, pb, pj, n_bins, ph_, py, plen, po, adaptive=adaptive, center=center, usable_ptr=pu)
            else:
                ctx.embed_stream_batch_dev(nimg, pc, w, h, pb, n_bins, ph_, py, plen, po, center=center, usable_ptr=pu)
            ctx.sync()
            return bufs.get(ob).copy(), bufs.get(ub).copy()
        sb, ps = bufs.put(extract_src)
        hb, ph_ = bufs.put(np.zeros((nimg, 38), np.uint8)); yb, py = bufs.put(np.zeros((nimg, plen), np.uint8))
        stb, pst = bufs.put(np.zeros(nimg, np.int32)); rb, pr = bufs.put(np.full((nimg, n_bins), 7, np.uint8))
        if walks:
            ctx.extract_stream_batch_walks_dev(nimg, ps, w, h, pb, pj, n_bins, ph_, py, plen, pst, pr, adaptive=adaptive, center=center)
        else:
            ctx.extract_stream_batch_dev(nimg, ps, w, h, pb, n_bins, ph_, py, plen, pst, pr, center=center)
        ctx.sync()
        return bufs.get(hb).copy(), bufs.get(yb).copy(), bufs.get(stb).copy(), bufs.get(rb).copy()
    finally:
        ctx.close()


def check_same_lists(lib, orc, bufs, w, h, nimg, slots, secret=8, jitter=0.05, adaptive=True, center=False, envs=WALK_ENVS, host=True):
    """n copies of ONE walk through the per-image calls return the bytes of the shared-list call: stego, usable_out, headers, payloads,
    statuses and raw bits, under every statistics / read / embed / stream variant in `envs`"""
    plen = secret + 16
    n_bins = 912 + 56 * plen + 200
    keys = orc.subkeys(PK)
    bins = B.Walk(keys[0], orc.next_pow2(h), orc.next_pow2(w), lib=lib).next(n_bins)
    jit = B.walk_jitter(b"".join(keys[1:4]), bins, jitter, lib=lib) if jitter else None
    tb = np.ascontiguousarray(np.broadcast_to(bins, (nimg, n_bins)))
    tj = np.ascontiguousarray(np.broadcast_to(jit, (nimg, n_bins))) if jit is not None else None
    covers = np.stack([cover_rgb(w, h, 300 + i) for i in range(nimg)])
    headers, payloads = _frames(nimg, secret, 40)
    first = None
    for env in envs:
        want_s, want_u = _run(lib, bufs, env, w, h, slots, covers, bins, jit, adaptive, headers, payloads, center, walks=False)
        got_s, got_u = _run(lib, bufs, env, w, h, slots, covers, tb, tj, adaptive, headers, payloads, center, walks=True)
        assert np.array_equal(got_s, want_s), ("stego", env, int((got_s != want_s).sum()))
        assert np.array_equal(got_u, want_u), ("usable_out", env, got_u, want_u)
        want_x = _run(lib, bufs, env, w, h, slots, covers, bins, jit, adaptive, headers, payloads, center, walks=False, extract_src=want_s)
        got_x = _run(lib, bufs, env, w, h, slots, covers, tb, tj, adaptive, headers, payloads, center, walks=True, extract_src=want_s)
        for what, g, wnt in zip(("header", "payload", "status", "raw bits"), got_x, want_x):
            assert np.array_equal(g, wnt), (what, env)
        if (orc.next_pow2(h), orc.next_pow2(w)) == (h, w):      # (a padded cover loses the stream in the crop, in the reference too)
            assert list(got_x[2]) == [secret] * nimg, got_x[2]
            assert np.array_equal(got_x[0], headers) and np.array_equal(got_x[1], payloads)
        if first is None:
            first = (got_s, got_x)
    if host:        # the three-stream host pipeline (parts of the ring are smaller chunks): the lists and jitter travel with the images
        want_s, want_u = _run(lib, bufs, envs[0], w, h, slots, covers, bins, jit, adaptive, headers, payloads, center, walks=False, host=True)
        hs, hu = _run(lib, bufs, envs[0], w, h, slots, covers, tb, tj, adaptive, headers, payloads, center, walks=True, host=True)
        assert np.array_equal(hs, want_s) and np.array_equal(hu, want_u)
        want_x = _run(lib, bufs, envs[0], w, h, slots, covers, bins, jit, adaptive, headers, payloads, center, walks=False, extract_src=want_s, host=True)
        hx = _run(lib, bufs, envs[0], w, h, slots, covers, tb, tj, adaptive, headers, payloads, center, walks=True, extract_src=want_s, host=True)
        for what, g, wnt in zip(("header", "payload", "status", "raw bits"), hx, want_x):
            assert np.array_equal(g, wnt), ("host pipeline", what)


def check_distinct_keys(lib, orc, bufs, w, h, nimg, slots, secret=8, jitter=0.05, adaptive=False, center=False, n_oracle=None,
                        lsb_frac=0.05, envs=({},), n_threads=4, rmin=0.05, rmax=0.45, pks=None):
    """every image with its own key: each stego within the LSB bar of the fp64 reference's embed with that image's own walk, the raw
    bits read from the reference's stego equal the reference's on every stream position (beyond the stream only bins on the decision
    line may differ), payloads round-trip (power-of-two covers), and image i read with image j's walk is "Magic not found" (-1)"""
    P = Params(jitter=jitter, adaptive_alpha=int(adaptive), center=int(center), rmin=rmin, rmax=rmax)
    plen = secret + 16
    n_str = 912 + 56 * plen
    n_bins = n_str + 300
    ph, pw = orc.next_pow2(h), orc.next_pow2(w)
    if pks is None:
        pks, keys = image_keys(orc, nimg)
    else:           # the caller's own path keys, one per image
        assert len(pks) == nimg
        keys = b"".join(b"".join(orc.subkeys(pk)) for pk in pks)
    bins, jit, st = B.walks_build(keys, ph, pw, n_bins, max_jitter=jitter if jitter else None, rmin=rmin, rmax=rmax, n_threads=n_threads, lib=lib)
    assert (st == 0).all()
    covers = np.stack([cover_rgb(w, h, 500 + i) for i in range(nimg)])
    headers, payloads = _frames(nimg, secret, 70)
    n_or = nimg if n_oracle is None else n_oracle
    want, want_raw = [], []
    for i in range(n_or):
        ws = orc.embed_rgb8(covers[i], pks[i], rep_stream(headers[i], payloads[i]), P)[0]
        want.append(ws)
        want_raw.append(orc.extract_bits(ws, pks[i], n_bins, P))
    ours = None
    for env in envs:
        s, u = _run(lib, bufs, env, w, h, slots, covers, bins, jit, adaptive, headers, payloads, center, walks=True)
        if ours is None:
            ours = s
        if env.get("TFFT_EMBED_DELTA") == "0":      # F' written and inverted: 1 LSB from the delta form on a few pixels
            dm = np.abs(s.astype(np.int16) - ours)
            assert dm.max() <= 1 and float((dm != 0).mean()) < lsb_frac, (env, dm.max())
        else:
            assert np.array_equal(s, ours), env
    for i in range(n_or):
        dd = np.abs(ours[i].astype(np.int16) - want[i])
        assert dd.max() <= 1 and float((dd != 0).mean()) < lsb_frac, ("stego vs the fp64 reference", i, dd.max(), float((dd != 0).mean()))
    # the reference's stego (then ours for the images it did not embed) read with every image's own walk
    src = np.stack(want + [ours[i] for i in range(n_or, nimg)])
    ho, po, so, ro = _run(lib, bufs, envs[0], w, h, slots, covers, bins, jit, adaptive, headers, payloads, center, walks=True, extract_src=src)
    pow2 = (ph, pw) == (h, w)           # a padded cover loses its stream in the crop, in the reference too: no round trip to ask for
    if pow2:
        assert list(so) == [secret] * nimg, so
        assert np.array_equal(ho, headers) and np.array_equal(po, payloads)
    for i in range(n_or):
        assert np.array_equal(ro[i, :n_str], want_raw[i][:n_str]), ("raw bits vs the reference", i)
        bad = np.nonzero(ro[i] != want_raw[i])[0]
        if len(bad):
            near = _phase_near_boundary(orc, want[i], bins[i][bad], jit[i][bad] if jit is not None else None, center)
            assert near.all(), ("mismatch away from the decision line", i, bad[~near][:10])
    # our own stego round-trips; with the walks rotated by one image, nothing is found
    _, _, so, _ = _run(lib, bufs, envs[0], w, h, slots, covers, bins, jit, adaptive, headers, payloads, center, walks=True, extract_src=ours)
    if pow2:
        assert list(so) == [secret] * nimg, so
    rb = np.roll(bins, 1, axis=0)
    rj = np.roll(jit, 1, axis=0) if jit is not None else None
    _, _, so, _ = _run(lib, bufs, envs[0], w, h, slots, covers, rb, rj, adaptive, headers, payloads, center, walks=True, extract_src=ours)
    assert list(so) == [-1] * nimg, so
    return ours, bins, jit


def check_errors(lib, orc, bufs, w=128, h=128):
    """shared-list state on the context -> TFFT_E_STATE; adaptive extraction with |alpha| >= pi/2 -> TFFT_E_INVALID; an out-of-grid bin in
    one image's list -> TFFT_E_BIN_RANGE (device and host forms)"""
    nimg, plen = 2, 16
    n_bins = 912 + 56 * plen + 50
    pks, keys = image_keys(orc, nimg, b"errors")
    bins, jit, st = B.walks_build(keys, h, w, n_bins, max_jitter=0.05, lib=lib)
    assert (st == 0).all()
    covers = np.stack([cover_rgb(w, h, 7 + i) for i in range(nimg)])
    headers, payloads = _frames(nimg, 0, 5)
    kb, pb = bufs.put(bins.view(np.uint8).reshape(-1, 8)); cb, pc = bufs.put(covers)
    hb, phd = bufs.put(headers); yb, py = bufs.put(payloads); ob, po = bufs.put(np.zeros_like(covers))
    stb, pst = bufs.put(np.zeros(nimg, np.int32))
    ctx = B.Context(w, h, slots=2, lib=lib)
    for setup in ("index", "jitter"):
        if setup == "index":
            ctx.set_bit_index(np.arange(n_bins, dtype=np.uint32))
        else:
            ctx.set_phase_options(np.zeros(n_bins, np.float32), False)
        with pytest.raises(B.TfftError) as ei:
            ctx.embed_stream_batch_walks_dev(nimg, pc, w, h, pb, None, n_bins, phd, py, plen, po)
        assert ei.value.status == -6
        with pytest.raises(B.TfftError) as ei:
            ctx.extract_stream_batch_walks_dev(nimg, pc, w, h, pb, None, n_bins, phd, py, plen, pst)
        assert ei.value.status == -6
        ctx.set_bit_index(None)
        ctx.set_phase_options()
    ctx.set_phase_options(None, True)       # the context's adaptive flag alone is no shared-list state: the call's own argument rules
    ctx.embed_stream_batch_walks_dev(nimg, pc, w, h, pb, None, n_bins, phd, py, plen, po)
    ctx.set_phase_options()
    with pytest.raises(B.TfftError) as ei:
        ctx.extract_stream_batch_walks_dev(nimg, pc, w, h, pb, None, n_bins, phd, py, plen, pst, adaptive=True, alpha=1.6)
    assert ei.value.status == -1
    ctx.extract_stream_batch_walks_dev(nimg, pc, w, h, pb, None, n_bins, phd, py, plen, pst, adaptive=True, alpha=1.5)
    ctx.sync()
    bad = bins.copy()
    bad[1, 17]["y"] = 0                      # an excluded axis, in the second image's list only
    kb2, pb2 = bufs.put(bad.view(np.uint8).reshape(-1, 8))
    for fn in ("embed", "extract"):
        with pytest.raises(B.TfftError) as ei:
            if fn == "embed":
                ctx.embed_stream_batch_walks_dev(nimg, pc, w, h, pb2, None, n_bins, phd, py, plen, po)
            else:
                ctx.extract_stream_batch_walks_dev(nimg, pc, w, h, pb2, None, n_bins, phd, py, plen, pst)
        assert ei.value.status == -8, fn
    with pytest.raises(B.TfftError) as ei:
        ctx.embed_stream_batch_walks_host(covers, bad, headers, payloads, np.zeros_like(covers))
    assert ei.value.status == -8
    # the flag does not stick: the good lists pass again
    ctx.embed_stream_batch_walks_dev(nimg, pc, w, h, pb, None, n_bins, phd, py, plen, po)
    ctx.close()


def check_lowfreq_batch(lib, host, bufs, golden_dir, max_pixels=None, n_copies=2):
    """tfft_lowfreq_mag_batch_dev = tfft_lowfreq_mag on each image alone, bit for bit, and the hashes the reference made"""
    for c in load_cover_hash_cases(golden_dir, max_pixels):
        if c["region"] == 0:
            continue
        w, h, r = c["w"], c["h"], c["region"]
        imgs = np.stack([cover_of(c)] + [cover_rgb(w, h, 900 + k) for k in range(n_copies)])
        ctx = B.Context(w, h, slots=2, lib=lib)
        single = []
        for img in imgs:
            ctx.forward_rgb8(img, c["center"])
            single.append(ctx.lowfreq_mag(r))
        ib, pi = bufs.put(imgs)
        ob, po = bufs.put(np.full((len(imgs), 3, r, r), -1.0))
        ctx.lowfreq_mag_batch_dev(len(imgs), pi, w, h, r, po, center=c["center"])
        ctx.sync()
        got = bufs.get(ob).copy()
        ctx.close()
        for k in range(len(imgs)):
            assert np.array_equal(got[k].view(np.uint64), np.asarray(single[k]).reshape(3, r, r).view(np.uint64)), (c["w"], c["h"], k)
        assert host_cover_hash(host, got[0]).hex() == c["hash"], (c["w"], c["h"], c["note"])
