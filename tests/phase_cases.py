"""Checks of the batched pipelines' phase options (tfft_set_phase_options: jitter, adaptive alpha), shared by the
emulated run (tests/test_emulated_phase.py, HostBufs) and the MI355X run (tests/test_gpu_phase_batch.py, TorchBufs)."""
import numpy as np
import pytest

from _checkers import Params
from parity_cases import PK, _ctx_with_env, make_header, rep_stream
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

# statistics variants of the batched embed: with adaptive alpha the embed waits for the medians, and every variant must give them
STATS_ENVS = ({}, {"TFFT_STATS_TILE": "0"}, {"TFFT_STATS_TILE": "2"}, {"TFFT_MEDIAN_FALLBACK": "1"}, {"TFFT_STATS_FUSED": "0"})


def _walk(lib, orc, w, h, n, jitter, rmax=0.45):
    ph, pw = orc.next_pow2(h), orc.next_pow2(w)
    keys = orc.subkeys(PK)
    bins = B.Walk(keys[0], ph, pw, rmax=rmax, lib=lib).next(n)
    assert len(bins) == n
    # jitter in stream order, computed BEFORE the list is sorted
    jit = B.walk_jitter(b"".join(keys[1:4]), bins, jitter, lib=lib) if jitter else None
    return bins, jit


def check_phase_batch(lib, orc, bufs, w, h, n_bits, nimg=3, slots=2, jitter=0.05, adaptive=False, center=False, sort=True,
                      lsb_frac=0.02, n_oracle=None, envs=STATS_ENVS, tile_modes=("3", "0"), usable=True, rmax=0.45):
    """tfft_embed_batch_dev / tfft_extract_batch_dev with the phase options against the fp64 reference (Params(jitter, adaptive_alpha)):
    stego within 1 LSB on all but a small fraction of pixels, and the raw bits the reference reads from its own stego."""
    P = Params(jitter=jitter, adaptive_alpha=int(adaptive), center=int(center), rmax=rmax)
    bins, jit = _walk(lib, orc, w, h, n_bits, jitter, rmax)
    ubins, idx = B.bins_sort(bins, lib=lib) if sort else (bins, None)
    covers = np.stack([cover_rgb(w, h, 90 + i) for i in range(nimg)])
    bits = np.random.default_rng(8).integers(0, 2, (nimg, n_bits)).astype(np.uint8)
    kb, pb = bufs.put(ubins.view(np.uint8).reshape(-1, 8))
    cb, pc = bufs.put(covers)
    bb, pbits = bufs.put(bits)

    def embed(env, options=True, clear_first=False, with_usable=usable):
        ctx = _ctx_with_env(env, w, h, slots=slots, lib=lib)
        if idx is not None:
            ctx.set_bit_index(idx)
        if clear_first:
            ctx.set_phase_options(jit, True)
            ctx.set_phase_options()
        if options:
            ctx.set_phase_options(jit, adaptive)
        ob, po = bufs.put(np.zeros_like(covers))
        ub, pu = bufs.put(np.zeros(nimg, np.uint64))
        ctx.embed_batch_dev(nimg, pc, w, h, pb, pbits, n_bits, po, center=center, rmax=rmax, usable_ptr=pu if with_usable else None)
        ctx.sync()
        ctx.close()
        return bufs.get(ob).copy(), bufs.get(ub).copy()

    sd, ud = embed(envs[0])
    for env in envs[1:]:
        s2, u2 = embed(env)
        assert np.array_equal(s2, sd) and np.array_equal(u2, ud), ("statistics variant", env)
    if usable:      # the capacities do not depend on the phase options; without usable_out the statistics still run for adaptive
        s2, _ = embed(envs[0], with_usable=False)
        assert np.array_equal(s2, sd)
        _, u3 = embed(envs[0], options=False)
        assert np.array_equal(u3, ud)
    # write F' and invert (k_embed's generic path with the device medians): 1 LSB from the delta form on a few pixels
    s0, _ = embed({"TFFT_EMBED_DELTA": "0"})
    dm = np.abs(s0.astype(np.int16) - sd)
    assert dm.max() <= 1 and float((dm != 0).mean()) < lsb_frac, (dm.max(), float((dm != 0).mean()))
    assert np.array_equal(bufs.get(cb), covers)

    n_or = nimg if n_oracle is None else n_oracle
    want = []
    for i in range(n_or):
        ws = orc.embed_rgb8(covers[i], PK, bits[i], P)[0]
        dd = np.abs(sd[i].astype(np.int16) - ws)
        assert dd.max() <= 1 and float((dd != 0).mean()) < lsb_frac, ("stego vs the fp64 reference", i, dd.max(), float((dd != 0).mean()))
        want.append(ws)
    # extraction: the reference's stego images (then ours), every tile-read mode, against what the reference reads
    src = np.stack(want + [sd[i] for i in range(n_or, nimg)])
    sb, ps = bufs.put(src)
    want_raw = [orc.extract_bits(src[i], PK, n_bits, P) for i in range(n_or)]
    raws = []
    for mode in tile_modes:
        ctx = _ctx_with_env({"TFFT_TILE_READ": mode}, w, h, slots=slots, lib=lib)
        if idx is not None:
            ctx.set_bit_index(idx)
        ctx.set_phase_options(jit, adaptive)
        rb, pr = bufs.put(np.full((nimg, n_bits), 7, np.uint8))
        ctx.extract_batch_dev(nimg, ps, w, h, pb, n_bits, pr, center=center)
        ctx.sync()
        raw = bufs.get(rb).copy()
        for i in range(n_or):
            assert np.array_equal(raw[i], want_raw[i]), ("raw bits vs the reference", mode, i, int((raw[i] != want_raw[i]).sum()))
        raws.append(raw)
        if mode == tile_modes[0]:
            # a list of another length while the jitter is set: TFFT_E_STATE; adaptive with alpha >= pi/2: TFFT_E_INVALID
            if jit is not None:
                with pytest.raises(B.TfftError) as ei:
                    ctx.extract_batch_dev(nimg, ps, w, h, pb, n_bits - 1, pr, center=center)
                assert ei.value.status == -6          # TFFT_E_STATE
            if adaptive:
                with pytest.raises(B.TfftError) as ei:
                    ctx.extract_batch_dev(nimg, ps, w, h, pb, n_bits, pr, alpha=1.6, center=center)
                assert ei.value.status == -1          # TFFT_E_INVALID
        ctx.close()
    for r in raws[1:]:
        assert np.array_equal(r, raws[0])
    # no options (and options set, then cleared): the bytes of a context that never had any
    a, _ = embed(envs[0], options=False)
    b, _ = embed(envs[0], options=False, clear_first=True)
    assert np.array_equal(a, b)
    if jitter or adaptive:
        assert not np.array_equal(a, sd)
    return sd, bins, jit


def _phase_near_boundary(orc, stego, bins, jit, center, tol=1e-5):
    """per bin: the reference's phase lies within tol of the decision line through j and j + pi"""
    spec, _ = orc.forward_rgb8(stego, center=center)
    t = B.bins_to_triples(bins)
    th = np.angle(spec[t[:, 0], t[:, 1], t[:, 2]])
    d = np.mod(th - (jit.astype(np.float64) if jit is not None else 0.0), np.pi)
    return np.minimum(d, np.pi - d) < tol


def check_phase_stream(lib, orc, bufs, w, h, secret=24, nimg=2, slots=2, jitter=0.05, adaptive=True, center=False, sort=True,
                       check_single=True):
    """tfft_embed_stream_batch_dev -> tfft_extract_stream_batch_dev with the phase options: header and payload come back, status = clen;
    on the reference's stego every stream position reads the reference's bit, the positions beyond the stream differ only on bins
    whose phase lies on the decision line; the single-image tfft_read_bins with jitter and adaptive reads the same stego."""
    P = Params(jitter=jitter, adaptive_alpha=int(adaptive), center=int(center))
    plen = secret + 16
    n_str = 912 + 56 * plen
    n_bins = n_str + 300
    bins, jit = _walk(lib, orc, w, h, n_bins, jitter)
    ubins, idx = B.bins_sort(bins, lib=lib) if sort else (bins, None)
    ctx = B.Context(w, h, slots=slots, lib=lib)
    if idx is not None:
        ctx.set_bit_index(idx)
    ctx.set_phase_options(jit, adaptive)
    kb, pb = bufs.put(ubins.view(np.uint8).reshape(-1, 8))
    rng = np.random.default_rng(31)
    covers = np.stack([cover_rgb(w, h, 130 + i) for i in range(nimg)])
    headers = np.stack([make_header(secret, i) for i in range(nimg)])
    payloads = np.stack([rng.integers(0, 256, plen).astype(np.uint8) for _ in range(nimg)])
    ci, cp = bufs.put(covers); hi, hp = bufs.put(headers); pi, pp = bufs.put(payloads)
    oi, op = bufs.put(np.zeros_like(covers))
    ctx.embed_stream_batch_dev(nimg, cp, w, h, pb, n_bins, hp, pp, plen, op, center=center)
    ctx.sync()
    ours = bufs.get(oi).copy()
    want, want_raw = [], []
    for i in range(nimg):
        st = rep_stream(headers[i], payloads[i])
        assert len(st) == n_str
        ws = orc.embed_rgb8(covers[i], PK, st, P)[0]
        assert np.abs(ours[i].astype(np.int16) - ws).max() <= 1
        want.append(ws)
        want_raw.append(orc.extract_bits(ws, PK, n_bins, P))
    for src in (np.stack(want), ours):
        si, sp = bufs.put(src)
        ho, hop = bufs.put(np.zeros((nimg, 38), np.uint8)); po_, pop = bufs.put(np.zeros((nimg, plen), np.uint8))
        so, sop = bufs.put(np.zeros(nimg, np.int32)); ro, rop = bufs.put(np.zeros((nimg, n_bins), np.uint8))
        ctx.extract_stream_batch_dev(nimg, sp, w, h, pb, n_bins, hop, pop, plen, sop, rop, center=center)
        ctx.sync()
        assert list(bufs.get(so)) == [secret] * nimg
        assert np.array_equal(bufs.get(ho), headers) and np.array_equal(bufs.get(po_), payloads)
        raw = bufs.get(ro).copy()
        if src is ours:
            ours_raw = raw
            continue
        for i in range(nimg):
            assert np.array_equal(raw[i, :n_str], want_raw[i][:n_str]), i
            bad = np.nonzero(raw[i] != want_raw[i])[0]
            if len(bad):
                near = _phase_near_boundary(orc, want[i], bins[bad], jit[bad] if jit is not None else None, center)
                assert near.all(), ("mismatch away from the decision line", i, bad[~near][:10])
    ctx.close()
    if check_single:            # the single-image calls with the same options read the batch's stego
        one = B.Context(w, h, lib=lib)
        for i in range(nimg):
            one.forward_rgb8(ours[i], center=center)
            med = one.medians()
            got = one.read_bins(bins, jitter=jit, adaptive=adaptive, med=med)
            assert np.array_equal(got, ours_raw[i]), i
        one.close()
