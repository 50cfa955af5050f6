"""Robustness analysis on the device (tfft_channel_batch[_dev], tfft_robustness_batch[_dev]), written once and run
twice: on the CPU-emulated build of the kernel sources (tests/test_emulated_robust.py) and on the MI355X (tests/test_gpu_robust.py, -m gpu).

The channels are checked against fp64 restatements of their definitions in numpy (awgn_ref, jpeg_ref below):
  AWGN  out is within 1 LSB of clamp(rint(v)), v = pixel + sigma*g in fp64, everywhere, and equal to it wherever v is farther than
        AWGN_BAR * max(1, sigma) from a half-integer; the share of bytes inside that bar is a property of the input and stays <= 1 %.
        (An fp32 evaluation of g differs from fp64 by at most 6e-5; the kernel forms both uniforms exactly and takes ln(u1) near 1 through
        log1p, so its g is a few fp32 ulps of sqrt, log and cos away: well inside 1e-4.)
  JPEG  a block is ambiguous when any of its 192 fp64 coefficients c has |frac(c/q) - 1/2| <= JPEG_BAR (the fp32 transform may then
        quantise it to the other level: a whole step q in that coefficient).  In every other block every pixel is within 1 LSB of the
        reference and at most 0.1 % of those pixels differ at all (a final value within fp32 error of a half-integer); the share of
        ambiguous blocks stays <= 1/8.  JPEG_BAR: the fp32 error of a coefficient is a few ulps of the block's largest value (|DC| <= 1024:
        6e-5 per ulp at the very top, typically 1e-5), divided by q >= 1.
The robustness call is compared with == against the sequence of public calls that defines it (compose below)."""
import functools

import numpy as np
import pytest

from parity_cases import make_header
from steganosaurus_amd import analysis as A
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb, gradient_cover

AWGN_BAR = 1e-4
JPEG_BAR = 1e-4
INVALID, TOO_LARGE, STATE = -1, -3, -6
GOLDEN = 0x9E3779B97F4A7C15
CHANNELS = [("none",), ("awgn", 2.0, 7), ("jpeg", 75), ("jpeg", 30)]

# ITU-T T.81 Annex K, tables K.1 and K.2, natural order
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
               103, 99], np.int64).reshape(8, 8)
K2 = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
              + [99] * 32, np.int64).reshape(8, 8)


def p2(v):
    return 1 << (int(v) - 1).bit_length()


def covers_of(w, h, n=3):
    """the inputs of the channel checks: cover_rgb(w, h, 3), gradient_cover(w, h, 3), then further synthetic covers"""
    return np.stack([cover_rgb(w, h, 3), gradient_cover(w, h, 3), cover_rgb(w, h, 4), gradient_cover(w, h, 5)][:n])


# ---- fp64 references ---------------------------------------------------------------------------------------------------
def awgn_value(rgb, sigma, seed, first_image=0):
    """v = pixel + sigma*g in fp64 for a packed batch (n, H, W, 3), byte for byte"""
    flat = rgb.reshape(-1)
    per = int(np.prod(rgb.shape[1:]))
    with np.errstate(over="ignore"):
        idx = np.uint64(first_image) * np.uint64(per) + np.arange(flat.size, dtype=np.uint64)
        z = np.uint64(seed) + np.uint64(GOLDEN) * idx + np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u1 = ((z >> np.uint64(40)).astype(np.float64) + 0.5) / 2.0 ** 24
    u2 = (((z >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) + 0.5) / 2.0 ** 24
    g = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return (flat.astype(np.float64) + float(sigma) * g).reshape(rgb.shape), g


def check_awgn(got, rgb, sigma, seed, first_image=0, tag=""):
    v, _ = awgn_value(rgb, sigma, seed, first_image)
    want = np.clip(np.rint(v), 0, 255)
    diff = np.abs(got.astype(np.float64) - want)
    assert diff.max() <= 1, (tag, "more than 1 LSB", diff.max())
    near = np.abs(v - np.floor(v) - 0.5) <= AWGN_BAR * max(1.0, float(sigma))
    share = float(near.mean())
    print("awgn", tag, "sigma", sigma, "inside the bar %.4f %%" % (100 * share), "differ", int((diff > 0).sum()))
    assert share <= 0.01, (tag, share)
    assert not (diff[~near] > 0).any(), (tag, int((diff[~near] > 0).sum()))


def quant_tables(q):
    s = 5000 // q if q < 50 else 200 - 2 * q
    return [np.clip((t * s + 50) // 100, 1, 255).astype(np.float64) for t in (K1, K2)]


def dct_matrix():
    k, n = np.mgrid[0:8, 0:8]
    d = 0.5 * np.cos((2 * n + 1) * k * np.pi / 16)
    d[0] = np.sqrt(1.0 / 8.0)
    return d


def jpeg_ref(rgb, q):
    """(reference pixels as fp64 before the final rint, ambiguous-block map (by, bx)) of one (H, W, 3) image"""
    h, w = rgb.shape[:2]
    h8, w8 = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    x = np.pad(rgb.astype(np.float64), ((0, h8 - h), (0, w8 - w), (0, 0)), mode="edge")
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    ycc = np.stack([.299 * r + .587 * g + .114 * b - 128.0, -.168736 * r - .331264 * g + .5 * b, .5 * r - .418688 * g - .081312 * b])
    blk = ycc.reshape(3, h8 // 8, 8, w8 // 8, 8).transpose(0, 1, 3, 2, 4)          # (3, by, bx, 8, 8)
    d = dct_matrix()
    co = np.einsum("ky,cabyx,lx->cabkl", d, blk, d)
    ql, qc = quant_tables(q)
    qt = np.stack([ql, qc, qc])[:, None, None]
    t = co / qt
    amb = (np.abs(t - np.floor(t) - 0.5) <= JPEG_BAR).any(axis=(0, 3, 4))
    back = np.einsum("ky,cabkl,lx->cabyx", d, np.rint(t) * qt, d)
    ycc2 = back.transpose(0, 1, 3, 2, 4).reshape(3, h8, w8)
    yy, cb, cr = ycc2[0] + 128.0, ycc2[1], ycc2[2]
    out = np.stack([yy + 1.402 * cr, yy - .344136 * cb - .714136 * cr, yy + 1.772 * cb], axis=-1)
    return out[:h, :w], amb


def check_jpeg(got, rgb, q, tag=""):
    """got, rgb: (n, H, W, 3)"""
    n, h, w = rgb.shape[:3]
    n_amb = n_blocks = n_pix = n_diff = 0
    for i in range(n):
        ref, amb = jpeg_ref(rgb[i], q)
        want = np.clip(np.rint(ref), 0, 255)
        ok = np.repeat(np.repeat(~amb, 8, axis=0), 8, axis=1)[:h, :w]
        diff = np.abs(got[i].astype(np.float64) - want)[ok]
        assert diff.size == 0 or diff.max() <= 1, (tag, i, q, "more than 1 LSB in an unambiguous block", diff.max())
        n_amb += int(amb.sum()); n_blocks += amb.size; n_pix += diff.size; n_diff += int((diff > 0).sum())
    print("jpeg", tag, "Q", q, "ambiguous blocks %.2f %%" % (100.0 * n_amb / n_blocks), "differing values %.4f %%" % (100.0 * n_diff / max(n_pix, 1)))
    assert n_amb <= n_blocks / 8, (tag, q, n_amb, n_blocks)
    assert n_diff <= 0.001 * n_pix, (tag, q, n_diff, n_pix)


# ---- channels ----------------------------------------------------------------------------------------------------------
def run_channel(bufs, ctx, rgb, channel, first_image=0, in_place=False):
    n, h, w = rgb.shape[:3]
    ii, ip = bufs.put(rgb)
    if in_place:
        oi, op = ii, ip
    else:
        oi, op = bufs.put(np.full(rgb.shape, 0x5A, np.uint8))
    ctx.channel_batch_dev(n, ip, w, h, channel, op, first_image=first_image)
    ctx.sync()
    out = np.asarray(bufs.get(oi)).reshape(rgb.shape).copy()
    if not in_place:
        assert np.array_equal(np.asarray(bufs.get(ii)).reshape(rgb.shape), rgb), "the input was written"
    return out


def check_channel_forms(lib, bufs, rgb, channel, slots=2):
    """one channel over a batch: out of place == in place == the host form == a second call == the images one by one with their index as
    first_image (several chunks: slots < n).  Returns the attacked batch"""
    n, h, w = rgb.shape[:3]
    ctx = B.Context(w, h, slots=slots, lib=lib)
    try:
        out = run_channel(bufs, ctx, rgb, channel)
        assert np.array_equal(run_channel(bufs, ctx, rgb, channel, in_place=True), out), (channel, "in place")
        assert np.array_equal(run_channel(bufs, ctx, rgb, channel), out), (channel, "second call")
        assert np.array_equal(ctx.channel_batch_host(rgb, channel), out), (channel, "host form")
        hp = rgb.copy()
        assert ctx.channel_batch_host(hp, channel, out=hp) is hp and np.array_equal(hp, out), (channel, "host form in place")
        for i in range(n):
            assert np.array_equal(run_channel(bufs, ctx, rgb[i:i + 1], channel, first_image=i)[0], out[i]), (channel, "single", i)
        return out
    finally:
        ctx.close()


def check_awgn_shape(lib, bufs, w, h, n=3, sigmas=(0.5, 2.0, 8.0), seed=7, slots=2):
    rgb = covers_of(w, h, n)
    for sigma in sigmas:
        out = check_channel_forms(lib, bufs, rgb, ("awgn", sigma, seed), slots)
        check_awgn(out, rgb, sigma, seed, 0, (w, h))
    ctx = B.Context(w, h, slots=slots, lib=lib)
    try:
        assert np.array_equal(run_channel(bufs, ctx, rgb, ("awgn", 0.0, seed)), rgb), "sigma 0"
        assert np.array_equal(run_channel(bufs, ctx, rgb, ("none",)), rgb), "kind 0"
        assert np.array_equal(run_channel(bufs, ctx, rgb, ("none",), in_place=True), rgb), "kind 0 in place"
        other = run_channel(bufs, ctx, rgb, ("awgn", 2.0, seed + 1))
        assert not np.array_equal(other, run_channel(bufs, ctx, rgb, ("awgn", 2.0, seed))), "the seed is used"
        check_awgn(run_channel(bufs, ctx, rgb[:1], ("awgn", 2.0, 2 ** 63 + 5), first_image=2 ** 40), rgb[:1], 2.0, 2 ** 63 + 5, 2 ** 40, "big index")
    finally:
        ctx.close()


def check_jpeg_shape(lib, bufs, w, h, n=3, qualities=(30, 75, 90, 100), slots=2):
    rgb = covers_of(w, h, n)
    for q in qualities:
        out = check_channel_forms(lib, bufs, rgb, ("jpeg", q), slots)
        check_jpeg(out, rgb, q, (w, h))


def check_channel_errors(lib, bufs, w=48, h=40):
    ctx = B.Context(w, h, slots=2, lib=lib)
    rgb = cover_rgb(w, h, 0)[None].copy()
    out = np.zeros_like(rgb)
    big = cover_rgb(w + 1, h, 0)[None].copy()
    tall = cover_rgb(w, h + 1, 0)[None].copy()
    keep = [bufs.put(a) for a in (rgb, out, big, tall)]      # the _dev form's buffers
    try:
        for fn, (src, dst, bg, tl) in ((lib.tfft_channel_batch, (rgb, out, big, tall)), (lib.tfft_channel_batch_dev, [k[1] for k in keep])):
            def call(ctxh, n, s, ww, hh, ch, d):
                c = None if ch is None else B.make_channels(ch if isinstance(ch, np.ndarray) else [ch])
                return fn(ctxh, n, B._ptr(s), ww, hh, B._ptr(c), 0, B._ptr(d))
            for ch in (("none",), ("awgn", 0.0), ("awgn", 3.5, 9), ("jpeg", 1), ("jpeg", 100)):
                assert call(ctx.h, 1, src, w, h, ch, dst) == 0, ch
            bad = B.make_channels([("none",)] * 2)
            bad[0]["kind"], bad[1]["kind"] = 3, -1
            for ch in (bad[0:1], bad[1:2], ("awgn", -0.5), ("awgn", float("nan")), ("awgn", float("inf")), ("jpeg", 0), ("jpeg", 101),
                       ("jpeg", 50.5), ("jpeg", float("nan"))):
                assert call(ctx.h, 1, src, w, h, ch, dst) == INVALID, ch
            ok = ("jpeg", 75)
            assert call(None, 1, src, w, h, ok, dst) == INVALID
            assert call(ctx.h, 0, src, w, h, ok, dst) == INVALID
            assert call(ctx.h, -1, src, w, h, ok, dst) == INVALID
            assert call(ctx.h, 1, None, w, h, ok, dst) == INVALID
            assert call(ctx.h, 1, src, w, h, ok, None) == INVALID
            assert call(ctx.h, 1, src, w, h, None, dst) == INVALID
            assert call(ctx.h, 1, src, 0, h, ok, dst) == INVALID
            assert call(ctx.h, 1, bg, w + 1, h, ok, bg) == TOO_LARGE
            assert call(ctx.h, 1, tl, w, h + 1, ok, tl) == TOO_LARGE
            ctx.sync()
    finally:
        ctx.close()


def check_channel_leaves_slots(lib, bufs, w=64, h=64):
    """a resident single-image forward keeps its answers across channel calls of both forms"""
    a, b = cover_rgb(w, h, 40), np.stack([cover_rgb(w, h, 41 + i) for i in range(3)])
    ctx = B.Context(w, h, slots=2, lib=lib)
    try:
        ctx.forward_rgb8(a)
        m1, med1 = ctx.lowfreq_mag(4), ctx.medians()
        ctx.channel_batch_host(b, ("jpeg", 50))
        run_channel(bufs, ctx, b, ("awgn", 1.0, 1))
        assert np.array_equal(ctx.lowfreq_mag(4), m1) and np.array_equal(ctx.medians(), med1)
    finally:
        ctx.close()


# ---- the robustness call -----------------------------------------------------------------------------------------------
KEYS = bytes(range(32)), bytes(range(100, 196))


@functools.lru_cache(maxsize=None)
def _walk(lib_id, ph, pw, n_bins, jitter):
    lib = _LIBS[lib_id]
    bins = B.Walk(KEYS[0], ph, pw, lib=lib).next(n_bins)
    jit = B.walk_jitter(KEYS[1], bins, 0.2, lib=lib) if jitter else None
    return bins, jit


_LIBS = {}


def flat_cover(w, h, seed):
    """A cover whose stego reads back every raw bit when w and h are powers of two: noise of standard deviation 24 about 128 whose
    spectrum has the same magnitude M = 24 sqrt(wh) in every bin.  The rounding of the stego to bytes moves a coefficient by about
    sqrt(wh/12), 1/80 of M; a bit flips only where that exceeds |F| sin(alpha), and in a white-noise cover (|F| Rayleigh distributed: the
    synthetic covers) one or two of 2500 bins are that small.  5 sigma stay inside 0..255: nothing is clamped."""
    rng = np.random.default_rng(seed)
    f = np.fft.fft2(rng.normal(size=(3, h, w)))
    x = np.fft.ifft2(f / np.abs(f)).real * (24.0 * np.sqrt(w * h))
    return np.moveaxis(np.clip(np.rint(128.0 + x), 0, 255), 0, 2).astype(np.uint8)


def make_case(lib, bufs, w, h, n, payload_len, sort, phase, center=False, alpha=0.5, extra_bins=500, seed=11):
    """n stegos of w x h through tfft_embed_stream_batch_dev with one shared walk, header and payload per image.  sort: address-ordered list +
    bit index; phase: jitter + adaptive alpha through tfft_set_phase_options.  Returns what the robustness call needs"""
    _LIBS[id(lib)] = lib
    n_bins = 912 + 56 * payload_len + extra_bins
    bins, jit = _walk(id(lib), p2(h), p2(w), n_bins, bool(phase))
    rng = np.random.default_rng(seed)
    hdr = np.stack([make_header(payload_len - 16, i) for i in range(n)])
    pay = rng.integers(0, 256, (n, payload_len)).astype(np.uint8)
    covers = np.stack([flat_cover(w, h, 60 + i) for i in range(n)])
    ubins, idx = (B.bins_sort(bins, lib=lib) if sort else (bins, None))
    ctx = B.Context(w, h, slots=n, lib=lib)
    try:
        configure(ctx, idx, jit, phase)
        ki, kp = bufs.put(np.ascontiguousarray(ubins).view(np.uint8).reshape(-1, 8))
        hi, hp = bufs.put(hdr)
        pi, pp = bufs.put(pay)
        ci, cp = bufs.put(covers)
        oi, op = bufs.put(np.zeros_like(covers))
        ctx.embed_stream_batch_dev(n, cp, w, h, kp, n_bins, hp, pp, payload_len, op, alpha=alpha, center=center)
        ctx.sync()
        stego = np.asarray(bufs.get(oi)).reshape(covers.shape).copy()
    finally:
        ctx.close()
    return dict(w=w, h=h, n=n, plen=payload_len, n_bins=n_bins, ubins=np.ascontiguousarray(ubins), idx=idx, jit=jit, phase=phase, hdr=hdr, pay=pay,
                stego=stego, center=center, alpha=alpha)


def configure(ctx, idx, jit, phase):
    if idx is not None:
        ctx.set_bit_index(idx)
    if phase:
        ctx.set_phase_options(jit, adaptive=True)


def compose(bufs, ctx, case, channels, first_image=0):
    """the definition: channel -> stream extract (raw bits, status) -> expand / majority at the known length -> counts, by public calls"""
    w, h, n, plen, n_bins = case["w"], case["h"], case["n"], case["plen"], case["n_bins"]
    ns = 912 + 56 * plen
    si, sp = bufs.put(case["stego"])
    ki, kp = bufs.put(case["ubins"].view(np.uint8).reshape(-1, 8))
    hi, hp = bufs.put(case["hdr"])
    pi, pp = bufs.put(case["pay"])
    ei, ep = bufs.put(np.zeros((n, ns), np.uint8))
    ctx.frame_expand_dev(n, hp, pp, plen, ep)
    ctx.sync()
    expect = np.asarray(bufs.get(ei)).reshape(n, ns).copy()
    out = np.zeros((len(channels), n, 4), np.uint32)
    for k, ch in enumerate(channels):
        ai, ap = bufs.put(np.zeros_like(case["stego"]))
        ctx.channel_batch_dev(n, sp, w, h, ch, ap, first_image=first_image)
        ho, hop = bufs.put(np.zeros((n, 38), np.uint8))
        po, pop = bufs.put(np.zeros((n, plen), np.uint8))
        so, sop = bufs.put(np.zeros(n, np.int32))
        ro, rop = bufs.put(np.zeros((n, n_bins), np.uint8))
        ctx.extract_stream_batch_dev(n, ap, w, h, kp, n_bins, hop, pop, plen, sop, raw_bits_out_ptr=rop, alpha=case["alpha"], center=case["center"])
        ctx.sync()
        raw = np.asarray(bufs.get(ro)).reshape(n, n_bins)[:, :ns].copy()
        status = np.asarray(bufs.get(so)).copy()
        ri, rp = bufs.put(raw)
        mh, mhp = bufs.put(np.zeros((n, 38), np.uint8))
        mp, mpp = bufs.put(np.zeros((n, plen), np.uint8))
        ctx.frame_majority_dev(n, rp, plen, mhp, mpp)
        ctx.sync()
        out[k, :, 0] = (raw != expect).sum(axis=1)
        out[k, :, 1] = (np.asarray(bufs.get(mh)).reshape(n, 38) != case["hdr"]).sum(axis=1)
        out[k, :, 2] = (np.asarray(bufs.get(mp)).reshape(n, plen) != case["pay"]).sum(axis=1)
        out[k, :, 3] = status.astype(np.uint32)
    return out


def run_robust_dev(bufs, ctx, case, channels, first_image=0):
    w, h, n = case["w"], case["h"], case["n"]
    si, sp = bufs.put(case["stego"])
    ki, kp = bufs.put(case["ubins"].view(np.uint8).reshape(-1, 8))
    hi, hp = bufs.put(case["hdr"])
    pi, pp = bufs.put(case["pay"])
    ri, rp = bufs.put(np.full((len(channels), n, 4), 0xDEADBEEF, np.uint32))
    ctx.robustness_batch_dev(n, sp, w, h, kp, case["n_bins"], hp, pp, case["plen"], channels, rp, alpha=case["alpha"], center=case["center"],
                             first_image=first_image)
    ctx.sync()
    assert np.array_equal(np.asarray(bufs.get(si)).reshape(case["stego"].shape), case["stego"]), "the stego was written"
    return np.asarray(bufs.get(ri)).reshape(len(channels), n, 4).copy()


def check_robustness(lib, bufs, case, channels=CHANNELS, slot_counts=(2, 1), reads_back=True, first_image=5):
    """the call in every slot count (partial last chunks), _dev and host form, twice == the composition in a context that holds the whole
    batch; `none` reads back; the slots are left as an extract batch call leaves them"""
    w, h, n, plen = case["w"], case["h"], case["n"], case["plen"]
    ref_ctx = B.Context(w, h, slots=n, lib=lib)
    try:
        configure(ref_ctx, case["idx"], case["jit"], case["phase"])
        want = compose(bufs, ref_ctx, case, channels, first_image)
    finally:
        ref_ctx.close()
    print("robustness", (w, h, n, plen), want.reshape(len(channels), -1).tolist())
    if reads_back:
        assert (want[0] == np.array([0, 0, 0, plen - 16], np.uint32)).all(), want[0]
        assert A.recovered(want, plen)[0].all() and (A.raw_ber(want, plen)[0] == 0).all() and (A.byte_error_rate(want, plen)[0] == 0).all()
    for slots in slot_counts:
        ctx = B.Context(w, h, slots=slots, lib=lib)
        try:
            configure(ctx, case["idx"], case["jit"], case["phase"])
            got = run_robust_dev(bufs, ctx, case, channels, first_image)
            assert np.array_equal(got, want), (slots, got.tolist(), want.tolist())
            assert np.array_equal(run_robust_dev(bufs, ctx, case, channels, first_image), want), (slots, "second call")
            host = ctx.robustness_batch_host(case["stego"], case["ubins"], case["hdr"], case["pay"], channels, alpha=case["alpha"],
                                             center=case["center"], first_image=first_image)
            assert np.array_equal(host, want), (slots, "host form", host.tolist(), want.tolist())
            for probe in (ctx.medians, lambda: ctx.lowfreq_mag(4)):      # no spectrum and no single image in the slots: as after an extract batch
                with pytest.raises(B.TfftError) as e:
                    probe()
                assert e.value.status == STATE
        finally:
            ctx.close()
    return want


def check_jpeg_order(lib, bufs, case):
    """a coarser quantiser costs more raw bits (an inequality only)"""
    ctx = B.Context(case["w"], case["h"], slots=2, lib=lib)
    try:
        configure(ctx, case["idx"], case["jit"], case["phase"])
        r = run_robust_dev(bufs, ctx, case, [("jpeg", 30), ("jpeg", 100)])
    finally:
        ctx.close()
    assert (r[0, :, 0] > r[1, :, 0]).all(), r.tolist()
    assert (A.raw_ber(r, case["plen"])[0] > A.raw_ber(r, case["plen"])[1]).all()


def check_robust_errors(lib, bufs, case):
    w, h, n, plen, n_bins = case["w"], case["h"], case["n"], case["plen"], case["n_bins"]
    ctx = B.Context(w, h, slots=2, lib=lib)
    ch = B.make_channels([("none",), ("jpeg", 75)])
    host = dict(stego=case["stego"], bins=case["ubins"], hdr=case["hdr"], pay=case["pay"], out=np.zeros((2, n, 4), np.uint32))
    keep = {k: bufs.put(v.view(np.uint8).reshape(-1, 8) if k == "bins" else v) for k, v in host.items()}
    dev = {k: v[1] for k, v in keep.items()}
    forms = ((lib.tfft_robustness_batch, host), (lib.tfft_robustness_batch_dev, dev))
    try:
        def call(fn, arrs, ctxh=ctx.h, n_images=n, ww=w, nb=n_bins, alpha=0.5, pl=plen, chans=ch, nch=2, **over):
            a = dict(arrs, **over)
            return fn(ctxh, n_images, B._ptr(a["stego"]), ww, h, 0, B._ptr(a["bins"]), nb, alpha, B._ptr(a["hdr"]), B._ptr(a["pay"]), pl, B._ptr(chans),
                      nch, 0, B._ptr(a["out"]))
        for fn, arrs in forms:
            assert call(fn, arrs) == 0
            bad = ch.copy(); bad[1]["param"] = 0
            for kw in (dict(ctxh=None), dict(n_images=0), dict(stego=None), dict(bins=None), dict(hdr=None), dict(pay=None), dict(chans=None), dict(out=None),
                       dict(nch=0), dict(nch=-1), dict(chans=bad), dict(nb=912 + 56 * plen - 1), dict(nb=0), dict(pl=2 ** 62)):
                assert call(fn, arrs, **kw) == INVALID, kw
            assert call(fn, arrs, ww=w + 1) == TOO_LARGE
            ctx.sync()
        ctx.set_bit_index(np.arange(n_bins - 1, dtype=np.uint32))
        assert [call(fn, arrs) for fn, arrs in forms] == [STATE, STATE]
        ctx.set_bit_index(None)
        ctx.set_phase_options(np.zeros(n_bins, np.float32), adaptive=True)
        assert [call(fn, arrs, alpha=2.0) for fn, arrs in forms] == [INVALID, INVALID]
        ctx.set_phase_options()
        ctx.sync()
    finally:
        ctx.close()
