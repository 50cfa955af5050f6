"""Stego analysis on the device (tfft_phase_hist_batch[_dev], tfft_quality_batch[_dev]), written once and run twice:
on the CPU-emulated build of the kernel sources (tests/test_emulated_analysis.py) and on the MI355X (tests/test_gpu_analysis.py, -m gpu).

The oracle spectrum is the fp64 one (the oracle's forward transform, or np.fft with the reference's sign convention: F = conj(fft2) of the
real centred, zero-padded planes).  Histograms: with no threshold every histogram sums to the oracle's annulus count exactly (integer
geometry); with one the sum may differ only by threshold-ambiguous values, and the L1 distance to the oracle histogram is at most twice the
number of ambiguous values: a value is ambiguous when its fp64 angle lies within (1e-5 |F| + 1e-6 rms) / |F| + 1e-6 rad of a bin edge (the
FFT bar of parity_cases.spec_errors plus atan2f's error) or, with a threshold, its fp64 |F| within that FFT bar of it.  Quality: SSE equals
the int64 sum exactly, SSIM lies within 1e-4 of the fp64 definition below."""
import struct
import zlib

import numpy as np

from parity_cases import make_header
from steganosaurus_amd import analysis as A
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

RADII = ((0.05, 0.45), (0.0, 0.7))
INVALID, TOO_LARGE = -1, -3


def p2(v):
    return 1 << (int(v) - 1).bit_length()


def np_spectrum(rgb, center=False):
    """(3, PH, PW) complex128: to_planes_u8 + apply_center + pad_to_fft + forward fft2 (S:912-921) in numpy fp64"""
    h, w = rgb.shape[:2]
    planes = np.zeros((3, p2(h), p2(w)), np.float64)
    planes[:, :h, :w] = np.moveaxis(rgb.astype(np.float64), 2, 0)
    if center:
        yy, xx = np.mgrid[0:h, 0:w]
        planes[:, :h, :w] *= np.where((yy + xx) & 1, -1.0, 1.0)
    return np.conj(np.fft.fft2(planes))


def median_abs(plane):
    """median_abs (S:404-409): element at sorted index P/2 of |F| over the full padded plane"""
    a = np.abs(plane).ravel()
    return float(np.partition(a, a.size // 2)[a.size // 2])


def annulus(ph, pw, rmin, rmax):
    """(ys, xs) of the bins count_plane (S:998-1008) visits: off the axes, rmin*mn <= hypot(y, x) <= rmax*mn (sqrt of the exact integer
    y*y + x*x is correctly rounded, as the reference's hypot)"""
    mn = min(ph, pw)
    hi = int(min(max(np.floor(rmax * mn) + 1, 0), max(ph, pw)))
    yy, xx = np.mgrid[0:min(hi, ph), 0:min(hi, pw)]
    r = np.sqrt((yy * yy + xx * xx).astype(np.float64))
    keep = (yy != 0) & (xx != 0) & (2 * yy != ph) & (2 * xx != pw) & ~(r < rmin * mn) & ~(r > rmax * mn)
    return yy[keep], xx[keep]


def oracle_hist(plane, rmin, rmax, nbins, thr=None):
    """(hist, count, ambiguous, threshold-ambiguous) of one fp64 plane"""
    ph, pw = plane.shape
    ys, xs = annulus(ph, pw, rmin, rmax)
    f = plane[ys, xs]
    mag = np.abs(f)
    rms = np.sqrt(np.mean(np.abs(plane) ** 2))
    bar = 1e-5 * mag + 1e-6 * rms
    amb_thr = np.zeros(mag.shape, bool)
    if thr is not None:
        amb_thr = np.abs(mag - thr) <= bar
        keep = ~(mag < thr)
    else:
        keep = np.ones(mag.shape, bool)
    t = (np.angle(f) + np.pi) * nbins / (2 * np.pi)
    frac = t - np.floor(t)
    edge = np.minimum(frac, 1.0 - frac) * (2 * np.pi / nbins)
    with np.errstate(divide="ignore", invalid="ignore"):
        amb_edge = ~(edge > bar / mag + 1e-6)
    b = np.floor(t).astype(np.int64) % nbins
    hist = np.bincount(b[keep], minlength=nbins)
    return hist, int(keep.sum()), int((amb_edge | amb_thr).sum()), int(amb_thr.sum())


def check_hist(got, spec, rmin, rmax, nbins, thr=None, tag=""):
    """got: (3, nbins) uint32 of one image; spec: its (3, PH, PW) fp64 spectrum; thr: 3 thresholds or None"""
    assert got.shape == (3, nbins), (tag, got.shape)
    for p in range(3):
        want, count, amb, amb_thr = oracle_hist(spec[p], rmin, rmax, nbins, None if thr is None else thr[p])
        s = int(got[p].sum(dtype=np.int64))
        if thr is None:
            assert s == count, (tag, p, s, count)
        else:
            assert abs(s - count) <= amb_thr, (tag, p, s, count, amb_thr)
        l1 = int(np.abs(got[p].astype(np.int64) - want).sum())
        assert l1 <= 2 * amb, (tag, p, "L1", l1, "ambiguous", amb)


def hist_dev(lib, bufs, ctx, covers, nbins, center=False, rmin=0.05, rmax=0.45, thr=None):
    n, h, w = covers.shape[:3]
    ii, ip = bufs.put(covers)
    oi, op = bufs.put(np.full(n * 3 * nbins, 0xFFFFFFFF, np.uint32))
    ctx.phase_hist_batch_dev(n, ip, w, h, op, nbins=nbins, center=center, rmin=rmin, rmax=rmax, thr=thr)
    ctx.sync()
    return np.asarray(bufs.get(oi)).reshape(n, 3, nbins).copy()


def check_hist_image(lib, bufs, rgb, center, spec, nbins_list=(8, 256, 4096), radii=RADII, slots=1):
    """every (nbins, radii, thr in {None, 0.01 x oracle median}) of one image through the host form, the _dev form agreeing"""
    h, w = rgb.shape[:2]
    med = np.array([median_abs(spec[p]) for p in range(3)])
    ctx = B.Context(w, h, slots=slots, lib=lib)
    try:
        for nbins in nbins_list:
            for (rmin, rmax) in radii:
                for thr in (None, 0.01 * med):
                    tag = (w, h, center, nbins, rmin, rmax, thr is not None)
                    got = ctx.phase_hist_batch_host(rgb[None], nbins=nbins, center=center, rmin=rmin, rmax=rmax, thr=thr)
                    check_hist(got[0], spec, rmin, rmax, nbins, thr, tag)
                    dev = hist_dev(lib, bufs, ctx, rgb[None], nbins, center, rmin, rmax, thr)
                    assert np.array_equal(dev, got), tag
    finally:
        ctx.close()


def check_hist_chunks(lib, bufs, covers, nbins=256, center=False, slots=2, rmin=0.05, rmax=0.45):
    """n images in `slots` slots (several chunks): identical counts to single-image calls, host form == _dev form"""
    n, h, w = covers.shape[:3]
    ctx = B.Context(w, h, slots=slots, lib=lib)
    one = B.Context(w, h, slots=1, lib=lib)
    try:
        got = hist_dev(lib, bufs, ctx, covers, nbins, center, rmin, rmax)
        host = ctx.phase_hist_batch_host(covers, nbins=nbins, center=center, rmin=rmin, rmax=rmax)
        assert np.array_equal(got, host)
        for i in range(n):
            single = one.phase_hist_batch_host(covers[i:i + 1], nbins=nbins, center=center, rmin=rmin, rmax=rmax)
            assert np.array_equal(single[0], got[i]), i
        return got
    finally:
        ctx.close()
        one.close()


# ---- quality ----------------------------------------------------------------------------------------------------------
def gauss11():
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def ssim_ref(a, b):
    """mean SSIM (Wang et al. 2004) of two uint8 planes in fp64: 11 x 11 Gaussian (sigma 1.5), K1 0.01, K2 0.03, L 255, population
    moments, the (W-10)(H-10) windows inside the image"""
    g = gauss11()
    x, y = a.astype(np.float64), b.astype(np.float64)
    H, W = x.shape

    def filt(z):
        hz = sum(g[k] * z[:, k:k + W - 10] for k in range(11))
        return sum(g[k] * hz[k:k + H - 10, :] for k in range(11))

    mx, my = filt(x), filt(y)
    sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    s = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    return float(s.mean())


def perturbed(rgb, seed, amp=3):
    """a stego-like copy: small noise, clamped"""
    rng = np.random.default_rng(seed)
    return np.clip(rgb.astype(np.int32) + rng.integers(-amp, amp + 1, rgb.shape), 0, 255).astype(np.uint8)


def check_quality(lib, bufs, a, b, slots=2):
    """SSE exact, SSIM within 1e-4 of ssim_ref, host == _dev, two calls byte-identical; identical inputs: SSE 0, SSIM exactly 1"""
    n, h, w = a.shape[:3]
    ctx = B.Context(w, h, slots=slots, lib=lib)
    try:
        sse, ssim = ctx.quality_batch_host(a, b)
        sse2, ssim2 = ctx.quality_batch_host(a, b)
        assert sse.tobytes() == sse2.tobytes() and ssim.tobytes() == ssim2.tobytes()
        for i in range(n):
            for p in range(3):
                d = a[i, :, :, p].astype(np.int64) - b[i, :, :, p].astype(np.int64)
                assert int(sse[i, p]) == int((d * d).sum()), (i, p)
                want = ssim_ref(a[i, :, :, p], b[i, :, :, p])
                assert abs(ssim[i, p] - want) <= 1e-4, (w, h, i, p, ssim[i, p], want)
        ai, ap = bufs.put(a)
        bi, bp = bufs.put(b)
        si, sp = bufs.put(np.zeros(n * 3, np.uint64))
        mi, mp = bufs.put(np.zeros(n * 3, np.float64))
        ctx.quality_batch_dev(n, ap, bp, w, h, sp, mp)
        ctx.sync()
        assert np.asarray(bufs.get(si)).reshape(n, 3).tobytes() == sse.tobytes()
        assert np.asarray(bufs.get(mi)).reshape(n, 3).tobytes() == ssim.tobytes()
        same_sse, same_ssim = ctx.quality_batch_host(a, a)
        assert (same_sse == 0).all() and (same_ssim == 1.0).all()
        only_sse, none = ctx.quality_batch_host(a, b, ssim=False)
        assert none is None and np.array_equal(only_sse, sse)
        return sse, ssim
    finally:
        ctx.close()


def check_errors(lib, w=48, h=40):
    import pytest
    ctx = B.Context(w, h, slots=2, lib=lib)
    rgb = cover_rgb(w, h, 0)[None]
    try:
        for nb in (0, 4, 7, 12, 100, 8192):
            with pytest.raises(B.TfftError) as e:
                ctx.phase_hist_batch_host(rgb, nbins=nb)
            assert e.value.status == INVALID, nb
        out = np.zeros(3 * 256, np.uint32)
        big = cover_rgb(w + 1, h, 0)
        for args, want in (((ctx.h, 1, None, w, h, 0, 0.05, 0.45, None, 256, B._ptr(out)), INVALID),
                           ((ctx.h, 1, B._ptr(rgb), w, h, 0, 0.05, 0.45, None, 256, None), INVALID),
                           ((None, 1, B._ptr(rgb), w, h, 0, 0.05, 0.45, None, 256, B._ptr(out)), INVALID),
                           ((ctx.h, 0, B._ptr(rgb), w, h, 0, 0.05, 0.45, None, 256, B._ptr(out)), INVALID),
                           ((ctx.h, -1, B._ptr(rgb), w, h, 0, 0.05, 0.45, None, 256, B._ptr(out)), INVALID),
                           ((ctx.h, 1, B._ptr(big), w + 1, h, 0, 0.05, 0.45, None, 256, B._ptr(out)), TOO_LARGE)):
            assert lib.tfft_phase_hist_batch(*args) == want, args
        sse = np.zeros(3, np.uint64)
        ssim = np.zeros(3, np.float64)
        a = B._ptr(rgb)
        for args, want in (((ctx.h, 1, None, a, w, h, B._ptr(sse), None), INVALID),
                           ((ctx.h, 1, a, None, w, h, B._ptr(sse), None), INVALID),
                           ((ctx.h, 1, a, a, w, h, None, B._ptr(ssim)), INVALID),
                           ((None, 1, a, a, w, h, B._ptr(sse), None), INVALID),
                           ((ctx.h, 0, a, a, w, h, B._ptr(sse), None), INVALID),
                           ((ctx.h, -2, a, a, w, h, B._ptr(sse), None), INVALID),
                           ((ctx.h, 1, B._ptr(big), B._ptr(big), w + 1, h, B._ptr(sse), None), TOO_LARGE)):
            assert lib.tfft_quality_batch(*args) == want, args
        # under 11 pixels: no SSIM, but the SSE
        narrow = cover_rgb(10, h, 1)[None]
        other = perturbed(narrow, 2)
        with pytest.raises(B.TfftError) as e:
            ctx.quality_batch_host(narrow, other)
        assert e.value.status == INVALID
        s, none = ctx.quality_batch_host(narrow, other, ssim=False)
        d = narrow.astype(np.int64) - other.astype(np.int64)
        assert np.array_equal(s[0], (d * d).sum(axis=(1, 2))[0]) and none is None
    finally:
        ctx.close()


def check_slots_after_calls(lib, w=64, h=64, slots=1):
    """a resident single-image forward keeps its answers across a quality call (the call leaves the slots alone), and a histogram call,
    which overwrites the slots' spectra, makes tfft_lowfreq_mag answer TFFT_E_STATE instead of reading another image"""
    import pytest
    a, b = cover_rgb(w, h, 40), cover_rgb(w, h, 41)
    ctx = B.Context(w, h, slots=slots, lib=lib)
    try:
        ctx.forward_rgb8(a)
        m1, med1, cap1 = ctx.lowfreq_mag(4), ctx.medians(), ctx.capacity(0.01 * ctx.medians())
        ctx.quality_batch_host(np.stack([b] * (slots + 1)), np.stack([b] * (slots + 1)))
        assert np.array_equal(ctx.lowfreq_mag(4), m1)
        assert np.array_equal(ctx.medians(), med1) and ctx.capacity(0.01 * med1) == cap1
        ctx.phase_hist_batch_host(b[None])
        with pytest.raises(B.TfftError) as e:
            ctx.lowfreq_mag(4)
        assert e.value.status == -6
    finally:
        ctx.close()


# ---- detector sanity -------------------------------------------------------------------------------------------------
def one_shot_stego(lib, bufs, rgb, payload_len, alpha=0.5, seed=5):
    """a one-shot stego of `rgb` through tfft_embed_stream_batch_dev (shared walk, no jitter); returns (stego, bins of the stream)"""
    h, w = rgb.shape[:2]
    n_bits = 912 + 56 * payload_len
    bins = B.Walk(bytes(range(32)), p2(h), p2(w), lib=lib).next(n_bits)
    rng = np.random.default_rng(seed)
    hdr = make_header(payload_len - 16)[None]
    pay = rng.integers(0, 256, (1, payload_len)).astype(np.uint8)
    ctx = B.Context(w, h, slots=1, lib=lib)
    try:
        ki, kp = bufs.put(np.ascontiguousarray(bins).view(np.uint8).reshape(-1, 8))
        hi, hp = bufs.put(hdr)
        pi, pp = bufs.put(pay)
        ii, ip = bufs.put(rgb[None])
        oi, op = bufs.put(np.zeros((1, h, w, 3), np.uint8))
        ctx.embed_stream_batch_dev(1, ip, w, h, kp, n_bits, hp, pp, payload_len, op, alpha=alpha)
        ctx.sync()
        return np.asarray(bufs.get(oi))[0].copy(), bins
    finally:
        ctx.close()


def check_peak_excess(lib, bufs, rgb, payload_len, nbins=64, alpha=0.5):
    """the two bins holding +-alpha of the stego's 64-bin histogram exceed the cover's by at least half the plane's embedded positions"""
    h, w = rgb.shape[:2]
    stego, bins = one_shot_stego(lib, bufs, rgb, payload_len, alpha)
    ctx = B.Context(w, h, slots=2, lib=lib)
    try:
        hist = ctx.phase_hist_batch_host(np.stack([rgb, stego]), nbins=nbins)
    finally:
        ctx.close()
    pk = A.peak_bins(nbins, alpha)
    assert len(pk) == 2
    per_plane = np.bincount(bins["plane"], minlength=3)
    excess = hist[1][:, pk].sum(axis=1).astype(np.int64) - hist[0][:, pk].sum(axis=1).astype(np.int64)
    for p in range(3):
        assert excess[p] >= 0.5 * per_plane[p], (p, int(excess[p]), int(per_plane[p]))
    return excess / per_plane


def png_read_rgb8(path):
    """(H, W, 3) uint8 of an 8-bit RGB, non-interlaced PNG (what the CLI writes): zlib + the five scanline filters, stdlib and numpy only"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body)
            assert (depth, ctype, interlace) == (8, 2, 0)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    stride = 3 * w
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + stride)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        f, line = raw[y, 0], raw[y, 1:].astype(np.int32)
        if f == 0:
            cur = line
        elif f == 1:
            cur = np.cumsum(line.reshape(w, 3), axis=0).ravel() & 255
        elif f == 2:
            cur = (line + prev) & 255
        else:
            cur = np.zeros(stride, np.int32)
            for i in range(stride):
                a = cur[i - 3] if i >= 3 else 0
                b = prev[i]
                c = prev[i - 3] if i >= 3 else 0
                if f == 3:
                    pred = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (line[i] + pred) & 255
        out[y] = cur
        prev = cur.astype(np.int32)
    return out.reshape(h, w, 3)
