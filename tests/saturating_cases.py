"""The quality and channel kernels (k_quality, k_channel_awgn, k_channel_jpeg; DESIGN.md sections 12 and 13) where they clamp and where
tiles end, written once and run twice: on the CPU-emulated build (tests/test_emulated_saturating.py) and on the MI355X
(tests/test_gpu_saturating.py, -m gpu).  The checks, references and bars are those of tests/analysis_cases.py and tests/robust_cases.py,
unchanged; what is new here is the input: the synthetic covers of those files stay within bytes 56..199, so no output of theirs meets a
clamp, and their GPU shapes are multiples of the quality kernel's 64-window tile.
  channels  AWGN and JPEG on contents that reach 0 and 255 (saturating), with conditions on the fp64 reference alone that keep the clamp
            exercised (check_awgn_saturating, check_jpeg_saturating)
  quality   SSE exact and SSIM within 1e-4 on pairs of such contents (saturating_pair), an SSE beyond 2^32, and SSIM within 2e-6 on pairs
            and shapes made so that one row or column of windows lost at a tile edge shows (check_quality_tiles)"""
import numpy as np

import analysis_cases as AC
import robust_cases as RC
from steganosaurus_amd import binding as B

SATURATING = ("full", "sat", "edges", "primaries8", "white", "black")
# 3 images in 2 slots: 3 * 101 * 37 is odd (images start at odd byte offsets); 259 = 256 + 3: a second strip of three columns whose one block is
# completed from column 258, 3 * 259 mod 4 = 1, 17 = 16 + 1: a last block row with one live row; 5 x 3: less than one block
SATURATING_SHAPES = [(101, 37), (259, 17), (5, 3)]


def saturating(kind, w, h, seed=0):
    """one (H, W, 3) uint8 image: full = uniform 0..255; sat = 0 or 255, each with probability 1/2; edges = 0..3 or 252..255; primaries8 =
    8 x 8 patches on the JPEG block grid in the eight corner colours of the RGB cube; white / black = flat 255 / 0"""
    rng = np.random.default_rng([SATURATING.index(kind), w, h, seed])
    shape = (h, w, 3)
    if kind == "full":
        x = rng.integers(0, 256, shape)
    elif kind == "sat":
        x = 255 * rng.integers(0, 2, shape)
    elif kind == "edges":
        x = rng.integers(0, 8, shape)
        x = np.where(x < 4, x, x + 248)
    elif kind == "primaries8":
        x = 255 * rng.integers(0, 2, ((h + 7) // 8, (w + 7) // 8, 3))
        x = np.repeat(np.repeat(x, 8, axis=0), 8, axis=1)[:h, :w]
    else:
        x = np.full(shape, {"white": 255, "black": 0}[kind])
    return x.astype(np.uint8)


def saturating_batch(kind, w, h, n=3, seed=0):
    return np.stack([saturating(kind, w, h, seed + i) for i in range(n)])


# ---- channels ----------------------------------------------------------------------------------------------------------
def outside_share(v):
    """the share of a reference's values, before rint and clamp, that only the clamp brings back into 0..255"""
    return float(((v < -0.5) | (v > 255.5)).mean())


def check_awgn_saturating(lib, bufs, kind, w, h, n=3, sigmas=(0.5, 2.0, 8.0), seed=7, slots=2):
    """check_awgn on a saturating content.  A condition on the reference alone keeps the clamp exercised: of white, black, sat and edges at
    least 10 % of the fp64 values lie outside [-0.5, 255.5].  P(g > 1/2sigma) is 15.9 % at sigma 0.5 for a byte on a clamp (white, black,
    sat) and more at a larger sigma.  edges holds its bytes at distances 1/2, 3/2, 5/2, 7/2 from the clamp, a quarter each: 19 % at sigma 2,
    40 % at sigma 8, but (P(g > 1) + P(g > 3)) / 4 = 4.0 % at sigma 0.5, whatever the seed: there the condition is half of that expectation"""
    rgb = saturating_batch(kind, w, h, n)
    for sigma in sigmas:
        if kind != "full":
            share = outside_share(RC.awgn_value(rgb, sigma, seed)[0])
            need = 0.02 if (kind, sigma) == ("edges", 0.5) else 0.10
            print("awgn", (kind, w, h), "sigma", sigma, "outside the clamp %.1f %%" % (100 * share))
            assert share >= need, (kind, w, h, sigma, share)
        out = RC.check_channel_forms(lib, bufs, rgb, ("awgn", sigma, seed), slots)
        RC.check_awgn(out, rgb, sigma, seed, 0, (kind, w, h))


# (content, Q) pairs whose fp64 reference stays inside check_jpeg's two caps at 101 x 37, 259 x 17 and 5 x 3.  sat at Q 90 and 100 is left out:
# the reference alone has 10.4 % and 16.8 % ambiguous blocks at 259 x 17 (cap 1/8)
JPEG_SATURATING = {"full": (30, 75, 90, 100), "sat": (30, 75), "edges": (30, 75, 90, 100), "primaries8": (30, 75, 90, 100),
                   "white": (30, 75, 90, 100), "black": (30, 75, 90, 100)}
# ... and those of them at which the reference itself leaves 0..255, so that only the clamp gives the right byte (>= 10 % of its values
# before the final rint outside [-0.5, 255.5]; 22-100 % here).  Not white and primaries8 at Q 75 and 90: their blocks are flat, the only
# coefficient is DC = 8 * 127 = 1016 per saturated component, which the Q 75 step 8 divides (255 exactly) and the Q 90 step 3 takes to
# 1017 (255.125, inside); not Q 100 (step 1: under 4 % of edges); not full (10 % at most) and black (0 stays 0)
JPEG_CLAMPS = {"white": (30,), "primaries8": (30,), "sat": (30, 75), "edges": (30, 75, 90)}


def check_jpeg_saturating(lib, bufs, kind, w, h, n=3, slots=2):
    rgb = saturating_batch(kind, w, h, n)
    for q in JPEG_SATURATING[kind]:
        if q in JPEG_CLAMPS.get(kind, ()):
            share = float(np.mean([outside_share(RC.jpeg_ref(rgb[i], q)[0]) for i in range(n)]))
            print("jpeg", (kind, w, h), "Q", q, "outside the clamp %.1f %%" % (100 * share))
            assert share >= 0.10, (kind, w, h, q, share)
        out = RC.check_channel_forms(lib, bufs, rgb, ("jpeg", q), slots)
        RC.check_jpeg(out, rgb, q, (kind, w, h))


# ---- quality -----------------------------------------------------------------------------------------------------------
# Pairs that reach 0 and 255, where the kernel's x - 128 is +-127 / -128 and acc2 - acc0 * acc0 cancels most
SATURATING_PAIRS = ("flat", "edges", "bright", "sat", "full")


def saturating_pair(kind, w, h, n=3):
    """(a, b) of n images each.  flat: 255 vs 254, 255 vs 0 and 0 vs 1, one pair per image; edges, full: the content under two seeds;
    bright: noise in 252..255 vs other such noise (images 0 and 2), 0..3 vs other 0..3 (image 1) -- means at either end, variances of about
    1; sat: b is a with 10 % of the bytes taken to the other end"""
    if kind == "flat":
        assert n == 3
        return tuple(np.stack([np.full((h, w, 3), v[k], np.uint8) for v in ((255, 254), (255, 0), (0, 1))]) for k in (0, 1))
    if kind in ("edges", "full"):
        return saturating_batch(kind, w, h, n), saturating_batch(kind, w, h, n, seed=100)
    rng = np.random.default_rng([SATURATING_PAIRS.index(kind), w, h])
    if kind == "bright":
        lo_a, lo_b = (rng.integers(0, 4, (n, h, w, 3)) for _ in range(2))
        top = np.array([252, 0, 252][:n]).reshape(-1, 1, 1, 1)
        return (top + lo_a).astype(np.uint8), (top + lo_b).astype(np.uint8)
    a = saturating_batch("sat", w, h, n)
    return a, np.where(rng.random(a.shape) < 0.1, 255 - a, a).astype(np.uint8)


def check_quality_pair(lib, bufs, a, b, slots=2):
    """analysis_cases.check_quality (SSE exact, SSIM within 1e-4, host == _dev, repeat calls identical), the worst SSIM error printed"""
    sse, ssim = AC.check_quality(lib, bufs, a, b, slots=slots)
    n, h, w = a.shape[:3]
    want = np.array([[AC.ssim_ref(a[i, :, :, p], b[i, :, :, p]) for p in range(3)] for i in range(n)])
    print("quality", (w, h, n), "worst |SSIM - fp64| %.3e" % np.abs(ssim - want).max())
    return sse, ssim


def check_quality_sse_wide(lib, w=300, h=300):
    """flat 255 vs flat 0: 255^2 w h = 5.85e9 per plane at 300 x 300, over 2^32 -- a 32-bit sum anywhere on either kernel's path shows"""
    a, b = np.full((1, h, w, 3), 255, np.uint8), np.zeros((1, h, w, 3), np.uint8)
    want = 255 * 255 * w * h
    assert want > 2 ** 32
    ctx = B.Context(w, h, slots=1, lib=lib)
    try:
        for with_ssim in (False, True):
            sse, _ = ctx.quality_batch_host(a, b, ssim=with_ssim)
            assert [int(v) for v in sse[0]] == [want] * 3, (with_ssim, sse.tolist(), want)
    finally:
        ctx.close()


def ssim_map(a, b):
    """the (H-10, W-10) fp64 SSIM of every window: analysis_cases.ssim_ref before its mean (check_quality_tiles holds the two together)"""
    g = AC.gauss11()
    x, y = a.astype(np.float64), b.astype(np.float64)
    H, W = x.shape

    def filt(z):
        hz = sum(g[k] * z[:, k:k + W - 10] for k in range(11))
        return sum(g[k] * hz[k:k + H - 10, :] for k in range(11))

    mx, my = filt(x), filt(y)
    sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    return ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))


def tile_pairs(w, h):
    """a = full; two b: every byte of a replaced by a fresh random byte with probability f(x, y), f1 = 0.05 + 0.9 (u + v)/2 and
    f2 = 0.05 + 0.9 (u^2 + v^2)/2, u = x/(W-1), v = y/(H-1): the SSIM falls from the top left to the bottom right, and the two profiles
    cross their means at different places, so that no row or column of windows is average in both"""
    rng = np.random.default_rng(w * 1000 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = xx / (w - 1), yy / (h - 1)
    a = saturating("full", w, h)
    bs = []
    for f in (0.05 + 0.9 * (u + v) / 2, 0.05 + 0.9 * (u * u + v * v) / 2):
        fresh = rng.integers(0, 256, a.shape).astype(np.uint8)
        bs.append(np.where(rng.random(a.shape) < f[..., None], fresh, a).astype(np.uint8))
    return np.stack([a, a]), np.stack(bs)


TILE_BAR = 2e-6
# tiles are 64 x 32 windows: the second tile column and row own pixels but no window (74 x 42), one window column / row (75 x 43), eleven: the
# whole halo read across the boundary (85 x 53); three tile columns and rows, the last with one window column / row and 11 pixels (139 x 75)
TILE_SHAPES = [(74, 42), (75, 43), (85, 53), (139, 75)]


def check_quality_tiles(lib, bufs, w, h):
    """check_quality on tile_pairs, and the mean SSIM per plane within TILE_BAR of ssim_ref.  The bar is fp32 rounding, not a measurement:
    in every window of these pairs sx + sy + C2 is several thousand, the fp32 error of the moments a few ulps of 16384 (4e-3), under 1e-6
    of it, and the ratio adds a few 6e-8.  It sees one row or column of windows, a condition asserted on the fp64 map m alone: column j of
    windows replaced by average ones moves a plane's mean by |mean(m[:, j]) - mean(m)| / (W-10), and for every j that is at least ten
    bars in one of the two pairs and three planes; the same for every row with H-10"""
    a, b = tile_pairs(w, h)
    col, row = np.zeros((2, 3, w - 10)), np.zeros((2, 3, h - 10))
    want = np.zeros((2, 3))
    for k in range(2):
        for p in range(3):
            m = ssim_map(a[k, :, :, p], b[k, :, :, p])
            want[k, p] = AC.ssim_ref(a[k, :, :, p], b[k, :, :, p])
            assert abs(m.mean() - want[k, p]) <= 1e-14, (w, h, k, p, "the map is not ssim_ref's")
            col[k, p] = np.abs(m.mean(axis=0) - m.mean()) / (w - 10)
            row[k, p] = np.abs(m.mean(axis=1) - m.mean()) / (h - 10)
    col, row = col.max(axis=(0, 1)), row.max(axis=(0, 1))
    print("tiles", (w, h), "least column %.2e, least row %.2e (x TILE_BAR: %.1f, %.1f)" % (col.min(), row.min(), col.min() / TILE_BAR, row.min() / TILE_BAR))
    assert col.min() >= 10 * TILE_BAR and row.min() >= 10 * TILE_BAR, (w, h, col.min(), row.min())
    sse, ssim = AC.check_quality(lib, bufs, a, b, slots=1)
    print("tiles", (w, h), "worst |SSIM - fp64| %.3e" % np.abs(ssim - want).max())
    assert np.abs(ssim - want).max() <= TILE_BAR, (w, h, ssim.tolist(), want.tolist())
