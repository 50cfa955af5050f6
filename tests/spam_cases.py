"""SPAM co-occurrence counts on the device (tfft_spam_batch[_dev]), written once and run twice: on the CPU-emulated
build of the kernel sources (tests/test_emulated_spam.py) and on the MI355X (tests/test_gpu_spam.py, -m gpu).

The reference is a numpy restatement of the definition -- a direct gather of the four pixels of every triple, not a port of the kernel --
and everything is integer arithmetic, so the device counts are held to it with == and no tolerance."""
import numpy as np

from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

DIRS = ((0, 1), (1, 0), (1, 1), (1, -1))      # right, down, down-right, down-left
INVALID, TOO_LARGE = -1, -3
# the kernel's tile (tfft_kernels.h): a workgroup counts TILE_COLS pixel columns, TILE_ROWS rows at a time, with a 3-pixel halo
TILE_COLS, TILE_ROWS = 256, 13
GUARD = 64                                      # guard words before and after the output of a _dev call
GUARD_WORD = 0xA5C3F00D


def n3(t):
    return (2 * t + 1) ** 3


def ref_counts(rgb, t=3):
    """(3, 4, n^3) int64 of one (H, W, 3) uint8 image: for every p with p + 3d inside, the clamped differences along d"""
    h, w = rgb.shape[:2]
    n = 2 * t + 1
    out = np.zeros((3, 4, n ** 3), np.int64)
    img = rgb.astype(np.int32)
    for k, (dy, dx) in enumerate(DIRS):
        y0, y1 = 0, h - 3 * dy                                                     # the p = (y, x) with p + 3d inside: y0 <= y < y1,
        x0, x1 = max(0, -3 * dx), w - max(0, 3 * dx)                               # x0 <= x < x1
        if y1 <= y0 or x1 <= x0:
            continue
        px = [img[y0 + j * dy:y1 + j * dy, x0 + j * dx:x1 + j * dx, :] for j in range(4)]      # I[p + j d]: (rows, cols, 3) each
        e = [np.clip(px[j] - px[j + 1], -t, t) + t for j in range(3)]
        idx = (e[0] * n + e[1]) * n + e[2]
        for p in range(3):
            out[p, k] = np.bincount(idx[:, :, p].ravel(), minlength=n ** 3)
    return out


def dir_totals(w, h):
    return [max(0, h - 3 * abs(dy)) * max(0, w - 3 * abs(dx)) for (dy, dx) in DIRS]


# ---- contents
def flat(w, h, v=97):
    return np.full((h, w, 3), v, np.uint8)


def checker(w, h, kind="checker"):
    """0 / 255 checkerboard, or its column / row stripe form; the planes start on different colours"""
    yy, xx = np.mgrid[0:h, 0:w]
    s = {"checker": yy + xx, "cols": xx, "rows": yy}[kind]
    return np.stack([np.where((s + p) & 1, 255, 0) for p in range(3)], axis=2).astype(np.uint8)


def single_bright(w, h):
    img = np.full((h, w, 3), 10, np.uint8)
    img[h // 2, w // 2, :] = (255, 12, 9)
    return img


def contents(w, h, seed=0):
    return {"cover": cover_rgb(w, h, seed), "flat": flat(w, h), "checker": checker(w, h), "cols": checker(w, h, "cols"),
            "rows": checker(w, h, "rows"), "bright": single_bright(w, h)}


# ---- calls
def spam_dev(bufs, ctx, imgs, t=3):
    """the _dev form into an output with guard words on both sides, which must come back untouched"""
    n, h, w = imgs.shape[:3]
    words = n * 12 * n3(t)
    ii, ip = bufs.put(imgs)
    fill = np.full(words + 2 * GUARD, GUARD_WORD, np.uint32)
    oi, op = bufs.put(fill)
    ctx.spam_batch_dev(n, ip, w, h, op + 4 * GUARD, t=t)
    ctx.sync()
    got = np.asarray(bufs.get(oi)).copy()
    assert (got[:GUARD] == GUARD_WORD).all() and (got[-GUARD:] == GUARD_WORD).all(), "guard words overwritten"
    return got[GUARD:-GUARD].reshape(n, 3, 4, n3(t))


def check_counts(got, imgs, t=3, tag=""):
    n, h, w = imgs.shape[:3]
    assert got.shape == (n, 3, 4, n3(t)) and got.dtype == np.uint32, (tag, got.shape, got.dtype)
    for i in range(n):
        want = ref_counts(imgs[i], t)
        assert want.sum(axis=2).tolist() == [dir_totals(w, h)] * 3, (tag, "reference totals")
        assert got[i].sum(axis=2, dtype=np.int64).tolist() == [dir_totals(w, h)] * 3, (tag, i, "totals")
        assert np.array_equal(got[i].astype(np.int64), want), (tag, i)


def check_images(lib, bufs, imgs, t=3, slots=1, tag="", repeat=False):
    """host form and _dev form against the reference, equal to each other"""
    n, h, w = imgs.shape[:3]
    ctx = B.Context(w, h, slots=slots, lib=lib)
    try:
        host = ctx.spam_batch_host(imgs, t=t)
        check_counts(host, imgs, t, (tag, "host"))
        dev = spam_dev(bufs, ctx, imgs, t)
        assert dev.tobytes() == host.tobytes(), (tag, "dev != host")
        if repeat:
            assert spam_dev(bufs, ctx, imgs, t).tobytes() == dev.tobytes() and ctx.spam_batch_host(imgs, t=t).tobytes() == host.tobytes(), tag
        return host
    finally:
        ctx.close()


def check_shape(lib, bufs, w, h, t=3, seed=0):
    """every content of one shape, as one batch (the images then start at every byte alignment the shape allows)"""
    c = contents(w, h, seed)
    imgs = np.stack([c[k] for k in sorted(c)])
    got = check_images(lib, bufs, imgs, t, slots=2, tag=(w, h, t))
    names = sorted(c)
    centre = (t * (2 * t + 1) + t) * (2 * t + 1) + t
    f = got[names.index("flat")]
    assert f[:, :, centre].tolist() == [dir_totals(w, h)] * 3, (w, h, "flat: everything in (0,0,0)")
    lo, hi = 0, n3(t) - 1                       # (-T,-T,-T) and (+T,+T,+T); the alternating corners (-T,+T,-T), (+T,-T,+T):
    n = 2 * t + 1
    alt = ((0 * n + (n - 1)) * n + 0, ((n - 1) * n + 0) * n + (n - 1))
    ck = got[names.index("checker")]
    for k, tot in enumerate(dir_totals(w, h)):
        if k < 2:                               # neighbours along a row or a column alternate: both signs of the clamped corner
            assert (ck[:, k, alt[0]].astype(np.int64) + ck[:, k, alt[1]] == tot).all(), (w, h, k)
            if tot > 1:
                assert (ck[:, k, alt[0]] > 0).all() and (ck[:, k, alt[1]] > 0).all(), (w, h, k)
        else:                                   # a diagonal of a checkerboard is flat
            assert (ck[:, k, centre] == tot).all(), (w, h, k)
    assert lo != centre and hi != centre
    return got


def check_batch_equals_singles(lib, bufs, imgs, slots, t=3):
    """image i of a batch (which starts at byte i*w*h*3: odd and unaligned for odd sizes) counts as it does alone; any slot count"""
    n, h, w = imgs.shape[:3]
    got = check_images(lib, bufs, imgs, t, slots=slots, tag=("batch", w, h, slots))
    one = B.Context(w, h, slots=1, lib=lib)
    try:
        for i in range(n):
            single = one.spam_batch_host(imgs[i:i + 1], t=t)
            assert single[0].tobytes() == got[i].tobytes(), (w, h, slots, i)
            assert spam_dev(bufs, one, imgs[i:i + 1], t)[0].tobytes() == got[i].tobytes(), (w, h, slots, i)
    finally:
        one.close()
    return got


def check_errors(lib, w=48, h=40):
    import pytest
    ctx = B.Context(w, h, slots=2, lib=lib)
    rgb = cover_rgb(w, h, 0)[None]
    big_w, big_h = cover_rgb(w + 1, h, 0)[None], cover_rgb(w, h + 1, 0)[None]
    out = np.zeros(12 * n3(4), np.uint32)
    try:
        for t in (0, 5, -1, 100):
            with pytest.raises(B.TfftError) as e:
                ctx.spam_batch_host(rgb, t=t)
            assert e.value.status == INVALID, t
        r, o = B._ptr(rgb), B._ptr(out)
        for fn in (lib.tfft_spam_batch, lib.tfft_spam_batch_dev):
            for args, want in (((ctx.h, 1, r, w, h, 0, o), INVALID), ((ctx.h, 1, r, w, h, 5, o), INVALID),
                               ((ctx.h, 0, r, w, h, 3, o), INVALID), ((ctx.h, -1, r, w, h, 3, o), INVALID),
                               ((ctx.h, 1, r, 0, h, 3, o), INVALID), ((ctx.h, 1, r, w, 0, 3, o), INVALID),
                               ((ctx.h, 1, r, -4, h, 3, o), INVALID),
                               ((ctx.h, 1, None, w, h, 3, o), INVALID), ((ctx.h, 1, r, w, h, 3, None), INVALID),
                               ((None, 1, r, w, h, 3, o), INVALID),
                               ((ctx.h, 1, B._ptr(big_w), w + 1, h, 3, o), TOO_LARGE), ((ctx.h, 1, B._ptr(big_h), w, h + 1, 3, o), TOO_LARGE)):
                assert fn(*args) == want, (fn, args)
        assert (out == 0).all()                  # a refused call writes nothing
    finally:
        ctx.close()


def check_slots_after_spam(lib, bufs, w=64, h=64, slots=1):
    """a resident single-image forward keeps its answers across both forms of the call: the call leaves the slots alone"""
    a, b = cover_rgb(w, h, 40), cover_rgb(w, h, 41)
    ctx = B.Context(w, h, slots=slots, lib=lib)
    try:
        ctx.forward_rgb8(a)
        m1, med1, cap1 = ctx.lowfreq_mag(4), ctx.medians(), ctx.capacity(0.01 * ctx.medians())
        batch = np.stack([b] * (slots + 1))
        host = ctx.spam_batch_host(batch)
        dev = spam_dev(bufs, ctx, batch)
        assert host.tobytes() == dev.tobytes()
        assert np.array_equal(ctx.lowfreq_mag(4), m1)
        assert np.array_equal(ctx.medians(), med1) and ctx.capacity(0.01 * med1) == cap1
    finally:
        ctx.close()
