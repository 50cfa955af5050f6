"""The batched pipelines on whole-plane, hand-built bin lists, written once and run twice: on the CPU-emulated build of the kernel
sources (tests/test_emulated_bin_lists.py, HostBufs: index math only) and on the MI355X (tests/test_gpu_bin_lists.py, TorchBufs).

Every other list the suite sends through the bucketed column kernels (k_fft_cols<COLS_READ | COLS_EMBED | COLS_EMIT | COLS_STAT>,
k_bucket_*, k_bins_last_row) is a turtle walk: a local random walk that touches a few percent of the plane in one contiguous block of
tiles.  What those kernels do depends on where the bins are and how many share a bucket, so the lists here are built by hand:

    dense_left / dense_right / dense_mixed   for every plane and every stored bin 1 <= x < PW/2, y not in {0, PH/2}: exactly one of the
                        bin and its mirror ((PH - y) % PH, PW - x) -- all from x < PW/2, all from x > PW/2 (every entry is read through
                        the conjugate of tile_bin_of), or a seeded coin per bin.  Every (plane, row group, tile) bucket is full.
    frame               all bins with y in {1, PH/2 - 1, PH/2 + 1, PH - 1} or x in {1, PW/2 - 1, PW/2 + 1, PW - 1}, one of each mirror pair
    tiles_first / tiles_last / tiles_alternate / tiles_first2_last
                        dense_mixed inside the named 16-column tiles of the stored half (the first, the last, the even ones, the first
                        two and the last), nothing elsewhere: the has_bins / "fetch this tile again" / stored-as-zeros paths
    low_rows            y = 1, x < PW/2 only: the last stored row (COLS_ROWLIMIT, k_bins_last_row) is 1
    low_rows_mirror     y = 1, x > PW/2 only: the last stored row is PH - 1, through mirror bins alone
    single              the one bin (2, PH - 1, PW - 1)
All in a seeded random order (the walks check also takes one in address order).  build_list asserts what a list must be before any
device work: every bin off the excluded axes, all (plane, y, x) distinct, no bin's mirror in the list.

The reference is ref_embed / ref_read below: numpy fp64 from the formulas of include/turtlefft_hip.h (write_bit_on_bin per listed bin
and its conjugate at the mirror, the oracle's fft2d inverse, crop, round half away from zero, clamp) for ANY list -- the oracle's own
embed only walks.  An empty list returns the cover (check_builders).

Rows: one small cover per plan, asserted with PM.assert_plan first.  L = 2^log_n2 is the length of the last forward column step, a
bucket is one (plane, row group g of G, 16-column tile) and holds up to 16 * L entries of which NE * T * 16 travel in registers (T = L / 16
threads per column, NE = 2, or 4 at L = 512); the rest is fetched by the `e0 + em_tid + NE * em_nthr` loops of COLS_EMBED, COLS_READ and
COLS_EMIT.  Dense lists fill every bucket, so those loops run at every L of the table (bucket_table computes the figures below from
the lists and check_builders asserts "largest bucket > registers" for every dense and tiles list):

    row          cover      grid       plan                      G   lists (length)                                                largest bucket / NE*T*16
    p2_direct    64x64      64x64      direct, L = 64            1   dense x3 (5766), frame (720), tiles first / last / alternate        992 / 128
                                                                     (2790 / 2976 / 2790), tiles_first2_last (5766: two tiles in all),
                                                                     low_rows, low_rows_mirror (93), single (1)
    d_L4         40x12      64x16      direct, L = 16            1   dense x3 (1302), frame (432), single                                224 / 32
    n_M8         12x40      16x64      direct, L = 64, M = 8     1   dense x3 (1302), frame (432), single                                434 / 128
    p2_two_step  32x512     32x512     two-step (4,5), M = 16    16  dense x3 (22950), frame (3216), low_rows, low_rows_mirror (45)      480 / 64
    ts_pad       40x300     64x512     two-step (4,5), padded    16  dense_mixed (47430), tiles first / last / alternate                 512 / 64
                                                                     (22950 / 24480 / 22950), tiles_first2_last (47430: two tiles)
    ts_5_6       40x1100    64x2048    two-step (5,6)            32  dense_mixed (190278), frame (12624)                                 1024 / 128
    p2_f2k_4     2048x128   2048x128   fused, 2048 wide, (3,4)   8   dense x3 (386694), tiles first / last / alternate / first2_last     256 / 32
                                                                     (5670 / 6048 / 193158 / 17766), frame (13008)
    f2k_6x2      1030x300   2048x512   fused (3,6), 2 / launch   8   dense_mixed (1565190), tiles_alternate (781830)                     1024 / 128
    f4k_4        2050x70    4096x128   fused, 4096 wide, (3,4)   8   dense_mixed (773766)                                                256 / 32
    f2k_9        1030x2100  2048x4096  fused (3,9), L = 512      8   tiles_first2_last (577254)                                          8192 / 2048
(NE * T * 16 is the same for the read and the embed side at every L of the table.)  The per-image check adds, on p2_direct, p2_two_step,
ts_pad and p2_f2k_4, three dense lists of the row's dense length, one per image.
The issue's p2_f2k_4 cover, 2048x16, pads to 16 rows and takes the direct plan (L = 16): 2048x128 is the smallest power-of-two cover
on the fused (3,4) plan -- the grid PM.ROWS' f2k_4 (1030x70) pads to, unpadded, so that header and payload round-trip.

Covers: cover_rgb(w, h, 70 + i), slots + 1 images per call (two chunks).  p2_direct and ts_pad also run with a saturating first cover
(half 0, half 255, a band of 254, isolated 1s, a noisy quarter): more than a tenth of the reference stego's pixels sit on the clamp.

Bars: nothing new.  Stego within 1 LSB of the fp64 reference on fewer than PM.lsb_frac_of(row) of the pixels; the sorted list with its
bit index, the in-place call and the host form give the default call's bytes; TFFT_EMBED_DELTA=0 within 1 LSB of it; usable_out does
not depend on the list or the statistics variant; extraction of the reference's stego equals orc.read_bins but where the reference's
own value has |Im| < 1e-5 |v| -- at most max(3, n / 20000) positions of a list, which the reference alone is held to first."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import parity_cases as PC
import plan_matrix_cases as PM
import walks_cases as WC
from phase_cases import _phase_near_boundary
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

DENSE = ("dense_left", "dense_right", "dense_mixed")
TILES = ("tiles_first", "tiles_last", "tiles_alternate", "tiles_first2_last")
LOWS = ("low_rows", "low_rows_mirror")
ALL_KINDS = DENSE + ("frame",) + TILES + LOWS + ("single",)


def row(name, w, h, kind, log_n1, log_n2, lists, slots=1, emu=True, walks=False, sat=(), host=False):
    """lists: the kinds of the shared-list checks; emu: the emulator affords the row (tests/test_emulated_bin_lists.py has the times);
    walks: the per-image check runs here; sat: the kinds that also run with the saturating cover; host: the host-buffer forms"""
    return dict(name=name, w=w, h=h, kind=kind, log_n1=log_n1, log_n2=log_n2, lists=tuple(lists), slots=slots, emu=emu, walks=walks,
                sat=tuple(sat), host=host, env={})


ROWS = [
    row("p2_direct", 64, 64, "direct", 0, 6, ALL_KINDS, walks=True, sat=("dense_mixed", "frame"), host=True),
    row("d_L4", 40, 12, "direct", 0, 4, DENSE + ("frame", "single")),
    row("n_M8", 12, 40, "direct", 0, 6, DENSE + ("frame", "single")),
    row("p2_two_step", 32, 512, "two_step", 4, 5, DENSE + ("frame",) + LOWS, walks=True),
    row("ts_pad", 40, 300, "two_step", 4, 5, ("dense_mixed",) + TILES, walks=True, sat=("dense_mixed",)),
    row("ts_5_6", 40, 1100, "two_step", 5, 6, ("dense_mixed", "frame"), emu=False),
    row("p2_f2k_4", 2048, 128, "fused", 3, 4, DENSE + TILES + ("frame",), walks=True),
    row("f2k_6x2", 1030, 300, "fused", 3, 6, ("dense_mixed", "tiles_alternate"), slots=2, emu=False),
    row("f4k_4", 2050, 70, "fused", 3, 4, ("dense_mixed",), slots=2, emu=False),
    row("f2k_9", 1030, 2100, "fused", 3, 9, ("tiles_first2_last",), emu=False),
]
BY_NAME = {r["name"]: r for r in ROWS}


def rows(emulated=False, walks=False, host=False):
    return [r for r in ROWS if (r["emu"] or not emulated) and (r["walks"] or not walks) and (r["host"] or not host)]


def shared_cases(emulated=False):
    """(row, list kind, saturating cover?) of the shared-list check"""
    out = []
    for r in rows(emulated):
        out += [(r, k, False) for k in r["lists"]] + [(r, k, True) for k in r["sat"]]
    return out


def case_id(c):
    return "%s-%s%s" % (c[0]["name"], c[1], "-saturating" if c[2] else "")


# ---- list builders (host) ------------------------------------------------------------------------------------------------------------
def _seed(kind, ph, pw, salt=0):
    return [ALL_KINDS.index(kind), ph, pw, salt]


def tiles_of(which, ntiles):
    return {"first": [0], "last": [ntiles - 1], "alternate": list(range(0, ntiles, 2)), "first2_last": sorted({0, min(1, ntiles - 1), ntiles - 1})}[which]


def assert_valid(bins, ph, pw):
    """what a list handed to embed / extract must be: off the excluded axes, distinct, no bin's mirror in the list"""
    p, y, x = (bins[f].astype(np.int64) for f in ("plane", "y", "x"))
    assert len(bins) > 0
    assert (p <= 2).all() and (y > 0).all() and (y < ph).all() and (x > 0).all() and (x < pw).all(), "inside the grid, off y = 0 and x = 0"
    assert (2 * y != ph).all() and (2 * x != pw).all(), "off y = PH/2 and x = PW/2"
    key = (p * ph + y) * pw + x
    mkey = (p * ph + (ph - y) % ph) * pw + (pw - x)
    assert len(np.unique(key)) == len(key), "distinct bins"
    assert not np.isin(mkey, key).any(), "no bin's mirror is in the list"


def build_list(kind, ph, pw, salt=0, order="shuffled"):
    """the list `kind` on a PH x PW grid as tfft_bin records; salt: another coin and another order of the same kind"""
    m = pw // 2
    rng = np.random.default_rng(_seed(kind, ph, pw, salt))
    if kind == "single":
        t = np.array([[2, ph - 1, pw - 1]])
    else:
        ys = np.array([y for y in range(1, ph) if 2 * y != ph])
        P, Y, X = (a.ravel() for a in np.meshgrid(np.arange(3), ys, np.arange(1, m), indexing="ij"))      # the stored bins, one per mirror pair
        coin = rng.integers(0, 2, len(P)).astype(bool)
        if kind == "dense_left":
            keep, mirror = np.ones(len(P), bool), np.zeros(len(P), bool)
        elif kind == "dense_right":
            keep, mirror = np.ones(len(P), bool), np.ones(len(P), bool)
        elif kind == "dense_mixed":
            keep, mirror = np.ones(len(P), bool), coin
        elif kind == "frame":       # (the frame is closed under the mirror: rows 1 <-> PH-1, PH/2-1 <-> PH/2+1, columns 1 <-> PW-1, PW/2-1 <-> PW/2+1)
            keep, mirror = np.isin(Y, [1, ph // 2 - 1, ph // 2 + 1, ph - 1]) | np.isin(X, [1, m - 1]), coin
        elif kind.startswith("tiles_"):
            keep, mirror = np.isin(X >> 4, tiles_of(kind[6:], (m + 15) // 16)), coin
        elif kind == "low_rows":
            keep, mirror = Y == 1, np.zeros(len(P), bool)
        elif kind == "low_rows_mirror":     # walk row 1 right of PW/2 = stored row PH - 1
            keep, mirror = Y == ph - 1, np.ones(len(P), bool)
        else:
            raise KeyError(kind)
        P, Y, X, mirror = P[keep], Y[keep], X[keep], mirror[keep]
        t = np.stack([P, np.where(mirror, ph - Y, Y), np.where(mirror, pw - X, X)], axis=1)
    if order == "shuffled":
        t = t[rng.permutation(len(t))]
    else:       # address order: (plane, y, x)
        t = t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]
    bins = B.make_bins(t)
    assert_valid(bins, ph, pw)
    x, y = bins["x"].astype(np.int64), bins["y"].astype(np.int64)
    if kind == "dense_left" or kind == "low_rows":
        assert (x < m).all()
    if kind == "dense_right" or kind == "low_rows_mirror":
        assert (x > m).all()
    if kind in ("dense_mixed", "frame") or kind.startswith("tiles_"):
        assert (x < m).any() and (x > m).any()
    if kind in LOWS:
        assert (y == 1).all() and stored_rows(bins, ph, pw).max() == (1 if kind == "low_rows" else ph - 1)
    if kind == "frame":
        assert set(np.unique(y)) >= {1, ph // 2 - 1, ph // 2 + 1, ph - 1} and set(np.unique(x)) >= {1, m - 1, m + 1, pw - 1}
    return bins


def stored_rows(bins, ph, pw):
    return np.where(bins["x"] > pw // 2, (ph - bins["y"].astype(np.int64)) % ph, bins["y"].astype(np.int64))


def bucket_lengths(r, bins):
    """entries per (plane, row group, tile) bucket, as tile_bin_of assigns them"""
    ph, pw = PM.grid_of(r)
    m, g = pw // 2, (1 if r["kind"] == "direct" else 1 << r["log_n1"])
    ntiles = (m + 15) // 16
    x = bins["x"].astype(np.int64)
    sx, sy = np.where(x > m, pw - x, x), stored_rows(bins, ph, pw)
    return np.bincount((bins["plane"].astype(np.int64) * g + sy % g) * ntiles + (sx >> 4), minlength=3 * g * ntiles)


def registers(r, embed=False):
    """NE * T * 16: the bucket entries a workgroup of the last forward step (embed: of the first inverse step) holds in registers"""
    ln = 1 << r["log_n2"]
    ne = (4 if r["log_n2"] == 9 else 2) if embed else (4 if r["log_n2"] >= 9 else 2)
    return ne * (ln // min(16, ln)) * 16


def bucket_table(r):
    ph, pw = PM.grid_of(r)
    out = []
    for kind in r["lists"]:
        bl = bucket_lengths(r, build_list(kind, ph, pw))
        out.append((kind, int(bl.sum()), int(bl.max()), int((bl == 0).sum()), len(bl)))
    return out


# ---- covers ---------------------------------------------------------------------------------------------------------------------------
def saturating_cover(w, h, seed=90):
    """half 0, half 255, a band of 254, isolated 1s and a noisy quarter: the clamp of the inverse is at work on a large part of the stego"""
    img = np.zeros((h, w, 3), np.uint8)
    img[h // 2:] = 255
    img[h // 2 + h // 8: h // 2 + h // 8 + max(1, h // 16)] = 254
    img[1:h // 2:3, 2::5] = 1
    img[h // 2:, w // 2:] = cover_rgb(w, h, seed)[h // 2:, w // 2:]
    return img


def covers_of(r, n, sat=False):
    c = np.stack([cover_rgb(r["w"], r["h"], 70 + i) for i in range(n)])
    if sat:
        c[0] = saturating_cover(r["w"], r["h"])
    return c


def _pmap(fn, items):
    """fn over items on one thread each: the oracle's transforms are C calls (no GIL), and at 2048 x 4096 they are the test's time"""
    items = list(items)
    with ThreadPoolExecutor(max_workers=max(1, len(items))) as ex:
        return list(ex.map(fn, items))


# ---- the numpy fp64 reference for an arbitrary list -------------------------------------------------------------------------------------
_SPECTRA = {}       # cover bytes -> (spectrum, medians) of the oracle's forward transform, read-only; small grids only


def ref_spectrum(orc, cover):
    key = (cover.shape, cover.tobytes())
    if key not in _SPECTRA:
        spec, med = orc.forward_rgb8(cover)
        if spec.nbytes > (32 << 20):
            return spec, med
        spec.setflags(write=False)
        if len(_SPECTRA) >= 8:
            _SPECTRA.pop(next(iter(_SPECTRA)))
        _SPECTRA[key] = (spec, med)
    return _SPECTRA[key]


def ref_embed(orc, cover, bins, bits, alpha=0.5, jitter=None, adaptive=False):
    """write_bit_on_bin (turtlefft_hip.h: S:712-732, S:704-710) over `bins`, then the inverse side (S:1100-1103), in fp64"""
    spec, med = ref_spectrum(orc, cover)
    h, w = cover.shape[:2]
    ph, pw = spec.shape[1:]
    F = np.array(spec)
    if len(bins):
        p, y, x = (bins[f].astype(np.int64) for f in ("plane", "y", "x"))
        mag = np.maximum(1e-12, np.abs(F[p, y, x]))
        a = alpha * np.clip(mag / np.maximum(1e-12, med[p]), 0.5, 2.0) if adaptive else alpha
        theta = np.where(np.asarray(bits) != 0, a, -a) + (np.asarray(jitter, np.float64) if jitter is not None else 0.0)
        nv = mag * (np.cos(theta) + 1j * np.sin(theta))
        F[p, y, x] = nv
        F[p, (ph - y) % ph, (pw - x) % pw] = np.conj(nv)
    out = np.empty((h, w, 3), np.uint8)
    for pl, z in enumerate(_pmap(lambda f: orc.fft2d(f, inverse=True), F)):
        v = z.real[:h, :w]
        out[:, :, pl] = np.clip(np.sign(v) * np.floor(np.abs(v) + 0.5), 0, 255)       # round half away from zero, clamp
    return out


def ref_read(orc, stego, bins, jitter=None, adaptive=False, alpha=0.5):
    """read_bit_from_bin over `bins` on the oracle's spectrum of `stego`; also the spectrum's values at the bins"""
    spec, med = orc.forward_rgb8(stego)
    t = B.bins_to_triples(bins)
    return orc.read_bins(spec, t, alpha, jitter, adaptive, med), spec[t[:, 0], t[:, 1], t[:, 2]]


def on_decision_line(v):
    """the existing criterion (parity_cases.check_embed_extract): the reference's own decision is a coin flip"""
    return np.abs(v.imag) < 1e-5 * np.abs(v)


# ---- the checks ---------------------------------------------------------------------------------------------------------------------------
def check_builders(lib, orc, r):
    """host only: the plan, every list of the row (build_list asserts its validity), the buckets against the registers, and the
    reference on an empty list"""
    PM.assert_plan(lib, r)
    ph, pw = PM.grid_of(r)
    for kind, n, longest, empty, nb in bucket_table(r):
        print("%-12s %-18s %8d bins, largest bucket %5d (registers: read %d, embed %d), empty buckets %d / %d"
              % (r["name"], kind, n, longest, registers(r), registers(r, True), empty, nb))
        if kind in DENSE or kind.startswith("tiles_"):
            assert longest > max(registers(r), registers(r, True)), (r["name"], kind, "the bucket fits the registers: no slow-way loop")
        if kind in DENSE:
            assert empty == 0, (r["name"], kind, "a bin at every (plane, group, tile)")
        if kind.startswith("tiles_") and (pw // 2 + 15) // 16 > 2:
            assert empty > 0, (r["name"], kind)
    if "tiles_alternate" in r["lists"]:
        bl = bucket_lengths(r, build_list("tiles_alternate", ph, pw)).reshape(-1, (pw // 2 + 15) // 16)
        assert (bl[:, 0::2] > 0).all() and (bl[:, 1::2] == 0).all()
    if r["walks"]:
        for b in walks_lists(r)[0]:
            assert_valid(b, ph, pw)
    if ph * pw <= (1 << 16):
        cover = covers_of(r, 1)[0]
        assert np.array_equal(ref_embed(orc, cover, B.make_bins(np.zeros((0, 3), np.int64)), np.zeros(0, np.uint8)), cover), "empty list: the cover"


def _embed_dev(lib, bufs, env, r, covers, bins, bits, index=None, inplace=False, usable=False):
    nimg, n = bits.shape
    ctx = PC._ctx_with_env(env, r["w"], r["h"], slots=r["slots"], lib=lib)
    try:
        if index is not None:
            ctx.set_bit_index(index)
        kb, pk = bufs.put(np.ascontiguousarray(bins).view(np.uint8).reshape(-1, 8))
        cb, pc = bufs.put(covers)
        bb, pb = bufs.put(bits)
        ob, po = (cb, pc) if inplace else bufs.put(np.zeros_like(covers))
        ub, pu = bufs.put(np.zeros(nimg, np.uint64))
        ctx.embed_batch_dev(nimg, pc, r["w"], r["h"], pk, pb, n, po, usable_ptr=pu if usable else None)
        ctx.sync()
        if not inplace:
            assert np.array_equal(bufs.get(cb), covers), "the cover buffer is read, never written"
        return np.asarray(bufs.get(ob)).copy(), np.asarray(bufs.get(ub)).copy()
    finally:
        ctx.close()


def _extract_dev(lib, bufs, env, r, src, bins, index=None, register=False):
    nimg, n = len(src), len(bins)
    ctx = PC._ctx_with_env(env, r["w"], r["h"], slots=r["slots"], lib=lib)
    try:
        if index is not None:
            ctx.set_bit_index(index)
        kb, pk = bufs.put(np.ascontiguousarray(bins).view(np.uint8).reshape(-1, 8))
        sb, ps = bufs.put(src)
        if register:
            ctx.bins_register_dev(pk, n)
        res = []
        for _ in range(2 if register else 1):
            rb, pr = bufs.put(np.full((nimg, n), 9, np.uint8))
            ctx.extract_batch_dev(nimg, ps, r["w"], r["h"], pk, n, pr)
            ctx.sync()
            res.append(np.asarray(bufs.get(rb)).copy())
        if register:
            ctx.bins_register_dev(None, 0)
            assert np.array_equal(res[0], res[1]), "the registered list, second call"
        return res[0]
    finally:
        ctx.close()


def check_shared(lib, orc, bufs, r, kind, sat=False):
    """one list shared by slots + 1 images: embed_batch_dev against the fp64 reference (shuffled, sorted + bit index, in place,
    TFFT_EMBED_DELTA=0) and extract_batch_dev of the reference's stego under every read variant"""
    PM.assert_plan(lib, r)
    ph, pw = PM.grid_of(r)
    nimg = r["slots"] + 1
    bins = build_list(kind, ph, pw)
    n = len(bins)
    covers = covers_of(r, nimg, sat)
    bits = np.random.default_rng(_seed(kind, ph, pw, 5)).integers(0, 2, (nimg, n)).astype(np.uint8)
    want = np.stack(_pmap(lambda i: ref_embed(orc, covers[i], bins, bits[i]), range(nimg)))
    if sat:
        clamped = float(np.isin(want[0], (0, 255)).mean())
        print(case_id((r, kind, sat)), "pixels of the reference stego at 0 or 255: %.3f" % clamped)
        assert clamped > 0.1, clamped
    # the reference's reading of its own stego, and how many listed bins it has on the decision line: the exception below is for those
    allowed = max(3, n // 20000)
    want_raw, line = [], []
    for i, (raw, v) in enumerate(_pmap(lambda i: ref_read(orc, want[i], bins), range(nimg))):
        want_raw.append(raw)
        line.append(on_decision_line(v))
        assert int(line[i].sum()) <= allowed, ("the reference alone has too many listed bins on its decision line", i, int(line[i].sum()), allowed)
    want_raw = np.stack(want_raw)
    lsb_frac = PM.lsb_frac_of(r)
    # a. embed
    sbins, idx = B.bins_sort(bins, lib=lib)
    s, _ = _embed_dev(lib, bufs, {}, r, covers, bins, bits)
    d = np.abs(s.astype(np.int16) - want)
    frac = [float((d[i] != 0).mean()) for i in range(nimg)]
    print(case_id((r, kind, sat)), "n = %d, largest difference to the fp64 stego %d LSB, fraction of differing pixels %s" % (n, d.max(), frac))
    assert d.max() <= 1, ("stego differs from the fp64 reference by more than 1 LSB", int(d.max()), int((d > 1).sum()))
    assert max(frac) < lsb_frac, (frac, lsb_frac)
    assert np.array_equal(_embed_dev(lib, bufs, {}, r, covers, sbins, bits, index=idx)[0], s), "sorted list + bit index"
    assert np.array_equal(_embed_dev(lib, bufs, {}, r, covers, bins, bits, inplace=True)[0], s), "in-place embedding"
    s0, _ = _embed_dev(lib, bufs, {"TFFT_EMBED_DELTA": "0"}, r, covers, bins, bits)
    dm = np.abs(s.astype(np.int16) - s0)
    assert dm.max() <= 1 and max(float((dm[i] != 0).mean()) for i in range(nimg)) < lsb_frac, ("TFFT_EMBED_DELTA=0", int(dm.max()), float((dm != 0).mean()))
    # b. extraction of the reference's stego
    for what, env, bl, index, reg in (("default", {}, bins, None, False), ("TFFT_TILE_READ=3", {"TFFT_TILE_READ": "3"}, bins, None, False),
                                      ("TFFT_TILE_READ=2", {"TFFT_TILE_READ": "2"}, bins, None, False), ("TFFT_TILE_READ=0", {"TFFT_TILE_READ": "0"}, bins, None, False),
                                      ("TFFT_TILE_READ=3, sorted", {"TFFT_TILE_READ": "3"}, sbins, idx, False),
                                      ("registered", {}, bins, None, True), ("registered, TFFT_TILE_READ=3", {"TFFT_TILE_READ": "3"}, bins, None, True)):
        got = _extract_dev(lib, bufs, env, r, want, bl, index=index, register=reg)
        assert set(np.unique(got)) <= {0, 1}, (what, "a position was not written", np.unique(got))
        for i in range(nimg):
            bad = np.nonzero(got[i] != want_raw[i])[0]
            assert len(bad) <= allowed and line[i][bad].all(), (what, "raw bits differ away from the reference's decision line", i, len(bad), bad[:8], bins[bad[:8]])


USABLE_ENVS = ({}, {"TFFT_STATS_TILE": "2"}, {"TFFT_STATS_TILE": "0"})


def usable_cases(emulated=False):
    return [(r, env) for r in rows(emulated) for env in USABLE_ENVS]


def usable_id(c):
    return "%s-%s" % (c[0]["name"], ",".join("%s=%s" % kv for kv in c[1].items()) or "default")


def check_usable(lib, bufs, r, env):
    """usable_out does not depend on the list (COLS_STAT shares its kernel with the entry fetches) nor on the statistics variant `env`:
    every list of the row gives what the row's first list gives by default"""
    PM.assert_plan(lib, r)
    ph, pw = PM.grid_of(r)
    nimg = r["slots"] + 1
    covers = covers_of(r, nimg)
    want = None
    for kind in r["lists"]:
        bins = build_list(kind, ph, pw)
        bits = np.ones((nimg, len(bins)), np.uint8)
        if want is None:
            want = _embed_dev(lib, bufs, {}, r, covers, bins, bits, usable=True)[1]
            print(r["name"], "usable_out", want)
            assert (want < 3 * ph * pw // 2).all()
            if not env:
                continue
        u = _embed_dev(lib, bufs, env, r, covers, bins, bits, usable=True)[1]
        assert np.array_equal(u, want), (r["name"], kind, env, u, want)


WALKS_ENVS = ({}, {"TFFT_TILE_READ": "3"}, {"TFFT_STATS_TILE": "2"})
WALKS_SLOTS = 2


def walks_lists(r):
    """three images, three kinds: dense left and dense right shuffled, dense mixed in address order; jitter uniform in +-0.05"""
    ph, pw = PM.grid_of(r)
    bins = np.stack([build_list("dense_left", ph, pw, salt=1), build_list("dense_right", ph, pw, salt=2),
                     build_list("dense_mixed", ph, pw, salt=3, order="address")])
    jit = np.random.default_rng([ph, pw, 17]).uniform(-0.05, 0.05, bins.shape).astype(np.float32)
    return bins, jit


def check_walks(lib, orc, bufs, r):
    """one list per image (tfft_*_stream_batch_walks_dev) with jitter and adaptive alpha: each stego against the fp64 reference with
    the image's own list, the raw bits of the reference's stego against orc.read_bins, and the round trip on power-of-two covers"""
    rw = dict(r, slots=max(WALKS_SLOTS, r["slots"]))
    PM.assert_plan(lib, rw)
    w, h = r["w"], r["h"]
    ph, pw = PM.grid_of(r)
    bins, jit = walks_lists(r)
    nimg, n_bins = bins.shape
    plen = (n_bins - 912 - 40) // 56            # the stream fills the list but for a tail of 40 .. 95 positions
    secret, n_str = plen - 16, 912 + 56 * plen
    assert secret >= 0 and 40 <= n_bins - n_str < 96
    covers = covers_of(r, nimg)
    headers, payloads = WC._frames(nimg, secret, 70)
    want, want_raw = [], []
    for i in range(nimg):
        want.append(ref_embed(orc, covers[i], bins[i][:n_str], PC.rep_stream(headers[i], payloads[i]), jitter=jit[i][:n_str], adaptive=True))
        want_raw.append(ref_read(orc, want[i], bins[i], jit[i], adaptive=True)[0])
    want = np.stack(want)
    ours = None
    for env in WALKS_ENVS:
        s, _ = WC._run(lib, bufs, env, w, h, rw["slots"], covers, bins, jit, True, headers, payloads, False, walks=True)
        if ours is None:
            ours = s
            d = np.abs(s.astype(np.int16) - want)
            frac = [float((d[i] != 0).mean()) for i in range(nimg)]
            print(r["name"], "walks: n_bins %d, stream %d, largest difference to the fp64 stego %d LSB, fractions %s" % (n_bins, n_str, d.max(), frac))
            assert d.max() <= 1 and max(frac) < PM.lsb_frac_of(r), ("stego vs the fp64 reference", int(d.max()), frac)
        assert np.array_equal(s, ours), ("stego", env)
        ho, po, so, ro = WC._run(lib, bufs, env, w, h, rw["slots"], covers, bins, jit, True, headers, payloads, False, walks=True, extract_src=want)
        for i in range(nimg):
            assert np.array_equal(ro[i, :n_str], want_raw[i][:n_str]), ("raw bits vs the reference", env, i, int((ro[i, :n_str] != want_raw[i][:n_str]).sum()))
            bad = n_str + np.nonzero(ro[i, n_str:] != want_raw[i][n_str:])[0]       # beyond the stream nothing was embedded: any phase occurs
            if len(bad):
                assert _phase_near_boundary(orc, want[i], bins[i][bad], jit[i][bad], False).all(), ("beyond the stream, away from the decision line", env, i, bad[:8])
        if (ph, pw) == (h, w):
            assert list(so) == [secret] * nimg, (env, so)
            assert np.array_equal(ho, headers) and np.array_equal(po, payloads), env


def check_host_form(lib, bufs, r, kind="dense_mixed"):
    """tfft_embed_batch / tfft_extract_batch (host buffers, the three-stream pipeline) return the bytes of the _dev calls"""
    PM.assert_plan(lib, r)
    ph, pw = PM.grid_of(r)
    nimg = r["slots"] + 1
    bins = build_list(kind, ph, pw)
    covers = covers_of(r, nimg)
    bits = np.random.default_rng(_seed(kind, ph, pw, 5)).integers(0, 2, (nimg, len(bins))).astype(np.uint8)
    s, u = _embed_dev(lib, bufs, {}, r, covers, bins, bits, usable=True)
    raw = _extract_dev(lib, bufs, {}, r, s, bins)
    ctx = B.Context(r["w"], r["h"], slots=r["slots"], lib=lib)
    try:
        hs, hu = np.zeros_like(covers), np.zeros(nimg, np.uint64)
        ctx.embed_batch_host(covers, bins, bits, hs, usable=hu)
        assert np.array_equal(hs, s) and np.array_equal(hu, u), "tfft_embed_batch"
        hr = np.full((nimg, len(bins)), 9, np.uint8)
        ctx.extract_batch_host(s, bins, hr)
        assert np.array_equal(hr, raw), "tfft_extract_batch"
    finally:
        ctx.close()
