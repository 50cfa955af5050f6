"""The batched pipelines at the smallest cover of every column plan, written once and run twice: on the CPU-emulated build of the
kernel sources (tests/test_emulated_plan_matrix.py, HostBufs: index math only) and on the MI355X (tests/test_gpu_plan_matrix.py,
TorchBufs: the gfx950 build -- waves, LDS layout and occupancy attributes are what the emulator cannot show).

k_fft_cols is one template per column length LOGL and per mode; plan_cols picks (direct | two-step | fused, log_n1, log_n2) from PH, PW
and the images in a launch.  One dimension of a cover selects the plan, the other stays at 24-40 pixels (for the fused plans: just above
1024 / 2048), so every row is small.  Which row covers which point of plan_cols (after this table every reachable (class, log_n2) is run
by the bucket modes; `*` marks the points the older tests already reach):

    direct (PH <= 256), last step L = 2^log_n2     log_n2 2: d_L2   3: d_L3   4: d_L4, d_L4_wide   5*, 6*, 7*, 8* (40x24 .. 300x200 elsewhere)
    two-step (log_n1, log_n2)                      (4,5): ts_narrow (and 40x300*)   (5,5)*: 20x600 elsewhere   (5,6): ts_5_6
                                                   (6,6)*: 1080p / 4K elsewhere     (6,7): ts_6_7              (7,7): ts_7_7
    fused, PW = 2048, log_n2                       4: f2k_4, f2k_4x2   5*: 2040x130 elsewhere   6: f2k_6, f2k_6x2   7: f2k_7, f2k_7x2
                                                   8*: 1080p elsewhere   9: f2k_9, f2k_9x2
    fused, PW = 4096 (launches of >= 2 images)     4: f4k_4 (and f4k_4_single: one image under TFFT_FUSE_WIDE=2)   5: f4k_5   6: f4k_6
                                                   7: f4k_7   8*, 9*: 4K batches elsewhere
    M = PW/2 (half width; the column tile is 16)   2: n_M2   4: n_M4   8: n_M8, n_M8_tall, ts_narrow   16: ts_7_7   32+: every other row
    rows at PW = 16384 (k_rows_fwd / inv <13,1>)   w_16k_L2, w_16k_L6

plan_info gives the stated plan for every row (asserted first in every check).  Two rows exist for the walks check alone, d_L4_wide
(130x12) and n_M8_tall (12x130): its stream needs 2108 bins, a walk marks every bin together with its mirror and skips three in ten,
and a 64x16 or 16x64 plane has 2604 bins -- 40x12 and 12x40 cannot hold it, the same L = 16 and M = 8 at 256 columns or rows can.

Inputs: with the default annulus a 64-wide, tall grid keeps every bin in rows y < 29 -- one k2 group of a two-step plan.  The rows
therefore walk the whole plane: rmin = 0 and rmax = whole_plane_rmax(PH, PW) >= hypot(PH, PW) / min(PH, PW) (tfft_walk_create only forms
rmax * min(PH, PW); the reference takes any rmax as well).  The turtle is still a local random walk from a key-dependent start, so
coverage() computes on the host what a list touches and assert_coverage() holds it to the conditions below before any device work:
  bins on both sides of x = PW/2 (PW >= 8); at least two 16-column tiles (M >= 32); for two-step and fused plans at least two distinct
  k1 = y mod N1 and two distinct k2 = y div N1, in walk coordinates and in the stored rows (a bin with x > PW/2 lives, conjugated, at
  (PH - y, PW - x)); bins in both y < PH/2 and y > PH/2.
No row needed a condition relaxed: PH = 4 (d_L2) has only y = 1, 3, which still are the two halves, and its plan is direct (no k1 / k2).

Bars: nothing new.  1 LSB to the fp64 stego; bit-exact extraction except where the reference's own decision is a coin flip;
1e-5 |F| + 1e-6 rms for spectra; 2e-6 for fp32 medians and <= 2 for fp32 capacities (PW > 8192 only); lsb_frac = 0.05 below 4096 pixels
and 0.01 from there on, as tests/test_emulated.py has it."""
import hashlib
import math
import os
from contextlib import contextmanager

import numpy as np
import pytest

import analysis_cases as AC
import exact_batch_cases as XC
import parity_cases as PC
import walks_cases as WC
from _checkers import Params
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb


class SharedOracle:
    """The fp64 oracle with its transforms of one input computed once: rows that differ only in the images per launch (f2k_4 / f2k_4x2,
    f4k_4 / f4k_4_single) ask for the same stego images, raw bits and capacities.  What it returns is shared: read-only."""
    CACHED = ("capacity_rgb8", "embed_rgb8", "extract_bits")      # (not forward_rgb8: its spectra are up to 400 MB each)

    def __init__(self, orc):
        self._orc = orc
        self._memo = {}

    @staticmethod
    def _key(v):
        if isinstance(v, np.ndarray):
            return ("a", v.shape, str(v.dtype), hashlib.sha1(np.ascontiguousarray(v)).digest())
        if isinstance(v, Params):
            return ("p", bytes(v))
        return v

    def __getattr__(self, name):
        fn = getattr(self._orc, name)
        if name not in self.CACHED:
            return fn

        def cached(*a, **kw):
            key = (name, tuple(self._key(v) for v in a), tuple(sorted((k, self._key(v)) for k, v in kw.items())))
            if key not in self._memo:
                res = fn(*a, **kw)
                for v in (res if isinstance(res, tuple) else (res,)):
                    if isinstance(v, np.ndarray):
                        v.setflags(write=False)
                self._memo[key] = res
            return self._memo[key]
        return cached


def whole_plane_rmax(ph, pw):
    """an rmax that makes every off-axis bin eligible: rmax * min(PH, PW) >= hypot(PH, PW)"""
    return math.hypot(ph, pw) / min(ph, pw) * 1.001


def row(name, w, h, kind, log_n1, log_n2, n_bits, key=0, walk_keys=(), slots=1, env=None, gpu_only=(), groups=()):
    """key: which of row_pk's keys the row walks with (see there), walk_keys: the same for the images of the walks check; slots: images
    per launch (the plan depends on it at PW = 4096); env: set around the whole row; gpu_only: the checks the emulator cannot afford at
    this row (tests/test_emulated_plan_matrix.py lists the measured times); groups: the further checks this row stands for its group in"""
    return dict(name=name, w=w, h=h, kind=kind, log_n1=log_n1, log_n2=log_n2, n_bits=n_bits, key=key, walk_keys=tuple(walk_keys), slots=slots,
                env=env or {}, gpu_only=tuple(gpu_only), groups=tuple(groups))


# groups: "walks" = the per-image walks pipeline (jitter + adaptive alpha), "stats" = phase histograms + batched capacities (every
# two-step row with whole column tiles is in it: with the default annulus the in-kernel statistics, COLS_STAT, serve those grids under
# TFFT_STATS_TILE=2, and on 2- and 1-tile grids their launch was refused until the launcher sized its reservations by the tiles a
# workgroup has), "limits" = the fallbacks above PW = 8192
ROWS = [
    # direct, L = 4, 8, 16 (H <= 16)
    row("d_L2", 40, 3, "direct", 0, 2, 120),
    row("d_L3", 40, 6, "direct", 0, 3, 300),
    row("d_L4", 40, 12, "direct", 0, 4, 600, groups=("stats",)),
    row("d_L4_wide", 130, 12, "direct", 0, 4, 600, key=1, walk_keys=(1, 2, 3), groups=("walks",)),      # (for the walks check: see the module docstring)
    # narrow covers: M = PW/2 = 2, 4, 8 (a 2-pixel-wide cover has no eligible bin: x = 1 is PW/2; W = 3 is the narrowest usable one)
    row("n_M2", 3, 40, "direct", 0, 6, 120),
    row("n_M4", 6, 40, "direct", 0, 6, 300),
    row("n_M8", 12, 40, "direct", 0, 6, 600, groups=("stats",)),
    row("n_M8_tall", 12, 130, "direct", 0, 8, 600, walk_keys=(0, 1, 2), groups=("walks",)),       # (for the walks check: see the module docstring)
    row("ts_narrow", 12, 600, "two_step", 5, 5, 1500),
    # two-step
    row("ts_5_6", 40, 1100, "two_step", 5, 6, 3000, groups=("stats",), gpu_only=("forward", "delta", "stats")),
    row("ts_6_7", 40, 5000, "two_step", 6, 7, 4000, walk_keys=(4, 5, 6), groups=("walks", "stats"), gpu_only=("forward", "delta", "walks", "stats")),
    row("ts_7_7", 24, 9000, "two_step", 7, 7, 4000, key=4, groups=("stats",), gpu_only=("forward", "delta", "stats")),
    # fused, 2048 wide: one image per launch, and two
    row("f2k_4", 1030, 70, "fused", 3, 4, 3000, key=35, walk_keys=(35, 39, 69), groups=("walks", "stats"), gpu_only=("stats",)),
    row("f2k_4x2", 1030, 70, "fused", 3, 4, 3000, key=35, slots=2),
    row("f2k_6", 1030, 300, "fused", 3, 6, 3000, key=14),
    row("f2k_6x2", 1030, 300, "fused", 3, 6, 3000, key=14, slots=2, gpu_only=("delta",)),
    row("f2k_7", 1030, 600, "fused", 3, 7, 3000, key=13, gpu_only=("forward", "delta")),
    row("f2k_7x2", 1030, 600, "fused", 3, 7, 3000, key=13, slots=2, gpu_only=("forward", "delta")),
    row("f2k_9", 1030, 2100, "fused", 3, 9, 3000, key=15, gpu_only=("forward", "delta")),
    row("f2k_9x2", 1030, 2100, "fused", 3, 9, 3000, key=15, slots=2, gpu_only=("forward", "delta")),
    # fused, 4096 wide: launches of two images (one image alone keeps the three-pass plan by default)
    row("f4k_4", 2050, 70, "fused", 3, 4, 3000, key=138, slots=2, groups=("stats",), gpu_only=("stats",)),
    row("f4k_5", 2050, 130, "fused", 3, 5, 3000, key=9, slots=2, gpu_only=("delta",)),
    row("f4k_6", 2050, 300, "fused", 3, 6, 3000, key=54, slots=2, gpu_only=("forward", "delta")),
    row("f4k_7", 2050, 600, "fused", 3, 7, 3000, key=3, slots=2, gpu_only=("forward", "delta")),
    row("f4k_4_single", 2050, 70, "fused", 3, 4, 3000, key=138, env={"TFFT_FUSE_WIDE": "2"}),
    # the row kernels at PW = 16384 = TFFT_MAX_DIM
    row("w_16k_L2", 8200, 3, "direct", 0, 2, 3000, key=426),
    row("w_16k_L6", 8200, 40, "direct", 0, 6, 3000, key=442, groups=("stats", "limits")),
]
BY_NAME = {r["name"]: r for r in ROWS}


def rows_of(group=None, check=None, emulated_only=False):
    return [r for r in ROWS if (group is None or group in r["groups"]) and not (emulated_only and check in r["gpu_only"])]


def forward_rows(emulated_only=False):
    """check_forward transforms one image at a time: one row per (size, environment) is all it can tell apart"""
    seen, out = set(), []
    for r in rows_of(check="forward", emulated_only=emulated_only):
        k = (r["w"], r["h"], tuple(sorted(r["env"].items())))
        if k not in seen:
            seen.add(k)
            out.append(r)
    return out


def grid_of(r):
    return AC.p2(r["h"]), max(2, AC.p2(r["w"]))


@contextmanager
def row_env(r):
    old = {k: os.environ.get(k) for k in r["env"]}
    os.environ.update(r["env"])
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def assert_plan(lib, r):
    """the row reaches the plan it is in the table for: a later change of plan_cols cannot silently move it onto a covered one"""
    with row_env(r):
        ctx = B.Context(r["w"], r["h"], slots=r["slots"], lib=lib)
    try:
        p = ctx.plan_info(r["w"], r["h"], r["slots"])
    finally:
        ctx.close()
    kind = "fused" if p["fused"] else ("direct" if p["direct"] else "two_step")
    assert (kind, p["log_n1"], p["log_n2"]) == (r["kind"], r["log_n1"], r["log_n2"]), (r["name"], p)
    ph, pw = grid_of(r)
    assert r["log_n1"] + r["log_n2"] == ph.bit_length() - 1, (r["name"], ph)
    return p


def row_rmax(r):
    return whole_plane_rmax(*grid_of(r))


def coverage(bins, ph, pw, log_n1):
    """what a bin list touches, from the list alone (host): walk coordinates (x, y) and the stored ones (a bin of the mirror half
    x > PW/2 is kept conjugated at (PH - y, PW - x) of the half spectrum)"""
    bins = np.asarray(bins).ravel()
    x, y = bins["x"].astype(np.int64), bins["y"].astype(np.int64)
    m = pw // 2
    mirror = x > m
    sx = np.where(mirror, pw - x, x)
    sy = np.where(mirror, (ph - y) % ph, y)
    n1 = 1 << log_n1
    cells = np.unique(np.stack([bins["plane"].astype(np.int64), y, x]), axis=1).shape[1]
    eligible = 3 * max(0, ph - 2) * max(0, pw - 2)
    return dict(left=int((x < m).sum()), right=int(mirror.sum()), low=int((2 * y < ph).sum()), high=int((2 * y > ph).sum()),
                tiles=len(np.unique(sx >> 4)), n_tiles=(m + 15) // 16,
                k1=len(np.unique(y % n1)), k2=len(np.unique(y // n1)), sk1=len(np.unique(sy % n1)), sk2=len(np.unique(sy // n1)),
                n_k1=n1, n_k2=ph // n1, fraction=cells / max(1, eligible))


def assert_coverage(r, bins, tag=""):
    ph, pw = grid_of(r)
    c = coverage(bins, ph, pw, r["log_n1"])
    print("%-13s %-8s %5dx%-5d grid %5dx%-5d bins %5d: %.4f of the plane, tiles %d/%d, k1 %d/%d, k2 %d/%d, x<M %d x>M %d, y<PH/2 %d y>PH/2 %d"
          % (r["name"], tag, r["w"], r["h"], pw, ph, np.asarray(bins).size, c["fraction"], c["tiles"], c["n_tiles"], c["k1"], c["n_k1"], c["k2"],
             c["n_k2"], c["left"], c["right"], c["low"], c["high"]))
    if pw >= 8:
        assert c["left"] > 0 and c["right"] > 0, (r["name"], tag, "both sides of x = PW/2", c)
    if pw // 2 >= 32:
        assert c["tiles"] >= 2, (r["name"], tag, "two 16-column tiles", c)
    if r["kind"] != "direct":
        assert min(c["k1"], c["k2"], c["sk1"], c["sk2"]) >= 2, (r["name"], tag, "two k1 and two k2", c)
    assert c["low"] > 0 and c["high"] > 0, (r["name"], tag, "both halves of y", c)
    return c


def row_pk(r, k=None):
    """The row's path key.  The turtle starts at a key-dependent bin and moves one bin at a time (x is a symmetric random walk, y drifts
    upwards, both wrap), so on a grid thousands of columns wide a few thousand bins stay within some tens of columns of the start: a
    row's key is the first of this sequence whose walk starts close enough to x = PW/2 (or to the wrap at x = 0) for the list to meet
    the coverage conditions -- found once on the host, recorded in the table, asserted by check_coverage."""
    return hashlib.sha256(b"plan-matrix#%d" % (r["key"] if k is None else k)).digest()


def walks_pks(r, ks=None):
    return [row_pk(r, k) for k in (r["walk_keys"] if ks is None else ks)]


def walks_lists(lib, orc, r, ks=None):
    """the lists (and jitter) WC.check_distinct_keys builds for the row's walks check"""
    ph, pw = grid_of(r)
    keys = b"".join(b"".join(orc.subkeys(pk)) for pk in walks_pks(r, ks))
    bins, jit, st = B.walks_build(keys, ph, pw, WALKS_BINS, max_jitter=0.05, rmin=0.0, rmax=row_rmax(r), n_threads=2, lib=lib)
    assert (st == 0).all(), (r["name"], st)
    return bins, jit


def shared_walk(lib, orc, r, n=None, rmin=0.0, k=None):
    """the list check_delta_embedding / check_tile_read walk for this row (the row's key, the whole plane)"""
    ph, pw = grid_of(r)
    return B.Walk(orc.subkeys(row_pk(r, k))[0], ph, pw, rmin=rmin, rmax=row_rmax(r), lib=lib).next(n or r["n_bits"])


def lsb_frac_of(r):
    return 0.05 if r["w"] * r["h"] < 4096 else 0.01


# ---- the checks, one row each -------------------------------------------------------------------------------------------------------
def check_coverage(lib, orc, r):
    """host only: plan, then the conditions on every list the row's checks will walk"""
    assert_plan(lib, r)
    assert_coverage(r, shared_walk(lib, orc, r), "shared")      # (check_delta and check_row_tile_read walk this list)
    if "walks" in r["groups"]:
        assert len(r["walk_keys"]) == WALKS_IMAGES
        bins, _ = walks_lists(lib, orc, r)
        for i in range(WALKS_IMAGES):
            assert_coverage(r, bins[i], "walk %d" % i)
        assert len({(int(b[0]["plane"]), int(b[0]["y"]), int(b[0]["x"])) for b in bins}) == WALKS_IMAGES, "distinct keys start in different places"


def check_forward(lib, orc, r):
    """forward against the fp64 oracle (both centrings) and forward -> inverse = identity, single image, at the row's size"""
    assert_plan(lib, r)
    with row_env(r):
        PC.check_forward_against_oracle(lib, orc, [(r["w"], r["h"])])
        PC.check_identity_roundtrip(lib, [(r["w"], r["h"])])


def check_delta(lib, orc, bufs, r):
    """PC.check_delta_embedding with the oracle: delta and write-then-invert embeds, in place, batched extraction, every statistics
    variant, 1 LSB to the fp64 stego, the reference's reading of our stego.  nimg = slots + 1: a full launch of `slots` images and a
    last chunk of one."""
    assert_plan(lib, r)
    with row_env(r):
        stats = PC.check_delta_embedding(lib, orc, bufs, r["w"], r["h"], r["n_bits"], nimg=r["slots"] + 1, rmin=0.0, rmax=row_rmax(r),
                                         lsb_frac=lsb_frac_of(r), with_oracle=True, pk=row_pk(r))
    print(r["name"], "fraction of +-1 LSB pixels vs the fp64 stego (delta, write-then-invert):", stats)


def check_tile_read(lib, orc, bufs, w, h, nimg=2, n=200, rmin=0.05, rmax=0.95, slots=None, pk=PC.PK):
    """Spectrum-free batched extraction (bins bucketed per tile, bits read in LDS by the last forward column step) against the spectrum +
    k_read path: TFFT_TILE_READ = 3 and 0 on the sorted list, 3 and 2 on the unsorted one -- the same bits every time."""
    ph, pw = orc.next_pow2(h), orc.next_pow2(w)
    bins = B.Walk(orc.subkeys(pk)[0], ph, pw, rmin=rmin, rmax=rmax, lib=lib).next(n)
    if ph >= 4 * pw:        # tall grid: the annulus reaches beyond PW/2
        assert (bins["x"] > pw // 2).any() and (bins["x"] < pw // 2).any()
    sbins, idx = B.bins_sort(bins, lib=lib)
    imgs = np.stack([cover_rgb(w, h, 20 + i) for i in range(nimg)])
    ib, pi = bufs.put(imgs)
    res = []
    for mode, bl, index in (("3", sbins, idx), ("0", sbins, idx), ("3", bins, None), ("2", bins, None)):
        ctx = PC._ctx_with_env({"TFFT_TILE_READ": mode}, w, h, slots=slots or nimg, lib=lib)
        if index is not None:
            ctx.set_bit_index(index)
        kb, pk = bufs.put(np.ascontiguousarray(bl).view(np.uint8).reshape(-1, 8))
        rb, pr = bufs.put(np.full((nimg, n), 9, np.uint8))
        ctx.extract_batch_dev(nimg, pi, w, h, pk, n, pr)
        ctx.sync(); ctx.close()
        res.append(np.asarray(bufs.get(rb)).copy())
    for r in res[1:]:
        assert np.array_equal(r, res[0])
    assert set(np.unique(res[0])) <= {0, 1}
    return res[0]


def check_row_tile_read(lib, orc, bufs, r):
    assert_plan(lib, r)
    with row_env(r):
        check_tile_read(lib, orc, bufs, r["w"], r["h"], nimg=r["slots"] + 1, n=r["n_bits"], rmin=0.0, rmax=row_rmax(r), slots=r["slots"],
                        pk=row_pk(r))


WALKS_IMAGES = 3
WALKS_SECRET = 0
WALKS_BINS = 912 + 56 * (WALKS_SECRET + 16) + 300      # what WC.check_distinct_keys walks for this secret


def check_walks(lib, orc, bufs, r):
    """the per-image walks pipeline (tfft_*_stream_batch_walks_dev) with jitter and adaptive alpha -- the PI / PH instantiations of the
    bucket modes -- against the fp64 reference image by image: WC.check_distinct_keys over the whole plane"""
    assert_plan(lib, r)
    with row_env(r):
        WC.check_distinct_keys(lib, orc, bufs, r["w"], r["h"], nimg=WALKS_IMAGES, slots=max(2, r["slots"]), secret=WALKS_SECRET, jitter=0.05,
                               adaptive=True, lsb_frac=lsb_frac_of(r), envs=({}, {"TFFT_TILE_READ": "0"}, {"TFFT_EMBED_DELTA": "0"}),
                               n_threads=2, rmin=0.0, rmax=row_rmax(r), pks=walks_pks(r))


def check_stats(lib, bufs, r):
    """phase histograms against the fp64 spectrum (host and _dev forms, chunks = single calls) and every batched usable_out =
    tfft_capacity(magmin * tfft_medians) of the image alone, under every statistics variant"""
    assert_plan(lib, r)
    w, h = r["w"], r["h"]
    with row_env(r):
        covers = np.stack([cover_rgb(w, h, 30 + i) for i in range(r["slots"] + 1)])
        spec = AC.np_spectrum(covers[0], False)
        AC.check_hist_image(lib, bufs, covers[0], False, spec, nbins_list=(8, 256), slots=r["slots"])
        AC.check_hist_chunks(lib, bufs, covers, nbins=256, slots=r["slots"])
        ph, pw = grid_of(r)
        if pw <= 8192:      # (above, the single-image call is itself the fp32 count: check_limits holds both to the oracle)
            PC.check_batch_capacity(lib, bufs, w, h, nimg=3, cases=((0.05, 0.45, 0.01), (0.0, 1.5, 0.3), (0.1, 0.6, 1.0)))


def check_limits(lib, orc, bufs, r):
    """above PW = 8192 the exact statistics do not apply (turtlefft_hip.h): tfft_medians / tfft_capacity return the fp32 answers (2e-6
    relative, <= 2 bins), tfft_exact_info says 0, a batched embed under tfft_set_batch_exact(ALL) reports -1 with the fp32 count of the
    mode-off call; beyond TFFT_MAX_DIM = 16384 in either dimension: TFFT_E_TOO_LARGE"""
    assert_plan(lib, r)
    w, h = r["w"], r["h"]
    assert grid_of(r)[1] > 8192
    covers = np.stack([cover_rgb(w, h, 70 + i) for i in range(2)])
    ctx = B.Context(w, h, lib=lib)
    try:
        for i in range(2):
            ctx.forward_rgb8(covers[i])
            med = ctx.medians()
            assert ctx.exact_info() == [0, 0, 0], ctx.exact_info()
            spec = AC.np_spectrum(covers[i])
            want = np.array([AC.median_abs(spec[p]) for p in range(3)])
            assert np.allclose(med, want, rtol=2e-6, atol=0), (i, med, want)
            _, want_med = orc.forward_rgb8(covers[i], want_spec=False)
            assert np.allclose(med, want_med, rtol=2e-6, atol=0), (i, med, want_med)
            cap = ctx.capacity(0.01 * med)
            assert ctx.exact_info() == [0, 0, 0], ctx.exact_info()
            cap_want, _ = orc.capacity_rgb8(covers[i], Params())
            assert abs(int(cap) - int(cap_want)) <= 2, (i, cap, cap_want)
    finally:
        ctx.close()
    bins = XC.shared_bins(lib, w, h)
    bits = np.ones((2, len(bins)), np.uint8)
    s_off, u_off, st_off = XC.embed_dev(lib, bufs, covers, bins, bits, 2, XC.OFF)
    s_all, u_all, st_all = XC.embed_dev(lib, bufs, covers, bins, bits, 2, XC.ALL)
    assert (st_off == 0).all() and (st_all == -1).all(), (st_off, st_all)
    assert np.array_equal(u_all, u_off) and np.array_equal(s_all, s_off), (u_all, u_off)
    for i in range(2):
        cap_want, _ = orc.capacity_rgb8(covers[i], Params())
        assert abs(int(u_off[i]) - int(cap_want)) <= 2, (i, u_off, cap_want)
    for (mw, mh) in ((16385, 8), (8, 16385)):
        with pytest.raises(B.TfftError) as ei:
            B.Context(mw, mh, lib=lib)
        assert ei.value.status == -3, (mw, mh, ei.value.status)      # TFFT_E_TOO_LARGE
