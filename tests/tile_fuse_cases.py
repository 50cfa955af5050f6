"""The fused statistics + embed + first inverse column step (k_fft_cols<COLS_STAT_EMBED>, TFFT_EMBED_TILE_FUSE) against the two launches it
replaces (COLS_STAT, then COLS_EMBED), written once and run twice: on the CPU-emulated build of the kernel sources
(tests/test_emulated_tile_fuse.py, HostBufs) and on the MI355X (tests/test_gpu_tile_fuse.py, TorchBufs).

Every case runs the same inputs with the knob at 2 and at 0 (both under TFFT_STATS_TILE=2, which lets COLS_STAT serve launches of any size)
and compares the two; the fp64 oracle comes in through the existing checkers (PH.check_phase_batch, WC.check_distinct_keys), which take the
pair as their `envs` and hold its first entry to the reference.

Rows.  One dimension of a cover selects the column plan; TFFT_COLS_LOG_N1 moves the split of a small two-step grid, so that every length
L = 2^log_n2 of the last forward step, 32 .. 512, is reached on a 64-wide grid of 512 or 1024 rows (two 16-column tiles, two images: the
emulator affords them), and the GPU run adds the natural plans of tests/plan_matrix_cases.py at their smallest covers (fused 2048-wide
plans (3,6) .. (3,9), two-step (6,7)).  40x300 is the smallest cover COLS_STAT reaches.  The plan ships fused at every one of these lengths,
L = 512 included -- and not at L = 16 (PAIR_ROWS: 40x300 split (5,4), and the fused 2048-wide plan (3,4)), where the
fused form would hold two workgroups per CU against COLS_STAT's three: there the knob changes nothing, and the rows check that.

Bars.  The medians (tfft_batch_medians: the fp32 values the embed's own statistics left on the device, per image and plane), usable_out at
three values of magmin and the raw bits read back from either stego are identical.  Every embed also says which launch sequence its chunk
took (tfft_embed_plan_info), shared list, per-image walks and fitted embed alike, so no comparison is one of a path with itself.  Stego bytes differ by at most 1 LSB, on a share of the bytes of at most twice the share at which the
TFFT_STATS_TILE=2 and =0 paths differ on the same inputs at the commit before this mode existed.  That share was measured with
measure_stats_tile_share() below, on the emulator and on the MI355X, over every row of this module: 0 differing bytes in every row on both
(-ffp-contract=on makes every instantiation round alike, csrc/Makefile).  MEASURED_SHARE = 0, so the bound is 0: the bytes are equal."""
import os
from contextlib import contextmanager

import numpy as np

import bin_list_cases as BL
import exact_batch_cases as XC
import fit_cases as FC
import parity_cases as PC
import phase_cases as PH
import plan_matrix_cases as PM
import walks_cases as WC
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

ON = {"TFFT_EMBED_TILE_FUSE": "2", "TFFT_STATS_TILE": "2"}
OFF = {"TFFT_EMBED_TILE_FUSE": "0", "TFFT_STATS_TILE": "2"}
MEASURED_SHARE = 0.0                 # stego bytes that differ between TFFT_STATS_TILE=2 and =0 at the parent commit (module docstring)
SHARE_BOUND = 2.0 * MEASURED_SHARE
MAGMINS = (0.01, 0.3, 1.0)
N_IMG = 2
STAGE_ORDER = [0, 1, 2, 10, 0, 1, 2, 8, 9, 3, 7, 4, 5, 6]      # bench.py's profile_stages


def _n1(v):
    return {"TFFT_COLS_LOG_N1": str(v)}


# name, w, h, kind, log_n1, log_n2, n_bits; key: PM.row_pk's (a walk that meets PM.assert_coverage, found on the host)
SMALL = [
    PM.row("s_L32", 40, 300, "two_step", 4, 5, 1500, slots=N_IMG),
    PM.row("s_L64", 40, 300, "two_step", 3, 6, 1500, slots=N_IMG, env=_n1(3)),
    PM.row("s_L128", 40, 300, "two_step", 2, 7, 1500, slots=N_IMG, env=_n1(2)),
    PM.row("s_L256", 40, 300, "two_step", 1, 8, 1500, slots=N_IMG, env=_n1(1)),
    PM.row("s_L512", 40, 600, "two_step", 1, 9, 1500, slots=N_IMG, env=_n1(1)),
]
NATURAL = [dict(PM.BY_NAME[n], slots=N_IMG) for n in ("f2k_6", "f2k_7", "f2k_9", "ts_6_7")] + \
          [PM.row("f2k_8", 1030, 1100, "fused", 3, 8, 3000, key=14, slots=N_IMG)]
# L = 16: COLS_STAT serves these plans, the fused form does not exist there (fewer resident workgroups than COLS_STAT): the pair, whatever the knob
PAIR_ROWS = [PM.row("s_L16", 40, 300, "two_step", 5, 4, 1500, slots=N_IMG, env=_n1(5)), dict(PM.BY_NAME["f2k_4"], slots=N_IMG)]
# hand-built lists (bin_list_cases): a 128 x 512 grid, four column tiles, L = 256 (one group per workgroup: a tile without entries is
# stored as zeros without the second transform) and L = 32 (eight groups per workgroup: every tile is transformed)
TILE_ROWS = [
    PM.row("t_L256", 100, 300, "two_step", 1, 8, 0, slots=N_IMG, env=_n1(1)),
    PM.row("t_L32", 100, 300, "two_step", 4, 5, 0, slots=N_IMG),
]
# tiles_alternate: tiles 0 and 2 hold entries, tile 1 between them none; dense_mixed: every bucket is a whole tile of 16 * L entries, NE * L
# of them in registers (the rest takes the loop through the value list), half of them addressed through the conjugate; dense_right: all of them
TILE_LISTS = ("tiles_alternate", "dense_mixed", "dense_right", "frame")


def ids(rows):
    return [r["name"] for r in rows]


@contextmanager
def env_set(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def both(r, extra=None):
    e = dict(r["env"], **(extra or {}))
    return dict(e, **ON), dict(e, **OFF)


def stage_launches(lib, orc, bufs, env, w, h, slots=N_IMG, n_bins=300, exact=False, adaptive=False):
    """tfft_profile_stage's launches per stage, set up as bench.py's profile_stages sets it up (tests/test_emulated_profile.py); exact /
    adaptive: with exact capacities (NEAR) or adaptive alpha switched on in the context first"""
    ctx = PC._ctx_with_env(env, w, h, slots=slots, lib=lib)
    try:
        if exact:
            ctx.set_batch_exact(XC.NEAR, XC.GUARD)
        if adaptive:
            ctx.set_phase_options(None, True)
        ph, pw = orc.next_pow2(h), orc.next_pow2(w)
        bins, idx = B.bins_sort(B.Walk(orc.subkeys(PC.PK)[0], ph, pw, lib=lib).next(n_bins), lib=lib)
        ctx.set_bit_index(idx)
        _kb, p_bins = bufs.put(bins.view(np.uint8).reshape(-1, 8))
        ctx.bins_register_dev(p_bins, n_bins)
        _ib, p_img = bufs.put(np.stack([cover_rgb(w, h, i) for i in range(slots)]))
        _ob, p_out = bufs.put(np.zeros((slots, h, w, 3), np.uint8))
        _bb, p_bits = bufs.put(np.random.default_rng(99).integers(0, 2, size=(slots, n_bins), dtype=np.uint8))
        _rb, p_raw = bufs.put(np.zeros((slots, n_bins), np.uint8))
        ctx.forward_rgb8_dev(p_img, w, h)
        ctx.sync()
        got = []
        for sid in STAGE_ORDER:
            _ms, nl = ctx.profile_stage(sid, 1, p_img, p_out, p_bins, p_bits, p_raw, n_bins, n_images=slots)
            got.append((B.Context.STAGES[sid], nl))
        ctx.sync()
        return got
    finally:
        ctx.close()


def assert_takes(lib, orc, bufs, env, w, h, fused, slots=N_IMG, **kw):
    """the plan a chunk of `slots` such covers takes under env: one launch for the pair, or the pair"""
    got = dict(stage_launches(lib, orc, bufs, env, w, h, slots, **kw))
    assert (got["cols_fwd_b"], got["cols_inv_a"]) == ((1, 0) if fused else (1, 1)), (env, w, h, got)


def _embed(lib, bufs, env, r, covers, bins, bits, magmin=0.01, info=None):
    """one tfft_embed_batch_dev: (stego, usable_out); info (a dict): also the fp32 medians the embed's statistics left per image
    (tfft_batch_medians) and the launch sequence its chunk took (tfft_embed_plan_info)"""
    nimg, n = bits.shape
    ctx = PC._ctx_with_env(env, r["w"], r["h"], slots=r["slots"], lib=lib)
    try:
        _kb, pk = bufs.put(np.ascontiguousarray(bins).view(np.uint8).reshape(-1, 8))
        cb, pc = bufs.put(covers)
        _bb, pb = bufs.put(bits)
        ob, po = bufs.put(np.zeros_like(covers))
        ub, pu = bufs.put(np.zeros(nimg, np.uint64))
        ctx.embed_batch_dev(nimg, pc, r["w"], r["h"], pk, pb, n, po, magmin=magmin, usable_ptr=pu)
        ctx.sync()
        assert np.array_equal(bufs.get(cb), covers), "the cover buffer is read, never written"
        if info is not None:
            assert nimg <= r["slots"]      # (one chunk: image i sits in slot i)
            info["med"] = ctx.batch_medians(nimg)
            info["plan"] = ctx.embed_plan_info()
        return np.asarray(bufs.get(ob)).copy(), np.asarray(bufs.get(ub)).copy()
    finally:
        ctx.close()


def compare_stego(tag, a, b, bound=SHARE_BOUND):
    d = np.abs(a.astype(np.int16) - b)
    share = float((d != 0).mean())
    print(tag, "largest difference %d LSB, share of differing bytes %.3g (bound %.3g)" % (d.max(), share, bound))
    assert d.max() <= 1, (tag, int(d.max()))
    assert share <= bound, (tag, share, bound)


def check_pair(lib, bufs, r, bins, extra=None, nimg=N_IMG, seed=5, fused=True):
    """one shared list, nimg covers: the fused form against the pair -- the medians, usable_out at three thresholds, the stego bytes, the
    bits read back; and each embed says which launch sequence it took (fused=False: a row whose plan keeps the pair whatever the knob)"""
    on, off = both(r, extra)
    covers = np.stack([cover_rgb(r["w"], r["h"], 30 + i) for i in range(nimg)])
    bits = np.random.default_rng([seed, len(bins)]).integers(0, 2, (nimg, len(bins))).astype(np.uint8)
    s_on = s_off = None
    for magmin in MAGMINS:
        ia, ib = {}, {}
        a, ua = _embed(lib, bufs, on, r, covers, bins, bits, magmin, info=ia)
        b, ub = _embed(lib, bufs, off, r, covers, bins, bits, magmin, info=ib)
        print(r["name"], "magmin", magmin, "usable_out", ua, ub, "medians", ia["med"].tolist(), "plans", ia["plan"], ib["plan"])
        assert ia["plan"]["delta"] and ib["plan"]["delta"] and ia["plan"]["stats"] == 1 and ib["plan"]["stats"] == 1, (ia["plan"], ib["plan"])
        assert ia["plan"]["tile_fuse"] == fused and not ib["plan"]["tile_fuse"], (r["name"], ia["plan"], ib["plan"])
        assert np.array_equal(ia["med"], ib["med"]) and (ia["med"] > 0).all(), (r["name"], ia["med"], ib["med"])
        assert np.array_equal(ua, ub), (r["name"], magmin, ua, ub)
        assert (ua > 0).any() or magmin == MAGMINS[-1], (r["name"], magmin, ua)
        if s_on is None:
            s_on, s_off = a, b
        else:
            assert np.array_equal(a, s_on) and np.array_equal(b, s_off), "the stego does not depend on magmin"
    compare_stego(r["name"], s_on, s_off)
    assert not np.array_equal(s_on, covers), "something was embedded"
    raw_on = BL._extract_dev(lib, bufs, r["env"], r, s_on, bins)
    raw_off = BL._extract_dev(lib, bufs, r["env"], r, s_off, bins)
    assert np.array_equal(raw_on, raw_off), (r["name"], int((raw_on != raw_off).sum()))
    assert set(np.unique(raw_on)) <= {0, 1}      # (a padded cover loses part of its stream in the crop, in the reference too: no round trip to ask for)
    return s_on, s_off


def check_plan_row(lib, orc, bufs, r):
    """every two-step plan: the row reaches its plan, COLS_STAT serves it, the knob decides between one launch and two, and the two agree"""
    PM.assert_plan(lib, r)
    on, off = both(r)
    assert_takes(lib, orc, bufs, on, r["w"], r["h"], True, r["slots"])
    assert_takes(lib, orc, bufs, off, r["w"], r["h"], False, r["slots"])
    bins = PM.shared_walk(lib, orc, r)
    c = PM.coverage(bins, *PM.grid_of(r), r["log_n1"])
    assert c["left"] > 0 and c["right"] > 0, (r["name"], c)      # entries on both sides of x = PW/2: some are addressed through the conjugate
    check_pair(lib, bufs, r, bins)


def check_pair_row(lib, orc, bufs, r):
    """L = 16: the fused form would hold fewer workgroups per CU than COLS_STAT, so the plan keeps the pair whatever
    the knob says -- the profiler and the embed itself say so, and the results are those of the knob at 0"""
    PM.assert_plan(lib, r)
    assert r["log_n2"] == 4
    on, off = both(r)
    assert_takes(lib, orc, bufs, on, r["w"], r["h"], False, r["slots"])
    assert_takes(lib, orc, bufs, off, r["w"], r["h"], False, r["slots"])
    check_pair(lib, bufs, r, PM.shared_walk(lib, orc, r), fused=False)


def _walks_plan(lib, bufs, env, r, b, fit=False, adaptive=False):
    """the launch sequence a per-image-walks embed (fit: a fitted embed) of batch b takes under env, and its stego"""
    nimg, n_bins, plen = len(b["covers"]), b["bins"].shape[1], b["payloads"].shape[1]
    ctx = PC._ctx_with_env(env, r["w"], r["h"], slots=nimg, lib=lib)
    try:
        _k, pb = bufs.put(np.ascontiguousarray(b["bins"]).view(np.uint8).reshape(-1, 8))
        _j, pj = bufs.put(b["jit"])
        _c, pc = bufs.put(b["covers"]); _h, phd = bufs.put(b["headers"]); _y, py = bufs.put(b["payloads"])
        ob, po = bufs.put(np.zeros_like(b["covers"])); _u, pu = bufs.put(np.zeros(nimg, np.uint64))
        if fit:
            _i, pi = bufs.put(np.full(nimg, -7, np.int32)); _w, pw_ = bufs.put(np.full(nimg, 7, np.uint32))
            ctx.embed_stream_batch_fit_dev(nimg, pc, r["w"], r["h"], pb, pj, n_bins, phd, py, plen, po, adaptive=adaptive, usable_ptr=pu,
                                           iters_ptr=pi, wrong_ptr=pw_, max_iters=4, margin=0.5)
        else:
            ctx.embed_stream_batch_walks_dev(nimg, pc, r["w"], r["h"], pb, pj, n_bins, phd, py, plen, po, adaptive=adaptive, usable_ptr=pu)
        ctx.sync()
        return ctx.embed_plan_info(), np.asarray(bufs.get(ob)).copy()
    finally:
        ctx.close()


def check_tile_contents(lib, orc, bufs, r, kind):
    """hand-built lists: empty tiles between full ones, buckets beyond the registers, conjugate entries, whole tiles; the fused stego also
    against the fp64 reference of bin_list_cases"""
    PM.assert_plan(lib, r)
    ph, pw = PM.grid_of(r)
    bins = BL.build_list(kind, ph, pw)
    bl = BL.bucket_lengths(r, bins)
    regs = BL.registers(r, embed=True)
    print(r["name"], kind, "n", len(bins), "largest bucket", int(bl.max()), "entries in registers", regs, "empty buckets", int((bl == 0).sum()))
    if kind.startswith("dense"):
        assert bl.max() > regs and bl.max() == 16 << r["log_n2"], (bl.max(), regs)
    if kind == "tiles_alternate":
        t = bl.reshape(-1, (pw // 2 + 15) // 16)
        assert (t[:, 0] > 0).all() and (t[:, 1] == 0).all() and (t[:, 2] > 0).all()
    if kind == "dense_right":
        assert (bins["x"] > pw // 2).all()
    s_on, _ = check_pair(lib, bufs, r, bins)
    covers = np.stack([cover_rgb(r["w"], r["h"], 30 + i) for i in range(N_IMG)])
    bits = np.random.default_rng([5, len(bins)]).integers(0, 2, (N_IMG, len(bins))).astype(np.uint8)
    want = BL.ref_embed(orc, covers[0], bins, bits[0])
    d = np.abs(s_on[0].astype(np.int16) - want)
    assert d.max() <= 1 and float((d != 0).mean()) < PM.lsb_frac_of(r), (r["name"], kind, int(d.max()), float((d != 0).mean()))


def check_walks_jitter(lib, orc, bufs, r):
    """one walk per image with jitter, two images with different keys, through the stream pipeline: the stream is shorter than the lists, so
    the entries behind its end carry bit = 2 and must leave their bins alone.  WC.check_distinct_keys holds the fused form (envs[0]) to
    the fp64 reference image by image and the pair (envs[1]) to the fused form's bytes and usable_out"""
    PM.assert_plan(lib, r)
    on, off = both(r)
    # the per-image calls do take the fused launch with the knob at 2, the pair at 0 and with adaptive alpha -- the embed itself says so
    b = FC.make_batch(orc, r["w"], r["h"], 2, secret=0, jitter=0.05, tag=b"tile-fuse", n_threads=2, lib=lib)
    p_on, s_on = _walks_plan(lib, bufs, on, r, b)
    p_off, s_off = _walks_plan(lib, bufs, off, r, b)
    p_ad, _ = _walks_plan(lib, bufs, on, r, b, adaptive=True)
    assert p_on["tile_fuse"] and p_on["stats"] == 1 and not p_off["tile_fuse"] and p_off["stats"] == 1 and not p_ad["tile_fuse"], (p_on, p_off, p_ad)
    compare_stego(r["name"] + " walks", s_on, s_off)
    WC.check_distinct_keys(lib, orc, bufs, r["w"], r["h"], nimg=2, slots=2, secret=0, jitter=0.05, adaptive=False, lsb_frac=PM.lsb_frac_of(r),
                           envs=(on, off), n_threads=2)


def check_bracket_miss(lib, bufs, orc, r):
    """TFFT_STATS_SKEW=5 moves every bracket off the median: the gated tail re-runs the plain forward step from `tmp` for every plane and the
    fallback kernels settle the statistics.  The capacities are those of the pair (and of the run without the skew): `tmp` survived"""
    bins = PM.shared_walk(lib, orc, r)
    covers = np.stack([cover_rgb(r["w"], r["h"], 30 + i) for i in range(N_IMG)])
    bits = np.ones((N_IMG, len(bins)), np.uint8)
    on, off = both(r, {"TFFT_STATS_SKEW": "5"})
    for magmin in MAGMINS[:2]:
        s_a, u_a = _embed(lib, bufs, on, r, covers, bins, bits, magmin)
        s_b, u_b = _embed(lib, bufs, off, r, covers, bins, bits, magmin)
        s_c, u_c = _embed(lib, bufs, both(r)[0], r, covers, bins, bits, magmin)
        assert np.array_equal(u_a, u_b) and np.array_equal(u_a, u_c), (magmin, u_a, u_b, u_c)
        compare_stego(r["name"] + " skew", s_a, s_b)
        assert np.array_equal(s_a, s_c)


def check_fallbacks(lib, orc, bufs, r):
    """adaptive alpha, the fit pipeline and exact capacities (NEAR) keep the two launches whatever the knob says: the same bytes with the
    knob at 2 and at 0, and the profiler (which asks the pipelines' own embed_path) counts the pair for adaptive alpha and exact
    capacities.  (The fitted embed's first iteration is the walks embed itself, and it reads the listed bins' values afterwards: it asks its
    chunk for that list, which keeps the pair: tfft_embed_plan_info says so after a fitted embed, and says "fused" after the plain walks
    embed of the same batch.)"""
    w, h = r["w"], r["h"]
    on, off = both(r)
    assert_takes(lib, orc, bufs, on, w, h, True)
    assert_takes(lib, orc, bufs, on, w, h, False, adaptive=True)
    assert_takes(lib, orc, bufs, on, w, h, False, exact=True)
    # adaptive alpha: the embed waits for the medians
    bins, jit = PH._walk(lib, orc, w, h, 600, 0.05)
    covers = np.stack([cover_rgb(w, h, 30 + i) for i in range(N_IMG)])
    bits = np.random.default_rng(3).integers(0, 2, (N_IMG, len(bins))).astype(np.uint8)
    res = []
    for env in (on, off):
        ctx = PC._ctx_with_env(env, w, h, slots=N_IMG, lib=lib)
        try:
            ctx.set_phase_options(jit, True)
            _kb, pk = bufs.put(np.ascontiguousarray(bins).view(np.uint8).reshape(-1, 8))
            _cb, pc = bufs.put(covers); _bb, pb = bufs.put(bits)
            ob, po = bufs.put(np.zeros_like(covers)); ub, pu = bufs.put(np.zeros(N_IMG, np.uint64))
            ctx.embed_batch_dev(N_IMG, pc, w, h, pk, pb, len(bins), po, usable_ptr=pu)
            ctx.sync()
            res.append((np.asarray(bufs.get(ob)).copy(), np.asarray(bufs.get(ub)).copy()))
        finally:
            ctx.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), "adaptive alpha"
    # the fit pipeline (it reads the values of the listed bins from the list the forward step writes)
    b = FC.make_batch(orc, w, h, N_IMG, secret=0, jitter=0.05, tag=b"tile-fuse", n_threads=2, lib=lib)
    fits = []
    for env in (on, off):
        fits.append(FC.run_fit(lib, bufs, b, N_IMG, False, False, max_iters=4, env=env))
    for x, y in zip(fits[0], fits[1]):
        assert np.array_equal(np.asarray(x), np.asarray(y)), "fit pipeline"
    p_fit, _ = _walks_plan(lib, bufs, on, r, b, fit=True)
    p_walks, _ = _walks_plan(lib, bufs, on, r, b)
    assert p_fit["stats"] == 1 and not p_fit["tile_fuse"] and p_walks["tile_fuse"], (p_fit, p_walks)      # the same batch: fitted -> the pair, plain walks -> fused
    # exact capacities, NEAR
    xb = XC.shared_bins(lib, w, h)
    xbits = np.ones((N_IMG, len(xb)), np.uint8)
    ex = []
    for env in (on, off):
        with env_set(env):
            ex.append(XC.embed_dev(lib, bufs, covers, xb, xbits, N_IMG, XC.NEAR))
    assert np.array_equal(ex[0][0], ex[1][0]) and np.array_equal(ex[0][1], ex[1][1]) and list(ex[0][2]) == list(ex[1][2]), "exact capacities (NEAR)"


def check_profiler(lib, orc, bufs, r):
    """the sequence of bench.py's profile_stages: the fused launch is timed as cols_fwd_b, cols_inv_a reports no launch, and the stages
    behind it still run (rows_inv reads the intermediate where the fused launch left it)"""
    on, off = both(r)
    got = stage_launches(lib, orc, bufs, on, r["w"], r["h"], r["slots"])
    print(r["name"], got)
    d = dict(got)
    assert d["cols_fwd_b"] == 1 and d["cols_inv_a"] == 0 and d["rows_inv"] == 1 and d["cols_inv_b"] == 1, got
    assert got[-1] == ("rows_inv", 1)
    d0 = dict(stage_launches(lib, orc, bufs, off, r["w"], r["h"], r["slots"]))
    assert d0["cols_fwd_b"] == 1 and d0["cols_inv_a"] == 1, d0
    assert d0["medians"] == d["medians"], (d0, d)
    # knob unset: a small launch forced into COLS_STAT keeps the pair (tests/test_emulated_profile.py pins that count too)
    d1 = dict(stage_launches(lib, orc, bufs, dict(r["env"], TFFT_STATS_TILE="2"), r["w"], r["h"], r["slots"]))
    assert d1["cols_inv_a"] == 1, d1


def measure_stats_tile_share(lib, bufs, orc, rows):
    """the share of stego bytes at which the TFFT_STATS_TILE=2 and =0 paths differ, per row (run at the parent commit, with that commit's
    library and binding: MEASURED_SHARE)"""
    out = {}
    for r in rows:
        bins = PM.shared_walk(lib, orc, r) if r["n_bits"] else BL.build_list("dense_mixed", *PM.grid_of(r))
        covers = np.stack([cover_rgb(r["w"], r["h"], 30 + i) for i in range(N_IMG)])
        bits = np.random.default_rng([5, len(bins)]).integers(0, 2, (N_IMG, len(bins))).astype(np.uint8)
        a, _ = _embed(lib, bufs, dict(r["env"], TFFT_STATS_TILE="2"), r, covers, bins, bits)
        b, _ = _embed(lib, bufs, dict(r["env"], TFFT_STATS_TILE="0"), r, covers, bins, bits)
        d = np.abs(a.astype(np.int16) - b)
        out[r["name"]] = (int(d.max()), int((d != 0).sum()), int(d.size))
        print("stats_tile 2 vs 0:", r["name"], out[r["name"]])
    return out
