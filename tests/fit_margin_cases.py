"""What the fitted embed (tfft_embed_stream_batch_fit[_dev]) promises about its margin, its counts and its frozen
images, against an fp64 restatement of that section.  Shared by the emulated run (tests/test_emulated_fit_margin.py, HostBufs) and the
MI355X run (tests/test_gpu_fit_margin.py, TorchBufs); tests/fit_cases.py checks that the stego reads back, this file what the call says
about it.

The reference (`reference`) is numpy over the fp64 checker's forward transform of the cover and of the returned bytes, not a port of the
fit kernels.  For stream entry k of an image: m_k = s_k Im(Fs e^{-i j_k}) the signed distance from the reader's decision line, mu_k the
margin the entry is fitted to, delta_k = 1e-5 |Fs| + 1e-6 rms(|Fs[plane]|) the off-axis bar of the fp32 forward transform
(parity_cases.spec_errors).  Per image, converged or not (`check_promises`):
  P1  iters_out >= 0  =>  every m_k >= mu_k / 2 - delta_k
  P2  #{m_k < -delta_k} <= wrong_out <= #{m_k < delta_k}
  P3  iters_out = -1  =>  some m_k < mu_k / 2 + delta_k
  P4  iters_out >= 0  =>  wrong_out = 0 and iters_out <= max_iters
and two conditions on the reference alone keep delta from swallowing a shortfall: max delta_k / mu_k <= 0.02, and at most two entries of
an image within delta_k of the line (P2 is an equality up to those)."""
import math
from types import SimpleNamespace

import numpy as np

import fit_cases as FC
from parity_cases import rep_stream
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

ALPHA = 0.5          # the calls' default
KAPPA = 3.0          # the floor of the margin in rounding deviations sigma = sqrt(W H / 24) (TFFT_FIT_KAPPA)
DELTA_SHARE = 0.02   # delta_k / mu_k, at most
NEAR_LINE = 2        # entries of one image within delta_k of the decision line, at most

# (w, h, jitter, adaptive, center): 65 x 130 keeps a quarter of its 128 x 256 grid (the tightest constraints); 100 x 300 pads to
# 128 x 512 (two-step columns); 120 x 200 has an odd row byte count
COMBOS = {"65x130": (65, 130, 0.0, False, False), "100x300": (100, 300, 0.05, True, False), "120x200": (120, 200, 0.05, False, True)}

# what the runs of one session measured, for DESIGN.md section 10 (printed by every check)
FIGURES = {"min m/mu, converged": math.inf, "max delta/mu": 0.0, "near the line": 0, "images": 0}


def contrast_rgb(w, h, seed, gain):
    """cover_rgb stretched about 128 and clamped: photo-like content with a share of its bytes at 0 and 255"""
    x = (cover_rgb(w, h, seed).astype(np.float64) - 128.0) * gain + 128.0
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def smooth_rgb(w, h, seed):
    """a low-contrast cover about 128: one slow wave of 20 grey levels and noise of 2.  Read with center = 1 its spectrum in the annulus is
    that noise, |F| about 2 sqrt(W H): tau |F| sin(alpha) is under the floor 3 sqrt(W H / 24) on most bins.  (fit_cases.gradient_rgb is
    not such a cover: its ramps end in a step of a hundred grey levels at the edge of the zero padding, which fills the annulus --
    15-25 % of its entries are at the floor)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 128 + 20 * np.sin(2 * np.pi * x / w) * np.cos(np.pi * y / h)
    img = np.stack([base + 10 * c for c in range(3)], axis=-1) + rng.normal(0, 2, (h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _covers(kind, w, h, nimg, seed):
    if kind == "photo":
        return None                                              # (make_batch's own cover_rgb(w, h, 700 + seed + i))
    if kind == "smooth":
        return np.stack([smooth_rgb(w, h, 800 + seed + i) for i in range(nimg)])
    assert kind[0] == "contrast"
    return np.stack([contrast_rgb(w, h, 700 + seed + i, kind[1]) for i in range(nimg)])


_BATCHES = {}


def batch(lib, orc, w, h, jitter, nimg=2, seed=0, margin_bins=300, cover="photo", tag=b"fit-margin"):
    """fit_cases.make_batch, made once per session; its fitted runs and cover spectra are kept with it and never written again"""
    key = (lib._name, w, h, jitter, nimg, seed, margin_bins, cover, tag)
    if key not in _BATCHES:
        b = FC.make_batch(orc, w, h, nimg, jitter=jitter, tag=tag, seed=seed, margin_bins=margin_bins, lib=lib,
                          covers=_covers(cover, w, h, nimg, seed))
        b["runs"], b["f0"] = {}, {}
        _BATCHES[key] = b
    return _BATCHES[key]


def take(b, idx):
    """the batch of images idx of b, in that order"""
    s = dict(b)
    s["pks"] = [b["pks"][i] for i in idx]
    for k in ("bins", "jit", "covers", "headers", "payloads"):
        s[k] = None if b[k] is None else np.ascontiguousarray(b[k][list(idx)])
    s["runs"], s["f0"] = {}, {}
    return s


def fitted(lib, bufs, b, adaptive, center, max_iters, margin=0.5, slots=2, host=False):
    """(stego, usable_out, iters_out, wrong_out) of one fitted call, run once"""
    key = (bufs.__name__, adaptive, center, max_iters, margin, slots, host)
    if key not in b["runs"]:
        b["runs"][key] = FC.run_fit(lib, bufs, b, slots, adaptive, center, max_iters=max_iters, margin=margin, host=host)
    return b["runs"][key]


def reference(orc, b, i, stego, adaptive, center, margin):
    """section 10 in fp64 for image i of the batch and the bytes `stego` a reader would get: per stream entry m, mu, delta, wrong"""
    plen = b["payloads"].shape[1]
    n_str = 912 + 56 * plen
    if (i, center) not in b["f0"]:
        b["f0"][(i, center)] = orc.forward_rgb8(b["covers"][i], center)
    F0, med0 = b["f0"][(i, center)]
    Fs, _ = orc.forward_rgb8(stego, center)
    t = B.bins_to_triples(b["bins"][i][:n_str])
    p, y, x = t[:, 0], t[:, 1], t[:, 2]
    f0, fs = F0[p, y, x], Fs[p, y, x]
    mag0 = np.maximum(1e-12, np.abs(f0))
    a = ALPHA * np.clip(mag0 / np.maximum(1e-12, med0[p]), 0.5, 2.0) if adaptive else np.full(n_str, ALPHA)
    floor = KAPPA * math.sqrt(b["w"] * b["h"] / 24.0)
    mu = np.maximum(margin * mag0 * np.sin(a), floor)
    j = b["jit"][i][:n_str].astype(np.float64) if b["jit"] is not None else np.zeros(n_str)
    u = (fs * np.exp(-1j * j)).imag
    bits = rep_stream(b["headers"][i], b["payloads"][i])
    assert len(bits) == n_str
    m = np.where(bits == 1, u, -u)
    wrong = np.where(bits == 1, u < 0, u >= 0)
    rms = np.sqrt(np.mean(np.abs(Fs) ** 2, axis=(1, 2)))
    delta = 1e-5 * np.abs(fs) + 1e-6 * rms[p]
    return SimpleNamespace(m=m, mu=mu, delta=delta, wrong=wrong, floor=floor, at_floor=(mu == floor), n=n_str)


def short_of_half(r):
    """the entry furthest below P1's bound mu / 2 - delta: (k, m_k - bound); negative: the bound is violated"""
    gap = r.m - (0.5 * r.mu - r.delta)
    k = int(np.argmin(gap))
    return k, float(gap[k])


def check_promises(orc, b, out, adaptive, center, max_iters, margin=0.5, tag=""):
    """P1-P4 and the two conditions on the reference for every image of one fitted call; returns the references"""
    s, _, it, wr = out
    refs = []
    for i in range(len(s)):
        r = reference(orc, b, i, s[i], adaptive, center, margin)
        refs.append(r)
        share = float((r.delta / r.mu).max())
        near = int((np.abs(r.m) < r.delta).sum())
        lo, hi = int((r.m < -r.delta).sum()), int((r.m < r.delta).sum())
        k, gap = short_of_half(r)
        least = float((r.m / r.mu).min())
        FIGURES["max delta/mu"] = max(FIGURES["max delta/mu"], share)
        FIGURES["near the line"] += near
        FIGURES["images"] += 1
        if it[i] >= 0:
            FIGURES["min m/mu, converged"] = min(FIGURES["min m/mu, converged"], least)
        print("fit margin", tag, "image", i, "iters_out", int(it[i]), "wrong_out", int(wr[i]), "fp64 wrong %d..%d" % (lo, hi),
              "min m/mu %.4f" % least, "max delta/mu %.2e" % share, "near the line", near)
        # conditions on the inputs, from the reference alone
        assert share <= DELTA_SHARE, (tag, i, "delta/mu", share)
        assert near <= NEAR_LINE, (tag, i, "entries within delta of the line", near)
        # P2: the count is the fp64 count, up to the entries on the line
        assert lo <= int(wr[i]) <= hi, (tag, i, "P2: wrong_out", int(wr[i]), "fp64 count between", lo, hi)
        assert it[i] >= -1
        if it[i] >= 0:
            # P1: entry k is the worst, `gap` its distance above mu_k / 2 - delta_k
            assert gap >= 0, (tag, i, "P1: entry", k, "m", float(r.m[k]), "mu", float(r.mu[k]), "delta", float(r.delta[k]), "short by", -gap)
            # P4
            assert wr[i] == 0 and it[i] <= max_iters, (tag, i, "P4", int(it[i]), int(wr[i]), max_iters)
        else:
            # P3: an image reported as not converged has an entry that is not clear of mu / 2
            over = float((r.m - (0.5 * r.mu + r.delta)).min())
            assert over < 0, (tag, i, "P3: every entry is above mu/2 + delta by at least", over)
    print("fit margin figures so far", FIGURES)
    return refs


# ---- 1. the margin at three tau --------------------------------------------------------------------------------------
def check_margin(lib, orc, bufs, combo, margin):
    """P1-P4 at `margin`, 32 corrections allowed.  On the reference alone: the one-shot stego violates P1's bound on every image (the fit
    had work to do), and tau = 1 puts mu above tau = 1/2's on at least 90 % of the entries (the floor does not hide tau)"""
    w, h, jitter, adaptive, center = COMBOS[combo]
    b = batch(lib, orc, w, h, jitter)
    one = fitted(lib, bufs, b, adaptive, center, 0)          # (the bytes of max_iters = 0 do not depend on the margin)
    for i in range(len(one[0])):
        r = reference(orc, b, i, one[0][i], adaptive, center, margin)
        k, gap = short_of_half(r)
        assert gap < 0, (combo, margin, i, "the one-shot embed already holds the margin: not a case for the fit", gap)
        r1 = reference(orc, b, i, one[0][i], adaptive, center, 1.0)
        r5 = reference(orc, b, i, one[0][i], adaptive, center, 0.5)
        raised = float((r1.mu > r5.mu).mean())
        assert raised >= 0.9, (combo, i, "share of entries whose mu tau = 1 raises", raised)
    out = fitted(lib, bufs, b, adaptive, center, 32, margin)
    check_promises(orc, b, out, adaptive, center, 32, margin, (combo, "tau", margin))
    return out


# ---- 2. the counts mid-flight ----------------------------------------------------------------------------------------
def check_counts(lib, orc, bufs, combo, max_iters, host=False):
    """P1-P4 after 0, 1 or 2 corrections, where the counts are not zero: at 0 and 1 the fp64 reference itself counts wrong bits in every
    image.  host: the host form reports the same iters_out and wrong_out"""
    w, h, jitter, adaptive, center = COMBOS[combo]
    b = batch(lib, orc, w, h, jitter)
    out = fitted(lib, bufs, b, adaptive, center, max_iters)
    refs = check_promises(orc, b, out, adaptive, center, max_iters, 0.5, (combo, "max_iters", max_iters))
    if max_iters <= 1:
        for i, r in enumerate(refs):
            assert int((r.m < -r.delta).sum()) > 0, (combo, max_iters, i, "no wrong bit in the reference: the count is not exercised")
    if host:
        hout = fitted(lib, bufs, b, adaptive, center, max_iters, host=True)
        assert np.array_equal(hout[2], out[2]) and np.array_equal(hout[3], out[3]), ("host form", hout[2], out[2], hout[3], out[3])
    return out


# ---- 3. the partition of k_fit_count ---------------------------------------------------------------------------------
def check_partition(lib, orc, bufs, w, h, margin_bins, max_iters, nimg=2):
    """P1-P4 where the per-workgroup shares of the count are unequal.  The library counts an image's n_bins entries in
    nblk = min(64, ceil(n_bins / 1024)) workgroups of ceil(n_bins / nblk): 2557 -> 853, 853, 851; 2258 -> 753, 753, 752; 2256 -> 3 x 752
    and no entry beyond the stream; 66001 -> 63 x 1032 and 985, the cap reached.  An entry that no workgroup counts shows only where it
    is a stream entry that reads wrong: with max_iters = 0 a sixth of the stream does, in every image, so six images are taken (tried
    with `per` rounded down: the entry dropped from image 2 of these keys is such an entry, at 2258 and at 2557)"""
    jitter, adaptive, center = (0.05, False, True) if (w, h) == (120, 200) else (0.05, False, False)
    b = batch(lib, orc, w, h, jitter, nimg=nimg, margin_bins=margin_bins)
    n_bins = b["bins"].shape[1]
    nblk = min(64, (n_bins + 1023) // 1024)
    per = (n_bins + nblk - 1) // nblk
    out = fitted(lib, bufs, b, adaptive, center, max_iters)
    check_promises(orc, b, out, adaptive, center, max_iters, 0.5, ((w, h), "n_bins", n_bins, "shares", per, n_bins - (nblk - 1) * per, "max_iters", max_iters))
    return n_bins, nblk, per


# ---- 4. freezing and prefixes ----------------------------------------------------------------------------------------
def check_freezing(lib, orc, bufs, w=120, h=200, nimg=4, seed=0):
    """image i converges after k_i corrections (a run with 32 allowed); a run with m allowed reports k_i where m >= k_i, with the final
    bytes -- frozen while its chunk mate iterates on -- and -1 elsewhere.  Needs images that converge at different counts"""
    jitter, adaptive, center = 0.05, True, False
    b = batch(lib, orc, w, h, jitter, nimg=nimg, seed=seed)
    final = fitted(lib, bufs, b, adaptive, center, 32)
    check_promises(orc, b, final, adaptive, center, 32, 0.5, ((w, h), "freezing, final"))
    k = final[2]
    print("fit margin freezing: k =", k.tolist())
    assert (k >= 1).all(), ("every image must converge, and none at once", k)
    kmin, kmax = int(k.min()), int(k.max())
    assert kmin < kmax, ("the images converge together: pick another seed", k)
    for m in sorted({kmin - 1, kmin, kmax - 1, kmax}):
        out = fitted(lib, bufs, b, adaptive, center, m)
        check_promises(orc, b, out, adaptive, center, m, 0.5, ((w, h), "freezing, max_iters", m))
        for i in range(nimg):
            if m >= k[i]:
                assert out[2][i] == k[i], ("iters_out", m, i, out[2].tolist(), k.tolist())
                assert np.array_equal(out[0][i], final[0][i]), ("bytes of a converged image moved", m, i, int((out[0][i] != final[0][i]).sum()))
                assert out[3][i] == 0
            else:
                assert out[2][i] == -1, ("iters_out", m, i, out[2].tolist(), k.tolist())
    return k


# ---- 5. placement ----------------------------------------------------------------------------------------------------
def _same_image(tag, got, j, want, i):
    assert np.array_equal(got[0][j], want[0][i]), (tag, "bytes of image", i, int((got[0][j] != want[0][i]).sum()))
    for what, g, wn in zip(("usable_out", "iters_out", "wrong_out"), got[1:], want[1:]):
        assert g[j] == wn[i], (tag, what, "image", i, int(g[j]), int(wn[i]))


def check_permutation(lib, orc, bufs, w=120, h=200, nimg=4, seed=0, order=(2, 0, 3, 1)):
    """the batch in another order, chunks of the same size: every image gets the same bytes, iters_out, wrong_out and usable_out"""
    jitter, adaptive, center = 0.05, True, False
    b = batch(lib, orc, w, h, jitter, nimg=nimg, seed=seed)
    want = fitted(lib, bufs, b, adaptive, center, 32)
    got = fitted(lib, bufs, take(b, order), adaptive, center, 32)
    for j, i in enumerate(order):
        _same_image("permuted", got, j, want, i)


def check_singles(lib, orc, bufs, w=120, h=200, nimg=4, seed=0):
    """every image alone in a context of one slot: the same again"""
    jitter, adaptive, center = 0.05, True, False
    b = batch(lib, orc, w, h, jitter, nimg=nimg, seed=seed)
    want = fitted(lib, bufs, b, adaptive, center, 32)
    for i in range(nimg):
        got = fitted(lib, bufs, take(b, [i]), adaptive, center, 32, slots=1)
        _same_image("alone", got, 0, want, i)


# ---- 6. a cover whose margins are the floor --------------------------------------------------------------------------
def check_floor_bound(lib, orc, bufs, w=100, h=300):
    """smooth_rgb read with center = 1: at least half of the stream entries of every image have mu = kappa sigma, the floor (reference
    alone; 70 % measured, so both sides of the max are taken); P1-P4"""
    jitter, adaptive, center = 0.05, True, True
    b = batch(lib, orc, w, h, jitter, cover="smooth")
    out = fitted(lib, bufs, b, adaptive, center, 32)
    refs = check_promises(orc, b, out, adaptive, center, 32, 0.5, ((w, h), "smooth"))
    for i, r in enumerate(refs):
        share = float(r.at_floor.mean())
        print("fit margin floor-bound image", i, "share of entries at the floor %.3f" % share)
        assert share >= 0.5, (i, "share of entries at the floor", share)
    return out


# ---- 7. covers that clamp --------------------------------------------------------------------------------------------
CLAMP_GAIN = 12.0


def check_clamping(lib, orc, bufs, max_iters, w=120, h=200):
    """high-contrast covers with at least 20 % of their bytes at 0 or 255 (asserted on the input; two thirds at this gain): the inverse
    clamps what the corrections ask for, so convergence is not required -- P1-P4 are: what the call reports is true of the bytes it
    returns"""
    jitter, adaptive, center = 0.05, False, False
    b = batch(lib, orc, w, h, jitter, cover=("contrast", CLAMP_GAIN))
    for i, c in enumerate(b["covers"]):
        clipped = float(((c == 0) | (c == 255)).mean())
        assert clipped >= 0.2, (i, "share of bytes at 0 or 255", clipped)
    out = fitted(lib, bufs, b, adaptive, center, max_iters)
    check_promises(orc, b, out, adaptive, center, max_iters, 0.5, ((w, h), "clamping, max_iters", max_iters))
    return out
