#!/usr/bin/env python3
"""tools/stealth_eval.py -- what the stego analysis calls measure, and what they cost, on one MI355X.

  --cost  wall time per call of tfft_phase_hist_batch_dev (256 bins, no threshold), tfft_quality_batch_dev (SSE + SSIM) and
          tfft_extract_stream_batch_dev (sorted, registered shared list, 4 KB payload) on the same batch: 32 x 1080p (16 slots) and
          8 x 4K centred (8 slots).  The legs are ALTERNATED inside one process (round r runs each once); median over rounds.
  --auc   the phase-histogram detector of the reference's security analysis (ATTACKS.md section 1) on synthetic covers (synth.cover_rgb,
          NOT photographs): per cell N covers of 1920 x 1080 and their one-shot stego (tfft_embed_stream_batch_dev, a 4 KB payload, one
          shared walk), alpha in {0.1, 0.22, 0.5} x jitter in {0, 0.05}, plus a fitted cell (tfft_embed_stream_batch_fit_dev, alpha 0.5,
          no jitter) beside the one-shot one; --payload sets another payload size.  Scores per image, summed over the planes, of the
          256-bin annulus phase histograms: KL against the pooled histogram of a disjoint set of reference covers (analysis.kl_divergence)
          and the mass in the +-alpha bins (analysis.peak_mass).  AUC (analysis.auc: stego positive, covers negative) per cell and score,
          PSNR / SSIM medians.
  --robust  what a one-shot stego survives, on synthetic covers (synth.cover_rgb, NOT photographs): 32 stegos of
          1920 x 1080 (default alpha 0.5 and density 0.7, a 4 KB payload, one shared walk) through tfft_robustness_batch_dev with AWGN of
          sigma 0.5, 1, 2, 4, 8 and JPEG quantisation at Q 95, 90, 75, 50: mean raw BER, mean byte error rate after the repetition code,
          share of images whose message came back.  Cost, measured like --cost (legs alternated in one process, median over rounds): the
          channel kernels alone, the robustness call with one channel and with all of them, against tfft_extract_stream_batch_dev on the
          same batch.

  --spam  the blind detector on synthetic covers (synth.cover_rgb, NOT photographs): per payload N covers of
          1920 x 1080 and their one-shot stego (default alpha 0.5 and density 0.7, one shared walk), payloads of 4096, 512 and 64 bytes
          (--payload, a comma list).  Per image the SPAM-686 features of tfft_spam_batch_dev (analysis.spam_features, mean over the planes);
          a Fisher linear discriminant (analysis.fld_fit) fitted on one half of the images and scored on the other, then the halves
          swapped: both AUCs, beside the KL and +-alpha-mass AUCs of --auc for the same images.
          --cost also times tfft_spam_batch_dev (T = 3) on the same batches.

    python tools/stealth_eval.py --cost [--rounds 5 --steps 5]
    python tools/stealth_eval.py --spam [--n 512 --n-ref 64 --payload 4096,512,64]
    python tools/stealth_eval.py --robust [--rounds 5 --steps 5]
    python tools/stealth_eval.py --auc [--n 256 --n-ref 64 --payload 4096] [--out FILE.json]
One JSON line on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"1080p": (1920, 1080, 32, 16, 0), "4k": (3840, 2160, 8, 8, 1)}
PLEN = 4096 + 16                      # 4 KB of ciphertext + the tag (--payload changes it for --auc)
NBINS = 256


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def header(plen):
    return np.frombuffer(b"FTTG\x02\x00" + bytes(28) + (plen - 16).to_bytes(4, "big"), np.uint8).copy()


def cost(name, rounds, steps, warmup):
    import torch
    from steganosaurus_amd import binding as B
    from steganosaurus_amd.synth import cover_rgb, gradient_cover
    w, h, nimg, slots, center = WORKLOADS[name]
    ph, pw = next_pow2(h), next_pow2(w)
    n_bins = 912 + 56 * PLEN
    bins = B.Walk(bytes(range(32)), ph, pw).next(n_bins)
    sbins, idx = B.bins_sort(bins)
    dev = "cuda:0"
    covers = torch.from_numpy(np.stack([cover_rgb(w, h, i) if i % 2 else gradient_cover(w, h, i) for i in range(nimg)])).to(dev)
    other = torch.clamp(covers.to(torch.int16) + torch.randint(-2, 3, covers.shape, dtype=torch.int16, device=dev), 0, 255).to(torch.uint8)
    flat = torch.full_like(covers, 97)
    d_bins = torch.from_numpy(sbins.view(np.uint8).reshape(-1, 8).copy()).to(dev)
    hist = torch.empty(nimg * 3 * NBINS, dtype=torch.int32, device=dev)
    sse = torch.empty(nimg * 3, dtype=torch.int64, device=dev)
    ssim = torch.empty(nimg * 3, dtype=torch.float64, device=dev)
    d_hdr = torch.empty(nimg * 38, dtype=torch.uint8, device=dev)
    d_pay = torch.empty(nimg * PLEN, dtype=torch.uint8, device=dev)
    d_st = torch.empty(nimg, dtype=torch.int32, device=dev)
    spam = torch.empty(nimg * 3 * 4 * 343, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = B.Context(w, h, slots=slots)
    ctx.set_bit_index(idx)
    ctx.bins_register_dev(d_bins.data_ptr(), n_bins)
    legs = {
        "extract_stream": lambda: ctx.extract_stream_batch_dev(nimg, covers.data_ptr(), w, h, d_bins.data_ptr(), n_bins, d_hdr.data_ptr(),
                                                               d_pay.data_ptr(), PLEN, d_st.data_ptr(), center=center),
        "phase_hist": lambda: ctx.phase_hist_batch_dev(nimg, covers.data_ptr(), w, h, hist.data_ptr(), nbins=NBINS, center=center),
        "quality": lambda: ctx.quality_batch_dev(nimg, covers.data_ptr(), other.data_ptr(), w, h, sse.data_ptr(), ssim.data_ptr()),
        "quality_sse_only": lambda: ctx.quality_batch_dev(nimg, covers.data_ptr(), other.data_ptr(), w, h, sse.data_ptr(), None),
        "spam": lambda: ctx.spam_batch_dev(nimg, covers.data_ptr(), w, h, spam.data_ptr(), t=3),
        "spam_flat": lambda: ctx.spam_batch_dev(nimg, flat.data_ptr(), w, h, spam.data_ptr(), t=3),
    }
    ms = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg, fn in legs.items():
            for _ in range(warmup):
                fn()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            ctx.sync()
            ms[leg].append((time.perf_counter() - t0) * 1e3 / steps)
    ctx.close()
    out = {leg: {"ms_per_call": round(statistics.median(v), 4), "ms_all_rounds": [round(x, 4) for x in v]} for leg, v in ms.items()}
    base = out["extract_stream"]["ms_per_call"]
    for leg in legs:
        out[leg]["vs_extract"] = round(out[leg]["ms_per_call"] / base, 4)
    out["spam"]["vs_quality_sse_only"] = round(out["spam"]["ms_per_call"] / out["quality_sse_only"]["ms_per_call"], 4)
    return {"image": [w, h], "images_per_call": nimg, "slots": slots, "center": center, "legs": out}


def auc_cells(n, n_ref, chunk, seed0, plen=PLEN):
    import torch
    from steganosaurus_amd import analysis as A
    from steganosaurus_amd import binding as B
    from steganosaurus_amd.synth import cover_rgb
    w, h = 1920, 1080
    ph, pw = next_pow2(h), next_pow2(w)
    n_bins = 912 + 56 * plen
    bins = B.Walk(bytes(range(32)), ph, pw).next(n_bins)
    dev = "cuda:0"
    ctx = B.Context(w, h, slots=chunk)
    d_bins = torch.from_numpy(bins.view(np.uint8).reshape(-1, 8).copy()).to(dev)
    d_walks = torch.from_numpy(np.tile(bins.view(np.uint8).reshape(-1, 8), (chunk, 1))).to(dev)       # one copy of the walk per image
    rng = np.random.default_rng(seed0)
    d_hdr = torch.from_numpy(np.tile(header(plen), chunk)).to(dev)
    d_pay = torch.from_numpy(rng.integers(0, 256, chunk * plen).astype(np.uint8)).to(dev)

    def hists(batch):
        out = torch.empty(len(batch) * 3 * NBINS, dtype=torch.int32, device=dev)
        ctx.phase_hist_batch_dev(len(batch), batch.data_ptr(), w, h, out.data_ptr(), nbins=NBINS)
        ctx.sync()
        return out.cpu().numpy().view(np.uint32).reshape(len(batch), 3, NBINS).astype(np.int64)

    ref = np.zeros((3, NBINS), np.int64)
    for i0 in range(0, n_ref, chunk):
        covers = torch.from_numpy(np.stack([cover_rgb(w, h, 100000 + i) for i in range(i0, min(n_ref, i0 + chunk))])).to(dev)
        ref += hists(covers).sum(axis=0)
    cells = [("one_shot", a, j) for a in (0.1, 0.22, 0.5) for j in (0.0, 0.05)] + [("fitted", 0.5, 0.0)]
    res = {}
    cover_h = []
    stego_h = {c: [] for c in cells}
    quality = {c: ([], []) for c in cells}
    iters = {c: [] for c in cells}
    for i0 in range(0, n, chunk):
        g = min(n, i0 + chunk) - i0
        covers = torch.from_numpy(np.stack([cover_rgb(w, h, seed0 + i) for i in range(i0, i0 + g)])).to(dev)
        cover_h.append(hists(covers))
        for cell in cells:
            kind, alpha, jit = cell
            stego = torch.empty_like(covers)
            if kind == "one_shot":
                jitter = B.walk_jitter(bytes(range(32, 128)), bins, jit) if jit else None
                ctx.set_phase_options(jitter)
                ctx.embed_stream_batch_dev(g, covers.data_ptr(), w, h, d_bins.data_ptr(), n_bins, d_hdr.data_ptr(), d_pay.data_ptr(), plen,
                                           stego.data_ptr(), alpha=alpha)
                ctx.set_phase_options()
            else:
                it = torch.empty(g, dtype=torch.int32, device=dev)
                ctx.embed_stream_batch_fit_dev(g, covers.data_ptr(), w, h, d_walks.data_ptr(), None, n_bins, d_hdr.data_ptr(), d_pay.data_ptr(),
                                               plen, stego.data_ptr(), alpha=alpha, iters_ptr=it.data_ptr())
                ctx.sync()
                iters[cell] += it.cpu().numpy().tolist()
            stego_h[cell].append(hists(stego))
            sse = torch.empty(g * 3, dtype=torch.int64, device=dev)
            ssim = torch.empty(g * 3, dtype=torch.float64, device=dev)
            ctx.quality_batch_dev(g, covers.data_ptr(), stego.data_ptr(), w, h, sse.data_ptr(), ssim.data_ptr())
            ctx.sync()
            quality[cell][0].append(A.psnr_db(sse.cpu().numpy().reshape(g, 3), w, h))
            quality[cell][1].append(ssim.cpu().numpy().reshape(g, 3))
            del stego
    ctx.close()
    cover_h = np.concatenate(cover_h)
    for cell in cells:
        kind, alpha, jit = cell
        sh = np.concatenate(stego_h[cell])
        kl_pos, kl_neg = A.kl_divergence(sh, ref).sum(axis=1), A.kl_divergence(cover_h, ref).sum(axis=1)
        pm_pos, pm_neg = A.peak_mass(sh, alpha).sum(axis=1), A.peak_mass(cover_h, alpha).sum(axis=1)
        psnr, ssim = np.concatenate(quality[cell][0]), np.concatenate(quality[cell][1])
        key = "%s_a%g_j%g" % (kind, alpha, jit)
        res[key] = {"embed": kind, "alpha": alpha, "jitter": jit, "n": int(len(sh)),
                    "auc_kl": round(A.auc(kl_pos, kl_neg), 4), "auc_peak": round(A.auc(pm_pos, pm_neg), 4),
                    "psnr_db_median": round(float(np.median(psnr)), 3), "ssim_median": round(float(np.median(ssim)), 6),
                    "kl_median_stego": float(np.median(kl_pos)), "kl_median_cover": float(np.median(kl_neg))}
        if iters[cell]:
            res[key]["fit_iters_median"] = float(np.median(iters[cell]))
            res[key]["fit_not_converged"] = int(sum(1 for v in iters[cell] if v < 0))
    return {"image": [w, h], "covers": "synth.cover_rgb (synthetic, not photographs)", "payload_bytes": plen, "n_bins": NBINS,
            "n_ref": n_ref, "cells": res}


def spam_cells(n, n_ref, chunk, seed0, payloads):
    """per payload: AUC of SPAM-686 + FLD (two folds) beside the white-box KL and +-alpha-mass AUCs, same covers and stegos"""
    import torch
    from steganosaurus_amd import analysis as A
    from steganosaurus_amd import binding as B
    from steganosaurus_amd.synth import cover_rgb
    w, h, alpha = 1920, 1080, 0.5
    ph, pw = next_pow2(h), next_pow2(w)
    dev = "cuda:0"
    ctx = B.Context(w, h, slots=chunk)
    rng = np.random.default_rng(seed0)
    streams = {}
    for plen in payloads:
        n_bins = 912 + 56 * plen
        bins = B.Walk(bytes(range(32)), ph, pw).next(n_bins)
        streams[plen] = (n_bins, torch.from_numpy(bins.view(np.uint8).reshape(-1, 8).copy()).to(dev),
                         torch.from_numpy(np.tile(header(plen), chunk)).to(dev),
                         torch.from_numpy(rng.integers(0, 256, chunk * plen).astype(np.uint8)).to(dev))

    def hists(batch):
        out = torch.empty(len(batch) * 3 * NBINS, dtype=torch.int32, device=dev)
        ctx.phase_hist_batch_dev(len(batch), batch.data_ptr(), w, h, out.data_ptr(), nbins=NBINS)
        ctx.sync()
        return out.cpu().numpy().view(np.uint32).reshape(len(batch), 3, NBINS).astype(np.int64)

    def feats(batch):
        out = torch.empty(len(batch) * 3 * 4 * 343, dtype=torch.int32, device=dev)
        ctx.spam_batch_dev(len(batch), batch.data_ptr(), w, h, out.data_ptr(), t=3)
        ctx.sync()
        counts = out.cpu().numpy().view(np.uint32).reshape(len(batch), 3, 4, 343)
        return A.spam_features(counts).mean(axis=1)                 # the per-image feature: the mean over the planes

    ref = np.zeros((3, NBINS), np.int64)
    for i0 in range(0, n_ref, chunk):
        covers = torch.from_numpy(np.stack([cover_rgb(w, h, 100000 + i) for i in range(i0, min(n_ref, i0 + chunk))])).to(dev)
        ref += hists(covers).sum(axis=0)
    cover_h, cover_f = [], []
    stego_h = {p: [] for p in payloads}
    stego_f = {p: [] for p in payloads}
    for i0 in range(0, n, chunk):
        g = min(n, i0 + chunk) - i0
        covers = torch.from_numpy(np.stack([cover_rgb(w, h, seed0 + i) for i in range(i0, i0 + g)])).to(dev)
        cover_h.append(hists(covers))
        cover_f.append(feats(covers))
        for plen in payloads:
            n_bins, d_bins, d_hdr, d_pay = streams[plen]
            stego = torch.empty_like(covers)
            ctx.embed_stream_batch_dev(g, covers.data_ptr(), w, h, d_bins.data_ptr(), n_bins, d_hdr.data_ptr(), d_pay.data_ptr(), plen,
                                       stego.data_ptr(), alpha=alpha)
            stego_h[plen].append(hists(stego))
            stego_f[plen].append(feats(stego))
            del stego
    ctx.close()
    cover_h, cover_f = np.concatenate(cover_h), np.concatenate(cover_f)
    half = n // 2
    res = {}
    for plen in payloads:
        sh, sf = np.concatenate(stego_h[plen]), np.concatenate(stego_f[plen])
        folds = []
        for (fit, test) in ((slice(0, half), slice(half, n)), (slice(half, n), slice(0, half))):
            model = A.fld_fit(sf[fit], cover_f[fit])
            folds.append(round(A.auc(A.fld_score(sf[test], model), A.fld_score(cover_f[test], model)), 4))
        kl_pos, kl_neg = A.kl_divergence(sh, ref).sum(axis=1), A.kl_divergence(cover_h, ref).sum(axis=1)
        pm_pos, pm_neg = A.peak_mass(sh, alpha).sum(axis=1), A.peak_mass(cover_h, alpha).sum(axis=1)
        res["payload_%d" % (plen - 16)] = {"payload_bytes": plen - 16, "stream_bits": 912 + 56 * plen, "n": int(n),
                                           "auc_spam_fld_folds": folds, "auc_kl": round(A.auc(kl_pos, kl_neg), 4),
                                           "auc_peak": round(A.auc(pm_pos, pm_neg), 4)}
    return {"image": [w, h], "covers": "synth.cover_rgb (synthetic, not photographs)", "alpha": alpha, "density": 0.7, "features": "SPAM-686, T = 3",
            "classifier": "Fisher linear discriminant, ridge 1e-3, fitted on one half and scored on the other", "n_ref": n_ref, "cells": res}


def robust(rounds, steps, warmup, plen=PLEN):
    import torch
    from steganosaurus_amd import analysis as A
    from steganosaurus_amd import binding as B
    from steganosaurus_amd.synth import cover_rgb
    w, h, nimg, slots = 1920, 1080, 32, 16
    n_bins = 912 + 56 * plen
    bins = B.Walk(bytes(range(32)), next_pow2(h), next_pow2(w)).next(n_bins)
    sbins, idx = B.bins_sort(bins)
    dev = "cuda:0"
    covers = torch.from_numpy(np.stack([cover_rgb(w, h, i) for i in range(nimg)])).to(dev)
    stego = torch.empty_like(covers)
    scratch = torch.empty_like(covers)
    d_bins = torch.from_numpy(sbins.view(np.uint8).reshape(-1, 8).copy()).to(dev)
    rng = np.random.default_rng(0)
    d_hdr = torch.from_numpy(np.tile(header(plen), nimg)).to(dev)
    d_pay = torch.from_numpy(rng.integers(0, 256, nimg * plen).astype(np.uint8)).to(dev)
    o_hdr = torch.empty(nimg * 38, dtype=torch.uint8, device=dev)
    o_pay = torch.empty(nimg * plen, dtype=torch.uint8, device=dev)
    o_st = torch.empty(nimg, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = B.Context(w, h, slots=slots)
    ctx.set_bit_index(idx)
    ctx.bins_register_dev(d_bins.data_ptr(), n_bins)
    ctx.embed_stream_batch_dev(nimg, covers.data_ptr(), w, h, d_bins.data_ptr(), n_bins, d_hdr.data_ptr(), d_pay.data_ptr(), plen, stego.data_ptr())
    ctx.sync()
    rows = [("none",)] + [("awgn", s, 1) for s in (0.5, 1.0, 2.0, 4.0, 8.0)] + [("jpeg", q) for q in (95, 90, 75, 50)]
    d_res = torch.empty(len(rows) * nimg * 4, dtype=torch.int32, device=dev)

    def rb(chs):
        ctx.robustness_batch_dev(nimg, stego.data_ptr(), w, h, d_bins.data_ptr(), n_bins, d_hdr.data_ptr(), d_pay.data_ptr(), plen, chs, d_res.data_ptr())
    rb(rows)
    ctx.sync()
    r = d_res.cpu().numpy().view(np.uint32).reshape(len(rows), nimg, 4)
    table = {}
    for k, ch in enumerate(rows):
        name = ":".join(str(v) for v in ch[:2])
        table[name] = {"raw_ber": round(float(A.raw_ber(r[k], plen).mean()), 6), "byte_error_rate": round(float(A.byte_error_rate(r[k], plen).mean()), 6),
                       "recovered_share": round(float(A.recovered(r[k], plen).mean()), 4)}
    legs = {
        "extract_stream": lambda: ctx.extract_stream_batch_dev(nimg, stego.data_ptr(), w, h, d_bins.data_ptr(), n_bins, o_hdr.data_ptr(),
                                                               o_pay.data_ptr(), plen, o_st.data_ptr()),
        "channel_awgn": lambda: ctx.channel_batch_dev(nimg, stego.data_ptr(), w, h, ("awgn", 2.0, 1), scratch.data_ptr()),
        "channel_jpeg": lambda: ctx.channel_batch_dev(nimg, stego.data_ptr(), w, h, ("jpeg", 75), scratch.data_ptr()),
        "robust_none": lambda: rb([("none",)]),
        "robust_awgn": lambda: rb([("awgn", 2.0, 1)]),
        "robust_jpeg": lambda: rb([("jpeg", 75)]),
        "robust_all_%d" % len(rows): lambda: rb(rows),
    }
    ms = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg, fn in legs.items():
            for _ in range(warmup):
                fn()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            ctx.sync()
            ms[leg].append((time.perf_counter() - t0) * 1e3 / steps)
    ctx.close()
    out = {leg: {"ms_per_call": round(statistics.median(v), 4), "ms_all_rounds": [round(x, 4) for x in v]} for leg, v in ms.items()}
    base = out["extract_stream"]["ms_per_call"]
    for leg in legs:
        out[leg]["vs_extract"] = round(out[leg]["ms_per_call"] / base, 4)
    return {"image": [w, h], "images_per_call": nimg, "slots": slots, "covers": "synth.cover_rgb (synthetic, not photographs)", "alpha": 0.5,
            "density": 0.7, "payload_bytes": plen, "table": table, "legs": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robust", action="store_true")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--auc", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workloads", default="1080p,4k")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--n-ref", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--spam", action="store_true")
    ap.add_argument("--payload", default=None, help="ciphertext bytes per image (the tag adds 16): --auc one value (default 4096), "
                                                    "--spam a comma list (default 4096,512,64)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    torch.zeros(1, device="cuda")
    res = {"tool": "stealth_eval"}
    if a.cost:
        res["cost"] = {wl: cost(wl, a.rounds, a.steps, a.warmup) for wl in a.workloads.split(",")}
    if a.auc:
        res["auc"] = auc_cells(a.n, a.n_ref, a.chunk, a.seed, int(a.payload or 4096) + 16)
    if a.spam:
        res["spam"] = spam_cells(a.n, a.n_ref, a.chunk, a.seed, [int(v) + 16 for v in (a.payload or "4096,512,64").split(",")])
    if a.robust:
        res["robust"] = robust(a.rounds, a.steps, a.warmup)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
