#!/usr/bin/env python3
"""tools/walks_cost.py -- cost of one walk per image (tfft_*_stream_batch_walks_dev) against one registered shared list on one MI355X.

Round trip = a stream embed with capacities (usable_out) + a stream extraction of a 4 KB payload's stream, 32 x 1080p and 8 x 4K per
call.  Variants, ALTERNATED inside one process (round r runs each once, so that clock and thermal drift fall on all alike):
  shared      tfft_embed_stream_batch_dev / tfft_extract_stream_batch_dev over ONE registered, address-ordered list (bit index set)
  walks       the per-image calls over n distinct walks in walk order (no jitter)
  walks+phase the same with per-image jitter 0.05 and adaptive alpha
Device time per round trip from the HIP event pair of tfft_timer_begin / tfft_timer_end (the per-image calls synchronise at their end
to report out-of-grid bins: that gap is inside the figure).  Also the host side: one walk (tfft_walk_create + next + jitter) and
tfft_walks_build over all images with 16 threads, and the PCIe bytes per image of the host forms.  Prints one JSON line.

    python tools/walks_cost.py [--rounds 5] [--steps 5] [--workloads 1080p,4k]
Under rocprofv3 (--kernel-trace --stats) run it with --rounds 1 --steps 2: the per-image kernels are k_bucket_count_walks,
k_bucket_fill_walks, k_gather_*_walks and the k_fft_cols instantiations with PI = true."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"1080p": (1920, 1080, 32), "4k": (3840, 2160, 8)}
VARIANTS = ("shared", "walks", "walks+phase")
PLEN = 4096 + 16


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def run(name, rounds, steps, warmup, threads):
    import torch
    from steganosaurus_amd import binding as B
    from steganosaurus_amd.synth import cover_rgb
    w, h, nimg = WORKLOADS[name]
    ph, pw = next_pow2(h), next_pow2(w)
    n_stream = 912 + 56 * PLEN
    n_bins = n_stream + n_stream // 4
    # host side: one walk the sequential way, then every image's on the thread pool
    keys = b"".join(hashlib.sha256(b"walks_cost %d %d" % (i, j)).digest() for i in range(nimg) for j in range(4))
    t0 = time.perf_counter()
    one = B.Walk(keys[:32], ph, pw).next(n_bins)
    B.walk_jitter(keys[32:128], one, 0.05)
    t_one = time.perf_counter() - t0
    t0 = time.perf_counter()
    wb, wj, st = B.walks_build(keys, ph, pw, n_bins, max_jitter=0.05, n_threads=threads)
    t_all = time.perf_counter() - t0
    assert (st == 0).all()
    sbins, idx = B.bins_sort(one)
    dev = "cuda:0"
    covers = torch.from_numpy(cover_rgb(w, h, 0)).unsqueeze(0).repeat(nimg, 1, 1, 1).contiguous().to(dev)
    d_shared = torch.from_numpy(sbins.view(np.uint8).reshape(-1, 8).copy()).to(dev)
    d_walks = torch.from_numpy(wb.view(np.uint8).reshape(-1, 8).copy()).to(dev)
    d_jit = torch.from_numpy(wj).to(dev)
    hdr = torch.from_numpy(np.frombuffer(b"FTTG\x02\x00" + bytes(28) + PLEN.to_bytes(4, "big"), np.uint8).copy()).repeat(nimg).to(dev)
    pay = torch.randint(0, 256, (nimg, PLEN), dtype=torch.uint8, device=dev)
    d_out = torch.empty_like(covers)
    d_us = torch.empty(nimg, dtype=torch.int64, device=dev)
    d_h = torch.empty((nimg, 38), dtype=torch.uint8, device=dev)
    d_p = torch.empty((nimg, PLEN), dtype=torch.uint8, device=dev)
    d_s = torch.empty(nimg, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx_s = B.Context(w, h, slots=nimg)
    ctx_s.set_bit_index(idx)
    ctx_s.bins_register_dev(d_shared.data_ptr(), n_bins)
    ctx_w = B.Context(w, h, slots=nimg)

    def step(v):
        if v == "shared":
            ctx_s.embed_stream_batch_dev(nimg, covers.data_ptr(), w, h, d_shared.data_ptr(), n_bins, hdr.data_ptr(), pay.data_ptr(), PLEN,
                                         d_out.data_ptr(), usable_ptr=d_us.data_ptr())
            ctx_s.extract_stream_batch_dev(nimg, d_out.data_ptr(), w, h, d_shared.data_ptr(), n_bins, d_h.data_ptr(), d_p.data_ptr(), PLEN,
                                           d_s.data_ptr())
            return
        jp = d_jit.data_ptr() if v == "walks+phase" else None
        ad = v == "walks+phase"
        ctx_w.embed_stream_batch_walks_dev(nimg, covers.data_ptr(), w, h, d_walks.data_ptr(), jp, n_bins, hdr.data_ptr(), pay.data_ptr(), PLEN,
                                           d_out.data_ptr(), adaptive=ad, usable_ptr=d_us.data_ptr())
        ctx_w.extract_stream_batch_walks_dev(nimg, d_out.data_ptr(), w, h, d_walks.data_ptr(), jp, n_bins, d_h.data_ptr(), d_p.data_ptr(), PLEN,
                                             d_s.data_ptr(), adaptive=ad)

    ms = {v: [] for v in VARIANTS}
    for _ in range(rounds):
        for v in VARIANTS:
            ctx = ctx_s if v == "shared" else ctx_w
            for _ in range(warmup):
                step(v)
            ctx.sync()
            ctx.timer_begin()
            for _ in range(steps):
                step(v)
            ms[v].append(ctx.timer_end() / steps)
    ctx_s.close()
    ctx_w.close()
    mpix = w * h * nimg / 1e6
    out = {}
    for v in VARIANTS:
        med = statistics.median(ms[v])
        out[v] = {"ms_per_round_trip": round(med, 4), "MPixels_per_s": round(mpix / (med / 1e3), 1), "ms_all_rounds": [round(x, 4) for x in ms[v]]}
    for v in VARIANTS:
        out[v]["vs_shared"] = round(out[v]["ms_per_round_trip"] / out["shared"]["ms_per_round_trip"], 4)
    return {"image": [w, h], "images_per_call": nimg, "n_bins": n_bins, "variants": out,
            "host": {"one_walk_plus_jitter_s": round(t_one, 4), "walks_build_s": round(t_all, 4), "walks_build_threads": threads,
                     "walks_build_s_per_image": round(t_all / nimg, 4)},
            "pcie_bytes_per_image": {"pixels": w * h * 3, "list": 8 * n_bins, "jitter": 4 * n_bins, "frame": 38 + PLEN}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--workloads", default="1080p,4k")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    torch.zeros(1, device="cuda")
    res = {wl: run(wl, a.rounds, a.steps, a.warmup, min(a.threads, 16)) for wl in a.workloads.split(",")}
    print(json.dumps({"tool": "walks_cost", "rounds": a.rounds, "steps": a.steps, "workloads": res}))


if __name__ == "__main__":
    main()
