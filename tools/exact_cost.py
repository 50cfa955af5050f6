#!/usr/bin/env python3
"""tools/exact_cost.py -- cost of the exact batched capacities (tfft_set_batch_exact) on one MI355X.

One call = tfft_embed_stream_batch_dev of a 4 KB payload's stream with capacities (usable_out), 32 x 1080p (16 slots: two chunks) and
8 x 4K centred per call.  Legs, ALTERNATED inside one process (round r runs each once, so that clock and thermal drift fall on all alike):
  off        mode OFF (the default: fp32 counts)
  near_none  mode NEAR, guard 64: no image's count lies near the 230 k-bit stream, so only the one read of the counts per chunk is added
  near_all   mode NEAR with a guard that takes every image: the cost of settling through the NEAR selection
  all        mode ALL
Wall time per call (the settle synchronises, so device-event timing would miss the host part), median over rounds.  A traced call per
leg (TFFT_BATCH_EXACT_TRACE=1) prints the rounds and the largest candidate list per plane of each chunk on stderr; the states go into the
JSON line.

    python tools/exact_cost.py [--rounds 5] [--steps 3] [--workloads 1080p,4k]"""
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
LEGS = {"off": (0, 64), "near_none": (2, 64), "near_all": (2, 1 << 62), "all": (1, 64)}
PLEN = 4096 + 16


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def run(name, rounds, steps, warmup):
    import torch
    from steganosaurus_amd import binding as B
    from steganosaurus_amd.synth import cover_rgb, gradient_cover
    w, h, nimg, slots, center = WORKLOADS[name]
    ph, pw = next_pow2(h), next_pow2(w)
    n_bins = 912 + 56 * PLEN
    bins = B.Walk(bytes(range(32)), ph, pw).next(n_bins)
    dev = "cuda:0"
    covers = torch.from_numpy(np.stack([cover_rgb(w, h, i) if i % 2 else gradient_cover(w, h, i) for i in range(nimg)])).to(dev)
    d_bins = torch.from_numpy(bins.view(np.uint8).reshape(-1, 8).copy()).to(dev)
    hdr = torch.from_numpy(np.frombuffer(b"FTTG\x02\x00" + bytes(28) + PLEN.to_bytes(4, "big"), np.uint8).copy()).repeat(nimg).to(dev)
    pay = torch.randint(0, 256, (nimg, PLEN), dtype=torch.uint8, device=dev)
    d_out = torch.empty_like(covers)
    d_us = torch.empty(nimg, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctxs = {}
    for leg, (mode, guard) in LEGS.items():
        ctxs[leg] = B.Context(w, h, slots=slots)
        ctxs[leg].set_batch_exact(mode, guard)

    def step(ctx):
        ctx.embed_stream_batch_dev(nimg, covers.data_ptr(), w, h, d_bins.data_ptr(), n_bins, hdr.data_ptr(), pay.data_ptr(), PLEN,
                                   d_out.data_ptr(), center=center, usable_ptr=d_us.data_ptr())

    ms = {leg: [] for leg in LEGS}
    for _ in range(rounds):
        for leg, ctx in ctxs.items():
            for _ in range(warmup):
                step(ctx)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(ctx)
            ctx.sync()
            ms[leg].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {}
    for leg, ctx in ctxs.items():
        out[leg] = {"ms_per_call": round(statistics.median(ms[leg]), 4), "ms_all_rounds": [round(x, 4) for x in ms[leg]],
                    "states": ctx.batch_exact_info(nimg).tolist()}
        ctx.close()
    for leg in LEGS:
        out[leg]["vs_off"] = round(out[leg]["ms_per_call"] / out["off"]["ms_per_call"], 4)
    # one traced call per settling leg (rounds, candidates per plane on stderr) and the counts it changes
    res_u = {}
    for leg in ("off", "all"):
        os.environ["TFFT_BATCH_EXACT_TRACE"] = "1"
        try:
            ctx = B.Context(w, h, slots=slots)
        finally:
            del os.environ["TFFT_BATCH_EXACT_TRACE"]
        ctx.set_batch_exact(*LEGS[leg])
        print("[%s %s]" % (name, leg), file=sys.stderr, flush=True)
        step(ctx)
        ctx.sync()
        res_u[leg] = d_us.cpu().numpy().astype(np.int64)
        ctx.close()
    diff = np.abs(res_u["all"] - res_u["off"])
    return {"image": [w, h], "images_per_call": nimg, "slots": slots, "center": center, "n_stream_bits": n_bins, "legs": out,
            "fp32_minus_exact": {"max_abs": int(diff.max()), "images_changed": int((diff > 0).sum())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workloads", default="1080p,4k")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    torch.zeros(1, device="cuda")
    res = {wl: run(wl, a.rounds, a.steps, a.warmup) for wl in a.workloads.split(",")}
    print(json.dumps({"tool": "exact_cost", "rounds": a.rounds, "steps": a.steps, "workloads": res}))


if __name__ == "__main__":
    main()
