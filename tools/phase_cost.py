#!/usr/bin/env python3
"""tools/phase_cost.py -- cost of the batched pipelines' phase options (tfft_set_phase_options) on one MI355X.

Round trip = tfft_embed_batch_dev (capacities asked for, as bench.py's step) + tfft_extract_batch_dev over a registered, address-ordered
bin list of a 4 KB payload's stream, 32 x 1080p and 8 x 4K per call.  The variants -- alpha only, jitter 0.05, adaptive alpha, both --
are ALTERNATED inside one process (round r times every variant once), so that clock and thermal drift fall on all of them alike.
Device time per round trip from the HIP event pair of tfft_timer_begin / tfft_timer_end.  Prints one JSON line.

    python tools/phase_cost.py [--rounds 5] [--steps 10] [--workloads 1080p,4k]
Under rocprofv3 (--kernel-trace --stats) run it with --rounds 1 --steps 3: the trace names COLS_EMBED / COLS_READ with the phase
options as their own instantiations (template argument PH = true) and k_gather_jitter."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"1080p": (1920, 1080, 32), "4k": (3840, 2160, 8)}
VARIANTS = (("alpha", 0.0, False), ("jitter", 0.05, False), ("adaptive", 0.0, True), ("jitter+adaptive", 0.05, True))


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def run(name, rounds, steps, warmup):
    import torch
    from steganosaurus_amd import binding as B
    from steganosaurus_amd.synth import cover_rgb
    w, h, nimg = WORKLOADS[name]
    n_stream = 912 + 56 * (4096 + 16)
    n_bins = n_stream + n_stream // 4
    key = hashlib.sha256(b"phase_cost").digest()
    bins = B.Walk(key, next_pow2(h), next_pow2(w)).next(n_bins)
    keys_rgb = hashlib.sha256(b"phase_cost rgb").digest() * 3
    jit = B.walk_jitter(keys_rgb, bins, 0.05)          # stream order, before the sort
    sbins, idx = B.bins_sort(bins)
    one = torch.from_numpy(cover_rgb(w, h, 0))
    covers = one.unsqueeze(0).repeat(nimg, 1, 1, 1).contiguous().to("cuda:0")
    d_bins = torch.from_numpy(sbins.view(np.uint8).reshape(-1, 8).copy()).to("cuda:0")
    d_bits = torch.randint(0, 2, (nimg, n_bins), dtype=torch.uint8, device="cuda:0")
    d_out = torch.empty_like(covers)
    d_raw = torch.empty((nimg, n_bins), dtype=torch.uint8, device="cuda:0")
    d_us = torch.empty(nimg, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx = B.Context(w, h, slots=nimg)
    ctx.set_bit_index(idx)
    ctx.bins_register_dev(d_bins.data_ptr(), n_bins)

    def step():
        ctx.embed_batch_dev(nimg, covers.data_ptr(), w, h, d_bins.data_ptr(), d_bits.data_ptr(), n_bins, d_out.data_ptr(),
                            usable_ptr=d_us.data_ptr())
        ctx.extract_batch_dev(nimg, d_out.data_ptr(), w, h, d_bins.data_ptr(), n_bins, d_raw.data_ptr())

    ms = {v[0]: [] for v in VARIANTS}
    for _ in range(rounds):
        for vname, jitter, adaptive in VARIANTS:
            ctx.set_phase_options(jit if jitter else None, adaptive)
            for _ in range(warmup):         # (the first call after the setter gathers the jitter into bucket order)
                step()
            ctx.sync()
            ctx.timer_begin()
            for _ in range(steps):
                step()
            ms[vname].append(ctx.timer_end() / steps)
    ctx.set_phase_options()
    ctx.close()
    mpix = w * h * nimg / 1e6
    out = {}
    for vname in ms:
        med = statistics.median(ms[vname])
        out[vname] = {"ms_per_round_trip": round(med, 4), "MPixels_per_s": round(mpix / (med / 1e3), 1),
                      "ms_all_rounds": [round(v, 4) for v in ms[vname]]}
    base = out["alpha"]["ms_per_round_trip"]
    for vname in ms:
        out[vname]["vs_alpha"] = round(out[vname]["ms_per_round_trip"] / base, 4)
    return {"image": [w, h], "images_per_call": nimg, "n_bins": n_bins, "variants": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default="1080p,4k")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    torch.zeros(1, device="cuda")
    res = {wl: run(wl, a.rounds, a.steps, a.warmup) for wl in a.workloads.split(",")}
    print(json.dumps({"tool": "phase_cost", "rounds": a.rounds, "steps": a.steps, "workloads": res}))


if __name__ == "__main__":
    main()
