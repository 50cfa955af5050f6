#!/usr/bin/env python3
"""tools/fit_cost.py -- what the fitted embed (tfft_embed_stream_batch_fit_dev) costs against the one-shot walks embed on one MI355X.

32 x 1080p and 8 x 4K per call, distinct keys, a payload near half the smallest capacity of the batch (usable_out of a first walks embed),
synthetic photo-like covers (synth.cover_rgb) or smooth gradients.  Per workload and cover kind: corrections to converge (iters_out),
device ms per batch call (the HIP event pair of tfft_timer_begin / tfft_timer_end; the fitted call synchronises once per iteration, that
gap is inside the figure), PSNR of the stego against its cover, and the images the library's walks reader decodes.  Variants alternate
inside one process.  Prints one JSON line.

    python tools/fit_cost.py [--rounds 3] [--workloads 1080p,4k] [--kinds synthetic,gradient] [--fill 0.5]"""
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


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def gradient(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 40 + 90 * x / (w - 1) + 60 * y / (h - 1)
    img = np.stack([base + 10 * c for c in range(3)], axis=-1) + rng.normal(0, 2, (h, w, 3)).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def psnr(a, b):
    m = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if m == 0 else 10 * np.log10(255.0 ** 2 / m)


def run(name, kind, rounds, fill, max_iters, threads):
    import torch
    from steganosaurus_amd import binding as B
    from steganosaurus_amd.synth import cover_rgb
    w, h, nimg = WORKLOADS[name]
    ph, pw = next_pow2(h), next_pow2(w)
    dev = "cuda:0"
    host_covers = np.stack([cover_rgb(w, h, 10 + i) if kind == "synthetic" else gradient(w, h, 10 + i) for i in range(nimg)])
    covers = torch.from_numpy(host_covers).to(dev)
    keys = b"".join(hashlib.sha256(b"fit_cost %d %d" % (i, j)).digest() for i in range(nimg) for j in range(4))
    ctx = B.Context(w, h, slots=nimg)
    d_out = torch.empty_like(covers)
    d_us = torch.zeros(nimg, dtype=torch.int64, device=dev)
    d_it = torch.zeros(nimg, dtype=torch.int32, device=dev)
    d_wr = torch.zeros(nimg, dtype=torch.int32, device=dev)

    def frames(plen):
        # (the header's length field counts the ciphertext; the payload is ciphertext || 16-byte tag)
        hdr = torch.from_numpy(np.frombuffer(b"FTTG\x02\x00" + bytes(28) + (plen - 16).to_bytes(4, "big"), np.uint8).copy()).repeat(nimg).to(dev)
        pay = torch.randint(0, 256, (nimg, plen), dtype=torch.uint8, device=dev)
        return hdr, pay

    # capacity of the batch: a walks embed of a minimal stream
    wb, _, st = B.walks_build(keys, ph, pw, 912 + 56 * 16, n_threads=threads)
    d_walks = torch.from_numpy(wb.view(np.uint8).reshape(-1, 8).copy()).to(dev)
    hdr, pay = frames(16)
    ctx.embed_stream_batch_walks_dev(nimg, covers.data_ptr(), w, h, d_walks.data_ptr(), None, wb.shape[1], hdr.data_ptr(), pay.data_ptr(), 16,
                                     d_out.data_ptr(), usable_ptr=d_us.data_ptr())
    ctx.sync()
    cap = int(d_us.min().item())
    plen = max(16, int((fill * cap - 912) // 56))
    n_bins = 912 + 56 * plen
    wb, _, st = B.walks_build(keys, ph, pw, n_bins, n_threads=threads)
    assert (st == 0).all()
    d_walks = torch.from_numpy(wb.view(np.uint8).reshape(-1, 8).copy()).to(dev)
    hdr, pay = frames(plen)
    d_h = torch.empty((nimg, 38), dtype=torch.uint8, device=dev)
    d_p = torch.empty((nimg, plen), dtype=torch.uint8, device=dev)
    d_s = torch.empty(nimg, dtype=torch.int32, device=dev)

    def embed(v):
        if v == "one_shot":
            ctx.embed_stream_batch_walks_dev(nimg, covers.data_ptr(), w, h, d_walks.data_ptr(), None, n_bins, hdr.data_ptr(), pay.data_ptr(),
                                             plen, d_out.data_ptr(), usable_ptr=d_us.data_ptr())
        else:
            ctx.embed_stream_batch_fit_dev(nimg, covers.data_ptr(), w, h, d_walks.data_ptr(), None, n_bins, hdr.data_ptr(), pay.data_ptr(),
                                           plen, d_out.data_ptr(), usable_ptr=d_us.data_ptr(), iters_ptr=d_it.data_ptr(),
                                           wrong_ptr=d_wr.data_ptr(), max_iters=max_iters)

    ms = {"one_shot": [], "fitted": []}
    res = {}
    for r in range(rounds + 1):             # round 0 warms up
        for v in ms:
            ctx.sync()
            ctx.timer_begin()
            embed(v)
            t = ctx.timer_end()
            if r:
                ms[v].append(t)
            if r == rounds:
                ctx.extract_stream_batch_walks_dev(nimg, d_out.data_ptr(), w, h, d_walks.data_ptr(), None, n_bins, d_h.data_ptr(), d_p.data_ptr(),
                                                   plen, d_s.data_ptr())
                ctx.sync()
                stego = d_out.cpu().numpy()
                ps = [psnr(stego[i], host_covers[i]) for i in range(nimg)]
                res[v] = {"ms_per_batch": round(statistics.median(ms[v]), 3), "ms_all_rounds": [round(x, 3) for x in ms[v]],
                          "psnr_db_mean": round(float(np.mean(ps)), 2), "psnr_db_min": round(float(np.min(ps)), 2),
                          "decoded": int((d_s.cpu().numpy() == plen - 16).sum())}
                if v == "fitted":
                    it = d_it.cpu().numpy()
                    res[v].update({"iters": it.tolist(), "iters_max": int(it.max()), "converged": int((it >= 0).sum()),
                                   "wrong_bits": d_wr.cpu().numpy().tolist()})
    ctx.close()
    res["fitted"]["vs_one_shot"] = round(res["fitted"]["ms_per_batch"] / res["one_shot"]["ms_per_batch"], 3)
    return {"image": [w, h], "images_per_call": nimg, "cover": kind, "min_usable_bits": cap, "n_bits": n_bins, "payload_bytes": plen,
            "variants": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default="1080p,4k")
    ap.add_argument("--kinds", default="synthetic,gradient")
    ap.add_argument("--fill", type=float, default=0.5)
    ap.add_argument("--max-iters", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    torch.zeros(1, device="cuda")
    out = [run(wl, k, a.rounds, a.fill, a.max_iters, min(a.threads, 16)) for wl in a.workloads.split(",") for k in a.kinds.split(",")]
    print(json.dumps({"tool": "fit_cost", "rounds": a.rounds, "fill": a.fill, "results": out}))


if __name__ == "__main__":
    main()
