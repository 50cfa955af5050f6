#!/usr/bin/env python3
"""bench.py -- MPixels/s of the embed+extract round trip (RGB 2-D FFT forward+inverse
+ keyed phase embed/extract) on MI355X, one process per GPU.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A "step" = one pass of the hot path over one batch of synthetic images that are already
resident in HBM, from packed bytes to packed bytes like do_embed / do_extract:
  embed   : header + payload bytes -> Rep-3/Rep-7 stream (device) -> forward FFT x3 -> medians + capacity
            -> keyed phase embed -> inverse FFT x3 -> u8 stego
  extract : stego -> forward FFT x3 -> raw bit of every position of the extractor's walk -> Rep-3 majority of the
            first 912 -> header -> clen -> Rep-7 majority of the payload (the length comes out of the image)
for every image of the per-GPU batch.  Images are independent, so ranks share nothing but the bin list
(broadcast once over RCCL before the timed region): weak scaling, no collective on the data path.

Prints ONE JSON line on rank 0 (contract in the task statement) with "roofline" (dominant kernel, HIP-event
timed, bytes = what the kernel has to move), "cpu_baseline" (+ parity of the GPU's image 0 against it) and
"other_workloads" (the 4K batch the north_star target is phrased on, and 8192^2).

--dump-outputs DIR writes what the last timed step of the workload computed to DIR/*.npy (dump_outputs); the inputs are
seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import hashlib
import hmac
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (W, H, secret_bytes, images_per_gpu, BASELINE.json config it corresponds to)
    "1080p_batch": (1920, 1080, 4096, 32, "configs[3] shard: 32 x (1920x1080 RGB, 4 KB payload) per GPU = configs[1] geometry"),
    "1080p_single": (1920, 1080, 4096, 1, "configs[1]: single 1920x1080 RGB, 4 KB payload"),
    "4k_single": (3840, 2160, 32768, 1, "configs[2]: single 3840x2160 RGB, 32 KB payload"),
    "4k_batch": (3840, 2160, 32768, 8, "8 x configs[2] (batched 4K UHD: the span north_star's >= 60 % target names)"),
    "8192_single": (8192, 8192, 131072, 1, "configs[4]: 8192x8192 RGB, 128 KB payload"),
    "512_single": (512, 512, 1024, 1, "configs[0]: 512x512 RGB, 1 KB secret"),
    "2048_batch": (2048, 2048, 4096, 16, "pow2 companion of configs[1] (SURVEY 8d): full payload recovery asserted"),
}
HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
C64 = 8                      # bytes per complex64 bin
WALK_SLACK = 1.25            # the extractor does not know the length: its walk is this much longer than the stream


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def survey_model_bytes(w, h, n_bits):
    """SURVEY.md 8(d) byte model (FULL complex64 planes, two passes per 2-D FFT).  Kept for reference only: this
    implementation stores the Hermitian half spectrum, so dividing these bytes by time is NOT a fraction of peak."""
    P = next_pow2(w) * next_pow2(h)
    b_embed = 3 * (6 * P * C64 + 2 * w * h) + 40 * n_bits
    b_extract = 3 * (3 * P * C64 + w * h) + 16 * n_bits
    return b_embed, b_extract


def kernel_bytes(stage, w, h, n_bits, n_bins, plan):
    """COMPULSORY HBM bytes of each kernel in this implementation's layout (Hermitian half spectrum of PH x PW/2 complex64 per
    plane; rows >= H never stored or loaded where they are known to be zero / not needed).  These are the algorithmic bytes
    `roofline.achieved` is computed from; rocprofv3 PMC traffic agrees with them within a few %."""
    PW, PH = max(2, next_pow2(w)), next_pow2(h)
    M = PW // 2
    plane_full = PH * M * C64
    plane_h = h * M * C64
    img = w * h
    mn = min(PH, next_pow2(w))
    bh = min(PH, int(0.45 * mn) + 1)
    bw = min(M, int(0.45 * mn) + 1)
    two_step = plan["two_step"]
    delta = plan.get("delta", False)
    if delta:
        # delta embedding: stego = cover + IFFT(F' - F).  k_embed is replaced by k_gather_bits (entry 8 B, bit 1 B
        # in, 1 B out); the last forward step also writes the listed bins' values (entry 8 B in, value 8 B out); the first inverse
        # step reads entry + value + bit instead of the spectrum and only WRITES its planes; the row kernel also reads the cover
        final_fwd = "cols_fwd_b" if two_step else "cols_fwd_a"
        if stage == "embed":
            return n_bits * (8 + 1 + 1)
        m2 = plan.get("m2", False)      # the spectrum is stored as |F|^2 (4 B per bin): all the statistics read, and nothing else reads it
        tile = plan.get("tile_stats", False)      # the statistics' full pass runs inside the last forward column step (COLS_STAT): nothing is stored
        cand = 3 * plane_full // 32               # but the candidate lists: 64 four-byte slots per wave and tile of 1024 values
        if tile and stage == final_fwd:
            return 3 * plane_full + cand + n_bits * (8 + 8)
        if tile and stage == "medians":           # the sample pass (a sixteenth of the plane) + two histogram passes over the candidate lists
            return 3 * plane_full // 16 + 2 * cand
        if stage == final_fwd and not (plan["fused"] and stage == "cols_fwd_a"):
            rd = (3 * plane_full) if two_step else 3 * plane_h
            if plan.get("no_store", False):      # no capacity asked for (--no-stats): nobody reads the spectrum, nothing is stored
                return rd + n_bits * (8 + 8)
            return rd + (3 * plane_full // 2 if m2 else 3 * plane_full) + n_bits * (8 + 8)
        if stage == "medians" and m2:
            return int(3 * (plane_full // 2) * (1 + 1.0 / 16))
        if stage == "cols_inv_a":
            return (3 * plane_full if two_step else 3 * plane_h) + n_bits * (8 + 8 + 1)
        if stage == "rows_inv":
            return (3 * plane_full if plan["fused"] else 3 * plane_h) + 6 * img
    if plan["fused"]:
        # fused kernels: u8 <-> full half-plane in one launch; the H x M intermediate never exists
        if stage == "rows_fwd":
            return 3 * img + 3 * plane_full
        if stage == "rows_inv":
            return 3 * plane_full + 3 * img
        if stage in ("cols_fwd_a", "cols_inv_b"):
            return 0
    return {
        "rows_fwd": 3 * img + 3 * plane_h,
        "cols_fwd_a": 3 * plane_h + 3 * plane_full,
        "cols_fwd_b": (6 * plane_full) if two_step else 0,
        "embed": n_bits * (8 + 1 + 8 + 8) + (n_bins - n_bits) * 12,
        "cols_inv_a": (6 * plane_full) if two_step else 3 * plane_full + 3 * plane_h,
        "cols_inv_b": (3 * plane_full + 3 * plane_h) if two_step else 0,
        "rows_inv": 3 * plane_h + 3 * img,
        "read": n_bins * (8 + 8 + 1),
        # one full read (bracket pass) + the 1/16-row sample; the candidate lists are a few 1e-3 of a plane
        "medians": int(3 * plane_full * (1 + 1.0 / 16)),
        # bounding box of the annulus: rows < bh, columns < bw of every plane
        "capacity": 3 * bh * bw * C64,
        # final forward column step of the extract path: reads everything, takes the bits out of its LDS-resident tiles
        "cols_fwd_read": 3 * plane_full + n_bins * (8 + 1),
    }[stage]


def stream_header(clen):
    """Header::to_bytes S:886-904 with the bench's fixed salt (bytes 0..15) and a zero nonce"""
    return np.frombuffer(b"FTTG" + bytes([2, 0]) + bytes(range(16)) + bytes(12) + int(clen).to_bytes(4, "big"), np.uint8).copy()


def rep_stream(header, payload):
    return np.concatenate([np.repeat(np.unpackbits(header), 3), np.repeat(np.unpackbits(payload), 7)])


class Workload:
    """inputs resident in HBM + a context; step() = embed batch + extract batch"""

    def __init__(self, name, torch, S, dev, local, rank, world, images=0, slots=0, stats=True, dist=None, backend="nccl", coll_dev=None):
        self.name, self.torch, self.S, self.dev, self.rank, self.world, self.stats = name, torch, S, dev, rank, world, stats
        W, H, secret, n_img, self.desc = WORKLOADS[name]
        if images > 0:
            n_img = images
        self.W, self.H, self.secret, self.n_img = W, H, secret, n_img
        from steganosaurus_amd.synth import cover_rgb, n_stream_bits
        self.n_bits = n_stream_bits(secret)
        self.plen = secret + 16
        self.n_bins = int(self.n_bits * WALK_SLACK)
        self.PW, self.PH = next_pow2(W), next_pow2(H)
        n_bits, n_bins = self.n_bits, self.n_bins
        covers = np.stack([cover_rgb(W, H, rank * n_img + i) for i in range(n_img)])
        self.covers = covers
        self.d_img = torch.from_numpy(covers).to(dev)
        rng = np.random.default_rng(1234 + rank)
        self.header = np.tile(stream_header(secret), (n_img, 1))
        self.payload = rng.integers(0, 256, size=(n_img, self.plen), dtype=np.uint8)
        self.d_header = torch.from_numpy(self.header).to(dev)
        self.d_payload = torch.from_numpy(self.payload).to(dev)
        self.d_bins = torch.empty((n_bins, 8), dtype=torch.uint8, device=dev)
        d_index = torch.zeros(n_bins, dtype=torch.int64, device=dev)
        self.sort_bins = os.environ.get("TFFT_BENCH_WALK_ORDER") != "1"      # "1": visit the bins in walk order (A/B knob)
        self.t_walk = self.t_sort = 0.0
        self.bins_walk = None
        if rank == 0:
            # host walk (sequential, content independent): computed once, shared by every image and rank
            pk = hashlib.sha256(b"test123").digest()
            key_walk = hmac.new(pk, b"turtle_keys" + b"\x01", hashlib.sha256).digest()     # HKDF-Expand first block (S:1054-1058)
            t0 = time.time()
            bins = S.Walk(key_walk, self.PH, self.PW).next(n_bins)
            self.t_walk = time.time() - t0
            self.bins_walk = bins
            if self.sort_bins:
                t0 = time.time()
                bins, bit_index = S.bins_sort(bins)
                self.t_sort = time.time() - t0
                d_index.copy_(torch.from_numpy(bit_index.astype(np.int64)))
            self.bins_used = bins
            self.d_bins.copy_(torch.from_numpy(bins.view(np.uint8).reshape(-1, 8).copy()))
        if world > 1:
            # the only collective: 8 B x n_bins (+ the bit index) over xGMI, before the timed region
            for tns in ((self.d_bins, d_index) if self.sort_bins else (self.d_bins,)):
                if backend == "nccl":
                    dist.broadcast(tns, src=0)
                else:
                    hb = tns.cpu()
                    dist.broadcast(hb, src=0)
                    tns.copy_(hb)
        self.d_stego = torch.empty_like(self.d_img)
        self.d_hdr_out = torch.zeros((n_img, 38), dtype=torch.uint8, device=dev)
        self.d_pay_out = torch.zeros((n_img, self.plen), dtype=torch.uint8, device=dev)
        self.d_status = torch.zeros(n_img, dtype=torch.int32, device=dev)
        self.d_usable = torch.zeros(n_img, dtype=torch.int64, device=dev)
        self.slots = max(1, min(slots if slots > 0 else 32, n_img))
        self.ctx = S.Context(W, H, slots=self.slots, device=local)
        self.plan = self.ctx.plan_info(W, H, min(self.slots, n_img))      # which kernels a launch over the chunk takes
        self.plan["delta"] = int(os.environ.get("TFFT_EMBED_DELTA", "1")) != 0      # the bin list is registered below: delta embedding applies
        PHp, PWp = next_pow2(H), max(2, next_pow2(W))
        # (tilestats_applies in tfft_capi.hip: two-step column plans of whole tiles, planes up to 2^24 bins; the default annulus stays left of PW/2)
        self.plan["tile_stats"] = (self.plan["delta"] and stats and int(os.environ.get("TFFT_STATS_TILE", "1")) != 0 and self.plan["two_step"]
                                   and 4 <= self.plan["log_n2"] <= 9 and PHp * PWp <= (1 << 24) and (PWp // 2) % 16 == 0
                                   and (min(self.slots, n_img) * PHp * PWp >= (1 << 24) or int(os.environ.get("TFFT_STATS_TILE", "1")) >= 2)
                                   and all(int(os.environ.get(k, "1")) != 0 for k in ("TFFT_STATS_FUSED", "TFFT_STATS_COMPACT"))
                                   and int(os.environ.get("TFFT_MEDIAN_FALLBACK", "0")) == 0)
        self.plan["m2"] = (self.plan["delta"] and stats and not self.plan["tile_stats"] and int(os.environ.get("TFFT_STATS_M2", "1")) != 0 and PHp * PWp <= (1 << 24))
        self.plan["no_store"] = self.plan["delta"] and not stats and int(os.environ.get("TFFT_STATS_M2", "1")) != 0
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self.h_index = d_index.cpu().numpy().astype(np.uint32) if self.sort_bins else None
        if self.sort_bins:
            self.ctx.set_bit_index(self.h_index)
        # the bin list does not change between calls: let the extraction keep its per-tile buckets (tfft_bins_register_dev)
        if os.environ.get("TFFT_BENCH_REGISTER_BINS", "1") != "0":
            self.ctx.bins_register_dev(self.d_bins.data_ptr(), n_bins)

    def embed(self, n=None):
        n = n or self.n_img
        self.ctx.embed_stream_batch_dev(n, self.d_img.data_ptr(), self.W, self.H, self.d_bins.data_ptr(), self.n_bins, self.d_header.data_ptr(),
                                        self.d_payload.data_ptr(), self.plen, self.d_stego.data_ptr(),
                                        usable_ptr=self.d_usable.data_ptr() if self.stats else None)

    def extract(self, n=None, raw_ptr=None, src=None):
        n = n or self.n_img
        self.ctx.extract_stream_batch_dev(n, (src if src is not None else self.d_stego).data_ptr(), self.W, self.H, self.d_bins.data_ptr(), self.n_bins,
                                          self.d_hdr_out.data_ptr(), self.d_pay_out.data_ptr(), self.plen, self.d_status.data_ptr(),
                                          raw_bits_out_ptr=raw_ptr)

    def step(self):
        self.embed()
        self.extract()

    def close(self):
        self.ctx.close()


def cross_path_check(wl, raw_batch):
    """Reference-free functional check of the kernels the timed step ran -- on EVERY workload and also with --no-cpu-baseline, so that
    an A/B run can never compare a broken kernel: the first and the last image of the batch go through the single-image calls of a second
    context (tfft_forward_rgb8_dev + tfft_embed_bins_dev + tfft_inverse_rgb8_dev, tfft_read_bins_dev: F' written into the stored
    spectrum and read back by k_read, for 4K a three-pass plan) and must give what the batched pipelines gave (delta embedding,
    tile-resident read, two-pass plan): raw bits equal but for rounding flips of bins whose imaginary part is ~0 (<= 1e-5 of the
    bits; a dropped tile alone would be 3e-4), stego bytes within 1 LSB on < 0.1 % of the pixels.  Asserted."""
    torch, S = wl.torch, wl.S
    W, H, n, nb = wl.W, wl.H, wl.n_bits, wl.n_bins
    sorted_bins = wl.d_bins.cpu().numpy().reshape(nb, 8)
    if wl.sort_bins:                     # sorted[j] carries stream bit h_index[j]: undo it -> walk (= stream) order
        walk = np.empty_like(sorted_bins)
        walk[wl.h_index.astype(np.int64)] = sorted_bins
    else:
        walk = sorted_bins
    d_walk = torch.from_numpy(np.ascontiguousarray(walk[:n])).to(wl.dev)
    d_out = torch.zeros(n, dtype=torch.uint8, device=wl.dev)
    d_img = torch.empty((H, W, 3), dtype=torch.uint8, device=wl.dev)
    g = S.Context(W, H, device=wl.dev.index or 0)
    bits_bad = px_bad = px_max = 0
    imgs = sorted({0, wl.n_img - 1})
    for i in imgs:
        g.forward_rgb8_dev(wl.d_stego[i].data_ptr(), W, H)
        g.read_bins_dev(d_walk.data_ptr(), n, d_out.data_ptr())
        g.sync()
        bits_bad += int((d_out.cpu().numpy() != raw_batch[i]).sum())
        d_bits = torch.from_numpy(np.ascontiguousarray(rep_stream(wl.header[i], wl.payload[i]))).to(wl.dev)
        g.forward_rgb8_dev(wl.d_img[i].data_ptr(), W, H)
        g.embed_bins_dev(d_walk.data_ptr(), d_bits.data_ptr(), n)
        g.inverse_rgb8_dev(d_img.data_ptr())
        g.sync()
        d = (d_img.to(torch.int16) - wl.d_stego[i].to(torch.int16)).abs()
        px_bad += int((d != 0).sum().item())
        px_max = max(px_max, int(d.max().item()))
    g.close()
    out = {"images": imgs, "raw_bit_mismatches": bits_bad, "bits": n * len(imgs), "stego_pixels_differing": px_bad,
           "stego_max_abs_diff": px_max, "pixel_values": W * H * 3 * len(imgs),
           "against": "the single-image calls of a second context (stored spectrum, k_embed / k_read, the single-image plan)"}
    out["ok"] = bool(bits_bad <= 1e-5 * out["bits"] and px_max <= 1 and px_bad < 1e-3 * out["pixel_values"])
    assert out["ok"], out
    return out


def timed(fn, steps, barrier):
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    barrier()
    return (time.perf_counter() - t0) / steps


def path_bytes(wl, span):
    """compulsory bytes of every kernel of the span ("roundtrip" | "embed"), per image"""
    fwd = ["rows_fwd", "cols_fwd_a", "cols_fwd_b"]
    e = fwd + (["medians", "capacity"] if wl.stats else []) + ["embed", "cols_inv_a", "cols_inv_b", "rows_inv"]
    x = ["rows_fwd", "cols_fwd_a", "cols_fwd_read"] if wl.plan["two_step"] else ["rows_fwd", "cols_fwd_read"]
    names = e if span == "embed" else e + x
    return sum(kernel_bytes(s, wl.W, wl.H, wl.n_bits, wl.n_bins, wl.plan) for s in names)


def profile_stages(wl, reps):
    """per-kernel timing with HIP events on the stream the kernels run on (tfft_profile_stage): each stage is ONE batched launch
    over the chunk of `slots` images, exactly as in the timed step"""
    torch, S, ctx = wl.torch, wl.S, wl.ctx
    slots = wl.slots
    rng = np.random.default_rng(99)
    d_bits = torch.from_numpy(rng.integers(0, 2, size=(slots, wl.n_bins), dtype=np.uint8)).to(wl.dev)
    d_raw = torch.zeros((slots, wl.n_bins), dtype=torch.uint8, device=wl.dev)
    ctx.forward_rgb8_dev(wl.d_img.data_ptr(), wl.W, wl.H)
    ctx.sync()
    stages = {}

    def prof(sid, r):
        return ctx.profile_stage(sid, r, wl.d_img.data_ptr(), wl.d_stego.data_ptr(), wl.d_bins.data_ptr(), d_bits.data_ptr(), d_raw.data_ptr(),
                                 wl.n_bins, n_images=slots)
    # the two-step column stages work in place, so repeating one of them destroys its input: time the forward stages first,
    # rebuild a clean spectrum, then time everything that reads the spectrum, and the inverse stages last
    for sid in [0, 1, 2, 10, "clean", 8, 9, 3, 7, 4, 5, 6]:
        if sid == "clean":
            for k in (0, 1, 2):
                prof(k, 1)
            continue
        name = S.Context.STAGES[sid]
        prof(sid, 1)            # untimed: first-launch costs (code object load, function attributes) stay out of the mean
        ms, nl = prof(sid, reps)
        if nl == 0:
            continue
        nb = wl.n_bins          # the profiled embed / read launches cover every position of the walk
        kb = kernel_bytes(name, wl.W, wl.H, nb, nb, wl.plan) * slots
        stages[name] = {"ms": round(ms, 5), "launches": nl, "images_per_launch": slots, "bytes": kb,
                        "GBs": round(kb / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
                        "frac": round(kb / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms > 0 else None,
                        "pmc_traffic_bytes": load_traffic(wl.name, name, slots)[0]}       # replayed from profiles/traffic.json (None: not captured)
        if name in ("embed", "read"):
            stages[name]["note"] = "scatter / gather of 8-byte bins: `bytes` are the bins themselves, the hardware moves whole 32/64-byte sectors (3-4x, see pmc_traffic_bytes)"
        if wl.plan["fused"] and name in ("rows_fwd", "rows_inv"):
            stages[name]["kernel"] = "rows + column step A fused" if name == "rows_fwd" else "column step B' + rows fused"
    return stages


def load_traffic(workload, stage, images_per_launch=None):
    """PMC bytes per launch captured by an earlier rocprofv3 run of the same command (tools/round_profiles.sh); only replayed
    when a launch of this run covers as many images as a launch of that one"""
    tf = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        t = json.load(open(tf))
        if images_per_launch is not None and t.get("_images_per_launch", {}).get(workload) != images_per_launch:
            return None, None
        v = t.get(workload, {}).get(stage)
        src = t.get("_source", {}).get(workload)
        return v, src
    except Exception:
        return None, None


def roofline_of(wl, stages, reps):
    fft = {k: v for k, v in stages.items() if k.startswith(("rows", "cols"))}
    dom = max(fft, key=lambda k: fft[k]["ms"])
    d = stages[dom]
    traffic, src = load_traffic(wl.name, dom, d["images_per_launch"])
    sm_e, sm_x = survey_model_bytes(wl.W, wl.H, wl.n_bits)
    note = None
    if wl.plan.get("m2") and dom in ("cols_fwd_a", "cols_fwd_b"):
        # the step's own byte count shrank late in round 2 (it stores |F|^2, 4 B per bin, instead of the complex spectrum): say what
        # the same launch time reads in the bytes it used to move, so that the drop in `frac` is not mistaken for a slower kernel
        plan_c = dict(wl.plan, m2=False)
        old_b = kernel_bytes(dom, wl.W, wl.H, wl.n_bins, wl.n_bins, plan_c) * d["images_per_launch"]
        note = ("this step stores |F|^2 (4 B per bin, all the statistics read) instead of the complex spectrum since profiles/r2g: %d B per launch instead of "
                "%d at the same speed; in the earlier byte count this launch time would read frac = %.3f.  The step is bound by its LDS exchanges and "
                "dependent issue, not by HBM (DESIGN.md section 5)" % (d["bytes"], old_b, old_b / (d["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS))
    return {"bound": "hbm", "kernel": dom, "note": note, "achieved": d["GBs"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": d["frac"],
            "traffic": traffic,
            "traffic_source": (src or "profiles/traffic.json") + " -- rocprofv3 PMC of an earlier run of this same command, replayed, not measured in this run"
            if traffic is not None else None,
            "algorithmic_bytes_per_launch": d["bytes"], "avg_launch_ms": d["ms"], "units_per_launch": d["images_per_launch"],
            "how": "slowest FFT kernel of the step.  achieved = bytes the kernel has to move (Hermitian half spectrum, DESIGN.md section 4) x images "
                   "per launch / mean launch time (HIP events on the launch stream, %d back-to-back launches); frac = achieved / 8 TB/s.  "
                   "SURVEY 8(d)'s full-complex-plane model would credit about twice these bytes and is not reported as a fraction" % reps}


def target_span(wl, res):
    """north_star: ">= 60 % of MI355X HBM-read roofline on batched 4K-UHD RGB forward+embed+inverse round-trip at 1 GPU".  Embed-only wall
    time of the 4k_batch workload (statistics included) in two byte models: the bytes the kernels of THIS layout have to move (Hermitian
    half spectrum, delta embedding, |F|^2 statistics plane: `frac_physical`) and SURVEY.md 8(d)'s fixed model (full complex planes, two
    passes per 2-D FFT: `frac_survey_8d`, which can exceed 1 because this layout moves about half of those bytes)."""
    e = res["path"]["embed_only"]
    sm_e, _ = survey_model_bytes(wl.W, wl.H, wl.n_bits)
    t = e["ms_per_step"] * 1e-3
    return {"workload": wl.name, "images_per_launch": wl.slots, "ms_embed_only": e["ms_per_step"], "MPixels_per_s_embed_only": e["MPixels_per_s"],
            "bytes_per_image_physical": e["bytes_per_image"], "frac_physical": e["frac_of_peak"],
            "bytes_per_image_survey_8d": sm_e, "frac_survey_8d": round(sm_e * wl.n_img / t / 1e9 / HBM_PEAK_GBS, 4),
            "ms_round_trip": res["ms_per_step"], "MPixels_per_s_round_trip": res["value"],
            "payloads": "non-power-of-two cover: raw bits identical to the reference's (cpu_baseline / tests), which does not round-trip these either",
            "target": 0.60}


DUMP_VALUES = 1 << 21       # values of one output that --dump-outputs keeps, summed over the ranks (a larger output is sampled)


def dump_positions(numel, k):
    """the fixed sample --dump-outputs keeps of a flattened output of numel > k values: seeded draws with replacement, deduplicated
    and sorted (host memory of the order of k)"""
    return np.unique(np.random.default_rng(0).integers(0, numel, k))


def dump_outputs(wl, out_dir, suffix=""):
    """--dump-outputs: what the last timed step handed its caller, as .npy files (bytes as float32, counts as float64) -- the stego
    images, the headers and payloads the extractor decoded, its status per image (the payload length it found) and the embed's
    capacities.  Each rank keeps at most k = DUMP_VALUES // world values of an output: a larger one is flattened and only its values at
    dump_positions(numel, k) are written, the same positions in every run.  So the files of all ranks together hold at most
    5 x DUMP_VALUES values (56 MiB) whatever --gpus; the default workload writes about 8.5 MiB at --gpus 1 and 12 MiB at --gpus 8."""
    torch = wl.torch
    os.makedirs(out_dir, exist_ok=True)
    k = DUMP_VALUES // wl.world
    outs = {"stego": wl.d_stego, "header_out": wl.d_hdr_out, "payload_out": wl.d_pay_out, "status": wl.d_status}
    if wl.stats:
        outs["usable_bits"] = wl.d_usable
    for name, t in outs.items():
        if t.numel() > k:
            t = t.reshape(-1)[torch.from_numpy(dump_positions(t.numel(), k)).to(t.device)]
        a = t.cpu().numpy()
        np.save(os.path.join(out_dir, name + suffix + ".npy"), a.astype(np.float32 if a.itemsize <= 2 else np.float64))


def run_workload(wl, steps, warmup, barrier, reduce_max, with_stages, stage_reps, single_leg, dump_dir=None):
    for _ in range(warmup):
        wl.step()
    dt = reduce_max(timed(wl.step, steps, barrier))
    if dump_dir:                # before the embed-only leg and the correctness read overwrite the step's outputs
        dump_outputs(wl, dump_dir, "_rank%d" % wl.rank if wl.world > 1 else "")
    dte = reduce_max(timed(wl.embed, steps, barrier))
    wl.ctx.sync()
    pix = wl.n_img * wl.W * wl.H
    b_rt, b_e = path_bytes(wl, "roundtrip"), path_bytes(wl, "embed")
    res = {"value": round(wl.world * pix / dt / 1e6, 1), "ms_per_step": round(dt * 1e3, 4),
           "path": {"roundtrip": {"bytes_per_image": b_rt, "GBs_per_gpu": round(b_rt * wl.n_img / dt / 1e9, 1),
                                  "frac_of_peak": round(b_rt * wl.n_img / dt / 1e9 / HBM_PEAK_GBS, 4)},
                    "embed_only": {"ms_per_step": round(dte * 1e3, 4), "MPixels_per_s": round(wl.world * pix / dte / 1e6, 1),
                                   "bytes_per_image": b_e, "GBs_per_gpu": round(b_e * wl.n_img / dte / 1e9, 1),
                                   "frac_of_peak": round(b_e * wl.n_img / dte / 1e9 / HBM_PEAK_GBS, 4)},
                    "note": "compulsory HBM bytes of every kernel of the span (half-spectrum layout, statistics included) / wall time / 8 TB/s"}}
    # ---- correctness inside the bench (untimed): the raw bits of the round trip, what the headers said, capacities
    torch = wl.torch
    d_raw = torch.zeros((wl.n_img, wl.n_bins), dtype=torch.uint8, device=wl.dev)
    wl.extract(raw_ptr=d_raw.data_ptr())
    wl.ctx.sync()
    raw = d_raw.cpu().numpy()[:, :wl.n_bits]
    want = np.stack([rep_stream(wl.header[i], wl.payload[i]) for i in range(wl.n_img)])
    status = wl.d_status.cpu().numpy()
    res["check"] = {"wrong_bits": int((raw != want).sum()), "bits": int(raw.size),
                    "headers_decoded": int((status == wl.secret).sum()),
                    "payloads_recovered": int(sum(status[i] == wl.secret and np.array_equal(wl.d_pay_out[i].cpu().numpy(), wl.payload[i]) for i in range(wl.n_img))),
                    "images": wl.n_img, "min_capacity_bits": int(wl.d_usable.min().item()) if wl.stats else None}
    res["check"]["cross_path"] = cross_path_check(wl, raw)
    if single_leg and wl.n_img > 1:
        for _ in range(3):
            wl.embed(1); wl.extract(1)
        t1 = timed(lambda: (wl.embed(1), wl.extract(1)), 20, lambda: torch.cuda.synchronize())
        res["single_image"] = {"value": round(wl.W * wl.H / t1 / 1e6, 1), "unit": "MPixels/s", "ms_per_image": round(t1 * 1e3, 4),
                               "note": "one image per call, same context"}
    if with_stages:
        res["stages"] = profile_stages(wl, stage_reps)
        res["roofline"] = roofline_of(wl, res["stages"], stage_reps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="1080p_batch", choices=sorted(WORKLOADS))
    ap.add_argument("--images", type=int, default=0, help="images per GPU (default: the workload's)")
    ap.add_argument("--slots", type=int, default=0, help="resident images per launch (default: the whole per-GPU batch, at most 32)")
    ap.add_argument("--no-stats", action="store_true", help="skip medians+capacity inside embed (not the default)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-others", action="store_true", help="skip the other_workloads legs (4k_batch, 8192_single)")
    ap.add_argument("--batched-only", action="store_true",
                    help="profiling runs: only the timed steps and the per-stage launches, so that every traced launch is a batched one")
    ap.add_argument("--stage-reps", type=int, default=20)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step of the workload computed to DIR/<name>.npy (seeded inputs: equal from run to run)")
    args = ap.parse_args()

    import torch
    import torch.distributed as dist
    import steganosaurus_amd as S

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback exists)"
    if world != args.gpus:
        # one process per GPU: N > 1 only exists under a launcher (python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N)
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE is %d: start it as `python -m torch.distributed.run --nnodes=1 --nproc-per-node %d "
                         "--master-addr 127.0.0.1 --master-port P bench.py --gpus %d ...` (a plain `python bench.py` measures one GPU)\n"
                         % (args.gpus, world, args.gpus, args.gpus))
        sys.exit(2)
    # rehearsal knobs for a one-GPU box: TFFT_BENCH_BACKEND=gloo runs the collectives on CPU copies and
    # TFFT_BENCH_SHARE_GPU=1 puts every rank on GPU 0 (the driver's multi-GPU runs use neither)
    backend = os.environ.get("TFFT_BENCH_BACKEND", "nccl")
    if os.environ.get("TFFT_BENCH_SHARE_GPU") == "1":
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)      # "nccl" is RCCL on ROCm
        else:
            dist.init_process_group(backend=backend)
    coll_dev = dev if backend == "nccl" else torch.device("cpu")
    stream = torch.cuda.Stream(device=dev)          # the contexts run on this torch-visible HIP stream
    torch.cuda.set_stream(stream)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def reduce_max(v):
        if world > 1:
            t = torch.tensor([v], dtype=torch.float64, device=coll_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        return v

    wl = Workload(args.workload, torch, S, dev, local, rank, world, args.images, args.slots, not args.no_stats, dist, backend, coll_dev)
    # every rank runs the same legs (timed steps, embed-only, correctness read); rank 0 alone adds the per-stage launches
    res = run_workload(wl, args.steps, args.warmup, barrier, reduce_max, with_stages=(rank == 0), stage_reps=args.stage_reps,
                       single_leg=(rank == 0 and not args.batched_only), dump_dir=args.dump_outputs)
    chk = res["check"]
    if world > 1:
        acc = torch.tensor([float(chk["wrong_bits"]), float(chk["bits"]), float(chk["headers_decoded"]), float(chk["payloads_recovered"]),
                            float(chk["images"])], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        chk["wrong_bits"], chk["bits"], chk["headers_decoded"], chk["payloads_recovered"], chk["images"] = (int(v) for v in acc.tolist())
        if chk["min_capacity_bits"] is not None:
            um = torch.tensor([float(chk["min_capacity_bits"])], dtype=torch.float64, device=coll_dev)
            dist.all_reduce(um, op=dist.ReduceOp.MIN)
            chk["min_capacity_bits"] = int(um.item())
    chk["roundtrip_ber"] = chk["wrong_bits"] / max(1, chk["bits"])
    pow2 = (wl.PW, wl.PH) == (wl.W, wl.H)
    chk["note"] = ("power-of-two cover: every header decodes and every payload byte comes back" if pow2 else
                   "non-power-of-two cover: the REFERENCE does not round-trip these either (raw BER ~0.31, 'Magic not found.', SURVEY finding 1); "
                   "parity with it is checked on image 0 under cpu_baseline.parity_vs_reference")
    if pow2:
        assert chk["payloads_recovered"] == chk["images"], chk

    out = {
        "metric": "MPixels/s embed+extract round-trip (RGB 2D-FFT fwd+inv)",
        "value": res["value"], "unit": "MPixels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": res["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": args.workload, "describes": wl.desc, "image": [wl.W, wl.H], "padded": [wl.PW, wl.PH],
                   "payload_bytes": wl.secret, "stream_bits": wl.n_bits, "walk_positions": wl.n_bins,
                   "images_per_gpu": wl.n_img, "images_per_launch": wl.slots, "stats_in_embed": wl.stats,
                   "dc_removal": os.environ.get("TFFT_DC_BIAS", "128") != "0",
                   "parallelism": "independent images per rank, no data-path collective",
                   "host_walk_s": round(wl.t_walk, 3),
                   "bin_order": "address order (tfft_bins_sort + tfft_set_bit_index)" if wl.sort_bins else "walk order",
                   "host_sort_s": round(wl.t_sort, 3),
                   "step": "packed bytes -> stego -> packed bytes: device framing, statistics, and the extractor learns the payload length from the header"},
        "check": chk, "path": res["path"],
    }
    if rank == 0:
        out["single_image"] = res.get("single_image")
        out["roofline"] = res["roofline"]
        out["stages"] = res["stages"]
        if world == 1 and not args.batched_only:
            out["pcie_inclusive"] = pcie_leg(wl, torch)
        if world == 1 and not args.batched_only:
            out["png_inclusive"] = png_leg(wl, torch)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(wl, S)
    wl.close()
    if rank == 0:
        out["roofline"]["target_span"] = target_span(wl, res) if args.workload == "4k_batch" else None
    if rank == 0 and world == 1 and not args.batched_only and not args.no_others and args.workload == "1080p_batch":
        others = {}
        for name in ("4k_batch", "8192_single", "1080p_single", "4k_single"):
            w2 = Workload(name, torch, S, dev, local, 0, 1, 0, 0, True)
            big = w2.n_img > 1 or name == "8192_single"
            r2 = run_workload(w2, 5 if big else 20, 2 if big else 5, barrier, reduce_max, with_stages=big, stage_reps=10, single_leg=False)
            others[name] = {"describes": w2.desc, "value": r2["value"], "unit": "MPixels/s", "ms_per_step": r2["ms_per_step"], "steps": 5 if big else 20,
                            "warmup": 2 if big else 5, "images_per_launch": w2.slots, "path": r2["path"], "check": r2["check"]}
            if big:
                others[name].update({"roofline": {k: r2["roofline"][k] for k in ("kernel", "achieved", "frac", "avg_launch_ms", "traffic")},
                                     "stages_ms": {k: v["ms"] for k, v in r2["stages"].items()},
                                     "stages_frac": {k: v["frac"] for k, v in r2["stages"].items()}})
            if name == "4k_batch":
                # the span north_star's >= 60 % target is phrased on rides INSIDE the roofline object (the driver keeps that whole)
                out["roofline"]["target_span"] = target_span(w2, r2)
            w2.close()
        out["other_workloads"] = others
        out["roofline"]["single_image_ms_per_round_trip"] = {k: others[k]["ms_per_step"] for k in ("1080p_single", "4k_single")}
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.barrier()          # rank 0 did its extra per-kernel profiling while the others waited here
        dist.destroy_process_group()


def pcie_leg(wl, torch):
    """side figure, never `value`: the same step when the caller hands over HOST buffers (pinned): tfft_embed_stream_batch /
    tfft_extract_stream_batch overlap the PCIe copies with the kernels on three streams; covers and stego images cross the bus
    as u8, the streams as packed bytes (38 + payload bytes per image in, header + payload + a status word out)"""
    import ctypes as C
    n_img, W, H = wl.n_img, wl.W, wl.H
    bins = np.ascontiguousarray(wl.bins_walk)
    ctx = wl.S.Context(W, H, slots=wl.slots, device=wl.dev.index or 0)
    h_img = torch.from_numpy(wl.covers).pin_memory()
    h_hdr = torch.from_numpy(wl.header).pin_memory()
    h_pay = torch.from_numpy(wl.payload).pin_memory()
    h_stego = torch.empty(h_img.shape, dtype=torch.uint8).pin_memory()
    h_hdr2 = torch.zeros(h_hdr.shape, dtype=torch.uint8).pin_memory()
    h_pay2 = torch.zeros(h_pay.shape, dtype=torch.uint8).pin_memory()
    h_st = torch.zeros(n_img, dtype=torch.int32).pin_memory()
    h_us = torch.zeros(n_img, dtype=torch.int64).pin_memory()
    lib, hnd = ctx.lib, ctx.h

    def host_step():
        rc = lib.tfft_embed_stream_batch(hnd, n_img, C.c_void_p(h_img.data_ptr()), W, H, 0, C.c_void_p(bins.ctypes.data), len(bins),
                                         C.c_void_p(h_hdr.data_ptr()), C.c_void_p(h_pay.data_ptr()), wl.plen, 0.5, 0.05, 0.45, 0.01,
                                         C.c_void_p(h_us.data_ptr()) if wl.stats else None, C.c_void_p(h_stego.data_ptr()))
        assert rc == 0, rc
        rc = lib.tfft_extract_stream_batch(hnd, n_img, C.c_void_p(h_stego.data_ptr()), W, H, 0, C.c_void_p(bins.ctypes.data), len(bins), 0.5,
                                           C.c_void_p(h_hdr2.data_ptr()), C.c_void_p(h_pay2.data_ptr()), wl.plen, C.c_void_p(h_st.data_ptr()), None)
        assert rc == 0, rc
    host_step()
    t0 = time.perf_counter()
    for _ in range(3):
        host_step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    wl.embed()                      # (the per-stage launches above used d_stego as their scratch output)
    wl.ctx.sync()
    same = bool((h_stego.numpy() == wl.d_stego.cpu().numpy()).all())
    ctx.close()
    return {"value": round(n_img * W * H / dt / 1e6, 1), "unit": "MPixels/s", "ms_per_step": round(dt * 1e3, 3),
            "with_cold_host_walk": round(n_img * W * H / (dt + wl.t_walk + wl.t_sort) / 1e6, 1),
            "stego_identical_to_resident_run": same,
            "note": "pinned host buffers through tfft_embed_stream_batch / tfft_extract_stream_batch: H2D of covers and packed stream bytes, "
                    "kernels and D2H of stego / header / payload / status overlapped on three HIP streams"}


def png_leg(wl, torch):
    """side figure, never `value`: PNG FILES in, PNG files out -- libtfpipe.so inflates the covers on worker threads into
    pinned buffers, feeds tfft_embed_stream_batch / tfft_extract_stream_batch chunk by chunk and deflates the stego images, the three stages
    overlapped; the codec (zlib on the host cores this process may use) is what the rate measures once the kernels are this fast"""
    import ctypes as C
    import shutil
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    from steganosaurus_amd import binding as B
    if os.environ.get("TFFT_LIB"):
        return {"skipped": "an A/B build of the device library is loaded (libtfpipe.so links the shipped one)"}
    n = min(16, wl.n_img)
    W, H = wl.W, wl.H
    cores, how = usable_cores()
    threads = max(1, min(32, cores))
    host = C.CDLL(os.path.join(ROOT, "steganosaurus_amd", "libtfhost.so"))
    d = tempfile.mkdtemp(prefix="tfft_png_")
    try:
        ins = [os.path.join(d, "c%02d.png" % i) for i in range(n)]
        outs = [os.path.join(d, "s%02d.png" % i) for i in range(n)]

        def wr(i):
            return host.tfh_png_write(ins[i].encode(), wl.covers[i].ctypes.data_as(C.c_void_p), W, H)
        with ThreadPoolExecutor(threads) as ex:
            assert all(r == 0 for r in ex.map(wr, range(n)))
        in_bytes = sum(os.path.getsize(p) for p in ins)
        ctx = wl.S.Context(W, H, slots=min(8, n), device=wl.dev.index or 0)
        bins = np.ascontiguousarray(wl.bins_walk)
        chunk = min(8, n)
        B.embed_png_batch(ctx, ins[:chunk], outs[:chunk], W, H, bins, wl.header[:chunk], wl.payload[:chunk], chunk=chunk, threads=threads, png_level=1)   # warm-up
        t0 = time.perf_counter()
        usable, ms_e = B.embed_png_batch(ctx, ins, outs, W, H, bins, wl.header[:n], wl.payload[:n], chunk=chunk, threads=threads, png_level=1)
        t1 = time.perf_counter()
        hdr, pay, st, ms_x = B.extract_png_batch(ctx, outs, W, H, bins, wl.plen, chunk=chunk, threads=threads)
        t2 = time.perf_counter()
        out_bytes = sum(os.path.getsize(p) for p in outs)
        # the files must hold what the resident run produced for the same images: read one back
        back = np.zeros((H, W, 3), np.uint8)
        w_, h_ = C.c_int(0), C.c_int(0)
        assert host.tfh_image_read(outs[0].encode(), back.ctypes.data_as(C.c_void_p), C.c_uint64(back.size), C.byref(w_), C.byref(h_)) == 0
        wl.embed()
        wl.ctx.sync()
        same = bool((back == wl.d_stego[0].cpu().numpy()).all())
        ctx.close()
        return {"value": round(n * W * H / (t2 - t0) / 1e6, 1), "unit": "MPixels/s", "images": n, "threads": threads, "cores": how,
                "embed_ms": round((t1 - t0) * 1e3, 1), "extract_ms": round((t2 - t1) * 1e3, 1),
                "embed_stage_ms": {"wall": round(ms_e[0], 1), "decode_thread_sum": round(ms_e[1], 1), "device_calls": round(ms_e[2], 1), "encode_thread_sum": round(ms_e[3], 1)},
                "extract_stage_ms": {"wall": round(ms_x[0], 1), "decode_thread_sum": round(ms_x[1], 1), "device_calls": round(ms_x[2], 1)},
                "png_bytes_in": in_bytes, "png_bytes_out": out_bytes, "png_level_out": 1,
                "stego_file_identical_to_resident_run": same,
                "note": "PNG inflate (zlib) -> pinned buffers -> tfft_embed_stream_batch -> PNG deflate (level 1, 'up' filter) + file write, then the same files "
                        "through inflate -> tfft_extract_stream_batch; decode / device / encode overlapped chunk by chunk (include/turtlefft_pipe.h)"}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def cpu_baseline(wl, S):
    """The reference CPU path (oracle/_ref, the reference TU compiled in place) timed on this host, one thread, one image of the
    same workload: embed + extract signal path, crypto/PNG excluded.  Falls back to the repo's own restatement (kind "port") when
    _ref did not travel.  The same image then goes through the GPU path and is compared with what the reference produced."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _checkers import Checker, Params, have_ref
    kind = "reference" if have_ref() else "port"
    chk = Checker("ref" if kind == "reference" else "orc")
    pk = hashlib.sha256(b"test123").digest()
    W, H = wl.W, wl.H
    cover = wl.covers[0]
    # bound the sample to ~10-30 s: a 4K image costs ~60 s on the reference, so larger workloads
    # are sampled on a 1920x1080 crop of the same cover with the config-2 payload
    if W * H > 1920 * 1080:
        cover = np.ascontiguousarray(cover[:1080, :1920])
        n = 38 * 24 + (4096 + 16) * 56
        sample = "one 1920x1080 crop of the workload's cover, 4 KB payload (a full image would exceed the 30 s bound)"
    else:
        n = wl.n_bits
        sample = "one image of the workload (%dx%d, %d stream bits)" % (W, H, n)
    b = np.ascontiguousarray(rep_stream(wl.header[0], wl.payload[0])[:n])
    t0 = time.perf_counter()
    stego, _, ref_bins = chk.embed_rgb8(cover, pk, b, Params(), want_bins=True)
    raw = chk.extract_bits(stego, pk, n, Params())
    dt = time.perf_counter() - t0
    h, w = cover.shape[:2]
    out = {"value": round(w * h / dt / 1e6, 4), "unit": "MPixels/s", "cores": 1, "kind": kind, "sample": sample,
           "seconds": round(dt, 2), "ber": float((raw != b).mean()), "host_cpus": os.cpu_count()}
    # ---- parity of the GPU path on the same image (untimed): same bins, stego within 1 LSB, raw bits of the reference's stego
    key_walk = hmac.new(pk, b"turtle_keys" + b"\x01", hashlib.sha256).digest()
    bins = S.Walk(key_walk, next_pow2(h), next_pow2(w)).next(n)
    g = S.Context(w, h)
    g.forward_rgb8(cover)
    g.embed_bins(bins, b)
    mine = g.inverse_rgb8(w, h)
    g.forward_rgb8(stego)
    got = g.read_bins(bins)
    g.close()
    d = mine.astype(np.int16) - stego
    out["parity_vs_reference"] = {
        "ok": bool(np.array_equal(S.bins_to_triples(bins), ref_bins) and np.abs(d).max() <= 1 and (d != 0).mean() < 0.01 and np.array_equal(got, raw)),
        "bin_list_identical": bool(np.array_equal(S.bins_to_triples(bins), ref_bins)),
        "stego_max_abs_diff": int(np.abs(d).max()), "stego_pixels_differing": int((d != 0).sum()), "pixels": int(d.size),
        "raw_bits_of_reference_stego_mismatches": int((got != raw).sum()), "bits": int(n)}
    assert out["parity_vs_reference"]["ok"], out["parity_vs_reference"]
    # ---- the same two comparisons THROUGH THE CALLS THIS BENCH TIMES (tfft_embed_stream_batch_dev / tfft_extract_stream_batch_dev on the
    # workload's own context, whole batch, packed bytes in and out): the timed embedder's image 0 against the reference's stego image,
    # and the reference's stego image, put in place of image 0 of the batch, through the timed extractor
    if (h, w) == (H, W) and n == wl.n_bits:
        torch = wl.torch
        wl.embed()
        wl.ctx.sync()
        d2 = wl.d_stego[0].cpu().numpy().astype(np.int16) - stego
        src = wl.d_stego.clone()
        src[0].copy_(torch.from_numpy(stego).to(wl.dev))
        d_raw = torch.zeros((wl.n_img, wl.n_bins), dtype=torch.uint8, device=wl.dev)
        wl.extract(raw_ptr=d_raw.data_ptr(), src=src)
        wl.ctx.sync()
        got2 = d_raw[0, :n].cpu().numpy()
        # what do_extract would decode from the reference's own raw bits (S:1223-1269): Rep-3 majority of the first 912, then -- if the
        # magic / version / clen come out -- Rep-7 majority of the payload
        hdr_ref = np.packbits((raw[:912].reshape(-1, 3).sum(axis=1) >= 2).astype(np.uint8))
        hdr_gpu = wl.d_hdr_out[0].cpu().numpy()
        status = int(wl.d_status[0].item())
        decodes = bytes(hdr_ref[:4]) == b"FTTG" and hdr_ref[4] == 2 and int.from_bytes(bytes(hdr_ref[34:38]), "big") == wl.secret
        pay_ok = None
        if decodes:
            pay_ref = np.packbits((raw[912:912 + wl.plen * 56].reshape(-1, 7).sum(axis=1) >= 4).astype(np.uint8))
            pay_ok = bool(status == wl.secret and np.array_equal(wl.d_pay_out[0].cpu().numpy(), pay_ref))
        out["parity_timed_api"] = {
            "calls": "tfft_embed_stream_batch_dev / tfft_extract_stream_batch_dev, %d images per call (the timed configuration)" % wl.n_img,
            "stego_image0_max_abs_diff": int(np.abs(d2).max()), "stego_image0_pixels_differing": int((d2 != 0).sum()), "pixels": int(d2.size),
            "raw_bits_of_reference_stego_mismatches": int((got2 != raw).sum()), "bits": int(n),
            "header_bytes_equal_reference_decode": bool(np.array_equal(hdr_gpu, hdr_ref)),
            "reference_header_decodes": bool(decodes), "status": status, "payload_bytes_equal_reference_decode": pay_ok}
        pt = out["parity_timed_api"]
        pt["ok"] = bool(pt["stego_image0_max_abs_diff"] <= 1 and pt["stego_image0_pixels_differing"] < 0.01 * d2.size and
                        pt["raw_bits_of_reference_stego_mismatches"] == 0 and pt["header_bytes_equal_reference_decode"] and
                        (pay_ok is not False))
        assert pt["ok"], pt
    else:
        out["parity_timed_api"] = {"ok": None, "note": "not run: the reference was timed on a crop (a full image of this workload costs it minutes); "
                                                       "the default workload and tests/test_gpu_parity.py cover the batched calls"}
    # the same image on every core of this GPU's host share at once (independent images are
    # how the path scales on a CPU too).  Threads, not processes: the checker is re-entrant C called through
    # ctypes (GIL released), and a GPU-initialised process must not exec children on this pool.
    ncore, how = usable_cores()
    if ncore > 1:
        from concurrent.futures import ThreadPoolExecutor

        def one(_):
            st, _, _ = chk.embed_rgb8(cover, pk, b, Params())
            return chk.extract_bits(st, pk, n, Params())
        t0 = time.perf_counter()
        with ThreadPoolExecutor(ncore) as ex:
            raws = list(ex.map(one, range(ncore)))
        dta = time.perf_counter() - t0
        out["all_cores"] = {"value": round(ncore * w * h / dta / 1e6, 4), "unit": "MPixels/s", "cores": ncore,
                            "seconds": round(dta, 2), "identical_results": bool(all((r == raw).all() for r in raws)),
                            "note": "one image per thread, %d threads at once (%s)" % (ncore, how)}
    return out


def usable_cores():
    """the cores this process can really run on: its affinity mask, cut down by a cgroup CPU quota when there is one"""
    try:
        n = len(os.sched_getaffinity(0))
        how = "sched_getaffinity: %d" % n
    except Exception:
        n = os.cpu_count() or 1
        how = "cpu_count: %d" % n
    for f in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(f).read().split()
            if f.endswith("cpu.max"):
                q = None if txt[0] == "max" else float(txt[0]) / float(txt[1])
            else:
                q = float(txt[0]) / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read()) if float(txt[0]) > 0 else None
            if q is not None and q < n:
                n = max(1, int(q))
                how += ", cgroup quota %.1f" % q
            break
        except Exception:
            continue
    return max(1, n), how


if __name__ == "__main__":
    main()
