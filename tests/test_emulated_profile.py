"""tfft_profile_stage on the CPU-emulated build (tests/emu): the launches it reports per stage, set up as bench.py's profile_stages sets
it up -- an address-ordered, registered shared list with its bit index, one single-image forward first, every stage over all the slots.
The profiler asks the batched pipelines' own plan functions which path a chunk takes, so the counts below are those of the launches an
embed or extract of such a chunk makes.  They were recorded on the emulator from the commit before the profiler did so; the host logic
that decides them is the same on gfx950, the kernels behind them are not checked here.

Covers: 64x64 (direct column plan) and 40x300 (two-step, PH = 512: the smallest plan the in-kernel statistics reach)."""
import os
import subprocess

import numpy as np
import pytest

import parity_cases as PC
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")

N_IMG = 2
N_BINS = 300
ORDER = [0, 1, 2, 10, 0, 1, 2, 8, 9, 3, 7, 4, 5, 6]      # bench.py: forward stages, a clean spectrum again, its readers, the inverse last
COVERS = {"64x64": (64, 64), "40x300": (40, 300)}
# env -> (medians at 64x64, medians at 40x300, capacity)
ENVS = [
    ({}, 7, 7, 0),
    ({"TFFT_STATS_TILE": "2"}, 7, 10, 0),
    ({"TFFT_STATS_TILE": "0"}, 7, 7, 0),
    ({"TFFT_EMBED_DELTA": "0"}, 6, 6, 0),
    ({"TFFT_TILE_READ": "3"}, 7, 7, 0),
    ({"TFFT_STATS_FUSED": "0"}, 5, 5, 2),
]


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


def env_id(e):
    return ",".join("%s=%s" % kv for kv in sorted(e[0].items())) or "default"


@pytest.mark.parametrize("cover", sorted(COVERS))
@pytest.mark.parametrize("case", ENVS, ids=[env_id(e) for e in ENVS])
def test_launches_per_stage(emu, orc, case, cover):
    env, med_direct, med_two_step, capacity = case
    w, h = COVERS[cover]
    bufs = PC.HostBufs
    ctx = PC._ctx_with_env(env, w, h, slots=N_IMG, lib=emu)
    plan = ctx.plan_info(w, h, N_IMG)
    assert plan["two_step"] == (cover == "40x300")
    ph, pw = orc.next_pow2(h), orc.next_pow2(w)
    bins, idx = B.bins_sort(B.Walk(orc.subkeys(PC.PK)[0], ph, pw, lib=emu).next(N_BINS), lib=emu)
    ctx.set_bit_index(idx)
    _kb, p_bins = bufs.put(bins.view(np.uint8).reshape(-1, 8))
    ctx.bins_register_dev(p_bins, N_BINS)
    _ib, p_img = bufs.put(np.stack([cover_rgb(w, h, i) for i in range(N_IMG)]))
    _ob, p_out = bufs.put(np.zeros((N_IMG, h, w, 3), np.uint8))
    _bb, p_bits = bufs.put(np.random.default_rng(99).integers(0, 2, size=(N_IMG, N_BINS), dtype=np.uint8))
    _rb, p_raw = bufs.put(np.zeros((N_IMG, N_BINS), np.uint8))
    ctx.forward_rgb8_dev(p_img, w, h)
    ctx.sync()
    want = {name: 1 for name in B.Context.STAGES}
    want["medians"] = med_two_step if plan["two_step"] else med_direct
    want["capacity"] = capacity
    if not plan["two_step"]:
        want["cols_fwd_b"] = want["cols_inv_b"] = 0
    got = []
    for sid in ORDER:
        _ms, nl = ctx.profile_stage(sid, 1, p_img, p_out, p_bins, p_bits, p_raw, N_BINS, n_images=N_IMG)
        got.append((B.Context.STAGES[sid], nl))
    ctx.sync()
    ctx.close()
    print(env_id(case), cover, got)
    assert got == [(B.Context.STAGES[sid], want[B.Context.STAGES[sid]]) for sid in ORDER]
