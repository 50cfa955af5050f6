"""The batched pipelines' phase options (tfft_set_phase_options: jitter, adaptive alpha) on the MI355X: delta embed, tile-resident and
generic reads, statistics variants, stream pipelines and libtfpipe.so against the fp64 reference and the reference CLI."""
import os
import subprocess

import numpy as np
import pytest

import parity_cases as PC
import phase_cases as PH
from _checkers import REF_CLI, have_ref
from steganosaurus_amd.synth import cover_rgb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")           # torch's HIP runtime first (see test_gpu_parity.py)
    from steganosaurus_amd import binding as B
    return B.load()


def test_1080p_jitter_and_adaptive_statistics_variants(lib, orc):
    PH.check_phase_batch(lib, orc, PC.TorchBufs, 1920, 1080, 20000, nimg=4, slots=4, jitter=0.05, adaptive=True, n_oracle=2,
                         envs=PH.STATS_ENVS)


@pytest.mark.parametrize("kw", [dict(jitter=0.05, adaptive=False, center=True), dict(jitter=0.0, adaptive=True, center=False)])
def test_1080p_one_option(lib, orc, kw):
    PH.check_phase_batch(lib, orc, PC.TorchBufs, 1920, 1080, 20000, nimg=4, slots=2, n_oracle=1, envs=({}, {"TFFT_STATS_TILE": "0"}), **kw)


def test_4k_jitter_and_adaptive(lib, orc):
    PH.check_phase_batch(lib, orc, PC.TorchBufs, 3840, 2160, 40000, nimg=2, slots=2, jitter=0.05, adaptive=True, center=True, n_oracle=1,
                         envs=({}, {"TFFT_STATS_TILE": "0"}))


def test_2048_wide_two_pass_plan(lib, orc):
    # pads to 2048 x 1024: rows fused with the first column step, buckets per row group of the last
    PH.check_phase_batch(lib, orc, PC.TorchBufs, 2040, 1000, 12000, nimg=3, slots=3, jitter=0.05, adaptive=True, n_oracle=1, sort=False,
                         envs=({}, {"TFFT_STATS_TILE": "2"}, {"TFFT_MEDIAN_FALLBACK": "1"}))


def test_stream_batch_round_trip(lib, orc):
    PH.check_phase_stream(lib, orc, PC.TorchBufs, 1024, 1024, secret=200, nimg=3, slots=2, jitter=0.05, adaptive=True, center=True)


@pytest.mark.skipif(not have_ref(), reason="reference CLI not present")
def test_png_pipeline_with_jitter_and_adaptive_is_read_by_the_reference(tmp_path, lib):
    import ctypes as C
    from steganosaurus_amd import binding as B
    host = C.CDLL(os.path.join(ROOT, "steganosaurus_amd", "libtfhost.so"))
    host.tfh_frame_bits.restype = C.c_uint64
    w = h = 256
    n = 4
    secrets = [("phase options #%d " % i + "y" * 10)[:24].encode() for i in range(n)]
    ins, outs = [], []
    for i in range(n):
        img = cover_rgb(w, h, 30 + i)         # textured: on the smooth gradient the weak bins of adaptive alpha (a = alpha/2) flip in 8-bit rounding
        p = str(tmp_path / ("c%d.png" % i))
        assert host.tfh_png_write(p.encode(), img.ctypes.data_as(C.c_void_p), w, h) == 0
        ins.append(p); outs.append(str(tmp_path / ("s%d.png" % i)))
    headers = np.zeros((n, 38), np.uint8); payloads = np.zeros((n, 24 + 16), np.uint8)
    for i in range(n):
        salt = bytes((29 * i + j) & 255 for j in range(16))
        bits = np.zeros(38 * 24 + 40 * 56, np.uint8)
        assert host.tfh_frame_bits(b"pw2", salt, 1000, secrets[i], len(secrets[i]), bits.ctypes.data_as(C.c_void_p), C.c_uint64(len(bits))) == len(bits)
        headers[i] = np.packbits(bits[:912].reshape(-1, 3)[:, 0])
        payloads[i] = np.packbits(bits[912:].reshape(-1, 7)[:, 0])
    pk = np.zeros(32, np.uint8); sub = np.zeros(128, np.uint8)
    host.tfh_turtle_subkeys(b"pw2", C.c_size_t(3), pk.ctypes.data_as(C.c_void_p), sub.ctypes.data_as(C.c_void_p))
    n_bits = 912 + 40 * 56
    bins = B.Walk(bytes(sub[:32]), h, w).next(int(n_bits * 1.25))
    jit = B.walk_jitter(bytes(sub[32:128]), bins, 0.05)
    ctx = B.Context(w, h, slots=3)
    ctx.set_phase_options(jit, True)
    B.embed_png_batch(ctx, ins, outs, w, h, bins, headers, payloads, chunk=2, threads=2, png_level=1)
    for i in range(n):
        r = subprocess.run([REF_CLI, "extract", "--in", outs[i], "--pass", "pw2", "--pbkdf2_iter", "1000", "--jitter", "0.05",
                            "--adaptive_alpha", "1"], capture_output=True, text=True)
        assert (r.returncode, r.stdout) == (0, secrets[i].decode() + "\n"), (i, r.stderr)
    hdr, pay, st, _ = B.extract_png_batch(ctx, outs, w, h, bins, 40, chunk=2, threads=2)
    assert (st == 24).all(), st
    assert np.array_equal(hdr, headers) and np.array_equal(pay, payloads)
    ctx.close()
