"""Robustness analysis on the MI355X (tfft_channel_batch[_dev], tfft_robustness_batch[_dev], `turtlefft embed --robust SPEC`): the checks
of tests/robust_cases.py -- both channels against their fp64 restatements at 640x360, 1919x1081 x 2, 1920x1080 x 3 and 2048^2, every form of
the calls against each other, the robustness counts against the composition of public calls (256^2 in four configurations, 640x360 on the
unfused plan with a 1 KB payload, 1920x1080 x 3 in 2 slots on the fused plan with a 4 KB payload), the error codes and the CLI line."""
import os
import re
import subprocess

import numpy as np
import pytest

import analysis_cases as AC
import robust_cases as RC
from parity_cases import TorchBufs
from steganosaurus_amd import binding as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "steganosaurus_amd", "turtlefft")

# (w, h, n): 3*1919 mod 4 = 1 and 1081 = 8*135 + 1 (every row its own byte shift, edge blocks on both sides); several strips per row
SHAPES = [(640, 360, 3), (1919, 1081, 2), (1920, 1080, 3), (2048, 2048, 1)]


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    # torch's HIP runtime first: initialised after the library's in the same process it finds no device
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")


@pytest.fixture(scope="module")
def lib():
    return B.load()


@pytest.mark.parametrize("w,h,n", SHAPES)
def test_awgn_against_the_reference(lib, w, h, n):
    RC.check_awgn_shape(lib, TorchBufs, w, h, n=n, sigmas=(0.5, 2.0, 8.0) if w == 640 else (2.0,))


@pytest.mark.parametrize("q", [30, 75, 90, 100])
@pytest.mark.parametrize("w,h,n", SHAPES)
def test_jpeg_against_the_reference(lib, w, h, n, q):
    RC.check_jpeg_shape(lib, TorchBufs, w, h, n=n, qualities=(q,))


def test_channel_errors(lib):
    RC.check_channel_errors(lib, TorchBufs)


def test_channel_calls_leave_the_slots_alone(lib):
    RC.check_channel_leaves_slots(lib, TorchBufs, 512, 512)


@pytest.mark.parametrize("sort,phase", [(False, False), (True, False), (False, True), (True, True)])
def test_robustness_equals_the_composition_256(lib, sort, phase):
    RC.check_robustness(lib, TorchBufs, RC.make_case(lib, TorchBufs, 256, 256, 3, 28, sort, phase))


def test_robustness_centred_128(lib):
    RC.check_robustness(lib, TorchBufs, RC.make_case(lib, TorchBufs, 128, 128, 3, 16, True, False, center=True, extra_bins=0))


def test_coarser_quantiser_costs_more_raw_bits(lib):
    RC.check_jpeg_order(lib, TorchBufs, RC.make_case(lib, TorchBufs, 256, 256, 2, 28, True, False))


def test_robustness_errors(lib):
    RC.check_robust_errors(lib, TorchBufs, RC.make_case(lib, TorchBufs, 128, 128, 2, 16, False, False, extra_bins=40))


# (w, h, n, slots, fused plan expected, payload bytes): 4 KB at 1080p, 1 KB at 640 x 360 (whose annulus holds ~120 k positions, 4 KB needs
# 231 k); covers that are not powers of two: their stegos lose bits to the crop even unattacked
BIG = [(640, 360, 2, 2, False, 1024 + 16), (1920, 1080, 3, 2, True, 4096 + 16)]


@pytest.mark.parametrize("w,h,n,slots,fused,plen", BIG)
def test_robustness_equals_the_composition_large(lib, w, h, n, slots, fused, plen):
    ctx = B.Context(w, h, slots=slots, lib=lib)
    try:
        assert ctx.plan_info(w, h, min(n, slots))["fused"] == fused
    finally:
        ctx.close()
    case = RC.make_case(lib, TorchBufs, w, h, n, plen, True, False)
    RC.check_robustness(lib, TorchBufs, case, slot_counts=(slots,), reads_back=False)


def test_cli_robust(tmp_path):
    import ctypes as C
    host = C.CDLL(os.path.join(ROOT, "steganosaurus_amd", "libtfhost.so"))
    cover = RC.flat_cover(512, 512, 0)
    cp, sp = str(tmp_path / "cover.png"), str(tmp_path / "stego.png")
    assert host.tfh_png_write(cp.encode(), cover.ctypes.data_as(C.c_void_p), 512, 512) == 0
    secret = "robust: the quick brown fox"
    plen = len(secret) + 16
    n_bits = 912 + 56 * plen
    args = ["embed", "--in", cp, "--out", sp, "--secret", secret, "--pass", "pw", "--pbkdf2_iter", "1000"]
    spec = "none,awgn:2:7,jpeg:75"
    r = subprocess.run([CLI, *args, "--robust", spec], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Embedded %d bits into %s (payload %d bytes, ver=2, salt/nonce in header)\n" % (n_bits, sp, len(secret))
    lines = r.stderr.splitlines()
    assert len(lines) == 1 and lines[0].startswith("Robustness: "), r.stderr
    items = lines[0][len("Robustness: "):].split("; ")
    assert len(items) == 3
    got = []
    for item, name in zip(items, spec.split(",")):
        m = re.fullmatch(re.escape(name) + r" raw=(\d+)/(\d+) hdr=(\d+)/38 pay=(\d+)/(\d+) (ok|lost)", item)
        assert m, item
        assert int(m.group(2)) == n_bits and int(m.group(5)) == plen
        got.append([int(m.group(1)), int(m.group(3)), int(m.group(4)), m.group(6) == "ok"])
    # the same inputs through the binding: the written pixels, the walk of the passphrase, the frame the stego carries (read back from it:
    # the salt is random, and the unattacked stego of a flat-spectrum power-of-two cover returns every byte)
    stego = AC.png_read_rgb8(sp)
    lib = B.load()
    sub = (C.c_uint8 * 128)()
    pk = (C.c_uint8 * 32)()
    host.tfh_turtle_subkeys(b"pw", C.c_size_t(2), pk, sub)
    bins = B.Walk(bytes(sub[:32]), 512, 512, lib=lib).next(n_bits)
    ctx = B.Context(512, 512, slots=1, lib=lib)
    try:
        hh = np.zeros((1, 38), np.uint8); hp = np.zeros((1, plen), np.uint8); hs = np.zeros(1, np.int32)
        ctx.extract_stream_batch_host(stego[None], bins, hh, hp, hs)
        assert hs[0] == len(secret)
        want = ctx.robustness_batch_host(stego[None], bins, hh, hp, [("none",), ("awgn", 2.0, 7), ("jpeg", 75)])
    finally:
        ctx.close()
    for k in range(3):
        ok = want[k, 0, 1] == 0 and want[k, 0, 2] == 0 and int(want[k, 0, 3].astype(np.int32)) == len(secret)
        assert got[k] == [int(want[k, 0, 0]), int(want[k, 0, 1]), int(want[k, 0, 2]), bool(ok)], (k, got[k], want[k, 0].tolist())
    assert got[0][1:] == [0, 0, True] and got[0][0] <= 3320 // 100      # the message comes back; a raw bit or two of 3320 may not (the salt is random)
    # together with --report 1: each prints its own line; stdout and the stego's message do not depend on either flag
    r2 = subprocess.run([CLI, *args, "--robust", spec, "--report", "1"], capture_output=True, text=True)
    assert r2.returncode == 0 and r2.stdout == r.stdout, r2.stderr
    l2 = r2.stderr.splitlines()
    assert len(l2) == 2 and l2[0].startswith("Report: ") and l2[1].startswith("Robustness: none raw="), r2.stderr
    r3 = subprocess.run([CLI, "extract", "--in", sp, "--pass", "pw", "--pbkdf2_iter", "1000"], capture_output=True, text=True)
    assert (r3.returncode, r3.stdout) == (0, secret + "\n"), r3.stderr
    # a malformed spec is a usage error, like any other bad argument
    unknown = subprocess.run([CLI, *args, "--bogus", "1"], capture_output=True, text=True)
    for bad in ("none,", ",jpeg:75", "blur:3", "awgn", "awgn:-1", "awgn:2:x", "jpeg:0", "jpeg:101", "jpeg:7.5", "jpeg:75:1", "none:1"):
        rb = subprocess.run([CLI, *args, "--robust", bad], capture_output=True, text=True)
        assert rb.returncode == unknown.returncode == 1 and rb.stdout == "" and "Usage:" in rb.stderr, (bad, rb.stderr)
