"""The batched stream pipelines with one walk per image (tfft_*_stream_batch_walks[_dev]) and tfft_lowfreq_mag_batch_dev on the MI355X:
the shared-list call's bytes for n copies of one walk, the fp64 reference image by image for distinct keys, the reference's cover
hashes, and the reference CLI's outcome with --cover_dependent_path 1 in both directions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import parity_cases as PC
import walks_cases as WC
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


@pytest.fixture(scope="module")
def host():
    h = C.CDLL(os.path.join(ROOT, "steganosaurus_amd", "libtfhost.so"))
    h.tfh_frame_bits.restype = C.c_uint64
    h.tfh_deframe_bits.restype = C.c_int64
    return h


def test_same_lists_1080p_chunk_of_ten(lib, orc):
    WC.check_same_lists(lib, orc, PC.TorchBufs, 1920, 1080, nimg=10, slots=10, secret=200, jitter=0.05, adaptive=True)


def test_same_lists_1080p_chunks_of_three(lib, orc):
    WC.check_same_lists(lib, orc, PC.TorchBufs, 1920, 1080, nimg=5, slots=3, secret=100, jitter=0.0, adaptive=False, center=True,
                        envs=({}, {"TFFT_TILE_READ": "0"}, {"TFFT_TILE_READ": "3"}, {"TFFT_STATS_TILE": "0"}, {"TFFT_EMBED_DELTA": "0"}))


def test_same_lists_without_jitter_chunk_of_eight(lib, orc):
    # the twin of the emulated case: the direct column plan, the per-image tile-resident read without phase options
    WC.check_same_lists(lib, orc, PC.TorchBufs, 128, 128, nimg=8, slots=8, secret=8, jitter=0.0, adaptive=False, envs=({},), host=False)


def test_same_lists_4k(lib, orc):
    WC.check_same_lists(lib, orc, PC.TorchBufs, 3840, 2160, nimg=3, slots=3, secret=200, jitter=0.05, adaptive=True,
                        envs=({}, {"TFFT_STATS_TILE": "0"}, {"TFFT_TILE_READ": "0"}))


@pytest.mark.parametrize("jitter,adaptive", [(0.0, False), (0.05, False), (0.0, True), (0.05, True)])
def test_distinct_keys_1080p(lib, orc, jitter, adaptive):
    WC.check_distinct_keys(lib, orc, PC.TorchBufs, 1920, 1080, nimg=9, slots=9, secret=40, jitter=jitter, adaptive=adaptive, n_oracle=1,
                           envs=({}, {"TFFT_STREAMS": "2"}, {"TFFT_STATS_TILE": "0"}), n_threads=8)


def test_distinct_keys_2048x1024_round_trip(lib, orc):
    # a power-of-two cover: the payloads come back (1080p and 4K pad, and lose the stream in the crop, in the reference too)
    WC.check_distinct_keys(lib, orc, PC.TorchBufs, 2048, 1024, nimg=9, slots=9, secret=200, jitter=0.05, adaptive=True, n_oracle=1,
                           envs=({}, {"TFFT_STREAMS": "2"}), n_threads=8)


def test_distinct_keys_4k(lib, orc):
    WC.check_distinct_keys(lib, orc, PC.TorchBufs, 3840, 2160, nimg=3, slots=3, secret=40, jitter=0.05, adaptive=True, center=True, n_oracle=1,
                           n_threads=3)


def test_errors(lib, orc):
    WC.check_errors(lib, orc, PC.TorchBufs)


def test_lowfreq_batch_matches_single_and_reference(lib, host, golden_dir):
    WC.check_lowfreq_batch(lib, host, PC.TorchBufs, golden_dir)


def _stable_cover(n, seed):
    """a cover whose 32-byte hash survives embedding (tests/test_gpu_cli.py): every magnitude of the 8x8 corner in the middle of its
    quantiser bucket"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n]
    img = cover_rgb(n, n, seed).astype(np.float64)
    for p in range(3):
        for y in range(8):
            for x in range(8):
                if y or x:
                    img[:, :, p] += (2 * 60000.0 / (n * n)) * np.cos(2 * np.pi * (y * yy + x * xx) / n + rng.uniform(0, 2 * np.pi))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _cover_dependent_walks(lib, host, imgs, passes, n_bins, max_jitter=None):
    """S:1020-1063 for a batch: cover hashes (tfft_lowfreq_mag_batch_dev -> quantiser + SHA-256) -> path keys -> HKDF subkeys -> walks"""
    from steganosaurus_amd import binding as B
    n, h, w = imgs.shape[:3]
    ph, pw = 1 << (h - 1).bit_length(), 1 << (w - 1).bit_length()
    region = min(8, min(ph, pw) // 8)
    ctx = B.Context(w, h, slots=n)
    ib, pi = PC.TorchBufs.put(imgs)
    ob, po = PC.TorchBufs.put(np.zeros((n, 3, region, region)))
    ctx.lowfreq_mag_batch_dev(n, pi, w, h, region, po)
    ctx.sync()
    mags = PC.TorchBufs.get(ob)
    ctx.close()
    keys = b""
    for i in range(n):
        ch = PC.host_cover_hash(host, mags[i])
        pk = C.create_string_buffer(32)
        host.tfh_path_key(passes[i], C.c_size_t(len(passes[i])), ch, pk)
        sub = C.create_string_buffer(128)
        host.tfh_hkdf_expand(pk.raw, b"turtle_keys", C.c_size_t(11), sub, C.c_size_t(128))
        keys += sub.raw
    bins, jit, st = B.walks_build(keys, ph, pw, n_bins, max_jitter=max_jitter, n_threads=4)
    assert (st == 0).all()
    return bins, jit


@pytest.mark.skipif(not have_ref(), reason="reference CLI not present")
def test_cover_dependent_paths_interoperate_with_the_reference_cli(tmp_path, lib, host):
    from steganosaurus_amd import binding as B
    n, w = 4, 256
    it = ["--pbkdf2_iter", "1000", "--cover_dependent_path", "1"]
    passes = [b"pw-%d" % i for i in range(n)]
    secrets = [b"cover dependent #%d" % i for i in range(n)]
    # covers whose hash survives embedding (on others the stego's hash, which the extractor computes, crosses a quantiser edge: whether
    # that happens depends on the last bit of every pixel, and the reference itself then fails, test_gpu_cli.py)
    imgs = np.stack([_stable_cover(w, 20 + i) for i in range(n)])
    plen = max(len(s) for s in secrets) + 16
    n_bins = 912 + 56 * plen
    # (1) batch embed, one cover-dependent walk per image; the reference CLI reads each stego as it reads its own stego of that cover
    headers = np.zeros((n, 38), np.uint8); payloads = np.zeros((n, plen), np.uint8)
    for i in range(n):
        bits = np.zeros(912 + 56 * (len(secrets[i]) + 16), np.uint8)
        salt = bytes((17 * i + j) & 255 for j in range(16))
        assert host.tfh_frame_bits(passes[i], salt, 1000, secrets[i], len(secrets[i]), bits.ctypes.data_as(C.c_void_p), C.c_uint64(len(bits))) == len(bits)
        # pad every stream to one length: the rest of the payload area is never read (clen in the header says how much is)
        headers[i] = np.packbits(bits[:912].reshape(-1, 3)[:, 0])
        pay = np.packbits(bits[912:].reshape(-1, 7)[:, 0])
        payloads[i, :len(pay)] = pay
    bins, _ = _cover_dependent_walks(lib, host, imgs, passes, n_bins)
    ctx = B.Context(w, w, slots=n)
    out = np.zeros_like(imgs)
    ctx.embed_stream_batch_walks_host(imgs, bins, headers, payloads, out)
    ctx.close()
    n_ok = 0
    for i in range(n):
        cov, ours, theirs = (str(tmp_path / ("%s%d.png" % (k, i))) for k in ("c", "o", "r"))
        for p, img in ((cov, imgs[i]), (ours, out[i])):
            assert host.tfh_png_write(p.encode(), img.ctypes.data_as(C.c_void_p), w, w) == 0
        r = subprocess.run([REF_CLI, "embed", "--in", cov, "--out", theirs, "--secret", secrets[i].decode(), "--pass", passes[i].decode(), *it],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = [subprocess.run([REF_CLI, "extract", "--in", p, "--pass", passes[i].decode(), *it], capture_output=True, text=True)
               for p in (ours, theirs)]
        assert (got[0].returncode, got[0].stdout) == (got[1].returncode, got[1].stdout), (i, got[0].stderr, got[1].stderr)
        n_ok += got[0].returncode == 0 and got[0].stdout == secrets[i].decode() + "\n"
    assert n_ok == n, n_ok          # the stable covers' hashes survive embedding: every image round-trips
    # (2) the reference's cover-dependent stego PNGs, extracted as a batch: the hash of the STEGO image picks the walk (S:1157-1169)
    stegos = []
    for i in range(n):
        rgb = np.zeros((w, w, 3), np.uint8)
        ww, hh = C.c_int(0), C.c_int(0)
        assert host.tfh_image_read(str(tmp_path / ("r%d.png" % i)).encode(), rgb.ctypes.data_as(C.c_void_p), C.c_uint64(rgb.size),
                                   C.byref(ww), C.byref(hh)) == 0
        stegos.append(rgb)
    stegos = np.stack(stegos)
    n_read = 912 + 56 * (plen + 16)
    bins, _ = _cover_dependent_walks(lib, host, stegos, passes, n_read)
    ctx = B.Context(w, w, slots=n)
    ho = np.zeros((n, 38), np.uint8); po = np.zeros((n, plen + 16), np.uint8); so = np.zeros(n, np.int32)
    ctx.extract_stream_batch_walks_host(stegos, bins, ho, po, so)
    ctx.close()
    for i in range(n):
        theirs = subprocess.run([REF_CLI, "extract", "--in", str(tmp_path / ("r%d.png" % i)), "--pass", passes[i].decode(), *it],
                                capture_output=True, text=True)
        if so[i] < 0:
            assert theirs.returncode != 0, (i, so[i], theirs.stdout)
            continue
        stream = PC.rep_stream(ho[i], po[i][:so[i] + 16])
        buf = C.create_string_buffer(256)
        k = host.tfh_deframe_bits(passes[i], 1000, stream.ctypes.data_as(C.c_void_p), C.c_uint64(len(stream)), buf, C.c_uint64(256))
        assert (theirs.returncode, theirs.stdout) == (0, buf.raw[:k].decode() + "\n"), (i, k, theirs.stderr)
        assert buf.raw[:k] == secrets[i]
