"""tfft_walks_build (host): n walks (+ jitter) on a pool of threads, bit for bit the sequential tfft_walk_create / tfft_walk_next /
tfft_walk_jitter calls of each image's own keys; per-image statuses for an exhausted walk.  No GPU needed."""
import hashlib

import numpy as np
import pytest

from steganosaurus_amd import binding as B


def _keys(n, tag=b"k"):
    return b"".join(hashlib.sha256(tag + b"%d.%d" % (i, j)).digest() for i in range(n) for j in range(4))


def _sequential(keys, ph, pw, n_bins, max_jitter, rmin=0.05, rmax=0.45, density=0.7):
    bins, jits = [], []
    for i in range(len(keys) // 128):
        k = keys[128 * i:128 * (i + 1)]
        b = B.Walk(k[:32], ph, pw, rmin=rmin, rmax=rmax, density=density).next(n_bins)
        bins.append(b)
        jits.append(B.walk_jitter(k[32:], b, max_jitter))
    return np.stack(bins), np.stack(jits)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("ph,pw,n_bins,max_jitter", [(128, 128, 1500, 0.05), (512, 256, 20000, 0.0), (128, 512, 4000, 0.3)])
def test_walks_build_equals_the_sequential_calls(threads, ph, pw, n_bins, max_jitter):
    keys = _keys(7)
    want_b, want_j = _sequential(keys, ph, pw, n_bins, max_jitter)
    bins, jit, st = B.walks_build(keys, ph, pw, n_bins, max_jitter=max_jitter, n_threads=threads)
    assert list(st) == [0] * 7
    assert bins.tobytes() == want_b.tobytes()
    assert jit.view(np.uint32).tobytes() == want_j.view(np.uint32).tobytes()
    # without jitter the positions are the same
    b2, j2, _ = B.walks_build(keys, ph, pw, n_bins, max_jitter=None, n_threads=threads)
    assert j2 is None and b2.tobytes() == want_b.tobytes()
    # every image's list differs from the others'
    assert len({bins[i].tobytes() for i in range(7)}) == 7


def test_walks_build_reports_an_exhausted_walk_per_image():
    keys = _keys(3, b"x")
    # a tiny annulus: the walk runs out long before 5000 positions, on every image; a wide one serves 500
    bins, jit, st = B.walks_build(keys, 64, 64, 5000, max_jitter=0.05, rmin=0.05, rmax=0.1, n_threads=2)
    assert list(st) == [-7] * 3
    w = B.Walk(keys[:32], 64, 64, rmin=0.05, rmax=0.1)
    with pytest.raises(B.TfftError) as ei:
        w.next(5000)
    assert ei.value.status == -7
    got = B.bins_to_triples(bins[0])
    found = int((got != 0).any(axis=1).sum())
    assert 0 < found < 5000 and not (got[found:] != 0).any()          # the positions found, then zeros
    lib = B.load()
    assert lib.tfft_walks_build(0, None, 64, 64, 0.05, 0.45, 0.7, 0.0, 10, 4, None, None, None) == 0
    assert lib.tfft_walks_build(1, None, 64, 64, 0.05, 0.45, 0.7, 0.0, 10, 4, None, None, None) == -1


def test_walks_build_more_threads_than_images():
    keys = _keys(2, b"y")
    want_b, want_j = _sequential(keys, 256, 256, 3000, 0.05)
    bins, jit, st = B.walks_build(keys, 256, 256, 3000, max_jitter=0.05, n_threads=16)
    assert list(st) == [0, 0] and bins.tobytes() == want_b.tobytes() and jit.tobytes() == want_j.tobytes()
