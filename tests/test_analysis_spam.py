"""The host arithmetic on top of the SPAM counts (steganosaurus_amd.analysis: spam_features, fld_fit, fld_score)
and the numpy reference the device tests hold the counts to (spam_cases.ref_counts), against hand counts.  CPU only."""
import numpy as np
import pytest

import spam_cases as SC
from steganosaurus_amd import analysis as A


def idx(a, b, c, t):
    n = 2 * t + 1
    return ((a + t) * n + (b + t)) * n + (c + t)


def brute_counts(rgb, t, dirs):
    """one triple at a time, for any list of directions (the four counted ones or their opposites)"""
    h, w = rgb.shape[:2]
    out = np.zeros((3, len(dirs), (2 * t + 1) ** 3), np.int64)
    for k, (dy, dx) in enumerate(dirs):
        for y in range(h):
            for x in range(w):
                if not (0 <= y + 3 * dy < h and 0 <= x + 3 * dx < w):
                    continue
                for p in range(3):
                    v = [int(rgb[y + j * dy, x + j * dx, p]) for j in range(4)]
                    e = [max(-t, min(t, v[j] - v[j + 1])) for j in range(3)]
                    out[p, k, idx(e[0], e[1], e[2], t)] += 1
    return out


@pytest.mark.parametrize("w,h,t", [(7, 6, 1), (9, 5, 3), (4, 4, 2), (3, 9, 3), (1, 1, 3)])
def test_the_reference_equals_a_triple_by_triple_count(w, h, t):
    rng = np.random.default_rng(w * 100 + h)
    rgb = rng.integers(0, 9, (h, w, 3)).astype(np.uint8) * 2 + 100      # differences inside and outside +-t
    assert np.array_equal(SC.ref_counts(rgb, t), brute_counts(rgb, t, SC.DIRS))
    assert SC.ref_counts(rgb, t).sum(axis=2).tolist() == [SC.dir_totals(w, h)] * 3


# a 1 x 6 row, T = 1: pixels 5 5 6 4 4 9 -> differences I[x] - I[x+1] = 0, -1, +2, 0, -5, clamped 0, -1, +1, 0, -1
ROW = np.array([5, 5, 6, 4, 4, 9], np.uint8)
RIGHT = {(0, -1, 1): 1, (-1, 1, 0): 1, (1, 0, -1): 1}                # hand counts, direction right
LEFT = {(1, 0, -1): 1, (0, -1, 1): 1, (-1, 1, 0): 1}                 # I[x] - I[x-1] from the right end: 1, 0, -1, 1, 0 (clamped)


def row_counts():
    rgb = np.repeat(ROW[None, :, None], 3, axis=2)
    c = SC.ref_counts(rgb, 1)
    want = np.zeros(27, np.int64)
    for k, v in RIGHT.items():
        want[idx(*k, 1)] = v
    assert np.array_equal(c[0, 0], want) and c[:, 1:].sum() == 0
    return rgb, c


def test_spam_features_on_a_hand_counted_row():
    rgb, c = row_counts()
    f = A.spam_features(c, t=1)
    assert f.shape == (3, 54) and f.dtype == np.float64
    # the first half: (M_right + M_left + M_down + M_up) / 4 with down and up empty; the second half all zeros
    want = np.zeros(27)
    for k, v in RIGHT.items():
        want[idx(*k, 1)] += v / 3.0 / 4.0
    for k, v in LEFT.items():
        want[idx(*k, 1)] += v / 3.0 / 4.0
    for p in range(3):
        assert np.allclose(f[p, :27], want, rtol=0, atol=1e-15)
        assert (f[p, 27:] == 0).all()
        assert abs(f[p, :27].sum() - 2 / 4) < 1e-15 and f[p, 27:].sum() == 0      # non-empty directions of the half, over 4


def test_the_opposite_directions_are_the_index_permutation():
    rng = np.random.default_rng(3)
    for (w, h, t) in ((9, 8, 1), (7, 7, 2), (5, 9, 3)):
        rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        rgb[:, : w // 2] //= 64                                           # small differences too
        fwd = brute_counts(rgb, t, SC.DIRS)
        bwd = brute_counts(rgb, t, [(-dy, -dx) for (dy, dx) in SC.DIRS])
        n = 2 * t + 1
        for a in range(-t, t + 1):
            for b in range(-t, t + 1):
                for c in range(-t, t + 1):
                    assert np.array_equal(bwd[:, :, idx(a, b, c, t)], fwd[:, :, idx(-c, -b, -a, t)])
        # and spam_features is the eight-direction average of the normalised counts
        tot = fwd.sum(axis=2, keepdims=True).astype(np.float64)
        m = (fwd / tot + bwd / tot) / 4.0
        want = np.concatenate([m[:, 0] + m[:, 1], m[:, 2] + m[:, 3]], axis=1)
        got = A.spam_features(fwd.astype(np.uint32), t=t)
        assert got.shape == (3, 2 * n ** 3) and np.allclose(got, want, rtol=0, atol=1e-15)
        assert np.allclose(got[:, : n ** 3].sum(axis=1), 1.0) and np.allclose(got[:, n ** 3:].sum(axis=1), 1.0)


def test_spam_features_broadcasts_over_images_and_checks_the_shape():
    rgb, c = row_counts()
    batch = np.stack([c, 2 * c, np.zeros_like(c)])
    f = A.spam_features(batch, t=1)
    assert f.shape == (3, 3, 54) and np.array_equal(f[0], f[1]) and (f[2] == 0).all()
    with pytest.raises(ValueError):
        A.spam_features(c, t=3)


def test_each_half_sums_to_its_share_of_non_empty_directions():
    # 3 x 9: right is empty (w < 4), down is not, both diagonals are empty; 9 x 3 the other way round
    for (w, h, first) in ((3, 9, 0.5), (9, 3, 0.5), (4, 4, 1.0), (1, 1, 0.0)):
        rgb = np.random.default_rng(w).integers(0, 256, (h, w, 3)).astype(np.uint8)
        f = A.spam_features(SC.ref_counts(rgb, 3))
        second = 1.0 if (w >= 4 and h >= 4) else 0.0
        assert np.allclose(f[:, :343].sum(axis=1), first) and np.allclose(f[:, 343:].sum(axis=1), second), (w, h)


def test_fld_exact_case():
    w, b = A.fld_fit([[2.0], [4.0]], [[-1.0], [1.0]], ridge=0)
    assert w.shape == (1,) and w[0] == 1.5 and b == -2.25
    assert np.array_equal(A.fld_score([[3.0], [0.0], [1.5]], (w, b)), [2.25, -2.25, 0.0])


def test_fld_with_a_duplicated_column_stays_finite_and_separates():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(40, 2))
    pos, neg = x[:20] + [3.0, 0.0], x[20:] - [3.0, 0.0]
    pos, neg = np.hstack([pos, pos[:, :1]]), np.hstack([neg, neg[:, :1]])      # column 2 = column 0: S is singular
    assert pos[:, 0].min() > neg[:, 0].max()                                    # separable
    model = A.fld_fit(pos, neg)
    assert np.isfinite(model[0]).all() and np.isfinite(model[1])
    assert A.auc(A.fld_score(pos, model), A.fld_score(neg, model)) == 1.0
    # constant features: trace(S) = 0, lambda = 1
    w, b = A.fld_fit(np.ones((3, 2)), np.zeros((3, 2)))
    assert np.array_equal(w, [1.0, 1.0]) and b == -1.0
