"""Detector and quality figures on top of the device analysis calls (numpy only).

The histograms come from ``Context.phase_hist_batch_*`` (tfft_phase_hist_batch[_dev]), the SSE from ``Context.quality_batch_*``
(tfft_quality_batch[_dev]); what is computed from them here is small host arithmetic:
  psnr_db       10 log10(255^2 W H / SSE) per plane, +inf when SSE is 0
  kl_divergence KL(P || Q) of two count histograms, add-half smoothed: P = (c + 0.5) / (N + 0.5 nb), natural log
  peak_mass     the share of a histogram in the bins that hold +alpha and -alpha (the phase-histogram detector's peak statistic)
  auc           the Mann-Whitney statistic: P(pos > neg) + P(pos == neg) / 2
and from the counts of ``Context.robustness_batch_*`` (tfft_robustness_batch[_dev]):
  raw_ber, byte_error_rate, recovered   raw bit error rate, byte error rate after the repetition code, and whether the message came back
and from the counts of ``Context.spam_batch_*`` (tfft_spam_batch[_dev]):
  spam_features        the 2 n^3 SPAM features per plane: the released extractor's normalisation and direction averaging
  fld_fit, fld_score   a Fisher linear discriminant with a ridge, the simple classifier the features are judged with
"""
import numpy as np


def psnr_db(sse, w, h):
    """PSNR in dB of an 8-bit plane of w x h pixels with the given sum of squared differences (any shape); +inf where SSE is 0."""
    sse = np.asarray(sse, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(sse > 0, 10.0 * np.log10(255.0 ** 2 * float(w) * float(h) / np.where(sse > 0, sse, 1.0)), np.inf)


def _smoothed(counts):
    c = np.asarray(counts, np.float64)
    nb = c.shape[-1]
    return (c + 0.5) / (c.sum(axis=-1, keepdims=True) + 0.5 * nb)


def kl_divergence(p_counts, q_counts):
    """KL(P || Q) in nats over the last axis of two count histograms of the same length, each smoothed by add-half:
    P = (c + 0.5) / (N + 0.5 nb).  Broadcasts over leading axes (e.g. (n, 3, nb) against a pooled (3, nb))."""
    p, q = _smoothed(p_counts), _smoothed(q_counts)
    return np.sum(p * np.log(p / q), axis=-1)


def peak_bins(nbins, alpha, half_width_bins=0):
    """indices of the bins that hold theta = +alpha and -alpha (bin = floor((theta + pi) nb / 2 pi) mod nb), each widened by
    half_width_bins on either side; sorted and distinct"""
    idx = set()
    for th in (alpha, -alpha):
        b = int(np.floor((th + np.pi) * nbins / (2 * np.pi))) % nbins
        for d in range(-int(half_width_bins), int(half_width_bins) + 1):
            idx.add((b + d) % nbins)
    return np.array(sorted(idx), np.int64)


def peak_mass(hist, alpha, half_width_bins=0):
    """share of the counts in the bins holding +-alpha (peak_bins), over the last axis; 0 for an empty histogram"""
    h = np.asarray(hist, np.float64)
    tot = h.sum(axis=-1)
    sel = h[..., peak_bins(h.shape[-1], alpha, half_width_bins)].sum(axis=-1)
    return np.where(tot > 0, sel / np.where(tot > 0, tot, 1.0), 0.0)


# ---- robustness: figures from the (n_channels, n_images, 4) uint32 result of Context.robustness_batch_*
def raw_ber(result, payload_len):
    """raw bit error rate per (channel, image): raw_bit_errors / (912 + 56 payload_len)"""
    r = np.asarray(result)
    return r[..., 0].astype(np.float64) / float(912 + 56 * int(payload_len))


def byte_error_rate(result, payload_len):
    """byte error rate after the repetition code, decoded at the known length: (header + payload byte errors) / (38 + payload_len)"""
    r = np.asarray(result)
    return (r[..., 1].astype(np.float64) + r[..., 2].astype(np.float64)) / float(38 + int(payload_len))


def recovered(result, payload_len):
    """True where the message came back: no header or payload byte differs and the extractor's status is the length the header
    announces, payload_len - 16"""
    r = np.asarray(result)
    return (r[..., 1] == 0) & (r[..., 2] == 0) & (r[..., 3].astype(np.int64) == int(payload_len) - 16)


# ---- blind steganalysis: SPAM features from the (..., 3, 4, n^3) uint32 counts of Context.spam_batch_*
def spam_features(counts, t=3):
    """(..., 3, 4, n^3) counts of the directions right, down, down-right, down-left -> (..., 3, 2 n^3) float64, n = 2t + 1.
    M_d = C_d / sum(C_d) for each of the eight directions (0 where the sum is 0); the four that are not counted are an index
    permutation, C_{-d}[a, b, c] = C_d[-c, -b, -a].  The first n^3 entries are the mean of M over right, left, down, up, the last n^3
    the mean over the four diagonals."""
    n = 2 * int(t) + 1
    c = np.asarray(counts, np.float64)
    if c.shape[-3:] != (3, 4, n ** 3):
        raise ValueError("spam_features: counts of shape (..., 3, 4, %d) wanted, got %r" % (n ** 3, c.shape))
    tot = c.sum(axis=-1, keepdims=True)
    m = np.where(tot > 0, c / np.where(tot > 0, tot, 1.0), 0.0)
    cube = m.reshape(m.shape[:-1] + (n, n, n))
    opp = np.swapaxes(cube[..., ::-1, ::-1, ::-1], -1, -3).reshape(m.shape)      # [a, b, c] <- [-c, -b, -a]
    both = m + opp
    return np.concatenate([(both[..., 0, :] + both[..., 1, :]) / 4.0, (both[..., 2, :] + both[..., 3, :]) / 4.0], axis=-1)


def fld_fit(pos, neg, ridge=1e-3):
    """Fisher linear discriminant of two (samples, d) classes -> (w, b): S the pooled within-class covariance (divisor n_pos + n_neg - 2),
    lambda = ridge * trace(S) / d (1 if the trace is 0), w = solve(S + lambda I, mu_pos - mu_neg), b = -w . (mu_pos + mu_neg) / 2"""
    pos = np.atleast_2d(np.asarray(pos, np.float64))
    neg = np.atleast_2d(np.asarray(neg, np.float64))
    d = pos.shape[1]
    if neg.shape[1] != d or pos.shape[0] + neg.shape[0] < 3:
        raise ValueError("fld_fit needs two classes of the same width and at least three samples")
    mp, mn = pos.mean(axis=0), neg.mean(axis=0)
    dp, dn = pos - mp, neg - mn
    s = (dp.T @ dp + dn.T @ dn) / float(pos.shape[0] + neg.shape[0] - 2)
    tr = float(np.trace(s))
    lam = ridge * tr / d if tr != 0.0 else 1.0
    w = np.linalg.solve(s + lam * np.eye(d), mp - mn)
    return w, float(-w @ (mp + mn) / 2.0)


def fld_score(x, model):
    """x . w + b for the (w, b) of fld_fit: positive on the side of its first class"""
    w, b = model
    return np.asarray(x, np.float64) @ w + b


def auc(pos_scores, neg_scores):
    """area under the ROC curve of a detector that calls a score stego when it is high: the Mann-Whitney statistic
    P(pos > neg) + P(pos == neg) / 2, from the ranks of the pooled scores (ties share their mean rank)"""
    pos = np.asarray(pos_scores, np.float64).ravel()
    neg = np.asarray(neg_scores, np.float64).ravel()
    if pos.size == 0 or neg.size == 0:
        raise ValueError("auc needs at least one score of each class")
    allv = np.concatenate([pos, neg])
    order = np.argsort(allv, kind="mergesort")
    ranks = np.empty(allv.size, np.float64)
    sv = allv[order]
    i = 0
    while i < sv.size:
        j = i
        while j + 1 < sv.size and sv[j + 1] == sv[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    u = ranks[:pos.size].sum() - pos.size * (pos.size + 1) / 2.0
    return float(u / (pos.size * neg.size))
