"""Detector and quality figures on top of the device analysis calls (numpy only).

The histograms come from ``Context.phase_hist_batch_*`` (tfft_phase_hist_batch[_dev]), the SSE from ``Context.quality_batch_*``
(tfft_quality_batch[_dev]); what is computed from them here is small host arithmetic:
  psnr_db       10 log10(255^2 W H / SSE) per plane, +inf when SSE is 0
  kl_divergence KL(P || Q) of two count histograms, add-half smoothed: P = (c + 0.5) / (N + 0.5 nb), natural log
  peak_mass     the share of a histogram in the bins that hold +alpha and -alpha (the phase-histogram detector's peak statistic)
  auc           the Mann-Whitney statistic: P(pos > neg) + P(pos == neg) / 2
and from the counts of ``Context.robustness_batch_*`` (tfft_robustness_batch[_dev]):
  raw_ber, byte_error_rate, recovered   raw bit error rate, byte error rate after the repetition code, and whether the message came back
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
