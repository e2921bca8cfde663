"""float64 numpy restatement of the diversification frame's loss and metrics — what the batched, padded and top_k_axis = 1 cases of
tests/test_diversity_gpu.py are compared with (the reference runs one unpadded query per call and has no document cut-off).

  alphadcg(preds [L], rele [T, L], rt, alpha, top_k, top_k_axis)        -> (loss, grad [L])     daletor.py:9-38 + its autograd, analytically
  alphadcg_batch(preds [B, L], rele [B, T, L], ..., lens, ntopics)      -> (loss_q [B], grad [B, L]); padded entries are never read
  div_metrics(preds [L], rele [T, L], ks, alpha, max_label)             -> (andcg [nk], err_ia [nk] | None, nerr_ia [nk] | None, valid)
  div_metrics_batch(preds, rele, ks, alpha, max_label, lens, ntopics)   -> the same, stacked

tests/test_diversity_cpu.py checks these against the reference's own float64 results stored in tests/golden/diversity.npz.
"""
import numpy as np


def robust_sigmoid(x):
    """ptranking/base/utils.py:57-95: 1 / (1 + exp(-x)) for x > 0, exp(x) / (1 + exp(x)) for x < 0, 0.5 at 0."""
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x > 0, 1.0 / (1.0 + e), np.where(x < 0, e / (1.0 + e), 0.5))


def keep_mask(T, L, top_k, top_k_axis):
    m = np.ones((T, L), np.float64)
    if top_k is not None and top_k > 0:
        if top_k_axis in (0, "reference"):
            m[top_k:, :] = 0.0           # daletor.py:30-35: sum over documents, then [0:top_k] of the SUBTOPIC rows
        elif top_k_axis in (1, "documents"):
            m[:, top_k:] = 0.0
        else:
            raise ValueError(top_k_axis)
    return m


def alphadcg(preds, rele, rt=10.0, alpha=0.5, top_k=10, top_k_axis=0):
    s = np.asarray(preds, np.float64).reshape(-1)
    R = np.asarray(rele, np.float64)
    T, L = R.shape
    assert s.shape == (L,)
    ind = robust_sigmoid(rt * (s[None, :] - s[:, None]))        # ind[i][j]
    pi = 0.5 + ind.sum(axis=1)
    cover = ind @ R.T - 0.5 * R.T                               # [i][t]
    lg = np.log2(1.0 + pi)
    m = keep_mask(T, L, top_k, top_k_axis)
    g = m.T * R.T * np.power(1.0 - alpha, cover) / lg[:, None]  # [i][t]
    loss = -g.sum()
    A = g.sum(axis=1) / (lg * np.log(2.0) * (1.0 + pi))
    Bc = -g * np.log(1.0 - alpha)                               # [i][t]
    G = A[:, None] + Bc @ R                                     # [i][j]
    W = G * rt * ind * (1.0 - ind)
    grad = W.sum(axis=0) - W.sum(axis=1)
    return loss, grad


def alphadcg_batch(preds, rele, rt=10.0, alpha=0.5, top_k=10, top_k_axis=0, lens=None, ntopics=None):
    preds, rele = np.asarray(preds), np.asarray(rele)
    B, T, L = rele.shape
    loss_q, grad = np.zeros(B), np.zeros((B, L))
    for q in range(B):
        n = L if lens is None else int(lens[q])
        nt = T if ntopics is None else int(ntopics[q])
        if n == 0 or nt == 0:
            continue
        loss_q[q], grad[q, :n] = alphadcg(preds[q, :n], rele[q, :nt, :n], rt, alpha, top_k, top_k_axis)
    return loss_q, grad


def sort_desc_order(preds):
    """ptr_sort_desc's order: value descending, original index ascending."""
    return np.argsort(-np.asarray(preds, np.float64), kind="stable")


def _alpha_dcg_cum(R, kmax, alpha):
    """diversity_metric.py:43-55: cumulated alpha-DCG at ranks 1 .. kmax of the columns of R in the given order."""
    Rk = R[:, :kmax]
    prior = np.cumsum(Rk, axis=1) - Rk
    gains = (np.power(1.0 - alpha, prior) * Rk / np.log2(np.arange(kmax) + 2.0)).sum(axis=0)
    return np.cumsum(gains)


def _err_ia_cum(R, kmax, max_label):
    """diversity_metric.py:189-221 (point=False): rank-wise ERR-IA at ranks 1 .. kmax, divided by ALL subtopics."""
    Rk = R[:, :kmax]
    satis = (np.power(2.0, Rk) - 1.0) / np.power(2.0, max_label)
    uns = np.cumprod(1.0 - satis, axis=1)
    casc = np.concatenate([np.ones((R.shape[0], 1)), uns[:, :-1]], axis=1)
    return np.cumsum(satis * casc / (np.arange(kmax) + 1.0), axis=1).sum(axis=0) / R.shape[0]


def div_metrics(preds, rele, ks, alpha=0.5, max_label=None):
    R = np.asarray(rele, np.float64)
    T, L = R.shape
    nk = len(ks)
    andcg = np.zeros(nk)
    err = None if max_label is None else np.zeros(nk)
    nerr = None if max_label is None else np.zeros(nk)
    valid = int(R.sum() >= 1.0)                                  # ranker.py:282, :319
    kmax = min(max(ks), L)
    if not valid or kmax <= 0:
        return andcg, err, nerr, valid
    sys_R = R[:, sort_desc_order(preds)]
    ds, di = _alpha_dcg_cum(sys_R, kmax, alpha), _alpha_dcg_cum(R, kmax, alpha)
    if max_label is not None:
        es, ei = _err_ia_cum(sys_R, kmax, max_label), _err_ia_cum(R, kmax, max_label)
    for c, k in enumerate(ks):
        if k < 1 or k > L:
            continue                                             # the reference's zero padding, diversity_metric.py:77-82
        andcg[c] = ds[k - 1] / di[k - 1] if di[k - 1] > 0 else 0.0
        if max_label is not None:
            err[c] = es[k - 1]
            nerr[c] = es[k - 1] / ei[k - 1] if ei[k - 1] > 0 else 0.0
    return andcg, err, nerr, valid


def div_metrics_batch(preds, rele, ks, alpha=0.5, max_label=None, lens=None, ntopics=None):
    preds, rele = np.asarray(preds), np.asarray(rele)
    B, T, L = rele.shape
    nk = len(ks)
    andcg, err, nerr, valid = np.zeros((B, nk)), np.zeros((B, nk)), np.zeros((B, nk)), np.zeros(B, np.int32)
    for q in range(B):
        n = L if lens is None else int(lens[q])
        nt = T if ntopics is None else int(ntopics[q])
        if n == 0 or nt == 0:
            continue
        a, e, ne, valid[q] = div_metrics(preds[q, :n], rele[q, :nt, :n], ks, alpha, max_label)
        andcg[q] = a
        if max_label is not None:
            err[q], nerr[q] = e, ne
    if max_label is None:
        return andcg, None, None, valid
    return andcg, err, nerr, valid


def need(a, b):
    """How many times the element-wise gate of golden_util.assert_close `a` needs against `b`."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if b.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / (1e-5 * np.abs(b) + 1e-6 * max(1.0, float(np.max(np.abs(b)))))))
