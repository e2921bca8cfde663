"""Restatement of the diversification frame's loss and metrics in torch, float64 by default — what the batched, padded and top_k_axis = 1
cases of tests/test_diversity_gpu.py are compared with (the reference runs one unpadded query per call and has no document cut-off), and
the one reference of the element-wise gate tests/diversity_bounds.py.

  alphadcg(preds [L], rele [T, L], rt, alpha, top_k, top_k_axis)        -> (loss, grad [L])     daletor.py:9-38 + its autograd, analytically
  alphadcg_batch(preds [B, L], rele [B, T, L], ..., lens, ntopics)      -> (loss_q [B], grad [B, L]); padded entries are never read
  div_metrics(preds [L], rele [T, L], ks, alpha, max_label)             -> (andcg [nk], err_ia [nk] | None, nerr_ia [nk] | None, valid)
  div_metrics_batch(preds, rele, ks, alpha, max_label, lens, ntopics)   -> the same, stacked

`dtype` (np.float64 / np.float32) is the precision every step is evaluated in; results come back as float64 numpy.  `kernel_consts` takes
alpha, rt and the two logarithms of c = 1 - alpha as the entry points hand them to the kernels: alpha and rt as fp32 values, log2 c and ln c
as float64 logarithms of 1 - (double)alpha rounded to fp32.  `detail` returns the intermediate quantities the error model needs.
lens and ntopics are clamped to [0, L] and [0, T] as the kernels clamp them.

The loss follows the kernel's form of the same mathematics (csrc/diversity.hip): the j = i indicator is left out of the sums (pi = 1 + sum,
cover = sum_{j != i} ind R: the reference's 0.5 and - R / 2 cancel it), both indicators of a pair are products of e = exp(-|x|) and
r = 1 / (1 + e), and d = ind_ij ind_ji.  A difference that is NaN (a NaN score, inf - inf) is a tie: both indicators 0.5, as
Robust_Sigmoid's two torch.where take it.

tests/test_diversity_cpu.py checks these against the reference's own float64 results stored in tests/golden/diversity.npz.
"""
import math

import numpy as np
import torch


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


def _td(dtype):
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def _t(a, td):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(td)


def c_logs(alpha, kernel_consts=False):
    """(alpha, log2 c, ln c) as Python floats; kernel_consts: as ptr_alphadcg_fwd_bwd / ptr_div_metrics_at_ks form them."""
    if not kernel_consts:
        return float(alpha), math.log2(1.0 - alpha), math.log(1.0 - alpha)
    a32 = float(np.float32(alpha))
    return a32, float(np.float32(math.log2(1.0 - a32))), float(np.float32(math.log(1.0 - a32)))


def alphadcg(preds, rele, rt=10.0, alpha=0.5, top_k=10, top_k_axis=0, dtype=np.float64, kernel_consts=False, detail=False):
    td = _td(dtype)
    s = _t(np.asarray(preds).reshape(-1), td)
    R = _t(rele, td)                                             # [T, L]
    T, L = R.shape
    assert s.shape == (L,)
    _, log2_c, ln_c = c_logs(alpha, kernel_consts)
    if kernel_consts:
        rt = float(np.float32(rt))
    Rt = R.t().contiguous()                                      # [i][t]
    x = rt * (s[None, :] - s[:, None])                           # x[i][j] = rt (s_j - s_i)
    e = torch.exp(-x.abs())
    r = 1.0 / (1.0 + e)
    sm = e * r
    half = torch.full((), 0.5, dtype=td)
    off = ~torch.eye(L, dtype=torch.bool)
    ind = torch.where(x > 0, r, torch.where(x < 0, sm, half)) * off        # ind[i][j], j != i
    inv = torch.where(x > 0, sm, torch.where(x < 0, r, half)) * off        # ind[j][i]
    pi = 1.0 + ind.sum(dim=1)
    cover = ind @ Rt                                             # [i][t]
    lg = torch.log2(1.0 + pi)
    m = _t(keep_mask(T, L, top_k, top_k_axis), td).t()
    Rk = Rt * m
    p = torch.exp2(cover * log2_c)
    g = Rk * p / lg[:, None]                                     # [i][t]
    loss = -g.sum()
    A = g.sum(dim=1) / (lg * math.log(2.0) * (1.0 + pi))
    Bc = -g * ln_c                                               # [i][t]
    d = ind * inv
    delta = (A[None, :] - A[:, None]) + Rt @ Bc.t() - Bc @ Rt.t()          # G[j][i] - G[i][j]
    grad = rt * (d * delta).sum(dim=1)
    if detail:
        f = lambda a: a.double().numpy()
        ax = torch.where(torch.isfinite(x), x.abs(), torch.zeros((), dtype=td))
        return dict(loss=float(loss), grad=f(grad), ax=f(ax), ind=f(ind), d=f(d), pi=f(pi), cover=f(cover), lg=f(lg), p=f(p), g=f(g), A=f(A),
                    Bc=f(Bc), delta=f(delta), R=f(Rt), Rk=f(Rk), rt=rt, log2_c=log2_c, ln_c=ln_c)
    return float(loss), grad.double().numpy()


def clamp_len(lens, q, L):
    return L if lens is None else int(min(max(int(lens[q]), 0), L))


def alphadcg_batch(preds, rele, rt=10.0, alpha=0.5, top_k=10, top_k_axis=0, lens=None, ntopics=None, dtype=np.float64, kernel_consts=False):
    preds, rele = np.asarray(preds), np.asarray(rele)
    B, T, L = rele.shape
    loss_q, grad = np.zeros(B), np.zeros((B, L))
    for q in range(B):
        n, nt = clamp_len(lens, q, L), clamp_len(ntopics, q, T)
        if n == 0 or nt == 0:
            continue
        loss_q[q], grad[q, :n] = alphadcg(preds[q, :n], rele[q, :nt, :n], rt, alpha, top_k, top_k_axis, dtype, kernel_consts)
    return loss_q, grad


def sort_desc_order(preds):
    """ptr_sort_desc's and torch.sort's order: value descending, NaN first, original index ascending (-0.0 ties with +0.0)."""
    s = np.asarray(preds, np.float64).reshape(-1)
    nan = np.isnan(s)
    return np.lexsort((np.arange(s.size), -np.where(nan, 0.0, s), ~nan))


def _walk(R, kmax, log2_c, max_label, td):
    """Ranks 1 .. kmax of the columns of R [T, L] in the given order, per subtopic (the kernel's lane): the alpha-DCG terms with their
    prior cover counts (diversity_metric.py:43-55) and, with a maximum label, the ERR terms with their satisfaction probabilities and
    cascades (:189-221).  torch tensors [T, kmax] of dtype td."""
    Rk = R[:, :kmax]
    cov = torch.cumsum(Rk, dim=1) - Rk
    den = torch.log2(torch.arange(kmax, dtype=td) + 2.0)
    out = dict(x=Rk, cov=cov, p=torch.exp2(cov * log2_c), den=den)
    out["gt"] = out["p"] * Rk / den
    if max_label is not None:
        sat = (torch.exp2(Rk) - 1.0) * 2.0 ** -float(max_label)
        uns = torch.cumprod(1.0 - sat, dim=1)
        casc = torch.cat([torch.ones((R.shape[0], 1), dtype=td), uns[:, :-1]], dim=1)
        out.update(sat=sat, casc=casc, et=sat * casc / (torch.arange(kmax, dtype=td) + 1.0))
    return out


def div_metrics(preds, rele, ks, alpha=0.5, max_label=None, dtype=np.float64, kernel_consts=False, detail=False, order=None):
    td = _td(dtype)
    R = _t(rele, td)
    T, L = R.shape
    nk = len(ks)
    andcg = np.zeros(nk)
    err = None if max_label is None else np.zeros(nk)
    nerr = None if max_label is None else np.zeros(nk)
    valid = int(float(np.asarray(rele, np.float64).sum()) >= 1.0)    # ranker.py:282, :319
    kmax = min(max(ks), L) if nk else 0
    if not valid or kmax <= 0:
        return (andcg, err, nerr, valid, None) if detail else (andcg, err, nerr, valid)
    _, log2_c, _ = c_logs(alpha, kernel_consts)
    order = torch.from_numpy(np.asarray(sort_desc_order(preds) if order is None else order, np.int64))     # order: a planted ranking
    ws, wi = _walk(R[:, order], kmax, log2_c, max_label, td), _walk(R, kmax, log2_c, max_label, td)
    ds, di = torch.cumsum(ws["gt"], dim=1).sum(dim=0), torch.cumsum(wi["gt"], dim=1).sum(dim=0)
    if max_label is not None:
        es, ei = torch.cumsum(ws["et"], dim=1).sum(dim=0) / T, torch.cumsum(wi["et"], dim=1).sum(dim=0) / T    # ALL subtopics count
    for c, k in enumerate(ks):
        if k < 1 or k > L:
            continue                                             # the reference's zero padding, diversity_metric.py:77-82
        andcg[c] = float(ds[k - 1] / di[k - 1]) if di[k - 1] > 0 else 0.0
        if max_label is not None:
            err[c] = float(es[k - 1])
            nerr[c] = float(es[k - 1] / ei[k - 1]) if ei[k - 1] > 0 else 0.0
    if detail:
        f = lambda w: {k: v.double().numpy() for k, v in w.items()}
        return andcg, err, nerr, valid, dict(sys=f(ws), ideal=f(wi), log2_c=log2_c, kmax=kmax)
    return andcg, err, nerr, valid


def div_metrics_batch(preds, rele, ks, alpha=0.5, max_label=None, lens=None, ntopics=None, dtype=np.float64, kernel_consts=False):
    preds, rele = np.asarray(preds), np.asarray(rele)
    B, T, L = rele.shape
    nk = len(ks)
    andcg, err, nerr, valid = np.zeros((B, nk)), np.zeros((B, nk)), np.zeros((B, nk)), np.zeros(B, np.int32)
    for q in range(B):
        n, nt = clamp_len(lens, q, L), clamp_len(ntopics, q, T)
        if n == 0 or nt == 0:
            continue
        a, e, ne, valid[q] = div_metrics(preds[q, :n], rele[q, :nt, :n], ks, alpha, max_label, dtype, kernel_consts)
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
