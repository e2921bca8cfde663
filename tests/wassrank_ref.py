"""Test-side restatement of WassRank (ptranking/ltr_adhoc/listwise/wassrank/wassRank.py:43-88, mode 'SinkhornOT', smooth_type 'ST',
norm_type 'BothST') in float64 numpy, log domain, every log-sum-exp with its own row's maximum — the contract of ptr_wassrank_fwd_bwd
(include/ptranking_amd.h).  Not product code: the tests compare the HIP kernel against it, and it against the reference's own outputs.

Where the reference's float64 run takes a value through fp32 (the FloatTensor constants non_rele_gap / var_penalty, the fp32 position
discounts of 'ddg'), so does this restatement."""
import math

import numpy as np
import torch

COST_TYPES = ("p1", "p2", "eg", "dg", "ddg")


def cost_matrix(y, cost_type, gain_base=4.0, non_rele_gap=100.0, var_penalty=math.e):
    """C [n, n] float64 for one query's labels y [n] (wasserstein_cost_mat.py:47-139)."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    pos = np.arange(n, dtype=np.float64)
    if cost_type in ("p1", "p2"):
        c = np.abs(pos[:, None] - pos[None, :])
        return c * c if cost_type == "p2" else c
    if cost_type == "eg":
        gap, vp = float(np.float32(non_rele_gap)), float(np.float32(var_penalty))
        g = np.power(float(gain_base), y) - 1.0
        g = np.where(g < 1.0, -gap, g)
        c = np.abs(g[:, None] - g[None, :])
        c = np.where(c < 1.0, vp, c)
        np.fill_diagonal(c, 0.0)
        return c
    if cost_type in ("dg", "ddg"):
        g = np.power(2.0, y) - 1.0
        c = np.abs(g[:, None] - g[None, :])
        if cost_type == "ddg":
            d = (np.float32(1.0) / np.log2(pos.astype(np.float32) + np.float32(2.0))).astype(np.float64)
            c = c * np.abs(d[:, None] - d[None, :])
        return c
    raise NotImplementedError(cost_type)


def _lse_rows(x):
    m = np.max(x, axis=1, keepdims=True)
    return (m + np.log(np.sum(np.exp(x - m), axis=1, keepdims=True)))[:, 0]


def _log_softmax(x):
    m = np.max(x)
    return x - m - np.log(np.sum(np.exp(x - m)))


def query(preds, labels, cost_type="eg", lam=0.1, sh_itr=20, gain_base=4.0, non_rele_gap=100.0, var_penalty=math.e,
          scale_by_max_label=False):
    """One query (unpadded, B = 1): (loss, dLoss/dpreds) in float64."""
    s = np.asarray(preds, dtype=np.float64)
    y = np.asarray(labels, dtype=np.float64)
    n = s.shape[0]
    if n <= 1:
        return 0.0, np.zeros(n)
    C = cost_matrix(y, cost_type, gain_base, non_rele_gap, var_penalty)
    m = float(np.max(y)) if scale_by_max_label else 1.0
    log_a, log_b = _log_softmax(m * s), _log_softmax(y)
    log_u = np.full(n, -math.log(n))
    log_v = np.full(n, -math.log(n))
    K = -C / lam
    for _ in range(sh_itr):
        log_v = log_b - _lse_rows(K.T + log_u[None, :])      # LSE_i(log u_i - C_ij / lam), row j
        log_u = log_a - _lse_rows(K + log_v[None, :])        # LSE_j(log v_j - C_ij / lam), row i
    loss = float(np.sum(C * np.exp(log_u[:, None] + K + log_v[None, :])))
    g = lam * log_u
    g = g - g.mean()
    g = g - g.mean()
    a = np.exp(log_a)
    return loss, m * a * (g - np.sum(a * g))


def batch(preds, labels, lens=None, **kw):
    """Padded batch [B, L]: (mean loss, per-query losses [B], grad [B, L]) — grad carries the 1/B, padded documents get 0."""
    preds = np.asarray(preds, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.float64)
    B, L = preds.shape
    lq = np.zeros(B)
    grad = np.zeros((B, L))
    for q in range(B):
        n = L if lens is None else int(lens[q])
        lq[q], gq = query(preds[q, :n], labels[q, :n], **kw)
        grad[q, :n] = gq / B
    return (float(lq.mean()) if B else 0.0), lq, grad


class _Restated(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, labels, lens, kw):
        lo, _, g = batch(preds.detach().cpu().numpy(), labels.detach().cpu().numpy(),
                         None if lens is None else lens.detach().cpu().numpy(), **kw)
        ctx.save_for_backward(torch.from_numpy(g).to(preds.device, preds.dtype))
        return torch.tensor(lo, dtype=preds.dtype, device=preds.device)

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return g * grad_out, None, None, None


def wassrank_loss(preds, labels, cost_type="eg", lam=0.1, sh_itr=20, gain_base=4.0, non_rele_gap=100.0, var_penalty=math.e,
                  scale_by_max_label=False, lens=None):
    """Drop-in for ptranking_amd.functional.wassrank_loss (same signature) on any device, computed by the float64 restatement."""
    kw = dict(cost_type=cost_type, lam=lam, sh_itr=sh_itr, gain_base=gain_base, non_rele_gap=non_rele_gap, var_penalty=var_penalty,
              scale_by_max_label=scale_by_max_label)
    return _Restated.apply(preds, labels, lens, kw)
