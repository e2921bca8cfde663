"""torch restatement (float64 by default) of DivProbRanker's objectives, in two forms, with autograd for the gradients:

  literal   the reference's formulas as it evaluates them: p = 1 - erfc(x) / 2 fed to F.binary_cross_entropy (each logarithm clamped at -100,
            the backward divided by max(p (1 - p), 1e-12)), the delta-alpha-DCG weights divided by the ideal value without a guard.
            tests/test_divprob_cpu.py checks it against the reference's own float64 results stored in tests/golden/divprob.npz.
  stable    the definition the kernel implements (include/ptranking_amd.h, ptr_divprob_fwd_bwd): log Q = log_ndtr(-sqrt(2) x) and
            log P = log_ndtr(sqrt(2) x), each clamped at -100 (a clamped logarithm passes no gradient), an ideal value <= 0 gives weight 0.
            The SuperSoft objectives (aNDCG, nERR-IA) are the same in both forms.

  loss(form, mus [L], vars [L], rele [T, L], objective, ...)                      -> 0-d tensor, differentiable in mus and vars
  loss_and_grads(form, mus, vars, rele, objective, dtype=float64, ...)            -> (loss, grad_mu [L], grad_var [L]) as numpy float64
  batch(form, mus [B, L], vars, rele [B, T, L], objective, lens, ntopics, ...)    -> (loss_q [B], grad_mu [B, L], grad_var [B, L]); padded
                                                                                      entries are never read
  expected_ranks(mus [L], vars [L])                                               -> numpy float64 [L]
  need(a, b)                                                                      -> how many times golden_util's element-wise gate a needs
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

OBJECTIVES = ("aNDCG", "nERR-IA", "PairCLS", "LambdaPairCLS")


def pair_args(mus, vars):
    """x[i][j] = (mu_i - mu_j) / sqrt(2 (var_i + var_j))"""
    return (mus[:, None] - mus[None, :]) / torch.sqrt(2.0 * (vars[:, None] + vars[None, :]))


def phi_offdiag(x):
    """Phi[i][j] = erfc(x[i][j]) / 2 with a zero diagonal"""
    return 0.5 * torch.erfc(x) * (1.0 - torch.eye(x.shape[0], dtype=x.dtype))


def target_probs(rele):
    """tb[i][j] = mean over subtopics of (1 + clamp(r_ti - r_tj, -1, 1)) / 2   (one subtopic at a time: nothing of size T x L x L)"""
    T, L = rele.shape
    tb = torch.zeros(L, L, dtype=rele.dtype)
    for t in range(T):
        tb += 0.5 * (1.0 + torch.clamp(rele[t][:, None] - rele[t][None, :], -1.0, 1.0))
    return tb / T


def delta_alpha_dcg(rele, beta):
    """| sum_t (g_ti - g_tj)(d_i f_ti - d_j f_tj) | and the alpha-DCG of the given order at k = L"""
    T, L = rele.shape
    prior = torch.cumsum(rele, dim=1) - rele
    focus = torch.pow(torch.as_tensor(1.0 - beta, dtype=rele.dtype), prior)
    # the rank discounts are fp32 numbers in BOTH forms: the reference builds them from a float32 arange whatever the dtype of the scores
    # (diversity_metric.py:25, :166-167), and the kernel computes them in fp32
    log2_pos = torch.log2(torch.arange(L, dtype=torch.float32) + 2.0)
    disc = (1.0 / log2_pos).to(rele.dtype)
    gains = torch.pow(torch.as_tensor(2.0, dtype=rele.dtype), rele) - 1.0
    h = focus * disc[None, :]
    delta = torch.zeros(L, L, dtype=rele.dtype)
    for t in range(T):
        delta += (gains[t][:, None] - gains[t][None, :]) * (h[t][:, None] - h[t][None, :])
    return torch.abs(delta), (focus * rele / log2_pos.to(rele.dtype)[None, :]).sum()


def loss(form, mus, vars, rele, objective, beta=0.5, top_k=None, top_k_axis=0, max_label=1.0, norm=True):
    assert form in ("literal", "stable") and objective in OBJECTIVES
    T, L = rele.shape
    x = pair_args(mus, vars)
    if objective in ("aNDCG", "nERR-IA"):
        ranks = 1.0 + phi_offdiag(x).sum(dim=1)
        if objective == "aNDCG":
            cover = rele @ phi_offdiag(x).T                                     # [t][i] = sum_j Phi[i][j] r[t][j]
            gains = rele * torch.pow(torch.as_tensor(1.0 - beta, dtype=rele.dtype), cover) / torch.log2(1.0 + ranks)[None, :]
            if top_k:
                gains = gains[:top_k, :] if top_k_axis in (0, "reference") else gains[:, :top_k]
            return -gains.sum()
        satis = (torch.pow(torch.as_tensor(2.0, dtype=rele.dtype), rele) - 1.0) / 2.0 ** max_label
        uns = torch.cumprod(1.0 - satis, dim=1)
        casc = torch.cat([torch.ones(T, 1, dtype=rele.dtype), uns[:, :-1]], dim=1)
        terms = satis * casc / ranks[None, :]
        if top_k:
            terms = terms[:, :top_k]
        return -terms.sum()
    tb = target_probs(rele)
    upper = torch.triu(torch.ones(L, L, dtype=rele.dtype), diagonal=1)
    weight = upper
    if objective == "LambdaPairCLS":
        delta, ideal = delta_alpha_dcg(rele, beta)
        if norm:
            if form == "literal":
                delta = delta / ideal
            else:
                delta = delta / ideal if float(ideal) > 0.0 else torch.zeros_like(delta)
        weight = upper * delta
    if form == "literal":
        p = 1.0 - 0.5 * torch.erfc(x)
        return F.binary_cross_entropy(input=p * upper, target=tb * upper, weight=weight, reduction="none").sum()
    root2 = math.sqrt(2.0)
    log_p = torch.clamp(torch.special.log_ndtr(root2 * x), min=-100.0)
    log_q = torch.clamp(torch.special.log_ndtr(-root2 * x), min=-100.0)
    return (weight * -(tb * log_p + (1.0 - tb) * log_q)).sum()                   # the weight of the lower triangle and of the diagonal is 0


def loss_and_grads(form, mus, vars, rele, objective, dtype=torch.float64, **kw):
    m = torch.as_tensor(np.asarray(mus, np.float64)).to(dtype).reshape(-1).requires_grad_(True)
    v = torch.as_tensor(np.asarray(vars, np.float64)).to(dtype).reshape(-1).requires_grad_(True)
    r = torch.as_tensor(np.asarray(rele, np.float64)).to(dtype)
    out = loss(form, m, v, r, objective, **kw)
    if not out.requires_grad:                                                    # a single document: no pair, a constant
        return float(out), np.zeros(m.shape[0]), np.zeros(m.shape[0])
    gm, gv = torch.autograd.grad(out, (m, v), allow_unused=True)
    z = lambda g: np.zeros(m.shape[0]) if g is None else g.detach().to(torch.float64).numpy()
    return float(out.detach()), z(gm), z(gv)


def batch(form, mus, vars, rele, objective, lens=None, ntopics=None, dtype=torch.float64, **kw):
    mus, vars, rele = np.asarray(mus), np.asarray(vars), np.asarray(rele)
    B, T, L = rele.shape
    loss_q, gm, gv = np.zeros(B), np.zeros((B, L)), np.zeros((B, L))
    for q in range(B):
        n = L if lens is None else int(lens[q])
        nt = T if ntopics is None else int(ntopics[q])
        if n == 0 or nt == 0:
            continue
        loss_q[q], gm[q, :n], gv[q, :n] = loss_and_grads(form, mus[q, :n], vars[q, :n], rele[q, :nt, :n], objective, dtype=dtype, **kw)
    return loss_q, gm, gv


def expected_ranks(mus, vars):
    m, v = torch.as_tensor(np.asarray(mus, np.float64)).reshape(-1), torch.as_tensor(np.asarray(vars, np.float64)).reshape(-1)
    return (1.0 + phi_offdiag(pair_args(m, v)).sum(dim=1)).numpy()


def max_abs_x(mus, vars):
    m, v = torch.as_tensor(np.asarray(mus, np.float64)).reshape(-1), torch.as_tensor(np.asarray(vars, np.float64)).reshape(-1)
    return float(pair_args(m, v).abs().max())


def need(a, b):
    """How many times the element-wise gate of golden_util.assert_close `a` needs against `b`."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if b.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        r = np.abs(a - b) / (1e-5 * np.abs(b) + 1e-6 * max(1.0, float(np.max(np.abs(b)))))
    return float(np.max(np.where(np.isnan(a) & np.isnan(b), 0.0, r)))
