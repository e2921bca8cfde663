"""Float64 restatement, with ELEMENT-WISE error bounds, of the Gaussian expected-rank metric objectives (csrc/gaussmetric.hip): P, AP, nERR
and nDCG of ptranking/metric/smooth_metric/metric_as_opt_objective.py on the expected ranks of get_expected_rank / get_expected_rank_const
(ptranking/ltr_diversification/util/prob_utils.py:62-101).

Per query of n documents, means m, variances v, presorted labels y:
    a_ij = 1 / sqrt(2 (v_i + v_j))    x_ij = (m_i - m_j) a_ij    Phi_ij = erfc(x_ij) / 2    g_ij = exp(-x_ij^2) / sqrt(pi)
    r_i    = 1 + sum_{j != i} Phi_ij
    loss   = - sum_i W_i phi(r_i),     phi(r) = 1 / r (P, AP, nERR) or 1 / log2(1 + r) (nDCG);     u_i = -W_i phi'(r_i)
    dloss/dm_i = sum_j d_ij (u_j - u_i),  d_ij = g_ij a_ij        dloss/dv_i = sum_j e_ij (u_i - u_j),  e_ij = d_ij x_ij a_ij
The weights W (constants of the backward) are smooth_ref.weights — the same function the smooth-rank objectives are checked with — from the
labels and the hard positions: the input index under opt_ideal, else the rank by (r ascending, index ascending), or the positions handed in
(`pos`: the GPU gate evaluates the re-sorted forms WITH the kernel's own positions).

Error model (u = 2^-24, c = C_GAUSS; every bound is c u times a sum of magnitudes, one unit per rounding, each pair term with its
conditioning in x; x itself carries a few roundings — the difference of the means, the sum of the variances, the reciprocal root, the
product — counted as ONE unit of relative error that c absorbs, as it absorbs the ulps of erfc and exp):
  * Phi_ij: c u (Phi + g |x|)  (its own rounding; dPhi/dx = -g times the error of x, |x| c u);  E_r = sum_j of that + c u r (the summation).
  * W, phi(r) and u = -W phi'(r): smooth_ref's E_W and its phi formulas with this E_r.
  * a mean-gradient term d_ij (u_j - u_i): c u d |u_j - u_i| (4 + 2 x^2)  (g: one rounding and 2 x^2 of conditioning; a; the difference; the
    product — and the summation folded in) + d (E_u_i + E_u_j);  a variance-gradient term: the same with |e| and (6 + 2 x^2).
  * underflow: fp32 has no number between 0 and TINY = 2^-126 that a flushing unit keeps, so g = exp(-x^2) — and with it Phi's tail —
    carries an ABSOLUTE error of up to TINY wherever it falls below (|x| > 9.3: the learned-head and saturated regimes): a gradient term
    gets TINY a |u_j - u_i| (TINY |x| a^2 |u_j - u_i| for the variance) and TINY for its own product, a rank TINY per partner.  The
    reference's fp32 returns exactly 0 for such elements (1e-45 in float64); without the floor their bound, 1e-50, could not be met by
    any fp32 arithmetic.
  * loss = -sum W phi(r): the terms' errors + c u sum |term|;  the batch total: f64_loss_bounds.batch_total.
A query the re-sorted top-k filter drops, and a query of length 0, is exactly 0 everywhere (valid 0).  NaN (a list without a relevant
document in the unfiltered forms of AP, nERR and nDCG: W = 0 / 0) is demanded exactly where the restatement has it.  A one-document list has
no pair: both gradients are exactly 0 even where the loss is NaN (the reference masks the diagonal out of its sum).

C_GAUSS is 2 x the worst need of the reference's own fp32 arithmetic — torch_composition below in fp32 on the CPU — on the small batches of
the GPU gate (SMALL_BATCHES), rounded up to a half: the factor 2 because another summation order is legitimate.  measure_fp32_need()
re-measures it (tests/test_gauss_metric_cpu.py), so the constant cannot drift.
"""
import math

import numpy as np
import torch

import smooth_ref as SR
from f64_bounds import U
from f64_loss_bounds import LN2, _f64, _qlen, labels_like

C_GAUSS = 3.5     # 2 x 1.75, the fp32 need of the eager-torch composition on SMALL_BATCHES (grad_mu; grad_var 1.73, ranks 1.23, loss_q 0.45)
NAMES = ("P", "AP", "nERR", "nDCG")
SQRT_PI = math.sqrt(math.pi)
TINY = 2.0 ** -126    # the smallest normal fp32 number

# (L, lens, regime) of the GPU gate.  One batch per register-form width (L <= 64, 128, 192, 256, 384, 512: 1, 2, 3, 4, 6, 8 documents per
# lane) holding the lengths 0, 1, 2, width - 1, width; the workgroup forms at L = 1024 and 2048 with short lists beside the long ones; one
# batch of every length class at L = 4096.  Regimes: `wide` variances in [0.05, 1.05] with means 2 N(0, 1), `head` (a learned
# sigmoid * limit_delta head) in [1e-4, 1e-2] with means 0.5 N(0, 1), `sat` the saturated case v = 1e-6 — all on a mean offset of 1e3.
GATE_BATCHES = [(64, [0, 1, 2, 63, 64], "wide"), (128, [0, 1, 2, 127, 128], "wide"), (192, [0, 1, 2, 191, 192], "wide"),
                (256, [0, 1, 2, 255, 256], "wide"), (384, [0, 1, 2, 383, 384], "wide"), (512, [0, 1, 2, 511, 512], "wide"),
                (64, [1, 2, 17, 64], "head"), (128, [65, 128, 3], "sat"), (128, [100, 128], "head"),
                (1024, [0, 1, 2, 40, 513, 1024], "wide"), (2048, [0, 1, 2, 40, 1025, 2048], "head"),
                (4096, [0, 1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1251, 2048, 4096], "wide")]
SMALL_BATCHES = [b for b in GATE_BATCHES if b[0] <= 128]
OFFSET = 1e3


def gate_inputs(L, lens, regime, seed):
    """A ragged batch [len(lens), L] -> (mus, vars, labels fp32 with NaN in the padding, lens int32)."""
    rng = np.random.default_rng(seed)
    B = len(lens)
    m, v, y = (np.full((B, L), np.nan, np.float32) for _ in range(3))
    for q, n in enumerate(lens):
        if n == 0:
            continue
        if regime == "wide":
            mq, vq = 2.0 * rng.standard_normal(n), rng.uniform(0.05, 1.05, n)
        elif regime == "head":
            mq, vq = 0.5 * rng.standard_normal(n), rng.uniform(1e-4, 1e-2, n)
        else:
            mq, vq = 0.5 * rng.standard_normal(n), np.full(n, 1e-6)
        yq = -np.sort(-labels_like(1, n, "mslr", rng)[0])
        yq[0] = max(yq[0], 1.0)                                  # every list holds a relevant document
        m[q, :n], v[q, :n], y[q, :n] = (mq + OFFSET).astype(np.float32), vq.astype(np.float32), yq
    return m, v, y, np.asarray(lens, np.int32)


def positions(r):
    """0-based rank by (r ascending, index ascending): torch.sort(ranks) with ties by index."""
    r = _f64(r)
    n = r.size
    order = np.lexsort((np.arange(n), r))
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    return pos


class PairStage:
    """The metric-independent half of a query: expected ranks, the pair derivatives d and e, and the coefficients K of |u_j - u_i| in their bounds."""

    def __init__(self, m, v, c=C_GAUSS):
        m, v = _f64(m), _f64(v)
        n = m.size
        self.n, self.c = n, c
        with np.errstate(invalid="ignore", divide="ignore"):
            a = 1.0 / np.sqrt(2.0 * (v[:, None] + v[None, :]))
            x = (m[:, None] - m[None, :]) * a
            off = ~np.eye(n, dtype=bool)
            Phi = np.where(off, 0.5 * torch.special.erfc(torch.from_numpy(x)).numpy(), 0.0)
            x2 = x * x
            g = np.exp(-x2) / SQRT_PI
            self.r = 1.0 + Phi.sum(1)
            self.E_r = c * U * ((Phi + np.where(off, g * np.abs(x), 0.0)).sum(1) + self.r) + (n - 1) * TINY
            self.d = np.where(off, g * a, 0.0)
            self.e = self.d * x * a
            self.K_mu = c * U * self.d * (4.0 + 2.0 * x2) + np.where(off, TINY * a, 0.0)
            self.K_var = c * U * np.abs(self.e) * (6.0 + 2.0 * x2) + np.where(off, TINY * np.abs(x) * a * a, 0.0)
        self.d_row, self.e_row, self.ae_row = self.d.sum(1), self.e.sum(1), np.abs(self.e).sum(1)
        self.pos = positions(self.r)


def query(stage, y, metric, top_k, opt_ideal, max_label, pos=None, fault=None):
    """One query from its PairStage -> dict(loss, E_loss, grad_mu, E_grad_mu, grad_var, E_grad_var, ranks, E_ranks, valid, W, pos).
    pos: the hard positions to weigh by (default: the input index under opt_ideal, else the order of the float64 ranks).  fault = (i, rel):
    W_i moved by rel of its value (the planted fault of the tests)."""
    n, c = stage.n, stage.c
    cu = c * U
    if pos is None:
        pos = np.arange(n) if opt_ideal else stage.pos
    pos = np.asarray(pos, dtype=np.int64)
    W, E_W, keep = SR.weights(y, pos, metric, top_k, opt_ideal, max_label, c)
    if fault is not None:
        W = W.copy()
        W[fault[0]] *= 1.0 + fault[1]
    r, E_r = stage.r, stage.E_r
    z = np.zeros(n)
    out = dict(ranks=r, E_ranks=E_r, W=W, pos=pos)
    if not keep:
        return dict(out, loss=0.0, E_loss=0.0, grad_mu=z, E_grad_mu=z, grad_var=z, E_grad_var=z, valid=0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        if metric == "nDCG":
            lg = np.log2(r + 1.0)
            E_lg = E_r / ((r + 1.0) * LN2) + cu * lg
            term = W / lg
            E_term = E_W / lg + np.abs(term) * (E_lg / lg + cu)
            ui = W / (LN2 * (1.0 + r) * lg * lg)
            E_ui = E_W / (LN2 * (1.0 + r) * lg * lg) + np.abs(ui) * (cu + E_r / (1.0 + r) + 2.0 * E_lg / lg)
        else:
            term = W / r
            E_term = E_W / r + np.abs(W) * E_r / r ** 2 + cu * np.abs(term)
            ui = W / r ** 2
            E_ui = E_W / r ** 2 + 2.0 * np.abs(W) * E_r / r ** 3 + cu * np.abs(ui)
        loss = -term.sum()
        E_loss = E_term.sum() + cu * np.abs(term).sum()
        if n == 1:                                               # no pair: the diagonal is masked out of the reference's sum
            gm, gv, E_gm, E_gv = z, z, z, z
        else:
            gm = stage.d @ ui - ui * stage.d_row
            gv = ui * stage.e_row - stage.e @ ui
            nz = np.flatnonzero(ui != 0.0)
            if n > 256 and 8 * nz.size < n:                      # a short cut-off: sum_j K_ij |u_j - u_i| from the few nonzero u alone
                au = np.abs(ui[nz])
                s_mu, s_var = stage.K_mu[:, nz] @ au, stage.K_var[:, nz] @ au
                AD = np.abs(ui[None, :] - ui[nz, None])
                s_mu[nz], s_var[nz] = (stage.K_mu[nz] * AD).sum(1), (stage.K_var[nz] * AD).sum(1)
            else:
                AD = np.abs(ui[None, :] - ui[:, None])
                s_mu, s_var = (stage.K_mu * AD).sum(1), (stage.K_var * AD).sum(1)
            E_gm = s_mu + stage.d @ E_ui + E_ui * stage.d_row + (n - 1) * TINY
            E_gv = s_var + np.abs(stage.e) @ E_ui + E_ui * stage.ae_row + (n - 1) * TINY
    nz = lambda a: np.nan_to_num(a, nan=0.0)
    return dict(out, loss=loss, E_loss=nz(E_loss), grad_mu=gm, E_grad_mu=nz(E_gm), grad_var=gv, E_grad_var=nz(E_gv), valid=1.0)


def stages(mus, vars_, lens, c=C_GAUSS):
    """The PairStage of every query of a padded batch (the expensive, metric-independent half: compute once, share)."""
    mus = np.asarray(mus)
    B, L = mus.shape
    return [PairStage(mus[q, :_qlen(lens, q, L)], vars_[q, :_qlen(lens, q, L)], c) for q in range(B)]


KEYS = ("grad_mu", "E_grad_mu", "grad_var", "E_grad_var", "ranks", "E_ranks")


def batch(st, labels, lens, metric, top_k=None, opt_ideal=True, max_label=None, pos=None):
    """A padded batch from its stages -> dict(q, loss_q, E_loss_q, grad_mu, E_grad_mu, grad_var, E_grad_var, ranks, E_ranks [B, L], valid_q,
    pos [B, L] (-1 on padding)).  max_label None: the batch maximum (nERR).  pos [B, L]: positions to weigh by (the kernel's own)."""
    labels = np.asarray(labels)
    B, L = labels.shape
    if max_label is None:
        max_label = SR.batch_max_label(labels, lens)
    res = dict(q=np.arange(B), loss_q=np.zeros(B), E_loss_q=np.zeros(B), valid_q=np.zeros(B), pos=np.full((B, L), -1, np.int64))
    for k in KEYS:
        res[k] = np.zeros((B, L))
    for q in range(B):
        n = st[q].n
        if n == 0:
            continue
        out = query(st[q], labels[q, :n], metric, top_k, opt_ideal, max_label, None if pos is None or opt_ideal else pos[q, :n])
        res["loss_q"][q], res["E_loss_q"][q], res["valid_q"][q] = out["loss"], out["E_loss"], out["valid"]
        res["pos"][q, :n] = out["pos"]
        for k in KEYS:
            res[k][q, :n] = out[k]
    return res


def torch_composition(mus, vars_, labels, metric, top_k, opt_ideal, max_label, const_std=None):
    """The reference's own op sequence for ONE unpadded query, restated in eager torch in the precision and on the device of `mus` (a [n]
    tensor): get_expected_rank (get_expected_rank_const with vars_ None), then the objective, then autograd -> (loss, grad_mu, grad_var or
    None, ranks), or zeros where the reference filters the query.  Used to measure what the fp32 evaluation this kernel replaces needs of the
    float64 bounds (the profile times a batched form of the same op sequence, profiles/prof_gauss_metric.py eager_loss_grad)."""
    m = mus.detach().clone().view(1, -1).requires_grad_(True)
    v = None if vars_ is None else vars_.detach().clone().view(1, -1).requires_grad_(True)
    y = labels.view(1, -1).to(m.dtype)
    n = m.size(1)
    sub = m.unsqueeze(2) - m.unsqueeze(1)                        # prob_utils.py:15
    pv = 2 * torch.as_tensor(const_std, dtype=m.dtype, device=m.device) ** 2 if v is None else v.unsqueeze(2) + v.unsqueeze(1)     # :24, :87
    Phi = 0.5 * torch.erfc(sub / torch.sqrt(2 * pv))             # :70
    r = (torch.triu(Phi, diagonal=1) + torch.tril(Phi, diagonal=-1)).sum(2) + 1.0     # :72-73
    nat = torch.arange(n, dtype=m.dtype, device=m.device).view(1, -1) + 1.0
    k = n if not top_k else min(int(top_k), n)
    kdiv = n if not top_k else int(top_k)
    yb = y.clamp(0, 1)
    if opt_ideal:
        rr, yy, bb = r, y, yb
    else:
        rr, idx = torch.sort(r, dim=1)
        yy, bb = torch.gather(y, 1, idx), torch.gather(yb, 1, idx)
    gains = torch.pow(2.0, yy) - 1.0
    zeros = torch.zeros(n, dtype=m.dtype, device=m.device)
    if not opt_ideal and top_k:
        crit = {"P": bb, "AP": bb, "nERR": yy, "nDCG": gains}[metric][:, :k].sum()
        if float(crit) == 0.0:
            return torch.zeros((), dtype=m.dtype), zeros, None if v is None else zeros, r.detach().view(-1)
    if metric == "P":
        val = (nat[:, :k] / rr[:, :k] * bb[:, :k]).sum(1) / kdiv
    elif metric == "AP" and not opt_ideal and not top_k:
        val = (torch.cumsum(bb, 1) / rr * bb).sum(1) / bb.sum(1)
    elif metric == "AP":
        pre = torch.cumsum(nat / rr, 1) / nat
        val = (pre[:, :k] * bb[:, :k]).sum(1) / bb[:, :k].sum(1)
    elif metric == "nERR":
        def err(lab, inv_rank):
            sat = (torch.pow(2.0, lab[:, :k]) - 1.0) / 2.0 ** float(max_label)
            cas = torch.ones_like(sat)
            cas[:, 1:] = torch.cumprod(1.0 - sat, 1)[:, :-1]
            return (inv_rank[:, :k] * sat * cas).sum(1)
        val = err(yy, 1.0 / rr) / err(y, 1.0 / nat)
    else:
        idcg = ((torch.pow(2.0, y) - 1.0) / torch.log2(nat + 1.0)).sum(1)
        val = ((gains / torch.log2(rr + 1.0))[:, :k] / idcg.view(-1, 1)).sum(1)
    loss = -val.sum()
    if not loss.requires_grad:
        return loss.detach(), zeros, None if v is None else zeros, r.detach().view(-1)
    loss.backward()
    gz = lambda t: zeros if t.grad is None else t.grad.view(-1)
    return loss.detach(), gz(m), None if v is None else gz(v), r.detach().view(-1)


OUTPUTS = ("ranks", "loss_q", "grad_mu", "grad_var")


def need_of(got, ref, E):
    """Worst |got - ref| / E over the elements with E > 0 (E evaluated at c = 1: the constant the data needs)."""
    got, ref, E = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, E))
    ok = (E > 0) & np.isfinite(ref)
    return float(np.max(np.abs(got[ok] - ref[ok]) / E[ok])) if ok.any() else 0.0


def measure_fp32_need(top_ks=(None, 1, 10)):
    """The constant the reference's fp32 arithmetic (torch_composition on fp32 CPU tensors) needs on SMALL_BATCHES, per output, over the 4
    metrics x both modes x top_ks.  The re-sorted forms are evaluated with the fp32 run's own order, as the kernel's are."""
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for k, (L, lens, regime) in enumerate(SMALL_BATCHES):
        m, v, y, n = gate_inputs(L, lens, regime, seed=900 + k)
        st = stages(m, v, n, c=1.0)
        for q, nq in enumerate(lens):
            if nq == 0:
                continue
            mq, vq, yq = (torch.from_numpy(a[q, :nq].copy()) for a in (m, v, y))
            for metric in NAMES:
                for oi in (True, False):
                    for tk in top_ks:
                        loss, gm, gv, r32 = torch_composition(mq, vq, yq, metric, tk, oi, 4.0)
                        ref = query(st[q], y[q, :nq], metric, tk, oi, 4.0, pos=None if oi else positions(r32.numpy()))
                        for name, got, rk, ek in (("ranks", r32.numpy(), "ranks", "E_ranks"), ("loss_q", [float(loss)], "loss", "E_loss"),
                                                  ("grad_mu", gm.numpy(), "grad_mu", "E_grad_mu"), ("grad_var", gv.numpy(), "grad_var", "E_grad_var")):
                            worst[name] = max(worst[name], need_of(got, np.atleast_1d(ref[rk]), np.atleast_1d(ref[ek])))
    return worst
