"""Float64 restatement, with ELEMENT-WISE error bounds, of the smooth-rank metric objectives (csrc/smoothmetric.hip): P, AP, nERR and nDCG
of ptranking/metric/smooth_metric/metric_as_opt_objective.py on the smooth ranks of get_approx_ranks (approxNDCG.py:19-27).

Per query of n documents, scores s, presorted labels y:
    r_i    = 1 + sum_{j != i} rs(alpha (s_j - s_i))
    loss   = - sum_i W_i phi(r_i),     phi(r) = 1 / r (P, AP, nERR) or 1 / log2(1 + r) (nDCG)
    grad_k = sum_i c_i d_ik - c_k sum_j d_kj,     c_i = -W_i phi'(r_i),   d_ij = alpha y_ij (1 - y_ij)
The weights W (constants of the backward) are listed in include/ptranking_amd.h; `weights()` restates them.

Error model: that of f64_loss_bounds._approx_query (E_pi, E_d, _dp; u = 2^-24, c = C_APPROX — the same family: sigmoid pair sums, a reciprocal
or a log2, one scaling), extended by
  * phi = 1 / r: term = W / r carries E_W / r + W E_r / r^2 + c u |term|; c_i = W / r^2 carries E_W / r^2 + 2 W E_r / r^3 + c u c_i;
  * E_W, the weight's own error.  Hard positions come from an exact sort: no error.  Each gain 2^y - 1, division and product costs c u
    relative; a scan by position (AP's suffix sum, the re-sorted full-list AP's count, nERR's prefix product) is an in-order chain — the kernel
    walks a chunk of ch = ceil(n / 64) positions, joins the chunks over 6 steps and walks the chunk again — and costs c u sqrt(2 ch + 6) of
    the sum of its terms (f64_loss_bounds.chain_factor; the product: of the sum of its factors' relative errors + 1):
        P      W = (pos + 1) b / Kdiv                               E_W = c u W
        AP     W = (pos + 1) T / S, T a suffix sum of bp / (p + 1)    E_W = c u W (3 + chain)   (term division, S, the scaling; + the chain)
        AP*    W = b cnt / S (opt_ideal = 0, top_k None)             E_W = c u W (2 + chain)
        nERR   sat = g / 2^max_label: 2 c u relative; f = 1 - sat by subtraction: c u (2 sat + f) absolute; E_p = prod_{p' < p} f: relative
               sum eps_f + c u chain; the ideal ERR a sum of sat E / (p + 1): per term 2 c u + rel(E) + 2 c u, + c u for the sum;
               W = sat E / ideal: rel(sat) + rel(E) + rel(ideal) + 2 c u
        nDCG   W = g / IDCG: c u (gain) + 2 c u (the IDCG: its discounts and its sum) + c u                     E_W = 4 c u W
A query the re-sorted top-k filter drops, and a query of length 0, is exactly 0 everywhere (valid 0).  NaN (a list without a relevant
document in the unfiltered forms of AP, nERR and nDCG: W = 0 / 0) is demanded exactly where the restatement has it (f64_loss_bounds.gate_nan):
the loss and every gradient element of the list (NaN c_i times a pair derivative).  A one-document list has no pair: its gradient is
c - c, exactly 0 or NaN with c, as the reference's backward through the diagonal of its difference matrix gives.
"""
import numpy as np

from f64_bounds import U
from f64_loss_bounds import C_APPROX, LN2, _dp, _f64, _gain, _qlen, _sig, chain_factor

def hard_positions(s):
    """0-based rank by (score descending, index ascending)."""
    n = s.size
    order = np.lexsort((np.arange(n), -_f64(s)))
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    return pos


def weights(y, pos, metric, top_k, opt_ideal, max_label, c=C_APPROX):
    """W [n], E_W [n], keep (False: the query is filtered) from the labels y (ideal order) and the hard positions pos."""
    y = _f64(y)
    n = y.size
    K = n if not top_k or top_k <= 0 else min(int(top_k), n)
    kdiv = float(n if not top_k or top_k <= 0 else top_k)
    filt = (not opt_ideal) and bool(top_k) and top_k > 0
    b = np.clip(y, 0.0, 1.0)
    g = _gain(y)
    top = pos < K
    inv = np.empty(n, dtype=np.int64)
    inv[pos] = np.arange(n)                                      # document at position p
    chain = chain_factor(2 * (-(-n // 64)) + 6)
    cu = c * U
    with np.errstate(divide="ignore", invalid="ignore"):
        if metric == "P":
            W = np.where(top, (pos + 1.0) * b / kdiv, 0.0)
            E = cu * np.abs(W)
            crit = b[top].sum()
        elif metric == "AP" and not opt_ideal and not (top_k and top_k > 0):
            bp = b[inv]
            cnt = np.cumsum(bp)[pos]
            W = b * cnt / b.sum()
            E = cu * np.abs(W) * (2.0 + chain)
            crit = 1.0
        elif metric == "AP":
            bp = np.where(np.arange(n) < K, b[inv] / (np.arange(n) + 1.0), 0.0)
            T = np.cumsum(bp[::-1])[::-1][pos]
            S = b[top].sum()
            W = np.where(top, (pos + 1.0) * T / S, 0.0)
            E = cu * np.abs(W) * (3.0 + chain)
            crit = S
        elif metric == "nERR":
            sat = g / 2.0 ** float(max_label)

            def cascade(satp):
                f = 1.0 - satp
                eps = cu * (2.0 * satp / f + 1.0)
                Ep = np.concatenate([[1.0], np.cumprod(f)[:-1]])
                rel = np.concatenate([[0.0], np.cumsum(eps)[:-1]]) + cu * chain
                return Ep, rel
            Ep, relp = cascade(sat[inv])
            num = np.where(top, sat * Ep[pos], 0.0)
            rel_num = 2.0 * cu + relp[pos] + cu
            Ei, reli = cascade(sat)
            terms = np.where(np.arange(n) < K, sat * Ei / (np.arange(n) + 1.0), 0.0)
            ideal = terms.sum()
            E_ideal = (terms * (4.0 * cu + reli)).sum() + cu * ideal
            W = np.where(top, num / ideal, 0.0)
            E = np.abs(W) * (rel_num + E_ideal / ideal + cu)
            crit = y[top].sum()
        else:
            idcg = (g / np.log2(np.arange(n) + 2.0)).sum()
            W = np.where(top, g / idcg, 0.0)
            E = 4.0 * cu * np.abs(W)
            crit = g[top].sum()
    keep = n > 0 and not (filt and crit == 0.0)
    if not keep:
        W, E = np.zeros(n), np.zeros(n)
    return W, np.where(np.isfinite(E), E, 0.0), keep


class PairStage:
    """The metric-independent half of a query: smooth ranks and pair derivatives with their bounds (f64_loss_bounds._approx_query)."""

    def __init__(self, s, alpha, c=C_APPROX):
        s = _f64(s)
        n = s.size
        self.n, self.c = n, c
        x = alpha * (s[None, :] - s[:, None])                    # [i, j] = alpha (s_j - s_i)
        ax = np.abs(x)
        yv = _sig(x)
        off = ~np.eye(n, dtype=bool)
        self.r = 1.0 + np.where(off, yv, 0.0).sum(1)
        self.E_r = np.where(off, _dp(yv, ax, c), 0.0).sum(1) + c * U * self.r
        self.d = np.where(off, alpha * yv * (1.0 - yv), 0.0)
        self.E_d = np.where(off, c * U * alpha * (yv * (1.0 - yv) * (2.0 + ax) + 1.0), 0.0)
        self.d_row, self.E_d_row = self.d.sum(1), self.E_d.sum(1)
        self.pos = hard_positions(s)


def query(stage, y, metric, top_k, opt_ideal, max_label, fault=None):
    """One query from its PairStage -> dict(loss, E_loss, grad, E_grad, ranks, E_ranks, valid, W).  fault = (i, rel): W_i moved by rel of its
    value (the planted fault of the tests)."""
    n, c = stage.n, stage.c
    cu = c * U
    pos = np.arange(n) if opt_ideal else stage.pos
    W, E_W, keep = weights(y, pos, metric, top_k, opt_ideal, max_label, c)
    if fault is not None:
        W = W.copy()
        W[fault[0]] *= 1.0 + fault[1]
    r, E_r = stage.r, stage.E_r
    if not keep:
        z = np.zeros(n)
        return dict(loss=0.0, E_loss=0.0, grad=z, E_grad=z, ranks=r, E_ranks=E_r, valid=0.0, W=W)
    with np.errstate(invalid="ignore"):
        if metric == "nDCG":
            lg = np.log2(r + 1.0)
            E_lg = E_r / ((r + 1.0) * LN2) + cu * lg
            term = W / lg
            E_term = E_W / lg + np.abs(term) * (E_lg / lg + cu)
            ci = W / (LN2 * (1.0 + r) * lg * lg)
            E_ci = E_W / (LN2 * (1.0 + r) * lg * lg) + np.abs(ci) * (cu + E_r / (1.0 + r) + 2.0 * E_lg / lg)
        else:
            term = W / r
            E_term = E_W / r + np.abs(W) * E_r / r ** 2 + cu * np.abs(term)
            ci = W / r ** 2
            E_ci = E_W / r ** 2 + 2.0 * np.abs(W) * E_r / r ** 3 + cu * np.abs(ci)
        loss = -term.sum()
        E_loss = E_term.sum() + cu * np.abs(term).sum()
        if n == 1:                                               # no pair: +c - c through the reference's diagonal (0, or NaN with c)
            grad, E_grad = ci - ci, np.zeros(1)
        else:
            d, E_d, aci = stage.d, stage.E_d, np.abs(ci)
            grad = d.T @ ci - ci * stage.d_row                   # T[i, j] = c_i d_ij: +T to j, -T to i
            E_grad = (d.T @ E_ci + E_d.T @ aci + E_ci * stage.d_row + aci * stage.E_d_row
                      + 2.0 * cu * (d.T @ aci + aci * stage.d_row))
    return dict(loss=loss, E_loss=np.nan_to_num(E_loss, nan=0.0), grad=grad, E_grad=np.nan_to_num(E_grad, nan=0.0), ranks=r, E_ranks=E_r,
                valid=1.0, W=W)


def batch_max_label(labels, lens):
    labels = np.asarray(labels)
    B, L = labels.shape
    vals = [labels[q, :_qlen(lens, q, L)].max() for q in range(B) if _qlen(lens, q, L) > 0]
    return float(max(vals)) if vals else 0.0


def stages(preds, lens, alpha, c=C_APPROX):
    """The PairStage of every query of a padded batch (the expensive, metric-independent half: compute once, share)."""
    preds = np.asarray(preds)
    B, L = preds.shape
    return [PairStage(preds[q, :_qlen(lens, q, L)], alpha, c) for q in range(B)]


def smooth(st, labels, lens, metric, top_k=None, opt_ideal=True, max_label=None):
    """A padded batch from its stages -> dict(q, loss_q, E_loss_q, grad, E_grad, ranks, E_ranks [B, L], valid_q).  max_label None: the batch
    maximum (nERR)."""
    labels = np.asarray(labels)
    B, L = labels.shape
    if max_label is None:
        max_label = batch_max_label(labels, lens)
    res = dict(q=np.arange(B), loss_q=np.zeros(B), E_loss_q=np.zeros(B), valid_q=np.zeros(B))
    for k in ("grad", "E_grad", "ranks", "E_ranks"):
        res[k] = np.zeros((B, L))
    for q in range(B):
        n = st[q].n
        if n == 0:
            continue
        out = query(st[q], labels[q, :n], metric, top_k, opt_ideal, max_label)
        res["loss_q"][q], res["E_loss_q"][q], res["valid_q"][q] = out["loss"], out["E_loss"], out["valid"]
        for k in ("grad", "E_grad", "ranks", "E_ranks"):
            res[k][q, :n] = out[k]
    return res


def torch_composition(preds, labels, metric, alpha, top_k, opt_ideal, max_label):
    """The reference's own op sequence for ONE unpadded query, restated in eager torch in the precision and on the device of `preds` (a [n]
    leaf tensor): get_approx_ranks, then the objective, then autograd -> (loss, grad), or (0, 0) where the reference filters the query.
    Used to measure what the fp32 evaluation this kernel replaces needs of the float64 bounds."""
    import torch
    s = preds.detach().clone().view(1, -1).requires_grad_(True)
    y = labels.view(1, -1).to(s.dtype)
    n = s.size(1)
    x = alpha * (s.unsqueeze(1) - s.unsqueeze(2))                # [b, i, j] = alpha (s_j - s_i)
    e = torch.exp(-x.abs())
    ind = torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    r = ind.sum(2) + 0.5
    nat = torch.arange(n, dtype=s.dtype, device=s.device).view(1, -1) + 1.0
    k = n if not top_k else min(int(top_k), n)
    kdiv = n if not top_k else int(top_k)
    yb = y.clamp(0, 1)
    if opt_ideal:
        rr, yy, bb = r, y, yb
    else:
        rr, idx = torch.sort(r, dim=1)
        yy, bb = torch.gather(y, 1, idx), torch.gather(yb, 1, idx)
    gains = torch.pow(2.0, yy) - 1.0
    if not opt_ideal and top_k:
        crit = {"P": bb, "AP": bb, "nERR": yy, "nDCG": gains}[metric][:, :k].sum()
        if float(crit) == 0.0:
            return torch.zeros((), dtype=s.dtype), torch.zeros(n, dtype=s.dtype)
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
    loss.backward()
    return loss.detach(), s.grad.view(-1)
