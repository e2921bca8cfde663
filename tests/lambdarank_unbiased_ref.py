"""Float64 restatement of the position-debiased lambdarank (csrc/tree.hip tree_lambdarank_ndcg_kernel<G, true> and
tree_position_bias_update_kernel; include/ptranking_amd.h states the rule) with ELEMENT-WISE error bounds, and an eager-torch fp32 form.
The rule is this project's own, modelled on Unbiased LambdaMART (Hu et al. 2019); it is compared with no other implementation.

Steps 1 to 3, 5 and 6 are lambdarank_ndcg_ref's.  Per counted pair, b(d) = min(position[d], P - 1):
    w = 1 / (t+[b(hi)] t-[b(lo)]),  lam = lam0 w,  h = h0 w,  c = delta log(1 + exp(-sigma ds))
    cost+[b(hi)] += c / t-[b(lo)],  cost-[b(lo)] += c / t+[b(hi)]                 (not multiplied by step 6's factor)
Bounds, on top of lambdarank_ndcg_ref's model (u = 2^-24, c the gate's constant):
  * w: two more roundings, 2 c u of lam and of h (the two reciprocals are correctly rounded, u / 2 each; their product and the product
    with lam0 u each: 3 u < 2 c u);
  * the softplus sp = max(-x, 0) + log1p(exp(-|x|)), x = sigma ds, one _dp-style term: c u (2 sp + 2 min(p, 1 - p) (1 + |x|)) — the
    logarithm and the sum round relative to sp, x carries 2 u |x| through d sp / d x = -p <= 1, exp(-|x|) carries (2 + |x|) u through
    d log1p(e) / d log e = min(p, 1 - p);
  * c / t: E_delta and E_sp through the product, and 3 c u (delta sp, the reciprocal, the product with it);
  * a document's two cost sums are chains like its lam sum: c u chain_factor(m) of the sum;
  * the fixed point: 2^-33 per contributing document and side; the integer sums are exact.
A pair's terms do not depend on the positions or the biases, and a document's own bias leaves its sums as a factor: query() evaluates the
pair matrix once and serves every variant (position, P, biases) of a test by matrix-vector products.
"""
import numpy as np
import torch

import f64_loss_bounds as FB
import lambdarank_ndcg_ref as LR
import tree_ref as TR
from f64_bounds import U

C = FB.C_PAIR
FIXED = 2.0 ** -33
FLOOR = 2.0 ** -10


def classes(n, pos, P):
    return np.minimum(np.arange(n) if pos is None else np.asarray(pos, np.int64), P - 1)


def _pairs(s, y, g, D, rank, r, cols, T, sigma, spread, inv, rel_inv, c):
    """Pair terms of documents r against partners cols, before any bias -> two lists (r is the pair's hi | r is its lo) of the six matrices
    lam, E_lam, h, E_h, cost, E_cost, each 0 where the pair does not count.  lam and h as lambdarank_ndcg_ref._block, plus 2 c u for w."""
    yi, yj = y[r, None], y[None, cols]
    M, hi = (yi != yj) & (np.minimum(rank[r, None], rank[None, cols]) < T), yi > yj
    ds = np.where(hi, 1.0, -1.0) * (s[r, None] - s[None, cols])
    dg, dD = np.abs(g[r, None] - g[None, cols]), np.abs(D[r, None] - D[None, cols])
    delta = dg * dD * inv
    E_delta = (c * U * (g[r, None] + g[None, cols]) * dD + dg * c * U * (D[r, None] + D[None, cols])) * inv + delta * (rel_inv + 2.0 * c * U)
    if spread:
        q = 0.01 + np.abs(ds)
        delta, E_delta = delta / q, E_delta / q + 4.0 * c * U * delta / q
    x = sigma * ds
    p = FB._sig(-x)
    dp, pq, sp = FB._dp(p, np.abs(x), c), p * (1.0 - p), np.logaddexp(0.0, -x)
    lam, h, cc = sigma * delta * p, sigma * sigma * delta * pq, delta * sp
    E_lam = sigma * (E_delta * p + delta * dp) + 5.0 * c * U * lam
    E_h = sigma * sigma * (E_delta * pq + delta * (np.abs(1.0 - 2.0 * p) * dp + c * U * pq)) + 5.0 * c * U * h
    E_sp = c * U * (2.0 * sp + 2.0 * np.minimum(p, 1.0 - p) * (1.0 + np.abs(x)))
    E_cc = E_delta * sp + delta * E_sp + 3.0 * c * U * cc
    mats = (lam, E_lam, h, E_h, cc, E_cc)
    return [np.where(M & hi, m, 0.0) for m in mats], [np.where(M & ~hi, m, 0.0) for m in mats]


def query(s, y, variants, T=30, sigma=1.0, norm=True, c=C):
    """One query under each variant (position or None, P, biases [2, P] or None) -> a list of (grad, E_grad, hess, E_hess over every
    document, cost [2, P], E_cost [2, P]), float64."""
    s, y = np.asarray(s, np.float64), np.asarray(y, np.float64)
    n = s.size
    bad = np.isnan(s).any() or np.isnan(y).any()
    res, live = [], []
    for pos, P, t in variants:
        if bad or (pos is not None and (np.asarray(pos) < 0).any()):
            res.append([np.full(n, np.nan), np.zeros(n), np.full(n, np.nan), np.zeros(n), np.zeros((2, P)), np.zeros((2, P))])
        else:
            res.append([np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((2, P)), np.zeros((2, P))])
            live.append((res[-1], classes(n, pos, P), 1.0 / (np.ones((2, P)) if t is None else np.asarray(t, np.float64)), np.zeros(n)))
    if n == 0 or not live:
        return res
    rank = TR.ranks_of(s)
    g, D = FB._gain(y), FB._disc(n)[rank]
    mx, a_mx = LR._max_dcg(g, T)
    inv = 1.0 / mx if mx > 0.0 else 0.0
    rel_inv = (c * U * a_mx / mx + c * U) if mx > 0.0 else 0.0
    spread = bool(norm) and s.max() != s.min()
    top, every = np.nonzero(rank < T)[0], np.arange(n)
    for a in range(0, n, LR.CHUNK):
        for inside in (True, False):
            r = every[a:a + LR.CHUNK]
            r, cols = r[(rank[r] < T) == inside], every if inside else top
            if r.size == 0 or cols.size == 0:
                continue
            as_hi, as_lo = _pairs(s, y, g, D, rank, r, cols, T, sigma, spread, inv, rel_inv, c)
            ch = c * U * FB.chain_factor(n - 1 if inside else min(int(T), n))
            for out, b, rt, L in live:
                # r as hi: its own 1 / t+ times the partner's 1 / t-; as lo the other way round.  The costs take the partner's alone.
                Hs, Ls = [m @ rt[1][b[cols]] for m in as_hi], [m @ rt[0][b[cols]] for m in as_lo]
                oh, ol = rt[0][b[r]], rt[1][b[r]]
                L[r] = oh * Hs[0] + ol * Ls[0]
                out[0][r], out[1][r] = ol * Ls[0] - oh * Hs[0], oh * Hs[1] + ol * Ls[1] + ch * L[r]
                out[2][r] = oh * Hs[2] + ol * Ls[2]
                out[3][r] = oh * Hs[3] + ol * Ls[3] + ch * out[2][r]
                for k, side in enumerate((Hs, Ls)):
                    np.add.at(out[4][k], b[r], side[4])
                    np.add.at(out[5][k], b[r], side[5] + ch * side[4] + FIXED * (side[4] > 0))
    for out, _, _, L in live:
        S = L.sum()
        if norm and S > 0.0:
            E_S = out[1].sum() + c * U * S
            f = np.log2(1.0 + S) / S
            E_f = f * ((1.0 - S / ((1.0 + S) * np.log1p(S))) * E_S / S + 3.0 * c * U)
            for k in (0, 2):
                out[k + 1] = out[k + 1] * f + np.abs(out[k]) * E_f + c * U * np.abs(out[k] * f)
                out[k] = out[k] * f
    return res


def batch(preds, labels, group, variants, **kw):
    """query over a ragged batch -> per variant a dict(idx, grad, E_grad, hess, E_hess) over every document (tree_ref.gate's form) with
    cost and E_cost [2, P].  variants: (position over the batch or None, P, biases or None)."""
    preds, labels, off = np.asarray(preds), np.asarray(labels), TR.offsets_of(group)
    keys = ("grad", "E_grad", "hess", "E_hess")
    res = [dict({k: np.zeros(preds.size) for k in keys}, idx=np.arange(preds.size), cost=np.zeros((2, P)), E_cost=np.zeros((2, P))) for _, P, _ in variants]
    for a, e in zip(off[:-1], off[1:]):
        got = query(preds[a:e], labels[a:e], [(None if pos is None else pos[a:e], P, t) for pos, P, t in variants], **kw)
        for one, v in zip(res, got):
            for k, x in zip(keys, v):
                one[k][a:e] = x
            one["cost"] += v[4]
            one["E_cost"] += v[5]
    return res


def gate_costs(acc, ref, what, c=C):
    """The int64 accumulator against the restatement's costs, element-wise.  Returns the worst err / E."""
    return FB.gate_nan(np.asarray(acc, np.float64) * 2.0 ** -32, ref["cost"], ref["E_cost"], f"{what} costs", c)


def update(cost, biases, p_norm):
    """The update rule in float64: (new biases [2, P])."""
    cost, out = np.asarray(cost, np.float64), np.array(biases, np.float64)
    for k in range(2):
        if cost[k, 0] > 0.0:
            m = cost[k] > 0.0
            out[k, m] = np.maximum(FLOOR, (cost[k, m] / cost[k, 0]) ** (1.0 / (1.0 + p_norm)))
    return out


def eager_query(s, y, pos=None, P=30, biases=None, T=30, sigma=1.0, norm=True):
    """The closed form in eager fp32 torch over the n x n pair matrix (what a plain fp32 implementation computes) -> grad, hess, cost."""
    sn, yn = np.asarray(s, np.float64), np.asarray(y, np.float64)
    n, f32 = sn.size, torch.float32
    S, Y, rank = torch.tensor(sn, dtype=f32), torch.tensor(yn, dtype=f32), torch.from_numpy(TR.ranks_of(sn))
    b = torch.from_numpy(classes(n, pos, P))
    rt = 1.0 / (torch.ones(2, P) if biases is None else torch.tensor(np.asarray(biases), dtype=f32))
    g, disc = torch.exp2(Y) - 1.0, 1.0 / torch.log2(torch.arange(n, dtype=f32) + 2.0)
    mx = (torch.sort(g, descending=True).values[:min(int(T), n)] * disc[:min(int(T), n)]).sum()
    inv = 1.0 / mx if float(mx) > 0.0 else torch.zeros(())
    M = (Y[:, None] != Y[None, :]) & (torch.minimum(rank[:, None], rank[None, :]) < T)
    hi = Y[:, None] > Y[None, :]
    d0 = S[:, None] - S[None, :]
    ds = torch.where(hi, d0, -d0)
    delta = (g[:, None] - g[None, :]).abs() * (disc[rank][:, None] - disc[rank][None, :]).abs() * inv
    if norm and float(S.max()) != float(S.min()):
        delta = delta / (0.01 + ds.abs())
    x = sigma * ds
    p = torch.sigmoid(-x)
    other = torch.where(hi, rt[1][b][None, :], rt[0][b][None, :])
    w = torch.where(hi, rt[0][b][:, None], rt[1][b][:, None]) * other
    zero = torch.zeros(())
    lam = torch.where(M, sigma * delta * p * w, zero)
    h = torch.where(M, sigma * sigma * delta * (p * (1.0 - p)) * w, zero)
    cc = torch.where(M, delta * torch.nn.functional.softplus(-x) * other, zero)
    grad, hess = torch.where(hi, -lam, lam).sum(1), h.sum(1)
    cost = torch.zeros(2, P)
    cost[0].index_add_(0, b, torch.where(hi, cc, zero).sum(1))
    cost[1].index_add_(0, b, torch.where(hi, zero, cc).sum(1))
    if norm and float(lam.sum()) > 0.0:
        f = torch.log1p(lam.sum()) / LR.LN2 / lam.sum()
        grad, hess = grad * f, hess * f
    return grad.double().numpy(), hess.double().numpy(), cost.double().numpy()


def given_positions(group, seed=3):
    """Shown positions that collide within a query and exceed every P of the tests (up to 299)."""
    return np.random.default_rng(seed).integers(0, 300, int(np.sum(group))).astype(np.int32)


def draw_biases(P, seed=4):
    return np.random.default_rng(seed + P).uniform(0.2, 1.5, (2, P)).astype(np.float32)


# the gate's variants: default positions and given ones, each under every P, biases drawn in [0.2, 1.5]
VARIANTS = [(given, P) for given in (False, True) for P in (1, 3, 30, 256)]
_REFS = {}


def reference(T, norm, sigma=1.0):
    """batch() on the straddle batch under every variant of VARIANTS, computed once per (T, norm) and shared (callers must not change it)."""
    if (T, norm) not in _REFS:
        s, y, group = LR.gpu_inputs()["straddle"]
        variants = [(given_positions(group) if given else None, P, draw_biases(P)) for given, P in VARIANTS]
        _REFS[(T, norm)] = dict(zip(VARIANTS, batch(s, y, group, variants, T=T, norm=norm, sigma=sigma)))
    return _REFS[(T, norm)]
