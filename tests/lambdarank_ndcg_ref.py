"""Float64 restatement of the truncated, normalised lambdarank (csrc/tree.hip tree_lambdarank_ndcg_kernel; include/ptranking_amd.h states the
rule) with ELEMENT-WISE error bounds, and an eager-torch fp32 evaluation of the same closed form.  The rule is this project's own, modelled
on LightGBM's LambdarankNDCG; LightGBM is installed nowhere this project is tested, so nothing here is compared with it.

For one query of n documents: scores s, labels y >= 0, g = 2^y - 1, r(i) the 0-based rank in predicted order (a higher score first, equal
scores by original index), D(r) = 1 / log2(r + 2), T the truncation level, sigma the sigmoid's steepness:
    maxDCG = sum of the min(T, n) largest gains, in descending order, times D(position);  inv = 1 / maxDCG (0 where maxDCG is 0)
    a pair {i, j} counts iff y_i != y_j and min(r(i), r(j)) < T;  hi: its larger label, lo: the other;  ds = s_hi - s_lo
    delta = (g_hi - g_lo) |D(r(hi)) - D(r(lo))| inv,  divided by (0.01 + |ds|) under norm where the query's scores are not all equal
    p = 1 / (1 + exp(sigma ds)),  lam = sigma delta p,  h = sigma^2 delta p (1 - p)
    grad[hi] -= lam, grad[lo] += lam, hess[hi] += h, hess[lo] += h, S += 2 lam
    under norm and S > 0: every grad and hess of the query times log2(1 + S) / S
With T >= n, norm off and sigma 1 this is tree_ref.pair_query(pair_type='NoTies', weighting='DeltaNDCG', eps=1, hessian='sum') on every
list with a relevant document, up to that form's 1e-16 Hessian floor (tests/test_lambdarank_ndcg_cpu.py: 4e-16 at worst).

Bounds: the error model of tests/f64_loss_bounds.py and tests/tree_ref.py (u = 2^-24, c the constant of the gate):
  * gains and discounts carry c u relative; |g_i - g_j| carries c u (g_i + g_j), |D_i - D_j| carries c u (D_i + D_j);
  * maxDCG: each term g D carries 3 c u (gain, discount, product), the sum c u sum |terms|; inv one more c u relative;
  * delta: the factors' errors to first order and c u per product.  The score difference is taken BEFORE sigma and rounds relative to
    |ds|, so 0.01 + |ds| carries 2 c u relative, its reciprocal and the product c u each: 4 c u of delta under norm;
  * p = sigmoid(-sigma ds) carries f64_loss_bounds._dp (absolute), p (1 - p) carries |1 - 2 p| dp + c u p (1 - p) as tree_ref's Hessian;
  * lam and h: E_delta through the product, the sigmoid's error, and 3 c u for sigma (sigma^2) and the products;
  * a document's partner sum is an in-order chain: c u chain_factor(m) sum_j |term|, m = n - 1 for a document ranked in the first T, and
    min(T, n) for any other (it meets the first T ranks only);
  * S = sum_i sum_j lam_ij: the documents' chain bounds, and c u S for the reduction;
  * the factor f = log2(1 + S) / S from the relative error of S: d log f / d log S = -(1 - S / ((1 + S) ln(1 + S))), between -1 and 0, so
    E_f = f (kappa E_S / S + 3 c u), kappa = 1 - S / ((1 + S) ln(1 + S)) (log1p, the change of base and the division: c u each; a form
    that rounds 1 + S before the logarithm loses u / ln(1 + S) relative, which this bound does not grant);
  * the scaled result: E f + |x| E_f + c u |x f|.
Exact results (E = 0): a list of one document, of equal labels, or without a relevant document is exactly 0 in both outputs (the last
differs from weighting='DeltaNDCG', which is NaN there).  A NaN score or label: NaN on every document of the list (gate_nan demands it).

The gate constant is f64_loss_bounds.C_PAIR = 2.5, unchanged.  Measured worst need (err / E times C_PAIR) over the inputs of
tests/test_lambdarank_ndcg_gpu.py (gpu_inputs below), every T x norm x sigma of its gate on the straddle batch:
    the eager fp32 form (CPU, test_lambdarank_ndcg_cpu.py)   1.47 (TreeObjective's first round, T 1; the straddle batch 1.42, T 1)
    the kernel on an MI355X (test_lambdarank_ndcg_gpu.py)    0.51 (the lists shorter than T; the straddle batch 0.46, T 30 without norm)
The kernel adds each document's partners into four interleaved chains; with one chain per sum it needed 2.52 on the 4096-document list
(T 5000, sigma 2), 0.36 with four.  The bound above still charges one chain of the full length.
"""
import math

import numpy as np
import torch

import f64_loss_bounds as FB
import tree_ref as TR
from f64_bounds import U

C = FB.C_PAIR
LN2 = math.log(2.0)
CHUNK = 512                      # rows per block of the S pass over a long list
FAULTS = ("trunc_le", "maxdcg_all", "no_001", "ln_factor", "sigma_hess", "divide_equal")


def _max_dcg(g, T):
    """(maxDCG, E without c u) over the min(T, n) largest gains."""
    n = g.size
    k = min(int(T), n)
    terms = -np.sort(-g)[:k] * FB._disc(n)[:k]
    return float(terms.sum()), 4.0 * float(np.abs(terms).sum())


def _block(s, y, g, D, rank, rows, cols, T, sigma, spread, inv, rel_inv, c, hess=True):
    """Pair terms of documents `rows` against partners `cols` -> (signed lam, |lam|, E_lam, h, E_h), each [len(rows), len(cols)], 0 where
    the pair does not count."""
    yi, yj = y[rows, None], y[None, cols]
    M = (yi != yj) & (np.minimum(rank[rows, None], rank[None, cols]) < T)
    hi = yi > yj
    d0 = s[rows, None] - s[None, cols]
    ds = np.where(hi, d0, -d0)
    dg = np.abs(g[rows, None] - g[None, cols])
    E_dg = c * U * (g[rows, None] + g[None, cols])
    dD = np.abs(D[rows, None] - D[None, cols])
    E_dD = c * U * (D[rows, None] + D[None, cols])
    delta = dg * dD * inv
    E_delta = (E_dg * dD + dg * E_dD) * inv + delta * (rel_inv + 2.0 * c * U)
    if spread:
        q = 0.01 + np.abs(ds)
        delta, E_delta = delta / q, E_delta / q + 4.0 * c * U * delta / q
    x = sigma * ds
    p = FB._sig(-x)
    dp = FB._dp(p, np.abs(x), c)
    lam = sigma * delta * p
    E_lam = sigma * (E_delta * p + delta * dp) + 3.0 * c * U * lam
    lam, E_lam = np.where(M, lam, 0.0), np.where(M, E_lam, 0.0)
    signed = np.where(hi, -lam, lam)
    if not hess:
        return signed, lam, E_lam, None, None
    pq = p * (1.0 - p)
    h = sigma * sigma * delta * pq
    E_h = sigma * sigma * (E_delta * pq + delta * (np.abs(1.0 - 2.0 * p) * dp + c * U * pq)) + 3.0 * c * U * h
    return signed, lam, E_lam, np.where(M, h, 0.0), np.where(M, E_h, 0.0)


def query(s, y, T=30, sigma=1.0, norm=True, c=C, rows=None):
    """One query -> (grad, E_grad, hess, E_hess), float64; rows: only these documents of the query (every partner still counts, and S is
    taken over the whole list)."""
    s, y = np.asarray(s, np.float64), np.asarray(y, np.float64)
    n = s.size
    rows = np.arange(n) if rows is None else np.asarray(rows)
    k = len(rows)
    if n == 0:
        return (np.zeros(0),) * 4
    if np.isnan(s).any() or np.isnan(y).any():
        return np.full(k, np.nan), np.zeros(k), np.full(k, np.nan), np.zeros(k)
    rank = TR.ranks_of(s)
    g, D = FB._gain(y), FB._disc(n)[rank]
    mx, a_mx = _max_dcg(g, T)
    inv = 1.0 / mx if mx > 0.0 else 0.0
    rel_inv = (c * U * a_mx / mx + c * U) if mx > 0.0 else 0.0
    spread = bool(norm) and s.max() != s.min()
    Tn = min(int(T), n)
    top = np.nonzero(rank < T)[0]
    every = np.arange(n)
    chain = lambda r: c * U * np.where(rank[r] < T, FB.chain_factor(n - 1), FB.chain_factor(Tn))
    args = (T, sigma, spread, inv, rel_inv, c)

    def sums(r, hess):
        """Partner sums of documents r that all rank in the first T (partners: everyone) or all outside (partners: the first T)."""
        out = [np.zeros(len(r)) for _ in range(6)]
        for inside in (True, False):
            sel = np.nonzero((rank[r] < T) == inside)[0]
            if sel.size == 0:
                continue
            sg, lam, E_lam, h, E_h = _block(s, y, g, D, rank, r[sel], every if inside else top, *args, hess=hess)
            ch = chain(r[sel])
            out[0][sel], out[1][sel], out[2][sel] = sg.sum(1), lam.sum(1), E_lam.sum(1) + ch * lam.sum(1)
            if hess:
                out[3][sel], out[4][sel] = h.sum(1), E_h.sum(1) + ch * h.sum(1)
        return out

    grad, L, E_L, hess, E_hess, _ = sums(rows, True)
    E_grad = E_L                                              # sum_j E_lam + chain sum_j |lam|: the same terms, signed or not
    if norm:
        S = E_S = 0.0
        if 2 * Tn < n:                                        # few pairs: the first T against everyone, everyone else against the first T
            for a in range(0, n, CHUNK):
                _, Lc, E_Lc, _, _, _ = sums(every[a:a + CHUNK], False)
                S, E_S = S + Lc.sum(), E_S + E_Lc.sum()
        else:                                                 # the pair matrix is symmetric: the blocks on and above the diagonal, mirrored
            La, Ea = np.zeros(n), np.zeros(n)
            for a in range(0, n, CHUNK):
                r = every[a:a + CHUNK]
                _, lam, E_lam, _, _ = _block(s, y, g, D, rank, r, every[a:], *args, hess=False)
                La[r] += lam.sum(1)
                Ea[r] += E_lam.sum(1)
                La[a + len(r):] += lam[:, len(r):].sum(0)
                Ea[a + len(r):] += E_lam[:, len(r):].sum(0)
            S, E_S = La.sum(), (Ea + chain(every) * La).sum()
        E_S += c * U * S
        if S > 0.0:
            f = math.log2(1.0 + S) / S
            kappa = 1.0 - S / ((1.0 + S) * math.log1p(S))
            E_f = f * (kappa * E_S / S + 3.0 * c * U)
            E_grad = E_grad * f + np.abs(grad) * E_f + c * U * np.abs(grad * f)
            E_hess = E_hess * f + np.abs(hess) * E_f + c * U * np.abs(hess * f)
            grad, hess = grad * f, hess * f
    return grad, E_grad, hess, E_hess


def batch(preds, labels, group, max_rows=None, seed=0, **kw):
    """query over a ragged batch -> dict(idx, grad, E_grad, hess, E_hess), aligned with idx, the flat indices of the compared documents
    (at most max_rows per list: tree_ref.sample_rows)."""
    preds, labels = np.asarray(preds), np.asarray(labels)
    off, rng = TR.offsets_of(group), np.random.default_rng(seed)
    parts = {k: [] for k in ("idx", "grad", "E_grad", "hess", "E_hess")}
    for a, b in zip(off[:-1], off[1:]):
        rows = TR.sample_rows(int(b - a), max_rows, rng)
        res = query(preds[a:b], labels[a:b], rows=rows, **kw)
        parts["idx"].append(a + rows)
        for k, v in zip(("grad", "E_grad", "hess", "E_hess"), res):
            parts[k].append(v)
    return {k: np.concatenate(v) if v else np.zeros(0) for k, v in parts.items()}


def gate(got_grad, got_hess, ref, what, c=C):
    """tree_ref.gate: element-wise, NaN exactly where the restatement is NaN.  Returns the worst err / E."""
    return TR.gate(got_grad, got_hess, ref, what, c)


# ---------------------------------------------------------------------------------------------------------------------------- fp32, eager
def eager_query(s, y, T=30, sigma=1.0, norm=True, fault=None, dtype=torch.float32):
    """The closed form evaluated by eager torch in `dtype` on the CPU, over the whole n x n pair matrix: what a plain fp32 implementation
    computes.  The gate must pass it, or the bounds are impossible.  fault: one of FAULTS, planted for the gate to reject."""
    assert fault is None or fault in FAULTS, fault
    sn, yn = np.asarray(s, np.float64), np.asarray(y, np.float64)
    n = sn.size
    if n == 0:
        return np.zeros(0), np.zeros(0)
    S, Y = torch.tensor(sn, dtype=dtype), torch.tensor(yn, dtype=dtype)
    rank = torch.from_numpy(TR.ranks_of(sn))
    g = torch.exp2(Y) - 1.0
    disc = 1.0 / torch.log2(torch.arange(n, dtype=dtype) + 2.0)
    D = disc[rank]
    k = n if fault == "maxdcg_all" else min(int(T), n)
    mx = (torch.sort(g, descending=True).values[:k] * disc[:k]).sum()
    inv = 1.0 / mx if float(mx) > 0.0 else torch.zeros((), dtype=dtype)
    lo_rank = torch.minimum(rank[:, None], rank[None, :])
    M = (Y[:, None] != Y[None, :]) & ((lo_rank <= T) if fault == "trunc_le" else (lo_rank < T))
    hi = Y[:, None] > Y[None, :]
    d0 = S[:, None] - S[None, :]
    ds = torch.where(hi, d0, -d0)                              # the difference first, sigma after
    delta = (g[:, None] - g[None, :]).abs() * (D[:, None] - D[None, :]).abs() * inv
    if norm and (fault == "divide_equal" or float(S.max()) != float(S.min())):
        delta = delta / ((0.0 if fault == "no_001" else 0.01) + ds.abs())
    p = torch.sigmoid(-(sigma * ds))
    zero = torch.zeros((), dtype=dtype)
    lam = torch.where(M, sigma * delta * p, zero)
    h = torch.where(M, (sigma if fault == "sigma_hess" else sigma * sigma) * delta * (p * (1.0 - p)), zero)
    grad, hess = torch.where(hi, -lam, lam).sum(1), h.sum(1)
    if norm:
        total = lam.sum()
        if float(total) > 0.0:
            f = (torch.log1p(total) if fault == "ln_factor" else torch.log1p(total) / LN2) / total
            grad, hess = grad * f, hess * f
    return grad.double().numpy(), hess.double().numpy()


def eager_batch(preds, labels, group, **kw):
    preds, labels = np.asarray(preds), np.asarray(labels)
    off = TR.offsets_of(group)
    grad, hess = np.zeros(preds.size), np.zeros(preds.size)
    for a, b in zip(off[:-1], off[1:]):
        grad[a:b], hess[a:b] = eager_query(preds[a:b], labels[a:b], **kw)
    return grad, hess


# ---------------------------------------------------------------------------------------------------------------------------- data
# first and last length of every form and of every length class the host launches separately (tests/test_tree_gpu.py STRADDLE)
STRADDLE = [0, 1, 2, 16, 17, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1251, 2048, 2049, 4096]
MAX_ROWS = 320                                                   # documents compared per long list (tree_ref.sample_rows)
CONFIGS = [(T, norm, sigma) for T in (1, 2, 30, 5000) for norm in (True, False) for sigma in (1.0, 2.0)]      # the gate's settings
MID = [1, 17, 64, 130, 300]
NAN_GROUP = [17, 64, 130, 3]
OBJECTIVE_GROUP = [12, 1, 18, 64, 3, 0, 200]
IDENTITY_GROUP = [2, 5, 17, 64, 130]


def gpu_inputs():
    """name -> (preds, labels, group): every input list of tests/test_lambdarank_ndcg_gpu.py's gated tests, in fp32."""
    out = {"straddle": TR.tree_inputs(STRADDLE, seed=11) + (STRADDLE,)}
    s, y = TR.tree_inputs(MID, seed=5)
    out["equal labels"] = (s, np.full_like(y, 2.0), MID)
    out["no relevant document"] = (s, np.zeros_like(y), MID)
    out["equal scores"] = (np.full_like(s, 0.25), y, MID)
    out["shorter than T"] = TR.tree_inputs([3, 29, 30, 31], seed=6) + ([3, 29, 30, 31],)
    out["offset 1e3"] = TR.tree_inputs(MID, seed=5, offset=1e3) + (MID,)
    out["nan"] = TR.tree_inputs(NAN_GROUP, seed=13) + (NAN_GROUP,)
    s, y = TR.tree_inputs(IDENTITY_GROUP, seed=17)
    out["identity"] = (s, plant_relevant(y, IDENTITY_GROUP), IDENTITY_GROUP)
    _, y = TR.tree_inputs(OBJECTIVE_GROUP, seed=21)
    for r in range(3):                                           # TreeObjective's rounds: scores of growing spread
        p = (np.random.default_rng(40 + r).standard_normal(len(y)) * (r + 1)).astype(np.float32)
        out[f"objective round {r}"] = (p, y, OBJECTIVE_GROUP)
    return out


_REFS = {}


def reference(name, T, norm, sigma):
    """batch() on gpu_inputs()[name], computed once per process and shared (callers must not change it)."""
    key = (name, T, norm, sigma)
    if key not in _REFS:
        s, y, group = gpu_inputs()[name]
        _REFS[key] = batch(s, y, group, max_rows=MAX_ROWS, T=T, norm=norm, sigma=sigma)
    return _REFS[key]


def plant_relevant(y, group):
    """Labels with a relevant document in every list of two or more documents that drew none (the first document gets grade 1)."""
    y = np.array(y, np.float32)
    off = TR.offsets_of(group)
    for a, b in zip(off[:-1], off[1:]):
        if b - a >= 2 and not (y[a:b] > 0).any():
            y[a] = 1.0
    return y
