"""Float64 restatement of the tree frame's custom objectives (csrc/tree.hip; the reference's ptranking/ltr_tree/util/lightgbm_util.py) with
ELEMENT-WISE error bounds, over LightGBM's ragged layout (flat arrays + group sizes).  The error model is the one written at the top of
tests/f64_loss_bounds.py, with that module's measured constants (C_PAIR for the pairwise objectives, C_LIST for ListNet); the gate is
f64_bounds.gate through f64_loss_bounds.gate_nan.

Closed form per document i, over the partners j != i of its query that pass the pair mask (d = s_i - s_j, sig the logistic function):
    grad_i = sum_j w_ij eps (sig(eps d) - (1 + clip(y_i - y_j, -1, 1)) / 2)
    h_ij   = max(eps^2 sig(d) (1 - sig(d)), 1e-16) w_ij                 (the Hessian's sigmoid ignores eps; the floor precedes the weight)
    hess_i = sum_j sign(rank_j - rank_i) h_ij   ('reference')     sum_j h_ij   ('sum')     1   ('constant')
    w_ij   = 1 | |G_i - G_j| |D_i - D_j|, G = (2^y - 1) / IDCG, D = 1 / log2(rank + 2) ('DeltaNDCG') | |g_i - g_j|, g = 2^y - 1 ('DeltaGain')
with rank 0-based in predicted order: a higher score first, equal scores by original index (the reference's np.flip(np.argsort(preds)) is
not stable: the fixtures never compare ties against it).  It reproduces per_query_gradient_hessian_lambda in float64 to 1e-12 over every
pair type x weighting x eps (tests/test_tree_cpu.py against tests/golden/tree.npz).

Bounds (u = 2^-24, c = C_PAIR):
  * the score difference rounds relative to |d| and reaches the gradient's sigmoid as c u |eps d|: dp = c u (max(p, 1 - p) + p (1 - p)
    (1 + |eps d|)) absolute on p, and on p - t (f64_loss_bounds._dp);
  * a pair term T = w eps (p - t):  E_T = eps (E_w |p - t| + w dp) + c u |T|;
  * the Hessian term takes its error from the sigmoid's absolute error through p (1 - p): with ph = sig(d),
    E_h0 = eps^2 (|1 - 2 ph| dph + c u ph (1 - ph)), E_h = E_h0 w + max(h0, 1e-16) E_w + c u h;
  * weights: G and D carry c u relative; |G_i - G_j| carries c u (G_i + G_j) (0 on equal labels), |D_i - D_j| carries c u (D_i + D_j),
    |g_i - g_j| carries c u (g_i + g_j) (0 on equal labels);
  * the partner sums are in-order chains of n - 1 terms: c u sqrt(n - 1) sum_j |T_ij|, and for the Hessian — signed or not —
    c u sqrt(n - 1) sum_j |h_ij|: never relative to |hess_i|, which the signs can cancel to nothing.
Exact results: a list of one document and a list without a pair under the mask are exactly 0 (E = 0); 'constant' is exactly 1.
NaN: without a relevant document the normalised gains are 0 / 0, and every document with a pair under the mask is NaN under DeltaNDCG, as
the reference.  A NaN score or label gives NaN on every document of that list (the product's rule, COVERAGE a9): the reference agrees
under 'All' pairs, where every document meets the NaN one.

ListNet: grad = softmax(s) - softmax(gain), hess = p (1 - p); f64_loss_bounds._log_softmax's bounds with C_LIST, E_h = |1 - 2 p| E_p + c u h.
"""
import numpy as np
import torch

import f64_loss_bounds as FB
from f64_bounds import U

PAIR_TYPES = ("All", "NoTies", "No00", "00")                  # PTR_TREE_PAIRS_*, triu_indice's four masks
WEIGHTINGS = (None, "DeltaNDCG", "DeltaGain")                 # PTR_TREE_W_*
HESSIANS = ("reference", "sum", "constant")                   # PTR_TREE_HESS_*
GAIN_TYPES = ("Power", "Label")                               # PTR_TREE_GAIN_*
H_FLOOR = 1e-16


def ranks_of(s):
    """0-based rank in predicted order: score descending, original index ascending."""
    n = len(s)
    order = np.lexsort((np.arange(n), -np.asarray(s, np.float64)))
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    return rank


def pair_mask(y, pair_type, rows=None):
    """[len(rows), n] boolean: partner j of document i = rows[k] passes (symmetric, no diagonal).  rows None: every document."""
    n = len(y)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    yi, yj = y[rows, None], y[None, :]
    both0 = (yi == 0) & (yj == 0)
    m = {"All": np.ones((len(rows), n), bool), "NoTies": yi != yj, "No00": ~both0, "00": both0}[pair_type]
    return m & (rows[:, None] != np.arange(n)[None, :])


def _weights(y, rank, weighting, c, rows):
    """(w, E_w) [len(rows), n]."""
    n = len(y)
    if weighting is None:
        return np.ones((len(rows), n)), np.zeros((len(rows), n))
    g = FB._gain(y)
    differ = y[rows, None] != y[None, :]
    if weighting == "DeltaGain":
        w = np.abs(g[rows, None] - g[None, :])
        return w, np.where(differ, c * U * (g[rows, None] + g[None, :]), 0.0)
    assert weighting == "DeltaNDCG", weighting
    idcg = (FB._gain(-np.sort(-y)) * FB._disc(n)).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        G = g / idcg
    D = FB._disc(n)[rank]
    dG, dD = np.abs(G[rows, None] - G[None, :]), np.abs(D[rows, None] - D[None, :])
    E_dG = np.where(differ, c * U * (G[rows, None] + G[None, :]), 0.0)
    E_dD = c * U * (D[rows, None] + D[None, :])
    w = dG * dD
    return w, E_dG * dD + dG * E_dD + c * U * w


def pair_abs_terms(s, y, pair_type="NoTies", weighting=None, eps=1.0):
    """sum_j |T_ij| and sum_j |h_ij| per document: what a gradient / Hessian element's error is measured against."""
    s, y = np.asarray(s, np.float64), np.asarray(y, np.float64)
    M = pair_mask(y, pair_type)
    w, _ = _weights(y, ranks_of(s), weighting, 1.0, np.arange(s.size))
    d = s[:, None] - s[None, :]
    t = 0.5 * (1.0 + np.clip(y[:, None] - y[None, :], -1.0, 1.0))
    ph = FB._sig(d)
    T = np.where(M, w * eps * (FB._sig(eps * d) - t), 0.0)
    h = np.where(M, np.maximum(eps * eps * ph * (1.0 - ph), H_FLOOR) * w, 0.0)
    return np.abs(T).sum(1), np.abs(h).sum(1)


def pair_query(s, y, pair_type="NoTies", weighting=None, eps=1.0, hessian="reference", c=FB.C_PAIR, rows=None):
    """One query -> (grad, E_grad, hess, E_hess), float64 [n]; rows: only these documents of the query ([len(rows)] each; every partner
    still counts)."""
    s, y = np.asarray(s, np.float64), np.asarray(y, np.float64)
    n = s.size
    rows = np.arange(n) if rows is None else np.asarray(rows)
    const = hessian == "constant"
    if n == 0:
        return (np.zeros(0),) * 4
    if np.isnan(s).any() or np.isnan(y).any():
        k = len(rows)
        return np.full(k, np.nan), np.zeros(k), (np.ones(k) if const else np.full(k, np.nan)), np.zeros(k)
    rank = ranks_of(s)
    M = pair_mask(y, pair_type, rows)
    w, Ew = _weights(y, rank, weighting, c, rows)
    d = s[rows, None] - s[None, :]
    x = eps * d
    p = FB._sig(x)
    t = 0.5 * (1.0 + np.clip(y[rows, None] - y[None, :], -1.0, 1.0))
    with np.errstate(invalid="ignore"):
        T = w * eps * (p - t)
        ET = eps * (Ew * np.abs(p - t) + w * FB._dp(p, np.abs(x), c)) + c * U * np.abs(T)
        T, ET = np.where(M, T, 0.0), np.where(M, ET, 0.0)
        chain = c * U * FB.chain_factor(n - 1)
        grad, E_grad = T.sum(1), ET.sum(1) + chain * np.abs(T).sum(1)
        if const:
            return grad, np.where(np.isfinite(grad), E_grad, 0.0), np.ones(len(rows)), np.zeros(len(rows))
        ph = FB._sig(d)
        h0 = eps * eps * ph * (1.0 - ph)
        E_h0 = eps * eps * (np.abs(1.0 - 2.0 * ph) * FB._dp(ph, np.abs(d), c) + c * U * ph * (1.0 - ph))
        hf = np.maximum(h0, H_FLOOR)
        h = hf * w
        E_h = E_h0 * w + hf * Ew + c * U * np.abs(h)
        sign = np.where(rank[None, :] > rank[rows, None], 1.0, -1.0) if hessian == "reference" else 1.0
        assert hessian in ("reference", "sum"), hessian
        h, E_h = np.where(M, h, 0.0), np.where(M, E_h, 0.0)
        hess, E_hess = (sign * h).sum(1), E_h.sum(1) + chain * np.abs(h).sum(1)
    return grad, np.where(np.isfinite(grad), E_grad, 0.0), hess, np.where(np.isfinite(hess), E_hess, 0.0)


def listnet_query(s, y, gain_type="Power", hessian="reference", c=FB.C_LIST):
    s, y = np.asarray(s, np.float64), np.asarray(y, np.float64)
    n = s.size
    const = hessian == "constant"
    if n == 0:
        return (np.zeros(0),) * 4
    if np.isnan(s).any() or np.isnan(y).any():
        return np.full(n, np.nan), np.zeros(n), (np.ones(n) if const else np.full(n, np.nan)), np.zeros(n)
    gains = FB._gain(y) if gain_type == "Power" else y
    assert gain_type in GAIN_TYPES, gain_type
    lsm, E_lsm, ps = FB._log_softmax(s, c)
    _, E_ly, py = FB._log_softmax(gains, c)
    E_ps, E_py = ps * (E_lsm + c * U), py * (E_ly + c * U)
    grad = ps - py
    E_grad = E_ps + E_py + c * U * np.abs(grad)
    if n == 1:
        E_grad = np.zeros(1)                                      # p = 1 on both sides, exactly
        E_ps = np.zeros(1)
    if const:
        return grad, E_grad, np.ones(n), np.zeros(n)
    hess = ps * (1.0 - ps)
    return grad, E_grad, hess, np.abs(1.0 - 2.0 * ps) * E_ps + c * U * hess


def offsets_of(group):
    g = np.asarray(group).astype(np.int64)
    return np.concatenate([[0], np.cumsum(g)])


def ragged(fn, preds, labels, group, *args, **kw):
    """Run a per-query restatement over LightGBM's layout -> dict(idx, grad, E_grad, hess, E_hess): flat float64, idx = every document."""
    preds, labels = np.asarray(preds), np.asarray(labels)
    off = offsets_of(group)
    assert off[-1] == preds.size == labels.size
    out = {k: np.zeros(preds.size) for k in ("grad", "E_grad", "hess", "E_hess")}
    for a, b in zip(off[:-1], off[1:]):
        res = fn(preds[a:b], labels[a:b], *args, **kw)
        for k, v in zip(("grad", "E_grad", "hess", "E_hess"), res):
            out[k][a:b] = v
    out["idx"] = np.arange(preds.size)
    return out


def sample_rows(n, max_rows, rng):
    """The documents of a long list that a test compares: the first and the last 64 and a random draw of the rest (every partner still
    enters their sums; the bit-identity tests cover every document)."""
    if max_rows is None or n <= max_rows:
        return np.arange(n)
    mid = rng.choice(np.arange(64, n - 64), size=max_rows - 128, replace=False)
    return np.sort(np.concatenate([np.arange(64), mid, np.arange(n - 64, n)]))


def pair(preds, labels, group, max_rows=None, seed=0, **kw):
    """pair_query over a ragged batch.  max_rows: compare at most that many documents of a list (sample_rows); the result's arrays are
    aligned with idx, the flat indices of the compared documents."""
    if max_rows is None:
        return ragged(pair_query, preds, labels, group, **kw)
    preds, labels = np.asarray(preds), np.asarray(labels)
    off, rng = offsets_of(group), np.random.default_rng(seed)
    parts = {k: [] for k in ("idx", "grad", "E_grad", "hess", "E_hess")}
    for a, b in zip(off[:-1], off[1:]):
        rows = sample_rows(int(b - a), max_rows, rng)
        res = pair_query(preds[a:b], labels[a:b], rows=rows, **kw)
        parts["idx"].append(a + rows)
        for k, v in zip(("grad", "E_grad", "hess", "E_hess"), res):
            parts[k].append(v)
    return {k: np.concatenate(v) if v else np.zeros(0) for k, v in parts.items()}


def listnet(preds, labels, group, **kw):
    return ragged(listnet_query, preds, labels, group, **kw)


def gate(got_grad, got_hess, ref, what, c):
    """Gate a (grad, hess) pair element-wise against ragged()'s result; NaN exactly where the restatement is NaN.  Returns the worst err/E."""
    idx = ref["idx"].astype(np.int64)
    w = FB.gate_nan(np.asarray(got_grad, np.float64)[idx], ref["grad"], ref["E_grad"], f"{what} grad", c)
    return max(w, FB.gate_nan(np.asarray(got_hess, np.float64)[idx], ref["hess"], ref["E_hess"], f"{what} hess", c))


# ---------------------------------------------------------------------------------------------------------------------------- fp32, eager
def eager_pair_query(s, y, pair_type="NoTies", weighting=None, eps=1.0, hessian="reference", dtype=torch.float32):
    """The closed form evaluated by eager torch in `dtype` on the CPU (what a straightforward fp32 implementation computes): the gate must
    pass it, or the bounds are impossible.  The difference is taken before eps, as the error model assumes."""
    sn, yn = np.asarray(s, np.float64), np.asarray(y, np.float64)
    n = sn.size
    S, Y = torch.tensor(sn, dtype=dtype), torch.tensor(yn, dtype=dtype)
    rank = torch.from_numpy(ranks_of(sn))
    M = torch.from_numpy(pair_mask(yn, pair_type))
    d = S[:, None] - S[None, :]
    p = torch.sigmoid(eps * d)
    t = 0.5 * (1.0 + torch.clamp(Y[:, None] - Y[None, :], -1.0, 1.0))
    w = torch.ones(n, n, dtype=dtype)
    g = torch.exp2(Y) - 1.0
    if weighting == "DeltaGain":
        w = (g[:, None] - g[None, :]).abs()
    elif weighting == "DeltaNDCG":
        disc = 1.0 / torch.log2(torch.arange(n, dtype=dtype) + 2.0)
        idcg = ((torch.exp2(torch.sort(Y, descending=True).values) - 1.0) * disc).sum()
        G, D = g / idcg, disc[rank]
        w = (G[:, None] - G[None, :]).abs() * (D[:, None] - D[None, :]).abs()
    zero = torch.zeros((), dtype=dtype)
    grad = torch.where(M, w * (eps * (p - t)), zero).sum(1)
    if hessian == "constant":
        return grad.double().numpy(), np.ones(n)
    ph = torch.sigmoid(d)
    h = torch.clamp((eps * eps) * (ph * (1.0 - ph)), min=H_FLOOR) * w
    if hessian == "reference":
        h = torch.where(rank[None, :] > rank[:, None], h, -h)
    return grad.double().numpy(), torch.where(M, h, zero).sum(1).double().numpy()


# ---------------------------------------------------------------------------------------------------------------------------- data
def tree_inputs(group, seed=0, offset=0.0, mix="mslr", distinct=True):
    """fp32 (preds, labels) over `group`: scores correlated with the label, spread over a few units (the range of a boosted model's raw
    scores), optionally offset by a common value; distinct: pairwise distinct within a query (asserted)."""
    g = np.random.default_rng(seed)
    N = int(np.sum(group))
    y = FB.labels_like(1, max(N, 1), mix, g)[0, :N]
    s = (0.8 * y + 1.5 * g.standard_normal(N) + offset).astype(np.float32)
    if distinct:
        off = offsets_of(group)
        for a, b in zip(off[:-1], off[1:]):
            for _ in range(64):
                if len(np.unique(s[a:b])) == b - a:
                    break
                s[a:b] = (s[a:b].astype(np.float64) + 1e-3 * g.standard_normal(b - a)).astype(np.float32)
            assert len(np.unique(s[a:b])) == b - a
    return s, y.astype(np.float32)
