"""Float64 references and ELEMENT-WISE error bounds for the ranking-loss kernels (csrc/pairwise.hip + ptr_ring.h, csrc/approxndcg.hip,
csrc/listwise.hip), and the structured scores / labels that make those bounds bite.  The gate itself is f64_bounds.gate.

Why: the loss tests compared against fp32 (the C oracle, the reference's own fp32 outputs) under golden_util.assert_close, 1e-5 relative
with a floor of 1e-6 of the largest value.  A document's gradient is a sum of +- terms over its partners; where they cancel that rule is
as noisy as either side and leans on its floor.  And only the batch total of the loss was ever compared: one query's loss_q could be a
few % wrong in a batch of 4096.  Here every per-query loss, every gradient element and ApproxNDCG's dcg_q / inv_idcg_q / scale get a
bound of their own, computed in float64 from the very fp32 inputs the kernel saw.

Error model, u = 2^-24, c one constant per family (set from GPU measurement, see below):
  * every transcendental and reciprocal the kernel evaluates (exp, log, the sigmoid's 1/(1+e), 2^y - 1, the discount table
    D = 1/log2(rank+2), sqrt) costs c u relative;
  * every reduction costs c u sum |terms|: ApproxNDCG's pair sums, the IDCG, the softmax normaliser, ListMLE's cumulative sums, and
    ptr_sum_f32 over loss_q (the batch total: sum of the per-query bounds + c u sum |loss_q|) — the RankNet / LambdaRank pair sums
    below grow with their in-order chains;
  * a score difference rounds relative to |ds| (never to |s|: a kernel that scaled the scores before subtracting them rounds relative
    to |s| and fails this on the cases with a common offset of ~1e3), and reaches the sigmoid's argument x = sigma ds as c u |x|.
    Through exp that is a relative error of c u |x| of e^-|x|, i.e. an ABSOLUTE error of the sigmoid
        dp = c u (max(p, 1 - p) + p (1 - p) (1 + |x|))
    which is also the absolute error of the gradient factor (p - t, 1 - p or p): whichever of p and 1 - p is near 1 is rounded there, and
    the other is formed from it by a subtraction (exact in fp32, but it keeps the absolute error: about u, not a relative one).  A loss
    term log(a), a = p or 1 - p, therefore carries dp / a + c u |log a| — for a RankNet pair far on the wrong side of 0, -log(1 - p)
    ~ p itself and that is a relative error of u / p;
  * pair weights: G = gain / IDCG and D carry c u relative; |G_i - G_j| carries c u (G_i + G_j) (0 on equal labels: both sides are the
    same fp32 value), |D_i - D_j| carries c u (D_i + D_j) — the cancellation of adjacent discounts deep in a long list;
  * ranks come from an exact sort with index tie-break: no error.
Pair sums (RankNet, LambdaRank) are the exception to the fixed c u sum |terms| of a reduction: their terms are added in order, in long
chains — a lane of the ring kernel adds its ~P / 64 pair losses into one accumulator, a thread of the LDS kernel its DPT x n / 2, and a
gradient element collects its n - 1 partner terms in two such chains — before a short tree joins the chains.  In-order rounding errors
add like a random walk: a chain of m terms costs ~sqrt(m) u sum |terms| (m u at worst).  So the pair sums carry
        E_loss_q = ... + c u sqrt(ceil(P / 64)) sum |l|,      E_grad_i = ... + c u sqrt(n - 1) sum_j |T_ij|
(P pairs of the query: at least one wavefront of 64 lanes shares them in every form).  With a fixed c, the 2.2 M pair losses of a
2100-document query (17 000 per LDS-kernel thread) needed c = 22.6 where the ring kernel's 8128 needed 0.65; a constant that large
would let a 1e-5 bias of every LambdaRank loss through, about what the old relative rule lets through.

The restatement takes the branches of the fp32 arithmetic, not those of exact math:
  * x >= X_ONE: the sigmoid rounds to 1 in fp32.  The gradient factor is exactly 0 and log(1 - p) is BCE's -100 clamp;
  * p (1 - p) < 1e-12 (RankNet, x < 0): the reference's clamped denominator, gradient (p - t) p (1 - p) / 1e-12;
  * RankCosine: |s| <= eps = 1e-8 takes eps and drops the second gradient term.
`pair_inputs` moves the scores of any pair whose sigma |ds| lies within the kernel's rounding of X_ONE or of the clamp (SCREEN_BANDS)
and asserts that such moves are rare (MAX_SCREENED); that band stays covered, unchanged, by tests/golden/losses_knife.npz against the
reference's own outputs.

Exact results (E = 0): padded slots have a gradient of exactly 0 and a zero-length query its formula's loss exactly (0, RankCosine 2).
A query without a relevant document is NaN for LambdaRank (n >= 2) and ApproxNDCG (per-query form) — as the reference — and
`gate_nan` demands NaN exactly where the reference is NaN and nowhere else.

Per loss (i, j partners; t target; w weight; T = a gradient term):
  RankNet / LambdaRank   x = sigma (s_i - s_j)  E_T = sigma (E_w |p - t| + w dp) + c u |T|,  E_l = E_w |l / w| + w (t dp/p + (1-t) dp/(1-p)
                         + c u |log|) + c u |l|;  grad_i = sum_j +-T, loss_q = sum l (LambdaRank: pairs in predicted order, weight
                         |dG| |dD|, target [G_i > G_j]; RankNet: input order, w = 1, t = (1 + clip(y_i - y_j)) / 2)
  ApproxNDCG             y_ij = rs(alpha (s_j - s_i)), pi_i = 1 + sum_{j != i} y_ij:  E_pi = sum dy + c u pi;  lg = log2(1 + pi);
                         dcg = sum g / lg;  c_i = g / (ln2 (1 + pi) lg^2);  d_ij = alpha y (1 - y) with E_d = c u alpha (y (1-y) (2 + |x|)
                         + 1) (the LDS kernel forms 1 - y by subtraction: absolute, as the gradient factor above);  grad scaled by
                         S = sum 1/IDCG (coupled), 1/IDCG (per query) or the caller's override
  ListNet                lsm_i = (s_i - m) - log Z:  E_lsm = c u (|s_i - m| + |log Z| + 1) + E_Z / Z;  softmax and target likewise
  ListMLE                T_i = sum_{k >= i} e_k, loss = sum (log T_i + m) - u_i, grad = e_i sum_{k <= i} 1/T_k - 1; both cumulative
                         sums are in-order chains (of n - i and i + 1 terms) and carry sqrt(chain) as the pair sums do; the loss term is
                         formed as the reference forms it (listmle.py: log-cumsum-exp + max, minus the score), so it rounds relative
                         to |log T_i + m|, not to |l_i|: on a query with a common offset that is the offset
  RankMSE                loss_q = sum d^2, grad = 2 d / B:  c u sum d^2, c u |grad|
  RankCosine             cos = sy / (|s| |y|):  sums c u sum |terms|, sqrt / division c u
"""
import math

import numpy as np
import torch

from f64_bounds import U, d64, gate

# ---- one constant per loss family (c above), set from GPU measurement on an MI355X: each gated test prints `MEASURED <what>: worst err/E
# (c C: needs c >= k)`; k is the constant that data needs.  Worst k over tests/test_loss_bounds_gpu.py:
C_PAIR = 2.5      # RankNet, LambdaRank (pairwise.hip, ptr_ring.h), with the in-order chains of the pair sums: worst 1.68 (RankNet loss_q,
                  # 3 x 2100, the LDS kernel), LambdaRank 1.30 (grad), every ring form included; 1.5x / 1.9x headroom
C_APPROX = 4.0    # ApproxNDCG (approxndcg.hip): worst 2.37 (inv_idcg_q); grad 1.47, dcg_q 0.72; 1.7x headroom.  The C oracle
                  # (in-order fp32 sums): 2.8 at 60 documents
C_LIST = 4.0      # ListNet, ListMLE, RankMSE, RankCosine (listwise.hip): worst 2.20 (RankMSE grad); ListNet 0.89, ListMLE 0.81,
                  # RankCosine 0.54; 1.8x headroom

LN2 = math.log(2.0)
X_ONE = math.log(2.0 ** 25 - 1.0)        # 17.33: from here on 1 / (1 + e^-x) rounds to 1 in fp32
X_DEN = -math.log(1e-12)                 # 27.63: p (1 - p) < 1e-12, RankNet's clamped denominator (x < 0)
SCREEN_BANDS = ((X_ONE - 2.0, X_ONE + 2.0), (X_DEN - 1.0, X_DEN + 1.0))
MAX_SCREENED = 0.01                      # at most this fraction of documents may be moved out of a band
COS_EPS = 1e-8


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _qlen(lens, q, L):
    return L if lens is None else int(min(max(int(lens[q]), 0), L))


def _gain(y):
    return np.exp2(y) - 1.0


def _disc(n):
    return 1.0 / np.log2(np.arange(n, dtype=np.float64) + 2.0)


def _sig(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _dp(p, ax, c):
    """Absolute error of a sigmoid value p, and of 1 - p, at |x| = ax (module docstring)."""
    return c * U * (np.maximum(p, 1.0 - p) + p * (1.0 - p) * (1.0 + ax))


# ---------------------------------------------------------------------------------------------------------------------------- data
def labels_like(B, L, mix, g):
    """Graded labels 0..4: 'mslr' (half irrelevant) or 'yahoo' (a quarter irrelevant)."""
    pr = {"mslr": [0.5, 0.3, 0.13, 0.05, 0.02], "yahoo": [0.25, 0.35, 0.25, 0.1, 0.05]}[mix]
    return g.choice(5, size=(B, L), p=pr).astype(np.float64)


def pair_inputs(B, L, sigma=1.0, mix="mslr", seed=0, quantise=False, offset=0.0, lens="ragged", specials=True, outliers=True, span=14.0,
                every_relevant=False, sort_labels=False):
    """fp32 (preds, labels, lens) shaped like a trained scorer's: scores correlated with the label, sigma |ds| within a query up to ~span
    (below the screened band), ~5 % of queries with one document 21..22 / sigma above the rest (past X_ONE: the rounded-to-1 branch),
    optionally quantised to sigma ds in quarters (ties) and offset by a common ~1e3.  specials: query 0 all-equal labels, 1 one relevant document,
    2 none, 3 length 1 (relevant), 4 length 0, 5 length 1 without a relevant document (B >= 6); lens 'ragged' draws the rest from 1..L
    with every tenth L, 'full' is all L.  sort_labels: each list's labels in descending order, as the reference feeds LambdaRank (its
    grade-0 tail fills whole slots of the ring kernel, which skips the pairs among them).
    every_relevant: no query of length 0 and none without a relevant document (the coupled ApproxNDCG scale S = sum 1/IDCG is inf
    otherwise, and so is every gradient of the batch).  Returns (preds [B, L] fp32, labels [B, L] fp32, lens [B] int32, screened fraction)."""
    g = np.random.default_rng(seed)
    y = labels_like(B, L, mix, g)
    if sort_labels:
        y = -np.sort(-y, axis=1)
    s = 0.6 * y + g.standard_normal((B, L))
    lo, hi = s.min(1, keepdims=True), s.max(1, keepdims=True)
    s = (s - lo) / np.maximum(hi - lo, 1e-30) * (span / sigma) - 0.5 * span / sigma
    n = np.full(B, L, np.int32)
    if lens == "ragged":
        n = g.integers(1, L + 1, size=B).astype(np.int32)
        n[::10] = L
    if specials and B >= 5:
        y[0] = 2.0
        y[1] = 0.0; y[1, g.integers(0, max(1, n[1]))] = 3.0
        y[2] = 0.0; n[2] = max(n[2], 2)
        n[3] = 1; y[3, 0] = 1.0
        n[4] = 0
        if B >= 6:
            n[5] = 1; y[5, 0] = 0.0
    if every_relevant:
        n = np.maximum(n, 1)
        for q in range(B):
            if not (y[q, :n[q]] > 0).any():
                y[q, g.integers(0, n[q])] = 1.0
    if outliers:
        for q in np.nonzero(g.random(B) < 0.05)[0]:
            if n[q] >= 3:
                rest = s[q, :n[q]]
                s[q, :n[q]] = rest.min() + (rest - rest.min()) * (4.0 / max(span, 1e-30))     # the rest spans 4 / sigma
                s[q, g.integers(0, n[q])] = s[q, :n[q]].max() + (21.0 + g.random()) / sigma     # x in 21..26
    if quantise:
        s = np.round(s * 4.0 * sigma) / (4.0 * sigma)                 # sigma ds on a grid of quarters: ties
    s = (s + offset).astype(np.float32)
    moved = _screen(s, n, sigma)
    return s, y.astype(np.float32), n, moved / max(1, int(n.sum()))


def _screen(s, n, sigma):
    """Move documents out of pairs whose sigma |ds| lies in SCREEN_BANDS (in place, fp32); returns the number of moves."""
    moved = 0
    for q in range(s.shape[0]):
        for _ in range(8):
            v = s[q, :n[q]].astype(np.float64)
            x = sigma * np.abs(v[:, None] - v[None, :])
            bad = np.zeros_like(x, dtype=bool)
            for a, b in SCREEN_BANDS:
                bad |= (x >= a) & (x <= b)
            if not bad.any():
                break
            i = int(np.nonzero(bad.any(1))[0][0])
            s[q, i] = np.float32(np.median(np.delete(v, i)))          # into the bulk of the query: sigma |ds| <= span there
            moved += 1
        else:
            raise AssertionError(f"query {q}: could not screen its pairs")
    return moved


def listwise_inputs(B, L, seed=0, offset=0.0, lens="ragged", mix="yahoo"):
    """fp32 (preds, labels, lens) for the listwise losses: scores ~ N(label / 2, 2) with a spread of up to ~30 inside a query (so ListMLE
    takes both of its routes), optionally offset by a common ~1e3; one all-zero score row (RankCosine's eps branch) and the specials of
    pair_inputs (no screening: these losses have no threshold)."""
    g = np.random.default_rng(seed)
    y = labels_like(B, L, mix, g)
    s = 0.5 * y + 2.0 * g.standard_normal((B, L)) * np.where(g.random((B, 1)) < 0.3, 4.0, 1.0)
    n = np.full(B, L, np.int32)
    if lens == "ragged":
        n = g.integers(1, L + 1, size=B).astype(np.int32)
        n[::10] = L
    if B >= 6:
        y[0] = 2.0
        n[3] = 1
        n[4] = 0
        s[5] = 0.0
    return (s + offset).astype(np.float32), y.astype(np.float32), n


def listmle_perm(labels, lens, seed=0):
    """A label-descending permutation with ties broken at random (what arg_shuffle_ties gives), int64 [B, L]."""
    g = np.random.default_rng(seed)
    B, L = labels.shape
    perm = np.tile(np.arange(L, dtype=np.int64), (B, 1))
    for q in range(B):
        n = _qlen(lens, q, L)
        r = g.random(n)
        perm[q, :n] = np.lexsort((r, -labels[q, :n].astype(np.float64)))
    return perm


# ---------------------------------------------------------------------------------------------------------------------------- pair losses
def _pair_core(x, t, w, Ew, sigma, c):
    """Per pair [n, n]: loss term, its bound, gradient term dL/ds_first and its bound (module docstring)."""
    ax = np.abs(x)
    p = _sig(x)
    one = x >= X_ONE
    p = np.where(one, 1.0, p)
    dp = np.where(one, 0.0, _dp(p, ax, c))
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.where(one, 0.0, np.maximum(np.log(p), -100.0))
        lq = np.where(one, -100.0, np.maximum(np.log1p(-p), -100.0))
        br = -(t * lp + (1.0 - t) * lq)
        l = w * br
        Ebr = np.where(t > 0, t * (dp / p + c * U * np.abs(lp)), 0.0) + np.where(t < 1, (1.0 - t) * (dp / (1.0 - p) + c * U * np.abs(lq)), 0.0)
    Ebr = np.where(one, 0.0, Ebr)
    El = Ew * np.abs(br) + w * Ebr + c * U * np.abs(l)
    den = p * (1.0 - p)
    r = np.where(one, 0.0, p - t)
    r = np.where(~one & (den < 1e-12), r * den / 1e-12, r)
    T = sigma * w * r
    ET = np.where(one, 0.0, sigma * (Ew * np.abs(r) + w * dp) + c * U * np.abs(T))
    return l, El, T, ET


def chain_factor(m):
    """sqrt(m) for a sum whose terms are added in order in chains of m (module docstring, 'pair sums')."""
    return math.sqrt(max(1.0, float(m)))


def _reduce_pairs(l, El, T, ET, pairs, c):
    """pairs: boolean [n, n] of the (first, second) pairs.  Returns loss, E_loss, grad [n] (first +T, second -T), E_grad.  The loss
    chains hold ceil(P / 64) of the P pair losses, a gradient element's chain its n - 1 partner terms."""
    l, El, T, ET = (np.where(pairs, a, 0.0) for a in (l, El, T, ET))
    n = pairs.shape[0]
    loss = l.sum()
    E_loss = El.sum() + c * U * chain_factor(-(-int(pairs.sum()) // 64)) * np.abs(l).sum()
    g = T.sum(1) - T.sum(0)
    E_g = ET.sum(1) + ET.sum(0) + c * U * chain_factor(n - 1) * (np.abs(T).sum(1) + np.abs(T).sum(0))
    return loss, E_loss, g, E_g


def ranknet_query(s, y, sigma, c):
    s, y = _f64(s), _f64(y)
    n = s.size
    x = sigma * (s[:, None] - s[None, :])
    t = 0.5 * (1.0 + np.clip(y[:, None] - y[None, :], -1.0, 1.0))
    pairs = np.triu(np.ones((n, n), dtype=bool), 1)
    l, El, T, ET = _pair_core(x, t, np.ones_like(x), np.zeros_like(x), sigma, c)
    return _reduce_pairs(l, El, T, ET, pairs, c)


def lambdarank_query(s, y, sigma, c):
    """Pairs in predicted order (score descending, index ascending), D by predicted rank, G = gain / IDCG with the IDCG over the labels in
    input order (the reference takes them as the ideal ranking).  NaN everywhere when IDCG = 0 and there is a pair."""
    s, y = _f64(s), _f64(y)
    n = s.size
    order = np.lexsort((np.arange(n), -s))
    ss, ys = s[order], y[order]
    idcg = (_gain(y) * _disc(n)).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        Gs = _gain(ys) / idcg
    D = _disc(n)
    dG = np.abs(Gs[:, None] - Gs[None, :])
    E_dG = np.where(ys[:, None] == ys[None, :], 0.0, c * U * (Gs[:, None] + Gs[None, :]))
    dD = np.abs(D[:, None] - D[None, :])
    E_dD = c * U * (D[:, None] + D[None, :])
    w = dG * dD
    Ew = E_dG * dD + dG * E_dD + c * U * w
    x = sigma * (ss[:, None] - ss[None, :])
    t = (Gs[:, None] > Gs[None, :]).astype(np.float64)
    pairs = np.triu(np.ones((n, n), dtype=bool), 1)
    l, El, T, ET = _pair_core(x, t, w, Ew, sigma, c)
    loss, E_loss, gs, E_gs = _reduce_pairs(l, El, T, ET, pairs, c)
    if n >= 2 and not idcg > 0:
        loss, gs = float("nan"), np.full(n, np.nan)
    g, E_g = np.empty(n), np.empty(n)
    g[order], E_g[order] = gs, E_gs
    return loss, E_loss, g, E_g


def _batched(fn, preds, labels, lens, queries, *args):
    """Run a per-query reference over `queries` (None: all) of a padded batch.  Returns dict(q, loss_q, E_loss_q, grad, E_grad) with
    grad [len(q), L] (padded slots 0, E 0)."""
    preds, labels = np.asarray(preds), np.asarray(labels)
    B, L = preds.shape
    qs = np.arange(B) if queries is None else np.asarray(queries)
    lq, Elq = np.zeros(len(qs)), np.zeros(len(qs))
    gr, Egr = np.zeros((len(qs), L)), np.zeros((len(qs), L))
    for k, q in enumerate(qs):
        n = _qlen(lens, q, L)
        lq[k], Elq[k], gr[k, :n], Egr[k, :n] = fn(preds[q, :n], labels[q, :n], *args)
    return dict(q=qs, loss_q=lq, E_loss_q=Elq, grad=gr, E_grad=Egr)


def ranknet(preds, labels, lens=None, sigma=1.0, c=C_PAIR, queries=None):
    return _batched(ranknet_query, preds, labels, lens, queries, sigma, c)


def lambdarank(preds, labels, lens=None, sigma=1.0, c=C_PAIR, queries=None):
    return _batched(lambdarank_query, preds, labels, lens, queries, sigma, c)


def batch_total(ref, c, scale=1.0):
    """ptr_sum_f32 over loss_q: (total, E) — the per-query bounds plus c u sum |loss_q| (all queries of ref)."""
    lq = ref["loss_q"]
    return scale * lq.sum(), abs(scale) * (ref["E_loss_q"].sum() + c * U * np.abs(lq).sum())


# ---------------------------------------------------------------------------------------------------------------------------- ApproxNDCG
def _approx_query(s, y, alpha, presort, c):
    """Unscaled per-query ApproxNDCG: dcg, E_dcg, idcg, grad (scale 1), E_grad."""
    s, y = _f64(s), _f64(y)
    n = s.size
    g = _gain(y)
    ideal = y if presort else -np.sort(-y)
    idcg = (_gain(ideal) * _disc(n)).sum()
    delta = s[None, :] - s[:, None]                             # [i, j] = s_j - s_i
    x = alpha * delta
    ax = np.abs(x)
    yv = _sig(x)
    off = ~np.eye(n, dtype=bool)
    dy = np.where(off, _dp(yv, ax, c), 0.0)
    yo = np.where(off, yv, 0.0)
    pi = 1.0 + yo.sum(1)
    E_pi = dy.sum(1) + c * U * pi
    lg = np.log2(pi + 1.0)
    E_lg = E_pi / ((pi + 1.0) * LN2) + c * U * lg
    dcg = (g / lg).sum()
    E_dcg = ((g / lg) * (E_lg / lg + c * U)).sum() + c * U * dcg
    ci = g / (LN2 * (1.0 + pi) * lg * lg)
    E_ci = ci * (c * U + E_pi / (1.0 + pi) + 2.0 * E_lg / lg)
    d = np.where(off, alpha * yv * (1.0 - yv), 0.0)
    E_d = np.where(off, c * U * alpha * (yv * (1.0 - yv) * (2.0 + ax) + 1.0), 0.0)
    T = ci[:, None] * d                                          # [i, j]: +T to j, -T to i
    ET = E_ci[:, None] * d + ci[:, None] * E_d + c * U * np.abs(T)
    grad = T.sum(0) - T.sum(1)
    E_grad = ET.sum(0) + ET.sum(1) + c * U * (np.abs(T).sum(0) + np.abs(T).sum(1))
    return dcg, E_dcg, idcg, grad, E_grad


def approx_inv_idcg(labels, lens, presort, c=C_APPROX):
    """1 / IDCG per query and S = their sum, with bounds (no pairs: cheap for a whole bench batch).  Returns (inv, E_inv, S, E_S)."""
    labels = np.asarray(labels)
    B, L = labels.shape
    inv = np.empty(B)
    for q in range(B):
        n = _qlen(lens, q, L)
        y = _f64(labels[q, :n])
        idcg = (_gain(y if presort else -np.sort(-y)) * _disc(n)).sum()
        with np.errstate(divide="ignore"):
            inv[q] = 1.0 / idcg if n > 0 else np.inf
    E_inv = c * U * inv
    return inv, E_inv, inv.sum(), E_inv.sum() + c * U * np.abs(inv).sum()


def approxndcg(preds, labels, lens=None, alpha=10.0, presort=True, couple_batch=True, override=0.0, c=C_APPROX, queries=None):
    """Float64 ApproxNDCG with bounds: dict(q, dcg_q, E_dcg_q, inv_idcg_q, E_inv_idcg_q, grad, E_grad [len(q), L], scale (the factor
    applied to the gradients), E_scale, S, E_S, loss, E_loss).  S, the scale and the loss need every query: they are None when `queries`
    is a sample.  A query without a relevant document has inv_idcg = inf; its (per-query) dcg * inv_idcg and gradients are NaN."""
    preds, labels = np.asarray(preds), np.asarray(labels)
    B, L = preds.shape
    qs = np.arange(B) if queries is None else np.asarray(queries)
    full = queries is None
    dcg, Edcg, inv, Einv = (np.zeros(len(qs)) for _ in range(4))
    gu, Egu = np.zeros((len(qs), L)), np.zeros((len(qs), L))
    for k, q in enumerate(qs):
        n = _qlen(lens, q, L)
        dcg[k], Edcg[k], _, gu[k, :n], Egu[k, :n] = _approx_query(preds[q, :n], labels[q, :n], alpha, presort, c)
    inv, Einv, _, _ = approx_inv_idcg(labels[qs], None if lens is None else np.asarray(lens)[qs], presort, c)
    res = dict(q=qs, dcg_q=dcg, E_dcg_q=Edcg, inv_idcg_q=inv, E_inv_idcg_q=Einv, S=None, E_S=None, scale=None, E_scale=None, loss=None,
               E_loss=None)
    S = E_S = None
    if full:
        _, _, S, E_S = approx_inv_idcg(labels, lens, presort, c)
        res.update(S=S, E_S=E_S)
    with np.errstate(invalid="ignore"):
        if couple_batch:
            if override > 0:
                f, E_f = float(np.float32(override)), 0.0
            else:
                f, E_f = S, E_S
            if f is not None:
                res["grad"] = gu * f
                res["E_grad"] = Egu * f + np.abs(gu) * E_f + c * U * np.abs(gu * f)
                D_ = dcg.sum()
                E_D = Edcg.sum() + c * U * np.abs(dcg).sum()
                res.update(scale=f, E_scale=E_f, loss=-D_ * f, E_loss=E_D * f + abs(D_) * E_f + c * U * abs(D_ * f))
        else:
            res["grad"] = gu * inv[:, None]
            res["E_grad"] = Egu * inv[:, None] + np.abs(gu) * Einv[:, None] + c * U * np.abs(res["grad"])
            if full:
                N = dcg * inv
                E_N = Edcg * inv + dcg * Einv + c * U * np.abs(N)
                res.update(scale=1.0, E_scale=0.0, loss=-N.sum(), E_loss=E_N.sum() + c * U * np.abs(N).sum())
    if "grad" in res:
        for k in range(len(qs)):                                  # padded slots are exactly 0, NaN or not
            n = _qlen(lens, qs[k], L)
            res["grad"][k, n:] = 0.0
            res["E_grad"][k, n:] = 0.0
    return res


# ---------------------------------------------------------------------------------------------------------------------------- listwise
def _log_softmax(v, c, E_in=None):
    """log-softmax of v with bounds (the max shift, exp per element, the normaliser, log).  E_in: absolute errors of v's elements."""
    m = v.max()
    dv = v - m
    e = np.exp(dv)
    Z = e.sum()
    Ee = e * c * U * (1.0 + np.abs(dv))
    E_Z = Ee.sum() + c * U * Z
    lz = np.log(Z)
    lsm = dv - lz
    sm = e / Z
    E_lsm = c * U * (np.abs(dv) + abs(lz) + 1.0) + E_Z / Z
    if E_in is not None:
        E_lsm = E_lsm + E_in + (sm * E_in).sum()
    return lsm, E_lsm, sm


def listnet_query(s, y, c):
    s, y = _f64(s), _f64(y)
    if s.size == 0:
        return 0.0, 0.0, np.zeros(0), np.zeros(0)
    lsm, E_lsm, ps = _log_softmax(s, c)
    ly, E_ly, py = _log_softmax(y, c)
    E_py = py * (E_ly + c * U)
    E_ps = ps * (E_lsm + c * U)
    terms = py * lsm
    loss = -terms.sum()
    E_loss = (np.abs(lsm) * E_py + py * E_lsm).sum() + c * U * np.abs(terms).sum()
    g = ps - py
    return loss, E_loss, g, E_ps + E_py + c * U * np.abs(g)


def listnet(preds, labels, lens=None, c=C_LIST, queries=None):
    return _batched(listnet_query, preds, labels, lens, queries, c)


def listmle_query(s, pi, c):
    s = _f64(s)
    n = s.size
    if n == 0:
        return 0.0, 0.0, np.zeros(0), np.zeros(0)
    pi = np.asarray(pi, dtype=np.int64)[:n]
    u_ = s[pi]
    m = u_.max()
    du = u_ - m
    e = np.exp(du)
    Ee = e * c * U * (1.0 + np.abs(du))
    T = np.cumsum(e[::-1])[::-1]
    k = np.arange(n, dtype=np.float64)
    E_T = np.cumsum(Ee[::-1])[::-1] + c * U * np.sqrt(np.maximum(1.0, n - k)) * T         # cumulative sums: in-order chains (pair sums)
    lt = np.log(T)
    l = lt - du
    E_l = E_T / T + c * U * (np.abs(lt) + np.abs(lt + m) + np.abs(l))       # (log T + m) - u, as the reference: relative to |m|
    loss = l.sum()
    E_loss = E_l.sum() + c * U * np.abs(l).sum()
    R = np.cumsum(1.0 / T)
    E_R = np.cumsum((1.0 / T) * (E_T / T + c * U)) + c * U * np.sqrt(k + 1.0) * R
    gp = e * R - 1.0
    E_gp = Ee * R + e * E_R + c * U * (e * R + np.abs(gp))
    g, E_g = np.empty(n), np.empty(n)
    g[pi], E_g[pi] = gp, E_gp
    return loss, E_loss, g, E_g


def listmle(preds, perm, lens=None, c=C_LIST, queries=None):
    return _batched(listmle_query, preds, np.asarray(perm), lens, queries, c)


def rankmse(preds, labels, lens=None, c=C_LIST, queries=None):
    """loss_q = per-query sum of squared errors, grad = 2 (s - y) / B (B: the batch's query count)."""
    B = np.asarray(preds).shape[0]

    def one(s, y, c_):
        d = _f64(s) - _f64(y)
        return (d * d).sum(), c_ * U * (d * d).sum(), 2.0 * d / B, c_ * U * np.abs(2.0 * d / B)
    return _batched(one, preds, labels, lens, queries, c)


def rankcosine_query(s, y, c):
    s, y = _f64(s), _f64(y)
    sy, ss, yy = (s * y).sum(), (s * s).sum(), (y * y).sum()
    E_sy, E_ss, E_yy = c * U * np.abs(s * y).sum(), c * U * ss, c * U * yy
    ns, ny = math.sqrt(ss), math.sqrt(yy)
    ds, dy = max(ns, COS_EPS), max(ny, COS_EPS)
    E_ns = ns * c * U + (E_ss / (2 * ns) if ns > 0 else 0.0)
    E_ny = ny * c * U + (E_yy / (2 * ny) if ny > 0 else 0.0)
    den = ds * dy
    E_den = den * ((E_ns / ns if ns > COS_EPS else 0.0) + (E_ny / ny if ny > COS_EPS else 0.0) + c * U)
    cs = sy / den
    E_c = E_sy / den + abs(cs) * E_den / den + c * U * abs(cs)
    loss = (1.0 - cs) / 0.5
    E_loss = 2.0 * E_c + c * U * 2.0 * (1.0 + abs(cs))
    a = y / den
    E_a = np.abs(a) * (E_den / den + c * U)
    if ns > COS_EPS:
        b = cs * s / ss
        E_b = np.abs(b) * c * U + E_c * np.abs(s) / ss + np.abs(cs * s) * E_ss / ss ** 2
    else:
        b, E_b = np.zeros_like(s), np.zeros_like(s)
    g = -2.0 * (a - b)
    return loss, E_loss, g, 2.0 * (E_a + E_b + c * U * (np.abs(a) + np.abs(b)))


def rankcosine(preds, labels, lens=None, c=C_LIST, queries=None):
    return _batched(rankcosine_query, preds, labels, lens, queries, c)


# ---------------------------------------------------------------------------------------------------------------------------- gates
def gate_nan(got, ref, E, what, c=None):
    """f64_bounds.gate where ref is finite; where it is not (NaN, +-inf: no relevant document, a zero-length query's 1/IDCG) got must be
    the very same value, and NaN / inf nowhere else."""
    __tracebackhide__ = True
    got, ref = d64(np.asarray(got, dtype=np.float64)), d64(np.asarray(ref, dtype=np.float64))
    E = d64(np.broadcast_to(np.asarray(E, dtype=np.float64), tuple(ref.shape)).copy())
    fin = torch.isfinite(ref)
    same = (torch.isnan(got) & torch.isnan(ref)) | (got == ref)
    bad = ~fin & ~same
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: the float64 reference is {float(ref.reshape(-1)[i])!r} at flat index {i}, got "
                             f"{float(got.reshape(-1)[i])!r}; {int(bad.sum())} elements")
    return gate(got[fin], ref[fin], E[fin], what, c) if bool(fin.any()) else 0.0


def gate_losses(got_lq, got_grad, ref, what, c, got_total=None, total=None):
    """Gate a kernel's loss_q [B] / grad [B, L] (rows ref['q'] are compared) and, optionally, its batch total.  Returns the worst err/E."""
    q = ref["q"]
    w = gate_nan(np.asarray(got_lq)[q], ref["loss_q"], ref["E_loss_q"], f"{what} loss_q", c)
    w = max(w, gate_nan(np.asarray(got_grad)[q], ref["grad"], ref["E_grad"], f"{what} grad", c))
    if got_total is not None:
        w = max(w, gate_nan(np.array([got_total]), np.array([total[0]]), np.array([total[1]]), f"{what} loss_out", c))
    return w
