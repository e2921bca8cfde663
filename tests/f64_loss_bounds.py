"""Float64 references and ELEMENT-WISE error bounds for the ranking-loss kernels (csrc/pairwise.hip + ptr_ring.h, csrc/approxndcg.hip,
csrc/listwise.hip, csrc/lambdaloss.hip), and the structured scores / labels that make those bounds bite.  The gate itself is
f64_bounds.gate.

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
`gate_nan` demands NaN exactly where the reference is NaN and nowhere else.  What the reference returns there for LambdaLoss and
SoftRank is recorded in tests/golden/losses_norel.npz: the normalised gains are 0 / 0, so NDCG_Loss1 is NaN, loss and the gradient of
EVERY document of the list, beyond k too; NDCG_Loss2 / Loss2++ are 0 (the label mask selects no entry) — their gradient is NaN in the
reference as well, but only as autograd's 0 * NaN through the unselected entries: the product returns the derivative of the constant,
0, and so does the restatement (the one place it departs from the reference's output).  SoftRank is NaN — except the gradient of a
one-document list, which has no pair and is exactly 0.
A NaN score is the second departure (LambdaLoss): the reference ranks it first, counts its differences as 0 and returns finite values
(tests/golden/losses_nanscore.npz); the product gives the list no ranking, and the restatement follows the product: the loss and the
gradient of every document of the list are NaN.
LambdaLoss's other exact zeros: every document ranked at or beyond k, and under Loss2 / Loss2++ every document whose label equals that
of each of its top-k partners.

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
  LambdaLoss             entry (i, j) of the kk x kk block by predicted rank, x = sigma (s_i - s_j), lp = log2 sigmoid(x) = -log1p(e^-x) /
                         ln2, z = w lp, loss term -max(z, log2 eps), T = -w sigma (1 - p) / ln2.  inv[r] = log2(r + 2) (the discount
                         inverted twice) carries c u relative, so delta_d = |inv[d-1] - inv[d]| and rho_ij = |inv[i] - inv[j]| carry
                         c u (inv_a + inv_b) ABSOLUTE — 1e-4 of delta at a rank distance of 100; G and |G_i - G_j| as above.  Loss2 w =
                         delta |dG|, Loss2++ w = (rho + mu delta) |dG| on the entries with label_i > label_j; Loss1 every entry, the
                         diagonal included (x = 0: no gradient), with the column's weight w_j = G_j inv[j].  log2 p is RELATIVE:
                         E_lp = c u (|lp| + |x| (1 - p) / ln2) — a kernel that takes the log of the rounded p loses e^-x / ln2 on every
                         pair whose p rounds to 1, all one way, and fails; E_z = E_w |lp| + w E_lp + c u |z| (+ c u / ln2 per pair with
                         `log_floor`: the top-k kernel's one hardware log of 1 + e, at most 55 pairs, and the fp32 p ** w of the oracle
                         and the reference; nowhere else); E_T = sigma / ln2 (E_w (1 - p) + w dp) + c u |T|, 1 - p by subtraction.  The
                         fp32 branches: p < eps gives lp = log2 eps and T = 0 exactly, z < log2 eps gives the term -log2 eps and T = 0
                         exactly; `lambdaloss_inputs` screens both.  Chains: ceil(P / 64) for the loss, kk - 1 for a gradient element
  SoftRank               x_ij = (s_i - s_j) inv_den (inv_den the entry point's fp32 value); the smaller indicator 0.5 erfc |x| carries c u
                         relative + e^{-x^2} / sqrt(pi) c u |x| (its argument), the complement c u absolute; an fp32 result below 2^-126
                         is flushed: that much absolute on every indicator and flow term.  E[rank], lg, dcg, c_i as ApproxNDCG (top_k cuts
                         by ideal position); flow phi_ij (c_i - c_j), phi = inv_den e^{-x^2} / sqrt(pi) with c u (2 + x^2) relative (the
                         fast exponential); loss_q = -dcg / idcg and grad / idcg per query, labels taken as presorted
  STListNet              z = (s + g) / T, g = -log(-log(u + 1e-20) + 1e-20): the inner log c u relative, so g c u (1 + |g|) absolute; the
                         sum rounds relative to |s + g| (the dominant term under a common offset); E_z reaches lsm_i as E_z_i +
                         sum_j softmax_j E_z_j (ListNet's bounds otherwise), the gradient carries the extra 1 / T
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
                  # SoftRank (approxndcg_kernel<SOFT>): worst 2.40 (grad, 5 x 2100), loss_q 0.61: 0.60 of the constant
C_LLOSS = 3.0     # LambdaLoss (lambdaloss.hip), both kernels: worst 1.75 (loss_q of the top-k kernel with its log floor, the persistent
                  # walk at L = 8), its grad 1.22, that batch's loss_out (24 593 queries) 0.09; the generic kernel 1.32 (grad, Loss1 at k = L = 64), loss_q 0.49; 1.7x headroom.  The C
                  # oracle and the reference's fp32 fixtures (fp32 p ** w, with the floor): 1.38 (grad, 16 documents)
C_LIST = 4.0      # ListNet, ListMLE, RankMSE, RankCosine (listwise.hip): worst 2.20 (RankMSE grad); ListNet 0.89, ListMLE 0.81,
                  # RankCosine 0.54; 1.8x headroom
                  # STListNet (listnet_kernel with the Gumbel prologue): worst 0.35 (grad), loss_q 0.20

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


# ---------------------------------------------------------------------------------------------------------------------------- LambdaLoss
LL_EPS = float(np.float32(1e-8))                     # the clamp, as the fp32 comparison sees it
LL_LOG2_EPS = float(np.float32(-26.575424759098897))  # log2(1e-8) as the kernels hold it
X_EPS = math.log(1e8)                                # 18.42: sigmoid(-x) < 1e-8 from here on
LL_SCREEN_X = 1.0                                    # sigma |ds| within +-1 of X_EPS is screened
LL_SCREEN_Z = 1e-3                                   # |w lp - log2 eps| < 1e-3 |log2 eps| is screened


def lambdaloss_query(s, y, k, sigma, mu, loss_type, presort, c, log_floor=False, detail=False):
    """lambdaloss.py:83-132 for one query (loss_type 0 NDCG_Loss1, 1 NDCG_Loss2, 2 NDCG_Loss2++), bug-compatible as csrc/lambdaloss.hip
    lists it.  Entry (i, j) of the kk x kk block, by predicted rank, stands for the probability sigmoid(sigma (s_i - s_j)) ** w_ij:
    Loss2 / Loss2++ keep the entries with label_i > label_j, Loss1 all of them (diagonal included) with the column's weight.
    Returns loss, E_loss, grad, E_grad; with detail, also the entries within the screened distance of a clamp (by document) and the
    number of entries on each clamp's far side."""
    s, y = _f64(s), _f64(y)
    n = s.size
    if n == 0:
        out = (0.0, 0.0, np.zeros(0), np.zeros(0))
        return out + (np.zeros(0, bool), 0, 0) if detail else out
    if np.isnan(s).any() or np.isnan(y).any():
        # NOT the reference (tests/golden/losses_nanscore.npz: it ranks a NaN score first, counts its differences as 0 and stays finite):
        # the product gives such a list no ranking, a NaN loss and a NaN gradient on every document
        out = (float("nan"), 0.0, np.full(n, np.nan), np.zeros(n))
        return out + (np.zeros(n, bool), 0, 0) if detail else out
    idx = np.arange(n)
    il = idx if presort else np.lexsort((idx, -y))               # ideal order: label descending, index ascending
    tp, ideal = s[il], y[il]
    ip = np.lexsort((idx, -tp))                                  # predicted order: score descending, ideal position ascending
    kk = min(max(int(k), 0), n)
    ss, ys = tp[ip][:kk], ideal[ip][:kk]
    idcg = (_gain(ideal) * _disc(n)).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        G = _gain(ys) / idcg
    E_G = c * U * G
    inv = np.log2(np.arange(max(kk, 1), dtype=np.float64) + 2.0)  # the discount inverted twice
    r = np.arange(kk)
    x = sigma * (ss[:, None] - ss[None, :])
    ax = np.abs(x)
    if loss_type == 0:
        act = np.ones((kk, kk), dtype=bool)
        w = np.broadcast_to((G * inv[:kk])[None, :], (kk, kk))
        Ew = np.broadcast_to((3.0 * c * U * G * inv[:kk])[None, :], (kk, kk))
    else:
        act = ys[:, None] > ys[None, :]
        d = np.abs(r[:, None] - r[None, :])
        dm = np.maximum(d - 1, 0)
        delta = np.where(d > 0, np.abs(inv[dm] - inv[d]), 0.0)
        E_delta = np.where(d > 0, c * U * (inv[dm] + inv[d]), 0.0)
        absG = np.abs(G[:, None] - G[None, :])
        E_absG = np.where(act | act.T, c * U * (G[:, None] + G[None, :]), 0.0)
        pos, E_pos = delta, E_delta
        if loss_type == 2:
            rho = np.abs(inv[:kk, None] - inv[None, :kk])
            pos = rho + mu * delta
            E_pos = c * U * (inv[:kk, None] + inv[None, :kk]) + mu * E_delta + c * U * pos
        w = pos * absG
        Ew = E_pos * absG + pos * E_absG + c * U * w
    with np.errstate(invalid="ignore", over="ignore"):
        p = _sig(x)
        small = p < LL_EPS                                       # clamp(min=eps) before the power: log2 eps, gradient exactly 0
        lp = np.where(small, LL_LOG2_EPS, -(np.maximum(-x, 0.0) + np.log1p(np.exp(-ax))) / LN2)
        E_lp = np.where(small, 0.0, c * U * (np.abs(lp) + ax * (1.0 - p) / LN2))     # RELATIVE: lp -> 0 as p -> 1 keeps its accuracy
        z = w * lp
        E_z = Ew * np.abs(lp) + w * E_lp + c * U * np.abs(z) + (c * U / LN2 if log_floor else 0.0)
        low = z < LL_LOG2_EPS                                    # clamp(min=eps) after the power: -log2 eps, gradient exactly 0
        l = np.where(low, -LL_LOG2_EPS, -z)
        El = np.where(low, 0.0, E_z)
        dead = small | low | np.eye(kk, dtype=bool)
        T = np.where(dead, 0.0, -(w * sigma * (1.0 - p)) / LN2)   # d / d s_i of entry (i, j); s_j gets -T
        ET = np.where(dead, 0.0, sigma / LN2 * (Ew * (1.0 - p) + w * _dp(p, ax, c)) + c * U * np.abs(T))
    l, El, T, ET = (np.where(act, a, 0.0) for a in (l, El, T, ET))
    P = int(act.sum())
    loss = l.sum()
    E_loss = El.sum() + c * U * chain_factor(-(-P // 64)) * np.abs(l).sum()
    gs, E_gs = np.zeros(n), np.zeros(n)
    gs[:kk] = T.sum(1) - T.sum(0)
    E_gs[:kk] = ET.sum(1) + ET.sum(0) + c * U * chain_factor(kk - 1) * (np.abs(T).sum(1) + np.abs(T).sum(0))
    if not idcg > 0:
        # gains 0 / 0: every weight is NaN (tests/golden/losses_norel.npz).  Loss1: the reference's clamp(min) keeps NaN, loss and the
        # gradient of EVERY document.  Loss2 / Loss2++ select no entry: loss 0 as the reference, gradient 0 (the reference's NaN
        # gradient there is autograd's 0 * NaN through the unselected entries; the product keeps the constant's derivative)
        loss, E_loss = (float("nan") if loss_type == 0 and kk > 0 else 0.0), 0.0
        gs, E_gs = (np.full(n, np.nan) if loss_type == 0 else np.zeros(n)), np.zeros(n)
    g, E_g = np.empty(n), np.empty(n)
    g[il[ip]], E_g[il[ip]] = gs, E_gs
    if not detail:
        return loss, E_loss, g, E_g
    with np.errstate(invalid="ignore"):
        nearx = np.abs(ax - X_EPS) <= LL_SCREEN_X
        nearz = act & ~small & (np.abs(z - LL_LOG2_EPS) < LL_SCREEN_Z * abs(LL_LOG2_EPS))
    near = np.zeros(n, dtype=bool)
    near[il[ip][:kk]] = (nearx | nearz).any(1) | (nearx | nearz).any(0)
    return loss, E_loss, g, E_g, near, int((act & small).sum()), int((act & low & ~small).sum())


def lambdaloss(preds, labels, lens=None, k=5, sigma=1.0, mu=5.0, loss_type=1, presort=True, c=None, queries=None, log_floor=False):
    """log_floor: lp carries c u / ln2 absolute on top of its relative bound — for the top-k kernel (one hardware log of 1 + e per pair,
    at most 55 pairs) and for the fp32 oracle / reference (which round p ** w near 1); nowhere else."""
    return _batched(lambdaloss_query, preds, labels, lens, queries, k, sigma, mu, loss_type, presort, C_LLOSS if c is None else c, log_floor)


def lambdaloss_inputs(B, L, k, sigma=1.0, mu=5.0, loss_type=1, presort=True, need_clamps=False, scale=1.0, **kw):
    """pair_inputs for LambdaLoss (label-sorted lists under presort), screened against both clamps: a document of a pair with sigma |ds|
    within LL_SCREEN_X of ln 1e8, or of an entry with |w lp - log2 eps| < LL_SCREEN_Z |log2 eps|, moves into the bulk of its query.  At
    most MAX_SCREENED of the documents may move.  need_clamps (the k = L cases): entries on the far side of p < eps must remain, and for
    Loss1 / Loss2++ (Loss2's weights are below 1: unreachable) of w lp < log2 eps too.  scale multiplies the scores (the libm-route
    case).  Returns (preds, labels, lens, screened fraction, entries with p < eps, entries with w lp < log2 eps)."""
    s, y, n, frac = pair_inputs(B, L, sigma=sigma, sort_labels=bool(presort), **kw)
    if scale != 1.0:
        s = (s.astype(np.float64) * scale).astype(np.float32)
    if need_clamps:
        # Two lists with one relevant document (G = 1) that put entries beyond the second clamp alone (p >= eps, w lp < log2 eps), which
        # the generated scores rarely do.  6: the relevant document third, the tail 12 / sigma below it (Loss1: column weight log2 4 = 2,
        # lp = -17.3).  7: the relevant document 12 / sigma below the rest (Loss2++: rho + mu delta > 2 against the best ranks) and one
        # document 21.5 / sigma above it (p < eps)
        assert B >= 8 and L >= 8
        off = float(kw.get("offset", 0.0))
        for q in (6, 7):
            n[q] = max(int(n[q]), 8)
            y[q] = 0.0
            y[q, 0] = 4.0
            j = np.arange(L, dtype=np.float64)
            v = -12.0 - 0.01 * j if q == 6 else 2.0 * ((j * 0.618) % 1.0)
            v[0] = 0.0 if q == 6 else -12.0
            v[1:3] = (2.0, 1.0) if q == 6 else (9.5, 1.25)
            s[q] = (v / sigma * scale + off).astype(np.float32)
    moved, n_small, n_low = 0, 0, 0
    for q in range(B):
        for _ in range(8):
            nq = int(n[q])
            *_, near, a, b = lambdaloss_query(s[q, :nq], y[q, :nq], k, sigma, mu, loss_type, presort, 1.0, detail=True)
            if not near.any():
                n_small, n_low = n_small + a, n_low + b
                break
            i = int(np.nonzero(near)[0][0])
            s[q, i] = np.float32(np.median(np.delete(s[q, :nq].astype(np.float64), i)))
            moved += 1
        else:
            raise AssertionError(f"query {q}: could not screen its pairs")
    frac += moved / max(1, int(n.sum()))
    assert frac <= MAX_SCREENED, f"screened {frac:.4f} of the documents"
    if need_clamps:
        print(f"lambdaloss_inputs: {n_small} entries with p < eps, {n_low} more with w lp < log2 eps")
        assert n_small > 0, "no entry with p < eps left"
        assert loss_type == 1 or n_low > 0, "no entry with w lp < log2 eps left"
    return s, y, n, frac, n_small, n_low


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


# ---------------------------------------------------------------------------------------------------------------------------- SoftRank
SQRT_PI = math.sqrt(math.pi)
F32_TINY = 2.0 ** -126                    # below this an fp32 result is flushed or loses its relative accuracy: an absolute floor


def softrank_inv_den(delta):
    """1 / sqrt(2 (2 delta^2)) as ptr_softrank_fwd_bwd forms it in fp32."""
    d = np.float32(delta)
    var = np.float32(2.0) * (d * d)
    return float(np.float32(1.0) / np.sqrt(np.float32(2.0) * var))


def softrank_query(s, y, inv_den, top_k, c):
    """One query (labels as the ideal order): loss, E_loss, grad, E_grad.  _approx_query's machinery with the Gaussian indicator."""
    s, y = _f64(s), _f64(y)
    n = s.size
    if n == 0:
        return 0.0, 0.0, np.zeros(0), np.zeros(0)
    g = _gain(y)
    idcg = (g * _disc(n)).sum()
    top = n if top_k is None or top_k <= 0 else min(int(top_k), n)
    x = (s[:, None] - s[None, :]) * inv_den                      # [i, j]: j's share of E[rank_i] is 0.5 erfc(x_ij)
    ax = np.abs(x)
    ex = np.exp(-ax * ax)
    sm = 0.5 * torch.special.erfc(torch.from_numpy(ax)).numpy()
    E_sm = c * U * sm + ex / SQRT_PI * c * U * ax + F32_TINY
    off = ~np.eye(n, dtype=bool)
    yv = np.where(off, np.where(x > 0, sm, np.where(x < 0, 1.0 - sm, 0.5)), 0.0)
    dy = np.where(off, np.where(x > 0, E_sm, np.where(x < 0, c * U, c * U * 0.5)), 0.0)
    pi = 1.0 + yv.sum(1)
    E_pi = dy.sum(1) + c * U * pi
    lg = np.log2(pi + 1.0)
    E_lg = E_pi / ((pi + 1.0) * LN2) + c * U * lg
    cut = np.arange(n) < top
    dcg = np.where(cut, g / lg, 0.0).sum()
    E_dcg = np.where(cut, (g / lg) * (E_lg / lg + c * U), 0.0).sum() + c * U * dcg
    ci = np.where(cut, g / (LN2 * (1.0 + pi) * lg * lg), 0.0)
    E_ci = ci * (c * U + E_pi / (1.0 + pi) + 2.0 * E_lg / lg)
    phi = np.where(off, inv_den * ex / SQRT_PI, 0.0)
    # the fast exponential: its argument x^2 log2(e) rounds relative to x^2
    E_phi = np.where(off, c * U * (2.0 + ax * ax) * phi + F32_TINY * max(1.0, inv_den), 0.0)
    T = ci[:, None] * phi                                        # [i, j]: +T to j, -T to i
    ET = E_ci[:, None] * phi + ci[:, None] * E_phi + c * U * np.abs(T) + np.where(off, F32_TINY, 0.0)
    gu = T.sum(0) - T.sum(1)
    E_gu = ET.sum(0) + ET.sum(1) + c * U * (np.abs(T).sum(0) + np.abs(T).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / idcg
        loss = -(dcg * inv)
        E_loss = E_dcg * inv + 2.0 * c * U * abs(loss)
        grad = gu * inv
        E_grad = E_gu * inv + 2.0 * c * U * np.abs(grad)
    if n == 1:                                                   # no pair: the reference's gradient is exactly 0, relevant or not (losses_norel.npz)
        grad, E_grad = np.zeros(1), np.zeros(1)
    return loss, (E_loss if np.isfinite(loss) else 0.0), grad, np.where(np.isfinite(grad), E_grad, 0.0)


def softrank(preds, labels, lens=None, delta=2.0, top_k=None, c=C_APPROX, queries=None):
    """Float64 SoftRank: loss_q = -dcg / idcg per query (no batch coupling), grad scaled by 1 / idcg.  A query with documents but no
    relevant one is NaN (loss, and gradient from two documents on), as the reference; a zero-length query is 0."""
    return _batched(softrank_query, preds, labels, lens, queries, softrank_inv_den(delta), top_k, c)


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


def listnet_query(s, y, c, E_s=None, gscale=1.0):
    """E_s: absolute errors of the scores as the kernel holds them (STListNet); gscale: the factor on the gradient (STListNet's 1 / T)."""
    s, y = _f64(s), _f64(y)
    if s.size == 0:
        return 0.0, 0.0, np.zeros(0), np.zeros(0)
    lsm, E_lsm, ps = _log_softmax(s, c, E_s)
    ly, E_ly, py = _log_softmax(y, c)
    E_py = py * (E_ly + c * U)
    E_ps = ps * (E_lsm + c * U)
    terms = py * lsm
    loss = -terms.sum()
    E_loss = (np.abs(lsm) * E_py + py * E_lsm).sum() + c * U * np.abs(terms).sum()
    g = (ps - py) * gscale
    return loss, E_loss, g, (E_ps + E_py) * gscale + c * U * np.abs(g) * (1.0 if gscale == 1.0 else 2.0)


def listnet(preds, labels, lens=None, c=C_LIST, queries=None):
    return _batched(listnet_query, preds, labels, lens, queries, c)


def gumbel(unif):
    """(g, E_g / (c u)) of g = -log(-log(u + 1e-20) + 1e-20) as fp32 forms it: u + 1e-20 is u itself unless u = 0; the inner log carries
    c u relative, which the outer log turns into c u absolute, plus its own c u |g|."""
    uu = (np.asarray(unif, np.float32) + np.float32(1e-20)).astype(np.float64)
    inner = -np.log(uu) + 1e-20
    g = -np.log(inner)
    return g, 1.0 + np.abs(g)


def stlistnet_query(s, y, unif, inv_t, c):
    s = _f64(s)
    g, Eg = gumbel(unif)
    z = (s + g) * inv_t
    E_z = (c * U * Eg + c * U * np.abs(s + g)) * inv_t + c * U * np.abs(z)      # the sum rounds relative to |s + g|: the offset's share
    return listnet_query(z, y, c, E_z, inv_t)


def stlistnet(preds, labels, unif, lens=None, temperature=1.0, c=C_LIST, queries=None):
    """ListNet on (preds + gumbel(unif)) / T; the kernel multiplies by the fp32 1 / T, and so does the gradient."""
    preds, labels, unif = np.asarray(preds), np.asarray(labels), np.asarray(unif)
    inv_t = float(np.float32(1.0) / np.float32(temperature))
    B, L = preds.shape
    qs = np.arange(B) if queries is None else np.asarray(queries)
    lq, Elq = np.zeros(len(qs)), np.zeros(len(qs))
    gr, Egr = np.zeros((len(qs), L)), np.zeros((len(qs), L))
    for k, q in enumerate(qs):
        n = _qlen(lens, q, L)
        lq[k], Elq[k], gr[k, :n], Egr[k, :n] = stlistnet_query(preds[q, :n], labels[q, :n], unif[q, :n], inv_t, c)
    return dict(q=qs, loss_q=lq, E_loss_q=Elq, grad=gr, E_grad=Egr)


def stlistnet_inputs(B, L, seed=0, offset=0.0):
    """listwise_inputs plus the uniform draws: [0, 1) fp32 with the three edges planted in query 1 (0: the 1e-20 guard; the largest float
    below 1: the inner log's smallest value; 2^-24: torch.rand's smallest non-zero draw).  Queries 3 and 4 have lengths 1 and 0."""
    p, y, n = listwise_inputs(B, L, seed=seed, offset=offset)
    g = np.random.default_rng(seed + 101)
    u = g.random((B, L), dtype=np.float32)
    n[1] = max(int(n[1]), min(L, 3))
    u[1, :3] = [0.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 2.0 ** -24]
    assert float(u.max()) < 1.0
    return p, y, u, n


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
