"""ELEMENT-WISE error bounds for the diversification kernels (csrc/diversity.hip: ptr_alphadcg_fwd_bwd, ptr_div_metrics_at_ks) beside the
float64 restatement tests/diversity_ref.py, and the case lists both tests/test_diversity_bounds_cpu.py and
tests/test_diversity_bounds_gpu.py run.  Conventions of tests/f64_loss_bounds.py: u = 2^-24, one family constant C_DIV, the gate is
f64_bounds.gate (|got - ref| <= E element by element, E = 0 demands equality), every gated test prints `MEASURED ...: needs c >= k`.

Why: tests/test_diversity_gpu.py compares under golden_util.assert_close, 1e-5 relative with a floor of 1e-6 of the tensor's largest value.
A DALETOR gradient element is a sum of +- pair terms d_ij (G_ji - G_ij); a document whose element is 1e-4 of the largest can be a few %
wrong under that floor, and so can a kernel that lost the relative accuracy of ind (1 - ind) in the saturated tail.

Reference and bounds are computed from the very fp32 inputs the kernel saw: alpha and rt as fp32 values, log2 c and ln c (c = 1 - alpha)
as the entry points form them (diversity_ref.c_logs).  No term is relative to a tensor's maximum, none to |s|.

Loss (alphadcg_kernel; i the thread's document, j its partner, t a subtopic, n documents, TINY = 2^-126):
  x_ij = rt (s_j - s_i)       the difference is one rounding relative to |ds| and reaches the exponential's argument as c u |x|
  e = exp(-|x|), r = 1 / (1 + e), sm = e r; both indicators are products, neither is formed by subtraction from 1:
      E_ind = c u ind (1 + (1 - ind) (1 + |x|)) + TINY          (relative to ind itself)
  d = ind_ij ind_ji           E_d = c u d (2 + |x|) + TINY      (no absolute "+ 1" as ApproxNDCG's LDS form has: that term would let
                              a 1 - y by subtraction through)
  pi_i = 1 + sum_j ind        E_pi = sum_j E_ind + c u sqrt(n - 1) pi                        (in-order chain of n - 1 terms in one thread)
  cover_ti = sum_j ind R_tj   E_cover = sum_j E_ind R_tj + c u sqrt(n - 1) sum_j ind R_tj    (likewise)
  lg = log2(1 + pi)           E_lg = E_pi / ((1 + pi) ln2) + c u lg
  p = c^cover                 E_p = p (|ln c| E_cover + c u (1 + |cover ln c|)) + TINY
  g = R p / lg (kept)         E_g = R (E_p / lg + p E_lg / lg^2) + c u g
  loss_q = - sum g            E_loss = sum E_g + c u sqrt(nt + ceil(n / 64)) sum g     (a thread adds the nt gains of a document, then its
                              at most ceil(n / 64) documents, in order; a short tree joins the threads)
  A_i = sum_t g / (lg ln2 (1 + pi))   E_A = (sum_t E_g + c u sqrt(nt) sum_t g) / (lg ln2 (1 + pi)) + A (E_lg / lg + E_pi / (1 + pi)) + c u A
  Bc_ti = -g ln c             E_Bc = E_g |ln c| + c u |Bc|
  D_ij = (A_j - A_i) + sum_t Bc_tj R_ti - sum_t Bc_ti R_tj
                              E_D = E_A_j + E_A_i + sum_t (E_Bc_tj R_ti + E_Bc_ti R_tj) + c u (|A_j| + |A_i| + sum_t (|Bc_tj| R_ti + |Bc_ti| R_tj))
                              (c u times the sum of the ABSOLUTE terms: the cancellation the old rule is blind to)
  grad_i = rt sum_j d D       E_grad = rt sum_j (E_d |D| + d E_D) + c u sqrt(n - 1) rt sum_j |d D| + rt TINY #{j: d D != 0}
                              (the last term is the floor of the OUTPUT's own format: a product d D below 2^-126 flushes in any fp32
                              evaluation, and a gradient element of 1e-40 cannot be demanded to seven digits.  It is 1e-35 at most.)
  loss_out                    f64_loss_bounds.batch_total
Flush to zero: TINY absolute on e (through both indicators), d, c^cover and the products that form a gradient element, nowhere else.  A non-finite difference has |x| taken as 0
in the bounds (its indicators are exactly 0, 1 or 0.5).
Exact (E = 0): the gradient of every padded slot; loss and gradient of a query with 0 documents or 0 subtopics; the gradient of a
1-document query; loss and gradient of a query whose kept relevance is all zero (every term above carries a factor of the kept R).

Metrics (div_metrics_kernel; one lane per subtopic, rank r = 0 .. k - 1, the system and the ideal ranking alike):
  1 / log2(r + 2), 2^x - 1    c u relative each
  cov = sum of earlier x      exact for integer grades, else c u sqrt(r) cov;    p = c^cov as above
  term = p x / log2(r + 2)    E_term = term (E_p / p + 2 c u)                      (the discount, and the product and quotient)
  dcg lane = sum_r term       E = sum E_term + c u sqrt(k) sum |term|              (in-order chain)
  sat = (2^x - 1) 2^-ml       c u relative;     casc_r = prod_{r' < r} (1 - sat)   c u per factor, relative, plus E_sat / (1 - sat)
  eterm = sat casc / (r + 1)  E = eterm (c u + rel_casc + 2 c u);   err lane = sum_r eterm as the dcg lane
  cross-lane sum              sum of the lanes' bounds + c u sum |lane values|;   ERR-IA: one more c u for the division by ntopics
  alpha-nDCG = Ds / Di, nERR-IA = Es / Ei     first order: E_num / den + num E_den / den^2 + c u |quotient|
Exact: `valid`; every output of an invalid query; every cut-off < 1 or beyond the list (0).  The ranking is exact: value descending,
NaN first, then original index (ptr_sort_desc's and torch.sort's order; -0.0 ties with +0.0).

C_DIV is MEASURED, not chosen, by the rule of metrics_ref.C_METRIC: min(4, 2 x the larger need of two fp32 evaluations that are not the
kernel, rounded up to a half), 4 being C_APPROX, the sibling family on the same robust_pair arithmetic:
  (a) diversity_ref in fp32 torch on every case of loss_cases() / metric_cases() / nan_metric_cases();
  (b) the reference's own fp32 loss32 / grad32 of tests/golden/diversity.npz, the two steep_* (rt = 100) cases included.
The reference's fp32 gradient does NOT fit the model above, and not for want of a term in |x|: Robust_Sigmoid saves sigma ind (1 - ind)
with 1 - ind formed by SUBTRACTION (utils.py:76).  Where ind rounds to 1 its d is 0 instead of e^-|x|: a document all of whose pairs are
saturated has a gradient of ~1e-13 there and gets exactly 0 — 4.1e5 times its bound (T1_L20; the steep cases 6.8e4 and 3.2e5).  That is
the very fault the gate exists to refuse (tests/test_diversity_bounds_cpu.py plants it), so need (b) is measured with the ONE term such a
subtraction adds, c u absolute on d (`sub_abs`, ApproxNDCG's LDS form) — a term the kernel's gate never gets.  With it every fixture
fits: 0.61 at worst, the steep cases 0.02.  tests/test_diversity_bounds_cpu.py re-measures all three figures.
"""
import math

import numpy as np

import diversity_ref as DR
from f64_bounds import U
from f64_loss_bounds import batch_total, chain_factor, gate_losses, gate_nan  # noqa: F401  (re-exported for the tests)

NEED_FP32_TORCH = 0.84        # (a): worst over the case lists (a gradient element of form_T12_L128_B9); the metrics 0.21
NEED_REFERENCE_FP32 = 0.61    # (b): worst over diversity.npz with the subtraction's term (grad32 of T1_L20); loss32 alone 0.12
MISFIT_REFERENCE_FP32 = 4.1e5  # (b) WITHOUT that term: the reference's fp32 1 - ind by subtraction (module docstring)
C_CAP = 4.0                   # f64_loss_bounds.C_APPROX


def constant_from_needs(*needs):
    return min(C_CAP, math.ceil(2.0 * max(needs) * 2.0) / 2.0)


C_DIV = 2.0                   # = constant_from_needs(NEED_FP32_TORCH, NEED_REFERENCE_FP32)
# The kernel's worst measured need per output on an MI355X (tests/test_diversity_bounds_gpu.py prints them; COVERAGE.md row f-6): the
# gradient 1.21 (steep_T7_L100, rt = 100), i.e. 0.6 of the constant; everything else below 0.3 of it.  The metric walk needs a fifth of what its model allows.
KERNEL_NEEDS = dict(loss_q=0.56, loss_out=0.29, grad=1.21, andcg=0.17, err_ia=0.24, nerr_ia=0.17)

LN2 = math.log(2.0)
TINY = 2.0 ** -126


# ---------------------------------------------------------------------------------------------------------------------------- kernel forms
# (G, TP) of alphadcg_kernel by (T, L) and (G, DPT) of div_metrics_kernel by L, as the case lists want them: tests/test_diversity_bounds_cpu.py
# asks the library (tests/launch_form.py) whether its launchers agree
LOSS_FORMS = {(3, 40): (64, 4), (7, 100): (64, 8), (12, 128): (64, 16), (30, 64): (64, 32), (4, 129): (256, 4), (8, 200): (256, 8),
              (16, 260): (256, 16), (32, 300): (256, 32)}
LOSS_LIMIT_FORMS = {(8, 2272): (256, 8), (3, 4092): (256, 4)}              # on the documented LDS limits, B = 1
METRIC_FORM_L = {(64, 1): (1, 64), (64, 2): (65, 128), (256, 1): (129, 256), (256, 2): (257, 512), (256, 4): (513, 1024),
                 (256, 8): (1025, 2048), (256, 16): (2049, 4096)}            # smallest and largest L of each form


# ---------------------------------------------------------------------------------------------------------------------------- loss
def alphadcg_query(s, R, rt, alpha, top_k, top_k_axis, c, sub_abs=False):
    """One query (s [n], R [nt, n], both as the kernel read them): loss, E_loss, grad [n], E_grad [n].  sub_abs: d carries c u ABSOLUTE on
    top, as a 1 - ind formed by subtraction does (the reference's own fp32, utils.py:76) — never for the kernel."""
    nt, n = R.shape
    k = DR.alphadcg(s, R, rt, alpha, top_k, top_k_axis, kernel_consts=True, detail=True)
    ax, ind, d, pi, cover, lg, p, g, A, Bc, D, Rt, Rk = (k[x] for x in ("ax", "ind", "d", "pi", "cover", "lg", "p", "g", "A", "Bc", "delta", "R", "Rk"))
    rt, lnc = k["rt"], abs(k["ln_c"])
    off = ~np.eye(n, dtype=bool)
    cu, ch = c * U, chain_factor(n - 1)
    E_ind = np.where(off, cu * ind * (1.0 + (1.0 - ind) * (1.0 + ax)) + TINY, 0.0)
    E_d = np.where(off, cu * d * (2.0 + ax) + TINY + (cu if sub_abs else 0.0), 0.0)
    E_pi = E_ind.sum(1) + cu * ch * pi
    E_cov = E_ind @ Rt + cu * ch * (ind @ Rt)
    E_lg = E_pi / ((1.0 + pi) * LN2) + cu * lg
    E_p = p * (lnc * E_cov + cu * (1.0 + np.abs(cover) * lnc)) + TINY
    E_g = Rk * (E_p / lg[:, None] + p * E_lg[:, None] / (lg * lg)[:, None]) + cu * g
    loss, E_loss = k["loss"], E_g.sum() + cu * chain_factor(nt + -(-n // 64)) * g.sum()
    den = lg * LN2 * (1.0 + pi)
    E_A = (E_g.sum(1) + cu * chain_factor(nt) * g.sum(1)) / den + A * (E_lg / lg + E_pi / (1.0 + pi)) + cu * A
    E_Bc = E_g * lnc + cu * np.abs(Bc)
    aA, aBc = np.abs(A), np.abs(Bc)
    E_D = (E_A[None, :] + E_A[:, None] + Rt @ E_Bc.T + E_Bc @ Rt.T
           + cu * (aA[None, :] + aA[:, None] + Rt @ aBc.T + aBc @ Rt.T))
    aT = np.abs(d * D)
    E_grad = rt * (E_d * np.abs(D) + d * E_D).sum(1) + cu * ch * rt * aT.sum(1) + rt * TINY * (aT > 0).sum(1)
    return loss, E_loss, k["grad"], E_grad


def alphadcg(preds, rele, lens=None, ntopics=None, rt=10.0, alpha=0.5, top_k=10, top_k_axis=0, c=None, queries=None, sub_abs=False):
    """Float64 alpha-DCG loss of a padded batch with bounds: dict(q, loss_q, E_loss_q, grad, E_grad) as f64_loss_bounds._batched
    (padded slots and empty queries: 0 with E = 0).  lens / ntopics are clamped as the kernel clamps them."""
    c = C_DIV if c is None else c
    preds, rele = np.asarray(preds), np.asarray(rele)
    B, T, L = rele.shape
    qs = np.arange(B) if queries is None else np.asarray(queries)
    lq, Elq = np.zeros(len(qs)), np.zeros(len(qs))
    gr, Egr = np.zeros((len(qs), L)), np.zeros((len(qs), L))
    for k, q in enumerate(qs):
        n, nt = DR.clamp_len(lens, q, L), DR.clamp_len(ntopics, q, T)
        if n == 0 or nt == 0:
            continue
        lq[k], Elq[k], gr[k, :n], Egr[k, :n] = alphadcg_query(preds[q, :n], rele[q, :nt, :n], rt, alpha, top_k, top_k_axis, c, sub_abs)
    return dict(q=qs, loss_q=lq, E_loss_q=Elq, grad=gr, E_grad=Egr)


# ---------------------------------------------------------------------------------------------------------------------------- metrics
def _lane_bounds(w, log2_c, cu, with_err):
    """Cumulated (over ranks) and lane-summed alpha-DCG and ERR of one walk (diversity_ref._walk as float64 numpy): value and bound per
    rank, each [kmax]; the ERR sums are not yet divided by the number of subtopics."""
    x, cov, p, gt = w["x"], w["cov"], w["p"], w["gt"]
    kmax = x.shape[1]
    r = np.arange(kmax, dtype=np.float64)
    lnc = abs(log2_c) * LN2
    integer = bool(np.all(x == np.round(x)))
    E_cov = np.zeros_like(cov) if integer else cu * np.sqrt(np.maximum(r, 1.0)) * cov
    E_p = p * (lnc * E_cov + cu * (1.0 + cov * lnc)) + TINY
    E_gt = x / w["den"] * E_p + 2.0 * cu * gt
    ch = np.sqrt(r + 1.0)
    lane, E_lane = np.cumsum(gt, 1), np.cumsum(E_gt, 1) + cu * ch * np.cumsum(np.abs(gt), 1)
    out = [lane.sum(0), E_lane.sum(0) + cu * np.abs(lane).sum(0)]
    if with_err:
        sat, casc, et = w["sat"], w["casc"], w["et"]
        step = cu + cu * sat / (1.0 - sat)
        rel_casc = np.cumsum(step, 1) - step
        E_et = et * (cu + rel_casc + 2.0 * cu)
        lane, E_lane = np.cumsum(et, 1), np.cumsum(E_et, 1) + cu * ch * np.cumsum(np.abs(et), 1)
        out += [lane.sum(0), E_lane.sum(0) + cu * np.abs(lane).sum(0)]
    return out


def _quot(a, Ea, b, Eb, cu):
    with np.errstate(divide="ignore", invalid="ignore"):
        qv = np.where(b > 0, a / b, 0.0)
        return qv, np.where(b > 0, Ea / b + a * Eb / (b * b) + cu * np.abs(qv), 0.0)


def metrics_query(s, R, ks, alpha, max_label, c):
    """One query: dict(andcg, E_andcg [, err_ia, E_err_ia, nerr_ia, E_nerr_ia], valid), each [nk]."""
    nt, n = R.shape
    nk, cu, we = len(ks), c * U, max_label is not None
    a, e, ne, valid, k = DR.div_metrics(s, R, ks, alpha, max_label, kernel_consts=True, detail=True)
    z = np.zeros(nk)
    out = dict(andcg=z.copy(), E_andcg=z.copy(), err_ia=z.copy(), E_err_ia=z.copy(), nerr_ia=z.copy(), E_nerr_ia=z.copy(), valid=valid)
    if k is None:
        return out
    S, I = _lane_bounds(k["sys"], k["log2_c"], cu, we), _lane_bounds(k["ideal"], k["log2_c"], cu, we)
    sel = np.array([kk - 1 if 1 <= kk <= n else -1 for kk in ks])
    hit = sel >= 0
    pick = lambda v: np.where(hit, v[np.maximum(sel, 0)], 0.0)
    out["andcg"], out["E_andcg"] = _quot(pick(S[0]), pick(S[1]), pick(I[0]), pick(I[1]), cu)
    assert np.allclose(out["andcg"], a, rtol=1e-12, atol=0)
    if we:
        es, E_es = pick(S[2]) / nt, pick(S[3]) / nt + cu * pick(S[2]) / nt
        ei, E_ei = pick(I[2]) / nt, pick(I[3]) / nt + cu * pick(I[2]) / nt
        out["err_ia"], out["E_err_ia"] = es, E_es
        out["nerr_ia"], out["E_nerr_ia"] = _quot(es, E_es, ei, E_ei, cu)
        assert np.allclose(es, e, rtol=1e-12, atol=0) and np.allclose(out["nerr_ia"], ne, rtol=1e-12, atol=0)
    return out


METRIC_OUTPUTS = ("andcg", "err_ia", "nerr_ia")


def metrics(preds, rele, ks, alpha=0.5, max_label=None, lens=None, ntopics=None, c=None):
    """Float64 diversity metrics of a padded batch with bounds: dict(andcg, E_andcg, err_ia, E_err_ia, nerr_ia, E_nerr_ia [B, nk], valid [B])."""
    c = C_DIV if c is None else c
    preds, rele = np.asarray(preds), np.asarray(rele)
    B, T, L = rele.shape
    nk = len(ks)
    out = {k: np.zeros((B, nk)) for m in METRIC_OUTPUTS for k in (m, "E_" + m)}
    out["valid"] = np.zeros(B, np.int32)
    for q in range(B):
        n, nt = DR.clamp_len(lens, q, L), DR.clamp_len(ntopics, q, T)
        if n == 0 or nt == 0:
            continue
        one = metrics_query(preds[q, :n], rele[q, :nt, :n], ks, alpha, max_label, c)
        for k, v in one.items():
            out[k][q] = v
    return out


def gate_metrics(got, ref, what, c=None, needs=None):
    """got: (andcg, err_ia | None, nerr_ia | None, valid) as arrays.  `valid` exactly, the rest element-wise.  Returns the worst err/E and
    records it per output in `needs`."""
    c = C_DIV if c is None else c
    a, e, ne, v = got
    assert np.array_equal(np.asarray(v).astype(np.int64), ref["valid"].astype(np.int64)), f"{what}: valid {np.asarray(v).tolist()} != {ref['valid'].tolist()}"
    worst = 0.0
    for name, arr in zip(METRIC_OUTPUTS, (a, e, ne)):
        if arr is None:
            continue
        w = gate_nan(np.asarray(arr), ref[name], ref["E_" + name], f"{what} {name}", c)
        worst = max(worst, w)
        if needs is not None:
            needs[name] = max(needs.get(name, 0.0), w * c)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------- loss cases
def _rele(g, B, T, L, kind):
    if kind == "binary05":
        R = (g.random((B, T, L)) < 0.05).astype(np.float32)
    elif kind == "binary30":
        R = (g.random((B, T, L)) < 0.3).astype(np.float32)
    elif kind == "graded":
        R = (g.random((B, T, L)) < 0.3).astype(np.float32) * g.integers(1, 4, size=(B, T, L)).astype(np.float32)
    elif kind == "deep":                                     # >= 40 graded-relevant documents per subtopic: c^cover leaves fp32's normal range at alpha = 0.9
        R = (g.random((B, T, L)) < 0.9).astype(np.float32) * g.integers(1, 4, size=(B, T, L)).astype(np.float32)
    else:
        raise ValueError(kind)
    return R


def _scores(g, B, L, family):
    """(preds fp32 [B, L], rt)."""
    s = g.standard_normal((B, L))
    if family == "normal":
        return s.astype(np.float32), 10.0
    if family == "offset+":
        return (s + 1e3).astype(np.float32), 10.0
    if family == "offset-":
        return (s - 1e3).astype(np.float32), 10.0
    if family == "ties":
        return (np.round(s * 8.0) / 8.0).astype(np.float32), 10.0
    if family == "steep":
        return s.astype(np.float32), 100.0
    if family == "spread":
        lo, hi = s.min(1, keepdims=True), s.max(1, keepdims=True)
        return ((s - lo) / (hi - lo) * 10.0 - 5.0).astype(np.float32), 10.0    # a spread of 10 within a query: rt |ds| up to 100, e flushes past 87
    raise ValueError(family)


def _lengths(g, B, T, L, pick):
    """lens / ntopics over the edges: 0, 1, 2, L, the clamped -3 and L + 7; ntopics 0, 1, T, T + 2."""
    len_pool = [L - 1, 0, 1, 2, -3, L + 7, max(1, L // 2), 3, L]
    nt_pool = [T, T, 1, T + 2, T, 0, T, max(1, T - 1), T]
    lens = np.array([len_pool[(pick + q) % len(len_pool)] for q in range(B)], np.int32)
    nts = np.array([nt_pool[(pick + q) % len(nt_pool)] for q in range(B)], np.int32)
    return lens, nts


def loss_case(name, T, L, B, family="normal", alpha=0.5, rele="binary30", top_k=None, axis=0, pick=0, seed=0, full=False):
    """dict(name, preds, rele, lens, ntopics, rt, alpha, top_k, axis): fp32 inputs as the kernel gets them, garbage (NaN) in every padded
    slot, one query of all-zero relevance in each batch of at least 2 (the last one)."""
    g = np.random.default_rng(seed * 7919 + T * 131 + L + B)
    s, rt = _scores(g, B, L, family)
    R = _rele(g, B, T, L, rele)
    lens, nts = _lengths(g, B, T, L, pick)
    if full:
        lens[:], nts[:] = L, T
    lens[0], nts[0] = L, T                                   # query 0 is always whole; the edges follow it
    if B >= 2:
        R[B - 1] = 0.0
        lens[B - 1], nts[B - 1] = L, T
    for q in range(B):
        n, nt = DR.clamp_len(lens, q, L), DR.clamp_len(nts, q, T)
        s[q, n:] = np.nan
        R[q, nt:, :] = np.nan
        R[q, :, n:] = np.nan
    return dict(name=name, preds=s, rele=R, lens=lens, ntopics=nts, rt=rt, alpha=alpha, top_k=top_k, axis=axis)


def loss_cases(limit_forms=True):
    """The GPU cases of ptr_alphadcg_fwd_bwd (tests/test_diversity_bounds_gpu.py), also what need (a) is measured on."""
    cases = []
    forms = sorted(LOSS_FORMS)
    for i, (T, L) in enumerate(forms):                       # every (G, TP) at its smallest shape, every batch size of the four-query workgroup
        Bs = (1, 4, 5, 9) if L <= 128 else (3,)
        for B in Bs:
            cases.append(loss_case(f"form_T{T}_L{L}_B{B}", T, L, B, alpha=(0.1, 0.5, 0.9)[(i + B) % 3], rele=("binary05", "binary30", "graded")[(i + B) % 3],
                                   top_k=(None, 6)[(i + B) % 2], axis=(i + B // 2) % 2, pick=i + B, seed=i))
    if limit_forms:
        for T, L in sorted(LOSS_LIMIT_FORMS):
            cases.append(loss_case(f"limit_T{T}_L{L}", T, L, 1, rele="binary05", top_k=10, seed=3))
    fam_forms = {"offset+": ((3, 40), (8, 200)), "offset-": ((7, 100), (16, 260)), "ties": ((12, 128), (4, 129), (3, 40)),
                 "steep": ((30, 64), (8, 200), (7, 100)), "spread": ((3, 40), (32, 300))}
    for fam, fl in fam_forms.items():
        for j, (T, L) in enumerate(fl):
            cases.append(loss_case(f"{fam}_T{T}_L{L}", T, L, 5 if L <= 128 else 3, family=fam, alpha=(0.5, 0.9, 0.1)[j], rele=("graded", "binary30", "binary05")[j],
                                   top_k=(None, 4, 10)[j], axis=j % 2, pick=2 + j, seed=11 + j))
    for a in (0.1, 0.5, 0.9):                                # alpha x relevance on two forms
        for j, (T, L) in enumerate(((7, 100), (4, 129))):
            cases.append(loss_case(f"alpha{a}_T{T}_L{L}", T, L, 4 if L <= 128 else 3, alpha=a, rele=("graded", "binary05")[j], top_k=None, pick=j, seed=21))
    cases.append(loss_case("deep_cover_T3_L100", 3, 100, 4, alpha=0.9, rele="deep", top_k=None, pick=0, seed=31, full=True))
    cases.append(loss_case("deep_cover_T8_L200", 8, 200, 3, alpha=0.9, rele="deep", top_k=None, pick=0, seed=32, full=True))
    for axis in (0, 1):                                      # the cut-off at and beyond both axes
        T, L = 7, 24
        for k in (None, 1, T - 1, T, T + 1, L, L + 5):
            cases.append(loss_case(f"topk{k}_axis{axis}", T, L, 5, rele="graded", top_k=k, axis=axis, pick=1, seed=41))
    return cases


def loss_case_ref(cs, c=None):
    return alphadcg(cs["preds"], cs["rele"], cs["lens"], cs["ntopics"], cs["rt"], cs["alpha"], cs["top_k"], cs["axis"], c)


# ---------------------------------------------------------------------------------------------------------------------------- metric cases
MAX_INVALID = 0.10


def metric_case(name, T, L, B, scores="free", max_label=1.0, alpha=0.5, seed=0, nan_at=(), ks=None, full=()):
    """dict(name, preds, rele, lens, ntopics, ks, alpha, max_label).  Queries 0..7 (B >= 8) are planted: relevance totals of exactly 0,
    0.75, 1 (one document), 0.5 + 0.5 and 2, a query of 0 documents, of 1 document, and one with ntopics = 0; among the random queries at
    most MAX_INVALID may be invalid and no total lies within 1e-3 of 1 other than exactly (asserted)."""
    g = np.random.default_rng(seed * 104729 + T * 257 + L + B)
    top = 1 if max_label is None else int(max_label)
    R = (g.random((B, T, L)) < max(0.08, 3.0 / (T * L))).astype(np.float32) * g.integers(1, top + 1, size=(B, T, L)).astype(np.float32)
    lens = g.integers(max(1, L // 2), L + 1, size=B).astype(np.int32)
    nts = g.integers(1, T + 1, size=B).astype(np.int32)
    lens[0], nts[0] = L, T
    for q in full:
        lens[q] = L
    if scores == "free":
        s = g.permutation(B * L).reshape(B, L).astype(np.float64) / 7.0 - 3.0
    elif scores == "ties":
        s = g.integers(0, 4, size=(B, L)).astype(np.float64)
    elif scores == "zeros":
        u_ = g.random((B, L))
        s = np.where(u_ < 0.4, 0.0, np.where(u_ < 0.8, -0.0, 1.0))
    elif scores == "inf":
        s = g.standard_normal((B, L))
        s[g.random((B, L)) < 0.1] = np.inf
        s[g.random((B, L)) < 0.1] = -np.inf
    else:
        raise ValueError(scores)
    s = s.astype(np.float32)
    planted = 0
    if B >= 8:
        planted = 8
        R[1:8] = 0.0
        lens[1:8], nts[1:8] = max(1, min(L, 5)), T
        R[2, 0, 0] = 0.75
        R[3, 0, 0] = 1.0
        R[4, 0, 0] = 0.5; R[4, T - 1, min(L, 5) - 1] = 0.5
        R[5, 0, 0] = 2.0
        lens[6] = 0
        lens[7] = 1; R[7, 0, 0] = 1.0
        if B >= 9:
            planted = 9
            nts[8] = 0
    for q, where in nan_at:
        n = DR.clamp_len(lens, q, L)
        for w in ([where] if not isinstance(where, (list, tuple)) else where):
            idx = {"first": 0, "middle": n // 2, "last": n - 1}.get(w, w)
            if idx == "all":
                s[q, :n] = np.nan
            else:
                s[q, idx] = np.nan
    invalid = 0
    for q in range(B):
        n, nt = DR.clamp_len(lens, q, L), DR.clamp_len(nts, q, T)
        if q >= planted and q % 16 != 15 and not R[q, :nt, :n].any():
            R[q, 0, int(g.integers(0, n))] = 1.0             # keeps the random queries valid (every sixteenth is left as drawn)
        tot = float(R[q, :nt, :n].astype(np.float64).sum())
        assert tot == 1.0 or abs(tot - 1.0) > 1e-3, (name, q, tot)
        if q >= planted and not (n > 0 and nt > 0 and tot >= 1.0):
            invalid += 1
        s[q, n:] = np.nan
        R[q, nt:, :] = np.nan
        R[q, :, n:] = np.nan
    assert invalid <= MAX_INVALID * max(1, B - planted), f"{name}: {invalid} of {B - planted} random queries are invalid"
    if ks is None:
        ks = [5, 1, min(L, 20), 0, 5, L, L + 3, max(1, L // 2)]       # unsorted, a duplicate, a 0, one equal to n (query 0) and one beyond
    return dict(name=name, preds=s, rele=R, lens=lens, ntopics=nts, ks=[int(k) for k in ks], alpha=alpha, max_label=max_label)


def metric_cases():
    cases = []
    i = 0
    for form in sorted(METRIC_FORM_L):
        for L in METRIC_FORM_L[form]:
            T = (1, 5, 32)[i % 3]
            B = 10 if L <= 512 else 3
            cases.append(metric_case(f"form_G{form[0]}_DPT{form[1]}_L{L}", T, L, B, scores=("free", "ties", "free", "zeros", "inf")[i % 5],
                                     max_label=(1.0, 3.0, None)[i % 3], alpha=(0.5, 0.1, 0.9)[i % 3], seed=i))
            i += 1
    for T in (1, 5, 32):
        for sc in ("ties", "zeros", "inf"):
            cases.append(metric_case(f"T{T}_{sc}", T, 37, 12, scores=sc, max_label=3.0 if T == 5 else 1.0, seed=50 + T))
    return cases


def nan_metric_cases():
    """A NaN at the first, a middle and the last document, several, and every score of the list, at three lengths that straddle a wave and at
    one four-wave length (rows 9 .. 12 at full length; rows 0 and 3 carry one NaN too)."""
    nan_at = [(0, "first"), (9, "middle"), (10, "last"), (11, ["first", "middle", "last", 1]), (12, "all"), (3, "first")]
    return [metric_case(f"nan_L{L}", 5, L, 14, scores="free", max_label=3.0, seed=70 + L, nan_at=nan_at, full=(9, 10, 11, 12)) for L in (63, 64, 65, 300)]


def metric_case_ref(cs, c=None):
    return metrics(cs["preds"], cs["rele"], cs["ks"], cs["alpha"], cs["max_label"], cs["lens"], cs["ntopics"], c)
