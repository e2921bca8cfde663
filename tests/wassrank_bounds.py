"""Float64 restatement of WassRank WITH element-wise error bounds (csrc/wassrank.hip, ptr_wassrank_fwd_bwd), the ragged NaN-padded batches of
the GPU gate (tests/test_wassrank_bounds_gpu.py) and the fp32 measurement that sets the family constant C_WASS.

The values are those of tests/wassrank_ref.py (wassRank.py:43-88, mode 'SinkhornOT', smooth_type 'ST', norm_type 'BothST'; the cost of
wasserstein_cost_mat.py:47-139; the log-domain Sinkhorn of pytorch_wasserstein.py:323-393 with every log-sum-exp on its own row's maximum);
tests/test_wassrank_cpu.py holds the two restatements to 1e-12 of each other.  The gate is f64_bounds.gate through f64_loss_bounds.gate_nan /
gate_losses:  |got - ref| <= E  element by element, E = c * A + F with u = 2^-24, c = C_WASS, A the first-order sum below at c = 1 and F the
fp32 underflow floors.  A NaN must appear exactly where the float64 result has one.

Per query of n documents, scores s, labels y, m = the maximum label over the REAL documents (scale_by_max_label) or 1:

  softmaxes   log a = log_softmax(m s), log b = log_softmax(y): f64_loss_bounds._log_softmax (ListNet's bound: the max shift, one exponential
              per element, the normaliser, its logarithm).  z_i = m s_i is one rounding relative to |m s_i| unless m is a power of two (then it
              is exact), and reaches log a_i as E_z_i + sum_j a_j E_z_j.  A common score offset therefore costs c u m |offset| when m is 3,
              nothing when it is 1, 2 or 4.
  cost        p1, p2: |i - j| and its square are integers below 2^24: exact, E_C = 0.
              eg: the gain k = gain_base^y - 1 is formed by the device power function: c u relative to gain_base^y = k + 1, kept where
              k >= 1; a gain below 1 is the constant -non_rele_gap (exact).  d = |k_i - k_j| carries E_k_i + E_k_j + u d; where d < 1 the
              cost is the constant var_penalty and on the diagonal 0: both exact.
              dg: k = 2^y - 1 likewise; equal labels are the same fp32 value on both sides: d = 0 exactly.
              ddg: d |D_i - D_j| with D = 1 / log2(pos + 2) taken in fp32 (as the reference does); each discount carries c u relative, so
              |D_i - D_j| carries c u (D_i + D_j) ABSOLUTE (the cancellation of adjacent discounts deep in a list); the product c u C.
              A cost error reaches every exponent divided by lam.
  one row     out_j = base_j - LSE_i(t_ij),  t_ij = x_i - C_ij / lam,  LSE = M_j + log S_j,  S_j = sum_i exp(t_ij - M_j) >= 1,
              w_ij = exp(t_ij - M_j) / S_j (sum_i w_ij = 1):
                  E_t_ij  = E_x_i + E_C_ij / lam + c u (|t_ij| + C_ij / lam)      (the fused multiply-add, and the fp32 factor 1 / lam)
                  E_out_j = E_base_j + sum_i w_ij (E_t_ij + c u (1 + |t_ij - M_j|))     (the shift by the maximum, the exponential)
                            + c u (1 + |log S_j| + |LSE_j| + |out_j|)                   (the sum of terms >= 1 at its maximum, the logarithm,
                                                                                         M + log S, base - LSE)
  iterations  the weights w of a row sum to 1, so a pass hands the bounds of its input on as a weighted MEAN: the Sinkhorn map does not
              expand errors in the log domain, and the 2 sh_itr + 1 row passes add their own roundings at most linearly — the bound of
              log u / log v after k passes is a sum of k per-pass terms, never a product.  log u = log v = -log n at the start: c u log n.
  loss        sum_ij C_ij exp(e_ij), e_ij = (log u_i - C_ij / lam) + log v_j:
                  E_e_ij = E_logu_i + E_logv_j + E_C_ij / lam + c u (1 + |e_ij| + |log u_i - C_ij / lam| + C_ij / lam)
                  E_term = term E_e + E_C exp(e) + 2^-126 max(1, C_ij)        (an exponential below fp32's normal range is flushed to 0
                                                                               before the cost multiplies it: the absolute floor F)
                  E_loss = sum E_term + c u loss.
              Without the floor the bound is useless wherever the loss itself lies below fp32's range (lam = 0.01: losses of 1e-51 and less).
  gradient    m a_i (g_i - sum_j a_j g_j) / B, g = lam log u.  The kernel centres g by its mean first; a shift of g cancels out of the
              result (sum a = 1), so the centring is not charged, but every rounding is relative to the CENTRED g, which is what the kernel
              holds:   E_g_i = lam E_logu_i + c u |g_i|,   E_a_i = a_i (E_loga_i + c u) + 2^-126,
                  E_d_i  = E_g_i + sum_j (a_j E_g_j + E_a_j |g_j|) + c u (sum_j a_j |g_j| + |g_i| + |sum a g|)
                  E_grad_i = m / B (E_a_i |d_i| + a_i E_d_i) + c u 2 |grad_i| + 2^-126 (1 + m |d_i| / B).
  exact       padded documents: gradient exactly 0.  A list of 0 or 1 documents: loss 0, gradient 0.  E = 0 demands equality.
  batch       loss_out = mean of loss_q: f64_loss_bounds.batch_total with scale 1 / B.

C_WASS is 2 x the worst need of the reference's own arithmetic in fp32 — `torch_fp32_query`, eager torch on the CPU running the same
per-row-maximum formulas — measured on exactly the batches of the GPU gate (GATE_CASES), rounded up to a half: the rule of C_GAUSS.
`measure_fp32_need` re-measures it (tests/test_wassrank_cpu.py), so the constant cannot drift, and it is never set from the kernel."""
import functools
import math

import numpy as np
import torch

import wassrank_ref as W
from f64_bounds import U
from f64_loss_bounds import _log_softmax, labels_like

# 2 x the worst need of the fp32 eager-torch evaluation over GATE_CASES (measure_fp32_need), rounded up to a half.  Measured on the CPU:
# grad 1.26 (sweep_L520_eg_lam0.1_itr1: one iteration, lists of 520 / 300 / 129 documents), loss_q 0.59 (sweep_L520_p1_lam0.1_itr0),
# loss_out 0.32 (sweep_L128_p1_lam0.1_itr0); the ragged batches need at most 0.90 (grad, L = 1028, ddg, scaled by the maximum label).
# The kernel on an MI355X (tests/test_wassrank_bounds_gpu.py, the MEASURED lines): grad 1.32 (sweep_L520_eg_lam0.1_itr1; ragged batches
# 0.90, L = 1028, p2, scaled), loss_q 0.74 (sweep_L520_p1_lam1_itr0), loss_out 0.38 (sweep_L520_eg_lam1_itr0): 0.44 of the constant.
C_WASS = 3.0
TINY = 2.0 ** -126
COSTS = W.COST_TYPES
DEFAULTS = dict(lam=0.1, sh_itr=20, gain_base=4.0, non_rele_gap=100.0, var_penalty=math.e)
PAD_LABEL = 9.0                       # padded slots: NaN scores and a label above every real one
FRAC_LABELS = (0.0, 0.3, 0.6, 0.8, 1.05, 1.1, 1.3, 2.0, 2.1)      # the fractional label set of tests/golden/wassrank.npz
SCREEN = 1e-3                         # every eg gain and gain difference of a random case keeps this distance from 1
MAX_SCREENED = 0.01


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _pow2(m):
    return m > 0 and math.frexp(m)[0] == 0.5


# ---------------------------------------------------------------------------------------------------------------------------- cost
def cost_and_bound(y, cost_type, gain_base, non_rele_gap, var_penalty, diag_fault=False):
    """C [n, n] float64 (wassrank_ref.cost_matrix's values) and A_C, its bound at c = 1, as torch tensors.  diag_fault: the planted fault
    of the tests — the eg diagonal costs var_penalty."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    pos = np.arange(n, dtype=np.float64)
    zero = np.zeros((n, n))
    if cost_type in ("p1", "p2"):
        c = np.abs(pos[:, None] - pos[None, :])
        return _t(c * c if cost_type == "p2" else c), _t(zero)
    if cost_type == "eg":
        gap, vp = float(np.float32(non_rele_gap)), float(np.float32(var_penalty))
        pw = np.power(float(gain_base), y)
        kept = (pw - 1.0) >= 1.0
        k = np.where(kept, pw - 1.0, -gap)
        Ek = np.where(kept, U * pw, 0.0)
        d = np.abs(k[:, None] - k[None, :])
        far = d >= 1.0
        c = np.where(far, d, vp)
        Ec = np.where(far, Ek[:, None] + Ek[None, :] + U * d, 0.0)
        if not diag_fault:
            np.fill_diagonal(c, 0.0)
        np.fill_diagonal(Ec, 0.0)
        return _t(c), _t(Ec)
    pw = np.power(2.0, y)
    k = pw - 1.0
    Ek = U * pw
    d = np.abs(k[:, None] - k[None, :])
    Ed = np.where(y[:, None] == y[None, :], 0.0, Ek[:, None] + Ek[None, :] + U * d)
    if cost_type == "dg":
        return _t(d), _t(Ed)
    D = (np.float32(1.0) / np.log2(pos.astype(np.float32) + np.float32(2.0))).astype(np.float64)
    dD = np.abs(D[:, None] - D[None, :])
    EdD = U * (D[:, None] + D[None, :])
    np.fill_diagonal(EdD, 0.0)
    c = d * dD
    return _t(c), _t(Ed * dD + d * EdD + U * c)


# ---------------------------------------------------------------------------------------------------------------------------- one query
def _row_pass(x, A_x, base, A_base, Kmat, Q):
    """out_j = base_j - LSE_i(x_i + Kmat_ij) and its bound at c = 1 (module docstring).  Kmat = -C / lam (symmetric), Q the static part
    of the per-term bound: A_C / lam + u (1 + C / lam)."""
    T = Kmat + x[None, :]
    M = T.max(dim=1, keepdim=True).values
    Dm = T - M
    Ex = torch.exp(Dm)
    S = Ex.sum(dim=1, keepdim=True)
    w = Ex / S
    lS = torch.log(S[:, 0])
    lse = M[:, 0] + lS
    out = base - lse
    loc = (w * (Q + U * (Dm.abs() + T.abs()))).sum(dim=1) + w @ A_x
    return out, A_base + loc + U * (1.0 + lS.abs() + lse.abs() + out.abs())


def query(preds, labels, cost_type="eg", lam=0.1, sh_itr=20, gain_base=4.0, non_rele_gap=100.0, var_penalty=math.e,
          scale_by_max_label=False, m_fault=None, diag_fault=False):
    """One unpadded query at B = 1 -> dict(loss, A_loss, F_loss, grad, A_grad, F_grad): float64 values, bounds at c = 1 and floors.
    The planted faults of the tests — m_fault: a maximum label to use in place of the list's own; diag_fault: the eg diagonal costs
    var_penalty, everywhere (True) or in the row passes alone ("rows": the loss sum keeps the right cost)."""
    s = np.asarray(preds, dtype=np.float64)
    y = np.asarray(labels, dtype=np.float64)
    n = s.shape[0]
    z0 = np.zeros(n)
    if n <= 1:
        return dict(loss=0.0, A_loss=0.0, F_loss=0.0, grad=z0, A_grad=z0, F_grad=z0)
    lam = float(lam)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = (float(np.max(y)) if m_fault is None else float(m_fault)) if scale_by_max_label else 1.0
        z = m * s
        A_z = np.zeros(n) if (_pow2(m) or m == 0.0) else U * np.abs(z)
        la, A_la, a = _log_softmax(z, 1.0, A_z)
        lb, A_lb, _ = _log_softmax(y, 1.0)
    C, A_C = cost_and_bound(y, cost_type, gain_base, non_rele_gap, var_penalty, diag_fault is True)
    Kmat = -C / lam
    Q = A_C / lam + U * (1.0 - Kmat)
    K_rows = -cost_and_bound(y, cost_type, gain_base, non_rele_gap, var_penalty, True)[0] / lam if diag_fault == "rows" else Kmat
    la_t, lb_t, A_la_t, A_lb_t = _t(la), _t(lb), _t(A_la), _t(A_lb)
    lu = torch.full((n,), -math.log(n), dtype=torch.float64)
    lv = lu.clone()
    A_lu = torch.full((n,), U * math.log(n), dtype=torch.float64)
    A_lv = A_lu.clone()
    for _ in range(int(sh_itr)):
        lv, A_lv = _row_pass(lu, A_lu, lb_t, A_lb_t, K_rows, Q)
        lu, A_lu = _row_pass(lv, A_lv, la_t, A_la_t, K_rows, Q)
    r = lu[:, None] + Kmat
    e = r + lv[None, :]
    Pm = torch.exp(e)
    term = C * Pm
    A_e = A_lu[:, None] + A_lv[None, :] + A_C / lam + U * (1.0 + e.abs() + r.abs() - Kmat)
    loss = float(term.sum())
    A_loss = float((term * A_e + A_C * Pm).sum()) + U * abs(loss)
    F_loss = TINY * float(C.clamp(min=1.0).sum())
    lu_n, A_lu_n = lu.numpy(), A_lu.numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        g = lam * lu_n
        g = g - g.mean()
        A_g = lam * A_lu_n + U * np.abs(g)
        A_a = a * (A_la + U)
        sag = np.sum(a * g)
        d = g - sag
        A_d = A_g + np.sum(a * A_g + A_a * np.abs(g)) + U * (np.sum(a * np.abs(g)) + np.abs(g) + abs(sag))
        grad = m * a * d
        A_grad = abs(m) * (A_a * np.abs(d) + a * A_d) + 2.0 * U * np.abs(grad)
        F_grad = TINY * (1.0 + 2.0 * abs(m) * np.abs(d))
    if not np.isfinite(loss):
        A_loss, F_loss = 0.0, 0.0
    nz = lambda v: np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)
    return dict(loss=loss, A_loss=nz(A_loss), F_loss=F_loss, grad=grad, A_grad=nz(A_grad), F_grad=nz(F_grad))


def batch(preds, labels, lens=None, **kw):
    """Padded batch [B, L] -> dict(q, loss_q, A_loss_q, F_loss_q, grad, A_grad, F_grad): grad carries the 1 / B, padded documents 0 with
    bound 0.  `with_c` turns it into what f64_loss_bounds.gate_losses takes."""
    preds, labels = np.asarray(preds), np.asarray(labels)
    B, L = preds.shape
    res = dict(q=np.arange(B), B=B)
    for k in ("loss_q", "A_loss_q", "F_loss_q"):
        res[k] = np.zeros(B)
    for k in ("grad", "A_grad", "F_grad"):
        res[k] = np.zeros((B, L))
    for q in range(B):
        n = L if lens is None else int(lens[q])
        out = query(preds[q, :n], labels[q, :n], **kw)
        res["loss_q"][q], res["A_loss_q"][q], res["F_loss_q"][q] = out["loss"], out["A_loss"], out["F_loss"]
        res["grad"][q, :n], res["A_grad"][q, :n], res["F_grad"][q, :n] = out["grad"] / B, out["A_grad"] / B, out["F_grad"]
    return res


def with_c(ref, c=None):
    """dict(q, loss_q, E_loss_q, grad, E_grad) at the constant c (default C_WASS) and the batch total (mean loss, its bound)."""
    c = C_WASS if c is None else c
    out = dict(q=ref["q"], loss_q=ref["loss_q"], E_loss_q=c * ref["A_loss_q"] + ref["F_loss_q"], grad=ref["grad"],
               E_grad=c * ref["A_grad"] + ref["F_grad"])
    lq = ref["loss_q"]
    with np.errstate(invalid="ignore"):
        total = (lq.sum() / ref["B"], (out["E_loss_q"].sum() + c * U * np.abs(lq).sum()) / ref["B"]) if ref["B"] else (0.0, 0.0)
    return out, total


def need_of(got, ref, A, F):
    """The constant c this data needs: the worst (|got - ref| - F) / A over the finite elements with A > 0."""
    got, ref, A, F = (np.asarray(v, np.float64).reshape(-1) for v in (got, ref, np.broadcast_to(A, np.shape(ref)), np.broadcast_to(F, np.shape(ref))))
    ok = (A > 0) & np.isfinite(ref)
    return float(np.max((np.abs(got[ok] - ref[ok]) - F[ok]) / A[ok])) if ok.any() else 0.0


def needs(lq, grad, total, ref):
    """Per-output needed constants of one batch result (loss_q [B], grad [B, L], loss_out) against ref = batch(...)."""
    B = ref["B"]
    lq64 = ref["loss_q"]
    with np.errstate(invalid="ignore"):
        A_tot = (ref["A_loss_q"].sum() + U * np.abs(lq64).sum()) / max(B, 1)
        F_tot = ref["F_loss_q"].sum() / max(B, 1)
        tot = lq64.sum() / max(B, 1)
    return dict(loss_q=need_of(lq, lq64, ref["A_loss_q"], ref["F_loss_q"]), grad=need_of(grad, ref["grad"], ref["A_grad"], ref["F_grad"]),
                loss_out=need_of([total], [tot], [A_tot], [F_tot]))


# ---------------------------------------------------------------------------------------------------------------------------- gate data
def eg_keys(y, gain_base, non_rele_gap):
    g = np.power(float(gain_base), np.asarray(y, np.float64)) - 1.0
    return g, np.where(g < 1.0, -float(np.float32(non_rele_gap)), g)


def eg_ambiguous(y, gain_base, non_rele_gap):
    """Documents of one list whose eg gain, or whose gain difference with another document, lies within SCREEN of 1: there the fp32 power
    function and the float64 one may land on different sides of a discontinuity of the cost."""
    y = np.asarray(y, np.float64)
    vals = np.unique(y)
    g, k = eg_keys(vals, gain_base, non_rele_gap)
    bad = np.abs(g - 1.0) < SCREEN
    dd = np.abs(np.abs(k[:, None] - k[None, :]) - 1.0) < SCREEN
    bad |= dd.any(axis=1)
    return np.isin(y, vals[bad])


def gate_inputs(L, lens, seed, sigmas=(1.0, 3.0), labels="mslr", gain_base=4.0, non_rele_gap=100.0):
    """A ragged batch [len(lens), L] -> (preds, labels fp32, lens int32).  Padded slots hold NaN scores and the label PAD_LABEL, above every
    real one.  List q has scores sigmas[q % len] N(0, 1), every third list on a common offset of 1e3; labels from the MSLR mix (or the
    fixtures' fractional set), sorted in every other PAIR of lists, unsorted in the rest (p1 / p2 go by position).  Every list is screened
    for the eg discontinuities (a screened document gets label 0); the screen must move fewer than MAX_SCREENED of the documents."""
    rng = np.random.default_rng(seed)
    B = len(lens)
    P = np.full((B, L), np.nan, np.float32)
    Y = np.full((B, L), PAD_LABEL, np.float32)
    moved = total = 0
    for q, n in enumerate(lens):
        assert 0 <= n <= L
        if n == 0:
            continue
        s = sigmas[q % len(sigmas)] * rng.standard_normal(n) + (1e3 if q % 3 == 2 else 0.0)
        if labels == "mslr":
            y = labels_like(1, n, "mslr", rng)[0]
        else:
            y = rng.choice(np.asarray(FRAC_LABELS), size=n)
        if (q // 2) % 2 == 0:
            y = -np.sort(-y)
        y = y.astype(np.float32)
        amb = eg_ambiguous(y, gain_base, non_rele_gap)
        y[amb] = 0.0
        moved, total = moved + int(amb.sum()), total + n
        assert float(y.max()) < PAD_LABEL
        P[q, :n], Y[q, :n] = s.astype(np.float32), y
    assert moved <= MAX_SCREENED * max(total, 1), f"the eg screen moved {moved} of {total} documents"
    assert not eg_screen_hits(Y, lens, gain_base, non_rele_gap)
    return P, Y, np.asarray(lens, np.int32)


def eg_screen_hits(Y, lens, gain_base, non_rele_gap):
    """Number of documents of a padded batch inside the screened bands (0 after gate_inputs)."""
    return sum(int(eg_ambiguous(Y[q, :n], gain_base, non_rele_gap).sum()) for q, n in enumerate(lens) if n)


# the ragged batches: padded width -> list lengths on the edges of the form (0, 1, 2 documents; the wave of 64, the tile G x DPT and the
# multiple of 4 on both sides; in the widest form one, two and three column tiles with one, two and all four waves alive in the last)
RAGGED = {62: [0, 1, 2, 3, 5, 61, 62],
          64: [0, 1, 2, 63, 64],
          128: [0, 1, 2, 63, 64, 65, 66, 127, 128],
          256: [0, 1, 2, 64, 65, 129, 191, 192, 193, 255, 256],
          1028: [0, 1, 2, 3, 255, 257, 511, 512, 513, 575, 576, 577, 769, 1023, 1025, 1028]}
SWEEP_LENS = {128: [128, 97, 2], 520: [520, 300, 129]}
SWEEP_LAMS = (0.01, 0.1, 1.0)
SWEEP_ITRS = (0, 1, 20, 50)
ALT_EG = ((3.0, 10.0, 0.5), (2.0, 25.0, 2.0))      # (gain_base, non_rele_gap, var_penalty) of the fixtures eg_params_*


def _case(name, L, lens, seed, cost, scale=False, sigmas=(1.0, 3.0), labels="mslr", **kw):
    return dict(name=name, L=L, lens=tuple(lens), seed=seed, sigmas=tuple(sigmas), labels=labels,
                kw=dict(DEFAULTS, cost_type=cost, scale_by_max_label=bool(scale), **kw))


def _gate_cases():
    ragged, sweep = [], []
    for k, (L, lens) in enumerate(RAGGED.items()):
        for cost in COSTS:
            for scale in (False, True):
                ragged.append(_case(f"ragged_L{L}_{cost}_{'scaled' if scale else 'plain'}", L, lens, 4100 + k, cost, scale))
    others = [c for c in COSTS if c != "eg"]
    for L, lens in SWEEP_LENS.items():
        k = 0
        for lam in SWEEP_LAMS:
            for itr in SWEEP_ITRS:
                for cost in ("eg", others[k % 4]):          # eg on every (lam, sh_itr); the other four costs in turn
                    sweep.append(_case(f"sweep_L{L}_{cost}_lam{lam:g}_itr{itr}", L, lens, 4200 + L, cost, k % 2 == 1, lam=lam, sh_itr=itr))
                k += 1
        gb, gap, vp = ALT_EG[0]                                 # base 3 on integer labels: gains 0, 2, 8, 26, 80
        sweep.append(_case(f"sweep_L{L}_eg_base3", L, lens, 4300 + L, "eg", True, gain_base=gb, non_rele_gap=gap, var_penalty=vp))
        gb, gap, vp = ALT_EG[1]                                 # base 2: an integer label 1 has the gain exactly 1 (EXACT_EG holds that case)
        sweep.append(_case(f"sweep_L{L}_eg_base2_frac", L, lens, 4310 + L, "eg", False, labels="frac", gain_base=gb, non_rele_gap=gap,
                           var_penalty=vp))
        sweep.append(_case(f"sweep_L{L}_eg_frac", L, lens, 4320 + L, "eg", True, labels="frac"))
        for cost in ("eg", "p1", "ddg"):
            sweep.append(_case(f"sweep_L{L}_{cost}_sigma10", L, lens, 4330 + L, cost, cost != "p1", sigmas=(10.0,)))
    return ragged, sweep


RAGGED_CASES, SWEEP_CASES = _gate_cases()
GATE_CASES = RAGGED_CASES + SWEEP_CASES
CASE_BY_NAME = {c["name"]: c for c in GATE_CASES}

# the exact cases of the eg cost: a gain of exactly 1 stays on the `gain >= 1` side (2^1 - 1 and 4^0.5 - 1 are exact in fp32 and float64)
EXACT_EG = (dict(gain_base=2.0, labels=(0.0, 1.0, 2.0)), dict(gain_base=4.0, labels=(0.0, 0.5, 1.0)))


def exact_eg_inputs(spec, L=64, B=4, seed=77):
    """A small ragged batch over the label set of an EXACT_EG case, every label present in every list of three or more documents."""
    rng = np.random.default_rng(seed)
    lens = [L, 3, 17, 40][:B]
    P = np.full((B, L), np.nan, np.float32)
    Y = np.full((B, L), PAD_LABEL, np.float32)
    vals = np.asarray(spec["labels"], np.float32)
    for q, n in enumerate(lens):
        y = rng.choice(vals, size=n)
        y[:3] = vals
        P[q, :n], Y[q, :n] = rng.standard_normal(n).astype(np.float32), (-np.sort(-y) if q % 2 else y)
    return P, Y, np.asarray(lens, np.int32)


def case_inputs(case):
    kw = case["kw"]
    return gate_inputs(case["L"], case["lens"], case["seed"], case["sigmas"], case["labels"], kw["gain_base"], kw["non_rele_gap"])


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(preds, labels, lens, ref) of a gate case; the float64 restatement with its bounds is computed once per process and left unchanged."""
    case = CASE_BY_NAME[name]
    P, Y, n = case_inputs(case)
    ref = batch(P, Y, n, **case["kw"])
    for v in (P, Y, n, *[a for a in ref.values() if isinstance(a, np.ndarray)]):
        v.setflags(write=False)
    return P, Y, n, ref


# ---------------------------------------------------------------------------------------------------------------------------- fp32
def torch_fp32_query(preds, labels, cost_type="eg", lam=0.1, sh_itr=20, gain_base=4.0, non_rele_gap=100.0, var_penalty=math.e,
                     scale_by_max_label=False):
    """The same formulas, every log-sum-exp on its own row's maximum, in eager fp32 torch on the CPU -> (loss, grad [n]) at B = 1: the
    arithmetic the kernel replaces, in the precision it runs in.  Measures what fp32 needs of the bounds; never compared with the kernel."""
    f = torch.float32
    s = torch.as_tensor(np.array(preds, dtype=np.float32))
    y = torch.as_tensor(np.array(labels, dtype=np.float32))
    n = s.numel()
    if n <= 1:
        return 0.0, np.zeros(n)
    pos = torch.arange(n, dtype=f)
    if cost_type in ("p1", "p2"):
        C = (pos[:, None] - pos[None, :]).abs()
        C = C * C if cost_type == "p2" else C
    elif cost_type == "eg":
        g = torch.pow(torch.tensor(gain_base, dtype=f), y) - 1.0
        g = torch.where(g < 1.0, torch.tensor(-non_rele_gap, dtype=f), g)
        C = (g[:, None] - g[None, :]).abs()
        C = torch.where(C < 1.0, torch.tensor(var_penalty, dtype=f), C)
        C.fill_diagonal_(0.0)
    else:
        g = torch.pow(torch.tensor(2.0, dtype=f), y) - 1.0
        C = (g[:, None] - g[None, :]).abs()
        if cost_type == "ddg":
            D = 1.0 / torch.log2(pos + 2.0)
            C = C * (D[:, None] - D[None, :]).abs()
    m = y.max() if scale_by_max_label else torch.tensor(1.0, dtype=f)

    def lsm(v):
        d = v - v.max()
        return d - torch.log(torch.exp(d).sum())

    def lse_rows(x):
        mx = x.max(dim=1, keepdim=True).values
        return (mx + torch.log(torch.exp(x - mx).sum(dim=1, keepdim=True)))[:, 0]

    la, lb = lsm(m * s), lsm(y)
    lam_t = torch.tensor(lam, dtype=f)
    Kmat = -C / lam_t
    lu = torch.full((n,), -math.log(n), dtype=f)
    lv = lu.clone()
    for _ in range(int(sh_itr)):
        lv = lb - lse_rows(Kmat + lu[None, :])
        lu = la - lse_rows(Kmat + lv[None, :])
    loss = (C * torch.exp(lu[:, None] + Kmat + lv[None, :])).sum()
    g = lam_t * lu
    g = g - g.mean()
    a = torch.exp(la)
    grad = m * a * (g - (a * g).sum())
    assert loss.dtype == f and grad.dtype == f
    return float(loss), grad.double().numpy()


def torch_fp32_batch(P, Y, lens, **kw):
    B, L = P.shape
    lq = np.zeros(B, np.float32)
    grad = np.zeros((B, L))
    for q in range(B):
        n = int(lens[q])
        lq[q], gq = torch_fp32_query(P[q, :n], Y[q, :n], **kw)
        grad[q, :n] = (torch.as_tensor(gq).float() * torch.tensor(1.0 / B, dtype=torch.float32)).double().numpy()
    total = float(torch.as_tensor(lq).sum() * torch.tensor(1.0 / B, dtype=torch.float32)) if B else 0.0
    return lq.astype(np.float64), grad, total


OUTPUTS = ("loss_q", "grad", "loss_out")


def measure_fp32_need(cases=None):
    """The constant the fp32 evaluation of the reference's formulas needs on the batches of the GPU gate, per output, and the case that
    needs it."""
    worst = {k: (0.0, None) for k in OUTPUTS}
    for case in (GATE_CASES if cases is None else cases):
        P, Y, n, ref = case_ref(case["name"])
        lq, grad, total = torch_fp32_batch(P, Y, n, **case["kw"])
        for k, v in needs(lq, grad, total, ref).items():
            if v > worst[k][0]:
                worst[k] = (v, case["name"])
    return worst


def constant_from_need(need):
    """Twice the worst need, rounded up to a half."""
    return math.ceil(2.0 * need * 2.0 - 1e-9) / 2.0

