"""Float64 restatement of the cross-entropy nDCG objective, LightGBM's rank_xendcg (csrc/tree.hip tree_xendcg_kernel; include/ptranking_amd.h
states the rule), with ELEMENT-WISE error bounds, an eager-torch fp32 evaluation of the same closed form with planted faults, and the
counter stream of its uniforms restated on tests/plsample_ref.py.  The rule is this project's own, modelled on LightGBM's RankXENDCG;
LightGBM is installed nowhere this project is tested, so nothing here is compared with it.

For one query of n documents, scores s, labels y >= 0, one uniform u_i in [0, 1) per document:
    n <= 1: grad = hess = 0 exactly
    rho_i = exp(s_i - max s) / Z                        phi_i = 2^y_i - u_i,  P = sum phi
    q_i = max(1 - rho_i, 2^-20)                         (the floor is this project's addition: every output is finite)
    a_i = rho_i - phi_i / P,   x_i = a_i / q_i,   A  = sum x
    b_i = rho_i (A - x_i),     z_i = b_i / q_i,   Bs = sum z
    c_i = rho_i (Bs - z_i)
    grad_i = (a_i + b_i) + c_i,   hess_i = rho_i (1 - rho_i)  (unfloored)
A NaN score or label, a negative label or a uniform outside [0, 1): NaN on every document of the list (a list of one document included).

Bounds: the error model of tests/f64_loss_bounds.py (u = 2^-24, c = C_LIST = 4, the constant of the softmax-based kernels; no new constant).
  * the softmax as f64_loss_bounds._log_softmax bounds it, in the form the kernel evaluates (e / Z, no logarithm is taken): an exponential
    carries c u (1 + |s - m|) relative — its own error and its argument's — except at s = m, where the argument is exactly 0 and exp(0)
    is exactly 1; Z carries the sum of those and c u Z; rho = e / Z one more c u:  E_rho = E_e / Z + rho (E_Z / Z + c u);
  * 1 - rho: E_rho + c u (1 - rho).  q = max(1 - rho, floor) is 1-Lipschitz: E_q = E_(1 - rho), and 0 where 1 - rho + E stays below the floor
    (then the kernel holds the floor exactly too).  A quotient by q is bounded with q's lower end qlo = max(q - E_q, floor), not to first
    order: near the floor E_q / q is no small number.  |1 / q^ - 1 / q| <= E_q / (q qlo) — THE 1 / q AMPLIFICATION;
  * phi = 2^y - u: c u (2^y + phi);  P: the sum of those and c u P;  phi / P: E_phi / P + (phi / P) E_P / P + c u phi / P;
  * a = rho - phi / P — THE FIRST CANCELLATION: E_a = E_rho + E_(phi / P) + c u |a|, absolute, whatever is left of a;
  * x = a / q: E_x = E_a / qlo + |a| E_q / (q qlo) + c u |x|;  A = sum x by a tree: sum E_x + c u sum |x|;
  * A - x_i — THE SECOND CANCELLATION: the kernel subtracts the very x_i^ it added, so x_i's own error drops out and what remains is the
    others' errors, the tree's rounding c u sum_j |x_j| (x_i's share included: on a list with one dominant document |x_i| is 2^20 |a_i| and
    A - x_i a number of order 1, known to c u 2^20 |a_i| and no better) and c u |A - x_i| for the subtraction;
  * b = rho (A - x_i): E_rho |A - x_i| + rho E_(A - x_i) + c u |b|;  z, Bs and Bs - z_i exactly as x, A and A - x_i — THE THIRD;
  * grad = (a + b) + c: E_a + E_b + E_c + c u (|a + b| + |grad|);  hess = rho (1 - rho): |1 - 2 rho| E_rho + c u hess, as tree_ref.listnet_query.
Exact results (E = 0): a list of one document is 0 in both outputs; a list with a bad input is NaN (gate_nan demands it).

Measured worst need (err / E times C_LIST) over gpu_inputs() below:
    the eager fp32 form (CPU, test_xendcg_cpu.py)          1.00 ('dominant'; 'straddle' 0.77)
    the kernel on an MI355X (test_xendcg_gpu.py)           1.00 ('dominant', the leading document of a list whose rho rounds to 1; 'straddle' 0.67)
"""
import numpy as np
import torch

import f64_loss_bounds as FB
import plsample_ref as PR
import tree_ref as TR
from f64_bounds import U

C = FB.C_LIST
FLOOR = 2.0 ** -20
FAULTS = ("no_second", "no_third", "phi_plus_u", "own_term", "hess_floored", "no_floor")
M32 = np.uint64(PR.M32)


# ---------------------------------------------------------------------------------------------------------------------------- the stream
def uniforms(seed, draw, d):
    """u(seed, draw, d) for global document indices d, bit for bit what the kernel draws: the counter hash of plsample_ref.uniforms_host with
    the round as its query, hi32(d) as its sample and lo32(d) as its index -> float32, multiples of 2^-24 in [0, 1)."""
    seed = int(seed) & (2 ** 64 - 1)
    draw = int(draw) & (2 ** 64 - 1)
    one = lambda v: np.array([v], np.uint64)
    lo, hi, qlo, qhi = one(seed & PR.M32), one(seed >> 32), one(draw & PR.M32), one(draw >> 32)
    mul = lambda a, c: (a * np.uint64(c)) & M32
    lb = PR._lowbias32
    ka_q = lb(lo ^ lb((hi + mul(qlo, 0x9E3779B1) + mul(qhi, 0xC2B2AE3D)) & M32))
    kb_q = lb(hi ^ lb((lo + mul(qlo, 0x85EBCA77) + mul(qhi, 0x27D4EB2F) + np.uint64(0x68E31DA4)) & M32))
    d = np.asarray(d, np.int64).astype(np.uint64).reshape(-1)
    s, i = d >> np.uint64(32), d & M32
    ka = lb((ka_q + mul(s, 0xC2B2AE3D)) & M32)
    kb = lb((kb_q + mul(s, 0x9E3779B1)) & M32)
    h = lb((ka + mul(i, 0x85EBCA77)) & M32)
    t = ((h ^ kb) * np.uint64(0x2C1B3C6D)) & M32
    return ((t >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------- float64
def _bad(s, y, u):
    with np.errstate(invalid="ignore"):
        return bool(np.isnan(s).any() or not (y >= 0).all() or not ((u >= 0) & (u < 1)).all())


def query(s, y, u, c=C, detail=False):
    """One query -> (grad, E_grad, hess, E_hess), float64 [n]; detail: a dict with a and E_a as well."""
    s, y, u = FB._f64(s), FB._f64(y), FB._f64(u)
    n = s.size
    pack = lambda g, Eg, h, Eh, **kw: dict(grad=g, E_grad=Eg, hess=h, E_hess=Eh, **kw) if detail else (g, Eg, h, Eh)
    if n == 0:
        return pack(*(np.zeros(0),) * 4, a=np.zeros(0), E_a=np.zeros(0))
    if _bad(s, y, u):
        return pack(np.full(n, np.nan), np.zeros(n), np.full(n, np.nan), np.zeros(n), a=np.full(n, np.nan), E_a=np.zeros(n))
    if n == 1:
        return pack(*(np.zeros(1),) * 4, a=np.zeros(1), E_a=np.zeros(1))
    cu = c * U
    im = int(np.argmax(s))
    dv = s - s[im]
    e = np.exp(dv)
    Z = e.sum()
    Ee = np.where(dv == 0.0, 0.0, e * cu * (1.0 + np.abs(dv)))
    E_Z = Ee.sum() + cu * Z
    rho = e / Z
    E_rho = Ee / Z + rho * (E_Z / Z + cu)
    omr = 1.0 - rho
    omr[im] = np.delete(e, im).sum() / Z                       # the largest rho may round to 1 even here: its complement from the others
    E_omr = E_rho + cu * omr
    q = np.maximum(omr, FLOOR)
    E_q = np.where(omr + E_omr <= FLOOR, 0.0, E_omr)
    qlo = np.maximum(q - E_q, FLOOR)
    E_iq = E_q / (q * qlo)
    g2 = np.exp2(y)
    phi = g2 - u
    E_phi = cu * (g2 + phi)
    P = phi.sum()
    E_P = E_phi.sum() + cu * P
    r = phi / P
    E_r = E_phi / P + r * E_P / P + cu * r
    a = rho - r
    E_a = E_rho + E_r + cu * np.abs(a)

    def order(prev, E_prev):
        """v = prev / q, V = sum v, rho (V - v) and its bound."""
        v = prev / q
        E_v = E_prev / qlo + np.abs(prev) * E_iq + cu * np.abs(v)
        rest = v.sum() - v
        E_rest = (E_v.sum() - E_v) + cu * np.abs(v).sum() + cu * np.abs(rest)
        nxt = rho * rest
        return nxt, E_rho * np.abs(rest) + rho * E_rest + cu * np.abs(nxt)

    b, E_b = order(a, E_a)
    cc, E_c = order(b, E_b)
    grad = a + b + cc
    E_grad = E_a + E_b + E_c + cu * (np.abs(a + b) + np.abs(grad))
    hess = rho * omr
    E_hess = np.abs(1.0 - 2.0 * rho) * E_rho + cu * hess
    return pack(grad, E_grad, hess, E_hess, a=a, E_a=E_a)


def batch(preds, labels, unif, group, c=C):
    """query over a ragged batch -> dict(idx, grad, E_grad, hess, E_hess): flat float64, every document."""
    preds, labels, unif = np.asarray(preds), np.asarray(labels), np.asarray(unif)
    off = TR.offsets_of(group)
    assert off[-1] == preds.size == labels.size == unif.size
    out = {k: np.zeros(preds.size) for k in ("grad", "E_grad", "hess", "E_hess")}
    for a, b in zip(off[:-1], off[1:]):
        for k, v in zip(("grad", "E_grad", "hess", "E_hess"), query(preds[a:b], labels[a:b], unif[a:b], c)):
            out[k][a:b] = v
    out["idx"] = np.arange(preds.size)
    return out


def gate(got_grad, got_hess, ref, what, c=C):
    """tree_ref.gate: element-wise, NaN exactly where the restatement is NaN.  Returns the worst err / E."""
    return TR.gate(got_grad, got_hess, ref, what, c)


# ---------------------------------------------------------------------------------------------------------------------------- fp32, eager
def eager_query(s, y, u, fault=None, dtype=torch.float32, parts=False):
    """The closed form evaluated by eager torch in `dtype` on the CPU: what a plain fp32 implementation computes.  The gate must pass it,
    or the bounds are impossible.  fault: one of FAULTS, planted for the gate to reject.  parts: return a as well."""
    assert fault is None or fault in FAULTS, fault
    sn, yn, un = FB._f64(s), FB._f64(y), FB._f64(u)
    n = sn.size
    ret = lambda g, h, a: (g, h, a) if parts else (g, h)
    if n == 0:
        return ret(np.zeros(0), np.zeros(0), np.zeros(0))
    if _bad(sn, yn, un):
        return ret(np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan))
    if n == 1:
        return ret(np.zeros(1), np.zeros(1), np.zeros(1))
    S, Y, Un = (torch.tensor(v, dtype=dtype) for v in (sn, yn, un))
    e = torch.exp(S - S.max())
    rho = e / e.sum()
    phi = (torch.exp2(Y) - 1.0 + Un) if fault == "phi_plus_u" else (torch.exp2(Y) - Un)
    omr = 1.0 - rho
    q = omr if fault == "no_floor" else torch.clamp(omr, min=FLOOR)
    a = rho - phi / phi.sum()
    x = a / q
    b = rho * (x.sum() if fault == "own_term" else x.sum() - x)
    z = b / q
    c = rho * (z.sum() if fault == "own_term" else z.sum() - z)
    grad = a
    if fault != "no_second":
        grad = grad + b
    if fault != "no_third":
        grad = grad + c
    hess = rho * (q if fault == "hess_floored" else omr)
    return ret(grad.double().numpy(), hess.double().numpy(), a.double().numpy())


def eager_batch(preds, labels, unif, group, **kw):
    preds, labels, unif = np.asarray(preds), np.asarray(labels), np.asarray(unif)
    off = TR.offsets_of(group)
    grad, hess = np.zeros(preds.size), np.zeros(preds.size)
    for a, b in zip(off[:-1], off[1:]):
        grad[a:b], hess[a:b] = eager_query(preds[a:b], labels[a:b], unif[a:b], **kw)
    return grad, hess


# ---------------------------------------------------------------------------------------------------------------------------- data
# first and last length of every form and of every length class the host launches separately (tests/test_tree_gpu.py STRADDLE)
STRADDLE = [0, 1, 2, 16, 17, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1251, 2048, 2049, 4096]
DOMINANT = [2, 2, 17, 17, 130, 130, 1025, 1025]                  # per length: one list led by 40, one by 12
MID = [1, 17, 64, 130, 300]
NAN_GROUP = [17, 64, 130, 3]
OBJECTIVE_GROUP = [12, 1, 18, 64, 3, 0, 200]
ONE_BELOW = float(np.float32(1.0) - np.float32(2.0 ** -24))      # the largest fp32 uniform below 1


def draw_uniforms(n, rng):
    """fp32 multiples of 2^-24 in [0, 1), as the stream gives them."""
    return (rng.integers(0, 2 ** 24, size=n).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def gpu_inputs():
    """name -> (preds, labels, unif, group): every input list of tests/test_xendcg_gpu.py's gated tests, in fp32."""
    out = {}
    g = np.random.default_rng(23)
    N = int(np.sum(STRADDLE))
    y = FB.labels_like(1, N, "mslr", g)[0].astype(np.float32)
    out["straddle"] = ((2.0 * g.standard_normal(N)).astype(np.float32), y, draw_uniforms(N, g), STRADDLE)
    N = int(np.sum(DOMINANT))
    s = (0.5 * g.standard_normal(N)).astype(np.float32)
    off = TR.offsets_of(DOMINANT)
    for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
        lead = a + int(g.integers(0, b - a))
        rest = np.delete(s[a:b], lead - a)
        s[lead] = np.float32(rest.max() + (40.0 if k % 2 == 0 else 12.0))
    out["dominant"] = (s, FB.labels_like(1, N, "mslr", g)[0].astype(np.float32), draw_uniforms(N, g), DOMINANT)
    s, y = TR.tree_inputs(MID, seed=5)
    N = s.size
    out["equal scores"] = (np.full_like(s, 0.25), y, draw_uniforms(N, g), MID)
    out["offset 1e3"] = TR.tree_inputs(MID, seed=5, offset=1e3) + (draw_uniforms(N, g), MID)
    out["edge uniforms"] = (s, y, np.where(g.integers(0, 2, N) == 0, np.float32(0.0), np.float32(ONE_BELOW)).astype(np.float32), MID)
    return out


_REFS = {}


def reference(name):
    """batch() on gpu_inputs()[name], computed once per process and shared (callers must not change it)."""
    if name not in _REFS:
        _REFS[name] = batch(*gpu_inputs()[name])
    return _REFS[name]
