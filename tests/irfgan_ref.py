"""Restatement of the IRFGAN point and pair kernels (csrc/irfgan.hip) in numpy / torch, from GIVEN uniforms, with gradients from autograd
and ELEMENT-WISE error bounds in the form of tests/irgan_ref.py (constant x fp32 unit round-off x sum of absolute terms).  The losses take a
dtype (float64 is the reference, float32 the CPU restatement whose own need sets the gate constant C_IRFGAN) and a form: 'literal' composes
conjugate_f(activation_f(v)) as ptranking/ltr_adversarial/util/f_divergence.py writes it, 'stable' evaluates the closed forms the kernel
uses (include/ptranking_amd.h lists them).

Reference lines.  pointwise/irfgan_point.py: the draws :179-192, the discriminator's loss :205, the generator's :213-216.
pairwise/irfgan_pair.py: :112-130, :143-150, :157-166.  util/pair_sampling.py: get_weighted_clipped_pos_diffs :26-50, generate_true_pairs
:53-77, sample_points_Bernoulli :111-122.

Sampling rules (include/ptranking_amd.h):
  positives / point fakes   as tests/irgan_ref.py: the V largest of P uniform keys; V rounds of arg-max of preds_i + gumbel(u_i), pinned
                            when the V + 1 largest keys are KEY_GAP apart.
  true pairs   the inverse CDF of w_ij = max(0, y_i - y_j) / (log2(2 + i) log2(2 + j)) in row-major order: draw k names the first pair
               whose running sum exceeds u_k W.  The kernel sums a row in fp32, j ascending (a chain of n additions: (n + 1) u relative),
               scans the row sums in tiles of 64 (a scan of depth 6, a carry per tile, the tile totals: (11 + ceil(P / 64)) u relative, met
               twice: at the prefix and at W), and rounds u_k W and the remainder once each.  A draw is PINNED by float64 when u_k W is not
               within true_margin(n, P) W of a boundary of the flat CDF, true_margin = 2 (n + 2 ceil(P / 64) + 25) u: twice that sum.
  fake pairs   b_ij = [u_ij < sigmoid(s_i - s_j)].  The kernel's sigmoid carries the rounding of the difference, u |d| sigma (1 - sigma),
               and of exp, the sum and the division, counted 4 u relative each way as tests/irgan_ref.py counts them: a bit is PINNED when
               |u_ij - sigma| > 2 u (|d| sigma (1 - sigma) + 4 sigma) + 2^-126.  Everything after the bits is integer arithmetic: M = the
               number of set bits, r_k = min(M - 1, floor(floor(u_k 2^24) M / 2^24)), the r-th set bit in row-major order — exact, never
               unpinned.

Error model of the losses, u = 2^-24, c the family constant.  A libm function (exp, expm1, tanh, log1p) counts 2 c u relative, an
arithmetic operation c u, softplus / sigmoid / log-sigmoid 4 c u as in tests/irgan_ref.py.  fdiv() returns each of a, a', c, c' with its
absolute bound in units of c u and the magnitude of the next derivative, through which the rounding of a difference v = head - tail
(c u |v|) reaches the value.  A mean over V is a wave butterfly (depth 6) and one product with 1 / V: 8 c u sum |terms|.  log p_i =
(x_i - m) - log Z carries d_i = c u |x_i - m|, Z's relative error eZ = sum p (d + 2 c u) + 8 c u, and the logarithm and the subtraction.
Every quantity built on an exponential carries the absolute floor 2^-126 times its cofactor."""
import numpy as np
import torch

from irgan_ref import KEY_GAP, TINY, U, _qlen, gumbel, order

F_DIVS = {"TVar": 0, "KL": 1, "RKL": 2, "PC": 3, "NC": 4, "SH": 5, "JS": 6, "GAN": 7}
MODES = {"POINT_D": 0, "PAIR_D": 1, "POINT_G": 2, "PAIR_G": 3}
LOG2 = float(np.log(2.0))
# The gate constant by the project's rule for C_METRIC: the need of the float32 CPU restatement on the GPU test's cases (c = 1), doubled,
# rounded up to a half, capped at 4: the float32 restatement needs 0.72 (the gradient of PAIR_D under TVar), hence 1.5.
# tests/test_irfgan_cpu.py::test_gate_constant_follows_the_fp32_restatement recomputes it.
C_IRFGAN = 1.5


# ------------------------------------------------------------------------------------------------------------- the divergences
def activation(f, v, log2_in_dtype=False):
    """activation_f of util/f_divergence.py, literally, in v's dtype.  Its JS writes log 2 as torch.log(torch.tensor(2.0)): a float32
    tensor whatever v's dtype, 0.6931471824645996, 1.9e-9 above log 2 — so the reference's float64 JS is not JS to better than that (its
    conjugate turns the offset into 1.9e-9 (1 + e^v), and into NaN from v = 20 on).  log2_in_dtype takes the constant in v's dtype."""
    if f == "TVar":
        return 0.5 * torch.tanh(v)
    if f in ("KL", "PC"):
        return v
    if f == "RKL":
        return -torch.exp(-v)
    if f in ("NC", "SH"):
        return 1.0 - torch.exp(-v)
    if f == "JS":
        return torch.log(torch.tensor(2.0, dtype=v.dtype if log2_in_dtype else torch.float32)) - torch.log(1.0 + torch.exp(-v))
    if f == "GAN":
        return -torch.log(1.0 + torch.exp(-v))
    raise KeyError(f)


def conjugate(f, t):
    """conjugate_f of util/f_divergence.py, literally."""
    if f == "TVar":
        return t
    if f == "KL":
        return torch.exp(t - 1)
    if f == "RKL":
        return -1.0 - torch.log(-t)
    if f == "PC":
        return 0.25 * torch.pow(t, exponent=2.0) + t
    if f == "NC":
        return 2.0 - 2.0 * torch.sqrt(1.0 - t)
    if f == "SH":
        return t / (1.0 - t)
    if f == "JS":
        return -torch.log(2.0 - torch.exp(t))
    if f == "GAN":
        return -torch.log(1.0 - torch.exp(t))
    raise KeyError(f)


def _half_tanh(v):
    """0.5 tanh v with the derivative the kernel evaluates, 0.5 sech^2 v = 2 s (1 - s), s = sigmoid(-2 |v|) <= 1/2: autograd's own
    0.5 (1 - tanh^2 v) cancels in float32 from |v| of 4 on, which would charge the float32 restatement with an error no kernel has (as
    tests/irgan_ref.py writes BCEWithLogits out for the same reason).  The value is tanh's; the second term is 0 and carries the gradient."""
    sgn = torch.where(v >= 0, 1.0, -1.0).to(v.dtype)
    s = sgn * (0.5 - torch.sigmoid(-2.0 * (v * sgn)))
    return (0.5 * torch.tanh(v)).detach() + (s - s.detach())


def _expm1(x, scale=1.0):
    """scale * expm1(x) with the derivative scale * exp(x), as the kernel evaluates it: autograd's expm1(x) + 1 cancels in float32 for x
    below -9 (the same reasoning as _half_tanh)."""
    s = scale * torch.exp(x)
    return (scale * torch.expm1(x)).detach() + (s - s.detach())


def act(f, v, form):
    """form 'literal': the reference's lines as written; 'literal64': the same with JS's log 2 in v's dtype; 'stable': the closed forms."""
    if form.startswith("literal"):
        return activation(f, v, form == "literal64")
    sp = torch.nn.functional.softplus
    if f == "TVar":
        return _half_tanh(v)
    if f in ("KL", "PC"):
        return v
    if f == "RKL":
        return -torch.exp(-v)
    if f in ("NC", "SH"):
        return _expm1(-v, -1.0)
    if f == "JS":
        return LOG2 - sp(-v)
    return -sp(-v)


def conj(f, v, form):
    """c(v) = conjugate_f(activation_f(v)): the composition, or the closed form."""
    if form.startswith("literal"):
        return conjugate(f, activation(f, v, form == "literal64"))
    sp = torch.nn.functional.softplus
    if f == "TVar":
        return _half_tanh(v)
    if f == "KL":
        return torch.exp(v - 1.0)
    if f == "RKL":
        return v - 1.0
    if f == "PC":
        return 0.25 * v * v + v
    if f == "NC":
        return _expm1(-0.5 * v, -2.0)
    if f == "SH":
        return _expm1(v)
    if f == "JS":
        return sp(v) - LOG2
    return sp(v)


def _sp(x):
    return np.logaddexp(0.0, x)


def _sg(x):
    return np.exp(-np.logaddexp(0.0, -x))


def fdiv(f, v):
    """float64 (a, a', |a''|, E_a, E_a') and (c, c', |c''|, E_c, E_c') at v, the bounds absolute in units of c u (module docstring)."""
    v = np.asarray(v, np.float64)
    one, zero = np.ones_like(v), np.zeros_like(v)
    if f == "TVar":
        th, s2 = np.tanh(v), 1.0 / np.cosh(v) ** 2
        A = C = (0.5 * th, 0.5 * s2, np.abs(s2 * th), 3.0 * np.abs(0.5 * th), 6.0 * 0.5 * s2)
    e, eh, ev = np.exp(-v), np.exp(-0.5 * v), np.exp(v)
    if f in ("KL", "PC"):
        A = (v, one, zero, zero, zero)
    if f == "KL":
        k = np.exp(v - 1.0)
        C = (k, k, k, k * (np.abs(v - 1.0) + 2.0), k * (np.abs(v - 1.0) + 2.0))
    if f == "RKL":
        A = (-e, e, e, 2.0 * e, 2.0 * e)
        C = (v - 1.0, one, zero, np.abs(v - 1.0), zero)
    if f == "PC":
        C = (0.25 * v * v + v, 0.5 * v + 1.0, 0.5 * one, 0.5 * v * v + np.abs(v) + np.abs(0.25 * v * v + v), 0.5 * np.abs(v) + 1.0)
    if f in ("NC", "SH"):
        A = (-np.expm1(-v), e, e, 2.0 * np.abs(np.expm1(-v)), 2.0 * e)
    if f == "NC":
        C = (-2.0 * np.expm1(-0.5 * v), eh, 0.5 * eh, 3.0 * np.abs(2.0 * np.expm1(-0.5 * v)), 2.0 * eh)
    if f == "SH":
        C = (np.expm1(v), ev, ev, 2.0 * np.abs(np.expm1(v)), 2.0 * ev)
    if f in ("JS", "GAN"):
        k = LOG2 if f == "JS" else 0.0
        a, c = k - _sp(-v), _sp(v) - k
        s2 = _sg(v) * _sg(-v)
        A = (a, _sg(-v), s2, 4.0 * _sp(-v) + k + np.abs(a), 4.0 * _sg(-v))
        C = (c, _sg(v), s2, 4.0 * _sp(v) + k + np.abs(c), 4.0 * _sg(v))
    return A, C


# ------------------------------------------------------------------------------------------------------------- the samplers
def point_sample(preds, num_pos, lens, S, unif):
    """ptr_irfgan_point_sample -> (pos_idx, neg_idx int64 [B, S], nsel int32 [B], pinned bool [B]).  unif fp32 [B, 2, L]."""
    preds, unif = np.asarray(preds, np.float32), np.asarray(unif, np.float32)
    B, L = preds.shape
    pos, neg = np.zeros((B, S), np.int64), np.zeros((B, S), np.int64)
    nsel, pinned = np.zeros(B, np.int32), np.ones(B, bool)
    for q in range(B):
        n = _qlen(lens, q, L)
        P = int(min(max(int(num_pos[q]), 0), n))
        V = min(P, S)                                                         # irfgan_point.py:182
        if V == 0 or np.isnan(preds[q, :n]).any():
            continue
        nsel[q] = V
        pos[q, :V] = order(unif[q, 0, :P])[:V]                                # :183 randperm(P)[:V]
        key = preds[q, :n].astype(np.float64) + gumbel(unif[q, 1, :n])        # :186, :192 multinomial(softmax, replacement=False)
        pi = order(key)
        neg[q, :V] = pi[:V]
        top = key[pi[:min(V + 1, n)]]
        pinned[q] = bool((top[:-1] - top[1:] > KEY_GAP).all()) if top.size > 1 else True
    return pos, neg, nsel, pinned


def pair_weights(labels, P):
    """get_weighted_clipped_pos_diffs (pair_sampling.py:26-50) in float64: w [P, n]."""
    y = np.asarray(labels, np.float64)
    n = y.size
    d = np.log2(2.0 + np.arange(n))
    return np.maximum(y[:P, None] - y[None, :], 0.0) / d[None, :] / d[:P, None]


def true_margin(n, P):
    return 2.0 * (n + 2 * -(-P // 64) + 25) * U


def point_fake_law(s, V):
    """Exact law of the V-th draw without replacement from softmax(s), by enumeration (small lists)."""
    import itertools
    w = np.exp(np.asarray(s, np.float64) - np.max(s))
    p = np.zeros(w.size)
    for seq in itertools.permutations(range(w.size), V):
        pr, rest = 1.0, w.sum()
        for i in seq:
            pr *= w[i] / rest
            rest -= w[i]
        p[seq[-1]] += pr
    return p


def fake_pair_law(s):
    """Exact law of ONE fake draw over the n x n pairs, by enumerating the 2^(n n) masks and conditioning on M > 0 (n <= 3)."""
    s = np.asarray(s, np.float64)
    n = s.size
    p = _sg(s[:, None] - s[None, :]).reshape(-1)
    law, alive = np.zeros(n * n), 0.0
    for mask in range(1, 2 ** (n * n)):
        bits = np.array([(mask >> k) & 1 for k in range(n * n)], bool)
        pr = float(np.prod(np.where(bits, p, 1.0 - p)))
        law += pr * bits / bits.sum()
        alive += pr
    return law / alive, alive


def pair_sample(preds, labels, num_pos, lens, S, unif_draw, unif_bern):
    """ptr_irfgan_pair_sample -> dict(true_head, true_tail, fake_head, fake_tail int64 [B, S], nsel, count int32 [B], loose_draw bool [B, S]
    (true draws float64 does not pin), loose_bern bool [B, L, L] (bits it does not pin)).  unif_draw fp32 [B, 2, S], unif_bern [B, L, L]."""
    preds, labels = np.asarray(preds, np.float32), np.asarray(labels, np.float32)
    ud, ub = np.asarray(unif_draw, np.float32), np.asarray(unif_bern, np.float32)
    B, L = preds.shape
    out = {k: np.zeros((B, S), np.int64) for k in ("true_head", "true_tail", "fake_head", "fake_tail")}
    out.update(nsel=np.zeros(B, np.int32), count=np.zeros(B, np.int32), loose_draw=np.zeros((B, S), bool), loose_bern=np.zeros((B, L, L), bool))
    for q in range(B):
        n = _qlen(lens, q, L)
        P = int(min(max(int(num_pos[q]), 0), n))
        if n == 0 or np.isnan(preds[q, :n]).any() or labels[q, 0] == labels[q, n - 1]:    # irfgan_pair.py:109, :120-123
            continue
        w = pair_weights(labels[q, :n], P).reshape(-1)
        Cs = np.cumsum(w)
        W = Cs[-1] if Cs.size else 0.0
        if not W > 0.0:
            continue
        s = preds[q, :n].astype(np.float64)
        d = s[:, None] - s[None, :]
        sig = _sg(d)
        u = ub[q, :n, :n].astype(np.float64)
        bits = u < sig                                                        # pair_sampling.py:113-114
        out["loose_bern"][q, :n, :n] = np.abs(u - sig) <= 2.0 * U * (np.abs(d) * sig * (1.0 - sig) + 4.0 * sig) + TINY
        M = int(bits.sum())
        out["count"][q] = M
        if M == 0:
            continue
        out["nsel"][q] = S
        x = ud[q, 0].astype(np.float64) * W                                   # :58 multinomial(w.view(1, -1), replacement=True)
        flat = np.minimum(np.searchsorted(Cs, x, side="right"), w.size - 1)
        for k in range(S):
            while w[flat[k]] == 0.0:
                flat[k] -= 1
        out["true_head"][q], out["true_tail"][q] = flat // n, flat % n        # :62-63
        bounds = np.unique(Cs)                                                # a zero weight adds no boundary
        j = np.searchsorted(bounds, x)
        near = np.minimum(np.abs(x - bounds[np.maximum(j - 1, 0)]), np.abs(x - bounds[np.minimum(j, bounds.size - 1)]))
        near = np.minimum(near, x)                                            # and 0, the start of the first pair
        out["loose_draw"][q] = near <= true_margin(n, P) * W
        setbits = np.flatnonzero(bits.reshape(-1))                            # :116 multinomial(mask, replacement=True): uniform over the set bits
        k24 = np.floor(np.clip(ud[q, 1].astype(np.float64), 0.0, 1.0) * 2.0 ** 24).astype(np.int64)
        r = np.minimum(M - 1, (k24 * M) >> 24)
        out["fake_head"][q], out["fake_tail"][q] = setbits[r] // n, setbits[r] % n      # :119-120
    return out


# ------------------------------------------------------------------------------------------------------------- the losses
def loss(x, nsel, mode, f_div, d_fake=None, idx_a=None, idx_b=None, lens=None, dtype=torch.float64, form="stable", c=None):
    """ptr_irfgan_fwd_bwd -> dict(loss_q, grad, valid_q, loss, E_loss_q, E_grad, E_loss); gradients from autograd on the reference's own
    expressions (the generator's log-softmax and log-sigmoid written as such)."""
    c = C_IRFGAN if c is None else c
    x_np = np.asarray(x, np.float32)
    B, W = x_np.shape
    gen = mode.endswith("_G")
    pair = mode.startswith("PAIR")
    S = idx_a.shape[1] if gen else W // (4 if pair else 2)
    out = dict(loss_q=np.zeros(B), grad=np.zeros((B, W)), valid_q=np.zeros(B), E_loss_q=np.zeros(B), E_grad=np.zeros((B, W)))
    cu = c * U
    for q in range(B):
        V = int(min(max(int(nsel[q]), 0), S))
        if V == 0:
            continue
        out["valid_q"][q] = 1.0
        xs = torch.tensor(x_np[q], dtype=dtype, requires_grad=True)
        if not gen:
            parts = [xs[p * V:(p + 1) * V] for p in range(4 if pair else 2)]
            vt, vf = (parts[0] - parts[1], parts[2] - parts[3]) if pair else parts
            ls = torch.mean(conj(f_div, vf, form)) - torch.mean(act(f_div, vt, form))      # irfgan_point.py:205, irfgan_pair.py:150
        else:
            n = _qlen(lens, q, W)
            ia = np.asarray(idx_a[q, :V], np.int64)
            ok = (ia >= 0) & (ia < n)
            dk = torch.tensor(np.asarray(d_fake[q], np.float32), dtype=dtype)
            if pair:                                                          # irfgan_pair.py:157-166
                ib = np.asarray(idx_b[q, :V], np.int64)
                ok &= (ib >= 0) & (ib < n)
                ck = conj(f_div, dk[:V] - dk[V:2 * V], form)
                sa, sb = torch.tensor(np.where(ok, ia, 0)), torch.tensor(np.where(ok, ib, 0))
                lg = torch.log(torch.sigmoid(xs[sa] - xs[sb])) if form != "stable" else torch.nn.functional.logsigmoid(xs[sa] - xs[sb])
            else:                                                             # irfgan_point.py:213-216
                ck = conj(f_div, dk[:V], form)
                sa = torch.tensor(np.where(ok, ia, 0))
                if n == 0:
                    lg = torch.zeros(V, dtype=dtype)
                else:
                    lg = (torch.log(torch.softmax(xs[:n], dim=0)) if form != "stable" else torch.log_softmax(xs[:n], dim=0))[sa]
            okt = torch.tensor(ok)
            ls = -(torch.where(okt, lg * torch.where(okt, ck, torch.zeros_like(ck)), torch.zeros(V, dtype=dtype))).sum() / V
        if ls.requires_grad:
            ls.backward()
            out["grad"][q] = xs.grad.double().numpy()
        out["loss_q"][q] = float(ls.detach())
        if dtype != torch.float64 or form != "stable":
            continue
        # ---- bounds (float64, closed forms)
        xd = x_np[q].astype(np.float64)
        if not gen:
            if pair:
                vt, vf = xd[:V] - xd[V:2 * V], xd[2 * V:3 * V] - xd[3 * V:4 * V]
                rt, rf = np.abs(vt), np.abs(vf)                               # the rounding of head - tail, in units of c u
            else:
                vt, vf, rt, rf = xd[:V], xd[V:2 * V], 0.0, 0.0
            (a, da, d2a, Ea, Eda), _ = fdiv(f_div, vt)
            _, (cc, dc, d2c, Ec, Edc) = fdiv(f_div, vf)
            out["E_loss_q"][q] = cu * ((Ea + da * rt).sum() + (Ec + np.abs(dc) * rf).sum() + 8.0 * (np.abs(a).sum() + np.abs(cc).sum())) / V + V * TINY
            ea = cu * (Eda + d2a * rt + 2.0 * np.abs(da)) / V + TINY
            ec = cu * (Edc + d2c * rf + 2.0 * np.abs(dc)) / V + TINY
            out["E_grad"][q, :(4 if pair else 2) * V] = np.concatenate([ea, ea, ec, ec] if pair else [ea, ec])
            continue
        dn = np.asarray(d_fake[q], np.float32).astype(np.float64)
        okf = ok.astype(np.float64)
        if pair:
            v = dn[:V] - dn[V:2 * V]
            _, (cc, dc, d2c, Ec, Edc) = fdiv(f_div, v)
            E_ck = cu * (Ec + np.abs(dc) * np.abs(v)) + TINY
            z = xd[sa.numpy()] - xd[sb.numpy()]
            dz = cu * np.abs(z)
            lsg, sg = -_sp(-z), _sg(-z)
            E_ls = dz * sg + 4.0 * cu * np.abs(lsg) + TINY
            E_sg = dz * sg * (1.0 - sg) + 4.0 * cu * sg + TINY
            t = np.abs(lsg * cc) / V
            out["E_loss_q"][q] = float((((E_ls * np.abs(cc) + np.abs(lsg) * E_ck) / V + 3.0 * cu * t) * okf).sum() + 8.0 * cu * (t * okf).sum())
            gk = sg * np.abs(cc) / V
            E_gk = (E_sg * np.abs(cc) + sg * E_ck) / V + 3.0 * cu * gk
            for i in range(n):
                touch = ok & ((ia == i) | (ib == i))
                if touch.any():
                    out["E_grad"][q, i] = 2.0 * E_gk[touch].sum() + 2.0 * touch.sum() * cu * gk[touch].sum() + TINY
            continue
        _, (cc, dc, d2c, Ec, Edc) = fdiv(f_div, dn[:V])
        E_ck = cu * Ec + TINY
        xr = xd[:n]
        if n == 0:
            continue
        m = xr.max()
        p = np.exp(xr - m)
        Z = p.sum()
        p /= Z
        lp = (xr - m) - np.log(Z)
        dzi = cu * np.abs(xr - m)
        eZ = float((p * (dzi + 2.0 * cu)).sum() + 8.0 * cu)
        E_lp = dzi + eZ + 2.0 * cu * abs(np.log(Z)) + cu * np.abs(lp)
        sel = sa.numpy()
        t = np.abs(lp[sel] * cc) / V
        out["E_loss_q"][q] = float((((E_lp[sel] * np.abs(cc) + np.abs(lp[sel]) * E_ck) / V + 3.0 * cu * t) * okf).sum() + 8.0 * cu * (t * okf).sum())
        csum, E_C = float((cc * okf).sum()), float((E_ck * okf).sum() + V * cu * (np.abs(cc) * okf).sum())
        e_p = dzi + eZ + 3.0 * cu
        for i in range(n):
            hit = ok & (ia == i)
            own, E_own = float(cc[hit].sum()), float(E_ck[hit].sum() + hit.sum() * cu * np.abs(cc[hit]).sum())
            out["E_grad"][q, i] = (E_own + p[i] * E_C + p[i] * abs(csum) * e_p[i] + 3.0 * cu * (abs(own) + p[i] * abs(csum)) + TINY * abs(csum)) / V + TINY
    out["loss"] = float(np.sum(out["loss_q"]))
    out["E_loss"] = float(np.sum(out["E_loss_q"]) + cu * np.abs(out["loss_q"]).sum())
    return out
