"""Restatement of the IRGAN point and pair kernels (csrc/irgan.hip) in torch, from GIVEN uniforms, with gradients from autograd and
ELEMENT-WISE error bounds in the form of tests/f64_bounds.py (constant x fp32 unit round-off x sum of absolute terms).  Every function
takes a dtype: float64 is the reference, float32 is the CPU restatement whose own need sets the gate constant (C_IRGAN below).

Reference lines.  ptranking/ltr_adversarial/pointwise/irgan_point.py: per_query_generation :130-146, the discriminator's BCEWithLogits
:161-169, the generator's step :184-217 (reward :42).  ptranking/ltr_adversarial/pairwise/irgan_pair.py: per_query_generation :140-161, the
discriminator's losses :180-184, the reward :39-42, the generator's draw and loss :207-218.

Sampling rules (include/ptranking_amd.h), z = preds / T:
  with replacement     w_i >= 0 the unnormalised weights, C = cumsum(w): draw k names the smallest i with u_k C_{n-1} < C_i, the last document
                       when there is none, then the nearest document at or below with w_i > 0.  (torch.multinomial(replacement=True) draws
                       from the same law.)  A draw is PINNED by float64 only when u_k C_{n-1} is not within 2^-12 C_{n-1} of a boundary.
  without replacement  V rounds of arg-max of key_i = log-weight_i + gumbel(u_i), (key descending, index ascending); pinned when the V + 1
                       largest keys are 1e-4 apart.
  positives            the V largest of P uniform keys, (key descending, index ascending); fp32 comparisons are exact: always pinned.

Error model, u = 2^-24, c the family constant.  z_i carries u |z_i| (the division by T), z_i - m one more rounding and m's own:
d_i = u (|z_i| + |m| + |z_i - m|); e_i = exp(z_i - m) is relative d_i + c u; Z = sum e relative eZ = sum p (d + c u) + c u;
log p_i = z_i - m - log Z absolute d_i + eZ + c u (|log Z| + |log p_i|); rho_i = e_i / w_i relative 2 (d_i + c u) + eZ + 2 c u.  A loss is a
sum of terms (c u sum |terms|) whose factors carry the above; a gradient h_j - p_j H carries E_h_j + p_j E_H + |p_j H| (d_j + eZ + 2 c u)
and the roundings of its own operations.  exp below 2^-126 flushes: every quantity built on e_i carries the absolute floor 2^-126 times its
cofactor.  softplus / sigmoid / log-sigmoid count 4 c u relative (exp, log1p or the division, the sum)."""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
MARGIN = 2.0 ** -12          # a with-replacement draw: distance of u C_{n-1} from every boundary, in units of C_{n-1}
KEY_GAP = 1e-4               # without replacement: the gap between competing Gumbel keys
SAMPLE_MODES = {"POINT_D": 0, "PAIR_D": 1, "PAIR_G": 2}
SEL_MODES = {"POINT_D": 0, "PAIR_D_SVM": 1, "PAIR_D_LOG": 2, "PAIR_G_SVM": 3, "PAIR_G_LOG": 4}
# The gate constant by the project's rule for C_METRIC: the need of the float32 CPU restatement on the GPU test's cases (c = 1), doubled,
# rounded up to a half, capped at 4: the float32 restatement needs 0.63 (the gradient of PAIR_D_LOG), hence 1.5.
# tests/test_irgan_cpu.py::test_gate_constant_follows_the_fp32_restatement recomputes it.
C_IRGAN = 1.5


def _qlen(lens, q, L):
    return L if lens is None else int(min(max(int(lens[q]), 0), L))


def _z(s, T, dtype=np.float64):
    s = np.asarray(s, dtype=dtype)
    t = dtype(np.float32(T))
    return s if t == 1.0 else s / t


def gumbel(u):
    """pl_gumbel in float64 on the fp32 sum u + 1e-20 (sampling_utils.py:68)."""
    uu = (np.asarray(u, np.float32) + np.float32(1e-20)).astype(np.float64)
    return -np.log(-np.log(uu) + 1e-20)


def order(key):
    key = np.asarray(key, dtype=np.float64)
    return np.lexsort((np.arange(key.size), -key))


def inverse_cdf(w, u):
    """(documents, pinned) of the with-replacement rule for weights w and uniforms u (float64 arithmetic on the fp32 inputs)."""
    w = np.asarray(w, np.float64)
    Cs = np.cumsum(w)
    total = Cs[-1]
    x = np.asarray(u, np.float64) * total
    i = np.minimum(np.searchsorted(Cs, x, side="right"), w.size - 1)
    for k in range(i.size):
        while i[k] > 0 and w[i[k]] == 0.0:
            i[k] -= 1
    if w.size == 1:
        return i.astype(np.int64), np.ones(x.shape, bool)
    bounds = Cs[:-1]                                                         # ascending: the nearest boundary is a neighbour of x's slot
    j = np.searchsorted(bounds, x)
    near = np.minimum(np.abs(x - bounds[np.maximum(j - 1, 0)]), np.abs(x - bounds[np.minimum(j, bounds.size - 1)]))
    return i.astype(np.int64), near > MARGIN * total


def gen_weights(g_row, P, T, lam):
    """w_i = (1 - lambda) e_i + [i < P] lambda Z / P of the generator step, float64."""
    z = _z(g_row, T)
    e = np.exp(z - z.max())
    w = (1.0 - float(np.float32(lam))) * e
    w[:P] += float(np.float32(lam)) * e.sum() / P
    return w


def sample(preds, num_pos, lens, S, mode, T, unif):
    """ptr_irgan_sample -> (pos_idx, neg_idx int64 [B, S], nsel int32 [B], pinned bool [B]).  unif fp32 [B, 2, L]."""
    preds, unif = np.asarray(preds, np.float32), np.asarray(unif, np.float32)
    B, L = preds.shape
    pos, neg = np.zeros((B, S), np.int64), np.zeros((B, S), np.int64)
    nsel, pinned = np.zeros(B, np.int32), np.ones(B, bool)
    for q in range(B):
        n = _qlen(lens, q, L)
        P = int(min(max(int(num_pos[q]), 0), n))
        V = min(P, S) if mode == "POINT_D" else min(P, n - P, S)
        if V == 0 or np.isnan(preds[q, :n]).any():
            continue
        nsel[q] = V
        pos[q, :V] = order(unif[q, 0, :P])[:V]                                # randperm(P)[:V], irgan_point.py:135 / irgan_pair.py:149
        z = _z(preds[q, :n], T)
        if mode == "POINT_D":                                                 # irgan_point.py:140-142
            neg[q, :V], ok = inverse_cdf(np.exp(z - z.max()), unif[q, 1, :V])
            pinned[q] = ok.all()
            continue
        first = P if mode == "PAIR_D" else 0                                  # irgan_pair.py:153-157 | :210-211
        lw = z if mode == "PAIR_D" else -np.logaddexp(0.0, -z)
        key = np.full(n, -np.inf)
        key[first:] = lw[first:] + gumbel(unif[q, 1, first:n])
        pi = order(key)
        neg[q, :V] = pi[:V]
        top = key[pi[:min(V + 1, n - first)]]
        pinned[q] = bool((top[:-1] - top[1:] > KEY_GAP).all()) if top.size > 1 else True
    return pos, neg, nsel, pinned


def gen_counts(g_preds, num_pos, lens, T, lam, dpp, unif):
    """The draw counts of ptr_irgan_point_gen_fwd_bwd -> (counts int32 [B, L], pinned bool [B, dpp * L] per draw).  unif fp32 [B, dpp, L]."""
    g_preds, unif = np.asarray(g_preds, np.float32), np.asarray(unif, np.float32)
    B, L = g_preds.shape
    counts = np.zeros((B, L), np.int32)
    pinned = np.ones((B, dpp * L), bool)
    for q in range(B):
        n = _qlen(lens, q, L)
        P = int(min(max(int(num_pos[q]), 0), n))
        if P == 0 or np.isnan(g_preds[q, :n]).any():
            continue
        K = dpp * P                                                           # irgan_point.py:203
        i, ok = inverse_cdf(gen_weights(g_preds[q, :n], P, T, lam), unif[q].reshape(-1)[:K])
        counts[q, :n] = np.bincount(i, minlength=n)
        pinned[q, :K] = ok
    return counts, pinned


def point_generator(g_preds, d_preds, num_pos, lens, T, lam, counts, dtype=torch.float64, c=C_IRGAN):
    """irgan_point.py:184-217 on given draw counts -> dict(loss_q, grad, valid_q, loss, E_loss_q, E_grad, E_loss).  The counts stand for
    choose_inds: sum over the draws = sum over the documents of c_i times the term."""
    g_np, d_np = np.asarray(g_preds, np.float32), np.asarray(d_preds, np.float32)
    B, L = g_np.shape
    out = dict(loss_q=np.zeros(B), grad=np.zeros((B, L)), valid_q=np.zeros(B), E_loss_q=np.zeros(B), E_grad=np.zeros((B, L)))
    Tt = float(np.float32(T))
    lam = float(np.float32(lam))
    cu = c * U
    for q in range(B):
        n = _qlen(lens, q, L)
        P = int(min(max(int(num_pos[q]), 0), n))
        if P == 0:
            continue
        out["valid_q"][q] = 1.0
        if np.isnan(g_np[q, :n]).any():
            out["loss_q"][q] = np.nan
            out["grad"][q, :n] = np.nan
            continue
        g = torch.tensor(g_np[q, :n], dtype=dtype, requires_grad=True)
        d = torch.tensor(d_np[q, :n], dtype=dtype)
        cnt = torch.tensor(np.asarray(counts[q, :n]), dtype=dtype)
        K = float(cnt.sum())
        z = g if Tt == 1.0 else g / Tt                                        # :28-33 predict
        logp = torch.log_softmax(z, dim=0)                                    # :197, as log-softmax
        p = torch.exp(logp)
        a = torch.zeros(n, dtype=dtype)
        a[:P] = lam / P
        qq = (1.0 - lam) * p + a                                              # :199-201
        reward = 2.0 * (d - 0.5)                                              # :42
        sel = cnt > 0
        terms = torch.zeros(n, dtype=dtype)
        terms[sel] = cnt[sel] * reward[sel] * logp[sel] * (p[sel] / qq[sel])  # :205-210, choose_IS not detached
        loss = -terms.sum() / K
        loss.backward()
        out["loss_q"][q] = float(loss.detach())
        out["grad"][q, :n] = g.grad.double().numpy()
        if dtype != torch.float64:
            continue
        # ---- bounds (float64 only)
        zz, pp, lp, qn = z.detach().numpy(), p.detach().numpy(), logp.detach().numpy(), qq.detach().numpy()
        cn, r, an = cnt.numpy(), reward.numpy(), a.numpy()
        m = zz.max()
        logZ = float(np.log(np.exp(zz - m).sum()))
        dz = cu * (np.abs(zz) + abs(m) + np.abs(zz - m))
        eZ = float((pp * (dz + cu)).sum() + cu)
        E_lp = dz + eZ + cu * (abs(logZ) + np.abs(lp))
        rho = np.where(qn > 0, pp / np.where(qn > 0, qn, 1.0), 0.0)
        e_rho = 2.0 * (dz + cu) + eZ + 2.0 * cu
        floor = np.where(qn > 0, TINY / np.where(qn > 0, qn, 1.0), 0.0)      # rho's absolute floor: e_i flushed
        cr = np.abs(cn * r) / K
        t = cr * np.abs(lp) * rho
        out["E_loss_q"][q] = float((t * (2.0 * cu + e_rho) + cr * rho * E_lp + cr * np.abs(lp) * floor).sum() + cu * t.sum())
        aq = np.where(qn > 0, an / np.where(qn > 0, qn, 1.0), 0.0)
        h = -(cn * r / K) * rho * (1.0 + lp * aq)
        e_w = dz + eZ + 3.0 * cu
        E_h = (np.abs(h) * (2.0 * cu + e_rho) + cr * rho * (E_lp * aq + np.abs(lp) * aq * (e_w + 3.0 * cu)) + cr * floor * (1.0 + np.abs(lp) * aq))
        H = h.sum()
        E_H = E_h.sum() + cu * np.abs(h).sum()
        E_p = pp * (dz + eZ + 2.0 * cu) + TINY
        gr = np.abs(h) + np.abs(pp * H)
        out["E_grad"][q, :n] = (E_h + pp * E_H + abs(H) * E_p + 2.0 * cu * gr) / Tt + cu * np.abs(out["grad"][q, :n])
    out["loss"] = float(np.sum(out["loss_q"]))
    out["E_loss"] = float(np.sum(out["E_loss_q"]) + cu * np.abs(out["loss_q"]).sum())
    return out


def _sp(x):
    return np.logaddexp(0.0, x)


def _sg(x):
    return np.exp(-np.logaddexp(0.0, -x))          # relative accuracy in both tails


def selected(x, nsel, mode, d_sel=None, neg_idx=None, lens=None, T=1.0, dtype=torch.float64, c=C_IRGAN):
    """ptr_irgan_sel_fwd_bwd -> dict(loss_q, grad, valid_q, loss, E_loss_q, E_grad, E_loss); gradients from autograd on the reference's
    own expressions."""
    x_np = np.asarray(x, np.float32)
    B, W = x_np.shape
    gen = mode.startswith("PAIR_G")
    S = (neg_idx.shape[1] if gen else W // 2)
    out = dict(loss_q=np.zeros(B), grad=np.zeros((B, W)), valid_q=np.zeros(B), E_loss_q=np.zeros(B), E_grad=np.zeros((B, W)))
    Tt = float(np.float32(T))
    cu = c * U
    one, zero = torch.ones(1, dtype=dtype), torch.zeros(1, dtype=dtype)
    for q in range(B):
        V = int(min(max(int(nsel[q]), 0), S))
        if V == 0:
            continue
        out["valid_q"][q] = 1.0
        xs = torch.tensor(x_np[q], dtype=dtype, requires_grad=True)
        ds_np = np.asarray(d_sel[q] if gen else x_np[q], np.float32)
        ds = torch.tensor(ds_np, dtype=dtype) if gen else xs
        dp, dn = ds[:V], ds[V:2 * V]
        if mode == "POINT_D":                                                 # irgan_point.py:161-169
            # BCEWithLogits(x, 1) = softplus(-x), BCEWithLogits(x, 0) = softplus(x): written out, since autograd's (sigmoid(x) - label)
            # cancels in float32 where the derivative -sigmoid(-x) of the stable form does not
            loss = (torch.nn.functional.softplus(-dp).sum() + torch.nn.functional.softplus(dn).sum()) / (2 * V)
        elif mode == "PAIR_D_SVM":                                            # irgan_pair.py:182
            loss = torch.mean(torch.max(zero, one - (dp - dn)))
        elif mode == "PAIR_D_LOG":                                            # :184, log(sigmoid) as log-sigmoid
            loss = -torch.mean(torch.nn.functional.logsigmoid(dp - dn))
        else:
            if mode == "PAIR_G_SVM":                                          # :40
                reward = torch.sigmoid(torch.max(zero, one - (dp - dn)))
            else:                                                             # :42
                reward = torch.nn.functional.logsigmoid(dn - dp)
            n = _qlen(lens, q, W)
            idx = np.asarray(neg_idx[q, :V], np.int64)
            ok = torch.tensor((idx >= 0) & (idx < n))
            safe = torch.tensor(np.where((idx >= 0) & (idx < n), idx, 0))
            zz = xs[safe] if Tt == 1.0 else xs[safe] / Tt                     # :19-25 predict
            loss = -(torch.where(ok, torch.nn.functional.logsigmoid(zz) * reward.detach(), torch.zeros(V, dtype=dtype))).sum() / V   # :218
        loss.backward()
        out["loss_q"][q] = float(loss.detach())
        out["grad"][q] = xs.grad.double().numpy()
        if dtype != torch.float64:
            continue
        a, b = ds_np[:V].astype(np.float64), ds_np[V:2 * V].astype(np.float64)
        gq = np.abs(out["grad"][q])
        if mode == "POINT_D":
            t = (_sp(-a) + _sp(b)) / (2 * V)
            out["E_loss_q"][q] = 5.0 * cu * t.sum() + cu * t.sum() + V * TINY
            out["E_grad"][q] = 5.0 * cu * gq + TINY
        elif mode == "PAIR_D_SVM":
            xx = 1.0 - (a - b)
            dx = cu * (np.abs(a - b) + np.abs(xx))
            out["E_loss_q"][q] = (dx.sum() + 2.0 * cu * np.maximum(xx, 0).sum()) / V
            out["E_grad"][q] = 2.0 * cu * gq
        elif mode == "PAIR_D_LOG":
            xx = a - b
            dx = cu * np.abs(xx)
            sg = _sg(-xx)
            out["E_loss_q"][q] = (dx * sg + 5.0 * cu * _sp(-xx)).sum() / V + cu * abs(out["loss_q"][q]) + V * TINY
            e = (dx * sg * (1.0 - sg) + 5.0 * cu * sg) / V + TINY
            out["E_grad"][q, :V] = e
            out["E_grad"][q, V:2 * V] = e
        else:
            if mode == "PAIR_G_SVM":
                xx = 1.0 - (a - b)
                dx = cu * (np.abs(a - b) + np.abs(xx))
                rw = _sg(np.maximum(xx, 0.0))
                E_rw = dx * rw * (1.0 - rw) + 5.0 * cu * rw
            else:
                xx = b - a
                rw = -_sp(-xx)
                E_rw = cu * np.abs(xx) * _sg(-xx) + 5.0 * cu * np.abs(rw) + TINY
            zn = (x_np[q].astype(np.float64)[safe.numpy()]) / Tt
            dzn = cu * np.abs(zn)
            ls, sg = -_sp(-zn), _sg(-zn)
            E_ls = dzn * sg + 5.0 * cu * np.abs(ls) + TINY
            okn = ok.numpy()
            out["E_loss_q"][q] = float(((E_ls * np.abs(rw) + np.abs(ls) * E_rw + 2.0 * cu * np.abs(ls * rw)) * okn).sum() / V + cu * abs(out["loss_q"][q]))
            E_sg = dzn * sg * (1.0 - sg) + 5.0 * cu * sg + TINY
            eg = (E_sg * np.abs(rw) + sg * E_rw + 3.0 * cu * sg * np.abs(rw)) / (V * Tt)
            for k in range(V):
                if okn[k]:
                    out["E_grad"][q, idx[k]] = eg[k]
    out["loss"] = float(np.sum(out["loss_q"]))
    out["E_loss"] = float(np.sum(out["E_loss_q"]) + cu * np.abs(out["loss_q"]).sum())
    return out


def sample_probabilities(s, P, mode, T):
    """Exact law of ONE negative draw (V = 1) of each sampler mode over the documents, float64."""
    z = _z(s, T)
    if mode == "POINT_D":
        w = np.exp(z - z.max())
    elif mode == "PAIR_D":
        w = np.exp(z - z[P:].max())
        w[:P] = 0.0
    else:
        w = _sg(z)
    return w / w.sum()
