"""Restatement of the list machines' kernels (csrc/adlist.hip) in numpy / torch, from GIVEN uniforms, with gradients from autograd and
ELEMENT-WISE first-order error bounds (constant x fp32 unit round-off x what the value is built from).  The losses take a dtype: float64 is
the reference, float32 the CPU restatement whose own need sets the gate constant C_ADLIST.

Reference lines.  listwise/irgan_list.py: per_query_generation :230-291, get_reward :294-312, the discriminator's loss :336-337, the
generator's :379-391.  listwise/irfgan_list.py: :295, :322, :375.  util/list_probability.py:24-30 (Plackett-Luce), :44-62 (Bradley-Terry).
util/list_sampling.py:16-36 (gumbel_softmax), :70-87 (arg_shuffle_ties).

Sampling rules (include/ptranking_amd.h).  Generated rankings: the order (preds_i + gumbel(u(s, i)) descending, index ascending); PINNED by
float64 when no two keys of a list lie within KEY_GAP = 1e-4 of each other (the fp32 keys carry a few 2^-24 (1 + |g| + |key|)).  Standard
rankings: (label descending, u(S + s, i) descending, index ascending) — labels and uniforms are compared exactly (multiples of 2^-24), so
they are always pinned.  Top Kq = min(top_k, n) positions, 0 beyond; kq = 0 for an empty list or a NaN score.

Error model of the losses, u = 2^-24, c the family constant, cu = c u.
  lp_PL   thread t owns ceil(K / G) consecutive positions; a suffix scan of log-sum-exp steps (lse2: a subtraction, exp, log1p, an
          addition: cu (|value| + 3) absolute per step, and a step passes the errors of its inputs on with weights that sum to 1), NSTEP(K) =
          ceil(K / 64) + 10 steps at most on any path (in-thread chain, wave scan of depth 6, up to 4 wave totals); then per position
          (v_p - m) - lam_p, summed in-thread and by a butterfly: NSTEP cu sum |terms|.  The gradient 1 - exp((v_r - m) + LQ_r) with LQ_r
          the prefix log-sum-exp of -lam_p: the same chain again on top of max E_lam.  (This is the kernel's fp32 log-domain path, taken
          beyond a spread of 600; below it the kernel runs both scans in double and stays far inside the same bound.)
  lp_BT   per pair z = v_p - v_r (cu |z|), log sigmoid(z) 4 cu |.| + sigmoid(-z) cu |z|, sigmoid 4 cu; a chain of K additions per position
          (K cu sum |terms| of that position), then the butterfly over positions (NSTEP cu sum |terms|).
  D       IRGAN: -lp_std exact in lp, -log1p(-lp_gen): E_lp / (1 - lp) + 2 cu |.|; the 2 S terms are added one after the other: 2 S cu
          sum |terms|.  IRFGAN: a(lp), c(lp) with the bounds of tests/irfgan_ref.py fdiv(), lp's error through a', c' (a'', c'' for the
          coefficients).  A document's gradient: sum over the rankings that name it of coef x D_p, each product 2 cu, the additions 2 S cu.
  G       key = x + g (cu |key| + E_g), z = (key - m) / T, y = exp(z - log Z) through the log-softmax (irfgan_ref's model of it); A =
          lp_PL(y_top) carries its own roundings plus sum |h_p| E_y_p, h its gradient plus 2 (1 - h_r) max E_y (the row sums of |dh/dy|);
          R carries the reward's AMPLIFICATION of the error of the discriminator's lp: |R| E_lp for the exponential forms, E_lp for -lp,
          E_lp / (1 - lp) for log(1 - lp), |c'| E_lp under IRFGAN.  loss = mean A R; grad_j = sum_s c_s (y_j h_j - y_j H_s), c_s = +-R_s /
          (S T), H_s = sum_p y_p h_p.
Every quantity built on an exponential carries the absolute floor 2^-126 times its cofactor."""
import math

import numpy as np
import torch

from f64_loss_bounds import gumbel as gumbel_E
from irfgan_ref import F_DIVS, act, conj, fdiv
from irgan_ref import KEY_GAP, TINY, U, _qlen

MODES = {"D": 0, "G": 1}
PROBS = {"PL": 0, "BT": 1}
FAMILIES = {"IRGAN": 0, "IRFGAN": 1}
REWARDS = {"neg_exp": 0, "neg_lp": 1, "exp_1m": 2, "log_1m": 3}
F32_MAX = 3.0e38
# The gate constant by the project's rule for C_METRIC: the need of the float32 CPU restatement on the GPU test's cases (c = 1), doubled,
# rounded up to a half, capped at 4: the float32 restatement needs 0.33, hence 1.0 (the kernels on the MI355X need 0.14).
# tests/test_adlist_cpu.py::test_gate_constant_follows_the_fp32_restatement recomputes it.
C_ADLIST = 1.0


def kq_of(top_k, n):
    return n if top_k is None or top_k <= 0 else min(int(top_k), n)


def kw_of(top_k, L):
    return L if top_k is None or top_k <= 0 else int(top_k)


# ------------------------------------------------------------------------------------------------------------- the sampler
def gen_order(preds_row, unif_row):
    """(the order of preds + gumbel, pinned?) for one list and one sample, float64 on the fp32 inputs."""
    g, _ = gumbel_E(unif_row)
    key = np.asarray(preds_row, np.float32).astype(np.float64) + g
    pi = np.lexsort((np.arange(key.size), -key))
    srt = key[pi]
    return pi, bool(key.size < 2 or np.min(srt[:-1] - srt[1:]) > KEY_GAP)


def std_order(labels_row, unif_row):
    y, u = np.asarray(labels_row, np.float64), np.asarray(unif_row, np.float64)
    return np.lexsort((np.arange(y.size), -u, -y))


def sample(preds, labels, lens, S, top_k, unif):
    """ptr_adlist_sample -> (std_idx, gen_idx int64 [B, S, Kw], kq int32 [B], pinned bool [B]).  unif fp32 [B, 2 S, L]."""
    preds, labels, unif = np.asarray(preds, np.float32), np.asarray(labels, np.float32), np.asarray(unif, np.float32)
    B, L = preds.shape
    Kw = kw_of(top_k, L)
    std, gen = np.zeros((B, S, Kw), np.int64), np.zeros((B, S, Kw), np.int64)
    kq, pinned = np.zeros(B, np.int32), np.ones(B, bool)
    for q in range(B):
        n = _qlen(lens, q, L)
        if n == 0 or np.isnan(preds[q, :n]).any():
            continue
        K = kq[q] = kq_of(top_k, n)
        for s in range(S):
            pi, ok = gen_order(preds[q, :n], unif[q, s, :n])
            pinned[q] &= ok
            gen[q, s, :K] = pi[:K]
            std[q, s, :K] = std_order(labels[q, :n], unif[q, S + s, :n])[:K]
    return std, gen, kq, pinned


# ------------------------------------------------------------------------------------------------------------- ranking probabilities
def lp_torch(prob, v):
    """log_ranking_prob_Plackett_Luce / _Bradley_Terry of util/list_probability.py for one ranking v [K] (the BT through log-sigmoid: the
    reference's e_p / (e_p + e_r) after a max shift is the same number)."""
    if prob == "PL":
        lcse = torch.flip(torch.logcumsumexp(torch.flip(v, dims=[0]), dim=0), dims=[0])    # listmle.py apply_LogCumsumExp
        return torch.sum(v - lcse)
    K = v.numel()
    if K < 2:
        return (v * 0.0).sum()
    z = v[:, None] - v[None, :]
    return torch.sum(torch.triu(torch.nn.functional.logsigmoid(z), diagonal=1))


def nstep(K):
    return math.ceil(K / 64) + 10


def lp_bounds(prob, v, cu):
    """float64 (lp, D = d lp / d v, E_lp, E_D, W = sum_j |d D_r / d v_j| bound per position) for the ranking v [K]."""
    v = np.asarray(v, np.float64)
    K = v.size
    N = nstep(K)
    if prob == "PL":
        m = v.max()
        b = v - m
        lam = np.logaddexp.accumulate(b[::-1])[::-1]
        t = b - lam
        big = np.maximum.accumulate(np.abs(lam)[::-1])[::-1]                  # the largest partial of a suffix scan ending at p
        E_lam = np.minimum(np.arange(K, 0, -1), N) * cu * (big + np.abs(b).max() + 3.0)
        E_lp = float((cu * np.abs(b) + E_lam + cu * np.abs(t)).sum() + N * cu * np.abs(t).sum())
        LQ = np.logaddexp.accumulate(-lam)
        a = b + LQ
        w = np.exp(a)
        bigq = np.maximum.accumulate(np.abs(LQ))
        E_LQ = np.maximum.accumulate(E_lam) + np.minimum(np.arange(1, K + 1), N) * cu * (bigq + np.abs(lam).max() + 3.0)
        E_D = w * (cu * np.abs(b) + E_LQ + cu * np.abs(a) + 2.0 * cu) + cu * np.abs(1.0 - w) + TINY
        return float(t.sum()), 1.0 - w, E_lp, E_D, 2.0 * w
    z = v[:, None] - v[None, :]
    ls, sg, sgn = -np.logaddexp(0.0, -z), np.exp(-np.logaddexp(0.0, -z)), np.exp(-np.logaddexp(0.0, z))
    up = np.triu(np.ones((K, K), bool), 1)
    E_ls = cu * np.abs(z) * sgn + 4.0 * cu * np.abs(ls) + TINY
    rows = (np.abs(ls) * up).sum(1)
    E_lp = float((E_ls * up).sum() + K * cu * rows.sum() + N * cu * rows.sum())
    D = (sgn * up).sum(1) - (sg * up.T).sum(1)
    E_s = cu * np.abs(z) * sg * sgn + 4.0 * cu * np.where(up, sgn, sg) + TINY
    off = up | up.T
    E_D = (E_s * off).sum(1) + K * cu * (np.where(up, sgn, sg) * off).sum(1) + TINY
    return float((ls * up).sum()), D, E_lp, E_D, 2.0 * (sg * sgn * off).sum(1)


def reward_torch(family, reward, f_div, lp):
    if family == "IRFGAN":
        return conj(f_div, lp, "stable")
    if reward == "neg_exp":
        return -torch.exp(lp)
    if reward == "neg_lp":
        return -lp
    if reward == "exp_1m":
        return torch.exp(1.0 - lp)
    return torch.log(1.0 - lp)


def reward_bounds(family, reward, f_div, lp, E_lp, cu):
    """(R, E_R): the reward in float64 and its bound, carrying the amplification of lp's error."""
    if family == "IRFGAN":
        _, (cc, dc, d2c, Ec, Edc) = fdiv(f_div, np.float64(lp))
        return float(cc), float(cu * Ec + abs(dc) * E_lp + TINY)
    if reward == "neg_exp":
        R = -math.exp(lp)
        return R, abs(R) * (E_lp + 2.0 * cu) + TINY
    if reward == "neg_lp":
        return -lp, E_lp
    if reward == "exp_1m":
        R = math.exp(min(1.0 - lp, 700.0))
        return R, abs(R) * (E_lp + cu * abs(1.0 - lp) + 2.0 * cu) + TINY
    R = math.log1p(-lp)
    return R, E_lp / (1.0 - lp) + 2.0 * cu * abs(R) + TINY


# ------------------------------------------------------------------------------------------------------------- the losses
def loss(x, mode, prob="PL", family="IRGAN", reward="exp_1m", f_div="KL", std_idx=None, gen_idx=None, kq=None, d_preds=None, S=None, top_k=None,
         T=1.0, unif=None, lens=None, dtype=torch.float64, c=None, bounds=True):
    """ptr_adlist_fwd_bwd -> dict(loss_q, grad, valid_q, inrange [B] bool (every float64 value inside fp32 range), loss, E_loss_q, E_grad,
    E_loss, and under 'G' gen_idx [B, S, Kw], pinned [B]).  unif fp32 [B, S, L] ('G')."""
    c = C_ADLIST if c is None else c
    cu = c * U
    x_np = np.asarray(x, np.float32)
    B, L = x_np.shape
    gen = mode == "G"
    if not gen:
        S = std_idx.shape[1]
    Kw = kw_of(top_k, L) if gen else std_idx.shape[2]
    out = dict(loss_q=np.zeros(B), grad=np.zeros((B, L)), valid_q=np.zeros(B), E_loss_q=np.zeros(B), E_grad=np.zeros((B, L)), inrange=np.ones(B, bool))
    if gen:
        out["gen_idx"], out["pinned"] = np.zeros((B, S, Kw), np.int64), np.ones(B, bool)
    tf = float(np.float32(T))
    sgn = -1.0 if family == "IRFGAN" else 1.0
    for q in range(B):
        n = _qlen(lens, q, L)
        if gen:
            K = 0 if n == 0 or np.isnan(x_np[q, :n]).any() else kq_of(top_k, n)
        else:
            K = int(min(max(int(kq[q]), 0), n, Kw))
            if K and not ((std_idx[q, :, :K] >= 0) & (std_idx[q, :, :K] < n) & (gen_idx[q, :, :K] >= 0) & (gen_idx[q, :, :K] < n)).all():
                K = 0
        if K == 0:
            continue
        out["valid_q"][q] = 1.0
        xs = torch.tensor(x_np[q, :n], dtype=dtype, requires_grad=True)
        xd = x_np[q, :n].astype(np.float64)
        Eg, terms, big = np.zeros(n), 0.0, 0.0
        if not gen:
            ls = torch.zeros((), dtype=dtype)
            El = 0.0
            for s in range(S):
                for which, idx in ((0, std_idx), (1, gen_idx)):
                    pi = np.asarray(idx[q, s, :K], np.int64)
                    lp = lp_torch(prob, xs[torch.tensor(pi)])
                    if family == "IRFGAN":                                    # irfgan_list.py:322
                        ls = ls + (conj(f_div, lp, "stable") if which else -act(f_div, lp, "stable")) / S
                    else:                                                     # irgan_list.py:336-337
                        ls = ls - (torch.log(1.0 - lp) if which else lp)
                    if not bounds or dtype != torch.float64:
                        continue
                    lpv, D, E_lp, E_D, _ = lp_bounds(prob, xd[pi], cu)
                    if family == "IRFGAN":
                        (a, da, d2a, Ea, Eda), (cc, dc, d2c, Ec, Edc) = fdiv(f_div, np.float64(lpv))
                        val, dv, d2v, Ev, Edv = (cc, dc, d2c, Ec, Edc) if which else (a, da, d2a, Ea, Eda)
                        big = max(big, abs(float(val)))
                        term, E_term = abs(float(val)) / S, (cu * Ev + abs(dv) * E_lp) / S + 2.0 * cu * abs(float(val)) / S
                        coef, E_coef = abs(float(dv)) / S, (cu * Edv + d2v * E_lp) / S + 2.0 * cu * abs(float(dv)) / S
                    elif which:
                        term, E_term = math.log1p(-lpv), E_lp / (1.0 - lpv) + 2.0 * cu * math.log1p(-lpv)
                        coef = 1.0 / (1.0 - lpv)
                        E_coef = coef * coef * E_lp + 2.0 * cu * coef
                    else:
                        term, E_term, coef, E_coef = abs(lpv), E_lp, 1.0, 0.0
                    terms += term
                    El += E_term
                    Eg[pi] += E_coef * np.abs(D) + coef * E_D + (2.0 + 2.0 * S) * cu * coef * np.abs(D) + TINY
            out["E_loss_q"][q] = El + 2.0 * S * cu * terms + TINY
            out["E_grad"][q, :n] = Eg
        else:
            dn = np.asarray(d_preds, np.float32)[q, :n].astype(np.float64)
            dt = torch.tensor(dn, dtype=dtype)
            ls = torch.zeros((), dtype=dtype)
            El = 0.0
            for s in range(S):
                pi, ok = gen_order(x_np[q, :n], np.asarray(unif, np.float32)[q, s, :n])
                out["pinned"][q] &= ok
                out["gen_idx"][q, s, :K] = pi[:K]
                g64, Egum = gumbel_E(np.asarray(unif, np.float32)[q, s, :n])
                top = torch.tensor(pi[:K])
                y = torch.softmax((xs + torch.tensor(g64, dtype=dtype)) / T, dim=0)       # list_sampling.py:29-33
                A = lp_torch("PL", y[top])                                    # irgan_list.py:379: the PL of the probabilities
                with torch.no_grad():
                    lpd = lp_torch(prob, dt[top])
                    R = reward_torch(family, reward, f_div, lpd)
                ls = ls + sgn * A * R / S                                     # :391, irfgan_list.py:375
                # ---- float64 values for the range check and the bounds
                key = xd + g64
                mk = key.max()
                z = (key - mk) / tf
                logZ = float(np.log(np.exp(z).sum()))
                yv = np.exp(z - logZ)
                lpdv, _, E_lpd, _, _ = lp_bounds(prob, dn[pi[:K]], cu)
                Rv, E_R = reward_bounds(family, reward, f_div, lpdv, E_lpd, cu)
                big = max(big, abs(Rv))
                if not bounds or dtype != torch.float64:
                    continue
                E_key = cu * np.abs(key) + cu * Egum
                E_z = (E_key + E_key[np.argmax(key)] + cu * np.abs(key - mk)) / tf + cu * np.abs(z)
                eZ = float((yv * (E_z + 2.0 * cu)).sum() + (math.ceil(n / 64) + 8) * cu)
                E_y = yv * (E_z + eZ + 2.0 * cu * abs(logZ) + cu * np.abs(z - logZ) + 2.0 * cu) + TINY
                Av, h, E_A, E_h, Wh = lp_bounds("PL", yv[pi[:K]], cu)
                Ey_top = E_y[pi[:K]]
                E_A += float((np.abs(h) * Ey_top).sum())
                E_h = E_h + Wh * Ey_top.max()
                yt = yv[pi[:K]]
                yh = yt * h
                E_yh = Ey_top * np.abs(h) + yt * E_h + cu * np.abs(yh)
                H = float(yh.sum())
                E_H = float(E_yh.sum() + nstep(K) * cu * np.abs(yh).sum())
                cs = abs(Rv) / (S * tf)
                E_c = E_R / (S * tf) + 3.0 * cu * cs
                El += (E_A * abs(Rv) + abs(Av) * E_R + 3.0 * cu * abs(Av * Rv)) / S
                terms += abs(Av * Rv) / S
                mag = yv * abs(H)
                mag[pi[:K]] += np.abs(yh)
                e = E_c * mag + cs * (E_y * abs(H) + yv * E_H) + (3.0 + 2.0 * S) * cu * cs * mag
                e[pi[:K]] += cs * E_yh
                Eg += e + TINY
            out["E_loss_q"][q] = El + S * cu * terms + TINY
            out["E_grad"][q, :n] = Eg
        ls.backward()
        out["grad"][q, :n] = xs.grad.double().numpy()
        out["loss_q"][q] = float(ls.detach())
        vals = np.concatenate([[out["loss_q"][q], big], out["grad"][q, :n]])
        out["inrange"][q] = bool(np.isfinite(vals).all() and np.abs(vals).max() < F32_MAX)
    keep = out["inrange"]
    out["loss"] = float(np.sum(out["loss_q"][keep]))
    out["E_loss"] = float(np.sum(out["E_loss_q"][keep]) + cu * np.abs(out["loss_q"][keep]).sum())
    return out
