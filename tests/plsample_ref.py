"""Float64 restatement of the device Plackett-Luce sampler and the multi-sample MDPRank loss (csrc/plsample.hip), from GIVEN uniforms, with
ELEMENT-WISE error bounds in the form of tests/f64_loss_bounds.py (constant x fp32 unit round-off x sum of absolute terms), plus the
counter hash of ptr_pl_uniforms restated with numpy integers.

Sampler (ptranking/ltr_adhoc/util/sampling_utils.py:31-81, ltr_adversarial/util/list_sampling.py:38-67): g = -log(-log(u + 1e-20) + 1e-20),
key = s / T + g ('PL'; s itself at T == 1) or s + g ('STPL'), ranking = (key descending, index ascending).  action = the raw scores in sampled
order ('PL') or (s + g) / T in sampled order ('STPL', no division at T == 1).  A ranking is only PINNED by float64 when no two adjacent
sorted keys are closer than the fp32 evaluation can move them: `gap_ok` demands a gap above 2^-16 max|key| (the device's keys carry a few
2^-24 (1 + |g| + |key|)); the tests redraw a list that violates it.

Loss per sampled ranking (ptranking/ltr_adhoc/listwise/mdprank.py:45-71), a = action by position, m = max a:
    r_t = (2^l - 1) / log2(2 + t) (t < top_k),  R_t = sum_{t' >= t} r_t',  w_t = gamma^(t+1) R_t,  T_t = sum_{j >= t} e^(a_j - m)
    loss = sum_{t < top_k} w_t ((log T_t + m) - a_t);   d loss / d a_j = e_j sum_{t <= min(j, top_k - 1)} w_t / T_t - [j < top_k] w_j
with d a / d s = 1 ('PL': T only shapes the draw) or 1 / T ('STPL').  loss_q and grad are the means over the S samples.
Error model as listmle_query's: exp / log / the discount / the power cost c u relative, the cumulative sums are chains (sqrt of their length),
the STPL action carries c u ((1 + |g|) + |s + g|) / T + c u |a| (stlistnet_query), which reaches e^(a - m) as a relative error and the loss
term absolutely through w.  The mean over S adds c u sum |terms| / S.  A list with a NaN score is NaN: its loss and every gradient element
of its real documents (bound 0); padded slots are exactly 0; n = 0 gives 0.  Every gradient term carries the absolute floor 2^-126 (F32_TINY of
f64_loss_bounds: below it an fp32 value is flushed or has lost its relative accuracy; a document 100 units below the maximum has a true
gradient of 1e-44 and less).
"""
import numpy as np

from f64_loss_bounds import C_LIST, F32_TINY, U, _f64, _gain, _qlen, gumbel

DIST = {"PL": 0, "STPL": 1}
GAP = 2.0 ** -16
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------- uniforms
def _lowbias32(x):
    x = x.astype(np.uint64) & M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def uniforms_host(B, L, S, seed, q0=0):
    """ptr_pl_uniforms on the host, bit for bit: float32 [B, S, L], multiples of 2^-24 in [0, 1)."""
    seed = int(seed) & (2 ** 64 - 1)
    lo, hi = np.uint64(seed & M32), np.uint64(seed >> 32)
    qg = (np.arange(B, dtype=np.int64) + np.int64(q0)).astype(np.uint64)
    qlo, qhi = qg & np.uint64(M32), qg >> np.uint64(32)
    mul = lambda a, c: (a * np.uint64(c)) & np.uint64(M32)
    ka_q = _lowbias32(lo ^ _lowbias32((hi + mul(qlo, 0x9E3779B1) + mul(qhi, 0xC2B2AE3D)) & np.uint64(M32)))
    kb_q = _lowbias32(hi ^ _lowbias32((lo + mul(qlo, 0x85EBCA77) + mul(qhi, 0x27D4EB2F) + np.uint64(0x68E31DA4)) & np.uint64(M32)))
    s = np.arange(S, dtype=np.uint64)
    ka = _lowbias32((ka_q[:, None] + mul(s, 0xC2B2AE3D)[None, :]) & np.uint64(M32))
    kb = _lowbias32((kb_q[:, None] + mul(s, 0x9E3779B1)[None, :]) & np.uint64(M32))
    i = np.arange(L, dtype=np.uint64)
    h = _lowbias32((ka[:, :, None] + mul(i, 0x85EBCA77)[None, None, :]) & np.uint64(M32))
    t = ((h ^ kb[:, :, None]) * np.uint64(0x2C1B3C6D)) & np.uint64(M32)
    return ((t >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------- sampler
def keys_f64(s, unif, temperature, dist):
    """(key, g, E_g / (c u)) in float64 from fp32 scores and uniforms."""
    s = _f64(s)
    g, Eg = gumbel(unif)
    t = float(np.float32(temperature))
    if DIST[dist] == 0:
        return (s if t == 1.0 else s / t) + g, g, Eg
    return s + g, g, Eg


def gap_ok(key):
    """No two adjacent sorted keys closer than 2^-16 max|key| (n <= 1: trivially)."""
    key = np.asarray(key, dtype=np.float64)
    if key.size <= 1:
        return True
    srt = -np.sort(-key)
    return bool(np.min(srt[:-1] - srt[1:]) > GAP * np.max(np.abs(key)))


def order(key):
    """(key descending, index ascending)."""
    key = np.asarray(key, dtype=np.float64)
    return np.lexsort((np.arange(key.size), -key))


def sample(preds, unif, lens=None, temperature=1.0, dist="PL", c=C_LIST):
    """perm int64 [B, S, L], action float64 [B, S, L], ok bool [B, S] (the gap condition), E_action [B, S, L] (0 under 'PL': the raw
    scores, exactly).  preds [B, L] fp32, unif [B, S, L] fp32."""
    preds, unif = np.asarray(preds), np.asarray(unif)
    B, L = preds.shape
    S = unif.shape[1]
    perm = np.tile(np.arange(L, dtype=np.int64), (B, S, 1))
    act, Eact = np.zeros((B, S, L)), np.zeros((B, S, L))
    ok = np.ones((B, S), dtype=bool)
    t = float(np.float32(temperature))
    for q in range(B):
        n = _qlen(lens, q, L)
        if n == 0:
            continue
        if np.isnan(preds[q, :n]).any():
            act[q, :, :n] = np.nan
            continue
        for k in range(S):
            key, _, Eg = keys_f64(preds[q, :n], unif[q, k, :n], temperature, dist)
            pi = order(key)
            ok[q, k] = gap_ok(key)
            perm[q, k, :n] = pi
            if DIST[dist] == 0:
                act[q, k, :n] = _f64(preds[q, :n])[pi]
            else:
                z = key if t == 1.0 else key / t
                act[q, k, :n] = z[pi]
                Eact[q, k, :n] = ((c * U * Eg + c * U * np.abs(key)) / t + c * U * np.abs(z))[pi]
    return perm, act, ok, Eact


# ---------------------------------------------------------------------------------------------------------------------------- loss
def episode(a, Ea, y_pi, top_k, gamma, c):
    """One sampled ranking: a = action by position (float64), Ea its absolute error, y_pi the labels by position.  Returns loss, E_loss,
    d loss / d a by position, its bound."""
    n = a.size
    top = n if (top_k is None or top_k <= 0 or top_k > n) else int(top_k)
    k = np.arange(n, dtype=np.float64)
    im = int(np.argmax(a))
    m, Em = a[im], Ea[im]
    du = a - m
    e = np.exp(du)
    Ee = e * (c * U * (1.0 + np.abs(du)) + Ea + Em)
    T = np.cumsum(e[::-1])[::-1]
    E_T = np.cumsum(Ee[::-1])[::-1] + c * U * np.sqrt(np.maximum(1.0, n - k)) * T
    cut = k < top
    r = np.where(cut, _gain(y_pi) / np.log2(2.0 + k), 0.0)
    E_r = 2.0 * c * U * np.abs(r)
    R = np.cumsum(r[::-1])[::-1]
    E_R = np.cumsum(E_r[::-1])[::-1] + c * U * np.sqrt(np.maximum(1.0, top - k)) * np.abs(R)
    gp_ = np.ones(n) if gamma == 1.0 else float(np.float32(gamma)) ** (k + 1.0)
    w = np.where(cut, R * gp_, 0.0)
    E_w = np.where(cut, E_R * gp_ + 2.0 * c * U * np.abs(w), 0.0)
    lt = np.log(T)
    br = (lt + m) - a
    l = w * br
    E_br = E_T / T + c * U * (np.abs(lt) + np.abs(lt + m) + np.abs(br)) + Ea + Em
    E_l = np.abs(w) * E_br + E_w * np.abs(br) + c * U * np.abs(l)
    loss = l.sum()
    E_loss = E_l.sum() + c * U * np.abs(l).sum()
    x = w / T
    E_x = E_w / T + np.abs(x) * (E_T / T + c * U)
    P = np.cumsum(x)
    E_P = np.cumsum(E_x) + c * U * np.sqrt(k + 1.0) * np.cumsum(np.abs(x))
    g = e * P - w
    E_g = Ee * np.abs(P) + e * E_P + c * U * (np.abs(e * P) + np.abs(g)) + E_w + F32_TINY     # an fp32 result below 2^-126 has no relative accuracy
    return loss, E_loss, g, E_g


def mdprank_sampled(preds, labels, unif, lens=None, top_k=10, gamma=1.0, temperature=1.0, dist="PL", c=C_LIST, perm=None):
    """The multi-sample loss from given uniforms (perm: use these rankings instead of sorting the float64 keys).  Returns
    dict(q, loss_q, E_loss_q, grad, E_grad, perm, ok, loss_s [B, S])."""
    preds, labels, unif = np.asarray(preds), np.asarray(labels), np.asarray(unif)
    B, L = preds.shape
    S = unif.shape[1]
    t = float(np.float32(temperature))
    inv_t = 1.0 / t
    lq, Elq = np.zeros(B), np.zeros(B)
    gr, Egr = np.zeros((B, L)), np.zeros((B, L))
    pm = np.tile(np.arange(L, dtype=np.int64), (B, S, 1))
    ok = np.ones((B, S), dtype=bool)
    ls = np.zeros((B, S))
    for q in range(B):
        n = _qlen(lens, q, L)
        if n == 0:
            continue
        if np.isnan(preds[q, :n]).any():
            lq[q] = np.nan
            gr[q, :n] = np.nan
            ls[q] = np.nan
            continue
        s, y = _f64(preds[q, :n]), _f64(labels[q, :n])
        acc, Eacc, aabs = np.zeros(n), np.zeros(n), np.zeros(n)
        Els = np.zeros(S)
        for k in range(S):
            key, g, Eg = keys_f64(preds[q, :n], unif[q, k, :n], temperature, dist)
            ok[q, k] = gap_ok(key)
            pi = order(key) if perm is None else np.asarray(perm[q, k, :n], dtype=np.int64)
            pm[q, k, :n] = pi
            if DIST[dist] == 0:
                a, Ea, sc = s[pi], np.zeros(n), 1.0
            else:
                z = key if t == 1.0 else key * inv_t
                Ez = (c * U * Eg + c * U * np.abs(key)) * inv_t + c * U * np.abs(z)
                a, Ea, sc = z[pi], Ez[pi], (1.0 if t == 1.0 else inv_t)
            ls[q, k], Els[k], gp, E_gp = episode(a, Ea, y[pi], top_k, gamma, c)
            gp, E_gp = gp * sc, E_gp * sc + (0.0 if sc == 1.0 else c * U * np.abs(gp * sc))
            acc[pi] += gp
            Eacc[pi] += E_gp
            aabs[pi] += np.abs(gp)
        lq[q] = ls[q].sum() / S
        Elq[q] = (Els.sum() + c * U * np.abs(ls[q]).sum()) / S + c * U * abs(lq[q])
        gr[q, :n] = acc / S
        Egr[q, :n] = (Eacc + c * U * aabs) / S + c * U * np.abs(gr[q, :n])
    return dict(q=np.arange(B), loss_q=lq, E_loss_q=Elq, grad=gr, E_grad=Egr, perm=pm, ok=ok, loss_s=ls)


def redraw(preds, unif, lens, temperature, dist, seed=0):
    """Make every (query, sample) satisfy the gap condition, in place: while two adjacent sorted float64 keys are closer than the gap, the
    uniform of the lower document of each such pair is drawn again (a whole-list redraw cannot work beyond a few hundred documents: 4096
    keys spread over ~15 units leave thousands of pairs closer than 2^-16 max|key| ~ 2e-4 in every draw).  Returns the number of
    (query, sample) lists touched and the number of uniforms drawn again."""
    g = np.random.default_rng(seed)
    B, L = preds.shape
    S = unif.shape[1]
    lists = draws = 0
    for q in range(B):
        n = _qlen(lens, q, L)
        if n < 2 or np.isnan(preds[q, :n]).any():
            continue
        for k in range(S):
            touched = False
            for _ in range(400):
                key = keys_f64(preds[q, :n], unif[q, k, :n], temperature, dist)[0]
                o = order(key)
                srt = key[o]
                close = np.nonzero(~(srt[:-1] - srt[1:] > GAP * np.max(np.abs(key))))[0]
                if close.size == 0:
                    break
                docs = np.unique(o[close + 1])
                unif[q, k, docs] = (g.integers(0, 2 ** 24, size=docs.size).astype(np.float64) * 2.0 ** -24).astype(np.float32)
                draws += docs.size
                touched = True
            else:
                raise AssertionError(f"query {q} sample {k}: no draw with separated keys")
            lists += int(touched)
    return lists, draws


def pl_probabilities(s, temperature=1.0):
    """Exact Plackett-Luce probability of each of the n! rankings of scores s (weights exp(s / T)), keyed by the ranking tuple: the law of
    torch.multinomial's sequential draw without replacement."""
    import itertools
    w = np.exp(_f64(s) / temperature)
    out = {}
    for pi in itertools.permutations(range(len(w))):
        p, rest = 1.0, w.sum()
        for i in pi:
            p *= w[i] / rest
            rest -= w[i]
        out[pi] = p
    return out
