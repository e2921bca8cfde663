"""Float64 restatement, ELEMENT-WISE error bounds and input builders for the evaluation kernels (csrc/metrics.hip: ptr_sort_desc and
ptr_metrics_at_ks, i.e. the Evaluator prologue + nDCG / nERR / AP / P at cut-offs).  The gate itself is f64_bounds.gate.

Why: every number the project reports (validation nDCG@k, adhoc_performance_at_ks, model selection, the benchmark's metric_path) comes out
of these kernels, and they were compared only against fp32 (the C oracle, the reference's own outputs) under golden_util.assert_close, on
inputs that always held a relevant document, never a NaN score and no cut-off beyond 100.  Here every element of every metric gets a bound
of its own, computed in float64 from the very fp32 inputs the kernel saw.

The restatement (`metrics`, `sort_desc`) follows ptranking/base/ranker.py:46-60 and ptranking/metric/adhoc/adhoc_metric.py:36-260 per query
of a padded batch (list length n = lens[q], L without lens):
  * predicted order: score descending, original index ascending on equal scores, and NaN scores FIRST, in index order — what
    torch.sort(descending=True, stable=True) returns.  -0.0 and +0.0 compare equal;
  * ideal order: the labels sorted descending, or as given under `presort`;
  * the cut-offs with 1 <= k <= n are compacted to the front of the row in the order given (duplicates kept), the rest of the row is 0
    (adhoc_metric.py:255-258); a zero-length list is a row of zeros;
  * max_label=None is the maximum over the valid labels of the BATCH (adhoc_metric.py:174-177);
  * 0 / 0 stays NaN: a list without a relevant document has nDCG = nERR = AP = NaN and P = 0 at every fitting cut-off.

Error model, u = 2^-24, one constant c = C_METRIC for the family.  At rank r (0-based), label y, k = r + 1:
  gain g = 2^y - 1        exact for integer labels (v_exp_f32 and exp2f are exact on integers, and so is the difference); otherwise the
                          power carries c u relative, which the subtraction keeps as an ABSOLUTE error: E_g = c u 2^y.  Permutation
                          labels are their own gain: exact
  discount d = 1/log2(r+2)  c u relative
  every prefix sum of terms t_0 .. t_r carries c u (sum |t| - |t_0|) on top of its terms' own errors: r additions, each rounding at most
                          u times a partial sum of |terms|; the prefix of ONE term is that term (written S|t| below)
  DCG = prefix sum of t = g d:   E_t = c u |t| + E_g d,   E_DCG = sum E_t + c u S|t|
  rel = clip(y, 0, 1), cumrel = prefix sum: a sum of integers below 2^24 is EXACT (integer labels); otherwise c u S|rel|
  prec = cumrel / k        the kernel claims a correctly rounded quotient: u |prec| + E_cumrel / k
  AP numerator = prefix sum of prec rel: E = sum (E_prec rel + c u |prec rel|) + c u S|prec rel|; its denominator, the prefix sum of the
                          GRADED ideal labels, is exact for integer labels (below 2^24) and carries c u S|y| otherwise
  sat = g / 2^max_label    integer max_label: the divisor is a power of two, E_sat = E_g / 2^max_label; otherwise the power and the
                          quotient each cost c u: E_sat = E_g / 2^max_label + 2 c u |sat|
  1 - sat                  E = E_sat + c u (absolute)
  cascade = EXCLUSIVE prefix product of (1 - sat):  a product of k factors carries c u k relative plus the factors' own relative errors
  ERR = prefix sum of e = sat cascade / k:  E_e = (E_sat |cascade| + |sat| E_cascade) / k + c u |e|,  E_ERR = sum E_e + c u S|e|
  every metric is a quotient a / b:  E = (E_a + |a / b| E_b) / |b| + c u |a / b|
Exact results (E = 0): P@k and the rank-wise precision wherever the clipped labels are integers — the expected value is
np.float32(cumrel / k) BIT FOR BIT, no bound (`p_exact`); with fractional labels cumrel itself is a rounded sum and P carries
E_cumrel / k + u P; cut-offs beyond the list are exactly 0; NaN appears exactly where the restatement has NaN and nowhere else
(`gate_nan`).

The input builders below are imported by the CPU tests (tests/test_metrics_cpu.py: the restatement against the reference's fixtures, the
constant measured against the fp32 references, planted faults) and by the GPU tests (tests/test_metrics_bounds_gpu.py), so what is
checked on the CPU is what the GPU sees.
"""
import math

import numpy as np
import torch

from f64_bounds import U, d64, gate

# ---- the family constant (c above).  It is set from the fp32 REFERENCES, not from the kernel: tests/test_metrics_cpu.py runs
# oracle/torch_ref.py (fp32 torch) and the C oracle (in-order fp32 sums, libm) on every input of the GPU cases A - E and records what each
# needs at c = 1; C_METRIC = 2 x the larger need, rounded up to the next half, never above 4 (the largest family constant of the losses).
# 2 x: the kernel's v_rcp_f32 / v_log_f32 are 1-ulp (2 u) where those references divide and call libm, and its scans are log-depth.
NEED_TORCH_REF = 0.57    # fp32 torch (torch.cumsum / cumprod): worst over the cases A - E is nDCG, 6 x 65 graded labels; AP 0.54, nERR 0.36;
                         # flat in the list length (0.47 - 0.54 at 4096 documents)
NEED_C_ORACLE = 7.80     # the C oracle: nDCG at k = 4096 .. 8192 of 4096 documents (6.52 up to 2049, 3.53 up to 1024: NEED_C_ORACLE_* below).  Its DCG is ONE
                         # in-order chain of 4096 additions, whose roundings add like a random walk (~sqrt(m) u sum |terms|); the kernel's
                         # longest chain is 64 chunk carries on top of a 6-step scan
C_METRIC = 4.0           # = min(4, ceil_to_half(2 x 7.80)): the cap decides.  The C oracle itself stays inside it up to 1024 documents
                         # Measured on an MI355X (tests/test_metrics_bounds_gpu.py): worst AP 1.88 (4096 documents, colliding keys), nDCG 1.45,
                         # nERR 0.68, P with fractional labels 1.87; P on integer labels is the correctly rounded quotient bit for bit
NEED_C_ORACLE_1024 = 3.53  # the C oracle over the cases of at most 1024 documents (nDCG): inside C_METRIC; 4.30 at 1025
NEED_C_ORACLE_2049 = 6.52  # ... of at most 2049 documents (nDCG at 2048)
C_CAP = 4.0


def constant_from_needs(*needs):
    return min(C_CAP, math.ceil(2.0 * max(needs) * 2.0) / 2.0)


METRICS = ("ndcg", "nerr", "ap", "p")


def _qlen(lens, q, L):
    return L if lens is None else int(min(max(int(lens[q]), 0), L))


# ---------------------------------------------------------------------------------------------------------------------------- restatement
def order_desc(s):
    """Indices of one list's scores in the predicted order: NaN first (index ascending), then score descending, index ascending."""
    s = np.asarray(s, dtype=np.float64)
    nan = np.isnan(s)
    return np.lexsort((np.arange(len(s)), -np.where(nan, 0.0, s), ~nan)).astype(np.int64)


def sort_desc(preds, lens=None):
    """(vals fp32 [B, L], idx int64 [B, L]) of ptr_sort_desc: the predicted order of each list, 0 / r on the padded slots r >= n."""
    preds = np.asarray(preds, dtype=np.float32)
    B, L = preds.shape
    vals, idx = np.zeros((B, L), np.float32), np.tile(np.arange(L, dtype=np.int64), (B, 1))
    for q in range(B):
        n = _qlen(lens, q, L)
        o = order_desc(preds[q, :n])
        idx[q, :n], vals[q, :n] = o, preds[q, :n][o]
    return vals, idx


def _quot(a, Ea, b, Eb, c):
    with np.errstate(all="ignore"):
        v = a / b
        E = (Ea + np.abs(v) * Eb) / np.abs(b) + c * U * np.abs(v)
    return v, np.where(np.isfinite(v), E, 0.0)


def _sabs(t):
    """S|t| of the module docstring: the prefix sums of |t| without the first term."""
    a = np.abs(t)
    return np.cumsum(a) - (a[0] if len(a) else 0.0)


def _is_int(y):
    return bool(np.all(y == np.floor(y)))


def query_metrics(ys, yi, m, linear_gain, max_label, c, which=METRICS):
    """Rank-wise values and bounds over ranks 0 .. m-1 of one list: ys / yi = labels in predicted / ideal order (float64 of the fp32
    inputs).  -> {name: (values [m], E [m])}, plus 'p_exact' (bool)."""
    out = {}
    r = np.arange(m, dtype=np.float64)
    ys, yi = ys[:m], yi[:m]
    cu = c * U
    ints = _is_int(ys) and _is_int(yi)

    def gain(y):
        if linear_gain:
            return y.copy(), np.zeros_like(y)
        p = np.exp2(y)
        return p - 1.0, np.where(y == np.floor(y), 0.0, cu * p)

    gs, Egs = gain(ys)
    gi, Egi = gain(yi)
    if "ndcg" in which:
        d = 1.0 / np.log2(r + 2.0)

        def dcg(g, Eg):
            t = g * d
            return np.cumsum(t), np.cumsum(cu * np.abs(t) + Eg * d) + cu * _sabs(t)
        out["ndcg"] = _quot(*dcg(gs, Egs), *dcg(gi, Egi), c)
    rel = np.clip(ys, 0.0, 1.0)
    rel_int = _is_int(rel)
    cumrel = np.cumsum(rel)
    E_cumrel = np.zeros(m) if rel_int else cu * _sabs(rel)
    prec = cumrel / (r + 1.0)
    E_prec = U * np.abs(prec) + E_cumrel / (r + 1.0)
    out["p_exact"] = rel_int
    if "p" in which:
        out["p"] = (prec, np.zeros(m) if rel_int else E_prec)
    if "ap" in which:
        pt = prec * rel
        num = np.cumsum(pt)
        E_num = np.cumsum(E_prec * rel + cu * np.abs(pt)) + cu * _sabs(pt)
        den = np.cumsum(yi)
        E_den = np.zeros(m) if (ints and float(np.abs(yi).sum()) < 2.0 ** 24) else cu * _sabs(yi)
        out["ap"] = _quot(num, E_num, den, E_den, c)
    if "nerr" in which:
        assert not linear_gain, "nERR is only defined for graded labels (adhoc_metric.py:157-164)"
        pw = 2.0 ** float(max_label)
        ml_int = float(max_label) == math.floor(float(max_label))

        def err(g, Eg):
            sat = g / pw
            E_sat = Eg / pw + (0.0 if ml_int else 2.0 * cu * np.abs(sat))
            un = 1.0 - sat
            E_un = E_sat + cu
            incl = np.cumprod(un)
            with np.errstate(all="ignore"):
                relerr = np.cumsum(np.where(un != 0.0, E_un / np.abs(un), 0.0))
            E_incl = np.abs(incl) * (cu * (r + 1.0) + relerr)
            casc = np.concatenate(([1.0], incl[:-1]))
            E_casc = np.concatenate(([0.0], E_incl[:-1]))
            e = sat * casc / (r + 1.0)
            E_e = (E_sat * np.abs(casc) + np.abs(sat) * E_casc) / (r + 1.0) + cu * np.abs(e)
            return np.cumsum(e), np.cumsum(E_e) + cu * _sabs(e)
        out["nerr"] = _quot(*err(gs, Egs), *err(gi, Egi), c)
    return out


def batch_max_label(labels, lens=None):
    labels = np.asarray(labels, dtype=np.float64)
    B, L = labels.shape
    mx = -np.inf
    for q in range(B):
        n = _qlen(lens, q, L)
        if n:
            mx = max(mx, float(labels[q, :n].max()))
    return mx


def metrics(preds, labels, lens, ks, presort=False, permutation_labels=False, max_label=None, c=None, which=METRICS, queries=None,
            orders=None):
    """The four metrics of a padded batch in float64 with their bounds: {name: [Q, nk]}, {'E_' + name: [Q, nk]}, 'p_exact' [Q] and 'q'
    (the rows restated: `queries`, default all).  nERR is left out under permutation_labels.  orders: predicted orders to use instead
    of order_desc (a list of index arrays per restated query)."""
    c = C_METRIC if c is None else c
    preds, labels = np.asarray(preds, dtype=np.float32), np.asarray(labels, dtype=np.float32)
    B, L = preds.shape
    ks = [int(k) for k in ks]
    which = tuple(m for m in which if not (permutation_labels and m == "nerr"))
    q_list = list(range(B)) if queries is None else [int(q) for q in queries]
    if "nerr" in which and max_label is None:
        max_label = batch_max_label(labels, lens)
    res = {m: np.zeros((len(q_list), len(ks))) for m in which}
    res.update({"E_" + m: np.zeros((len(q_list), len(ks))) for m in which})
    res["p_exact"] = np.ones(len(q_list), bool)
    res["q"] = np.asarray(q_list, np.int64)
    for j, q in enumerate(q_list):
        n = _qlen(lens, q, L)
        used = [k for k in ks if 1 <= k <= n]
        if not used:
            continue
        y = labels[q, :n].astype(np.float64)
        o = order_desc(preds[q, :n]) if orders is None else np.asarray(orders[j])
        yi = y if presort else -np.sort(-y, kind="stable")
        rw = query_metrics(y[o], yi, max(used), permutation_labels, max_label, c, which)
        res["p_exact"][j] = rw["p_exact"]
        ix = np.asarray(used) - 1
        for m in which:
            res[m][j, :len(used)] = rw[m][0][ix]
            res["E_" + m][j, :len(used)] = rw[m][1][ix]
    return res


# ---------------------------------------------------------------------------------------------------------------------------- gates
def gate_nan(got, ref, E, what, c=None):
    """f64_bounds.gate where the restatement is finite; where it is not (0 / 0 of a list without a relevant document) got must be the very
    same value, and NaN / inf nowhere else (gate() itself refuses a non-finite got).  Returns the worst err/E."""
    __tracebackhide__ = True
    got, ref = d64(np.asarray(got, dtype=np.float64)), d64(np.asarray(ref, dtype=np.float64))
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    E = d64(np.broadcast_to(np.asarray(E, dtype=np.float64), tuple(ref.shape)).copy())
    fin = torch.isfinite(ref)
    same = (torch.isnan(got) & torch.isnan(ref)) | (got == ref)
    bad = ~fin & ~same
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: the float64 restatement is {float(ref.reshape(-1)[i])!r} at flat index {i}, got "
                             f"{float(got.reshape(-1)[i])!r}; {int(bad.sum())} elements")
    return gate(got[fin], ref[fin], E[fin], what, c) if bool(fin.any()) else 0.0


def p_bits(ref_p):
    """The fp32 value a correctly rounded cumrel / k has."""
    return np.asarray(ref_p, dtype=np.float64).astype(np.float32)


def gate_metrics(got, ref, what, c=None):
    """Gate a kernel's (or an fp32 reference's) outputs {name: [B, nk]} against `metrics()`'s result: nDCG / nERR / AP inside their bounds
    with NaN placement exact, P bit for bit on the rows whose clipped labels are integers (inside its bound on the others).  Metrics
    missing from `got` are not judged.  Returns {name: worst err/E} (P: 0 when every row is exact)."""
    __tracebackhide__ = True
    c = C_METRIC if c is None else c
    q = ref["q"]
    worst = {}
    for m in METRICS:
        if m not in ref or got.get(m) is None:
            continue
        g = np.asarray(got[m], dtype=np.float32)[q]
        if m == "p":
            ex = ref["p_exact"]
            want = p_bits(ref["p"])
            same = g[ex].view(np.uint32) == want[ex].view(np.uint32)
            print(f"MEASURED {what} p: {int((~same).sum())} of {same.size} elements differ from the correctly rounded quotient")
            if not same.all():
                i = np.argwhere(~same)[0]
                raise AssertionError(f"{what} p: not the correctly rounded cumrel / k at row {int(np.flatnonzero(ex)[i[0]])} slot {int(i[1])}: got "
                                     f"{float(g[ex][tuple(i)])!r}, expected {float(want[ex][tuple(i)])!r}; {int((~same).sum())} elements")
            worst[m] = gate_nan(g[~ex], ref["p"][~ex], ref["E_p"][~ex], f"{what} p (fractional labels)", c) if (~ex).any() else 0.0
        else:
            worst[m] = gate_nan(g, ref[m], ref["E_" + m], f"{what} {m}", c)
    return worst


def need(got, ref):
    """max |got - ref| / E over the bounded elements of every metric `got` holds, for a `ref` computed at c = 1: the constant `got` needs."""
    w = 0.0
    for m in ("ndcg", "nerr", "ap"):
        if m in ref and got.get(m) is not None:
            g, r, E = np.asarray(got[m], np.float64)[ref["q"]], ref[m], ref["E_" + m]
            ok = np.isfinite(r) & (E > 0)
            if ok.any():
                w = max(w, float((np.abs(g - r)[ok] / E[ok]).max()))
    return w


# ---------------------------------------------------------------------------------------------------------------------------- data
MIXES = {"mslr": [0.5, 0.3, 0.13, 0.05, 0.02], "yahoo": [0.25, 0.35, 0.25, 0.1, 0.05]}      # the mixes of f64_loss_bounds.labels_like
LABEL_KINDS = ("mslr", "yahoo", "binary", "perm", "frac")
SCORE_KINDS = ("normal", "tied", "const", "offset", "collide")
NAN_KINDS = ("nan1", "nan_several", "nan_nm1", "nan_all", "inf")


def make_labels(kind, B, L, g, presort=False):
    """fp32 labels [B, L]: 'mslr' / 'yahoo' graded 0..4, 'binary', 'perm' (a random permutation of L .. 1 per list: LABEL_TYPE.Permutation),
    'frac' (uniform in [0, 4]).  No list is forced to hold a relevant document.  presort: every row sorted descending."""
    if kind in MIXES:
        y = g.choice(5, size=(B, L), p=MIXES[kind]).astype(np.float32)
    elif kind == "binary":
        y = (g.random((B, L)) < 0.3).astype(np.float32)
    elif kind == "perm":
        y = np.stack([g.permutation(L) + 1 for _ in range(B)]).astype(np.float32)
    elif kind == "frac":
        y = (4.0 * g.random((B, L))).astype(np.float32)
    else:
        raise ValueError(kind)
    return -np.sort(-y, axis=1) if presort else y


def ragged_lens(B, L, g):
    """int32 list lengths in [0, L] that always contain 0, 1, 2 and L (as far as L and B allow)."""
    must = sorted({0, 1, min(2, L), L})
    assert B >= len(must), "the batch is too small to hold the lengths 0, 1, 2 and L"
    lens = np.concatenate([np.asarray(must), g.integers(0, L + 1, size=B - len(must))]).astype(np.int32)
    return lens[g.permutation(B)]


def packed_key_bits(L):
    """Index bits of the packed (score, index) key a list of L documents is sorted by (65 .. 1024 documents: N = 64 DPT slots)."""
    return max(6, int(math.ceil(math.log2(max(L, 2)))))


def make_scores(kind, B, L, g, lens=None):
    """fp32 scores [B, L]: 'normal' N(0,1); 'tied' rounded to halves; 'const'; 'offset' N(0,1) + 1e3; 'collide' 1 + i 2^-23 shuffled
    (distinct scores that agree in the packed key's score bits); 'inf' N(0,1) with +inf and -inf planted; 'nan1' / 'nan_several' /
    'nan_nm1' / 'nan_all': N(0,1) with 1, about a fifth, n - 1 and all of each list's scores NaN."""
    s = g.standard_normal((B, L)).astype(np.float32)
    if kind == "normal":
        return s
    if kind == "tied":
        return (np.round(s * 2.0) / 2.0).astype(np.float32)
    if kind == "const":
        return np.full((B, L), 0.25, np.float32)
    if kind == "offset":
        return (s + np.float32(1e3)).astype(np.float32)
    if kind == "collide":
        out = np.stack([(1.0 + g.permutation(L).astype(np.float64) * 2.0 ** -23) for _ in range(B)]).astype(np.float32)
        if L >= 2:
            v = np.sort(out[0]).view(np.uint32) >> packed_key_bits(L)
            assert (v[1:] == v[:-1]).any(), "no adjacent pair collides in the packed key's score bits"
            assert len(np.unique(out[0])) == L
        return out
    for q in range(B):
        n = _qlen(lens, q, L)
        if n == 0:
            continue
        if kind == "inf":
            pos = g.permutation(n)[:min(n, 4)]
            s[q, pos] = np.asarray([np.inf, -np.inf, np.inf, -np.inf], np.float32)[:len(pos)]
        elif kind == "nan1":
            s[q, g.integers(n)] = np.nan
        elif kind == "nan_several":
            s[q, g.permutation(n)[:max(2, n // 5)]] = np.nan
        elif kind == "nan_nm1":
            s[q, g.permutation(n)[:max(1, n - 1)]] = np.nan
        elif kind == "nan_all":
            s[q, :n] = np.nan
        else:
            raise ValueError(kind)
    return s


CUTOFF_POOL = (1, 2, 3, 5, 10, 63, 64, 65, 127, 128, 129, 192, 193, 1023, 1024, 1025)
MAX_CUTOFFS = 32                                           # PTR_MAX_CUTOFFS


def cutoffs_for(L, g=None):
    """Up to 32 of {1, 2, 3, 5, 10, 63 .. 1025, L - 1, L, L + 1, 2 L} that make sense for L (the pool below 2 L, and the four around L),
    ascending; with g: shuffled, one duplicate added."""
    ks = sorted({k for k in CUTOFF_POOL if k <= 2 * L} | {k for k in (L - 1, L, L + 1, 2 * L) if k >= 1})
    assert len(ks) < MAX_CUTOFFS
    if g is not None:
        ks = ks + [ks[len(ks) // 2]]
        ks = [ks[i] for i in g.permutation(len(ks))]
    return ks


TILING_LENGTHS = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)
NAN_LENGTHS = (8, 64, 130, 512, 1024, 1500, 4096)


def case(B, L, label_kind, score_kind, seed, ragged=True, presort=False, ks=None, shuffle_ks=False, max_label=None):
    """One input of the gates: a dict with preds, labels (fp32 [B, L]), lens (int32 [B] or None), ks, presort, permutation_labels,
    max_label."""
    g = np.random.default_rng(seed)
    lens = ragged_lens(B, L, g) if ragged else None
    labels = make_labels(label_kind, B, L, g, presort=False)
    if presort:                                            # sorted over the valid part of each list (what presort promises)
        for q in range(B):
            n = _qlen(lens, q, L)
            labels[q, :n] = -np.sort(-labels[q, :n])
    preds = make_scores(score_kind, B, L, g, lens)
    if ks is None:
        ks = cutoffs_for(L, g if shuffle_ks else None)
    return dict(preds=preds, labels=labels, lens=lens, ks=list(ks), presort=bool(presort), permutation_labels=label_kind == "perm",
                max_label=max_label)


def cases_A(L):
    """Case A for one list length: every (score kind, ragged, presort), the label mix and the cut-off order alternating so that each occurs
    with every score kind, ragged or not, presorted or not."""
    B = 6
    out = []
    for si, sk in enumerate(SCORE_KINDS):
        for ragged in (True, False):
            for presort in (False, True):
                j = int(ragged) + int(presort)
                mix = ("mslr", "binary")[(si + j) % 2]
                shuffle = bool((si + int(ragged)) % 2)
                name = f"A L{L} {sk} {'ragged' if ragged else 'full'} presort{int(presort)} {mix} ks-{'shuffled' if shuffle else 'ascending'}"
                out.append((name, case(B, L, mix, sk, 1000 * L + 20 * si + 2 * int(ragged) + int(presort), ragged, presort, shuffle_ks=shuffle)))
    return out


def cases_C():
    """Case C without the 3700 x 1024 batch (built by the GPU test itself): Permutation labels, fractional labels, the max_label routes."""
    out = []
    for L in (130, 1025, 4096):
        out.append((f"C perm L{L}", case(5, L, "perm", "normal", 7000 + L, ragged=True, presort=False)))
    for L in (65, 300, 1500):
        for ml in (4.0, 2.0, 2.5, None):
            if ml is not None and ml < 4.0 and L > 300:
                continue           # a max_label below the labels makes |1 - sat| up to 2.75: the cascade of a long ideal list overflows fp32
            for kind, sk, seed in (("frac", "normal", 7100 + L), ("yahoo", "tied", 7200 + L)):
                cs = case(6, L, kind, sk, seed, ragged=True, max_label=ml)
                if ml is not None:
                    un = np.abs(1.0 - (np.exp2(-np.sort(-cs["labels"].astype(np.float64), axis=1)) - 1.0) / 2.0 ** ml)
                    assert float(np.cumprod(np.maximum(un, 1.0), axis=1).max()) < 2.0 ** 100, "the cascade must stay far inside the fp32 range"
                out.append((f"C {kind} L{L} max_label {ml}", cs))
    # max_label=None: batch_max_kernel with lens (above), with an odd total (no lens, 3 x 65), batch_max_vec_kernel (no lens, 4 x 64)
    out.append(("C max odd total", case(3, 65, "mslr", "normal", 7301, ragged=False)))
    out.append(("C max vec", case(4, 64, "mslr", "normal", 7302, ragged=False)))
    return out


DEGENERATE_LENGTHS = (1, 5, 64, 65, 300, 1500)


def cases_D():
    """Case D: lists without a relevant document (every label 0) of 1 .. 1500 documents beside ordinary neighbours, a zero-length list, and
    relevant documents only beyond every cut-off."""
    out = []
    for n in DEGENERATE_LENGTHS:
        L = max(n, 8)
        g = np.random.default_rng(8000 + n)
        B = 5
        labels = make_labels("mslr", B, L, g)
        labels[:, 0] = np.maximum(labels[:, 0], 1.0)       # the neighbours hold a relevant document
        preds = make_scores("normal", B, L, g)
        lens = np.asarray([L, n, 0, n, L], np.int32)
        labels[1, :] = 0.0
        labels[3, :] = 0.0
        ks = [k for k in (1, 3, 5, 10, 64, 65, 128, 300, 1500) if k <= 2 * L]
        out.append((f"D norel n{n}", dict(preds=preds, labels=labels, lens=lens, ks=ks, presort=False, permutation_labels=False, max_label=4.0,
                                          norel_rows=(1, 3), empty_rows=(2,), neighbour_rows=(0, 4))))
    for L in (40, 200, 1500):                              # the relevant documents are ranked beyond every cut-off
        g = np.random.default_rng(8100 + L)
        B = 3
        preds = make_scores("normal", B, L, g)
        labels = np.zeros((B, L), np.float32)
        for q in range(B):
            o = order_desc(preds[q])
            labels[q, o[20:]] = g.choice(5, size=L - 20, p=MIXES["yahoo"]).astype(np.float32)
            labels[q, o[-1]] = 2.0
        out.append((f"D beyond L{L}", dict(preds=preds, labels=labels, lens=None, ks=[1, 5, 10, 20], presort=False, permutation_labels=False,
                                           max_label=None)))
    return out


def cases_E(L):
    """Case E for one row length: 1, several, n - 1 and all NaN scores, and +-inf, ragged."""
    out = []
    for i, kind in enumerate(NAN_KINDS):
        out.append((f"E L{L} {kind}", case(6, L, ("mslr", "yahoo")[i % 2], kind, 9000 + 10 * L + i, ragged=True,
                                           ks=[k for k in (1, 2, 5, 10, 64, 65, 129, 1024, 1025, L - 1, L) if 1 <= k <= L] + [L + 1])))
    return out


def all_gpu_cases():
    """Every input of the GPU cases A - E that has a reference on the CPU (everything but the 3700 x 1024 batch of case C)."""
    for L in TILING_LENGTHS:
        yield from cases_A(L)
    yield from cases_C()
    yield from cases_D()
    for L in NAN_LENGTHS:
        yield from cases_E(L)


def restate(cs, c=None, **kw):
    return metrics(cs["preds"], cs["labels"], cs["lens"], cs["ks"], presort=cs["presort"], permutation_labels=cs["permutation_labels"],
                   max_label=cs["max_label"], c=c, **kw)
