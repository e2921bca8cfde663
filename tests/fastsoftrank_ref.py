"""FastSoftRank, the rule of include/ptranking_amd.h in plain numpy: stack pool-adjacent-violators under the strict-violation merge, starting
from the fp32 keys z.  float64 is the reference of the GPU tests; at float32 it is the eager evaluation whose error sets the gate's constant.
Also returns the element-wise rounding bounds: 2^-24 times the sum of the magnitudes each output is built from.  Shares nothing with the kernel."""
import numpy as np

EPS32 = 2.0 ** -24


def keys(theta, eps):
    return (-theta.astype(np.float32) / np.float32(eps)).astype(np.float32)


def pav(u):
    """Non-increasing isotonic regression of u -> (v, start): v by position, start[p] = first position of p's block.  Pools merge only on a
    strict violation (left mean < right mean)."""
    sums, cnts = [], []
    for x in u:
        sums.append(x)
        cnts.append(1)
        while len(sums) > 1 and sums[-2] / cnts[-2] < sums[-1] / cnts[-1]:
            s, c = sums.pop(), cnts.pop()
            sums[-1] += s
            cnts[-1] += c
    first = np.cumsum([0] + cnts[:-1])
    return np.repeat(np.array(sums, dtype=u.dtype) / np.array(cnts, dtype=u.dtype), cnts), np.repeat(first, cnts)


def cumsum_form(u):
    """The same regression from prefix sums -> (v, start, margin): g(j) = max_{k>j} (S_k - S_j) / (k - j), v = running minimum of g, a block
    starting where g is strictly below the minimum so far; margin = min |g(j) - minimum so far| / max |u| (inf for one document)."""
    n = len(u)
    S = np.concatenate(([0.0], np.cumsum(u)))
    g = np.array([((S[j + 1:] - S[j]) / np.arange(1, n - j + 1)).max() for j in range(n)])
    v = np.minimum.accumulate(g)
    new = np.concatenate(([True], g[1:] < v[:-1]))
    margin = np.abs(g[1:] - v[:-1]).min() / np.abs(u).max() if n > 1 else np.inf
    return v, np.maximum.accumulate(np.where(new, np.arange(n), 0)), margin


def block_mean(a, start):
    ids = np.unique(start, return_inverse=True)[1]
    return (np.bincount(ids, weights=a) / np.bincount(ids))[ids].astype(a.dtype)


def query(theta, y, eps, objective, dtype=np.float64):
    """One query of n real documents -> dict(loss, ranks, grad by document; b_* their bounds; start by position; u)."""
    n = len(theta)
    z = keys(theta, eps)
    order = np.argsort(-z, kind="stable")                                       # descending, equal keys by the lower index
    s = z[order].astype(dtype)
    u = s - np.arange(n, 0, -1).astype(dtype)
    v, start = pav(u)
    r = s - v
    ys = y[order].astype(dtype)
    if objective == "spearman":
        target = ((ys[None, :] > ys[:, None]).sum(1) + ((ys[None, :] == ys[:, None]).sum(1) + 1) / 2).astype(dtype)
        a = r - target
        terms = a * a / 2
    else:
        gain = np.exp2(ys) - 1
        idcg = (np.sort(gain)[::-1] / np.log2(np.arange(n).astype(dtype) + 2)).sum()
        w = gain / idcg if idcg > 0 else np.zeros(n, dtype)
        lg = np.log2(1 + r)
        terms, a = -w / lg, w / (lg * lg * (1 + r) * dtype(np.log(2)))
    out = dict(start=start, u=u, loss=terms.sum(), b_loss=EPS32 * np.abs(terms).sum())
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    out["ranks"], out["b_ranks"] = r[inv], (EPS32 * (np.abs(s) + np.abs(v)))[inv]
    out["grad"] = (-(a - block_mean(a, start)) / dtype(eps))[inv]
    out["b_grad"] = (EPS32 * (np.abs(a) + block_mean(np.abs(a), start)) / dtype(eps))[inv]
    return out


def batch(preds, labels, lens, eps, objective, dtype=np.float64):
    """preds, labels [B, L] numpy, lens [B] or None -> dict of loss_q [B], ranks / grad [B, L] and b_* (float64), per-query block counts."""
    B, L = preds.shape
    out = {k: np.zeros((B, L)) for k in ("ranks", "grad", "b_ranks", "b_grad")}
    out.update(loss_q=np.zeros(B), b_loss_q=np.zeros(B), blocks=[], u=[])
    for q in range(B):
        n = L if lens is None else int(lens[q])
        if n == 0:
            continue
        if np.isnan(preds[q, :n]).any():
            out["loss_q"][q] = out["ranks"][q, :n] = out["grad"][q, :n] = np.nan
            continue
        one = query(preds[q, :n], labels[q, :n], eps, objective, dtype)
        out["blocks"].append((n, len(np.unique(one["start"]))))
        out["u"].append(one["u"])
        out["loss_q"][q], out["b_loss_q"][q] = one["loss"], one["b_loss"]
        for k in ("ranks", "grad", "b_ranks", "b_grad"):
            out[k][q, :n] = one[k]
    return out
