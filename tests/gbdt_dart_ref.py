"""Plain-numpy restatement of DART boosting in the native booster (ptranking_amd/csrc/gbdt_dart.hip: ptr_gbdt_dart_walk,
ptr_gbdt_dart_select, ptr_gbdt_dart_scale; boosting_type='dart' of ptranking_amd/gbdt.py).  include/ptranking_amd.h states the rule.  Test
infrastructure, never imported by the package.  Nothing here is LightGBM's: the rule is this project's own.
"""
import numpy as np

from gbdt_sample_ref import uniforms

SKIP_UNIT = 0xFFFFFFFF


def probabilities(w, drop_rate, max_drop, uniform_drop):
    """p_t float32 [T] from the weights: rate = min(drop_rate, max_drop / T) when max_drop > 0; uniform: rate; else min(1, rate w / mean(w))."""
    w = np.asarray(w, np.float64)
    rate = min(drop_rate, max_drop / w.size) if max_drop > 0 and w.size else drop_rate
    return (np.full(w.size, rate) if uniform_drop or not w.size else np.minimum(1.0, rate * w / w.mean())).astype(np.float32)


def select(p, seed, draw, skip_drop):
    """The trees a round drops, ascending: none iff u(seed, draw, 0xFFFFFFFF) < float32(skip_drop), else those with u(seed, draw, t) < p[t]."""
    p = np.asarray(p, np.float32)
    if uniforms(seed, draw, [SKIP_UNIT])[0] < np.float32(skip_drop):
        return []
    return np.nonzero(uniforms(seed, draw, np.arange(p.size)) < p)[0].tolist()


def rates(lr, k, xgboost_mode=False):
    """(the learning rate of the new tree, the factor of the dropped trees) with k trees dropped."""
    if k == 0:
        return lr, 1.0
    return (lr / (lr + k), k / (k + lr)) if xgboost_mode else (lr / (1.0 + k), k / (k + 1.0))


def scaled(values, factor):
    return (np.asarray(values, np.float32).astype(np.float64) * factor).astype(np.float32)


def leaf_values(bins, F, tree):
    """value[leaf(bins_i)] of one tree in bin space (feature, bin, also, left, right, value) -> float32 [n]; NaN for a malformed tree."""
    feature, bin, also, left, right, value = (np.asarray(a) for a in tree)
    nn, n = len(feature), bins.shape[0]
    node = np.full(n, 0 if nn else ~0, np.int64)
    for _ in range(nn):                                                  # every row takes one step; a row that has ended stays where it is
        at = np.where((node >= 0) & (node < nn), node, 0)
        live = (node >= 0) & (node < nn) & (feature[at] >= 0) & (feature[at] < F)
        b = bins[np.arange(n), np.where(live, feature[at], 0)]
        node = np.where(live, np.where((b <= bin[at]) | (b == also[at]), left[at], right[at]), node)
    ok = (node < 0) & (~node <= nn)
    return np.where(ok, np.asarray(value, np.float32)[np.where(ok, ~node, 0)], np.float32(np.nan)).astype(np.float32)


def walk(scores, per_tree, trees, sign):
    """out = in + sign * acc, acc = 0.0f + the listed trees' values in list order, every add in float32.  per_tree: leaf_values by tree, or
    None for a list entry outside the forest."""
    acc = np.zeros(scores.size, np.float32)
    for t in trees:
        acc = acc + (per_tree[t] if 0 <= t < len(per_tree) else np.float32(np.nan))
    return (np.asarray(scores, np.float32) + np.float32(sign) * acc).astype(np.float32)


def replay_selection(rounds, lr, drop_rate, max_drop, skip_drop, uniform_drop, seed, xgboost_mode=False, first_draw=0):
    """The drops of every round from the weights this restatement tracks alone -> [(dropped, tree lr, factor)] per round."""
    w, out = [], []
    for r in range(rounds):
        drop = select(probabilities(w, drop_rate, max_drop, uniform_drop), seed, first_draw + r, skip_drop) if w else []
        new_lr, factor = rates(lr, len(drop), xgboost_mode)
        for t in drop:
            w[t] *= factor
        w.append(new_lr)
        out.append((drop, new_lr, factor))
    return out
