#!/usr/bin/env python3
"""Generate tests/golden/gbdt_sklearn.npz by RUNNING SCIKIT-LEARN: whole regression fits of HistGradientBoostingRegressor (its
LightGBM-style histogram trainer) and one DecisionTreeRegressor (the exact greedy best-first tree), the outside implementation the
gradient-boosted trees of ptranking_amd/gbdt.py are compared with.  LightGBM itself is not installed where this project is developed.

Run on the build machine (scikit-learn is needed here only; the tests read the archive), never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gbdt_sklearn.py

The rules of HistGradientBoostingRegressor that coincide with this project's: histogram splits, best-first growth under max_leaf_nodes,
min_samples_leaf, l2_regularization, min_hessian_to_split = 1e-3, bins at the midpoints when a feature has no more distinct values than
bins, left on x <= threshold; under squared error a round's inputs are g = (score - y) * w and h = w.  So every feature here has at most
max_bin distinct values (the quantile rule for more is this project's own and is NOT pinned), early_stopping is off, there are no
categorical or missing features, and n is far below sklearn's 200 000-row binning subsample.

Everything is exact in fp32: X = codes / 8 (uint8 codes, so a midpoint is a multiple of 1 / 16), y = y64 / 64, w = w16 / 16.  Per case
<c> of CASES (tests/gbdt_sk.py load() unpacks them):

  <c>/codes uint8 [n, F]    <c>/y64 int16 [n]    <c>/w16 uint8 [n] (weighted cases only)
  <c>/params float64 [9]    gbdt_sk.PARAM_NAMES: max_bin, num_leaves, min_data_in_leaf, learning_rate, lambda_l2, rounds, max_depth (-1:
                            none), exact_tree (1: DecisionTreeRegressor), seed (the redraw that passed the screen)
  <c>/baseline float64      sklearn's prediction before the first tree (the weighted mean of y; 0 for the single exact tree)
  <c>/nodes float64 [K, 3]  per round, concatenated: the internal nodes' (feature, fp32 threshold, rows under the node), sorted
  <c>/leaves float64 [L, 2] per round, concatenated: the leaves' (value, rows), sorted
  <c>/tree_offsets int32 [rounds + 1, 2]  where a round's nodes / leaves begin
  <c>/staged float64 [rounds, n]  staged_predict on the training rows
  <c>/fresh16 int16 [m, F]  about 100 fresh rows, X = fresh16 / 16: rows on the grid, just off it (code +- 0.5), exactly on thresholds of the
                            fitted trees, below and above the training range
  <c>/fresh_pred float64 [m]  predict on them
  sklearn_version

The screen (a condition on the inputs, decided by the restatement tests/gbdt_ref.py alone): every split search of every round keeps a
relative gap of at least gbdt_sk.MIN_MARGIN between the best gain and the runner-up, because sklearn's gains carry about 1e-7 of
relative noise and a closer call would be a tie-break, not an error.  A case that fails it redraws its seed, 20 times at the most.  The
archive is written only if the restatement then reproduces every tree and every prediction of sklearn's (a disagreement on a screened
case is a finding, not a case to drop), with fixed zip timestamps, so a rerun reproduces it byte for byte.
"""
import io
import os
import sys
import zipfile

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import gbdt_sk as SK

FILE = "gbdt_sklearn.npz"
SEED = 1307
N_FRESH = 100
# name: rows, F, max_bin, leaves, min_data, lr, l2, rounds, max_depth, weights, exact tree
CASES = {"a": (600, 7, 63, 8, 5, 0.5, 0.25, 5, -1, False, False),
         "b": (1500, 17, 255, 31, 20, 0.1, 0.0, 6, -1, False, False),
         "c": (1500, 17, 255, 31, 3, 0.3, 1.0, 4, -1, True, False),
         "d": (900, 33, 64, 64, 2, 0.2, 0.0, 3, 3, True, False),
         "e": (257, 1, 16, 4, 1, 1.0, 0.0, 2, -1, False, False),
         "f": (600, 7, 63, 8, 5, 1.0, 0.0, 1, -1, False, True)}
WIDE_FEATURE, WIDE_VALUES = 5, 200          # case b: one feature of 200 distinct values, so the split scan's upper lanes carry bins


def write_npz(path, store):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.array(store[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def inputs(name, seed):
    """(codes uint8 [n, F], y64 int16 [n], w16 uint8 [n] or None) — seeded, sklearn-free.  A feature takes between 2 and min(max_bin, 40)
    of the 256 codes; the label is a sum of a slope, a step, an interaction and a wave over the first features, plus noise."""
    n, nf, max_bin, weights = CASES[name][0], CASES[name][1], CASES[name][2], CASES[name][9]
    rng = np.random.default_rng([SEED, ord(name), seed])
    codes = np.zeros((n, nf), np.uint8)
    for f in range(nf):
        card = WIDE_VALUES if (name == "b" and f == WIDE_FEATURE) else int(rng.integers(min(8, max_bin), min(max_bin, 40) + 1))
        levels = np.sort(rng.choice(256, card, replace=False))
        codes[:, f] = levels[rng.integers(0, card, n)]
    z = codes.astype(np.float64) / 256.0
    col = lambda k: z[:, k % nf]
    s = 3.0 * col(0) + 2.0 * (col(1) > 0.5) - 2.0 * col(2) * col(0) + np.sin(6.0 * col(3)) + 1.5 * col(WIDE_FEATURE) ** 2 + 0.3 * rng.standard_normal(n)
    y64 = np.rint(s * 64.0).astype(np.int16)
    w16 = rng.integers(1, 33, n).astype(np.uint8) if weights else None
    return codes, y64, w16


def fit(name, codes, y64, w16):
    """Runs sklearn -> (baseline, [(nodes, leaves)] per round in canonical form, staged [rounds, n], the fitted estimator)."""
    from sklearn.ensemble import HistGradientBoostingRegressor
    from sklearn.tree import DecisionTreeRegressor
    n, nf, max_bin, leaves, min_data, lr, l2, rounds, max_depth, _, exact = CASES[name]
    X, y = codes.astype(np.float64) / 8.0, y64.astype(np.float64) / 64.0
    w = None if w16 is None else w16.astype(np.float64) / 16.0
    trees = []
    if exact:
        est = DecisionTreeRegressor(max_leaf_nodes=leaves, min_samples_leaf=min_data, random_state=0).fit(X, y)
        t = est.tree_
        leaf = t.children_left < 0
        thr = t.threshold[~leaf].astype(np.float32)
        assert np.array_equal(thr.astype(np.float64), t.threshold[~leaf])
        trees.append((SK.sort_rows(np.stack([t.feature[~leaf], thr, t.n_node_samples[~leaf]], axis=1)),
                      SK.sort_rows(np.stack([t.value[leaf, 0, 0], t.n_node_samples[leaf]], axis=1))))
        return 0.0, trees, est.predict(X)[None, :].astype(np.float64), est
    est = HistGradientBoostingRegressor(loss="squared_error", learning_rate=lr, max_iter=rounds, max_leaf_nodes=leaves,
                                        max_depth=None if max_depth < 0 else max_depth, min_samples_leaf=min_data, l2_regularization=l2,
                                        max_bins=max_bin, early_stopping=False, random_state=0).fit(X, y, sample_weight=w)
    assert est.n_iter_ == rounds
    for (pred,) in est._predictors:
        nd = pred.nodes
        leaf = nd["is_leaf"].astype(bool)
        thr = nd["num_threshold"][~leaf].astype(np.float32)
        assert np.array_equal(thr.astype(np.float64), nd["num_threshold"][~leaf])          # a midpoint of two codes / 8: exact in fp32
        trees.append((SK.sort_rows(np.stack([nd["feature_idx"][~leaf], thr, nd["count"][~leaf]], axis=1).reshape(-1, 3)),
                      SK.sort_rows(np.stack([nd["value"][leaf], nd["count"][leaf]], axis=1))))
    staged = np.stack([np.asarray(s, np.float64) for s in est.staged_predict(X)])
    return float(np.ravel(est._baseline_prediction)[0]), trees, staged, est


def fresh_rows(name, seed, codes, trees):
    """int16 [N_FRESH, F] in units of 1 / 16."""
    rng = np.random.default_rng([SEED, ord(name), seed, 1])
    n, nf = codes.shape
    out = 2 * codes[rng.integers(0, n, N_FRESH)].astype(np.int16)
    out[40:60] += rng.choice([-1, 1], (20, nf)).astype(np.int16)                            # just off the grid: (code +- 0.5) / 8
    nodes = np.concatenate([t[0] for t in trees])
    for i, k in enumerate(rng.permutation(nodes.shape[0])[:30]):                            # exactly on a threshold: goes left
        out[60 + i, int(nodes[k, 0])] = np.int16(round(nodes[k, 1] * 16.0))
    out[90:93], out[93:96] = -16, 2 * 255 + 40                                              # below and above the training range
    mixed = rng.random((4, nf))
    out[96:100] = np.where(mixed < 0.3, -16, np.where(mixed > 0.7, 2 * 255 + 40, out[96:100]))
    return out


def case_store(name, seed):
    """-> the archive members of one case."""
    n, nf, max_bin, leaves, min_data, lr, l2, rounds, max_depth, _, exact = CASES[name]
    codes, y64, w16 = inputs(name, seed)
    assert all(np.unique(codes[:, f]).size <= max_bin for f in range(nf))
    baseline, trees, staged, est = fit(name, codes, y64, w16)
    fresh16 = fresh_rows(name, seed, codes, trees)
    store = {"codes": codes, "y64": y64, "baseline": np.float64(baseline),
             "params": np.array([max_bin, leaves, min_data, lr, l2, rounds, max_depth, int(exact), seed], np.float64),
             "nodes": np.concatenate([t[0] for t in trees]), "leaves": np.concatenate([t[1] for t in trees]),
             "tree_offsets": np.concatenate([[[0, 0]], np.cumsum([[t[0].shape[0], t[1].shape[0]] for t in trees], axis=0)]).astype(np.int32),
             "staged": staged, "fresh16": fresh16, "fresh_pred": np.asarray(est.predict(fresh16.astype(np.float64) / 16.0), np.float64)}
    if w16 is not None:
        store["w16"] = w16
    return {f"{name}/{k}": np.asarray(v) for k, v in store.items()}


def unpack(store):
    """The cases of an in-memory store, as gbdt_sk.load() gives them."""
    buf = io.BytesIO()
    np.savez(buf, **{k: v for k, v in store.items()})
    buf.seek(0)
    return SK.load(buf)[0]


def generate(verbose=False):
    import sklearn
    store = {"sklearn_version": np.array(sklearn.__version__)}
    for name in CASES:
        for seed in range(20):
            part = case_store(name, seed)
            case = unpack(dict(part, sklearn_version=store["sklearn_version"]))[name]
            miss, need, leaf_need, margin = SK.compare_restatement(case)
            if margin >= SK.MIN_MARGIN:
                break
            if verbose:
                print(f"case {name} seed {seed}: margin {margin:.2e} fails the screen, redrawn", flush=True)
        else:
            raise SystemExit(f"case {name}: no seed of 20 passes the screen")
        if miss is not None:
            raise SystemExit(f"case {name} seed {seed}: the restatement disagrees with sklearn ({miss}) at margin {margin:.2e}: NOT written")
        if verbose:
            print(f"case {name} seed {seed}: margin {margin:.2e}, predictions need {need:.2f}, leaf values {leaf_need:.2f}, "
                  f"max |score| {float(np.abs(case['staged']).max()):.2f}", flush=True)
        store.update(part)
    return store


def main():
    store = generate(verbose=True)
    out = os.path.join(HERE, FILE)
    write_npz(out, store)
    print(f"wrote {out}: {len(store)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
