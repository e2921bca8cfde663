#!/usr/bin/env python3
"""Generate tests/golden/gbdt_sklearn_missing.npz by RUNNING SCIKIT-LEARN: whole regression fits of HistGradientBoostingRegressor on data
with NaNs, the outside implementation the missing-value handling of ptranking_amd/gbdt.py (use_missing=True) is compared with.  sklearn
keeps a dedicated NaN bin per feature and learns a default direction per split (missing_go_to_left); its rules, where they are
deterministic, are the ones tests/gbdt_missing_ref.py restates.

Run on the build machine (scikit-learn is needed here only; the tests read the archive), never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gbdt_sklearn_missing.py

It follows make_golden_gbdt_sklearn.py (imported: the archive writer, the zip timestamps): exact fp32 inputs from integer codes (X = codes /
8, y = y64 / 64, w = w16 / 16), a seeded redraw under gbdt_sk.MIN_MARGIN, nothing written unless the restatement reproduces sklearn.  A
few features hold NaNs at a rate of about 0.25 (a mask beside the codes), and the label depends on the missingness of two of them, so that
NaN-against-the-rest splits and both directions occur.  sklearn is given max_bins = min(max_bin, 255): its NaN bin lies outside max_bins,
this project's inside max_bin, so a feature with a NaN has at most max_bin - 1 distinct values here.

  case  rows x features  max_bin  what it reaches
  p     600 x 7          63       the small case; one feature tile with a tail
  q     1500 x 17        255      a feature of 200 distinct values plus NaN: the scan's upper lanes carry bins and the NaN bin
  r     1500 x 17        256      a feature of exactly 255 distinct values plus NaN: nan_bin = 255; sample weights
  s     900 x 33         64       max_depth 3; sample weights; three tiles
  t     900 x 9          64       max_depth 4 with max_leaf_nodes=None: the trees depth-wise growth gives as well (params: depthwise = 1)

Members per case <c>, beside make_golden_gbdt_sklearn.py's (codes, y64, w16, params, baseline, leaves, tree_offsets, staged, fresh16,
fresh_pred):

  <c>/nan uint8 [n, F]        1 where X is NaN (the code there is 0)
  <c>/params float64 [10]     gbdt_missing_ref.PARAM_NAMES: gbdt_sk's nine and depthwise
  <c>/nodes float64 [K, 5]    per round: (feature, fp32 threshold (+inf: NaN against the rest), training rows under the node,
                              missing_go_to_left, training rows under the node that are missing in the split feature), sorted; every
                              node through gbdt_missing_ref.canonical_node, which writes ONE spelling where sklearn's choice between
                              several spellings of one partition is rounding noise
  <c>/fresh_nan uint8 [m, F]  NaNs of the fresh rows, also in features that never had one in training
  <c>/fresh_compared uint8 [m]  0 where the row's walk through sklearn's trees meets, with a NaN in the split feature, a node whose
                              direction is undecided: a feature with training NaNs, none of them under that node.  sklearn's choice there
                              is rounding noise between two identical partitions; this project takes the majority child.  0 as well where
                              it meets a node that has several spellings for one partition of its training rows with a value on which
                              the spellings part (gbdt_missing_ref.canonical_node, which also writes such nodes one way in <c>/nodes).

Refused unless at least 90 % of the NaN-bearing fresh rows of every case are compared.
"""
import importlib.util
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import gbdt_missing_ref as MR
import gbdt_sk as SK

_spec = importlib.util.spec_from_file_location("make_golden_gbdt_sklearn", os.path.join(HERE, "make_golden_gbdt_sklearn.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

FILE = "gbdt_sklearn_missing.npz"
SEED = 1409
N_FRESH = 120
NAN_RATE = 0.25
MIN_COMPARED = 0.9
# name: rows, F, max_bin, leaves, min_data, lr, l2, rounds, max_depth, weights, depthwise (sklearn: max_leaf_nodes=None; leaves = 2^max_depth)
CASES = {"p": (600, 7, 63, 8, 5, 0.5, 0.25, 5, -1, False, False),
         "q": (1500, 17, 255, 31, 20, 0.1, 0.0, 6, -1, False, False),
         "r": (1500, 17, 256, 31, 3, 0.3, 1.0, 4, -1, True, False),
         "s": (900, 33, 64, 64, 2, 0.2, 0.0, 3, 3, True, False),
         "t": (900, 9, 64, 16, 3, 0.2, 0.5, 4, 4, False, True)}
NAN_FEATURES = (1, 2, 5)                    # the features that hold NaNs; the label depends on the missingness of the first and the last
WIDE_FEATURE, WIDE_VALUES = 5, {"q": 200, "r": 255}


def inputs(name, seed):
    """(codes uint8 [n, F], nan bool [n, F], y64 int16 [n], w16 uint8 [n] or None) — seeded, sklearn-free."""
    n, nf, max_bin, weights = CASES[name][0], CASES[name][1], CASES[name][2], CASES[name][9]
    rng = np.random.default_rng([SEED, ord(name), seed])
    codes = np.zeros((n, nf), np.uint8)
    for f in range(nf):
        card = WIDE_VALUES[name] if (name in WIDE_VALUES and f == WIDE_FEATURE) else int(rng.integers(min(8, max_bin), min(max_bin, 40) + 1))
        levels = np.sort(rng.choice(256, card, replace=False))
        codes[:, f] = levels[rng.integers(0, card, n)]
        if name in WIDE_VALUES and f == WIDE_FEATURE:
            codes[:card, f] = levels                                                  # every level occurs ...
    nan = np.zeros((n, nf), bool)
    for f in NAN_FEATURES:
        nan[:, f] = rng.random(n) < NAN_RATE
    if name in WIDE_VALUES:
        nan[:WIDE_VALUES[name], WIDE_FEATURE] = False                                 # ... among the rows that are not missing
    codes[nan] = 0
    z = np.where(nan, 0.5, codes.astype(np.float64) / 256.0)
    col = lambda k: z[:, k % nf]
    s = (3.0 * col(0) + 2.0 * (col(1) > 0.5) - 2.0 * col(2) * col(0) + np.sin(6.0 * col(3)) + 1.5 * col(WIDE_FEATURE) ** 2
         + 1.5 * nan[:, NAN_FEATURES[0]] - 1.25 * nan[:, NAN_FEATURES[2]] + 0.3 * rng.standard_normal(n))
    y64 = np.rint(s * 64.0).astype(np.int16)
    w16 = rng.integers(1, 33, n).astype(np.uint8) if weights else None
    return codes, nan, y64, w16


def walk(nd, X):
    """The training rows under every node of one of sklearn's predictors, by its own rule -> {node: rows}."""
    at, out = {0: np.arange(X.shape[0])}, {}
    for i in range(nd.shape[0]):                                                      # a child's index is above its parent's
        rows = at.pop(i)
        out[i] = rows
        if nd["is_leaf"][i]:
            continue
        x = X[rows, nd["feature_idx"][i]]
        go_left = np.where(np.isnan(x), bool(nd["missing_go_to_left"][i]), x <= nd["num_threshold"][i])
        at[int(nd["left"][i])], at[int(nd["right"][i])] = rows[go_left], rows[~go_left]
    return out


def fit(name, codes, nan, y64, w16):
    """Runs sklearn -> (baseline, [(nodes, leaves)] per round in canonical form, staged [rounds, n], the estimator)."""
    from sklearn.ensemble import HistGradientBoostingRegressor
    n, nf, max_bin, leaves, min_data, lr, l2, rounds, max_depth, _, depthwise = CASES[name]
    assert not depthwise or leaves == 2 ** max_depth
    X = np.where(nan, np.nan, codes.astype(np.float64) / 8.0)
    X32, has_nan = X.astype(np.float32), nan.any(axis=0)                              # codes / 8: exact in fp32
    y = y64.astype(np.float64) / 64.0
    w = None if w16 is None else w16.astype(np.float64) / 16.0
    est = HistGradientBoostingRegressor(loss="squared_error", learning_rate=lr, max_iter=rounds, max_leaf_nodes=None if depthwise else leaves,
                                        max_depth=None if max_depth < 0 else max_depth, min_samples_leaf=min_data, l2_regularization=l2,
                                        max_bins=min(max_bin, 255), early_stopping=False, random_state=0).fit(X, y, sample_weight=w)
    assert est.n_iter_ == rounds
    trees = []
    for (pred,) in est._predictors:
        nd = pred.nodes
        under = walk(nd, X)
        leaf = nd["is_leaf"].astype(bool)
        assert all(under[i].size == nd["count"][i] for i in range(nd.shape[0]))
        thr = nd["num_threshold"].astype(np.float32)
        assert np.array_equal(thr.astype(np.float64), nd["num_threshold"])             # a midpoint of two codes / 8, or +inf: exact in fp32
        nodes = [MR.canonical_node(X32, under[i], int(nd["feature_idx"][i]), thr[i], nd["missing_go_to_left"][i], has_nan)[0]
                 for i in np.nonzero(~leaf)[0]]
        trees.append((MR.sort_nodes(np.array(nodes, np.float64).reshape(-1, 5)), SK.sort_rows(np.stack([nd["value"][leaf], nd["count"][leaf]], axis=1))))
    staged = np.stack([np.asarray(s, np.float64) for s in est.staged_predict(X)])
    return float(np.ravel(est._baseline_prediction)[0]), trees, staged, est


def fresh_rows(name, seed, codes, nan, trees):
    """(int16 [N_FRESH, F] in units of 1 / 16, NaN mask bool [N_FRESH, F]): rows on the grid, just off it, exactly on thresholds, outside the
    training range; the rows from 30 on carry NaNs, in any feature."""
    rng = np.random.default_rng([SEED, ord(name), seed, 1])
    n, nf = codes.shape
    pick = rng.integers(0, n, N_FRESH)
    out, mask = 2 * codes[pick].astype(np.int16), nan[pick].copy()
    for f in np.nonzero(nan.any(axis=0))[0]:                                          # a value of the feature under every NaN that is taken away below
        seen = codes[~nan[:, f], f]
        out[mask[:, f], f] = 2 * seen[rng.integers(0, seen.size, int(mask[:, f].sum()))].astype(np.int16)
    mask[:30] = False
    out[40:60] += rng.choice([-1, 1], (20, nf)).astype(np.int16)
    nodes = np.concatenate([t[0] for t in trees])
    nodes = nodes[np.isfinite(nodes[:, 1])]
    for i, k in enumerate(rng.permutation(nodes.shape[0])[:30]):                      # exactly on a threshold: goes left
        out[60 + i, int(nodes[k, 0])] = np.int16(round(nodes[k, 1] * 16.0))
        mask[60 + i, int(nodes[k, 0])] = False
    out[90:93], out[93:96] = -16, 2 * 255 + 40
    mask[90:96] = False
    mask[96:] |= rng.random((N_FRESH - 96, nf)) < 0.2                                 # NaNs in features that never had one in training
    mask[30:40] |= rng.random((10, nf)) < 0.1
    out[mask] = 0
    return out, mask


def compared(est, fresh, feature_has_nan, X):
    """bool [m]: the fresh row's walk meets no undecided node with a NaN in its feature, and no node of the two kinds that have several
    spellings (gbdt_missing_ref.canonical_node) with a value on which the spellings part: outside the node's training range where the
    node sets the NaNs against every value, inside the empty stretch around the threshold where it holds no missing rows."""
    keep = np.ones(fresh.shape[0], bool)
    for (pred,) in est._predictors:
        nd = pred.nodes
        under = walk(nd, X)
        for r in range(fresh.shape[0]):
            i = 0
            while not nd["is_leaf"][i]:
                f = int(nd["feature_idx"][i])
                x = fresh[r, f]
                col = X[under[i], f]
                miss = np.isnan(col)
                left = np.where(miss, bool(nd["missing_go_to_left"][i]), col <= nd["num_threshold"][i])
                if np.isnan(x):
                    if feature_has_nan[f] and not miss.any():
                        keep[r] = False
                    go = bool(nd["missing_go_to_left"][i])
                else:
                    if miss.any() and (np.array_equal(left, miss) or np.array_equal(left, ~miss)) and not col[~miss].min() <= x <= col[~miss].max():
                        keep[r] = False
                    if feature_has_nan[f] and not miss.any() and col[left].max() < x < col[~left].min():
                        keep[r] = False
                    go = x <= nd["num_threshold"][i]
                i = int(nd["left"][i] if go else nd["right"][i])
    return keep


def case_store(name, seed):
    """-> the archive members of one case."""
    n, nf, max_bin, leaves, min_data, lr, l2, rounds, max_depth, _, depthwise = CASES[name]
    codes, nan, y64, w16 = inputs(name, seed)
    for f in range(nf):
        assert np.unique(codes[~nan[:, f], f]).size <= (max_bin - 1 if nan[:, f].any() else min(max_bin, 255))
    if name in WIDE_VALUES:
        assert np.unique(codes[~nan[:, WIDE_FEATURE], WIDE_FEATURE]).size == WIDE_VALUES[name] and nan[:, WIDE_FEATURE].any()
    baseline, trees, staged, est = fit(name, codes, nan, y64, w16)
    fresh16, fresh_nan = fresh_rows(name, seed, codes, nan, trees)
    X = np.where(nan, np.nan, codes.astype(np.float64) / 8.0)
    fresh = np.where(fresh_nan, np.nan, fresh16.astype(np.float64) / 16.0)
    keep = compared(est, fresh, nan.any(axis=0), X)
    bearing = fresh_nan.any(axis=1)
    if keep[bearing].mean() < MIN_COMPARED:
        raise SystemExit(f"case {name} seed {seed}: only {keep[bearing].mean():.2f} of the NaN-bearing fresh rows can be compared: NOT written")
    store = {"codes": codes, "nan": nan.astype(np.uint8), "y64": y64, "baseline": np.float64(baseline),
             "params": np.array([max_bin, leaves, min_data, lr, l2, rounds, max_depth, 0, seed, int(depthwise)], np.float64),
             "nodes": np.concatenate([t[0] for t in trees]), "leaves": np.concatenate([t[1] for t in trees]),
             "tree_offsets": np.concatenate([[[0, 0]], np.cumsum([[t[0].shape[0], t[1].shape[0]] for t in trees], axis=0)]).astype(np.int32),
             "staged": staged, "fresh16": fresh16, "fresh_nan": fresh_nan.astype(np.uint8), "fresh_compared": keep.astype(np.uint8),
             "fresh_pred": np.asarray(est.predict(fresh), np.float64)}
    if w16 is not None:
        store["w16"] = w16
    return {f"{name}/{k}": np.asarray(v) for k, v in store.items()}


def unpack(store):
    """The cases of an in-memory store, as gbdt_missing_ref.load() gives them."""
    import io
    buf = io.BytesIO()
    np.savez(buf, **{k: v for k, v in store.items()})
    buf.seek(0)
    return MR.load(buf)[0]


def generate(verbose=False):
    import sklearn
    store = {"sklearn_version": np.array(sklearn.__version__)}
    worst_need = 0.0
    for name in CASES:
        for seed in range(20):
            part = case_store(name, seed)
            case = unpack(dict(part, sklearn_version=store["sklearn_version"]))[name]
            miss, need, leaf_need, margin = MR.compare_restatement(case)
            if margin >= SK.MIN_MARGIN:
                break
            if verbose:
                print(f"case {name} seed {seed}: margin {margin:.2e} fails the screen, redrawn", flush=True)
        else:
            raise SystemExit(f"case {name}: no seed of 20 passes the screen")
        if miss is not None:
            raise SystemExit(f"case {name} seed {seed}: the restatement disagrees with sklearn ({miss}) at margin {margin:.2e}: NOT written")
        worst_need = max(worst_need, need)
        if verbose:
            nodes = np.concatenate(case["nodes"])
            und = ~MR.decided(nodes, case["nan"].any(axis=0))
            bearing = case["fresh_nan"].any(axis=1)
            print(f"case {name} seed {seed}: margin {margin:.2e}, predictions need {need:.2f}, leaf values {leaf_need:.2f}; nodes {nodes.shape[0]}: "
                  f"{int(np.isinf(nodes[:, 1]).sum())} NaN against the rest, {int(((nodes[:, 4] > 0) & (nodes[:, 3] > 0)).sum())} missing-left and "
                  f"{int(((nodes[:, 4] > 0) & (nodes[:, 3] == 0) & np.isfinite(nodes[:, 1])).sum())} missing-right with missing rows, {int(und.sum())} undecided; "
                  f"fresh rows with a NaN {int(bearing.sum())}, compared {int(case['fresh_compared'][bearing].sum())}", flush=True)
        store.update(part)
    if verbose:
        print(f"the restatement's worst need {worst_need:.2f}: the gate constant is twice that, rounded up", flush=True)
    return store


def main():
    store = generate(verbose=True)
    out = os.path.join(HERE, FILE)
    B.write_npz(out, store)
    print(f"wrote {out}: {len(store)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
