#!/usr/bin/env python3
"""Generate tests/golden/gbdt_sklearn_depth.npz by RUNNING SCIKIT-LEARN: whole regression fits of HistGradientBoostingRegressor with
max_leaf_nodes=None and max_depth=d, the outside implementation the DEPTH-WISE growth of ptranking_amd/gbdt.py (grow_policy='depthwise')
is compared with.  Under a depth limit alone sklearn's best-first trainer splits every leaf that has a valid split down to depth d, which
is the set of leaves depth-wise growth splits when its leaf cap (2^d here) cannot bind.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gbdt_sklearn_depth.py

Everything else is make_golden_gbdt_sklearn.py's, imported from it: the input recipe (codes / 8, labels in 1 / 64, weights in 1 / 16), the
archive layout (tests/gbdt_sk.py load() unpacks it; num_leaves holds 2^max_depth), the canonical form, the fresh rows, the fixed zip
timestamps, and the screen: every split search keeps a relative gap of at least gbdt_sk.MIN_MARGIN between the best gain and the
runner-up, or the seed is redrawn; nothing is written if the depth-wise restatement (tests/gbdt_level_ref.py) disagrees with sklearn.

  case  rows x features  max_bin  max_depth  what it reaches
  g     600 x 7          63       3          one feature tile with a tail
  h     1500 x 17        255      5          two tiles; ragged levels; direct-form and LDS-form segments in one level
  i     900 x 33         64       4          three tiles; sample weights, so Hessians are not 1
  j     257 x 1          16       2          one row over the direct / LDS bound
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

import gbdt_level_ref as LR
import gbdt_sk as SK

_spec = importlib.util.spec_from_file_location("make_golden_gbdt_sklearn", os.path.join(HERE, "make_golden_gbdt_sklearn.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

FILE = "gbdt_sklearn_depth.npz"
# name: rows, F, max_bin, leaves (2^max_depth: the cap that cannot bind), min_data, lr, l2, rounds, max_depth, weights, exact tree
CASES = {"g": (600, 7, 63, 8, 5, 0.5, 0.25, 5, 3, False, False),
         "h": (1500, 17, 255, 32, 20, 0.1, 0.0, 4, 5, False, False),
         "i": (900, 33, 64, 16, 3, 0.2, 1.0, 3, 4, True, False),
         "j": (257, 1, 16, 4, 1, 1.0, 0.0, 2, 2, False, False)}
B.CASES = CASES                                     # the base generator's inputs() reads the shapes from its table


def fit(name, codes, y64, w16):
    """Runs sklearn without a leaf limit -> (baseline, [(nodes, leaves)] per round in canonical form, staged [rounds, n], the estimator)."""
    from sklearn.ensemble import HistGradientBoostingRegressor
    n, nf, max_bin, leaves, min_data, lr, l2, rounds, max_depth, _, _ = CASES[name]
    assert leaves == 2 ** max_depth
    X, y = codes.astype(np.float64) / 8.0, y64.astype(np.float64) / 64.0
    w = None if w16 is None else w16.astype(np.float64) / 16.0
    est = HistGradientBoostingRegressor(loss="squared_error", learning_rate=lr, max_iter=rounds, max_leaf_nodes=None, max_depth=max_depth,
                                        min_samples_leaf=min_data, l2_regularization=l2, max_bins=max_bin, early_stopping=False,
                                        random_state=0).fit(X, y, sample_weight=w)
    assert est.n_iter_ == rounds
    trees = []
    for (pred,) in est._predictors:
        nd = pred.nodes
        leaf = nd["is_leaf"].astype(bool)
        thr = nd["num_threshold"][~leaf].astype(np.float32)
        assert np.array_equal(thr.astype(np.float64), nd["num_threshold"][~leaf])          # a midpoint of two codes / 8: exact in fp32
        trees.append((SK.sort_rows(np.stack([nd["feature_idx"][~leaf], thr, nd["count"][~leaf]], axis=1).reshape(-1, 3)),
                      SK.sort_rows(np.stack([nd["value"][leaf], nd["count"][leaf]], axis=1))))
    staged = np.stack([np.asarray(s, np.float64) for s in est.staged_predict(X)])
    return float(np.ravel(est._baseline_prediction)[0]), trees, staged, est


def case_store(name, seed):
    """-> the archive members of one case, in the base generator's layout."""
    n, nf, max_bin, leaves, min_data, lr, l2, rounds, max_depth, _, exact = CASES[name]
    codes, y64, w16 = B.inputs(name, seed)
    assert all(np.unique(codes[:, f]).size <= max_bin for f in range(nf))
    baseline, trees, staged, est = fit(name, codes, y64, w16)
    fresh16 = B.fresh_rows(name, seed, codes, trees)
    store = {"codes": codes, "y64": y64, "baseline": np.float64(baseline),
             "params": np.array([max_bin, leaves, min_data, lr, l2, rounds, max_depth, int(exact), seed], np.float64),
             "nodes": np.concatenate([t[0] for t in trees]), "leaves": np.concatenate([t[1] for t in trees]),
             "tree_offsets": np.concatenate([[[0, 0]], np.cumsum([[t[0].shape[0], t[1].shape[0]] for t in trees], axis=0)]).astype(np.int32),
             "staged": staged, "fresh16": fresh16, "fresh_pred": np.asarray(est.predict(fresh16.astype(np.float64) / 16.0), np.float64)}
    if w16 is not None:
        store["w16"] = w16
    return {f"{name}/{k}": np.asarray(v) for k, v in store.items()}


def generate(verbose=False):
    import sklearn
    store = {"sklearn_version": np.array(sklearn.__version__)}
    for name in CASES:
        for seed in range(20):
            part = case_store(name, seed)
            case = B.unpack(dict(part, sklearn_version=store["sklearn_version"]))[name]
            miss, need, leaf_need, margin = LR.compare_restatement(case)
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
                  f"leaves per tree {[int(t.shape[0]) for t in case['leaves']]}", flush=True)
        store.update(part)
    return store


def main():
    store = generate(verbose=True)
    out = os.path.join(HERE, FILE)
    B.write_npz(out, store)
    print(f"wrote {out}: {len(store)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
