#!/usr/bin/env python3
"""Generate tests/golden/gbdt_sklearn_cat.npz by RUNNING SCIKIT-LEARN: whole regression fits of
HistGradientBoostingRegressor(categorical_features=...), the outside implementation the categorical splits of ptranking_amd/gbdt.py
(categorical_feature) are compared with.  Its rules, where they are deterministic, are the ones tests/gbdt_cat_ref.py restates.

Run on the build machine (scikit-learn is needed here only; the tests read the archive), never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gbdt_sklearn_cat.py

It follows make_golden_gbdt_sklearn.py (imported: the archive writer, the zip timestamps): exact fp32 inputs from integer codes
(y = y64 / 64, w = w16 / 16), a seeded redraw under the screen, nothing written unless the restatement reproduces sklearn.

The estimator moves categorical columns to the front and ordinal-encodes them, so a node's feature_idx and raw_left_cat_bitsets live in
the transformed space.  Here the categorical columns ARE the leading columns and every one holds the contiguous codes 0 .. k - 1, each of
them at least once: both maps are the identity (asserted on the fitted preprocessor's categories).  A categorical column holds the code
itself, a numeric one codes / 8.

  case  rows x features  categorical  max_bin  what it reaches
  a     800 x 5          5            64       every feature categorical; skewed codes: several hold fewer than cat_smooth rows
  b     1200 x 9         3            255      numeric and categorical features mixed
  c     900 x 7          2            64       NaNs in categorical column 1, under use_missing: the NaN bin as one more category
  d     1000 x 6         3            64       sample weights below 1: TC / TH is about 3.5 and the Hessians are no counts
  e     1500 x 4         2            255      column 0 holds 200 codes, 80 of them rare: the scan's upper lanes carry keys
  f     900 x 6          2            64       max_depth 3 with max_leaf_nodes=None: the trees depth-wise growth gives as well

The screen (a condition on the inputs, decided by the restatement alone): at every node visited the best gain keeps gbdt_sk.MIN_MARGIN
over the runner-up, and adjacent sort keys and every support test keep a relative gap of the same size from equality (with unit Hessians
both sides of a support test are exact integers in both implementations, and equality is no accident to screen).  A case that fails
redraws its seed, at most 20 times.

Members per case <c>, beside make_golden_gbdt_sklearn.py's (codes, y64, w16, baseline, leaves, tree_offsets, staged, fresh16, fresh_pred):

  <c>/nan uint8 [n, F]        1 where X is NaN (the code there is 0)
  <c>/params float64 [12]     gbdt_cat_ref.PARAM_NAMES: gbdt_missing_ref's ten, ncat (the leading columns that are categorical), use_missing
  <c>/nodes float64 [K, 13]   per round, sorted: feature, categorical, fp32 threshold (0 at a categorical node), training rows under the
                              node, missing_go_to_left, the left code set as 8 uint32 words (bit c of the set: code c goes left)
  <c>/fresh_nan uint8 [m, F]  NaNs of the fresh rows: only in a categorical column that holds NaNs in training
Fresh rows hold codes seen in training only: scikit-learn treats an unseen code as missing, this project sends it right.
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

import gbdt_cat_ref as CR
import gbdt_sk as SK

_spec = importlib.util.spec_from_file_location("make_golden_gbdt_sklearn", os.path.join(HERE, "make_golden_gbdt_sklearn.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

FILE = "gbdt_sklearn_cat.npz"
SEED = 1511
N_FRESH = 100
# name: rows, F, max_bin, leaves, min_data, lr, l2, rounds, max_depth, weights, depthwise, the categorical columns' cardinalities, NaN column
CASES = {"a": (800, 5, 64, 8, 5, 0.5, 0.25, 5, -1, False, False, (6, 12, 23, 40, 9), None),
         "b": (1200, 9, 255, 31, 20, 0.1, 0.0, 6, -1, False, False, (23, 8, 50), None),
         "c": (900, 7, 64, 16, 3, 0.3, 1.0, 4, -1, False, False, (17, 11), 1),
         "d": (1000, 6, 64, 12, 4, 0.2, 0.5, 4, -1, True, False, (23, 14, 30), None),
         "e": (1500, 4, 255, 31, 2, 0.2, 0.0, 4, -1, False, False, (200, 15), None),
         "f": (900, 6, 64, 8, 3, 0.2, 0.5, 4, 3, False, True, (19, 10), None)}
NAN_RATE = 0.2
RARE = {"e": 80}                            # case e: that many of column 0's codes hold 2 rows each


def inputs(name, seed):
    """(codes uint8 [n, F], nan bool [n, F], y64 int16 [n], w16 uint8 [n] or None) — seeded, sklearn-free."""
    n, nf, max_bin, weights, cards, nan_col = CASES[name][0], CASES[name][1], CASES[name][2], CASES[name][9], CASES[name][11], CASES[name][12]
    rng = np.random.default_rng([SEED, ord(name), seed])
    codes = np.zeros((n, nf), np.uint8)
    effect = np.zeros(n)
    for f, card in enumerate(cards):
        if name in RARE and f == 0:                                                   # the rare codes 2 rows each, the others share the rest
            rare = rng.permutation(card)[:RARE[name]]
            common = np.setdiff1d(np.arange(card), rare)
            col = np.concatenate([np.repeat(rare, 2), common, common[rng.integers(0, common.size, n - 2 * rare.size - common.size)]])
        else:                                                                         # skewed: a few codes hold most rows, every code at least one
            p = rng.dirichlet(np.full(card, 0.6))
            col = np.concatenate([np.arange(card), rng.choice(card, n - card, p=p)])
        codes[:, f] = rng.permutation(col)
        lift = rng.standard_normal(card) * (1.5 if f < 2 else 0.6)                    # the label: a scattered effect per code
        effect += lift[codes[:, f]]
    for f in range(len(cards), nf):
        card = int(rng.integers(8, min(max_bin, 40) + 1))
        levels = np.sort(rng.choice(256, card, replace=False))
        codes[:, f] = levels[rng.integers(0, card, n)]
    nan = np.zeros((n, nf), bool)
    if nan_col is not None:
        nan[:, nan_col] = rng.random(n) < NAN_RATE
        keep = np.zeros(n, bool)
        for c in range(cards[nan_col]):                                               # every code keeps at least one row that is not missing
            keep[np.nonzero(codes[:, nan_col] == c)[0][0]] = True
        nan[keep, nan_col] = False
        effect += 1.5 * nan[:, nan_col]
    codes[nan] = 0
    z = codes.astype(np.float64) / 256.0
    num = list(range(len(cards), nf))
    s = effect + 0.3 * rng.standard_normal(n)
    if num:
        s += 3.0 * z[:, num[0]] + np.sin(6.0 * z[:, num[-1]]) - 2.0 * z[:, num[len(num) // 2]] * z[:, num[0]]
    y64 = np.rint(s * 64.0).astype(np.int16)
    w16 = rng.integers(1, 9, n).astype(np.uint8) if weights else None                # weights of 1/16 .. 1/2: TC / TH is about 3.5
    return codes, nan, y64, w16


def matrix(name, codes, nan):
    """The float64 matrix sklearn is given: the code itself in a categorical column, codes / 8 in a numeric one, NaN where nan."""
    ncat = len(CASES[name][11])
    X = codes.astype(np.float64) / 8.0
    X[:, :ncat] = codes[:, :ncat]
    X[nan] = np.nan
    return X


def sk_goes_left(nd, i, x, left_sets):
    """sklearn's own rule for raw values x at node i."""
    miss = np.isnan(x)
    if nd["is_categorical"][i]:
        words = left_sets[int(nd["bitset_idx"][i])]
        c = np.where(miss, 0, x).astype(np.int64)
        go = ((words[c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)
    else:
        go = x <= nd["num_threshold"][i]
    return np.where(miss, bool(nd["missing_go_to_left"][i]), go)


def walk(nd, X, left_sets):
    """The training rows under every node of one of sklearn's predictors, by its own rule -> {node: rows}."""
    at, out = {0: np.arange(X.shape[0])}, {}
    for i in range(nd.shape[0]):                                                      # a child's index is above its parent's
        rows = at.pop(i)
        out[i] = rows
        if nd["is_leaf"][i]:
            continue
        go = sk_goes_left(nd, i, X[rows, nd["feature_idx"][i]], left_sets)
        at[int(nd["left"][i])], at[int(nd["right"][i])] = rows[go], rows[~go]
    return out


def fit(name, codes, nan, y64, w16):
    """Runs sklearn -> (baseline, [(nodes, leaves)] per round in canonical form, staged [rounds, n], the estimator)."""
    from sklearn.ensemble import HistGradientBoostingRegressor
    n, nf, max_bin, leaves, min_data, lr, l2, rounds, max_depth, _, depthwise, cards, _ = CASES[name]
    assert not depthwise or leaves == 2 ** max_depth
    ncat = len(cards)
    X = matrix(name, codes, nan)
    y = y64.astype(np.float64) / 64.0
    w = None if w16 is None else w16.astype(np.float64) / 16.0
    est = HistGradientBoostingRegressor(loss="squared_error", learning_rate=lr, max_iter=rounds, max_leaf_nodes=None if depthwise else leaves,
                                        max_depth=None if max_depth < 0 else max_depth, min_samples_leaf=min_data, l2_regularization=l2,
                                        max_bins=min(max_bin, 255), categorical_features=list(range(ncat)), early_stopping=False,
                                        random_state=0).fit(X, y, sample_weight=w)
    assert est.n_iter_ == rounds
    enc = est._preprocessor.named_transformers_["encoder"]                            # the identity: codes 0 .. k - 1 in the leading columns
    assert [c[~np.isnan(c)].tolist() for c in enc.categories_] == [list(range(k)) for k in cards]      # (a NaN is listed behind the codes)
    assert np.array_equal(est._preprocessor.output_indices_["encoder"].indices(nf), (0, ncat, 1))
    trees = []
    for (pred,) in est._predictors:
        nd, sets = pred.nodes, pred.raw_left_cat_bitsets
        under = walk(nd, X, sets)
        leaf = nd["is_leaf"].astype(bool)
        assert all(under[i].size == nd["count"][i] for i in range(nd.shape[0]))
        nodes = []
        for i in np.nonzero(~leaf)[0]:
            f, cat = int(nd["feature_idx"][i]), bool(nd["is_categorical"][i])
            assert cat == (f < ncat)
            bits = 0
            if cat:
                bits = sum(int(wd) << (32 * k) for k, wd in enumerate(sets[int(nd["bitset_idx"][i])]))
                assert bits < (1 << cards[f])                                         # known codes only
            else:
                thr = np.float32(nd["num_threshold"][i])
                assert np.float64(thr) == nd["num_threshold"][i]                      # a midpoint of two codes / 8: exact in fp32
            nodes.append(CR.node_row(f, cat, nd["num_threshold"][i], nd["count"][i], nd["missing_go_to_left"][i], bits))
        trees.append((CR.sort_nodes(nodes), SK.sort_rows(np.stack([nd["value"][leaf], nd["count"][leaf]], axis=1))))
    staged = np.stack([np.asarray(s, np.float64) for s in est.staged_predict(X)])
    return float(np.ravel(est._baseline_prediction)[0]), trees, staged, est


def fresh_rows(name, seed, codes, nan):
    """(int16 [N_FRESH, F] in units of 1 / 16, NaN mask): training rows recombined; numeric columns just off the grid in the rows 40 ..
    59 and outside the training range in the last six; categorical columns hold seen codes only; NaNs only where training had them."""
    rng = np.random.default_rng([SEED, ord(name), seed, 1])
    n, nf = codes.shape
    ncat, nan_col = len(CASES[name][11]), CASES[name][12]
    out = np.zeros((N_FRESH, nf), np.int16)
    for f in range(nf):
        seen = codes[~nan[:, f], f]
        out[:, f] = seen[rng.integers(0, seen.size, N_FRESH)].astype(np.int16) * (16 if f < ncat else 2)
    out[40:60, ncat:] += rng.choice([-1, 1], (20, nf - ncat)).astype(np.int16)
    out[94:97, ncat:], out[97:, ncat:] = -16, 2 * 255 + 40
    mask = np.zeros((N_FRESH, nf), bool)
    if nan_col is not None:
        mask[20:40, nan_col] = True
    out[mask] = 0
    return out, mask


def case_store(name, seed):
    """-> the archive members of one case."""
    n, nf, max_bin, leaves, min_data, lr, l2, rounds, max_depth, _, depthwise, cards, nan_col = CASES[name]
    codes, nan, y64, w16 = inputs(name, seed)
    for f, k in enumerate(cards):
        assert np.array_equal(np.unique(codes[~nan[:, f], f]), np.arange(k)) and k <= min(max_bin, 255) - (1 if nan[:, f].any() else 0)
    baseline, trees, staged, est = fit(name, codes, nan, y64, w16)
    fresh16, fresh_nan = fresh_rows(name, seed, codes, nan)
    fresh = fresh16.astype(np.float64) / 16.0
    fresh[fresh_nan] = np.nan
    store = {"codes": codes, "nan": nan.astype(np.uint8), "y64": y64, "baseline": np.float64(baseline),
             "params": np.array([max_bin, leaves, min_data, lr, l2, rounds, max_depth, 0, seed, int(depthwise), len(cards), int(nan_col is not None)], np.float64),
             "nodes": np.concatenate([t[0] for t in trees]), "leaves": np.concatenate([t[1] for t in trees]),
             "tree_offsets": np.concatenate([[[0, 0]], np.cumsum([[t[0].shape[0], t[1].shape[0]] for t in trees], axis=0)]).astype(np.int32),
             "staged": staged, "fresh16": fresh16, "fresh_nan": fresh_nan.astype(np.uint8), "fresh_pred": np.asarray(est.predict(fresh), np.float64)}
    if w16 is not None:
        store["w16"] = w16
    return {f"{name}/{k}": np.asarray(v) for k, v in store.items()}


def unpack(store):
    """The cases of an in-memory store, as gbdt_cat_ref.load() gives them."""
    import io
    buf = io.BytesIO()
    np.savez(buf, **{k: v for k, v in store.items()})
    buf.seek(0)
    return CR.load(buf)[0]


def generate(verbose=False):
    import sklearn
    store = {"sklearn_version": np.array(sklearn.__version__)}
    worst_need = 0.0
    for name in CASES:
        for seed in range(20):
            part = case_store(name, seed)
            case = unpack(dict(part, sklearn_version=store["sklearn_version"]))[name]
            miss, need, leaf_need, margin = CR.compare_restatement(case)
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
            cat = nodes[nodes[:, 1] > 0]
            sizes = [bin(int(sum(int(w) << (32 * k) for k, w in enumerate(row[5:])))).count("1") for row in cat]
            print(f"case {name} seed {seed}: margin {margin:.2e}, predictions need {need:.2f}, leaf values {leaf_need:.2f}; nodes {nodes.shape[0]}, "
                  f"{cat.shape[0]} categorical (left sets of {min(sizes, default=0)} .. {max(sizes, default=0)} codes, "
                  f"{int((cat[:, 4] > 0).sum())} with missing_go_to_left)", flush=True)
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
