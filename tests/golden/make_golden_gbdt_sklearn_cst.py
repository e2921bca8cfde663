#!/usr/bin/env python3
"""Generate tests/golden/gbdt_sklearn_cst.npz by RUNNING SCIKIT-LEARN: whole regression fits of
HistGradientBoostingRegressor(monotonic_cst=..., interaction_cst=...), the outside implementation the monotone and interaction constraints
of ptranking_amd/gbdt.py are compared with.  Its rules, where they are deterministic, are the ones tests/gbdt_cst_ref.py restates.

Run on the build machine (scikit-learn is needed here only; the tests read the archive), never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gbdt_sklearn_cst.py

It follows make_golden_gbdt_sklearn_cat.py (imported: the walk of sklearn's nodes; make_golden_gbdt_sklearn.py's archive writer): exact fp32
inputs from integer codes (a numeric column holds codes / 8 with codes in 0 .. 23, a categorical one the code itself, y = y64 / 64,
w = w16 / 16), squared error, a seeded redraw under the conditions below, nothing written unless the restatement reproduces sklearn.
The label is a sine of every constrained feature, so an unconstrained fit is not monotone in it.

  case  rows x features  what it reaches
  a     600 x 5          +1 / -1 / 0 mix, leaf-wise with a binding leaf cap (8)
  b     600 x 5          (a) with lambda_l2 = 0.5 and sample weights
  c     600 x 5          max_leaf_nodes=None with max_depth 4: the trees depth-wise growth gives as well
  d     600 x 5          NaNs under use_missing in column 0, which is constrained +1
  e     600 x 5          column 0 categorical (12 codes) beside the constrained numeric columns 1 (+1) and 2 (-1)
  f     600 x 5          interaction_cst [{0, 1}, {2, 3}], column 4 unlisted: it forms the third group
  g     600 x 5          monotone and interaction constraints together

Conditions on the inputs, asserted here; a case that fails one redraws its seed (at most 40 times):
  - every split search of the restatement keeps gbdt_sk.MIN_MARGIN: the best gain over the runner-up, and every order test that does
    not compare two equal values over equality;
  - in every monotone case at least one search's winner differs from the winner without the order test (a rejection decided), and at
    least one stored leaf value is a clamped one;
  - in (f) some tree of the restatement WITHOUT the constraint uses two features that share no group on one path;
  - the unconstrained scikit-learn fit of case (a) is not monotone on the stored sweep (and the constrained one is).

Members per case <c>, beside make_golden_gbdt_sklearn_cat.py's (codes, nan, y64, w16, baseline, params, nodes, leaves, tree_offsets, staged,
fresh16, fresh_nan, fresh_pred):

  <c>/mono int8 [F]            the monotone constraints (zeros: none)
  <c>/groups uint8 [G, F]      the interaction groups as membership rows (G = 0: none); the unlisted features' group is NOT stored
  <c>/sweep16 int16 [S, F]     monotone cases: for every constrained feature three training rows with that feature swept over the codes
                               0 .. 23 in ascending order (units of 1 / 16); sweep_nan the NaNs of the other columns
  <c>/sweep_feature, sweep_block int32 [S]   the swept feature and the number of the sweep a row belongs to
  <c>/sweep_pred, sweep_free float64 [S]     scikit-learn's predictions under the constraints, and of the same fit without them
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
import gbdt_cst_ref as TR
import gbdt_sk as SK


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


B = _load("make_golden_gbdt_sklearn")
CG = _load("make_golden_gbdt_sklearn_cat")

FILE = "gbdt_sklearn_cst.npz"
SEED = 1789
N, NF, NCODES, N_FRESH, SWEEP_ROWS = 600, 5, 24, 100, 3
# name: max_bin, leaves, min_data, lr, l2, rounds, max_depth, weights, depthwise, ncat, NaN column, mono, groups
CASES = {"a": (64, 8, 5, 0.3, 0.0, 5, -1, False, False, 0, None, (1, -1, 0, 0, 0), ()),
         "b": (64, 8, 5, 0.3, 0.5, 5, -1, True, False, 0, None, (1, -1, 0, 0, 0), ()),
         "c": (64, 16, 5, 0.3, 0.25, 4, 4, False, True, 0, None, (1, 0, -1, 0, 0), ()),
         "d": (64, 12, 4, 0.3, 0.0, 4, -1, False, False, 0, 0, (1, -1, 0, 0, 0), ()),
         "e": (64, 12, 4, 0.3, 0.5, 4, -1, False, False, 1, None, (0, 1, -1, 0, 0), ()),
         "f": (64, 12, 5, 0.3, 0.0, 4, -1, False, False, 0, None, (0, 0, 0, 0, 0), ((0, 1), (2, 3))),
         "g": (64, 12, 5, 0.3, 0.25, 4, -1, False, False, 0, None, (1, 0, -1, 0, 0), ((0, 1), (2, 3)))}
CAT_CODES = 12
NAN_RATE = 0.2


def inputs(name, seed):
    """(codes uint8 [n, F], nan bool [n, F], y64 int16 [n], w16 uint8 [n] or None) — seeded, sklearn-free."""
    weights, ncat, nan_col, mono = CASES[name][7], CASES[name][9], CASES[name][10], CASES[name][11]
    rng = np.random.default_rng([SEED, ord(name), seed])
    codes = rng.integers(0, NCODES, (N, NF)).astype(np.uint8)
    s = 0.3 * rng.standard_normal(N)
    for f in range(NF):
        if f < ncat:
            col = np.concatenate([np.arange(CAT_CODES), rng.integers(0, CAT_CODES, N - CAT_CODES)])
            codes[:, f] = rng.permutation(col)
            s += (rng.standard_normal(CAT_CODES) * 1.2)[codes[:, f]]
            continue
        z = codes[:, f].astype(np.float64) / NCODES
        if mono[f]:                                                       # a trend the constraint agrees with, under a sine it does not
            s += mono[f] * 2.0 * z + 1.5 * np.sin(9.0 * z + f)
        else:
            s += np.sin(5.0 * z + f) * 0.8
    s += 1.5 * (codes[:, 0].astype(np.float64) / NCODES) * (codes[:, 2].astype(np.float64) / NCODES) * (0 if ncat else 1)   # across the groups of f and g
    nan = np.zeros((N, NF), bool)
    if nan_col is not None:
        nan[:, nan_col] = rng.random(N) < NAN_RATE
        s += 1.0 * nan[:, nan_col]
    codes[nan] = 0
    y64 = np.rint(s * 64.0).astype(np.int16)
    w16 = rng.integers(4, 33, N).astype(np.uint8) if weights else None
    return codes, nan, y64, w16


def matrix(name, codes, nan):
    """The float64 matrix sklearn is given: the code itself in a categorical column, codes / 8 in a numeric one, NaN where nan."""
    ncat = CASES[name][9]
    X = codes.astype(np.float64) / 8.0
    X[:, :ncat] = codes[:, :ncat]
    X[nan] = np.nan
    return X


def estimator(name, constrained=True):
    from sklearn.ensemble import HistGradientBoostingRegressor
    max_bin, leaves, min_data, lr, l2, rounds, max_depth, _, depthwise, ncat, _, mono, groups = CASES[name]
    assert not depthwise or leaves == 2 ** max_depth
    return HistGradientBoostingRegressor(loss="squared_error", learning_rate=lr, max_iter=rounds, max_leaf_nodes=None if depthwise else leaves,
                                         max_depth=None if max_depth < 0 else max_depth, min_samples_leaf=min_data, l2_regularization=l2,
                                         max_bins=min(max_bin, 255), categorical_features=list(range(ncat)) if ncat else None,
                                         monotonic_cst=list(mono) if constrained and any(mono) else None,
                                         interaction_cst=[set(g) for g in groups] if constrained and groups else None, early_stopping=False,
                                         random_state=0)


def fit(name, codes, nan, y64, w16):
    """Runs sklearn -> (baseline, [(nodes, leaves)] per round in canonical form, staged [rounds, n], the estimator)."""
    ncat = CASES[name][9]
    X = matrix(name, codes, nan)
    y = y64.astype(np.float64) / 64.0
    w = None if w16 is None else w16.astype(np.float64) / 16.0
    est = estimator(name).fit(X, y, sample_weight=w)
    assert est.n_iter_ == CASES[name][5]
    if ncat:
        enc = est._preprocessor.named_transformers_["encoder"]           # the identity: codes 0 .. k - 1 in the leading columns
        assert [c[~np.isnan(c)].tolist() for c in enc.categories_] == [list(range(CAT_CODES))] * ncat
        assert np.array_equal(est._preprocessor.output_indices_["encoder"].indices(NF), (0, ncat, 1))
    trees = []
    for (pred,) in est._predictors:
        nd, sets = pred.nodes, pred.raw_left_cat_bitsets
        under = CG.walk(nd, X, sets)
        leaf = nd["is_leaf"].astype(bool)
        assert all(under[i].size == nd["count"][i] for i in range(nd.shape[0]))
        nodes = []
        for i in np.nonzero(~leaf)[0]:
            f, cat = int(nd["feature_idx"][i]), bool(nd["is_categorical"][i])
            assert cat == (f < ncat)
            bits = 0
            if cat:
                bits = sum(int(wd) << (32 * k) for k, wd in enumerate(sets[int(nd["bitset_idx"][i])]))
                assert bits < (1 << CAT_CODES)
            else:
                assert np.float64(np.float32(nd["num_threshold"][i])) == nd["num_threshold"][i]
            nodes.append(CR.node_row(f, cat, nd["num_threshold"][i], nd["count"][i], nd["missing_go_to_left"][i], bits))
        trees.append((CR.sort_nodes(nodes), SK.sort_rows(np.stack([nd["value"][leaf], nd["count"][leaf]], axis=1))))
    staged = np.stack([np.asarray(s, np.float64) for s in est.staged_predict(X)])
    return float(np.ravel(est._baseline_prediction)[0]), trees, staged, est


def fresh_rows(name, seed, codes, nan):
    """(int16 [N_FRESH, F] in units of 1 / 16, NaN mask): training rows recombined; numeric columns just off the grid in the rows 40 .. 59
    and outside the training range in the last six; categorical columns hold seen codes only; NaNs only where training had them."""
    rng = np.random.default_rng([SEED, ord(name), seed, 1])
    ncat, nan_col = CASES[name][9], CASES[name][10]
    out = np.zeros((N_FRESH, NF), np.int16)
    for f in range(NF):
        seen = codes[~nan[:, f], f]
        out[:, f] = seen[rng.integers(0, seen.size, N_FRESH)].astype(np.int16) * (16 if f < ncat else 2)
    out[40:60, ncat:] += rng.choice([-1, 1], (20, NF - ncat)).astype(np.int16)
    out[94:97, ncat:], out[97:, ncat:] = -16, 2 * 255 + 40
    mask = np.zeros((N_FRESH, NF), bool)
    if nan_col is not None:
        mask[20:40, nan_col] = True
    out[mask] = 0
    return out, mask


def sweep_rows(name, seed, codes, nan):
    """For every constrained feature SWEEP_ROWS training rows with the feature swept over the codes 0 .. 23, ascending."""
    rng = np.random.default_rng([SEED, ord(name), seed, 2])
    ncat, mono = CASES[name][9], CASES[name][11]
    rows, masks, feats, blocks = [], [], [], []
    for f in np.nonzero(mono)[0]:
        for base in rng.integers(0, N, SWEEP_ROWS):
            r = np.repeat(codes[base:base + 1].astype(np.int16), NCODES, axis=0)
            r[:, :ncat] *= 16
            r[:, ncat:] *= 2
            r[:, f] = np.arange(NCODES) * 2
            m = np.repeat(nan[base:base + 1], NCODES, axis=0)
            m[:, f] = False
            r[m] = 0
            rows.append(r); masks.append(m); feats.append(np.full(NCODES, f)); blocks.append(np.full(NCODES, len(blocks)))
    return np.concatenate(rows), np.concatenate(masks), np.concatenate(feats).astype(np.int32), np.concatenate(blocks).astype(np.int32)


def steps(pred, feature, block, mono):
    """The smallest step of a prediction along its sweeps, in the direction the constraint demands (>= 0: monotone)."""
    worst = np.inf
    for b in np.unique(block):
        sel = block == b
        worst = min(worst, float((np.diff(pred[sel]) * mono[int(feature[sel][0])]).min()))
    return worst


def case_store(name, seed):
    """-> the archive members of one case."""
    max_bin, leaves, min_data, lr, l2, rounds, max_depth, _, depthwise, ncat, nan_col, mono, groups = CASES[name]
    codes, nan, y64, w16 = inputs(name, seed)
    baseline, trees, staged, est = fit(name, codes, nan, y64, w16)
    fresh16, fresh_nan = fresh_rows(name, seed, codes, nan)
    fresh = fresh16.astype(np.float64) / 16.0
    fresh[fresh_nan] = np.nan
    member = np.zeros((len(groups), NF), np.uint8)
    for k, g in enumerate(groups):
        member[k, list(g)] = 1
    store = {"codes": codes, "nan": nan.astype(np.uint8), "y64": y64, "baseline": np.float64(baseline),
             "params": np.array([max_bin, leaves, min_data, lr, l2, rounds, max_depth, 0, seed, int(depthwise), ncat, int(nan_col is not None)], np.float64),
             "nodes": np.concatenate([t[0] for t in trees]), "leaves": np.concatenate([t[1] for t in trees]),
             "tree_offsets": np.concatenate([[[0, 0]], np.cumsum([[t[0].shape[0], t[1].shape[0]] for t in trees], axis=0)]).astype(np.int32),
             "staged": staged, "fresh16": fresh16, "fresh_nan": fresh_nan.astype(np.uint8), "fresh_pred": np.asarray(est.predict(fresh), np.float64),
             "mono": np.array(mono, np.int8), "groups": member}
    if w16 is not None:
        store["w16"] = w16
    info = {}
    if any(mono):
        sw16, sw_nan, sw_f, sw_b = sweep_rows(name, seed, codes, nan)
        sw = sw16.astype(np.float64) / 16.0
        sw[sw_nan] = np.nan
        free = estimator(name, constrained=False).fit(matrix(name, codes, nan), y64.astype(np.float64) / 64.0,
                                                      sample_weight=None if w16 is None else w16.astype(np.float64) / 16.0)
        store.update(sweep16=sw16, sweep_nan=sw_nan.astype(np.uint8), sweep_feature=sw_f, sweep_block=sw_b,
                     sweep_pred=np.asarray(est.predict(sw), np.float64), sweep_free=np.asarray(free.predict(sw), np.float64))
        info = {"step": steps(store["sweep_pred"], sw_f, sw_b, mono), "free_step": steps(store["sweep_free"], sw_f, sw_b, mono)}
    return {f"{name}/{k}": np.asarray(v) for k, v in store.items()}, info


def unpack(store):
    """The cases of an in-memory store, as gbdt_cst_ref.load() gives them."""
    import io
    buf = io.BytesIO()
    np.savez(buf, **{k: v for k, v in store.items()})
    buf.seek(0)
    return TR.load(buf)[0]


def conditions(name, case, info):
    """-> (None or the condition that fails, the restatement's comparison)."""
    miss, need, leaf_need, margin = TR.compare_restatement(case)
    out = (miss, need, leaf_need, margin)
    if margin < SK.MIN_MARGIN:
        return f"margin {margin:.2e}", out
    if np.any(case["mono"]):
        stats = TR.run_restatement(case)[3]
        if sum(s["changed"] for s in stats) == 0:
            return "no search decided by a rejection", out
        if sum(s["clamped"] for s in stats) == 0:
            return "no clamped leaf value", out
        if not info["step"] >= 0.0:
            return f"sklearn's constrained fit steps by {info['step']}", out
        if name == "a" and not info["free_step"] < 0.0:
            return "the unconstrained fit is monotone on the sweep", out
    if name == "f":
        free = TR.run_restatement(case, groups=None)[0]
        if not any(TR.forbidden_pairs(TR.tree_paths(t), case["groups"], case["X"].shape[1]) for t, _ in free):
            return "no forbidden pair without the constraint", out
    return None, out


def generate(verbose=False):
    import sklearn
    store = {"sklearn_version": np.array(sklearn.__version__)}
    worst_need = 0.0
    for name in CASES:
        for seed in range(40):
            part, info = case_store(name, seed)
            case = unpack(dict(part, sklearn_version=store["sklearn_version"]))[name]
            why, (miss, need, leaf_need, margin) = conditions(name, case, info)
            if why is None:
                break
            if verbose:
                print(f"case {name} seed {seed}: {why}, redrawn", flush=True)
        else:
            raise SystemExit(f"case {name}: no seed of 40 meets the conditions")
        if miss is not None:
            raise SystemExit(f"case {name} seed {seed}: the restatement disagrees with sklearn ({miss}) at margin {margin:.2e}: NOT written")
        worst_need = max(worst_need, need)
        if verbose:
            print(f"case {name} seed {seed}: margin {margin:.2e}, predictions need {need:.2f}, leaf values {leaf_need:.2f}; "
                  f"nodes {np.concatenate(case['nodes']).shape[0]}; sweep steps {info}", flush=True)
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
