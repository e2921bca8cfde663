"""GPU: TreeSHAP feature contributions of the native booster (GBDT.set_background, predict(pred_contrib=True); ptr_gbdt_leaf_counts and
ptr_gbdt_shap of csrc/gbdt.hip).  Fitted models against the exponential oracle (the Shapley definition, tests/gbdt_shap_ref.py), hand-built
trees against the polynomial restatement, both per element within C_SHAP x 2^-52 x sum over trees of max |leaf value| (C_SHAP is set by
test_gbdt_shap_cpu.py); local accuracy against predict under the derived fp32 summation bound; the dummy feature, the selected leaf, bit
stability, the background, and the tree ranges."""
import functools
import json

import numpy as np
import pytest
import torch

import gbdt_ref as R
import gbdt_shap_ref as SR

pytestmark = pytest.mark.gpu
SIZES = (1, 64, 65, 130)
# kind -> (F, trees, params): 1 to 8 trees of 2 to 16 leaves, F = 6 and 8; column F - 1 is constant in training (no tree can use it)
MODELS = {"plain": (6, 5, {"num_leaves": 7, "min_data_in_leaf": 5, "max_bin": 63}),
          "missing": (8, 8, {"num_leaves": 16, "min_data_in_leaf": 4, "max_bin": 31, "use_missing": True}),
          "cat": (6, 3, {"num_leaves": 6, "min_data_in_leaf": 5, "max_bin": 63, "categorical_feature": [1, 4], "cat_smooth": 1.0}),
          "depthwise": (8, 4, {"num_leaves": 12, "min_data_in_leaf": 5, "max_bin": 63, "grow_policy": "depthwise", "max_depth": 4}),
          "bagged": (8, 6, {"num_leaves": 9, "min_data_in_leaf": 5, "max_bin": 63, "bagging_fraction": 0.7, "bagging_freq": 1}),
          "stump": (6, 1, {"num_leaves": 2, "min_data_in_leaf": 5, "max_bin": 15})}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)


def data(kind, F, n, seed):
    rng = np.random.default_rng([seed, len(kind)])
    X = (np.round(rng.standard_normal((n, F)) * 4) / 4).astype(np.float32)
    if kind == "cat":
        X[:, 1], X[:, 4] = rng.integers(0, 8, n), rng.integers(0, 5, n)
    y = X[:, 0] * 1.5 - X[:, 2] + 0.7 * X[:, 0] * X[:, 3] + (np.isin(X[:, 1], (1, 2, 6)) * 2.0 if kind == "cat" else 0.5 * X[:, 1])
    if kind == "missing":
        X[rng.random((n, F)) < 0.15] = np.nan
    X[:, F - 1] = 0.5                                                       # the dummy
    return X, (y + 0.3 * rng.standard_normal(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fitted(kind):
    """-> (booster with the training matrix as background, training X, 130 evaluation rows, the exponential oracle on them, the leaf counts
    of the numpy walk)."""
    import ptranking_amd as pa
    F, rounds, params = MODELS[kind]
    X, y = data(kind, F, 300, 1)
    booster = pa.GBDT(dict(params, learning_rate=0.3), X)
    for _ in range(rounds):
        booster.update(booster.scores - dev(y), torch.ones(X.shape[0], device="cuda"))
    assert len(booster.trees) == rounds
    booster.set_background(X)
    Xe = np.concatenate([X[:50], data(kind, F, 80, 2)[0]])
    counts = [SR.leaf_counts(t, X) for t in booster.trees]
    return booster, X, Xe, SR.shap_exponential(booster.trees, counts, Xe, F), counts


def local_accuracy_bound(trees, X):
    """(T + 1) 2^-24 sum_t |v_t(x)|: predict adds T fp32 leaf values in order, each partial sum at most sum_t |v_t(x)| and each addition
    rounding by at most 2^-24 of it (T - 1 additions; one more unit for the float64 sums of phi, which are far below it)."""
    reach = sum(np.abs(np.asarray(t["value"], np.float32).astype(np.float64))[SR.leaf_of(t, X)] for t in trees) if trees else np.zeros(X.shape[0])
    return (len(trees) + 1) * 2.0 ** -24 * reach


# ---------------------------------------------------------------- fitted models against the Shapley definition
@pytest.mark.parametrize("kind", list(MODELS))
def test_fitted_models_match_the_exponential_oracle(kind):
    booster, X, Xe, want, counts = fitted(kind)
    F = X.shape[1]
    assert 1 <= len(booster.trees) <= 8 and all(2 <= t["value"].size <= 16 for t in booster.trees) and F in (6, 8)
    if kind == "cat":
        assert any((t["cat_index"] >= 0).any() for t in booster.trees) and any((t["cat_index"] < 0).any() for t in booster.trees)
    if kind == "missing":
        assert np.isnan(Xe).any() and any(t["default_left"].any() for t in booster.trees)
    tol = SR.C_SHAP * SR.bound(booster.trees)
    for n in SIZES:
        got = booster.predict(Xe[:n], pred_contrib=True)
        assert got.dtype == torch.float64 and tuple(got.shape) == (n, F + 1) and got.is_cuda
        err = np.abs(got.cpu().numpy() - want[:n]).max()
        print(f"{kind} n={n}: need {err / SR.bound(booster.trees):.3f} of C_SHAP {SR.C_SHAP}")
        assert err <= tol, (kind, n, err / SR.bound(booster.trees))


@pytest.mark.parametrize("kind", list(MODELS))
def test_local_accuracy_the_dummy_and_the_leaf_counts(kind):
    booster, X, Xe, want, counts = fitted(kind)
    F = X.shape[1]
    phi = booster.predict(Xe, pred_contrib=True).cpu().numpy()
    pred = booster.predict(Xe).cpu().numpy().astype(np.float64)
    assert (np.abs(phi.sum(axis=1) - pred) <= local_accuracy_bound(booster.trees, Xe)).all()
    assert np.array_equal(phi[:, F - 1].view(np.uint64), np.zeros(len(Xe), np.uint64))       # no tree uses the dummy: exactly +0.0
    assert all(F - 1 not in t["feature"] for t in booster.trees)
    # the device's leaf counts are the numpy walk's, and the training matrix reaches every leaf
    assert np.array_equal(booster._shap["leaf_counts"], np.concatenate(counts)) and min(c.min() for c in counts) > 0
    # the expected value is the cover-weighted mean of the training scores' tree values
    mean = sum(float((np.asarray(t["value"], np.float64) * c).sum() / c.sum()) for t, c in zip(booster.trees, counts))
    assert np.abs(phi[:, F] - mean).max() <= 64 * SR.bound(booster.trees)


def test_the_training_matrix_gives_the_counts_the_tree_was_grown_on():
    import ptranking_amd as pa
    params = {"num_leaves": 8, "min_data_in_leaf": 5, "max_bin": 63, "lambda_l2": 0.1}
    for seed in range(3, 23):                                               # the screen of test_gbdt_gpu.py: no split search decided by a near tie
        X, y = data("plain", 6, 300, seed)
        booster = pa.GBDT(params, X)
        p = booster.params
        qg, qh, expo, flag = R.quantize(-y, np.ones(300, np.float32))
        bins = R.bin_matrix(X, booster.edges, booster.nbins)
        want, leaf_rows, margin = R.grow_tree(bins, qg, qh, expo, booster.edges, booster.nbins, p["max_bin"], p["num_leaves"], p["learning_rate"],
                                              p["lambda_l2"], p["min_data_in_leaf"], p["min_sum_hessian_in_leaf"], p["min_gain_to_split"], p["max_depth"])
        if margin > 1e-9:
            break
    assert margin > 1e-9
    got = booster.update(dev(-y), torch.ones(300, device="cuda"))
    assert np.array_equal(got["feature"], want["feature"]) and np.array_equal(got["left"], want["left"]) and np.array_equal(got["right"], want["right"])
    booster.set_background(X)
    assert booster._shap["leaf_counts"].tolist() == [r.size for r in leaf_rows]


# ---------------------------------------------------------------- hand-built trees through a model file
def write_model(path, trees, F):
    """A format-1 model file with these trees (the keys GBDT.save_model writes)."""
    cat = lambda k, dt: np.concatenate([t[k] for t in trees]).astype(dt) if trees else np.zeros(0, dt)
    offs = np.concatenate([[0], np.cumsum([t["feature"].size for t in trees])]).astype(np.int32)
    np.savez(path, format=np.int64(1), params=np.array(json.dumps({"num_leaves": 4})), edges=np.zeros((F, 2), np.float32), nbins=np.full(F, 3, np.int32),
             best_iteration=np.int64(0), feature=cat("feature", np.int32), threshold=cat("threshold", np.float32), left=cat("left", np.int32),
             right=cat("right", np.int32), value=cat("value", np.float32), tree_offsets=offs)


def chain_rows(features, thresholds, F, fill):
    """Row i reaches leaf i of the chain: right at the nodes before i, left at node i; repeated 1 + i % 3 times, so that the covers differ."""
    rows = []
    for i in range(len(features) + 1):
        x = np.full(F, fill, np.float32)
        for j in range(min(i + 1, len(features))):
            x[features[j]] = thresholds[j] + (1.0 if j < i else -0.5)
        rows += [x] * (1 + i % 3)
    return np.stack(rows)


def hand_cases():
    rng = np.random.default_rng(7)
    f63 = rng.permutation(70)[:63].tolist()
    wide = SR.chain_tree(f63, [0.0] * 63, rng.standard_normal(64))
    wide_bg = chain_rows(f63, [0.0] * 63, 70, -1.0)
    wide_x = np.concatenate([wide_bg[::3], np.where(rng.random((40, 70)) < 0.85, 1.0, -1.0).astype(np.float32)])
    reuse_f = [i % 2 for i in range(40)]
    reuse_t = [float(i) for i in range(40)]
    reuse = SR.chain_tree(reuse_f, reuse_t, rng.standard_normal(41))
    # row i: its feature just below threshold i (and above threshold i - 2), the other feature above every threshold
    reuse_bg = np.stack([np.array([i - 0.5 if i % 2 == 0 else 99.0, i - 0.5 if i % 2 == 1 else 99.0, 0.0], np.float32) for i in range(40)]
                        + [np.array([99.0, 99.0, 0.0], np.float32)] * 2)
    reuse_x = np.concatenate([reuse_bg, (rng.random((60, 3)) * 45 - 2).astype(np.float32)])
    leaf = {"feature": np.zeros(0, np.int32), "threshold": np.zeros(0, np.float32), "left": np.zeros(0, np.int32), "right": np.zeros(0, np.int32),
            "value": np.array([-0.375], np.float32)}
    three = rng.standard_normal((9, 3)).astype(np.float32)
    return {"wide": ([wide], 70, wide_bg, wide_x), "reuse": ([reuse], 3, reuse_bg, reuse_x), "leaf": ([leaf], 3, three, three),
            "mixed": ([leaf, reuse, leaf], 3, reuse_bg, reuse_x), "none": ([], 3, three, three)}


@pytest.mark.parametrize("name", ["wide", "reuse", "leaf", "mixed", "none"])
def test_hand_built_trees_match_the_polynomial_restatement(name, tmp_path):
    import ptranking_amd as pa
    from ptranking_amd import gbdt
    trees, F, bg, X = hand_cases()[name]
    write_model(tmp_path / "m.npz", trees, F)
    booster = pa.GBDT.load_model(tmp_path / "m.npz")
    assert len(booster.trees) == len(trees)
    with pytest.raises(RuntimeError, match="set_background"):
        booster.predict(X, pred_contrib=True)                              # a loaded model has no covers
    booster.set_background(bg)
    counts = [SR.leaf_counts(t, bg) for t in trees]
    tb = gbdt.shap_tables(trees, counts)
    if name == "wide":
        assert int(np.diff(tb["elem_offsets"]).max()) == 63                  # the full wavefront: 63 elements and the bias
    if name == "reuse":
        assert int(np.diff(tb["elem_offsets"]).max()) == 2 and int(np.diff(tb["path_offsets"]).max()) == 40
    want = SR.shap_polynomial(tb, trees, X, F)
    got = booster.predict(X, pred_contrib=True).cpu().numpy()
    assert got.shape == (len(X), F + 1)
    if name == "none":
        assert np.array_equal(got.view(np.uint64), np.zeros_like(got).view(np.uint64))       # zero trees: all zeros
        return
    err = np.abs(got - want).max()
    print(f"{name}: need {err / SR.bound(trees):.3f} of C_SHAP {SR.C_SHAP}")
    assert err <= SR.C_SHAP * SR.bound(trees)
    if name == "leaf":                                                     # (predict itself takes no model whose trees are all single leaves)
        assert np.array_equal(got, np.tile(np.array([0.0, 0.0, 0.0, -0.375]), (len(X), 1)))
        return
    pred = booster.predict(X).cpu().numpy().astype(np.float64)
    assert (np.abs(got.sum(axis=1) - pred) <= local_accuracy_bound(trees, X)).all()


# ---------------------------------------------------------------- the selected leaf
@pytest.mark.parametrize("kind", ["plain", "missing", "cat"])
def test_the_leaf_whose_one_fractions_are_all_one_is_the_leaf_predict_reaches(kind):
    """With the leaf values replaced by 1 + the leaf's index, a tree's contributions sum to the mark of the one leaf whose o's are all 1 (every
    other leaf's terms cancel), and predict under the same marks names the leaf the walk reaches."""
    import ptranking_amd as pa
    booster, X, Xe, want, counts = fitted(kind)
    fl, tables = booster._flat, booster._shap["tables"]
    offs = booster._shap["tree_leaf_offsets"]
    walk = {"default_left": fl.get("default_left"), **booster._cat_walk(dev(Xe))}
    for t in range(len(booster.trees)):
        lo, hi = int(offs[t]), int(offs[t + 1])
        marks = torch.zeros_like(tables["leaf_value"])
        marks[lo:hi] = torch.arange(1, hi - lo + 1, device="cuda", dtype=torch.float32)
        tb = dict(tables, leaf_value=marks[lo:hi], path_offsets=tables["path_offsets"][lo:hi + 1], elem_offsets=tables["elem_offsets"][lo:hi + 1])
        phi = pa.functional.gbdt_shap(dev(Xe), fl["feature"], fl["threshold"], tb, **walk)
        chosen = np.rint(phi.sum(dim=1).cpu().numpy()).astype(np.int64) - 1
        assert np.abs(phi.sum(dim=1).cpu().numpy() - (chosen + 1)).max() < 1e-9
        if kind == "cat":
            reached = pa.functional.gbdt_predict_cat(dev(Xe), fl["feature"], fl["threshold"], fl["left"], fl["right"], marks, fl["tree_offsets"],
                                                     walk["is_cat"], fl["cat_index"], fl["cat_sets"], default_left=fl.get("default_left"))
        else:
            reached = pa.functional.gbdt_predict(dev(Xe), fl["feature"], fl["threshold"], fl["left"], fl["right"], marks, fl["tree_offsets"],
                                                 default_left=fl.get("default_left"))
        assert np.array_equal(chosen, reached.cpu().numpy().astype(np.int64) - 1)
        assert np.array_equal(chosen, SR.leaf_of(booster.trees[t], Xe))


# ---------------------------------------------------------------- bits
@pytest.mark.parametrize("kind", ["plain", "missing", "cat"])
def test_bits_do_not_depend_on_the_run_the_batch_or_the_place(kind):
    booster, X, Xe, want, counts = fitted(kind)
    a, b = booster.predict(Xe, pred_contrib=True), booster.predict(Xe, pred_contrib=True)
    assert np.array_equal(bits(a), bits(b))
    for r in (0, 63, 64, 129):
        assert np.array_equal(bits(booster.predict(Xe[r:r + 1], pred_contrib=True))[0], bits(a)[r])          # alone and inside the batch of 130
    back = booster.predict(Xe[::-1].copy(), pred_contrib=True)
    assert np.array_equal(bits(back)[::-1], bits(a))                                                      # its place in the batch
    many = booster.predict(np.tile(Xe[:7], (1200, 1)), pred_contrib=True)                                  # 8400 rows: more rows than workgroups
    assert np.array_equal(bits(many).reshape(1200, 7, -1), np.broadcast_to(bits(a)[:7], (1200, 7, Xe.shape[1] + 1)))


def test_the_kernel_and_the_polynomial_restatement_agree_on_a_fitted_model():
    from ptranking_amd import gbdt
    booster, X, Xe, want, counts = fitted("missing")
    pol = SR.shap_polynomial(gbdt.shap_tables(booster.trees, counts), booster.trees, Xe, X.shape[1])
    got = booster.predict(Xe, pred_contrib=True).cpu().numpy()
    assert np.abs(got - pol).max() <= SR.C_SHAP * SR.bound(booster.trees)


# ---------------------------------------------------------------- the background, the ranges, the surface
def test_another_background_changes_phi_and_keeps_local_accuracy(tmp_path):
    import ptranking_amd as pa
    booster, X, Xe, want, counts = fitted("plain")
    booster.save_model(tmp_path / "a.npz")
    other = pa.GBDT.load_model(tmp_path / "a.npz")
    bg = np.concatenate([X, X[X[:, 0] > 0]])                                # another mix of the same rows: every leaf is still reached
    other.set_background(bg)
    assert not np.array_equal(other._shap["leaf_counts"], booster._shap["leaf_counts"])
    phi = other.predict(Xe, pred_contrib=True).cpu().numpy()
    assert np.abs(phi - want).max() > 1e-3                                  # other covers, other contributions
    cnt = [SR.leaf_counts(t, bg) for t in other.trees]
    assert np.abs(phi - SR.shap_exponential(other.trees, cnt, Xe, X.shape[1])).max() <= SR.C_SHAP * SR.bound(other.trees)
    pred = other.predict(Xe).cpu().numpy().astype(np.float64)
    assert (np.abs(phi.sum(axis=1) - pred) <= local_accuracy_bound(other.trees, Xe)).all()
    # the covers live in memory only: the file is the one written without a background
    other.save_model(tmp_path / "b.npz")
    assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
    with pytest.raises(ValueError, match=r"tree \d+: node .* has cover 0"):
        other.set_background(X[:1])


@pytest.mark.parametrize("kind,first,stop", [("plain", 0, 3), ("plain", 2, 5), ("missing", 3, 4), ("cat", 1, 3), ("cat", 2, 2)])
def test_tree_ranges_are_the_contributions_of_the_sub_model(kind, first, stop):
    import ptranking_amd as pa
    booster, X, Xe, want, counts = fitted(kind)
    got = booster.predict(Xe, num_iteration=stop, first_tree=first, pred_contrib=True)
    sub = pa.GBDT(booster.params)
    sub.edges, sub.nbins, sub.nan_bin, sub.trees = booster.edges, booster.nbins, booster.nan_bin, booster.trees[first:stop]
    sub.set_background(X)
    assert np.array_equal(bits(got), bits(sub.predict(Xe, pred_contrib=True)))
    ref = SR.shap_exponential(booster.trees[first:stop], counts[first:stop], Xe, X.shape[1])
    assert np.abs(got.cpu().numpy() - ref).max() <= SR.C_SHAP * max(SR.bound(booster.trees[first:stop]), 0.0)
    with pytest.raises(ValueError, match="trees"):
        booster.predict(Xe, num_iteration=len(booster.trees) + 1, pred_contrib=True)


def test_a_grown_booster_needs_its_background_again_and_false_is_todays_call():
    import ptranking_amd as pa
    X, y = data("plain", 6, 300, 5)
    booster = pa.GBDT({"num_leaves": 4, "min_data_in_leaf": 5}, X)
    ones = torch.ones(300, device="cuda")
    booster.update(booster.scores - dev(y), ones)
    with pytest.raises(RuntimeError, match="set_background"):
        booster.predict(X, pred_contrib=True)
    booster.set_background(X)
    before = booster.predict(X)
    assert tuple(booster.predict(X, pred_contrib=True).shape) == (300, 7)
    assert np.array_equal(before.cpu().numpy().view(np.uint32), booster.predict(X, pred_contrib=False).cpu().numpy().view(np.uint32))
    assert before.dtype == torch.float32 and np.array_equal(before.cpu().numpy().view(np.uint32), booster.scores.cpu().numpy().view(np.uint32))
    booster.update(booster.scores - dev(y), ones)
    with pytest.raises(RuntimeError, match="set_background"):               # the tables were built for one tree
        booster.predict(X, pred_contrib=True)
    with pytest.raises(ValueError, match="columns"):
        booster.set_background(X[:, :5])
    assert booster.feature_importance().sum() == sum(t["feature"].size for t in booster.trees)


def test_lambdamart_explains_its_scores():
    import ptranking_amd as pa
    rng = np.random.default_rng(11)
    group = rng.integers(5, 30, 30)
    n = int(group.sum())
    X = rng.standard_normal((n, 8)).astype(np.float32)
    y = np.clip(np.round(1.2 * X[:, 0] + 0.9 * X[:, 1] + 1), 0, 4).astype(np.float32)
    lm = pa.LambdaMART({"num_leaves": 8, "num_trees": 6, "min_data_in_leaf": 5, "learning_rate": 0.2})
    with pytest.raises(RuntimeError, match="fit"):
        lm.set_background(X)
    lm.fit(X, y, group)
    with pytest.raises(RuntimeError, match="set_background"):
        lm.predict(X, pred_contrib=True)
    assert lm.set_background(X) is lm
    phi = lm.predict(X[:65], pred_contrib=True).cpu().numpy()
    pred = lm.predict(X[:65]).cpu().numpy().astype(np.float64)
    assert phi.shape == (65, 9) and (np.abs(phi.sum(axis=1) - pred) <= local_accuracy_bound(lm.booster.trees, X[:65])).all()
    top = np.argsort(-np.abs(phi[:, :8]).mean(axis=0))[:2]
    assert set(top.tolist()) == {0, 1}                                      # the two features the labels were made of
    assert lm.booster.feature_importance()[top].min() > 0
