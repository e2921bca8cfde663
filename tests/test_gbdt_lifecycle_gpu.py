"""GPU: a trained GBDT carried onto new data.  predict(pred_leaf=True), ptr_gbdt_leaf_sums and GBDT.refit against the numpy restatement
(tests/gbdt_lifecycle_ref.py); a fit split in two (train, save, load, continue) against the unsplit fit.  Every comparison is exact:
integers, or fp32 bits."""
import copy
import functools

import numpy as np
import pytest
import torch

import gbdt_lifecycle_ref as LR
from launch_form import launch_form

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257, 5000)
F_ = 8
BASE = {"learning_rate": 0.3, "num_leaves": 8, "min_data_in_leaf": 5, "max_bin": 63}
MODELS = {"plain": {}, "missing": {"use_missing": True}, "cat": {"categorical_feature": [1, 4], "cat_smooth": 1.0},
          "depthwise": {"grow_policy": "depthwise", "max_depth": 3}}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def data(kind, n, seed, codes=(8, 5)):
    """X [n, 8] on a grid of quarters and a target; 'cat': the columns 1 and 4 hold codes; 'missing': NaNs in every column but the last."""
    rng = np.random.default_rng([seed, len(kind)])
    X = (np.round(rng.standard_normal((n, F_)) * 4) / 4).astype(np.float32)
    if kind == "cat":
        X[:, 1], X[:, 4] = rng.integers(0, codes[0], n), rng.integers(0, codes[1], n)
    y = X[:, 0] * 1.5 - X[:, 2] + 0.7 * X[:, 0] * X[:, 3] + (np.isin(X[:, 1], (1, 2, 6)) * 2.0 if kind == "cat" else 0.5 * X[:, 1])
    if kind == "missing":
        X[:, :F_ - 1][rng.random((n, F_ - 1)) < 0.15] = np.nan
    return X, (y + 0.3 * rng.standard_normal(n)).astype(np.float32)


def squared_error(y):
    yd = dev(y)
    return lambda scores: (scores - yd, torch.ones_like(scores))


def grow(params, X, y, rounds, init_model=None):
    import ptranking_amd as pa
    booster = pa.GBDT(params).fit_bins(X, **({} if init_model is None else {"init_model": init_model}))
    gh = squared_error(y)
    for _ in range(rounds):
        booster.update(*gh(booster.scores))
    return booster


def is_cat_of(booster):
    cats = booster.params["categorical_feature"]
    if not cats:
        return None
    m = np.zeros(F_, np.uint8)
    m[list(cats)] = 1
    return m


@functools.lru_cache(maxsize=None)
def fitted(kind):
    """-> (booster of 6 trees on 600 rows, X, y)."""
    X, y = data(kind, 600, 1)
    booster = grow(dict(BASE, **MODELS[kind]), X, y, 6)
    assert len(booster.trees) == 6 and all(2 <= t["value"].size <= 8 for t in booster.trees)
    return booster, X, y


def with_unsplit_tree(booster, at=2):
    """A copy of the booster with a tree that never split (no node, one leaf) among its trees."""
    stub = {"feature": np.zeros(0, np.int32), "threshold": np.zeros(0, np.float32), "left": np.zeros(0, np.int32), "right": np.zeros(0, np.int32),
            "value": np.array([0.125], np.float32)}
    if booster.params["use_missing"]:
        stub["default_left"] = np.zeros(0, np.uint8)
    if booster.params["categorical_feature"]:
        stub["cat_index"], stub["cat_set"] = np.zeros(0, np.int32), np.zeros((0, 4), np.int64)
    new = copy.copy(booster)
    new.trees = booster.trees[:at] + [stub] + booster.trees[at:]
    new._flat = new._shap = None
    return new


@functools.lru_cache(maxsize=None)
def leaf_case(kind):
    """-> (booster with an unsplit tree, 5000 evaluation rows, the restatement's leaf indices on them)."""
    booster, X, _ = fitted(kind)
    booster = with_unsplit_tree(booster)
    Xe = np.concatenate([X[:100], data(kind, max(SIZES) - 100, 2, codes=(12, 9))[0]])      # 'cat': codes the training data never held
    want = LR.pred_leaf(booster.trees, Xe, is_cat_of(booster))
    want.setflags(write=False)
    return booster, Xe, want


# ---------------------------------------------------------------- pred_leaf
@pytest.mark.parametrize("kind", list(MODELS))
def test_pred_leaf_equals_the_restatement(kind):
    booster, Xe, want = leaf_case(kind)
    assert want.min() >= 0 and (want[:, 2] == 0).all() and want.max() >= 3
    if kind == "missing":
        assert np.isnan(Xe).any() and any(t["default_left"].any() for t in booster.trees)
    if kind == "cat":
        assert any((t["cat_index"] >= 0).any() for t in booster.trees) and Xe[:, 1].max() > 7
    for n in SIZES:
        got = booster.predict(Xe[:n], pred_leaf=True)
        assert got.dtype == torch.int32 and tuple(got.shape) == (n, 7) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want[:n]), (kind, n)
        # value[leaf] summed in tree order in fp32 is predict, bit for bit
        assert np.array_equal(bits(LR.sum_leaf_values(booster.trees, want[:n])), bits(booster.predict(Xe[:n]))), (kind, n)


@pytest.mark.parametrize("kind", list(MODELS))
def test_pred_leaf_slices_the_trees_as_predict_does(kind):
    booster, Xe, want = leaf_case(kind)
    X = Xe[:300]
    for first, stop in ((0, 7), (2, 5), (2, 3), (3, 3), (6, 7), (0, 1)):
        got = booster.predict(X, num_iteration=stop, first_tree=first, pred_leaf=True)
        assert tuple(got.shape) == (300, stop - first) and np.array_equal(got.cpu().numpy(), want[:300, first:stop]), (first, stop)
    assert np.array_equal(booster.predict(X, num_iteration=4, pred_leaf=True).cpu().numpy(), want[:300, :4])
    early = copy.copy(booster)
    early.best_iteration = 3                                               # the default stop is predict's: up to best_iteration
    assert np.array_equal(early.predict(X, pred_leaf=True).cpu().numpy(), want[:300, :3])
    with pytest.raises(ValueError):
        booster.predict(X, num_iteration=8, pred_leaf=True)


def test_lambdamart_forwards_pred_leaf():
    rk, X, _, _ = ranker("lambdarank")
    assert torch.equal(rk.predict(X, pred_leaf=True), rk.booster.predict(X, pred_leaf=True))
    assert tuple(rk.predict(X, num_iteration=2, pred_leaf=True).shape) == (X.shape[0], 2)


# ---------------------------------------------------------------- leaf_sums on hand-built chains
BUDGET = 1024                                                              # asserted against ptr_launch_form below


def lossy(t):
    """The chain with nodes that lose rows: a leaf the tree does not have at node 3, a feature out of range at the last node."""
    t = {k: np.array(v) for k, v in t.items()}
    nn = t["feature"].size
    if nn > 3:
        t["left"][3] = ~(nn + 7)
    if nn > 1:
        t["feature"][nn - 1] = 5
    return t


def run_leaf_sums(t, X, qg, qh, nleaves=None):
    import ptranking_amd.functional as F
    leaf, sums = F.gbdt_leaf_sums(dev(X), dev(t["feature"]), dev(t["threshold"]), dev(t["left"]), dev(t["right"]), qg, qh, nleaves)
    return leaf.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("nleaves", (1, 2, 31, BUDGET, BUDGET + 1))
def test_leaf_sums_equal_the_restatement_on_each_side_of_the_form_boundary(nleaves):
    assert launch_form("ptr_gbdt_leaf_sums", 1, 1)[4] == BUDGET
    rng = np.random.default_rng(nleaves)
    for n in (1, 255, 1024, 1025, 5000):                                   # one workgroup up to 1024 rows, two from 1025
        kind, _, groups = launch_form("ptr_gbdt_leaf_sums", n, nleaves)[:3]
        assert kind == (1 if nleaves <= BUDGET else 2) and groups == -(-n // 1024)
        X = rng.uniform(-2.0, (nleaves - 1) * 0.25 + 2.0, (n, 1)).astype(np.float32)
        qg = torch.randint(-2 ** 30, 2 ** 30, (n,), device="cuda", dtype=torch.int32)
        qh = torch.randint(0, 2 ** 30, (n,), device="cuda", dtype=torch.int32)
        for t in (LR.chain_tree(nleaves, step=0.25), lossy(LR.chain_tree(nleaves, step=0.25))):
            want_leaf = LR.leaf_index_numeric(t, X)
            want = LR.leaf_sums(want_leaf, qg.cpu().numpy(), qh.cpu().numpy(), nleaves)
            leaf, sums = run_leaf_sums(t, X, qg, qh)
            assert leaf.dtype == np.int32 and sums.dtype == np.int64 and sums.shape == (nleaves, 3)
            assert np.array_equal(leaf, want_leaf) and np.array_equal(sums, want), (nleaves, n)
            again = run_leaf_sums(t, X, qg, qh)
            assert np.array_equal(again[0], leaf) and np.array_equal(again[1], sums)
        if nleaves > 3 and n >= 255:
            assert (want_leaf < 0).any() and (want_leaf >= 0).any()       # the lossy chain lost rows and kept others
    # fewer cells than leaves: the rows of the leaves beyond are lost, on each side of the boundary too
    if nleaves > 2:
        t = LR.chain_tree(nleaves, step=0.25)
        want_leaf = LR.leaf_index_numeric(t, X, nleaves=nleaves - 1)
        leaf, sums = run_leaf_sums(t, X, qg, qh, nleaves - 1)
        assert np.array_equal(leaf, want_leaf) and np.array_equal(sums, LR.leaf_sums(want_leaf, qg.cpu().numpy(), qh.cpu().numpy(), nleaves - 1))


@pytest.mark.parametrize("n", (1024 * 1024, 1024 * 1024 + 1))
def test_leaf_sums_at_the_grid_cap(n):
    """1024 workgroups serve 1024 x 1024 rows at 1024 rows each; one more row and each takes more, the grid stays."""
    assert launch_form("ptr_gbdt_leaf_sums", n, 31)[2] == 1024 == launch_form("ptr_gbdt_leaf_sums", 2 * n, 31)[2]
    assert launch_form("ptr_gbdt_leaf_sums", 1023 * 1024, 31)[2] == 1023       # below the cap the grid still follows n
    g = torch.Generator(device="cuda").manual_seed(n)
    Xd = torch.rand((n, 1), device="cuda", generator=g) * 9.0 - 1.0
    qg = torch.randint(-2 ** 30, 2 ** 30, (n,), device="cuda", dtype=torch.int32, generator=g)
    qh = torch.randint(0, 2 ** 30, (n,), device="cuda", dtype=torch.int32, generator=g)
    t = lossy(LR.chain_tree(31, step=0.25))
    X = Xd.cpu().numpy()
    want_leaf = LR.leaf_index_numeric(t, X)
    leaf, sums = run_leaf_sums(t, X, qg, qh)
    assert np.array_equal(leaf, want_leaf) and np.array_equal(sums, LR.leaf_sums(want_leaf, qg.cpu().numpy(), qh.cpu().numpy(), 31))
    assert np.array_equal(run_leaf_sums(t, X, qg, qh)[1], sums)


def test_add_by_leaf_skips_what_is_no_leaf():
    import ptranking_amd.functional as F
    rng = np.random.default_rng(3)
    for n in (1, 255, 257, 3000):
        leaf = rng.integers(-2, 7, n).astype(np.int32)                     # -2, -1, 5 and 6 are no leaves of five values
        values, scores = rng.standard_normal(5).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        hit = (leaf >= 0) & (leaf < 5)
        want = scores.copy()
        want[hit] = (scores[hit] + values[leaf[hit]]).astype(np.float32)
        got = F.gbdt_add_by_leaf(dev(scores), dev(leaf), dev(values))
        assert np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------- a split fit equals a whole fit
SPLIT = {"leafwise": ("plain", {}), "depthwise": ("plain", {"grow_policy": "depthwise", "max_depth": 3}),
         "missing": ("missing", {"use_missing": True}), "cat": ("cat", {"categorical_feature": [1, 4], "cat_smooth": 1.0}),
         "bagging": ("plain", {"bagging_fraction": 0.7, "bagging_freq": 2}),
         "goss": ("plain", {"data_sample_strategy": "goss", "top_rate": 0.3, "other_rate": 0.2})}
T1, T2 = 3, 4             # tree 3, the first of the second part, is GOSS's first sampled tree (floor(1 / 0.3) = 3) and sits inside bagging draw 1


def assert_same_trees(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert sorted(a) == sorted(b)
        for k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("name", list(SPLIT))
def test_a_split_fit_equals_the_whole_fit(name, tmp_path):
    import ptranking_amd as pa
    kind, extra = SPLIT[name]
    params = dict(BASE, **extra)
    X, y = data(kind, 2000, 7)
    whole = grow(params, X, y, T1 + T2)
    first = grow(params, X, y, T1)
    path = str(tmp_path / "first.npz")
    first.save_model(path)
    loaded = pa.GBDT.load_model(path)
    for init in (path, loaded):
        second = grow(params, X, y, T2, init_model=init)
        assert len(second.trees) == T1 + T2 and second.best_iteration is None
        assert_same_trees(second.trees, whole.trees)
        assert np.array_equal(bits(second.scores), bits(whole.scores))
        assert np.array_equal(bits(second.predict(X)), bits(second.scores))
        assert np.array_equal(second.edges, whole.edges) and np.array_equal(second.nbins, whole.nbins)
    assert len(loaded.trees) == T1 and len(first.trees) == T1              # the initial model is copied, not grown
    if name in ("bagging", "goss"):
        assert any(not np.array_equal(a["value"], b["value"]) for a, b in zip(whole.trees[T1:], grow(dict(BASE), X, y, T1 + T2).trees[T1:]))   # the sampling bit
    # the continued model saves in the format its kind always had, and loads to the same predictions
    again = str(tmp_path / "second.npz")
    second.save_model(again)
    with np.load(path) as a, np.load(again) as b:
        assert int(a["format"]) == int(b["format"]) and sorted(a.files) == sorted(b.files)
    assert np.array_equal(bits(pa.GBDT.load_model(again).predict(X)), bits(whole.scores))


def test_continued_training_takes_the_trees_predict_uses():
    booster, X, y = fitted("plain")
    early = copy.copy(booster)
    early.best_iteration = 4
    second = grow(dict(BASE), X, y, 1, init_model=early)
    assert len(second.trees) == 5 and second.best_iteration is None
    assert_same_trees(second.trees[:4], booster.trees[:4])
    second.trees[0]["value"][:] = 0                                        # its trees are its own
    assert booster.trees[0]["value"].any()


def queries(seed, nq):
    rng = np.random.default_rng(seed)
    group = rng.integers(15, 35, nq)
    n = int(group.sum())
    X = (np.round(rng.standard_normal((n, F_)) * 4) / 4).astype(np.float32)
    rel = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.5 * rng.standard_normal(n)
    return X, np.clip(np.round(rel + 1.5), 0, 4).astype(np.float32), group


@pytest.mark.parametrize("objective", ("lambdarank", "lambdarank_ndcg"))
def test_lambdamart_continues_with_an_eval_set(objective, tmp_path):
    import ptranking_amd as pa
    params = dict(BASE, min_data_in_leaf=10)
    X, y, group = queries(1, 40)
    Xv, yv, gv = queries(2, 20)
    fit = lambda rounds, **kw: pa.LambdaMART(params, objective=objective).fit(X, y, group, eval_set=(Xv, yv), eval_group=gv, num_boost_round=rounds, **kw)
    whole = fit(T1 + T2, early_stopping_rounds=50)
    first = fit(T1)
    assert first.best_iteration is None and len(first.evals_result) == T1
    path = str(tmp_path / "rk.npz")
    first.booster.save_model(path)
    for init in (first, path, first.booster):
        second = fit(T2, early_stopping_rounds=50, init_model=init)
        assert_same_trees(second.booster.trees, whole.booster.trees)
        assert np.array_equal(bits(second.booster.scores), bits(whole.booster.scores))
        assert second.evals_result == whole.evals_result[T1:] and first.evals_result == whole.evals_result[:T1]
        assert second.best_iteration == T1 + 1 + int(np.argmax(second.evals_result)) == second.booster.best_iteration      # in total trees
        assert np.array_equal(bits(second.predict(Xv)), bits(whole.predict(Xv, num_iteration=second.best_iteration)))
    assert len(first.booster.trees) == T1


# ---------------------------------------------------------------- refit
@pytest.mark.parametrize("kind", list(MODELS))
def test_refit_on_the_training_data_with_decay_zero_returns_every_leaf_value(kind):
    booster, X, y = fitted(kind)
    before, reads = copy.deepcopy(booster.trees), booster.host_reads
    new = booster.refit(X, squared_error(y), decay_rate=0)
    assert new is not booster and len(new.trees) == 6
    assert_same_trees(new.trees, booster.trees)                            # structures and, bit for bit, values
    assert all(a["value"] is not b["value"] for a, b in zip(new.trees, booster.trees))
    assert np.array_equal(bits(new.scores), bits(booster.scores)) and np.array_equal(bits(new.predict(X)), bits(new.scores))
    assert new.host_reads == reads + 6 and booster.host_reads == reads
    assert_same_trees(booster.trees, before)
    assert new.params == booster.params and np.array_equal(new.edges, booster.edges)


@pytest.mark.parametrize("kind", list(MODELS))
def test_refit_on_other_data_equals_the_restatement(kind):
    booster, X, _ = fitted(kind)
    booster = with_unsplit_tree(booster)
    X2, y2 = data(kind, 300, 9)
    X2[:, 0] = np.abs(np.nan_to_num(X2[:, 0])) + 0.5                       # half of feature 0's range is empty: leaves no row reaches
    before = copy.deepcopy(booster.trees)
    new = booster.refit(X2, squared_error(y2), decay_rate=0.9)
    p = booster.params
    values, scores = LR.refit(booster.trees, X2, lambda s: ((s - y2).astype(np.float32), np.ones_like(s)), p["lambda_l2"], p["learning_rate"], 0.9,
                              is_cat_of(booster))
    leaves = LR.pred_leaf(booster.trees, X2, is_cat_of(booster))
    unreached = moved = 0
    for k, (t, old, v) in enumerate(zip(new.trees, before, values)):
        assert t["value"].dtype == np.float32 and t["value"].tobytes() == v.tobytes(), (kind, k)
        for l in set(range(v.size)) - set(leaves[:, k].tolist()):
            unreached += 1
            assert t["value"][l].tobytes() == old["value"][l].tobytes()   # an unreached leaf keeps its value
        moved += int((t["value"] != old["value"]).sum())
        for key in old:
            if key != "value":
                assert np.array_equal(t[key], old[key])
    assert unreached > 0 and moved > 0
    assert np.array_equal(bits(new.scores), bits(scores)) and np.array_equal(bits(new.predict(X2)), bits(new.scores))
    assert_same_trees(booster.trees, before)                               # self is unchanged
    assert new.host_reads == booster.host_reads + 7


def test_refit_raises_on_gradients_that_are_not_finite():
    booster, X, y = fitted("plain")
    with pytest.raises(FloatingPointError):
        booster.refit(X, lambda s: (torch.full_like(s, float("nan")), torch.ones_like(s)))


@functools.lru_cache(maxsize=None)
def ranker(objective):
    import ptranking_amd as pa
    X, y, group = queries(1, 40)
    return pa.LambdaMART(dict(BASE, min_data_in_leaf=10), objective=objective).fit(X, y, group, num_boost_round=4), X, y, group


@pytest.mark.parametrize("objective", ("lambdarank", "lambdarank_ndcg"))
def test_lambdamart_refit(objective):
    import ptranking_amd as pa
    rk, X, y, group = ranker(objective)
    before = copy.deepcopy(rk.booster.trees)
    X2, y2, g2 = queries(5, 30)
    new = rk.refit(X2, y2, g2, decay_rate=0.5)
    assert isinstance(new, pa.LambdaMART) and new is not rk and new.booster is not rk.booster and new.objective == objective
    assert np.array_equal(bits(new.booster.scores), bits(new.predict(X2))) and new.booster.scores.shape[0] == X2.shape[0]
    assert_same_trees(rk.booster.trees, before)
    assert any(not np.array_equal(a["value"], b["value"]) for a, b in zip(new.booster.trees, before))
    for a, b in zip(new.booster.trees, before):
        assert all(np.array_equal(a[k], b[k]) for k in b if k != "value")
    same = rk.refit(X, y, group, decay_rate=0)                             # its own data and objective: its own values
    assert_same_trees(same.booster.trees, before)


# ---------------------------------------------------------------- what continued training refuses
def test_a_code_above_the_models_largest_raises():
    booster, X, y = fitted("cat")
    bad = X.copy()
    bad[3, 1] = 8                                                          # the training codes of column 1 are 0 .. 7
    with pytest.raises(ValueError, match="largest"):
        grow(dict(BASE, **MODELS["cat"]), bad, y, 0, init_model=booster)
    ok = X.copy()
    ok[3, 1] = 7
    assert len(grow(dict(BASE, **MODELS["cat"]), ok, y, 0, init_model=booster).trees) == 6


def test_a_nan_where_the_model_keeps_no_nan_bin_raises():
    booster, X, y = fitted("missing")
    assert booster.nan_bin[F_ - 1] == -1 and (booster.nan_bin[:F_ - 1] >= 0).all()
    bad = X.copy()
    bad[5, F_ - 1] = np.nan
    with pytest.raises(ValueError, match="nan_bin"):
        grow(dict(BASE, **MODELS["missing"]), bad, y, 0, init_model=booster)
    plain, Xp, yp = fitted("plain")
    bad = Xp.copy()
    bad[5, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):                           # without use_missing a NaN raises as it always did
        grow(dict(BASE), bad, yp, 0, init_model=plain)
