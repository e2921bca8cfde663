"""DART boosting on the device against plain numpy (tests/gbdt_dart_ref.py), bit for bit: no tolerances."""
import numpy as np
import pytest
import torch

import gbdt_dart_ref as D
from launch_form import launch_form
from test_gbdt_sample_gpu import bits, dev

pytestmark = pytest.mark.gpu
FIT = dict(num_leaves=8, learning_rate=0.2, drop_rate=0.5, drop_seed=5, min_data_in_leaf=5, max_bin=31)   # test_gbdt_dart_cpu.py: why seed 5
ROUNDS = 12


def same(got, want):
    """Equal bits, a NaN for a NaN (the sign and payload of a NaN are nobody's rule)."""
    got, want = np.asarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got), np.asarray(want)
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])


def forest(F, rng):
    """Trees in bin space (feature, bin, also, left, right, value): leaf-only, a stump, a chain of 40 nodes, one with also-left nodes (the
    bin 255), a chain of 600 nodes (above kDartLdsNodes) and a malformed one (a cycle)."""
    def chain(nn):
        return (rng.integers(0, F, nn), rng.integers(0, 200, nn), None, ~np.arange(nn), np.r_[np.arange(1, nn), ~nn], rng.standard_normal(nn + 1))
    trees = [(np.zeros(0, int), np.zeros(0, int), None, np.zeros(0, int), np.zeros(0, int), [0.375]),
             ([F - 1], [100], None, [~0], [~1], [-1.5, 2.25]), chain(40),
             (rng.integers(0, F, 3), [10, 60, 120], [255, 60, 255], [1, ~0, ~2], [2, ~1, ~3], rng.standard_normal(4)), chain(600),
             ([0, 0], [5, 5], None, [1, 0], [1, 0], [1.0, 2.0, 3.0])]
    return [tuple(np.asarray(a if a is not None else t[1]) for a in t[:5]) + (np.asarray(t[5], np.float32),) for t in trees]


@pytest.mark.parametrize("F", [1, 17, 136, 150])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_walk_equals_numpy_float32(n, F):
    from ptranking_amd import functional as Fn
    rng = np.random.default_rng(n * 1000 + F)
    trees = forest(F, rng)
    stride = (F + 15) // 16 * 16
    bins = np.zeros((n, stride), np.uint8)
    bins[:, :F] = rng.integers(0, 256, (n, F))
    bins[0, :F] = 255                                                    # a row of the largest bin: left at the also-left nodes alone
    kind, _, groups, _, lds_nodes, staged = launch_form("ptr_gbdt_dart_walk", n, F, 600)[:6]
    assert (kind, groups, lds_nodes, staged) == (2 if F == 150 else 1, -(-n // 256), 511, 0) and launch_form("ptr_gbdt_dart_walk", n, F, 511)[5] == 1
    nodes = dev(np.concatenate([Fn.gbdt_dart_pack(t[0], t[1], t[3], t[4], t[2]) for t in trees]))
    values = dev(np.concatenate([t[5] for t in trees]))
    offsets = dev(np.concatenate([[0], np.cumsum([len(t[0]) for t in trees])]).astype(np.int32))
    per_tree = [D.leaf_values(bins, F, t) for t in trees]
    assert not np.isnan(np.stack(per_tree[:5])).any() and np.isnan(per_tree[5]).all()
    start, dbins = rng.standard_normal(n).astype(np.float32), dev(bins)
    for lst in ([2], [3, 0], [4, 1, 2, 0, 3], [1, 5], [1, 99], []):      # k = 1, 2, 5; a malformed tree; an entry outside the forest; nothing
        for sign in (1, -1):
            want = D.walk(start, per_tree, lst, sign)
            assert np.isnan(want).all() == (lst[-1:] in ([5], [99]))
            got = Fn.gbdt_dart_walk(dev(start), dbins, F, nodes, values, offsets, dev(np.array(lst, np.int32)), sign, out=torch.empty(n, device="cuda"))
            assert same(got, want), (lst, sign)
            inplace = dev(start)
            assert Fn.gbdt_dart_walk(inplace, dbins, F, nodes, values, offsets, dev(np.array(lst, np.int32)), sign) is inplace
            assert same(inplace, want), (lst, sign)
    scaled = Fn.gbdt_dart_scale(values.clone(), offsets, dev(np.array([4, 1], np.int32)), 2.0 / 3.0)
    want = np.concatenate([D.scaled(t[5], 2.0 / 3.0) if i in (1, 4) else t[5] for i, t in enumerate(trees)])
    assert np.array_equal(bits(scaled), bits(want))


@pytest.mark.parametrize("skip_drop", [0.0, 1.0])
@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("T", [0, 1, 300])
def test_select_equals_the_restatement(T, uniform, skip_drop):
    from ptranking_amd import functional as Fn
    w = np.random.default_rng(T).random(T) + 0.05
    p = D.probabilities(w, 0.3, 50, uniform)
    for draw in (0, 7):
        sel = Fn.gbdt_dart_select(dev(p), 9, draw, skip_drop).cpu().numpy()
        want = D.select(p, 9, draw, skip_drop)
        assert sel[0] == len(want) and sel[1:1 + sel[0]].tolist() == want
        assert T < 300 or bool(want) == (skip_drop == 0.0)               # 300 trees at about 0.17 each: some are dropped unless the round is skipped


def squared_error_data(missing):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((600, 10)).astype(np.float32)
    y = (X[:, 0] + (X[:, 1] > 0.3) * 1.5 + X[:, 3] * X[:, 4] + 0.2 * rng.standard_normal(600)).astype(np.float32)
    if missing:
        X[rng.random(X.shape) < 0.1] = np.nan
    return X, y


def fit(params, X, y, twin=False):
    """ROUNDS rounds on the bare booster; per round (dropped, their values before, the tree lr, the factor, every tree's values after, the scores)."""
    import ptranking_amd as pa
    booster = pa.GBDT(params, boosting="dart").fit_bins(X)
    yd, rounds = dev(y), []
    want = D.replay_selection(ROUNDS, params["learning_rate"], params["drop_rate"], params.get("max_drop", 50), params.get("skip_drop", 0.5), False,
                              params["drop_seed"], params.get("xgboost_dart_mode", False))
    for r in range(ROUNDS):
        reads = booster.host_reads
        s = booster.begin_round()
        drop, lr, factor = want[r]
        assert booster.last_drop == tuple(drop) and booster.host_reads == reads + (1 if r else 0)     # the weights the restatement tracks alone
        before = {t: booster.trees[t]["value"].copy() for t in drop}
        grad, hess = s - yd, torch.ones_like(s)
        if twin:                                                         # born at the effective rate: the tree a 'gbdt' booster of that rate grows there
            other = pa.GBDT(dict(params, learning_rate=lr)).fit_bins(X)
            born = other.update(grad.clone(), hess.clone())
        tree = booster.update(grad, hess)
        if twin:
            assert all(np.array_equal(bits(np.asarray(tree[k], np.float32)), bits(np.asarray(born[k], np.float32))) for k in ("feature", "threshold", "left", "right", "value"))
        for t in drop:
            assert np.array_equal(bits(booster.trees[t]["value"]), bits(D.scaled(before[t], factor))), (r, t)
        rounds.append((drop, before, [t["value"].copy() for t in booster.trees], booster.scores.cpu().numpy()))
    with pytest.raises(RuntimeError, match="begin_round"):
        booster.update(grad, hess)
    return booster, rounds


def replay(rounds, leaf):
    """The scores after every round in numpy fp32 from the leaf indices [n, trees]: the dropped trees' old values leave (summed first, in
    list order), the new tree's leaf value is added, the rescaled values come back."""
    sc = np.zeros(leaf.shape[0], np.float32)
    for r, (drop, before, after, _) in enumerate(rounds):
        if drop:
            sc = D.walk(sc, [before[t][leaf[:, t]] if t in before else None for t in range(r)], drop, -1)
        sc = sc + after[r][leaf[:, r]]
        if drop:
            sc = D.walk(sc, [a[leaf[:, t]] for t, a in enumerate(after[:r])], drop, 1)
        yield sc


@pytest.mark.parametrize("case", ["plain", "bagging", "missing"])
def test_whole_fit_on_the_bare_booster(case):
    extra = {"bagging": dict(bagging_fraction=0.6, bagging_freq=1), "missing": dict(use_missing=True)}.get(case, {})
    X, y = squared_error_data(case == "missing")
    booster, rounds = fit(dict(FIT, **extra), X, y, twin=case != "bagging")
    ks = [len(r[0]) for r in rounds]
    assert 0 in ks[1:] and max(ks) >= 2
    leaf = booster.predict(X, pred_leaf=True).cpu().numpy()
    for r, sc in enumerate(replay(rounds, leaf)):
        assert np.array_equal(bits(sc), bits(rounds[r][3])), r
    again, rounds2 = fit(dict(FIT, **extra), X, y)
    assert np.array_equal(bits(again.scores), bits(booster.scores))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(rounds[-1][2], rounds2[-1][2]))


def test_skip_drop_one_is_gbdt_and_xgboost_mode_changes_the_factors():
    import ptranking_amd as pa
    X, y = squared_error_data(False)
    yd = dev(y)
    pair = [pa.GBDT(dict(FIT, skip_drop=1.0), boosting=b).fit_bins(X) for b in ("dart", "gbdt")]
    for _ in range(4):
        for b in pair:
            s = b.begin_round()
            b.update(s - yd, torch.ones_like(s))
    assert pair[0].last_drop == () and torch.equal(pair[0].scores, pair[1].scores)
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for a, b in zip(pair[0].trees, pair[1].trees) for k in a)
    fit(dict(FIT, skip_drop=0.0, xgboost_dart_mode=True), X, y, twin=True)                # its asserts use k / (k + lr) and lr / (lr + k)


def test_lambdamart_under_dart(tmp_path):
    import ptranking_amd as pa
    rng = np.random.default_rng(11)
    group, vgroup = np.full(30, 10), np.full(12, 10)
    X, Xv = rng.standard_normal((300, 6)).astype(np.float32), rng.standard_normal((120, 6)).astype(np.float32)
    y, yv = (np.clip(np.round(m[:, 0] + 0.5 * m[:, 1] + 1), 0, 4).astype(np.float32) for m in (X, Xv))
    params = dict(FIT, skip_drop=0.0, num_leaves=4)
    run = lambda r: pa.LambdaMART(params, boosting="dart").fit(X, y, group, eval_set=(Xv, yv), eval_group=vgroup, num_boost_round=r)
    models = [run(r) for r in range(1, 7)]                               # fits are deterministic: r rounds are the first r of r + 1
    last = models[-1]
    assert len(last.evals_result) == 6 and last.best_iteration is None and max(len(m.booster.last_drop) for m in models) >= 2
    values = [[t["value"] for t in m.booster.trees] for m in models]
    rounds = [(list(m.booster.last_drop), {t: values[r - 1][t] for t in m.booster.last_drop}, values[r], None) for r, m in enumerate(models)]
    for M, want in ((X, last.booster.scores), (Xv, last.valid_scores)):
        *_, sc = replay(rounds, last.predict(M, pred_leaf=True).cpu().numpy())
        assert np.array_equal(bits(sc), bits(want))
    with pytest.raises(ValueError, match="early_stopping_rounds"):
        pa.LambdaMART(params, boosting="dart").fit(X, y, group, eval_set=(Xv, yv), eval_group=vgroup, early_stopping_rounds=2)
    with pytest.raises(ValueError, match="categorical_feature"):
        pa.LambdaMART(dict(params, categorical_feature=[0]), boosting="dart")
    with pytest.raises(RuntimeError, match="begin_round"):
        pa.GBDT(params, boosting="dart").fit_bins(X).update(dev(y), dev(np.ones_like(y)))
    path = str(tmp_path / "dart.npz")
    last.booster.save_model(path)
    loaded = pa.GBDT.load_model(path)
    assert loaded.params["boosting_type"] == "dart" and torch.equal(loaded.predict(Xv), last.predict(Xv))
