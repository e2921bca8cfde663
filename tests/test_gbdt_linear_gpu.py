"""Linear trees on the device (csrc/gbdt_linear.hip) against the float64 restatement tests/gbdt_linear_ref.py: the moments under a derived
bound, the solve under the residual bound, the leaf output within fp32 ulps, whole fits, and LambdaMART."""
import numpy as np
import pytest
import torch

import gbdt_linear_ref as L
from test_gbdt_sample_gpu import bits, dev

pytestmark = pytest.mark.gpu
FIT = dict(num_leaves=6, learning_rate=0.5, max_bin=63, min_data_in_leaf=5, linear_tree=True)
ROUNDS = 5
ROWS, KS, R1 = (1, 3, 4, 5, 63, 65, 257), (1, 15, 16, 17, 30), 1024 + 1
# every k at two row counts, every row count at two k: the MFMA's four-row step, a wave boundary, a chunk boundary, the 16-column block, the cap
MOMENT_CASES = sorted({(m, k) for k in KS for m in (5, 257)} | {(m, k) for m in ROWS + (R1,) for k in (1, 17)})


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("m,k", MOMENT_CASES)
def test_moments_within_the_derived_bound(m, k, nan):
    from ptranking_amd import functional as Fn
    assert Fn.GBDT_LINEAR_CHUNK_ROWS + 1 == R1 and Fn.GBDT_LINEAR_MAX_FEATURES == L.K
    rng = np.random.default_rng(1000 * m + k)
    counts, F = (m, m + 2), 40
    n = sum(counts) + 7
    X = rng.standard_normal((n, F)).astype(np.float32)
    g, h = rng.standard_normal(n).astype(np.float32), (0.25 + rng.random(n)).astype(np.float32)
    rows = rng.permutation(n)[:sum(counts)].astype(np.int32)              # a shuffled row list, two leaves
    offsets = np.array([0, m, sum(counts)])
    P = [rng.permutation(F)[:k].tolist(), rng.permutation(F)[:k].tolist()]
    if nan:
        X[rows[::3], P[0][0]] = np.nan                                     # every third entry of the list is unusable in leaf 0 ...
        X[rows[m + 1], P[1][-1]] = np.nan                                  # ... and one row of leaf 1, in its last regressor
    feats = np.full((2, L.K), -1, np.int32)
    feats[0, :k], feats[1, :k] = P
    items, item_offsets = Fn.gbdt_linear_items(offsets, [k, k])
    assert item_offsets.tolist() == [0, -(-m // 1024), -(-m // 1024) + -(-(m + 2) // 1024)]
    args = (dev(X), dev(rows), dev(items), dev(feats), dev(np.array([k, k], np.int32)), dev(g), dev(h))
    ws, usable = Fn.gbdt_linear_moments(*args)
    again = Fn.gbdt_linear_moments(*args)
    ws, usable = ws.cpu().numpy(), usable.cpu().numpy()
    for l in range(2):
        seg = rows[offsets[l]:offsets[l + 1]]
        A, b, m_u, absA, absb = L.moments(X, seg, P[l], g, h, np.longdouble)
        part = ws[item_offsets[l]:item_offsets[l + 1]].sum(0)
        assert usable[item_offsets[l]:item_offsets[l + 1]].sum() == m_u and (m_u < seg.size) == (nan and (l == 1 or m > 0))
        upper = np.triu(np.ones((k + 1, k + 1), bool))
        bound = (seg.size + 2) * 2.0 ** -53
        assert (np.abs(part[:k + 1, :k + 1] - A)[upper] <= (bound * absA)[upper]).all(), np.abs(part[:k + 1, :k + 1] - A).max()
        assert (np.abs(part[:k + 1, k + 1] - b) <= bound * absb).all()
    same = np.triu(np.ones((32, 32), bool))[None] & (np.arange(32)[None, None, :] <= k + 1) & (np.arange(32)[None, :, None] <= k)
    assert np.array_equal(again[0].cpu().numpy()[np.broadcast_to(same, ws.shape)].view(np.int64), ws[np.broadcast_to(same, ws.shape)].view(np.int64))
    assert np.array_equal(again[1].cpu().numpy(), usable)


def solve_on(systems, lam, lr=0.1):
    from ptranking_amd import functional as Fn
    ws, usable, item_offsets, nfeat = L.workspace(systems)
    return [t.cpu().numpy() for t in Fn.gbdt_linear_solve(dev(ws), dev(usable), dev(item_offsets), dev(nfeat), lam, lr)]


@pytest.mark.parametrize("k,lam", L.SOLVE_CASES)
def test_solve_within_the_residual_bound(k, lam):
    A, b, m_u = L.solve_case(k, lam)
    lr = 0.1
    coeff, const, status, mu = solve_on([(A, b, m_u, k)], lam, lr)
    assert status.tolist() == [0] and mu.tolist() == [m_u] and (coeff[0, k:] == 0).all()
    c = np.r_[coeff[0, :k], const[0]] / lr
    factor = L.residual_factor(A, b, k, lam, c)
    print("residual factor", k, lam, factor)
    assert factor <= L.GAMMA


def test_solve_falls_back_by_the_rule():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((40, 4)).astype(np.float32)
    g, h, every = rng.standard_normal(40).astype(np.float32), np.ones(40, np.float32), np.arange(40)
    Xc = X.copy()
    Xc[:, 2] = 1.0                                                          # constant over the leaf
    Xn = np.full_like(X, np.nan)                                            # all rows unusable
    good = L.moments(X, every, [0, 1, 2], g, h)[:3] + (3,)
    systems = [good, L.moments(Xc, every, [0, 1, 2], g, h)[:3] + (3,), L.moments(X, every[:3], [0, 1, 2], g, h)[:3] + (3,),
               L.moments(Xn, every, [0, 1], g, h)[:3] + (2,), (np.zeros((1, 1)), np.zeros(1), 40, 0), (np.zeros((31, 31)), np.zeros(31), 40, 30)]
    for s in systems[:4]:
        st, ratio = L.solve(*s[:2], s[3], s[2], 0.0)[1:]
        assert ratio > 2.0 ** -20 or ratio < 2.0 ** -45 or st == 3          # no decision sits near the floor
    ws, usable, item_offsets, nfeat = L.workspace(systems)
    nfeat[5] = 31                                                           # a slot holds 30 regressors: k = 31 is reported from nfeat alone
    from ptranking_amd import functional as Fn
    coeff, const, status, mu = [t.cpu().numpy() for t in Fn.gbdt_linear_solve(dev(ws), dev(usable), dev(item_offsets), dev(nfeat), 0.0, 0.1)]
    assert status.tolist() == [0, 4, 3, 3, 1, 2] and mu[2:4].tolist() == [3, 0] and not coeff[1:].any() and not const[1:].any() and coeff[0, :3].all()


def forest(F):
    """Three hand-made trees over F features under use_missing: two linear leaves on one feature; a depth-2 tree with a two-feature linear
    leaf, a one-feature one and a constant leaf; a stump whose right leaf regresses on the last feature, NaN in some rows."""
    a, b, z = 0, F - 1, np.zeros
    lf = lambda rows: np.array([r + [-1] * (L.K - len(r)) for r in rows], np.int32)
    lc = lambda rows: np.array([r + [0.0] * (L.K - len(r)) for r in rows], np.float64)
    return [{"feature": np.array([a], np.int32), "threshold": np.array([0.1], np.float32), "left": np.array([~0], np.int32), "right": np.array([~1], np.int32),
             "default_left": np.array([1], np.uint8), "value": np.array([0.5, -0.25], np.float32), "leaf_features": lf([[a], [a]]),
             "leaf_coeff": lc([[0.3], [-1.7]]), "leaf_const": np.array([0.125, 2.0])},
            {"feature": np.array([b, a], np.int32), "threshold": np.array([-0.2, 0.6], np.float32), "left": np.array([1, ~0], np.int32),
             "right": np.array([~2, ~1], np.int32), "default_left": np.array([0, 1], np.uint8), "value": np.array([1.5, -2.5, 0.75], np.float32),
             "leaf_features": lf([[b, a], [], [b]]), "leaf_coeff": lc([[0.11, -0.07], [], [1e-3]]), "leaf_const": np.array([-0.4, 0.0, 3.0])},
            {"feature": np.array([a], np.int32), "threshold": np.array([-0.5], np.float32), "left": np.array([~0], np.int32), "right": np.array([~1], np.int32),
             "default_left": np.array([0], np.uint8), "value": np.array([0.0625, -0.875], np.float32), "leaf_features": lf([[], [b]]),
             "leaf_coeff": lc([[], [0.9]]), "leaf_const": np.array([0.0, -0.3])}]


@pytest.mark.parametrize("F", [1, 17, 136])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_leaf_output_and_predict_within_fp32_ulps(n, F):
    from ptranking_amd import functional as Fn
    rng = np.random.default_rng(n + F)
    X = rng.standard_normal((n, F)).astype(np.float32)
    X[::4, F - 1] = np.nan
    trees = forest(F)
    fl = {k: dev(v) for k, v in L.flat(trees).items()}
    call = lambda first, stop: Fn.gbdt_predict_linear(dev(X), fl["feature"], fl["threshold"], fl["left"], fl["right"], fl["value"], fl["tree_offsets"],
                                                      fl["leaf_features"], fl["leaf_coeff"], fl["leaf_const"], first, stop,
                                                      default_left=fl["default_left"]).cpu().numpy().astype(np.float64)
    outs = [L.tree_outputs(X, t) for t in trees]
    for t, want in enumerate(outs):
        assert (np.abs(call(t, t + 1) - want) <= np.spacing(np.abs(want).astype(np.float32))).all(), t
    terms = np.abs(np.stack(outs)).sum(0)
    assert (np.abs(call(0, 3) - np.stack(outs).sum(0)) <= (len(trees) + 1) * np.spacing(terms.astype(np.float32))).all()
    scores = dev(rng.standard_normal(n).astype(np.float32))
    start = scores.clone()
    t = {k: dev(v) for k, v in trees[1].items()}
    Fn.gbdt_add_tree_linear(scores, dev(X), t["feature"], t["threshold"], t["left"], t["right"], t["value"], t["leaf_features"], t["leaf_coeff"],
                            t["leaf_const"], default_left=t["default_left"])
    assert np.array_equal(bits(scores), bits(start + dev(call(1, 2).astype(np.float32))))      # training adds what predict gives


def fit_data(missing, n=600, F=6):
    rng = np.random.default_rng(11)
    X = rng.standard_normal((n, F)).astype(np.float32)
    y = (np.where(X[:, 0] > 0, 2.0 * X[:, 1] + 1.0, -1.5 * X[:, 2]) + np.where(X[:, 3] > 0.5, X[:, 0], 0.0)).astype(np.float32)
    if missing:
        X[rng.random((n, F)) < 0.05] = np.nan
    return X, y


CASES = {"plain": {}, "bagging": dict(bagging_fraction=0.6, bagging_freq=2), "goss": dict(data_sample_strategy="goss", top_rate=0.3, other_rate=0.3),
         "missing": dict(use_missing=True), "depthwise": dict(grow_policy="depthwise"), "quantized": dict(use_quantized_grad=True, num_grad_quant_bins=16)}


def fit(params, X, y, check=None):
    from ptranking_amd import gbdt
    b = gbdt.GBDT(params).fit_bins(X)
    yd = dev(y)
    for _ in range(ROUNDS):
        g, h = b.scores - yd, torch.ones_like(yd)
        b.update(g, h)
        if check is not None:
            check(b, g, h)
    return b


@pytest.mark.parametrize("case", sorted(CASES))
def test_whole_fits(case, tmp_path):
    """The restatement's moments are summed in extended precision and rounded once to float64.  Plain float64 numpy sums are not exact
    enough to be the reference here: on one leaf of the `plain` fit (k = 1, 353 rows) they are off by 4.8e-13 in sum x^2, the kernel's by
    1.4e-13, and the solution of the EXACT moments misses the residual bound on numpy's float64 moments (factor 2.7 against 1.2)."""
    from ptranking_amd import gbdt
    params = dict(FIT, **CASES[case])
    X, y = fit_data(case == "missing")
    seen, factors = [], []

    def check(b, g, h):
        """The last tree's fits against the restatement on the rows it assigns: the bag, walked down the tree; the pair quantization got."""
        t, p = b.trees[-1], b.params
        sampled = gbdt.sampling(p) and not (gbdt.sampling(p) == "goss" and len(b.trees) - 1 < int(1.0 / p["learning_rate"]))
        bag = np.nonzero(b._mask.cpu().numpy())[0] if sampled else np.arange(len(X))
        if sampled and gbdt.sampling(p) == "goss":
            g, h = b._gg, b._gh
        g, h, leaf = g.cpu().numpy(), h.cpu().numpy(), L.assign(X[bag], t)
        for l, P in enumerate(L.path_features(t)):
            A, bb, m_u = L.moments(X, bag[leaf == l], P, g, h, np.longdouble)[:3]      # summed in extended precision, then rounded once:
            A, bb = np.asarray(A, np.float64), np.asarray(bb, np.float64)             # numpy's own float64 sums err by more than the bound
            c, status, ratio = L.solve(A, bb, len(P), m_u, 0.0)
            assert ratio > 2.0 ** -20 or ratio < 2.0 ** -45, (l, ratio)      # the decision does not sit near the floor
            assert b.last_linear_status[l] == status, (l, status, b.last_linear_status)
            seen.append(status)
            if status == 0:
                got = np.r_[t["leaf_coeff"][l, :len(P)], t["leaf_const"][l]] / p["learning_rate"]
                assert t["leaf_features"][l, :len(P)].tolist() == P
                factors.append(float(L.residual_factor(A, bb, len(P), 0.0, got)))
            else:
                assert (t["leaf_features"][l] == -1).all()

    b = fit(params, X, y, check)
    const = fit(dict(params, linear_tree=False), X, y)
    assert 0 in seen and torch.equal(b.scores, b.predict(X)) and b.host_reads == const.host_reads + ROUNDS
    assert b.predict(X, pred_leaf=True).shape == (len(X), ROUNDS)
    path = tmp_path / "m.npz"
    b.save_model(path)
    loaded = gbdt.GBDT.load_model(path)
    assert int(np.load(path)["format"]) == 4 and loaded.params["linear_tree"] and torch.equal(loaded.predict(X), b.scores)
    const.save_model(path)
    assert int(np.load(path)["format"]) == (2 if case == "missing" else 1) and "linear_tree" not in str(np.load(path)["params"])
    loss = lambda s: float(((s.cpu().numpy() - y) ** 2).mean())
    print(case, "loss linear", loss(b.scores), "constant", loss(const.scores))
    assert loss(b.scores) < loss(const.scores)
    print(case, "worst residual factor on the restatement's moments", max(factors), "of", len(factors), "fitted leaves; bound", L.GAMMA)
    assert max(factors) <= L.GAMMA


def test_lambdamart_trains_predicts_and_continues(tmp_path):
    from ptranking_amd import gbdt
    rng = np.random.default_rng(2)
    group = np.array([20] * 12)
    X = rng.standard_normal((240, 5)).astype(np.float32)
    y = np.clip(np.round(X[:, 0] + 0.5 * X[:, 1] + 1.0), 0, 4).astype(np.float32)
    params = dict(num_leaves=4, learning_rate=0.3, min_data_in_leaf=5, max_bin=31, num_trees=4, linear_tree=True, linear_lambda=1.0)
    m = gbdt.LambdaMART(params).fit(X, y, group, eval_set=(X[:100], y[:100]), eval_group=group[:5])
    assert len(m.evals_result) == 4 and np.isfinite(m.evals_result).all() and torch.equal(m.predict(X), m.booster.scores)
    assert torch.equal(m.valid_scores, m.predict(X[:100]))
    assert any((t["leaf_features"] >= 0).any() for t in m.booster.trees)
    path = tmp_path / "m.npz"
    m.booster.save_model(path)
    more = gbdt.LambdaMART(params).fit(X, y, group, num_boost_round=2, init_model=path)
    assert len(more.booster.trees) == 6 and torch.equal(more.predict(X), more.booster.scores)
    assert torch.equal(more.booster.predict(X, num_iteration=4), m.booster.scores)
    with pytest.raises(ValueError, match="linear_tree"):
        gbdt.LambdaMART(dict(params, linear_tree=False)).fit(X, y, group, num_boost_round=1, init_model=path)
