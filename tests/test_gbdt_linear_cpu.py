"""CPU: the parameters and refusals of linear trees, the host's path features, and what the GPU tests take from the restatement alone
(tests/gbdt_linear_ref.py): numpy's own residual factor on the solve cases, pivots far from the floor, the loss gap of the plain fit."""
import numpy as np
import pytest

import gbdt_linear_ref as L


def test_parameters():
    from ptranking_amd import gbdt
    assert gbdt.DEFAULT_PARAMS["linear_tree"] is False and gbdt.DEFAULT_PARAMS["linear_lambda"] == 0.0 and gbdt.LINEAR_KEYS == ("linear_tree", "linear_lambda")
    p = gbdt._params({"linear_tree": True, "linear_lambda": 2})
    assert p["linear_tree"] is True and p["linear_lambda"] == 2.0 and type(p["linear_lambda"]) is float
    for bad in ({"linear_tree": 1}, {"linear_tree": "yes"}, {"linear_lambda": -1.0}, {"linear_lambda": float("inf")}, {"linear_lambda": float("nan")},
                {"linear_lambda": "x"}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            gbdt._params(bad)


REFUSALS = {"dart": lambda g: g._params({"linear_tree": True}, "dart"),
            "categorical_feature": lambda g: g._params({"linear_tree": True, "categorical_feature": [0]}),
            "monotone_constraints": lambda g: g._params({"linear_tree": True, "monotone_constraints": [1, 0]}),
            "quant_train_renew_leaf": lambda g: g._params({"linear_tree": True, "use_quantized_grad": True, "quant_train_renew_leaf": True}),
            "refit": lambda g: g.GBDT({"linear_tree": True}).refit(np.zeros((2, 2), np.float32), None),
            "set_background": lambda g: g.GBDT({"linear_tree": True}).set_background(np.zeros((2, 2), np.float32)),
            "pred_contrib": lambda g: g.GBDT({"linear_tree": True}).predict(np.zeros((2, 2), np.float32), pred_contrib=True),
            "init_model": lambda g: g._initial_model(g.GBDT({}), g._params({"linear_tree": True}))}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_name_their_reason(what):
    from ptranking_amd import gbdt
    with pytest.raises(ValueError, match="linear_tree"):
        REFUSALS[what](gbdt)
    gbdt._params({"linear_tree": True, "monotone_constraints": [0, 0], "interaction_constraints": [[0, 1]], "use_quantized_grad": True, "use_missing": True})


def test_path_features_on_a_chain_of_31_features_and_a_revisited_one():
    from ptranking_amd import gbdt
    nn = 31
    chain = {"feature": np.arange(nn), "left": ~np.arange(nn), "right": np.r_[np.arange(1, nn), ~nn]}
    feats, nfeat = gbdt.linear_path_features(chain["feature"], chain["left"], chain["right"])
    assert nfeat.tolist() == list(range(1, 32)) + [31] and (feats[30:] == -1).all()          # 31 distinct features: the two deepest leaves stay constant
    assert feats[29].tolist() == list(range(30)) and L.solve(None, None, 31, 100, 0.0)[1] == 2
    tree = {"feature": np.array([3, 1, 3]), "left": np.array([1, ~0, ~2]), "right": np.array([2, ~1, ~3])}
    feats, nfeat = gbdt.linear_path_features(tree["feature"], tree["left"], tree["right"])
    want = L.path_features(tree)
    assert want == [[3, 1], [3, 1], [3], [3]] and nfeat.tolist() == [2, 2, 1, 1] and all(feats[l, :len(P)].tolist() == P for l, P in enumerate(want))
    assert gbdt.linear_path_features([], [], [])[1].tolist() == [0]


def test_numpy_residual_factor_and_pivots_far_from_the_floor():
    """GAMMA_NUMPY bounds numpy's own float64 Cholesky solve on the solve cases (the kernel gets four times that), every pivot of those
    cases is above 2^-20 of its diagonal, and the degenerate cases are degenerate exactly or to rounding, never near 2^-40."""
    worst = 0.0
    for k, lam in L.SOLVE_CASES:
        A, b, m_u = L.solve_case(k, lam)
        M = A + np.diag([lam] * k + [0.0])
        c = -np.linalg.solve(np.linalg.cholesky(M).T, np.linalg.solve(np.linalg.cholesky(M), b))
        worst = max(worst, L.residual_factor(A, b, k, lam, c))
        own, status, ratio = L.solve(A, b, k, m_u, lam)
        assert status == 0 and ratio > 2.0 ** -20 and L.residual_factor(A, b, k, lam, own) <= L.GAMMA
    print("numpy residual factor", worst)
    assert worst <= L.GAMMA_NUMPY
    X = np.random.default_rng(1).standard_normal((50, 3)).astype(np.float32)
    X[:, 1] = 2.5                                                           # constant over the leaf: collinear with the intercept
    A, b, m_u = L.moments(X, np.arange(50), [0, 1, 2], np.ones(50), np.ones(50))[:3]
    _, status, ratio = L.solve(A, b, 3, m_u, 0.0)
    assert status == 4 and ratio < 2.0 ** -45


def test_the_plain_fit_gains_from_linear_leaves_in_the_restatement():
    from test_gbdt_linear_gpu import FIT, ROUNDS, fit_data
    X, y = fit_data(False)
    kw = dict(num_leaves=FIT["num_leaves"], lr=FIT["learning_rate"], max_bin=FIT["max_bin"], min_data=FIT["min_data_in_leaf"])
    loss = [float(((L.fit_squared_error(X, y, ROUNDS, lin, **kw)[1] - y) ** 2).mean()) for lin in (False, True)]
    assert loss[1] < 0.5 * loss[0], loss
