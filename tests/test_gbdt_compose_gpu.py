"""GPU: the native GBDT under composed options against ONE restatement of GBDT.update (tests/gbdt_compose_ref.py) over the case table of
tests/gbdt_compose_cases.py, bit for bit: every round's tree, the scores, predict on fresh rows, a fit split by save_model / init_model, the
host reads, and on composed models pred_leaf, TreeSHAP, refit and LambdaMART.  Two comparisons reuse existing gates and add no tolerance:
linear leaves (test_gbdt_linear_gpu.py's residual bound gbdt_linear_ref.GAMMA) and SHAP (gbdt_shap_ref.C_SHAP)."""
import numpy as np
import pytest
import torch

import gbdt_compose_cases as CC
import gbdt_compose_ref as C
import gbdt_lifecycle_ref as LR
import gbdt_linear_ref as L
import gbdt_sample_ref as S
import gbdt_shap_ref as SR
from launch_form import launch_form
from test_gbdt_sample_gpu import bits, dev

pytestmark = pytest.mark.gpu
SHAP_CASES = ("depth_miss_cat_inter", "miss_cat_inter_bag_renew", "cat_mono_goss_q16")
REFIT_CASES = ("depth_miss_cat_inter", "miss_cat_inter_bag_renew")


def host(t):
    return t.cpu().numpy()


def copy_tree(t):
    return {k: np.array(v) for k, v in t.items()}


def device_fit(case, rounds, init_model=None):
    """`rounds` rounds of squared error on the device alone."""
    import ptranking_amd as pa
    d = case["data"]
    booster = pa.GBDT(case["params"], boosting=case["boosting"]).fit_bins(d["X"], group=d["group"], **({} if init_model is None else {"init_model": init_model}))
    yd = dev(d["y"])
    for _ in range(rounds):
        s = booster.begin_round()
        booster.update(s - yd, torch.ones_like(s))
    return booster


def check_linear(booster, case, t, g):
    """test_gbdt_linear_gpu.py's comparison of the last tree's fits: the statuses equal the restatement's on the bag's rows the tree assigns,
    no decision sits near the pivot floor, and the device's coefficients meet the residual bound on the restatement's moments."""
    d, p, tree = case["data"], booster.params, booster.trees[-1]
    g2, h2, mask = S.tree_mask(p, t, g, np.ones_like(g), d["qid"])
    bag = np.arange(g.size) if mask is None else np.nonzero(mask)[0]
    leaf, factors = L.assign(d["X"][bag], tree), []
    for l, P in enumerate(L.path_features(tree)):
        A, b, m_u = (np.asarray(a, np.float64) for a in L.moments(d["X"], bag[leaf == l], P, g2, h2, np.longdouble)[:3])
        c, status, ratio = L.solve(A, b, len(P), int(m_u), p["linear_lambda"])
        assert ratio > 2.0 ** -20 or ratio < 2.0 ** -45, (l, ratio)
        assert booster.last_linear_status[l] == status, (l, status, booster.last_linear_status)
        if status == 0:
            assert tree["leaf_features"][l, :len(P)].tolist() == P
            factors.append(float(L.residual_factor(A, b, len(P), p["linear_lambda"], np.r_[tree["leaf_coeff"][l, :len(P)], tree["leaf_const"][l]] / booster._tree_lr)))
        else:
            assert (tree["leaf_features"][l] == -1).all()
    return factors


def run(name):
    """The case on the device, the restatement driven by the device's own gradients -> (case, booster, the device's trees as born, the
    restated final trees, the restated rounds, the reads per round, the linear residual factors)."""
    import ptranking_amd as pa
    case = CC.case(name)
    d, linear = case["data"], case["values"]["linear"]
    booster = pa.GBDT(case["params"], boosting=case["boosting"]).fit_bins(d["X"], group=d["group"])
    yd, got, reads, factors = dev(d["y"]), [], [], []

    def gradients(r, at):
        before = booster.host_reads
        s = booster.begin_round()
        assert linear or np.array_equal(bits(s), bits(at)), (name, r)       # the scores with the round's drops taken out
        g = s - yd
        tree = booster.update(g, torch.ones_like(g))
        reads.append(booster.host_reads - before)
        got.append(copy_tree(tree))
        if linear:
            factors.extend(check_linear(booster, case, r, host(g)))
        return host(g)

    trees, rounds = C.fit(case, gradients)
    return case, booster, got, trees, rounds, reads, factors


@pytest.mark.parametrize("name", CC.CASES)
def test_composed_fit_equals_the_restatement(name, tmp_path):
    case, booster, got, trees, rounds, reads, factors = run(name)
    d, p, v = case["data"], case["params"], case["values"]
    depthwise, linear, dart = v["grow_policy"] == "depthwise", v["linear"], v["boosting"] == "dart"
    same = (lambda a, b: C.same_canonical(a, b, d["X"], d["nbins"])) if depthwise else C.same_tree
    for r, (tree, want) in enumerate(zip(got, rounds)):
        assert same(tree, want["tree"]) and tree["feature"].size >= 3, (name, r)
        assert "default_left" in tree or not v["use_missing"]
        assert reads[r] == C.host_reads(want["tree"], want["stats"]["leaf_rows"], p, dropped_before=dart and r > 0), (name, r, reads[r])
    for k, (tree, want) in enumerate(zip(booster.trees, trees)):           # the final values: DART has rescaled the dropped trees
        assert same(tree, want), (name, k)
    fresh = d["fresh"]
    if dart:
        # under 'dart' the resident scores are the fp32 walk (dropped trees out, the new tree in, the rescaled trees back), which no sum in
        # tree order reproduces bit for bit: the scores are pinned to the restated walk below, predict(X) to the restated predict here
        assert np.array_equal(bits(booster.predict(d["X"])), bits(C.predict(d["X"], trees)))
    else:
        assert torch.equal(booster.predict(d["X"]), booster.scores)
    if linear:
        print(name, "worst residual factor", max(factors), "of", len(factors), "fitted leaves; bound", L.GAMMA)
        assert factors and max(factors) <= L.GAMMA
        outs = np.stack([C.tree_outputs(fresh, t).astype(np.float64) for t in booster.trees])      # the device's own coefficients
        terms = np.abs(outs).sum(0)
        assert (np.abs(host(booster.predict(fresh)).astype(np.float64) - outs.sum(0)) <= (len(outs) + 1) * np.spacing(terms.astype(np.float32))).all()
    else:
        assert np.array_equal(bits(booster.scores), bits(rounds[-1]["scores"]))
        assert np.array_equal(bits(booster.predict(fresh)), bits(C.predict(fresh, trees)))
    # a fit split by save_model / init_model after round 2
    first = device_fit(case, 2)
    first.save_model(tmp_path / "two.npz")
    cont = device_fit(case, case["rounds"] - 2, init_model=tmp_path / "two.npz")
    assert len(cont.trees) == case["rounds"] and (dart or torch.equal(cont.predict(d["X"]), cont.scores))
    if dart:
        # not refused, and documented NOT to equal the unsplit fit: the trees of an initial model are never dropped and carry no weight
        assert all(k >= 2 for k in cont.last_drop) and all(C.same_tree(a, b) for a, b in zip(cont.trees[:2], first.trees))
    else:
        for a, b in zip(cont.trees, booster.trees):
            assert a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a), name
        assert torch.equal(cont.scores, booster.scores)


def test_the_replayed_drops_are_the_boosters():
    case = CC.case("dart_miss_mono_byquery")
    import ptranking_amd as pa
    d = case["data"]
    booster = pa.GBDT(case["params"], boosting="dart").fit_bins(d["X"], group=d["group"])
    yd, sel = dev(d["y"]), C.selection(case)
    for r in range(case["rounds"]):
        s = booster.begin_round()
        assert booster.last_drop == tuple(sel[r][0]), r
        booster.update(s - yd, torch.ones_like(s))
    assert any(drop for drop, _, _ in sel)


def test_the_shapes_reach_both_histogram_forms():
    """600 rows, 8 features, max_bin 31: the root takes the LDS form, a child of at most 256 rows the direct form, with and without the packed
    cells.  The packed kernel's flush period under 16 levels is 65535 rows: no fit of this table flushes, test_gbdt_quant_gpu.py pins that."""
    direct, lds = (launch_form("ptr_gbdt_histogram", m, CC.F_, CC.MAX_BIN)[0] for m in (256, CC.N))
    assert direct == 1 and lds != direct
    for B in (4, 16):
        assert launch_form("ptr_gbdt_histogram_packed", 256, CC.F_, CC.MAX_BIN, B // 2, B)[0] == 1 != launch_form("ptr_gbdt_histogram_packed", CC.N, CC.F_, CC.MAX_BIN, B // 2, B)[0]
        assert launch_form("ptr_gbdt_histogram_packed", CC.N, CC.F_, CC.MAX_BIN, B // 2, B)[5] == (2 ** 20 - 1) // B > CC.N
    case, (_, rounds) = CC.case("plain"), C.fit(CC.case("plain"))
    sizes = [rows.size for r in rounds for rows in r["stats"]["leaf_rows"]]
    assert min(sizes) <= 256 < CC.N


def is_cat_of(case):
    return case["data"]["is_cat"].astype(np.uint8) if case["values"]["categorical"] else None


@pytest.mark.parametrize("name", SHAP_CASES)
def test_pred_leaf_and_shap_on_composed_models(name):
    case = CC.case(name)
    d = case["data"]
    booster = device_fit(case, case["rounds"])
    Xe = np.concatenate([d["X"][:40], d["fresh"][:40]])
    assert np.array_equal(host(booster.predict(Xe, pred_leaf=True)), LR.pred_leaf(booster.trees, Xe, is_cat_of(case)))
    booster.set_background(d["X"])
    counts = [SR.leaf_counts(t, d["X"]) for t in booster.trees]
    want = SR.shap_exponential(booster.trees, counts, Xe, CC.F_)
    got = host(booster.predict(Xe, pred_contrib=True))
    need = np.abs(got - want).max() / SR.bound(booster.trees)
    print(f"{name}: need {need:.3f} of C_SHAP {SR.C_SHAP}")
    assert need <= SR.C_SHAP


@pytest.mark.parametrize("name", REFIT_CASES)
def test_refit_on_composed_models(name):
    case = CC.case(name)
    d, p = case["data"], case["params"]
    booster = device_fit(case, case["rounds"])
    X2 = d["fresh"]
    y2 = np.random.default_rng(3).standard_normal(X2.shape[0]).astype(np.float32)
    yd = dev(y2)
    new = booster.refit(X2, lambda s: (s - yd, torch.ones_like(s)), decay_rate=0.9)
    values, scores = LR.refit(booster.trees, X2, lambda s: ((s - y2).astype(np.float32), np.ones_like(s)), 0.0, p["learning_rate"], 0.9, is_cat_of(case))
    for k, (t, old, val) in enumerate(zip(new.trees, booster.trees, values)):
        assert t["value"].dtype == np.float32 and t["value"].tobytes() == val.tobytes(), (name, k)
        assert all(np.array_equal(t[key], old[key]) for key in old if key != "value")
    assert np.array_equal(bits(new.scores), bits(scores)) and np.array_equal(bits(new.predict(X2)), bits(new.scores))


def test_lambdamart_under_composed_options(monkeypatch):
    """lambdarank_ndcg with use_missing, categories, interaction constraints, GOSS and quantization with renewal: each tree equals the
    restatement on the gradients the ranker handed the booster."""
    import ptranking_amd as pa
    from ptranking_amd import gbdt as G
    values = dict(grow_policy="leafwise", use_missing=True, categorical=True, monotone=False, interaction=True, sampling="goss", quant="renew",
                  quant_bins=16, boosting="gbdt", linear=False)
    d = CC.binned(True, True)
    params = dict(CC.params_of(values), min_sum_hessian_in_leaf=1e-6)
    y = np.clip(np.round(CC.target(d["X"], 0) + 1), 0, 4).astype(np.float32)
    seen, real = [], G.GBDT.update
    monkeypatch.setattr(G.GBDT, "update", lambda self, g, h: (seen.append((host(g).copy(), host(h).copy())), real(self, g, h))[1])
    model = pa.LambdaMART(params, objective="lambdarank_ndcg").fit(d["X"], y, d["group"], num_boost_round=3)
    trees = model.booster.trees
    assert len(trees) == len(seen) == 3 and all(t["feature"].size > 0 for t in trees)
    for t, (g, h) in enumerate(seen):
        want, mask, _, margin, _ = C.grow(d["X"], d["bins"], g, h, d["edges"], d["nbins"], d["nan_bin"], d["is_cat"], model.booster.params, t, d["qid"])
        print("tree", t, "margin", margin, "sampled", mask is not None)
        assert (mask is not None) == (t >= 1) and C.same_tree(trees[t], want), t
