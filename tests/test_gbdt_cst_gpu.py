"""GPU: monotone and interaction constraints in the native booster (monotone_constraints, interaction_constraints; the *_cst entry points of
csrc/gbdt.hip) against the numpy restatement tests/gbdt_cst_ref.py, bit for bit; whole fits against scikit-learn's
HistGradientBoostingRegressor(monotonic_cst=..., interaction_cst=...) (tests/golden/gbdt_sklearn_cst.npz) under the gate the restatement set
(test_gbdt_cst_cpu.py); and the properties that must hold exactly: predict is monotone in a constrained feature, no path leaves a group."""
import os
import subprocess
import sys
import zipfile

import numpy as np
import pytest
import torch

import gbdt_cat_ref as CR
import gbdt_cst_ref as TR
import gbdt_ref as R
import gbdt_sk as SK

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPO = (10, 10)
ONE = 1 << 10
NBINS = (1, 2, 63, 64, 65, 255)
INF = np.inf


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


# ---------------------------------------------------------------- the split scan on hand-made histograms
def layout(nf, max_bin, kind):
    """(nbins, nan_bin or None, is_cat or None) of a call: the features cycle through NBINS (capped by max_bin); kind 'nan' gives every
    third feature a NaN bin behind its value bins, kind 'cat' also makes feature 1 categorical."""
    nbins = np.array([min(NBINS[(f + nf + max_bin) % len(NBINS)], max_bin) for f in range(nf)], np.int32)
    nan_bin = is_cat = None
    if kind in ("nan", "cat"):
        nan_bin = np.full(nf, -1, np.int32)
        for f in range(0, nf, 3):
            nbins[f] = min(nbins[f], max_bin - 1)
            nan_bin[f] = nbins[f]
    if kind == "cat":
        is_cat = np.zeros(nf, np.uint8)
        if nf > 1 and max_bin >= 8:
            is_cat[1], nbins[1] = 1, min(12, max_bin)
    return nbins, nan_bin, is_cat


def leaf_hist(rng, nbins, nan_bin, max_bin, rows=160):
    b = np.stack([rng.integers(0, nb, rows) for nb in nbins], axis=1)
    if nan_bin is not None:
        for f in np.nonzero(nan_bin >= 0)[0]:
            b[rng.random(rows) < 0.25, f] = nan_bin[f]
    qg = (rng.standard_normal(rows) * 4 * ONE + (b[:, 0] % 5) * ONE - (b[:, -1] % 3) * ONE).astype(np.int32)
    qh = rng.integers(ONE // 2, 2 * ONE, rows).astype(np.int32)
    return R.histogram(b.astype(np.uint8), qg, qh, None, max_bin)


def bounds_case(k, hist, nbins, nan_bin, is_cat, rng):
    """(lo, hi, v) of leaf k: infinite, finite on both sides, clamping one child only, lo == hi, then random finite ones."""
    tot = hist[0].sum(axis=0)
    v = float(TR.node_value(tot[0], tot[1], EXPO, 0.0))
    free = TR.best_split(hist, nbins, nan_bin, np.zeros(len(nbins), bool) if is_cat is None else is_cat, EXPO, min_data=2, cat_smooth=3.0,
                         mono=np.zeros(len(nbins), np.int64), cst=(-INF, INF, v))
    vl, vr = (free["vl"], free["vr"]) if free["feature"] >= 0 else (v - 1.0, v + 1.0)
    cases = [(-INF, INF, v), (min(vl, vr) - 0.25, max(vl, vr) + 0.25, v), (-INF, (vl + vr) / 2, min(v, (vl + vr) / 2)), (v, v, v),
             ((vl + vr) / 2, INF, max(v, (vl + vr) / 2))]
    if k < len(cases):
        return cases[k]
    lo = v + rng.uniform(-1.0, 0.5)
    return (lo, lo + rng.uniform(0.0, 1.5), v + rng.uniform(-0.5, 0.5))


def run_both(hists, nbins, nan_bin, is_cat, mono, cst, allowed, slots=None, l2=0.0):
    """The device's records (and sets) of the leaves, through the leaf form or the slot form, and the restatement's."""
    from ptranking_amd import functional as F
    up = lambda a, dt: None if a is None else dev(np.ascontiguousarray(a, dtype=dt))
    args = (dev(nbins), dev(np.array(EXPO, np.int32)), up(mono, np.int8), up(cst, np.float64), up(allowed, np.uint8), up(is_cat, np.uint8), 3.0, l2, 2, 1e-3, 0.0)
    if slots is None:
        rec, sets = F.gbdt_best_split_cst(dev(np.stack(hists)), *args, nan_bin=up(nan_bin, np.int32))
        slots = range(len(hists))
    else:
        rec, sets = F.gbdt_best_split_slots_cst(dev(np.stack(hists)), slots, *args, nan_bin=up(nan_bin, np.int32))
    rec = rec.cpu().numpy()
    sets = None if sets is None else sets.cpu().numpy()
    cat = np.zeros(len(nbins), bool) if is_cat is None else is_cat.astype(bool)
    want = []
    for k, slot in enumerate(slots):
        if not 0 <= slot < len(hists):
            want.append((TR.record(TR.NONE, nan_bin is not None), dict(TR.NONE)))
            continue
        s = TR.best_split(hists[slot], nbins, nan_bin, cat, EXPO, l2, 2, 1e-3, 0.0, 3.0, mono, None if cst is None else tuple(cst[k]),
                          None if allowed is None else allowed[k].astype(bool))
        want.append((TR.record(s, nan_bin is not None), s))
    return rec, sets, want


def assert_equal(rec, sets, want, what=""):
    for k, ((w_rec, w_set), s) in enumerate(want):
        assert np.array_equal(rec[k], w_rec), (what, k, rec[k].tolist(), w_rec.tolist(), s)
        if sets is not None:
            assert np.array_equal(sets[k], w_set), (what, k)


@pytest.mark.parametrize("max_bin", [2, 64, 255, 256])
@pytest.mark.parametrize("nf", [1, 3, 17])
def test_split_scan_equals_the_restatement(nf, max_bin):
    """Records bit for bit: one leaf through the leaf form and 31 slots through the slot form; +1, -1 and 0 in one call; every bounds case;
    the kinds (plain, NaN bins, NaN bins and a categorical feature) rotate over the shapes."""
    kind = ("plain", "nan", "cat")[(nf + max_bin) % 3]
    rng = np.random.default_rng([nf, max_bin])
    nbins, nan_bin, is_cat = layout(nf, max_bin, kind)
    mono = np.array([(1, -1, 0)[f % 3] for f in range(nf)], np.int8)
    if is_cat is not None:
        mono[is_cat != 0] = 0
    pool = [leaf_hist(rng, nbins, nan_bin, max_bin) for _ in range(7)]
    cst1 = np.array([bounds_case(1, pool[0], nbins, nan_bin, is_cat, rng)])
    assert_equal(*run_both(pool[:1], nbins, nan_bin, is_cat, mono, cst1, None), what="leaf form")
    slots = [int(s) for s in rng.integers(0, 7, 31)]
    slots[5], slots[17] = -1, 7                                          # outside the pool: the record without a split
    cst = np.array([bounds_case(k, pool[s], nbins, nan_bin, is_cat, rng) if 0 <= s < 7 else (-INF, INF, 0.0) for k, s in enumerate(slots)])
    allowed = (rng.random((31, nf)) < 0.7).astype(np.uint8)
    rec, sets, want = run_both(pool, nbins, nan_bin, is_cat, mono, cst, allowed, slots)
    assert_equal(rec, sets, want, what="slot form")
    assert (rec[[5, 17], 1] == -1).all()
    if nf > 1 and max_bin > 2:
        assert (rec[:, 1] >= 0).sum() > 10                               # the call is no row of empty records
    rec2, _, want2 = run_both(pool, nbins, nan_bin, is_cat, mono, cst[:8], None, slots[:8])       # monotone constraints alone
    assert_equal(rec2, None, want2, what="slot form, cst alone")


@pytest.mark.parametrize("kind", ["plain", "nan", "cat"])
def test_split_scan_bounds_cases_and_masks(kind):
    """F = 5, max_bin 64, the five bounds cases on one histogram; allowed all, one feature, none; interaction constraints alone give the
    bits of the unconstrained entry points on the allowed features."""
    from ptranking_amd import functional as F
    rng = np.random.default_rng(7)
    nf, max_bin = 5, 64
    nbins, nan_bin, is_cat = layout(nf, max_bin, kind)
    mono = np.array([1, 0, -1, 0, 1], np.int8)
    h = leaf_hist(rng, nbins, nan_bin, max_bin, rows=300)
    cst = np.array([bounds_case(k, h, nbins, nan_bin, is_cat, rng) for k in range(5)])
    rec, sets, want = run_both([h] * 5, nbins, nan_bin, is_cat, mono, cst, None)
    assert_equal(rec, sets, want)
    clamped, flat = want[2][1], want[3][1]
    free = TR.best_split(h, nbins, nan_bin, np.zeros(nf, bool) if is_cat is None else is_cat, EXPO, min_data=2, cat_smooth=3.0, mono=np.zeros(nf, np.int64),
                         cst=tuple(cst[0]))                              # the split the bounds of the cases 1, 2 and 4 were cut around
    assert free["feature"] >= 0 and max(free["vl"], free["vr"]) > cst[2, 1] > min(free["vl"], free["vr"])     # the bound of case 2 cuts one child only
    assert clamped["feature"] < 0 or max(clamped["vl"], clamped["vr"]) <= cst[2, 1]
    assert flat["feature"] < 0 or flat["vl"] == flat["vr"] == cst[3, 0]                                    # lo == hi: every candidate has vL == vR
    masks = np.array([[1] * 5, [0, 0, 1, 0, 0], [0] * 5, [1, 0, 0, 0, 1]], np.uint8)
    for c in (np.repeat(cst[:1], 4, axis=0), None):
        rec, sets, want = run_both([h] * 4, nbins, nan_bin, is_cat, mono, c, masks)
        assert_equal(rec, sets, want)
        assert rec[2, 1] == -1 and rec[1, 1] in (2, -1) and rec[3, 1] in (0, 4, -1)
    up = lambda a: None if a is None else dev(a)
    if is_cat is None:
        old = F.gbdt_best_split(dev(h[None]), dev(nbins), dev(np.array(EXPO, np.int32)), 0.0, 2, 1e-3, 0.0, nan_bin=up(nan_bin))
    else:
        old = F.gbdt_best_split_cat(dev(h[None]), dev(nbins), dev(np.array(EXPO, np.int32)), dev(is_cat), 3.0, 0.0, 2, 1e-3, 0.0, nan_bin=up(nan_bin))[0]
    assert np.array_equal(rec[0], old.cpu().numpy()[0])                  # all allowed, no bounds: today's record


def test_a_leaf_where_the_order_test_rejects_every_candidate():
    """Gradients that grow with t; a +1 feature binned along t and a -1 feature binned against it: every candidate has the larger value on
    the wrong side, the record is the one without a split; constraint 0 on the same histograms finds one."""
    rows = 256
    t = np.arange(rows)
    nbins = np.array([16, 32, 1], np.int32)
    b = np.stack([t * 16 // rows, 31 - t * 32 // rows, np.zeros(rows, np.int64)], axis=1).astype(np.uint8)
    h = R.histogram(b, ((t - 128) * ONE // 8).astype(np.int32), np.full(rows, ONE, np.int32), None, 64)
    v = float(TR.node_value(h[0].sum(axis=0)[0], h[0].sum(axis=0)[1], EXPO, 0.0))
    cst = np.array([(-INF, INF, v), (-3.0, 3.0, v)])
    rec, _, want = run_both([h, h], nbins, None, None, np.array([1, -1, 1], np.int8), cst, None)
    assert_equal(rec, None, want)
    assert (rec[:, 1] == -1).all() and (rec[:, 0].view(np.float64) == -INF).all() and not rec[:, 3:].any()
    rec, _, want = run_both([h, h], nbins, None, None, np.array([0, 0, 0], np.int8), cst, None)
    assert_equal(rec, None, want)
    assert (rec[:, 1] >= 0).all()
    rec, _, want = run_both([h, h], nbins, None, None, np.array([-1, 1, 0], np.int8), cst, None)         # the agreeing signs reject nothing
    assert_equal(rec, None, want)
    assert (rec[:, 1] >= 0).all()


def test_malformed_tables_are_read_as_untrusted():
    """A mono entry outside -1 .. 1 reads as 0; a NaN among a leaf's (lo, hi, v), or lo > hi, makes that leaf's record 'no split'."""
    rng = np.random.default_rng(3)
    nf, max_bin = 3, 64
    nbins, _, _ = layout(nf, max_bin, "plain")
    h = leaf_hist(rng, nbins, None, max_bin)
    v = float(TR.node_value(h[0].sum(axis=0)[0], h[0].sum(axis=0)[1], EXPO, 0.0))
    odd = np.array([5, -7, 127], np.int8)
    cst = np.array([(-INF, INF, v), (np.nan, INF, v), (-INF, np.nan, v), (0.0, 1.0, np.nan), (1.0, 0.0, v), (INF, -INF, v), (-1.0, 2.0, v)])
    rec, _, want = run_both([h] * 7, nbins, None, None, odd, cst, None)
    assert_equal(rec, None, want)
    zero, _, _ = run_both([h] * 7, nbins, None, None, np.zeros(3, np.int8), cst, None)
    assert np.array_equal(rec, zero)
    assert (rec[1:6, 1] == -1).all() and rec[0, 1] >= 0 and rec[6, 1] >= 0


# ---------------------------------------------------------------- whole fits against scikit-learn and the restatement
NAMES = ("a", "b", "c", "d", "e", "f", "g")
MONO = ("a", "b", "c", "d", "e", "g")


def fit_case(c, extra=None, rounds=None, baseline=True, params=None, X=None):
    import ptranking_amd as pa
    p = c["params"]
    booster = pa.GBDT(dict(TR.booster_params(c) if params is None else params, **(extra or {})), c["X"] if X is None else X)
    base = np.float32(c["baseline"] if baseline else 0.0)
    booster.scores.fill_(float(base))
    y, w = dev(c["y"]), dev(np.ones_like(c["y"]) if c["w"] is None else c["w"])
    out = []
    for _ in range(p["rounds"] if rounds is None else rounds):
        tree = booster.update((booster.scores - y) * w, w)
        out.append((tree, booster.scores.cpu().numpy().copy()))
    return booster, out


@pytest.fixture(scope="module")
def cases():
    got = TR.load()[0]
    assert tuple(sorted(got)) == NAMES
    return got


@pytest.fixture(scope="module")
def restated(cases):
    return {name: TR.run_restatement(c) for name, c in cases.items()}


@pytest.fixture(scope="module")
def fits(cases):
    out = {}
    for name, c in cases.items():
        booster, rounds = fit_case(c)
        base = float(np.float32(c["baseline"]))
        out[name] = dict(case=c, booster=booster, rounds=rounds, fresh=(booster.predict(c["fresh"]) + base).cpu().numpy())
    return out


@pytest.mark.parametrize("name", NAMES)
def test_whole_fits_match_sklearn(fits, name):
    """Trees equal to HistGradientBoostingRegressor's in canonical form (nodes and leaf row counts exactly), leaf values, training scores
    after every round and the fresh rows within C_GBDT_SK_CST 2^-24 max(1, max |score|).  Case c is fitted depth-wise."""
    fit = fits[name]
    c, p, b = fit["case"], fit["case"]["params"], fit["booster"]
    nbins = TR.setup(c)[1]
    assert np.array_equal(b.nbins, nbins) and (b.params["grow_policy"] == "depthwise") == bool(p["depthwise"])
    for r, (tree, scores) in enumerate(fit["rounds"]):
        nodes, leaves = TR.canonical(tree, c["X"], nbins)
        miss = TR.tree_mismatch(nodes, leaves, c, r)
        assert miss is None, f"round {r}: {miss}"
        err = float(np.abs(scores.astype(np.float64) - c["staged"][r]).max())
        print(f"MEASURED gbdt constrained vs sklearn, case {name} round {r}: training scores need C >= {err / SK.need_unit(c['staged'][r]):.2f}")
        assert err <= TR.gate(c["staged"][r]), r
    err = float(np.abs(fit["fresh"].astype(np.float64) - c["fresh_pred"]).max())
    print(f"MEASURED gbdt constrained vs sklearn, case {name}: fresh rows need C >= {err / SK.need_unit(c['fresh_pred']):.2f}")
    assert err <= TR.gate(c["fresh_pred"])


def same_tree(tree, ref, r):
    for k in ("feature", "left", "right") + tuple(k for k in ("default_left", "cat_index", "cat_set") if k in tree):
        assert np.array_equal(tree[k], ref[k]) and tree[k].dtype == ref[k].dtype, (r, k)
    assert np.array_equal(bits(tree["threshold"]), bits(ref["threshold"])) and np.array_equal(bits(tree["value"]), bits(ref["value"])), r


@pytest.mark.parametrize("name", NAMES)
def test_whole_fits_equal_the_restatement_bit_for_bit(fits, restated, name):
    """Nodes, fp32 leaf values, scores; the scores are predict(X) bit for bit.  Depth-wise numbers its nodes by level, so case c is compared
    in canonical form (values included, exactly) and fitted leaf-wise as well, where its cap cannot bind either."""
    fit = fits[name]
    c = fit["case"]
    want, fresh, _, _ = restated[name]
    nbins = fit["booster"].nbins
    for r, ((tree, scores), (ref, ref_scores)) in enumerate(zip(fit["rounds"], want)):
        if c["params"]["depthwise"]:
            for x, y in zip(TR.canonical(tree, c["X"], nbins), TR.canonical(ref, c["X"], nbins)):
                assert np.array_equal(x, y), r
        else:
            same_tree(tree, ref, r)
        assert np.array_equal(bits(scores), bits(ref_scores)), r
    assert np.array_equal(bits(fit["fresh"]), bits(fresh))
    zero, _ = fit_case(c, rounds=2, baseline=False)                      # from zero scores the resident scores are predict(X) bit for bit
    assert np.array_equal(bits(zero.scores), bits(zero.predict(c["X"])))
    if c["params"]["depthwise"]:
        params = {k: v for k, v in TR.booster_params(c).items() if k != "grow_policy"}
        booster, lw = fit_case(c, params=params)
        for r, ((tree, scores), (ref, ref_scores)) in enumerate(zip(lw, want)):
            same_tree(tree, ref, r)
            assert np.array_equal(bits(scores), bits(ref_scores)) and np.array_equal(bits(scores), bits(fit["rounds"][r][1])), r
        assert fit["booster"].host_reads < booster.host_reads


def sweep_steps(pred, c):
    """The smallest step of a prediction along the sweeps of a case, in the direction its constraint demands."""
    pred = np.asarray(pred, np.float64)
    return min(float((np.diff(pred[c["sweep_block"] == b]) * c["mono"][c["sweep_feature"][c["sweep_block"] == b][0]]).min()) for b in np.unique(c["sweep_block"]))


@pytest.mark.parametrize("name", MONO)
def test_predict_is_monotone_in_every_constrained_feature(fits, name):
    """fp32 addition is monotone, so no tolerance: along every sweep the prediction never steps against the constraint."""
    fit = fits[name]
    step = sweep_steps(fit["booster"].predict(fit["case"]["sweep"]).cpu().numpy(), fit["case"])
    print(f"MEASURED gbdt constrained, case {name}: smallest sweep step {step}")
    assert step >= 0.0


def test_the_unconstrained_fit_of_the_same_data_is_not_monotone(fits):
    c = fits["a"]["case"]
    params = {k: v for k, v in TR.booster_params(c).items() if k != "monotone_constraints"}
    booster, _ = fit_case(c, params=params)
    step = sweep_steps(booster.predict(c["sweep"]).cpu().numpy(), c)
    print(f"MEASURED gbdt unconstrained, case a: smallest sweep step {step}")
    assert step < 0.0


@pytest.mark.parametrize("policy", ["leafwise", "depthwise"])
@pytest.mark.parametrize("extra", [{"bagging_fraction": 0.5, "bagging_freq": 1}, {"data_sample_strategy": "goss", "learning_rate": 0.5}], ids=["bagging", "goss"])
def test_sampled_fits_stay_monotone_and_equal_to_predict(fits, extra, policy, monkeypatch):
    """Bagging and GOSS combine with the constraints, under use_missing too (case d): the sweeps stay monotone, the scores stay predict(X)
    bit for bit, and every device-to-host read inside update() is one host_reads counts."""
    for name in ("a", "d"):
        c = fits[name]["case"]
        reads = []
        real = torch.Tensor.cpu
        monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(1), real(self, *a, **k))[1])
        booster, rounds = fit_case(c, dict(extra, grow_policy=policy), rounds=4, baseline=False)
        monkeypatch.undo()
        assert len(reads) == booster.host_reads + 4                       # fit_case reads the scores once per round itself
        assert np.array_equal(bits(booster.scores), bits(booster.predict(c["X"])))
        assert sweep_steps(booster.predict(c["sweep"]).cpu().numpy(), c) >= 0.0
        assert all(t["feature"].size > 0 for t, _ in rounds)


def test_lambdamart_stays_monotone_under_lambdarank_ndcg():
    """30 queries of 20 documents; the relevance follows a sine of column 0, which the ranker is told to be non-decreasing in, and column 1
    with -1: along sweeps of either column the scores never step against the constraint."""
    import ptranking_amd as pa
    rng = np.random.default_rng(23)
    q, d = 30, 20
    X = (rng.integers(0, 24, (q * d, 4)) / 8.0).astype(np.float32)
    s = 2.0 * np.sin(3.0 * X[:, 0]) + X[:, 0] - 1.5 * np.cos(2.0 * X[:, 1]) + 0.5 * X[:, 2] + 0.3 * rng.standard_normal(q * d)
    y = np.digitize(s, np.quantile(s, [0.5, 0.8, 0.95])).astype(np.float32)
    for mono in ([1, -1, 0, 0], [0, 0, 0, 0]):
        m = pa.LambdaMART({"monotone_constraints": mono, "num_leaves": 8, "num_trees": 6, "min_data_in_leaf": 5, "learning_rate": 0.3,
                           "lambdarank_truncation_level": 10}, objective="lambdarank_ndcg")
        m.fit(X, y, np.full(q, d))
        assert m.booster.params["monotone_constraints"] == tuple(mono) and len(m.booster.trees) == 6
        worst = INF
        for f, sign in ((0, 1), (1, -1)):
            for base in X[:5]:
                sweep = np.repeat(base[None], 24, axis=0)
                sweep[:, f] = np.arange(24) / 8.0
                worst = min(worst, float((np.diff(m.predict(sweep).cpu().numpy().astype(np.float64)) * sign).min()))
        print(f"MEASURED LambdaMART lambdarank_ndcg, monotone_constraints {mono}: smallest sweep step {worst}")
        assert worst >= 0.0 or not any(mono)


@pytest.mark.parametrize("name", ["f", "g"])
def test_no_path_uses_two_features_that_share_no_group(fits, name):
    fit = fits[name]
    c = fit["case"]
    assert all(t["feature"].size > 1 for t, _ in fit["rounds"])
    assert all(not TR.forbidden_pairs(TR.tree_paths(t), c["groups"], 5) for t, _ in fit["rounds"])
    if name == "f":                                                      # without the constraint the same data gives a forbidden pair
        params = {k: v for k, v in TR.booster_params(c).items() if k != "interaction_constraints"}
        _, free = fit_case(c, params=params)
        assert any(TR.forbidden_pairs(TR.tree_paths(t), c["groups"], 5) for t, _ in free)
        for policy in ("depthwise",):
            _, dw = fit_case(c, extra={"grow_policy": policy})
            assert all(not TR.forbidden_pairs(TR.tree_paths(t), c["groups"], 5) for t, _ in dw)


# ---------------------------------------------------------------- invariants
@pytest.mark.parametrize("policy", ["leafwise", "depthwise"])
def test_host_reads_equal_those_of_the_unconstrained_fit(fits, policy):
    """Constraints that cannot bind make the twin: a monotone constraint on a constant column (every search then takes the bounded gain
    under infinite bounds and rejects nothing) and one interaction group of all features.  Both fits grow the unconstrained fit's trees
    (the two gain formulas differ by rounding alone, far inside the margin of the data) with the same fp32 scores, and must cost the same
    reads: one per split leaf-wise, one per level depth-wise."""
    c = fits["f"]["case"]
    X = np.concatenate([c["X"], np.ones((c["X"].shape[0], 1), np.float32)], axis=1)
    base = dict({k: v for k, v in TR.booster_params(c).items() if k != "interaction_constraints"}, grow_policy=policy)
    free_b, free_r = fit_case(c, params=base, X=X)
    for extra in ({"monotone_constraints": [0, 0, 0, 0, 0, 1]}, {"interaction_constraints": [list(range(6))]},
                  {"monotone_constraints": [0, 0, 0, 0, 0, -1], "interaction_constraints": [[0, 1, 2], [2, 3, 4, 5, 0, 1]]}):
        b, r = fit_case(c, params=dict(base, **extra), X=X)
        for (ta, sa), (tb, sb) in zip(free_r, r):
            assert all(np.array_equal(ta[k], tb[k]) for k in ("feature", "left", "right", "threshold")), extra
            assert np.array_equal(bits(sa), bits(sb)), extra
        assert b.host_reads == free_b.host_reads > c["params"]["rounds"], extra
    nodes = sum(t["feature"].size for t, _ in free_r)
    assert free_b.host_reads <= c["params"]["rounds"] + nodes
    if policy == "depthwise":
        assert free_b.host_reads < nodes


def test_inactive_constraints_change_nothing(fits, tmp_path, monkeypatch):
    """All-zero monotone_constraints and empty interaction_constraints: today's calls, today's trees, today's model file bytes."""
    import ptranking_amd as pa
    from ptranking_amd import functional as F
    c = fits["a"]["case"]
    base = {k: v for k, v in TR.booster_params(c).items() if k != "monotone_constraints"}
    called = []
    for name in ("gbdt_best_split_cst", "gbdt_best_split_slots_cst"):
        monkeypatch.setattr(F, name, lambda *a, _n=name, **k: called.append(_n))
    files, trees = [], []
    for k, prm in enumerate((base, dict(base, monotone_constraints=[0] * 5, interaction_constraints=[]), dict(base, monotone_constraints=(), grow_policy="depthwise"))):
        booster, rounds = fit_case(c, params=prm, rounds=2)
        booster.save_model(tmp_path / f"{k}.npz")
        with zipfile.ZipFile(tmp_path / f"{k}.npz") as z:
            files.append([(i.filename, z.read(i.filename)) for i in z.infolist()])
        trees.append(rounds)
    assert not called
    assert files[0] == files[1]
    for (ta, sa), (tb, sb) in zip(trees[0], trees[1]):
        assert sorted(ta) == sorted(tb) and all(np.array_equal(ta[k], tb[k]) for k in ta) and np.array_equal(bits(sa), bits(sb))
    with np.load(tmp_path / "1.npz", allow_pickle=False) as z:
        assert int(z["format"]) == 1 and "monotone" not in str(z["params"]) and "interaction" not in str(z["params"])
    assert pa.GBDT.load_model(tmp_path / "1.npz").params["monotone_constraints"] == ()


def test_a_constrained_model_saves_loads_and_predicts_the_same_bits(fits, tmp_path):
    import ptranking_amd as pa
    for name in ("e", "g"):
        b, c = fits[name]["booster"], fits[name]["case"]
        b.save_model(tmp_path / f"{name}.npz")
        back = pa.GBDT.load_model(tmp_path / f"{name}.npz")
        assert back.params == b.params and pa.gbdt.constraints(back.params)
        assert torch.equal(back.predict(c["fresh"]), b.predict(c["fresh"]))


def test_two_fits_give_the_same_bits(fits):
    for name in ("c", "e", "g"):
        first = fits[name]
        _, again = fit_case(first["case"])
        for (a, sa), (b, sb) in zip(first["rounds"], again):
            assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a) and np.array_equal(bits(sa), bits(sb))


def test_fit_bins_refuses_what_does_not_fit_the_columns():
    import ptranking_amd as pa
    X = np.zeros((8, 3), np.float32)
    with pytest.raises(ValueError, match="monotone_constraints holds 2 entries"):
        pa.GBDT({"monotone_constraints": [1, 0]}, X)
    with pytest.raises(ValueError, match="interaction_constraints 5 with 3 columns"):
        pa.GBDT({"interaction_constraints": [[0, 5]]}, X)


def test_example_runs_with_the_new_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_lambdamart_native.py"), "--queries", "120", "--rounds", "20",
                          "--monotone", "0:1,5:-1", "--interaction", "0,1,5;2,3"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("round ")]
    assert len(lines) == 2 and "nDCG@5" in lines[0], out.stdout
    assert "constraints: monotone, interaction" in out.stdout and "[0, 5]" in out.stdout
