"""CPU: the composed gate of the native GBDT before any GPU runs.  The case table of gbdt_compose_cases.py covers every pair of option values
that ptranking_amd.gbdt._params accepts (and claims none it refuses); every case is honest (its options decide something, no split search
sits on a tie); each planted fault of gbdt_compose_ref.py changes at least one case; with every option off the composition is
gbdt_ref.grow_tree bit for bit; and its predict equals the single-option restatements on their golden fixtures."""
import functools
import itertools

import numpy as np
import pytest

import gbdt_cat_ref as CR
import gbdt_compose_cases as CC
import gbdt_compose_ref as C
import gbdt_missing_ref as MR
import gbdt_ref as R

MARGIN = 1e-9                  # the screen of test_gbdt_gpu.py, test_gbdt_level_gpu.py and test_gbdt_sample_gpu.py


@functools.lru_cache(maxsize=None)
def clean(name):
    case = CC.case(name)
    return case, C.fit(case)


def all_pairs():
    return [((a, va), (b, vb)) for a, b in itertools.combinations(CC.AXES, 2) for va in CC.AXES[a] for vb in CC.AXES[b]]


# ---------------------------------------------------------------- the table hides no gap
def test_every_pair_of_option_values_is_covered_or_refused():
    from ptranking_amd import gbdt
    held = set()
    for name in CC.CASES:
        v = CC.axis_values(name)
        assert all(v[a] in CC.AXES[a] for a in CC.AXES), name
        held |= {frozenset(((a, v[a]), (b, v[b]))) for a, b in itertools.combinations(CC.AXES, 2)}
    covered = refused = 0
    for pair in all_pairs():
        params, boosting = CC.minimal_params(pair)
        if frozenset(pair) in held:                                       # a covered pair must be one the product accepts
            assert frozenset(pair) not in CC.REFUSED, pair
            gbdt._params(params, boosting)
            covered += 1
        else:                                                             # anything else must be refused, by the product itself
            assert frozenset(pair) in CC.REFUSED, f"neither covered nor refused: {pair}"
            with pytest.raises(ValueError):
                gbdt._params(params, boosting)
            refused += 1
    print(f"pairs covered {covered}, refused {refused}, uncovered 0, of {len(all_pairs())}")
    assert refused == len(CC.REFUSED) == 6 and covered + refused == len(all_pairs()) and 16 <= len(CC.CASES) <= 24
    with pytest.raises(ValueError, match="goss"):                       # the seventh refusal: two values of the table's one sampling axis
        gbdt._params({"data_sample_strategy": "goss", "bagging_fraction": 0.6, "bagging_freq": 2})
    for name in CC.CASES:                                                 # and every case's full dict is accepted
        case = CC.case(name)
        gbdt._params(case["params"], case["boosting"])


def test_the_data_is_what_the_issue_of_the_table_needs():
    from ptranking_amd import gbdt
    for missing, cat in itertools.product((False, True), repeat=2):
        d = CC.binned(missing, cat)
        X = d["X"]
        assert X.shape == (600, 8) and d["qid"].size == 600 and np.bincount(d["qid"]).tolist() == [30] * 20
        got = gbdt.bin_edges(X, CC.MAX_BIN, missing, CC.CATS if cat else ())
        assert np.array_equal(got[0], d["edges"]) and np.array_equal(got[1], d["nbins"])        # the product bins as the restatement does
        assert not missing or np.array_equal(got[2], d["nan_bin"])
        assert np.unique(X[:, 7]).size == 1 and np.unique(X[:, 6]).size == 5
        for f in CC.CATS:
            col = X[:, f][~np.isnan(X[:, f])]
            assert set(col.tolist()) == set(range(12))
        frac = np.isnan(X).mean(axis=0)
        assert (frac[[2, 4]] > 0.05).all() and (frac[[2, 4]] < 0.15).all() if missing else not np.isnan(X).any()
        assert not frac[[0, 1, 3, 5, 6, 7]].any()
        fresh = CC.fresh(missing, cat, d["edges"])
        assert fresh.shape == (200, 8) and (fresh[:, 1][~np.isnan(fresh[:, 1])] > 11).any() and np.isnan(fresh).any() == missing
        assert all(np.isin(fresh[:40, f][~np.isnan(fresh[:40, f])], d["edges"][f]).all() for f in (0, 2, 3, 5))


# ---------------------------------------------------------------- every case is honest
def honesty(case, rounds):
    """The first honesty condition a fit misses, or None."""
    v, p = case["values"], case["params"]
    worst = min(r["margin"] for r in rounds)
    if not worst > MARGIN:
        return f"margin {worst:.3g}"
    if not all(r["tree"]["feature"].size >= 3 for r in rounds):
        return "a tree of fewer than 3 internal nodes"
    if v["monotone"] and not any(r["stats"]["changed"] > 0 or r["stats"]["clamped"] > 0 for r in rounds):
        return "the monotone constraints decide nothing"
    if v["interaction"]:
        free = C.fit(case, params={k: x for k, x in p.items() if k != "interaction_constraints"})[1]
        if all(C.same_tree(a["tree"], b["tree"]) for a, b in zip(rounds, free)):
            return "the interaction constraints decide nothing"
    if v["categorical"] and not any(r["stats"]["cat_nodes"] for r in rounds):
        return "no categorical node"
    if v["use_missing"]:
        dl = [d for r in rounds for d in r["stats"]["default_left"]]
        if not (0 in dl and 1 in dl):
            return "default_left takes one value only"
    if v["sampling"] != "none":
        sampled = [r for r in rounds if r["mask"] is not None]
        if not sampled or not all(r["stats"]["oob"] > 0 for r in sampled):
            return "a sampled round without an out-of-bag row"
    if v["boosting"] == "dart" and not any(r["drop"] for r in rounds):
        return "no round drops a tree"
    if v["linear"] and not any(s[3] == 0 for r in rounds for s in r["stats"]["linear"]):
        return "no leaf is fitted"
    if v["linear"] and not all(s[4] > 2.0 ** -20 or s[4] < 2.0 ** -45 for r in rounds for s in r["stats"]["linear"]):
        return "a linear fit decides near the pivot floor"
    return None


@pytest.mark.parametrize("name", CC.CASES)
def test_every_case_is_honest(name):
    case, (trees, rounds) = clean(name)
    assert len(rounds) == case["rounds"] == (CC.DART_ROUNDS if case["boosting"] == "dart" else CC.ROUNDS)
    assert honesty(case, rounds) is None
    if case["boosting"] == "dart":                                        # the replayed selection itself
        assert any(drop for drop, _, _ in C.selection(case))
    if case["values"]["grow_policy"] == "depthwise":
        assert case["params"]["num_leaves"] >= 2 ** case["params"]["max_depth"]
    print(name, "seed", case["seed"], "smallest margin", min(r["margin"] for r in rounds))


# ---------------------------------------------------------------- every case can fail
def differs(name, fault):
    case, (trees, rounds) = clean(name)
    got_trees, got = C.fit(case, fault=fault)
    fresh = case["data"]["fresh"]
    return (not all(C.same_tree(a, b) for a, b in zip(got_trees, trees)) or any(a["scores"].tobytes() != b["scores"].tobytes() for a, b in zip(got, rounds))
            or C.predict(fresh, got_trees).tobytes() != C.predict(fresh, trees).tobytes())


def applies(name, fault):
    v = CC.axis_values(name)
    return {"quant_ignores_bag": v["quant"] == "renew" and v["sampling"] != "none", "renew_plain_lr": v["quant"] == "renew" and v["boosting"] == "dart",
            "cat_row0_set": v["categorical"], "stale_default_left": v["use_missing"], "groups_after_cat": v["categorical"] and v["interaction"]}[fault]


@pytest.mark.parametrize("fault", C.FAULTS)
def test_each_planted_fault_fails_a_case(fault):
    names = [n for n in CC.CASES if applies(n, fault)]
    caught = [n for n in names if differs(n, fault)]
    print(fault, "caught by", caught, "of", names)
    assert caught


# ---------------------------------------------------------------- options off: the first restatement
def test_all_options_off_is_the_plain_restatement_bit_for_bit():
    case = CC.case("plain")
    d, p = case["data"], case["params"]
    scores = np.zeros(CC.N, np.float32)
    for t in range(3):
        g, h = scores - d["y"], np.ones(CC.N, np.float32)
        tree, mask, add, margin, stats = C.grow(d["X"], d["bins"], g, h, d["edges"], d["nbins"], None, d["is_cat"], p, t)
        qg, qh, expo, _ = R.quantize(g, h)
        want, leaf_rows, wmargin = R.grow_tree(d["bins"], qg, qh, expo, d["edges"], d["nbins"], p["max_bin"], p["num_leaves"], p["learning_rate"], 0.0,
                                               p["min_data_in_leaf"], 1e-3, 0.0, -1)
        assert mask is None and margin == wmargin and all(np.asarray(tree[k]).tobytes() == want[k].tobytes() for k in want) and (tree["cat_index"] == -1).all()
        ref = R.add_leaf_values(scores.copy(), leaf_rows, want["value"])
        scores = (scores + add).astype(np.float32)
        assert scores.tobytes() == ref.tobytes()
        assert C.host_reads(tree, stats["leaf_rows"], p) == 1 + sum(1 for k in range(tree["feature"].size) if k + 2 < p["num_leaves"])


# ---------------------------------------------------------------- predict against the single-option restatements
def test_predict_equals_the_single_option_restatements_on_their_fixtures():
    cases, _ = CR.load()
    seen = 0
    for name, case in sorted(cases.items())[:3]:
        rounds, _, _ = CR.run_restatement(case)
        trees = [t for t, _ in rounds]
        for M in (case["fresh"], case["X"][:100]):
            assert C.predict(M, trees).tobytes() == CR.predict(M, trees).tobytes(), name
        seen += int(any((t["cat_index"] >= 0).any() for t in trees))
    assert seen
    cases, _ = MR.load()
    for name, case in sorted(cases.items())[:3]:
        rounds = MR.run_restatement(case)[0]
        trees = [t for t, _ in rounds]
        assert np.isnan(case["fresh"]).any() and C.predict(case["fresh"], trees).tobytes() == MR.predict(case["fresh"], trees).tobytes(), name
