"""CPU: the truncated, normalised lambdarank without a GPU — the float64 restatement (tests/lambdarank_ndcg_ref.py) against tree_ref's
Delta-nDCG form under the identity that links them, its invariants and exact zeros, the eager fp32 form under the gate on every input of
the GPU tests, planted faults the gate must reject, the parameters, the model file, the ABI and the Python surface."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import f64_loss_bounds as FB
import lambdarank_ndcg_ref as LR
import tree_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
ENTRY = "ptr_tree_lambdarank_ndcg_grad_hess"
NEW_DEFAULTS = {"lambdarank_truncation_level": 30, "lambdarank_norm": True, "sigmoid": 1.0}


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("n", [2, 5, 17, 64, 130])
def test_no_truncation_no_norm_is_the_delta_ndcg_form(n):
    s, y = TR.tree_inputs([n], seed=n)
    y = LR.plant_relevant(y, [n])
    for T in (n, n + 7, 5000):
        grad, _, hess, _ = LR.query(s, y, T=T, sigma=1.0, norm=False)
        want = TR.pair_query(s, y, pair_type="NoTies", weighting="DeltaNDCG", eps=1.0, hessian="sum")
        # the other form floors each pair's p (1 - p) at 1e-16 before the weight: at most (n - 1) 1e-16 per document
        assert np.abs(grad - want[0]).max() <= 1e-15 and np.abs(hess - want[2]).max() <= 1e-15 + (n - 1) * 1e-16


@pytest.mark.parametrize("T,norm,sigma", [(1, True, 1.0), (3, False, 2.0), (30, True, 2.0), (5000, True, 1.0)])
def test_gradients_sum_to_zero_and_no_hessian_is_negative(T, norm, sigma):
    group = [2, 5, 17, 64, 130]
    s, y = TR.tree_inputs(group, seed=3)
    ref = LR.batch(s, y, group, T=T, norm=norm, sigma=sigma)
    off = TR.offsets_of(group)
    for a, b in zip(off[:-1], off[1:]):
        assert abs(ref["grad"][a:b].sum()) <= 1e-13 * max(1.0, np.abs(ref["grad"][a:b]).sum())
    assert (ref["hess"] >= 0).all() and (ref["E_grad"] >= 0).all() and (ref["E_hess"] >= 0).all()
    assert np.abs(ref["grad"]).max() > 0


def test_the_exact_zero_cases():
    s = np.array([0.3, -1.2, 2.0, 0.1], np.float32)
    for y in ([2.0, 2.0, 2.0, 2.0], [0.0, 0.0, 0.0, 0.0]):              # equal labels; no relevant document
        for norm in (True, False):
            res = LR.query(s, np.array(y, np.float32), T=2, norm=norm)
            assert all((v == 0).all() for v in res)                     # the bounds too: exact
            eg, eh = LR.eager_query(s, np.array(y, np.float32), T=2, norm=norm)
            assert (eg == 0).all() and (eh == 0).all()
    assert all((v == 0).all() and v.shape == (1,) for v in LR.query([0.5], [3.0]))
    assert all(v.shape == (0,) for v in LR.query([], []))
    # the Delta-nDCG weighting is NaN without a relevant document wherever a pair passes its mask: the difference the header states
    nan = TR.pair_query(s, np.zeros(4), pair_type="All", weighting="DeltaNDCG", hessian="sum")
    assert np.isnan(nan[0]).all()
    bad = LR.query(np.array([0.1, np.nan, 0.3]), np.array([1.0, 0.0, 2.0]))
    assert np.isnan(bad[0]).all() and np.isnan(bad[2]).all()


@pytest.mark.parametrize("n", [2, 17, 64])
def test_a_truncation_level_from_n_minus_1_on_changes_nothing(n):
    """min(r(i), r(j)) < n - 1 holds for every pair: the two ranks differ, so the smaller is at most n - 2.  maxDCG at n - 1 misses only the
    smallest gain, so the lists here end their ideal order with an irrelevant document."""
    s, y = TR.tree_inputs([n], seed=40 + n)
    y = LR.plant_relevant(y, [n])
    y[-1] = 0.0
    for norm in (True, False):
        want = LR.query(s, y, T=5000, norm=norm, sigma=2.0)
        for T in (n - 1, n, n + 1):
            got = LR.query(s, y, T=max(T, 1), norm=norm, sigma=2.0)
            for a, b in zip(got, want):                      # float64 sums of one more or one less zero term: rounding alone
                assert np.allclose(a, b, rtol=1e-13, atol=0.0), (T, norm)


# ---------------------------------------------------------------------------------------------------------------- 2. the eager form
EAGER_WORST = {}


@pytest.mark.parametrize("T,norm,sigma", LR.CONFIGS)
def test_eager_fp32_passes_the_gate_on_the_straddle_batch(T, norm, sigma):
    s, y, group = LR.gpu_inputs()["straddle"]
    grad, hess = LR.eager_batch(s, y, group, T=T, norm=norm, sigma=sigma)
    w = LR.gate(grad, hess, LR.reference("straddle", T, norm, sigma), f"eager straddle T {T} norm {norm} sigma {sigma}")
    EAGER_WORST[(T, norm, sigma)] = w
    print(f"eager fp32: worst err/E {w:.3f}: needs C_PAIR >= {w * FB.C_PAIR:.2f}")


@pytest.mark.parametrize("name", [k for k in LR.gpu_inputs() if k != "straddle"])
def test_eager_fp32_passes_the_gate_on_every_other_gpu_input(name):
    s, y, group = LR.gpu_inputs()[name]
    worst = 0.0
    for T, norm, sigma in ((1, True, 2.0), (2, False, 1.0), (30, True, 1.0), (5000, True, 2.0), (5000, False, 1.0)):
        grad, hess = LR.eager_batch(s, y, group, T=T, norm=norm, sigma=sigma)
        worst = max(worst, LR.gate(grad, hess, LR.reference(name, T, norm, sigma), f"eager {name} T {T} norm {norm} sigma {sigma}"))
    print(f"eager fp32 on {name}: needs C_PAIR >= {worst * FB.C_PAIR:.2f}")


FAULT_GROUP = [40, 130]


def fault_inputs(fault):
    s, y = TR.tree_inputs(FAULT_GROUP, seed=3)
    y = LR.plant_relevant(y, FAULT_GROUP)
    if fault == "divide_equal":
        s = np.full_like(s, 0.25)
    return s, y


@pytest.mark.parametrize("fault", LR.FAULTS)
def test_the_gate_rejects_a_planted_fault(fault):
    s, y = fault_inputs(fault)
    kw = dict(T=10, norm=True, sigma=2.0)
    ref = LR.batch(s, y, FAULT_GROUP, **kw)
    LR.gate(*LR.eager_batch(s, y, FAULT_GROUP, **kw), ref, f"unfaulted, the inputs of {fault}")
    with pytest.raises(AssertionError, match="bound failed"):
        LR.gate(*LR.eager_batch(s, y, FAULT_GROUP, fault=fault, **kw), ref, fault)


# ---------------------------------------------------------------------------------------------------------------- 3. the parameters
def test_the_three_settings_are_parameters_under_lightgbms_names():
    from ptranking_amd import gbdt
    for k, v in NEW_DEFAULTS.items():
        assert gbdt.DEFAULT_PARAMS[k] == v and type(gbdt.DEFAULT_PARAMS[k]) is type(v), k
        assert gbdt._params({k: v})[k] == v and gbdt.GBDT({k: v}).params == gbdt.GBDT().params
        assert k not in gbdt.IGNORED_PARAMS
    p = gbdt._params({"lambdarank_truncation_level": 5, "lambdarank_norm": False, "sigmoid": 2, "objective": "lambdarank"})
    assert (p["lambdarank_truncation_level"], p["lambdarank_norm"], p["sigmoid"]) == (5, False, 2.0)
    assert type(p["lambdarank_truncation_level"]) is int and type(p["sigmoid"]) is float and type(p["lambdarank_norm"]) is bool
    assert "objective" not in p and "objective" in gbdt.IGNORED_PARAMS                     # accepted and ignored, as before
    assert gbdt._params({"lambdarank_truncation_level": np.int64(7), "lambdarank_norm": np.bool_(False)})["lambdarank_truncation_level"] == 7
    with pytest.raises(ValueError, match="unknown parameter 'label_gain'"):
        gbdt._params({"label_gain": [0, 1, 3, 7]})
    # the reference's own dictionary passes through (lightgbm_lambdaMART.py:170-185, without its num_iterations alias)
    gbdt._params({"boosting_type": "gbdt", "objective": "lambdarank", "metric": "ndcg", "learning_rate": 0.05, "num_leaves": 400,
                  "num_trees": 1000, "num_threads": 16, "min_data_in_leaf": 50, "min_sum_hessian_in_leaf": 200, "eval_at": 5,
                  "verbosity": -1, "lambdarank_truncation_level": 30, "lambdarank_norm": True, "sigmoid": 1.0})


BAD = [{"lambdarank_truncation_level": 0}, {"lambdarank_truncation_level": -3}, {"lambdarank_truncation_level": 2.5},
       {"lambdarank_truncation_level": float("nan")}, {"lambdarank_truncation_level": True}, {"lambdarank_truncation_level": "30"},
       {"lambdarank_truncation_level": None}, {"lambdarank_norm": 1}, {"lambdarank_norm": "true"}, {"lambdarank_norm": None},
       {"sigmoid": 0.0}, {"sigmoid": -1.0}, {"sigmoid": float("nan")}, {"sigmoid": float("inf")}, {"sigmoid": 1e-60}, {"sigmoid": "1"},
       {"sigmoid": None}, {"sigmoid": True}]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join(f"{k}={v!r}" for k, v in d.items()))
def test_bad_settings_raise_before_any_gpu_is_asked_for(bad, monkeypatch):
    from ptranking_amd import gbdt
    import ptranking_amd as pa
    import ptranking_amd.functional as F_
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError) as e:
        gbdt._params(bad)
    assert "unknown parameter" not in str(e.value) and next(iter(bad)) in str(e.value)
    for build in (lambda: gbdt.GBDT(bad), lambda: gbdt.LambdaMART(bad, objective="lambdarank_ndcg"), lambda: gbdt.LambdaMART(bad)):
        with pytest.raises(ValueError):
            build()
    kw = {{"lambdarank_truncation_level": "truncation_level", "lambdarank_norm": "norm", "sigmoid": "sigmoid"}[k]: v for k, v in bad.items()}
    with pytest.raises(ValueError):
        pa.TreeObjective(objective="lambdarank_ndcg", **kw)
    with pytest.raises(ValueError):
        F_.tree_lambdarank_ndcg_grad_hess(torch.zeros(3), torch.zeros(3), torch.tensor([0, 3]), **kw)


def test_settings_of_the_other_objectives_do_not_apply(monkeypatch):
    from ptranking_amd import gbdt
    import ptranking_amd as pa
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for kw in (dict(weighting=None), dict(weighting="DeltaGain"), dict(hessian="reference"), dict(hessian="constant"), dict(pair_type="NoTies"),
               dict(epsilon=2.0), dict(gain_type="Label")):
        with pytest.raises(ValueError, match=f"{next(iter(kw))}=.*does not apply"):
            gbdt.LambdaMART(objective="lambdarank_ndcg", **kw)
    for kw in (dict(weighting="DeltaNDCG"), dict(hessian="sum"), dict(pair_type="All"), dict(epsilon=0.5), dict(gain_type="Label")):
        with pytest.raises(ValueError, match=f"{next(iter(kw))}=.*does not apply"):
            pa.TreeObjective(objective="lambdarank_ndcg", **kw)
    lazy = pa.TreeObjective(objective="lambdarank_ndcg", truncation_level=7, sigmoid=2, norm=False)
    assert (lazy.kind, lazy.truncation_level, lazy.sigmoid, lazy.norm, lazy.uploads) == ("lambdarank_ndcg", 7, 2.0, False, 0)
    assert pa.TreeObjective(objective="lambdarank_ndcg").truncation_level == 30
    assert pa.tree.OBJECTIVES["lambdarank_ndcg"][0] == "lambdarank_ndcg" and list(pa.tree.OBJECTIVES)[:3] == ["ranknet", "lambdarank", "listnet"]
    assert len(pa.tree.DROP_IN_NAMES) == 6 and not any("ndcg" in n for n in pa.tree.DROP_IN_NAMES)
    # the defaults stay: LambdaMART's objective is the custom all-pairs 'lambdarank'
    import inspect
    assert inspect.signature(gbdt.LambdaMART.__init__).parameters["objective"].default == "lambdarank"


def test_without_a_gpu_the_new_paths_raise_loudly(monkeypatch):
    from ptranking_amd import gbdt
    import ptranking_amd as pa
    import ptranking_amd.functional as F_
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    labels, group = np.array([1.0, 0.0, 2.0]), np.array([3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gbdt.LambdaMART({"lambdarank_truncation_level": 5}, objective="lambdarank_ndcg")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pa.TreeObjective(labels, group, "lambdarank_ndcg")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pa.TreeObjective(objective="lambdarank_ndcg").sklearn(labels, np.zeros(3), group)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.tree_lambdarank_ndcg_grad_hess(torch.zeros(3), torch.zeros(3), torch.tensor([0, 3]))


def test_the_settings_travel_in_the_model_file_and_an_older_file_loads(tmp_path):
    from ptranking_amd import gbdt
    m = gbdt.GBDT({"lambdarank_truncation_level": 12, "lambdarank_norm": False, "sigmoid": 2.0, "num_leaves": 4, "max_bin": 16})
    m.edges, m.nbins = np.full((2, 15), np.inf, np.float32), np.ones(2, np.int32)
    m.trees = [{"feature": np.array([0], np.int32), "threshold": np.array([0.5], np.float32), "left": np.array([~0], np.int32),
                "right": np.array([~1], np.int32), "value": np.array([-1.0, 1.0], np.float32)}]
    m.save_model(tmp_path / "m.npz")
    back = gbdt.GBDT.load_model(tmp_path / "m.npz")
    assert back.params == m.params and back.params["lambdarank_truncation_level"] == 12 and back.params["lambdarank_norm"] is False
    with np.load(tmp_path / "m.npz", allow_pickle=False) as z:
        store = {k: z[k] for k in z.files}
    assert int(store["format"]) == 1
    old = json.loads(str(store["params"]))
    for k in NEW_DEFAULTS:
        del old[k]                                                         # the file as it was written before the three keys existed
    store["params"] = np.array(json.dumps(old))
    with open(tmp_path / "old.npz", "wb") as fh:
        np.savez(fh, **store)
    parent = gbdt.GBDT.load_model(tmp_path / "old.npz")
    assert {k: parent.params[k] for k in NEW_DEFAULTS} == NEW_DEFAULTS and len(parent.trees) == 1


# ---------------------------------------------------------------------------------------------------------------- 4. the ABI
def test_the_symbol_is_declared_exported_and_bound(lib):
    from ptranking_amd import _lib
    import ptranking_amd.functional as F_
    doc = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == _lib.ABI_VERSION == lib.ptr_abi_version()
    proto = re.search(ENTRY + r"\s*\(([^)]*)\)", src).group(1)
    assert hasattr(lib, ENTRY) and proto.count(",") + 1 == len(_lib.SIGNATURES[ENTRY]) == 13
    assert "int truncation_level, float sigmoid, int norm" in proto
    for phrase in ("modelled on LightGBM's LambdarankNDCG", "compared with nothing of LightGBM's", "no parity with it is claimed",
                   "DIFFERS from PTR_TREE_W_DELTA_NDCG", "min(r(i), r(j)) < T", "log2(1 + S) / S", "0.01 + |ds|"):
        assert phrase in doc, phrase
    assert "tree_lambdarank_ndcg_grad_hess" in F_.__all__ and callable(F_.tree_lambdarank_ndcg_grad_hess)
    for name, what in (("COVERAGE.md", "lambdarank_ndcg"), ("DESIGN.md", "lambdarank_ndcg"), ("README.md", "lambdarank_ndcg")):
        text = open(os.path.join(ROOT, name)).read()
        assert what in text and (name == "README.md" or "compared with nothing of LightGBM's" in text), name


def test_argument_errors_need_no_gpu(lib):
    one, f = ctypes.c_void_p(16), ctypes.c_float
    INVALID, UNSUPPORTED = 1001, 1002

    def call(preds=one, labels=one, offsets=one, B=2, queries=None, nq=2, max_len=8, T=30, sigma=1.0, norm=1, grad=one, hess=one):
        return getattr(lib, ENTRY)(preds, labels, offsets, B, queries, nq, max_len, T, f(sigma), norm, grad, hess, None)

    for kw in (dict(preds=None), dict(labels=None), dict(offsets=None), dict(grad=None), dict(hess=None)):
        assert call(**kw) == INVALID and b"NULL" in lib.ptr_last_error(), kw
    for kw in (dict(B=-1, nq=-1), dict(nq=-1, queries=one), dict(max_len=-1)):
        assert call(**kw) == INVALID and b"negative" in lib.ptr_last_error(), kw
    assert call(nq=1) == INVALID and b"nq must equal B" in lib.ptr_last_error()
    for T in (0, -1):
        assert call(T=T) == INVALID and b"truncation_level" in lib.ptr_last_error()
    for sigma in (0.0, -1.0, float("nan")):
        assert call(sigma=sigma) == INVALID and b"sigmoid" in lib.ptr_last_error()
    assert call(max_len=4097) == UNSUPPORTED and b"PTR_MAX_LIST_LEN" in lib.ptr_last_error()
    assert call(max_len=4097, T=0) == INVALID                                   # an argument error wins over the unsupported length
    assert call(max_len=4096, B=0, nq=0) == 0
    assert call(preds=None, labels=None, offsets=None, grad=None, hess=None, B=0, nq=0) == 0
    assert call(preds=None, labels=None, offsets=None, grad=None, hess=None, B=3, queries=one, nq=0) == 0
