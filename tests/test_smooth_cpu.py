"""CPU: the smooth-rank metric objectives (csrc/smoothmetric.hip) — the float64 restatement (tests/smooth_ref.py) against the reference's own
float64 runs (tests/golden/smooth_metric.npz), central differences, the fairness of the golden gate, the ABI and the Python surface."""
import ctypes
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import smooth_ref as SR
from f64_loss_bounds import C_APPROX, gate_nan
from golden_util import _load, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
NAMES = ("P", "AP", "nERR", "nDCG")
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=12, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False)}
# Restatement vs the reference's float64: P and AP are the same arithmetic in another order (1e-11).  nERR and nDCG get 1e-8 because the
# reference's float64 runs are not float64 throughout: it forms its ideal ERR from fp32 pieces (torch.tensor([2.0], dtype=torch.float) and an
# fp32 rank row, adhoc_metric.py:132-139) and its IDCG with an fp32 discount table (torch_dcg_at_k's fp32 arange), worth 5.8e-10 and 3.9e-9.
RTOL64 = {"P": 1e-11, "AP": 1e-11, "nERR": 1e-8, "nDCG": 1e-8}


@pytest.fixture(scope="module")
def golden():
    return _load("smooth_metric.npz")


def rows(case):
    """(metric name, opt_ideal, top_k or None, res64, res32, valid) per recorded run of a golden case."""
    for k, (m, oi, tk) in enumerate(case["combos"]):
        yield NAMES[m], bool(oi), (int(tk) or None), case["res64"][k], case["res32"][k], case["valid"][k]


def restate(case, metric, opt_ideal, top_k):
    """The restatement on a golden case -> (loss, grad flattened over the batch, valid [B])."""
    P, Y = np.atleast_2d(case["preds"]), np.atleast_2d(case["labels"])
    st = SR.stages(P, None, float(case["alpha"]), C_APPROX)
    res = SR.smooth(st, Y, None, metric, top_k, opt_ideal, float(case["max_label"]))
    return res["loss_q"].sum(), res["grad"].reshape(-1), res["valid_q"]


def test_restatement_reproduces_every_golden_float64_run(golden):
    n_runs = 0
    for fam in ("main", "edge"):
        for name, case in golden[fam].items():
            for metric, oi, tk, r64, _, valid in rows(case):
                loss, grad, v = restate(case, metric, oi, tk)
                got = np.concatenate([[loss], grad])
                what = f"{fam}/{name} {metric} opt_ideal={oi} top_k={tk}"
                assert np.array_equal(np.isnan(got), np.isnan(r64)), f"{what}: NaN placement {got} vs {r64}"
                fin = np.isfinite(r64)
                tol = RTOL64[metric] * max(1.0, float(np.abs(r64[fin]).max())) if fin.any() else 0.0
                assert np.all(np.abs(got[fin] - r64[fin]) <= RTOL64[metric] * np.abs(r64[fin]) + 1e-3 * tol), \
                    f"{what}: worst {np.abs(got[fin] - r64[fin]).max():.3e}"
                assert np.array_equal(v, valid), what
                n_runs += 1
    assert n_runs == 470


def test_restatement_gradient_is_the_derivative_of_its_loss(golden):
    """Central differences in float64 on the restatement itself (cases of 17 documents, every form)."""
    for name in ("n17_a1", "n17_a10"):
        case = golden["main"][name]
        s0, y, alpha = case["preds"].astype(np.float64), case["labels"], float(case["alpha"])
        for metric, oi, tk, _, _, valid in rows(case):
            if not valid[0]:
                continue
            base = SR.query(SR.PairStage(s0, alpha), y, metric, tk, oi, float(case["max_label"]))
            h = 1e-6
            for i in (0, 5, 16):
                lo, hi = s0.copy(), s0.copy()
                lo[i] -= h; hi[i] += h
                fd = (SR.query(SR.PairStage(hi, alpha), y, metric, tk, oi, float(case["max_label"]))["loss"]
                      - SR.query(SR.PairStage(lo, alpha), y, metric, tk, oi, float(case["max_label"]))["loss"]) / (2 * h)
                assert abs(fd - base["grad"][i]) <= 1e-6 * max(1.0, np.abs(base["grad"]).max()), (name, metric, oi, tk, i, fd, base["grad"][i])


def test_the_references_fp32_passes_the_golden_gate_on_every_main_case(golden):
    """The condition under which holding the kernel to assert_close against the reference's float64 is fair: the fp32 evaluation it replaces
    passes the same gate on the same inputs."""
    for name, case in golden["main"].items():
        for metric, oi, tk, r64, r32, _ in rows(case):
            assert_close(r32, r64, f"main/{name} {metric} opt_ideal={oi} top_k={tk} (reference fp32 vs float64)")


def test_a_planted_weight_fault_fails_the_float64_gate(golden):
    """One W_i moved by 1e-5 of its value fails the gate the GPU tests apply (loss_q and every gradient element, each under its own bound);
    the clean restatement passes it.  The fault shows in the gradient elements: the document's own coefficient moves by 1e-5, ten times the
    bound of an element it dominates, while the query's loss — a sum over all documents — may stay inside its own bound."""
    def full_gate(got, ref, what):
        gate_nan(np.array([got["loss"]]), np.array([ref["loss"]]), np.array([ref["E_loss"]]), f"{what} loss_q", C_APPROX)
        gate_nan(got["grad"], ref["grad"], ref["E_grad"], f"{what} grad", C_APPROX)

    # short lists: the bound of a smooth rank grows with the list (E_pi sums one sigmoid error per partner: ~1e-5 of r for the top documents
    # of 64), and a fault can only show where the bounds are tighter than it
    for name, alpha in (("n3_a10", 10.0), ("n3_a1", 1.0), ("n17_a10", 10.0)):
        case = golden["main"][name]
        st = SR.PairStage(case["preds"], alpha)
        for metric in NAMES:
            ref = SR.query(st, case["labels"], metric, None, True, float(case["max_label"]))
            i = int(np.argmax(ref["W"] / (st.r if metric != "nDCG" else np.log2(1.0 + st.r))))
            bad = SR.query(st, case["labels"], metric, None, True, float(case["max_label"]), fault=(i, 1e-5))
            full_gate(ref, ref, "clean")
            with pytest.raises(AssertionError):
                full_gate(bad, ref, f"{name} {metric} planted")


def test_torch_composition_matches_the_golden_runs(golden):
    """smooth_ref.torch_composition (the eager restatement of the reference's op sequence that the GPU tests and the profile run on the
    device, where the reference is not) returns the reference's float64 results."""
    for name in ("n17_a10", "n65_a1"):
        case = golden["main"][name]
        for metric, oi, tk, r64, _, _ in rows(case):
            loss, grad = SR.torch_composition(torch.from_numpy(case["preds"]).double(), torch.from_numpy(case["labels"]), metric,
                                              float(case["alpha"]), tk, oi, float(case["max_label"]))
            got = np.concatenate([[float(loss)], grad.numpy()])
            assert np.allclose(got, r64, rtol=1e-8, atol=1e-12), (name, metric, oi, tk)


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbol_is_declared_exported_and_bound(lib):
    from ptranking_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"ptr_smoothmetric_fwd_bwd\s*\(([^)]*)\)", src).group(1)
    assert proto.count(",") + 1 == len(_lib.SIGNATURES["ptr_smoothmetric_fwd_bwd"]) == 17
    assert hasattr(lib, "ptr_smoothmetric_fwd_bwd")
    for k, v in (("P", 0), ("AP", 1), ("NERR", 2), ("NDCG", 3)):
        assert re.search(rf"#define PTR_SMOOTH_{k} {v}\b", src)
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == lib.ptr_abi_version() == _lib.ABI_VERSION
    from ptranking_amd import build
    assert "smoothmetric.hip" in build.SOURCES


def test_every_argument_error_needs_no_gpu(lib):
    f, one = ctypes.c_float, ctypes.c_void_p(16)
    call = lib.ptr_smoothmetric_fwd_bwd

    def args(preds=one, labels=one, B=1, L=8, metric=0, alpha=10.0, max_label=4.0, loss_q=one, ws=None, grad=one):
        return (preds, labels, None, B, L, metric, 1, 0, f(alpha), f(max_label), None, loss_q, None, None, ws, grad, None)
    for bad, word in ((dict(preds=None), b"NULL"), (dict(labels=None), b"NULL"), (dict(loss_q=None), b"NULL"), (dict(grad=None), b"NULL"),
                      (dict(metric=4), b"metric"), (dict(metric=-1), b"metric"), (dict(alpha=0.0), b"alpha"), (dict(alpha=-1.0), b"alpha"),
                      (dict(alpha=float("nan")), b"alpha"), (dict(L=4097), b"PTR_MAX_LIST_LEN"), (dict(L=0), b"shape"),
                      (dict(metric=2, max_label=-1.0), b"max_label_ws")):
        assert call(*args(**bad)) == 1001 and word in lib.ptr_last_error(), bad
    assert call(*args(B=0, preds=None, labels=None, loss_q=None, grad=None)) == 0          # an empty batch launches nothing


def test_cpu_tensors_raise():
    import ptranking_amd.functional as F
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.smooth_metric_objective(torch.zeros(2, 4), torch.zeros(2, 4), "AP")
    with pytest.raises(ValueError, match="metric"):
        F.smooth_metric_objective(torch.zeros(2, 4), torch.zeros(2, 4), "MRR")


def test_public_names():
    import ptranking_amd as pa
    import ptranking_amd.functional as F
    assert "smooth_metric_objective" in F.__all__ and "SMOOTH_METRICS" in F.__all__
    assert not [n for n in F.__all__ if "smooth" in n and n.endswith("_loss")]              # the *_loss set of __all__ is pinned elsewhere
    assert {k: F.SMOOTH_METRICS[k] for k in NAMES} == {"P": 0, "AP": 1, "nERR": 2, "nDCG": 3}
    assert pa.METRIC_RANKER_NAMES == ("SmoothMetric",)
    assert pa.RANKER_NAMES == ("RankNet", "LambdaRank", "LambdaLoss", "ApproxNDCG", "ListNet", "ListMLE", "STListNet", "RankCosine", "RankMSE",
                               "SoftRank", "WassRank")
    assert pa.EXTRA_RANKER_NAMES == ("DASALC", "MDPRank")
    assert pa.SmoothMetric is pa.rankers.SmoothMetric and pa.DEFAULT_PARAS["SmoothMetric"]["metric"] == "nDCG"


def test_class_signature_and_eval_setting():
    import ptranking_amd as pa
    assert list(inspect.signature(pa.SmoothMetric.__init__).parameters) == ["self", "sf_para_dict", "model_para_dict", "gpu", "device"]
    r = pa.SmoothMetric(sf_para_dict=SF, model_para_dict=dict(metric="AP", alpha=10.0, top_k=10, opt_ideal=False), gpu=False, device="cpu")
    assert (r.metric, r.alpha, r.top_k, r.opt_ideal, r.max_label) == ("AP", 10.0, 10, False, None)
    ed = dict(do_validation=True, vali_metric="nDCG")
    r.uniform_eval_setting(eval_dict=ed)
    assert ed["vali_metric"] == "AP"
    d = pa.SmoothMetric(sf_para_dict=SF, model_para_dict=pa.DEFAULT_PARAS["SmoothMetric"], gpu=False, device="cpu")
    assert (d.metric, d.top_k, d.opt_ideal) == ("nDCG", None, True)
    with pytest.raises(NotImplementedError):
        pa.SmoothMetric(sf_para_dict=SF, model_para_dict=dict(metric="MRR", alpha=10.0, top_k=None, opt_ideal=True), gpu=False, device="cpu")
    with pytest.raises(AssertionError):                                                     # presort is asserted, as the reference does
        r.custom_loss_function(torch.zeros(1, 4), torch.zeros(1, 4), presort=False, label_type=pa.LABEL_TYPE.MultiLabel)


def test_install_with_explicit_names_round_trips(monkeypatch):
    """install(names=RANKER_NAMES + METRIC_RANKER_NAMES) binds SmoothMetric in the driver module and uninstall() takes it away again; the
    default install() leaves it alone.  (Stand-in driver modules: the round trip is the same code path as with the reference installed.)"""
    import ptranking_amd as pa
    from ptranking_amd.host import PointScorerRanker
    ltr = types.ModuleType("fake_smooth_ltr")
    ltr.LambdaRank = object
    base_mod = types.ModuleType("ptranking.base.adhoc_ranker")
    base_mod.AdhocNeuralRanker = PointScorerRanker
    monkeypatch.setitem(sys.modules, "fake_smooth_ltr", ltr)
    for name in ("ptranking", "ptranking.base"):
        if name not in sys.modules:
            monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    monkeypatch.setitem(sys.modules, "ptranking.base.adhoc_ranker", base_mod)
    done = pa.install(ltr_module="fake_smooth_ltr")
    try:
        assert set(done) == set(pa.RANKER_NAMES) and not hasattr(ltr, "SmoothMetric")
    finally:
        pa.uninstall("fake_smooth_ltr")
    done = pa.install(names=pa.RANKER_NAMES + pa.METRIC_RANKER_NAMES, ltr_module="fake_smooth_ltr")
    try:
        assert set(done) == set(pa.RANKER_NAMES) | {"SmoothMetric"}
        assert ltr.SmoothMetric is done["SmoothMetric"] and issubclass(ltr.SmoothMetric, PointScorerRanker)
        assert ltr.LambdaRank is done["LambdaRank"]
    finally:
        pa.uninstall("fake_smooth_ltr")
    assert not hasattr(ltr, "SmoothMetric") and ltr.LambdaRank is object
