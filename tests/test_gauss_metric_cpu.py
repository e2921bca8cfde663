"""CPU: the Gaussian expected-rank metric objectives (csrc/gaussmetric.hip) — the float64 restatement (tests/gauss_metric_ref.py) against the
reference's own float64 runs (tests/golden/gauss_metric.npz), central differences in the means and the variances, the fairness of the golden
gate, where C_GAUSS comes from, the ABI and the Python surface."""
import ctypes
import inspect
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import gauss_metric_ref as GR
from f64_loss_bounds import gate_nan
from gauss_metric_ref import C_GAUSS, NAMES
from golden_util import _load, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=12, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False)}
# Restatement vs the reference's float64: the tightest each metric meets.  P and AP are the same arithmetic in another order (worst 8.9e-14
# and 7.5e-14 of the element, 1e-3 of the row maximum as the floor).  nERR and nDCG get 1e-8 for the reason tests/test_smooth_cpu.py states:
# the reference forms its ideal ERR and its IDCG from fp32 pieces even in a float64 run (worst 5.8e-10 and 3.2e-9).
RTOL64 = {"P": 1e-12, "AP": 1e-12, "nERR": 1e-8, "nDCG": 1e-8}
N_RUNS = 724


@pytest.fixture(scope="module")
def golden():
    return _load("gauss_metric.npz")


def rows(case):
    """(metric name, opt_ideal, top_k or None, res64, res32, valid) per recorded run of a golden case."""
    for k, (m, oi, tk) in enumerate(case["combos"]):
        yield NAMES[m], bool(oi), (int(tk) or None), case["res64"][k], case["res32"][k], case["valid"][k]


def case_inputs(case):
    """(mus [B, n], vars [B, n] float64 — const_std^2 in the constant-variance family —, labels, has_vars)"""
    M, Y = np.atleast_2d(case["mus"]), np.atleast_2d(case["labels"])
    if "vars" in case:
        return M, np.atleast_2d(case["vars"]), Y, True
    return M, np.full(M.shape, float(case["const_std"]) ** 2), Y, False


def restate(case, st, metric, opt_ideal, top_k):
    """The restatement on a golden case -> (loss, both gradients flattened as the fixture has them, valid [B])."""
    M, V, Y, has_vars = case_inputs(case)
    res = GR.batch(st, Y, None, metric, top_k, opt_ideal, float(case["max_label"]))
    return np.concatenate([[res["loss_q"].sum()], res["grad_mu"].reshape(-1)] + ([res["grad_var"].reshape(-1)] if has_vars else [])), res["valid_q"]


def test_restatement_reproduces_every_golden_float64_run(golden):
    n_runs = 0
    for fam in ("main", "edge"):
        for name, case in golden[fam].items():
            M, V, Y, _ = case_inputs(case)
            st = GR.stages(M, V, None)
            assert np.array_equal(np.argsort(np.stack([s.pos for s in st]), axis=1), np.atleast_2d(case["order"])), f"{fam}/{name}: sort order"
            np.testing.assert_allclose(np.stack([s.r for s in st]), np.atleast_2d(case["ranks64"]), rtol=1e-13)
            for metric, oi, tk, r64, _, valid in rows(case):
                got, v = restate(case, st, metric, oi, tk)
                what = f"{fam}/{name} {metric} opt_ideal={oi} top_k={tk}"
                assert np.array_equal(np.isnan(got), np.isnan(r64)), f"{what}: NaN placement {got} vs {r64}"
                fin = np.isfinite(r64)
                tol = RTOL64[metric] * max(1.0, float(np.abs(r64[fin]).max())) if fin.any() else 0.0
                assert np.all(np.abs(got[fin] - r64[fin]) <= RTOL64[metric] * np.abs(r64[fin]) + 1e-3 * tol), \
                    f"{what}: worst {np.abs(got[fin] - r64[fin]).max():.3e}"
                assert np.array_equal(v, valid), what
                n_runs += 1
    assert n_runs == N_RUNS


def test_fixture_grid_and_rank_separation(golden):
    """The grid the issue names, and adjacent sorted float64 expected ranks more than 1e-3 apart in every main case."""
    want = {f"{fam}_n{n}" for fam in ("wide", "head", "const") for n in (1, 2, 3, 17, 64, 65, 130)}
    assert set(golden["main"]) == want
    assert {"n1_norel", "norel_n5", "rel_beyond_k", "topk_gt_n", "batch3"} <= set(golden["edge"])
    for name, case in golden["main"].items():
        r = np.sort(np.atleast_2d(case["ranks64"]), axis=1)
        assert r.shape[1] < 2 or np.diff(r, axis=1).min() > 1e-3, name
        n = r.shape[1]
        forms = {(m, oi, tk) for m, oi, tk in case["combos"].tolist()}
        for m in range(4):
            for oi in (0, 1):
                for tk in {0, 1, 5, n}:
                    assert (m, oi, tk) in forms or (m == 2 and tk > n), (name, m, oi, tk)
        v = case["vars"] if "vars" in case else None
        if name.startswith("wide"):
            assert v.min() >= 0.05 and v.max() <= 1.05
        elif name.startswith("head"):
            assert v.min() >= 1e-4 and v.max() <= 1e-2
        else:
            assert v is None and float(case["const_std"]) == 0.5
    assert golden["edge"]["batch3"]["valid"][0].tolist() == [1.0, 0.0, 1.0]


def test_restatement_gradients_are_the_derivatives_of_its_loss(golden):
    """Central differences in float64 on the restatement itself, in the means and in the variances (17 documents, every form)."""
    for name in ("wide_n17", "head_n17"):
        case = golden["main"][name]
        m0, v0, y, ml = case["mus"].astype(np.float64), case["vars"].astype(np.float64), case["labels"], float(case["max_label"])
        scale = 1e-6 if name == "wide_n17" else 1e-8
        for metric, oi, tk, _, _, valid in rows(case):
            if not valid[0]:
                continue
            base = GR.query(GR.PairStage(m0, v0), y, metric, tk, oi, ml)
            f = lambda m, v: GR.query(GR.PairStage(m, v), y, metric, tk, oi, ml, pos=base["pos"])["loss"]
            for i in (0, 5, 16):
                for which, key, h in ((0, "grad_mu", scale * 10), (1, "grad_var", scale)):
                    lo, hi = [m0.copy(), v0.copy()], [m0.copy(), v0.copy()]
                    lo[which][i] -= h; hi[which][i] += h
                    fd = (f(*hi) - f(*lo)) / (2 * h)
                    assert abs(fd - base[key][i]) <= 1e-5 * max(1.0, np.abs(base[key]).max()), (name, metric, oi, tk, i, key, fd, base[key][i])


def test_the_references_fp32_passes_the_golden_gate_on_every_main_case(golden):
    """The condition under which holding the kernel to assert_close against the reference's float64 is fair: the fp32 evaluation it replaces
    passes the same gate on the same inputs."""
    for name, case in golden["main"].items():
        for metric, oi, tk, r64, r32, _ in rows(case):
            assert_close(r32, r64, f"main/{name} {metric} opt_ideal={oi} top_k={tk} (reference fp32 vs float64)")


def test_a_planted_weight_fault_fails_the_float64_gate(golden):
    """One W_i moved by 1e-5 of its value fails the gate the GPU tests apply (loss_q and every element of both gradients, each under its own
    bound); the clean restatement passes it."""
    def full_gate(got, ref, what):
        gate_nan(np.array([got["loss"]]), np.array([ref["loss"]]), np.array([ref["E_loss"]]), f"{what} loss_q", C_GAUSS)
        gate_nan(got["grad_mu"], ref["grad_mu"], ref["E_grad_mu"], f"{what} grad_mu", C_GAUSS)
        gate_nan(got["grad_var"], ref["grad_var"], ref["E_grad_var"], f"{what} grad_var", C_GAUSS)

    for name in ("wide_n3", "head_n3", "wide_n17"):
        case = golden["main"][name]
        st = GR.PairStage(case["mus"], case["vars"])
        for metric in NAMES:
            ref = GR.query(st, case["labels"], metric, None, True, float(case["max_label"]))
            i = int(np.argmax(ref["W"] / (st.r if metric != "nDCG" else np.log2(1.0 + st.r))))
            bad = GR.query(st, case["labels"], metric, None, True, float(case["max_label"]), fault=(i, 1e-5))
            full_gate(ref, ref, "clean")
            with pytest.raises(AssertionError):
                full_gate(bad, ref, f"{name} {metric} planted")


def test_torch_composition_matches_the_golden_runs(golden):
    """gauss_metric_ref.torch_composition (the eager restatement of the reference's op sequence that the C_GAUSS measurement and the profile
    run, where the reference is not) returns the reference's float64 results."""
    for name in ("wide_n17", "head_n65", "const_n17"):
        case = golden["main"][name]
        const = float(case["const_std"]) if "const_std" in case else None
        for metric, oi, tk, r64, _, _ in rows(case):
            if metric == "nERR" and tk and tk > case["mus"].size:
                continue
            v = None if const else torch.from_numpy(case["vars"]).double()
            loss, gm, gv, _ = GR.torch_composition(torch.from_numpy(case["mus"]).double(), v, torch.from_numpy(case["labels"]), metric, tk, oi,
                                                   float(case["max_label"]), const_std=const)
            got = np.concatenate([[float(loss)], gm.numpy()] + ([] if const else [gv.numpy()]))
            assert np.allclose(got, r64, rtol=1e-8, atol=1e-12), (name, metric, oi, tk)


def test_c_gauss_is_twice_the_fp32_need_rounded_up_to_a_half():
    """C_GAUSS is not chosen: it is 2 x what the reference's own fp32 arithmetic needs of these bounds on the small batches of the GPU gate,
    rounded up to a half: C_GAUSS is that value, or one step above it where another machine's torch sums in another order and needs less."""
    need = GR.measure_fp32_need()
    worst = max(need.values())
    print("MEASURED fp32 need of the eager-torch composition per output: " + ", ".join(f"{k} {v:.2f}" for k, v in need.items()))
    derived = math.ceil(2.0 * worst * 2.0) / 2.0
    assert 0.0 <= C_GAUSS - derived <= 0.5, (need, derived, C_GAUSS)


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbol_is_declared_exported_and_bound(lib):
    from ptranking_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"ptr_gaussmetric_fwd_bwd\s*\(([^)]*)\)", src).group(1)
    assert proto.count(",") + 1 == len(_lib.SIGNATURES["ptr_gaussmetric_fwd_bwd"]) == 20
    assert hasattr(lib, "ptr_gaussmetric_fwd_bwd")
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == lib.ptr_abi_version() == _lib.ABI_VERSION
    assert "gaussmetric.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "ptranking_amd", "csrc", "gaussmetric.hip"))
    # the pair primitives and the weight step are shared through headers, not copied
    csrc = os.path.join(ROOT, "ptranking_amd", "csrc")
    for fn, header in (("pair_geo", "ptr_gauss.h"), ("pair_phi", "ptr_gauss.h"), ("smooth_weights", "ptr_smooth.h"), ("wave_scan_row", "ptr_smooth.h")):
        defs = [f for f in sorted(os.listdir(csrc)) if os.path.isfile(os.path.join(csrc, f))
                and re.search(rf"__device__ __forceinline__ [\w ]+\b{fn}\(", open(os.path.join(csrc, f)).read())]
        assert defs == [header], (fn, defs)


def test_every_argument_error_needs_no_gpu(lib):
    f, one = ctypes.c_float, ctypes.c_void_p(16)
    call = lib.ptr_gaussmetric_fwd_bwd

    def args(mus=one, vars_=one, labels=one, B=1, L=8, metric=0, const_std=0.0, max_label=4.0, loss_q=one, ws=None, grad_mu=one, grad_var=one):
        return (mus, vars_, labels, None, B, L, metric, 1, 0, f(const_std), f(max_label), None, loss_q, None, None, None, ws, grad_mu, grad_var, None)
    for bad, word in ((dict(mus=None), b"NULL"), (dict(labels=None), b"NULL"), (dict(loss_q=None), b"NULL"), (dict(grad_mu=None), b"NULL"),
                      (dict(vars_=None, const_std=0.0), b"const_std"), (dict(vars_=None, const_std=-1.0), b"const_std"),
                      (dict(vars_=None, const_std=float("nan")), b"const_std"), (dict(grad_var=None), b"grad_var"),
                      (dict(metric=4), b"metric"), (dict(metric=-1), b"metric"), (dict(L=4097), b"PTR_MAX_LIST_LEN"), (dict(L=0), b"shape"),
                      (dict(metric=2, max_label=-1.0), b"max_label_ws")):
        assert call(*args(**bad)) == 1001 and word in lib.ptr_last_error(), bad
    assert call(*args(B=0, mus=None, labels=None, loss_q=None, grad_mu=None)) == 0          # an empty batch launches nothing
    assert call(*args(B=0, vars_=None, const_std=0.5, grad_var=None, mus=None, labels=None, loss_q=None, grad_mu=None)) == 0


def test_cpu_tensors_raise():
    import ptranking_amd.functional as F
    z = torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.gaussian_metric_objective(z, z + 1, z, "AP")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.gaussian_metric_objective(z, None, z, "AP", const_std=0.5)
    with pytest.raises(ValueError, match="metric"):
        F.gaussian_metric_objective(z, z + 1, z, "MRR")
    with pytest.raises(ValueError, match="const_std"):
        F.gaussian_metric_objective(z, None, z, "AP")
    with pytest.raises(ValueError, match="const_std"):
        F.gaussian_metric_objective(z, None, z, "AP", const_std=0.0)
    with pytest.raises(ValueError, match="not both"):
        F.gaussian_metric_objective(z, z + 1, z, "AP", const_std=0.5)


def test_public_names():
    import ptranking_amd as pa
    import ptranking_amd.functional as F
    assert "gaussian_metric_objective" in F.__all__ and not [n for n in F.__all__ if "gauss" in n and n.endswith("_loss")]
    assert list(inspect.signature(F.gaussian_metric_objective).parameters) == ["mus", "vars", "labels", "metric", "top_k", "opt_ideal", "max_label",
                                                                                "lens", "const_std", "return_parts"]
    assert pa.PROB_RANKER_NAMES == ("ProbSmoothMetric",) == pa.rankers.PROB_RANKER_NAMES
    assert pa.METRIC_RANKER_NAMES == ("SmoothMetric",)
    assert pa.RANKER_NAMES == ("RankNet", "LambdaRank", "LambdaLoss", "ApproxNDCG", "ListNet", "ListMLE", "STListNet", "RankCosine", "RankMSE",
                               "SoftRank", "WassRank")
    assert pa.EXTRA_RANKER_NAMES == ("DASALC", "MDPRank")
    assert pa.ProbSmoothMetric is pa.rankers.ProbSmoothMetric
    d = pa.DEFAULT_PARAS["ProbSmoothMetric"]
    assert (d["metric"], d["top_k"], d["opt_ideal"], d["limit_delta"], d["const_std"], d["sort_id"]) == ("nDCG", None, True, 0.01, None, "ExpRele")


def test_class_signature_heads_and_eval_setting():
    import ptranking_amd as pa
    assert list(inspect.signature(pa.ProbSmoothMetric.__init__).parameters) == ["self", "sf_para_dict", "model_para_dict", "gpu", "device"]
    paras = dict(metric="AP", top_k=10, opt_ideal=False, limit_delta=0.02, sort_id="RiskAware")
    r = pa.ProbSmoothMetric(sf_para_dict=SF, model_para_dict=paras, gpu=False, device="cpu")
    assert (r.metric, r.top_k, r.opt_ideal, r.max_label, r.limit_delta, r.const_std, r.sort_id) == ("AP", 10, False, None, 0.02, None, "RiskAware")
    assert r.sf_para_dict["pointsf"]["out_dim"] == 2 and "out_dim" not in SF["pointsf"]          # the caller's dict is left alone
    ed = dict(do_validation=True, vali_metric="nDCG")
    r.uniform_eval_setting(eval_dict=ed)
    assert ed["vali_metric"] == "AP"
    # the heads: sigmoid * limit_delta, exp, and the constant standard deviation (out_dim = 1)
    comp = torch.tensor([[[0.5, -1.0], [0.25, 2.0]]])
    mus, vars_ = r._head(comp)
    assert torch.equal(mus, comp[:, :, 0]) and torch.equal(vars_, torch.sigmoid(comp[:, :, 1]) * 0.02)
    assert torch.equal(r._sort_scores(mus, vars_), mus - 0.1 * vars_)
    e = pa.ProbSmoothMetric(sf_para_dict=SF, model_para_dict=dict(paras, limit_delta=None, sort_id="ExpRele"), gpu=False, device="cpu")
    assert torch.equal(e._head(comp)[1], torch.exp(comp[:, :, 1])) and e._sort_scores(*e._head(comp)) is not None
    c = pa.ProbSmoothMetric(sf_para_dict=SF, model_para_dict=dict(paras, const_std=0.5), gpu=False, device="cpu")
    assert c.sf_para_dict["pointsf"]["out_dim"] == 1 and c._head(comp[:, :, 0])[1] is None
    assert torch.equal(c._sort_scores(comp[:, :, 0], None), comp[:, :, 0] - 0.1 * 0.25)
    d = pa.ProbSmoothMetric(sf_para_dict=SF, model_para_dict=pa.DEFAULT_PARAS["ProbSmoothMetric"], gpu=False, device="cpu")
    assert (d.metric, d.top_k, d.opt_ideal, d.sort_id) == ("nDCG", None, True, "ExpRele")
    for bad, err in ((dict(metric="MRR"), NotImplementedError), (dict(sort_id="Random"), ValueError), (dict(const_std=0.0), ValueError)):
        with pytest.raises(err):
            pa.ProbSmoothMetric(sf_para_dict=SF, model_para_dict=dict(paras, **bad), gpu=False, device="cpu")
    with pytest.raises(NotImplementedError):
        pa.ProbSmoothMetric(sf_para_dict=dict(SF, sf_id="listsf"), model_para_dict=paras, gpu=False, device="cpu")
    with pytest.raises(AssertionError):                                                     # presort is asserted, as the reference does
        r.custom_loss_function(torch.zeros(1, 4, 2), torch.zeros(1, 4), presort=False, label_type=pa.LABEL_TYPE.MultiLabel)


def test_install_with_explicit_names_round_trips(monkeypatch):
    """install(names=RANKER_NAMES + PROB_RANKER_NAMES) binds ProbSmoothMetric in the driver module and uninstall() takes it away again; the
    default install() and install(names=RANKER_NAMES + METRIC_RANKER_NAMES) leave it alone.  (Stand-in driver modules: the round trip is the
    same code path as with the reference installed.)"""
    import ptranking_amd as pa
    from ptranking_amd.host import PointScorerRanker
    ltr = types.ModuleType("fake_gauss_ltr")
    ltr.LambdaRank = object
    base_mod = types.ModuleType("ptranking.base.adhoc_ranker")
    base_mod.AdhocNeuralRanker = PointScorerRanker
    monkeypatch.setitem(sys.modules, "fake_gauss_ltr", ltr)
    for name in ("ptranking", "ptranking.base"):
        if name not in sys.modules:
            monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    monkeypatch.setitem(sys.modules, "ptranking.base.adhoc_ranker", base_mod)
    for names in (pa.RANKER_NAMES, pa.RANKER_NAMES + pa.METRIC_RANKER_NAMES):
        done = pa.install(names=names, ltr_module="fake_gauss_ltr")
        try:
            assert set(done) == set(names) and not hasattr(ltr, "ProbSmoothMetric")
        finally:
            pa.uninstall("fake_gauss_ltr")
    done = pa.install(names=pa.RANKER_NAMES + pa.PROB_RANKER_NAMES, ltr_module="fake_gauss_ltr")
    try:
        assert set(done) == set(pa.RANKER_NAMES) | {"ProbSmoothMetric"}
        assert ltr.ProbSmoothMetric is done["ProbSmoothMetric"] and issubclass(ltr.ProbSmoothMetric, PointScorerRanker)
        assert ltr.LambdaRank is done["LambdaRank"]
    finally:
        pa.uninstall("fake_gauss_ltr")
    assert not hasattr(ltr, "ProbSmoothMetric") and ltr.LambdaRank is object
