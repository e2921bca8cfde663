"""CPU: FastSoftRank without a GPU — properties of the float64 restatement (tests/fastsoftrank_ref.py) that pin the rule itself, the argument
errors of the C entry point and of the Python surface, the names and the install round trip, the header's statement of the rule."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

import fastsoftrank_ref as R

ENTRY = "ptr_fastsoftrank_fwd_bwd"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ptranking_amd.h")


@pytest.mark.parametrize("n", [1, 2, 17, 200])
def test_stack_pav_equals_the_cumulative_sum_form(n):
    rng = np.random.default_rng(n)
    for scale in (0.3, 3.0, 30.0):
        u = rng.standard_normal(n) * scale - np.arange(n, 0, -1)
        v, start = R.pav(u)
        w, start2, margin = R.cumsum_form(u)
        assert np.abs(v - w).max() <= 1e-12 * np.abs(u).max() and np.all(np.diff(v) <= 0)
        assert margin < 1e-8 or np.array_equal(start, start2)


def test_the_limits_of_eps_and_a_finite_difference_gradient():
    rng = np.random.default_rng(7)
    theta, y = rng.standard_normal(23).astype(np.float32), rng.integers(0, 5, 23).astype(np.float32)
    hard = (theta[None, :] > theta[:, None]).sum(1) + 1.0
    assert np.array_equal(R.query(theta, y, 1e-4, "spearman")["ranks"], hard)
    assert np.abs(R.query(theta, y, 1e4, "spearman")["ranks"] - 12.0).max() <= 2 * np.abs(theta).max() / 1e4      # z - mean(z) remains
    # the keys are fp32, so the difference quotient is taken in z: theta = -eps z with eps = 1/16 and z on a grid fp32 holds exactly
    theta = np.round(theta * 4096) / 4096
    h = 2.0 ** -10
    for objective in ("spearman", "nDCG"):
        ref = R.query(theta, y, 0.0625, objective)
        assert 1 < len(np.unique(ref["start"])) < 23
        for i in range(23):
            d = np.zeros(23, np.float32)
            d[i] = h
            fd = (R.query(theta + d, y, 0.0625, objective)["loss"] - R.query(theta - d, y, 0.0625, objective)["loss"]) / (2 * h)
            assert abs(fd - ref["grad"][i]) <= 1e-5 * max(1.0, np.abs(ref["grad"]).max()), (objective, i)


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


def _args(preds=16, labels=16, B=1, L=8, eps=1.0, objective=1, loss_q=16):
    p = lambda a: ctypes.c_void_p(a) if a else None
    return (p(preds), p(labels), None, B, L, ctypes.c_float(eps), objective, None, p(loss_q), None, None, None)


@pytest.mark.parametrize("bad, code, word", [(dict(B=-1), 1001, b"shape"), (dict(L=0), 1001, b"shape"), (dict(L=4097), 1002, b"PTR_MAX_LIST_LEN=4096"),
                                             (dict(eps=0.0), 1001, b"eps"), (dict(eps=float("nan")), 1001, b"eps"), (dict(objective=2), 1001, b"objective"),
                                             (dict(preds=0), 1001, b"NULL"), (dict(labels=0), 1001, b"NULL"), (dict(loss_q=0), 1001, b"NULL")])
def test_argument_errors_need_no_gpu(lib, bad, code, word):
    assert getattr(lib, ENTRY)(*_args(**bad)) == code and word in lib.ptr_last_error()
    assert getattr(lib, ENTRY)(*_args(B=0, preds=0, labels=0, loss_q=0)) == 0                # an empty batch launches nothing


def test_python_surface_names_and_header():
    import ptranking_amd as pa
    F, z = pa.functional, torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.fastsoftrank_objective(z, z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.soft_ranks(z)
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(objective="MRR")):
        with pytest.raises(ValueError):
            F.fastsoftrank_objective(z, z, **kw)
    with pytest.raises(ValueError, match="4096"):
        F.fastsoftrank_objective(torch.zeros(1, 4097), torch.zeros(1, 4097))
    assert F.FASTSOFTRANK_MAX_LEN == 4096 and F.FASTSOFTRANK_OBJECTIVES == {"spearman": 0, "nDCG": 1}
    assert pa.PROJ_RANKER_NAMES == ("FastSoftRank",) and "FastSoftRank" not in pa.RANKER_NAMES and pa.FastSoftRank is pa.rankers.FastSoftRank
    cut = F.fastsoftrank_form(1)["cutover"]
    assert [F.fastsoftrank_form(L)["G"] for L in (1, cut, cut + 1, 4096)] == [64, 64, 256, 256]
    assert all(f["G"] * f["DPT"] >= L and f["lds_bytes"] == f["QPB"] * (28 * ((L + 3) // 4 * 4) + 160) <= 160 * 1024
               for L in (1, 65, cut, cut + 1, 1000, 4096) for f in [F.fastsoftrank_form(L)])
    text = " ".join(open(HEADER).read().split())
    for phrase in ("ptr_fastsoftrank_fwd_bwd", "projection onto the permutahedron", "merge only on a STRICT", "g(j) = max_{k > j} (S_k - S_j) / (k - j)",
                   "#define PTR_FSR_SPEARMAN 0", "#define PTR_FSR_NDCG 1"):
        assert phrase in text, phrase


def test_install_with_explicit_names_round_trips(monkeypatch):
    import ptranking_amd as pa
    from ptranking_amd.host import PointScorerRanker
    ltr, base_mod = types.ModuleType("fake_proj_ltr"), types.ModuleType("ptranking.base.adhoc_ranker")
    base_mod.AdhocNeuralRanker = PointScorerRanker
    monkeypatch.setitem(sys.modules, "fake_proj_ltr", ltr)
    for name in ("ptranking", "ptranking.base"):
        if name not in sys.modules:
            monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    monkeypatch.setitem(sys.modules, "ptranking.base.adhoc_ranker", base_mod)
    try:
        assert "FastSoftRank" not in pa.install(ltr_module="fake_proj_ltr") and not hasattr(ltr, "FastSoftRank")
    finally:
        pa.uninstall("fake_proj_ltr")
    try:
        done = pa.install(names=pa.RANKER_NAMES + pa.PROJ_RANKER_NAMES, ltr_module="fake_proj_ltr")
        assert ltr.FastSoftRank is done["FastSoftRank"] and issubclass(ltr.FastSoftRank, PointScorerRanker)
    finally:
        pa.uninstall("fake_proj_ltr")
    assert not hasattr(ltr, "FastSoftRank")
