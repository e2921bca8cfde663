"""CPU: the diversification frame without a GPU — the float64 restatement against the reference's own float64 results, the ABI v8 entry points
(declared, exported, bound, argument errors before any launch), the DALETOR class surface, install_diversification() and DivQueryBatches."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import diversity_ref as DR
import golden_util as GU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
REF = os.environ.get("PTRANKING_REF") or "/root/reference"
ENTRY_POINTS = ("ptr_alphadcg_fwd_bwd", "ptr_div_metrics_at_ks")


def golden():
    return GU._load("diversity.npz")


def header_src():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import build, _lib
    build.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("case", sorted(golden()["daletor"]))
def test_ref_reproduces_the_reference_loss_in_float64(case):
    c = golden()["daletor"][case]
    loss, grad = DR.alphadcg(c["preds"][0], c["rele"].astype(np.float64), rt=float(c["rt"]), alpha=0.5, top_k=int(c["top_k"]) or None,
                             top_k_axis=0)
    assert abs(loss - float(c["loss64"])) <= 1e-12 * max(1.0, abs(float(c["loss64"])))
    scale = max(1.0, float(np.max(np.abs(c["grad64"]))))
    assert np.max(np.abs(grad - c["grad64"][0])) <= 1e-12 * scale
    assert abs(DR.need(c["grad32"], c["grad64"]) - float(c["need32"])) <= 1e-9


def test_golden_loss_cases_cover_the_issue_list():
    d = golden()["daletor"]
    shape = {k: (c["rele"].shape[0], c["rele"].shape[1], int(c["top_k"])) for k, c in d.items()}
    assert any(T == 1 for T, L, k in shape.values())
    assert any(k and L < k for T, L, k in shape.values())
    assert any(k and T < k for T, L, k in shape.values()) and any(k and T > k for T, L, k in shape.values())
    assert any(L == 1000 for T, L, k in shape.values())
    assert any(len(np.unique(c["preds"])) < c["preds"].size for c in d.values())                # tied scores
    assert any(not c["rele"].any() for c in d.values())                                         # all-zero R
    assert any(c["rele"].any() and not c["rele"].any(axis=1).all() for c in d.values())         # a subtopic without a relevant document
    steep = [k for k in d if k.startswith("steep_")]
    assert len(steep) >= 2 and all(float(d[k]["rt"]) == 100.0 for k in steep)
    assert all(float(c["need32"]) <= 0.5 for k, c in d.items() if k not in steep)
    assert any(float(d[k]["need32"]) > 1.0 for k in steep)


@pytest.mark.parametrize("case", sorted(golden()["metrics"]))
def test_ref_reproduces_the_reference_metrics(case):
    c = golden()["metrics"][case]
    ks = [int(k) for k in c["ks"]]
    a, e, ne, valid = DR.div_metrics(c["preds"], c["rele"].astype(np.float64), ks, alpha=0.5, max_label=float(c["max_label"]))
    assert valid == int(c["valid"])
    for got, want in ((a, c["andcg"]), (e, c["err_ia"]), (ne, c["nerr_ia"])):
        assert np.max(np.abs(got - want)) <= 1e-6 * max(1.0, float(np.max(np.abs(want))))
    a1, e1, n1, _ = DR.div_metrics(c["preds"], c["rele"].astype(np.float64), [int(c["k1"])], alpha=0.5, max_label=float(c["max_label"]))
    for got, want in ((a1, c["andcg_k1"]), (e1, c["err_ia_k1"]), (n1, c["nerr_ia_k1"])):
        assert abs(got[0] - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    assert DR.div_metrics(c["preds"], c["rele"].astype(np.float64), ks, alpha=0.5, max_label=None)[1:3] == (None, None)


def test_ref_padding_and_axis_semantics():
    rng = np.random.default_rng(3)
    B, T, L = 3, 6, 20
    preds, rele = rng.standard_normal((B, L)), (rng.random((B, T, L)) < 0.3).astype(np.float64)
    lens, nts = np.array([20, 7, 13]), np.array([6, 2, 4])
    lq, g = DR.alphadcg_batch(preds, rele, top_k=5, top_k_axis=1, lens=lens, ntopics=nts)
    junk_p, junk_r = preds.copy(), rele.copy()
    for q in range(B):
        junk_p[q, lens[q]:] = np.nan
        junk_r[q, nts[q]:, :] = np.nan
        junk_r[q, :, lens[q]:] = np.nan
    lq2, g2 = DR.alphadcg_batch(junk_p, junk_r, top_k=5, top_k_axis=1, lens=lens, ntopics=nts)
    assert np.array_equal(lq, lq2) and np.array_equal(g, g2) and not g[1, 7:].any()
    # the document cut-off differs from the reference's subtopic cut-off by O(1), and equals it without a cut-off
    l0, _ = DR.alphadcg(preds[0], rele[0], top_k=3, top_k_axis=0)
    l1, _ = DR.alphadcg(preds[0], rele[0], top_k=3, top_k_axis=1)
    assert abs(l0 - l1) > 1e-3
    assert DR.alphadcg(preds[0], rele[0], top_k=None, top_k_axis=0)[0] == DR.alphadcg(preds[0], rele[0], top_k=None, top_k_axis=1)[0]
    # numerical gradient of the restatement
    eps = 1e-6
    _, ga = DR.alphadcg(preds[0], rele[0], top_k=4, top_k_axis=1)
    for j in (0, 5, 19):
        p = preds[0].copy(); p[j] += eps
        m = preds[0].copy(); m[j] -= eps
        num = (DR.alphadcg(p, rele[0], top_k=4, top_k_axis=1)[0] - DR.alphadcg(m, rele[0], top_k=4, top_k_axis=1)[0]) / (2 * eps)
        assert abs(num - ga[j]) <= 1e-6 * max(1.0, abs(ga[j]))


# ---------------------------------------------------------------------------------------------------------------- 2. ABI v8
def test_abi_v8_declares_exports_and_binds_both_entry_points(lib):
    from ptranking_amd import _lib
    src = header_src()
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == _lib.ABI_VERSION == lib.ptr_abi_version()
    assert _lib.MAX_SUBTOPICS == int(re.search(r"#define PTR_MAX_SUBTOPICS (\d+)", src).group(1))
    for name in ENTRY_POINTS:
        proto = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert hasattr(lib, name) and proto.count(",") + 1 == len(_lib.SIGNATURES[name]), name
    assert "diversity.hip" in __import__("ptranking_amd.build", fromlist=["SOURCES"]).SOURCES


# ---------------------------------------------------------------------------------------------------------------- 3. argument errors
def test_argument_errors_need_no_gpu(lib):
    one, f = ctypes.c_void_p(16), ctypes.c_float
    INVALID, UNSUPPORTED = 1001, 1002

    def loss(preds=one, rele=one, B=1, T=4, L=8, rt=10.0, alpha=0.5, top_k=10, axis=0):
        return lib.ptr_alphadcg_fwd_bwd(preds, rele, None, None, B, T, L, f(rt), f(alpha), top_k, axis, None, one, one, None)

    ks = (ctypes.c_int32 * 40)(*range(1, 41))

    def met(preds=one, rele=one, B=1, T=4, L=8, nk=3, alpha=0.5, max_label=1.0, err=one):
        return lib.ptr_div_metrics_at_ks(preds, rele, None, None, B, T, L, ks, nk, f(alpha), f(max_label), one, err, err, one, None)

    assert loss(preds=None) == INVALID and b"NULL" in lib.ptr_last_error()
    assert met(preds=None) == INVALID and b"NULL" in lib.ptr_last_error()
    for a in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert loss(alpha=a) == INVALID and b"alpha" in lib.ptr_last_error()
        assert met(alpha=a) == INVALID and b"alpha" in lib.ptr_last_error()
    for rt in (0.0, -1.0, float("nan")):
        assert loss(rt=rt) == INVALID and b"rt" in lib.ptr_last_error()
    assert loss(T=33) == UNSUPPORTED and b"PTR_MAX_SUBTOPICS" in lib.ptr_last_error()
    assert met(T=33) == UNSUPPORTED and b"PTR_MAX_SUBTOPICS" in lib.ptr_last_error()
    assert loss(T=0) == INVALID
    assert loss(L=4097) == UNSUPPORTED and b"PTR_MAX_LIST_LEN" in lib.ptr_last_error()
    assert met(L=4097) == UNSUPPORTED and b"PTR_MAX_LIST_LEN" in lib.ptr_last_error()
    assert met(nk=40) == UNSUPPORTED and b"PTR_MAX_CUTOFFS" in lib.ptr_last_error()
    for axis in (-1, 2):
        assert loss(axis=axis) == INVALID and b"top_k_axis" in lib.ptr_last_error()
    assert met(max_label=-1.0) == INVALID and b"max_label" in lib.ptr_last_error()
    assert met(max_label=-1.0, err=None, B=0) == 0                                    # alpha-nDCG alone needs no maximum label
    # a query tile beyond the LDS of a compute unit is refused with the documented limit: T <= 32 serves L <= 620, T <= 8 L <= 2272
    assert loss(T=32, L=621) == UNSUPPORTED and b"LDS" in lib.ptr_last_error()
    assert loss(T=8, L=2273) == UNSUPPORTED and loss(T=16, L=1205) == UNSUPPORTED
    assert loss(T=4, L=4093) == UNSUPPORTED
    for T, L in ((32, 620), (16, 1204), (8, 2272), (4, 4092)):
        assert loss(B=0, T=T, L=L) == 0
    assert loss(preds=None, rele=None, B=0) == 0 and met(preds=None, rele=None, B=0) == 0


def test_cpu_tensors_are_refused():
    import ptranking_amd.functional as F_
    p, r = torch.zeros(2, 8), torch.zeros(2, 3, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.alphadcg_loss(p, r)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.div_metrics_at_ks(p, r, [1, 5])
    with pytest.raises(ValueError, match="top_k_axis"):
        F_.alphadcg_loss(p, r, top_k_axis="rows")


# ---------------------------------------------------------------------------------------------------------------- 4. the ranker class
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=6, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False, dropout=0.0)}
METHODS = ("__init__", "div_forward", "div_predict", "div_train_op", "div_custom_loss_function", "div_train", "div_validation", "alpha_ndcg_at_k",
           "alpha_ndcg_at_ks", "err_ia_at_k", "nerr_ia_at_k", "srd_performance_at_ks")


def test_daletor_surface_and_scope():
    import ptranking_amd as pa
    assert pa.DIV_RANKER_NAMES == ("DALETOR",)
    assert pa.RANKER_NAMES == ("RankNet", "LambdaRank", "LambdaLoss", "ApproxNDCG", "ListNet", "ListMLE", "STListNet", "RankCosine", "RankMSE",
                               "SoftRank", "WassRank")
    assert "DALETOR" not in pa.RANKER_NAMES + pa.EXTRA_RANKER_NAMES
    for m in METHODS:
        assert callable(getattr(pa.DALETOR, m)), m
    sf = {**SF, "pointsf": dict(SF["pointsf"])}
    r = pa.DALETOR(sf_para_dict=sf, model_para_dict={"rt": 10.0, "top_k": 10}, gpu=False, device="cpu")
    assert (r.rt, r.top_k, r.id) == (10.0, 10, "DALETOR")
    assert r.sf_para_dict["pointsf"]["num_features"] == 18 and sf["pointsf"]["num_features"] == 6       # [q | q * doc | doc]; the caller's dict is left alone
    r.init()
    assert r.div_forward(torch.randn(1, 6), torch.randn(5, 6)).shape == (1, 5)
    with pytest.raises(AssertionError):
        r.div_custom_loss_function(torch.zeros(1, 5), torch.zeros(2, 5))                                  # presort is required (daletor.py:59)
    with pytest.raises(NotImplementedError, match="out of scope"):
        pa.DALETOR(sf_para_dict={"sf_id": "listsf", "opt": "Adam", "lr": 1e-3, "listsf": {}}, model_para_dict={"rt": 10.0, "top_k": 10})
    with pytest.raises(NotImplementedError):
        r.div_validation(vali_metric="nDCG")
    with pytest.raises(NotImplementedError, match="generate_div_run"):
        r.srd_performance_at_ks(test_data=[], max_label=1.0, generate_div_run=True)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "ptranking")), reason="the reference checkout is not on this machine")
def test_daletor_signatures_match_the_reference():
    import ptranking_amd as pa
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    try:
        from ptranking.ltr_diversification.score_and_sort.daletor import DALETOR as RefDALETOR
        for m in METHODS:
            assert inspect.signature(getattr(pa.DALETOR, m)) == inspect.signature(getattr(RefDALETOR, m)), m
    finally:
        sys.path.remove(REF)
        for m in [m for m in sys.modules if m == "ptranking" or m.startswith("ptranking.")]:
            del sys.modules[m]


@pytest.fixture
def stand_in_div_module(tmp_path, monkeypatch):
    """A minimal package with the module path install_diversification() binds into; its DALETOR is a placeholder."""
    root = tmp_path / "stand_in"
    files = {"ptranking/__init__.py": "", "ptranking/ltr_diversification/__init__.py": "", "ptranking/ltr_diversification/eval/__init__.py": "",
             "ptranking/ltr_diversification/eval/ltr_diversification.py": "class DALETOR:\n    pass\n\n\nclass DivProbRanker:\n    pass\n"}
    for rel, text in files.items():
        p = root / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(text)
    monkeypatch.setattr(sys, "dont_write_bytecode", True)
    monkeypatch.syspath_prepend(str(root))
    for m in [m for m in sys.modules if m == "ptranking" or m.startswith("ptranking.")]:
        monkeypatch.delitem(sys.modules, m)
    yield
    for m in [m for m in sys.modules if m == "ptranking" or m.startswith("ptranking.")]:
        del sys.modules[m]


def test_install_diversification_round_trip(stand_in_div_module):
    import ptranking_amd as pa
    import ptranking.ltr_diversification.eval.ltr_diversification as mod
    original, other = mod.DALETOR, mod.DivProbRanker
    installed = pa.install_diversification()
    try:
        assert set(installed) == {"DALETOR"} and mod.DALETOR is pa.DALETOR is installed["DALETOR"] and mod.DivProbRanker is other
        r = vars(mod)["DALETOR"](sf_para_dict={**SF, "pointsf": dict(SF["pointsf"])}, model_para_dict={"rt": 10.0, "top_k": 10}, gpu=False, device="cpu")
        assert type(r) is pa.DALETOR
        with pytest.raises(KeyError):
            pa.install_diversification(names=("DivProbRanker",))
    finally:
        pa.uninstall()
    assert mod.DALETOR is original and mod.DivProbRanker is other


# ---------------------------------------------------------------------------------------------------------------- 5. packing
def test_div_query_batches_packing():
    from ptranking_amd.diversity import DivQueryBatches
    q0, d0 = np.array([[1.0, 2.0]], np.float32), np.array([[1, 1], [2, 3], [4, 5]], np.float32)
    r0 = np.array([[1, 0, 0], [0, 2, 0]], np.float32)
    q1, d1 = np.array([0.5, -1.0], np.float32), np.arange(10, dtype=np.float32).reshape(5, 2)
    r1 = np.array([[1, 1, 0, 0, 0]], np.float32)
    q2, d2 = np.array([[3.0, 0.0]], np.float32), np.array([[1, 2]], np.float32)
    r2 = np.array([[0], [1], [0]], np.float32)
    data = [("a", torch.from_numpy(q0), ["x", "y", "z"], torch.from_numpy(d0), 1.0, {}, torch.from_numpy(r0)),      # the reference's 7-tuple
            (q1, d1, r1), (q2, d2, r2)]                                                                              # plain 3-tuples
    b = DivQueryBatches(data, "cpu", pad_to=4)
    assert (b.num_queries, b.num_features, b.presort, len(b)) == (3, 2, True, 2)
    (ids4, X4, R4, l4, t4), (ids8, X8, R8, l8, t8) = list(b)
    assert ids4 == ["a", 2] and ids8 == [1]
    assert X4.shape == (2, 4, 6) and R4.shape == (2, 3, 4) and X8.shape == (1, 8, 6) and R8.shape == (1, 1, 8)
    assert l4.dtype == t4.dtype == torch.int32 and l4.tolist() == [3, 1] and t4.tolist() == [2, 3] and l8.tolist() == [5] and t8.tolist() == [1]
    want0 = np.concatenate([np.repeat(q0, 3, axis=0), q0 * d0, d0], axis=1)                                          # [q | q * doc | doc]
    assert np.array_equal(X4[0, :3].numpy(), want0) and not X4[0, 3:].any()
    assert np.array_equal(X4[0, 1].numpy(), np.array([1, 2, 2, 6, 2, 3], np.float32))
    assert np.array_equal(R4[0].numpy(), np.array([[1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 0, 0]], np.float32))
    assert np.array_equal(R4[1].numpy(), np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]], np.float32))
    assert np.array_equal(X8[0, :5, 2:4].numpy(), q1[None, :] * d1) and not X8[0, 5:].any() and not R8[0, :, 5:].any()
    with pytest.raises(ValueError):
        DivQueryBatches([(q0, d0, r1)], "cpu")
