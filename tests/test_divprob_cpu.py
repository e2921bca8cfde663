"""CPU: DivProbRanker without a GPU — the float64 restatement (tests/divprob_ref.py) against the reference's own float64 results, the admission
condition of the parity families, the two additive ABI v8 entry points (declared, exported, bound, argument errors before any launch), the class
surface, the refused configurations, install_diversification(extras=True) and the mean / variance heads."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import divprob_ref as DR
import golden_util as GU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
REF = os.environ.get("PTRANKING_REF") or "/root/reference"
ENTRY_POINTS = ("ptr_divprob_fwd_bwd", "ptr_divprob_expected_ranks")
NAMES = {0: "aNDCG", 1: "nERR-IA", 2: "PairCLS", 3: "LambdaPairCLS"}


def golden():
    return GU._load("divprob.npz")


def rows(fams, objectives=(0, 1, 2, 3)):
    """(family, shape, row) of every stored reference run of the given families and objectives"""
    g = golden()
    return [(f, s, r) for f in fams for s in sorted(g[f]) for r, (o, _, _) in enumerate(g[f][s]["combos"]) if int(o) in objectives]


def case(fam, shape, row):
    c = golden()[fam][shape]
    obj, top_k, norm = (int(x) for x in c["combos"][row])
    L = c["mus"].shape[0]
    kw = dict(top_k=top_k or None, norm=bool(norm), max_label=float(c["max_label"]) if fam == "a" else 1.0)
    split = lambda res: (float(res[row][0]), np.asarray(res[row][1:1 + L], np.float64), np.asarray(res[row][1 + L:], np.float64))
    return c, NAMES[obj], kw, split(c["res32"]), split(c["res64"])


def header_src():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import build, _lib
    build.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- 1. the restatement
def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.nanmax(np.abs(a - b), initial=0.0)) / max(1.0, float(np.nanmax(np.abs(b), initial=0.0)))


@pytest.mark.parametrize("fam,shape,row", rows("abc"))
def test_literal_reproduces_the_reference_in_float64(fam, shape, row):
    c, objective, kw, _, (l64, gm64, gv64) = case(fam, shape, row)
    loss, gm, gv = DR.loss_and_grads("literal", c["mus"], c["vars"], c["rele"], objective, **kw)
    assert rel([loss], [l64]) <= 1e-12
    assert rel(gm, gm64) <= 1e-9 and rel(gv, gv64) <= 1e-9


@pytest.mark.parametrize("fam,shape,row", rows("a", (0, 1)) + rows("b"))
def test_stable_equals_literal_where_the_reference_is_well_conditioned(fam, shape, row):
    c, objective, kw, _, _ = case(fam, shape, row)
    a = DR.loss_and_grads("stable", c["mus"], c["vars"], c["rele"], objective, **kw)
    b = DR.loss_and_grads("literal", c["mus"], c["vars"], c["rele"], objective, **kw)
    for x, y in zip(a, b):
        assert rel(np.atleast_1d(x), np.atleast_1d(y)) <= 1e-9


@pytest.mark.parametrize("shape", sorted(golden()["a"]))
def test_expected_ranks_restatement(shape):
    c = golden()["a"][shape]
    assert rel(DR.expected_ranks(c["mus"], c["vars"]), c["ranks64"]) <= 1e-12


def test_golden_cases_cover_the_issue_list():
    g = golden()
    shapes = {s: c["rele"].shape for s, c in g["a"].items()}
    assert {L for _, L in shapes.values()} >= {1, 2, 7, 40, 130} and {T for T, _ in shapes.values()} >= {1, 3, 8, 20}
    assert any(c["rele"].max() > 1 for c in g["a"].values()) and any(c["rele"].max() == 1 for c in g["a"].values())
    assert any(not c["rele"].any() for c in g["a"].values())                                       # a query without a relevant document
    assert any(c["rele"].any() and not c["rele"].any(axis=1).all() for c in g["a"].values())       # a subtopic without a document
    for c in g["a"].values():
        combos = {tuple(int(x) for x in r) for r in c["combos"]}
        L = c["mus"].shape[0]
        assert {(0, k, 0) for k in (0, 3, 10)} | {(2, 0, 0), (3, 0, 0), (3, 0, 1)} <= combos
        assert {(1, k, 0) for k in (0, 3, 10) if not k > L > 1} <= combos                           # the reference's top_k > L does not run
    assert len(g["b"]) >= 3 and all(float(c["max_abs_x"]) <= 3.0 for c in g["b"].values())
    assert len(g["c"]) == 3 and all(float(c["max_abs_x"]) > 3.8 for c in g["c"].values())
    assert all({int(r[0]) for r in c["combos"]} == {2, 3} for f in "bc" for c in g[f].values())


# ---------------------------------------------------------------------------------------------------------------- 2. which family may be a target
@pytest.mark.parametrize("fam,shape,row", rows("b"))
def test_well_conditioned_family_admits_the_reference_as_target(fam, shape, row):
    """The reference's own fp32 is within the element-wise gate of its float64 on every case of family (b): a parity family may ask for that."""
    _, _, _, (l32, gm32, gv32), (l64, gm64, gv64) = case(fam, shape, row)
    needs = (DR.need([l32], [l64]), DR.need(gm32, gm64), DR.need(gv32, gv64))
    print(f"{shape}[{row}]: the reference's fp32 needs {needs} of the gate")
    assert max(needs) <= 1.0


@pytest.mark.parametrize("fam,shape,row", rows("c"))
def test_saturated_family_documents_the_departure(fam, shape, row):
    """On family (c) the reference's fp32 is NOT a faithful evaluation of its own float64 (1 - erfc(x) / 2 has rounded to 1), so the kernel is
    compared with the exact definition there, not with the reference."""
    _, _, _, (l32, gm32, gv32), (l64, gm64, gv64) = case(fam, shape, row)
    assert max(DR.need(gm32, gm64), DR.need(gv32, gv64)) > 1.0
    assert DR.need([l32], [l64]) > 1.0


@pytest.mark.parametrize("objective", DR.OBJECTIVES)
def test_central_differences_on_the_stable_form(objective):
    rng = np.random.default_rng(11)
    T, L = 5, 12
    mus, vars_ = rng.standard_normal(L), rng.uniform(0.05, 0.5, L)
    rele = (rng.random((T, L)) < 0.4).astype(np.float64) * rng.integers(1, 3, (T, L))
    kw = dict(top_k=4, top_k_axis=1, max_label=2.0, norm=True)
    _, gm, gv = DR.loss_and_grads("stable", mus, vars_, rele, objective, **kw)
    f = lambda m, v: DR.loss_and_grads("stable", m, v, rele, objective, **kw)[0]
    for j in (0, 3, 11):
        for which, grad, eps in (("mu", gm, 1e-6), ("var", gv, 1e-7)):
            p, m = (mus.copy(), vars_.copy()), (mus.copy(), vars_.copy())
            p[which == "var"][j] += eps
            m[which == "var"][j] -= eps
            num = (f(*p) - f(*m)) / (2 * eps)
            assert abs(num - grad[j]) <= 2e-6 * max(1.0, abs(grad[j])), (which, j, num, grad[j])


def test_padding_and_the_two_cut_off_axes():
    rng = np.random.default_rng(5)
    B, T, L = 3, 6, 20
    mus, vars_ = rng.standard_normal((B, L)), rng.uniform(0.1, 1.0, (B, L))
    rele = (rng.random((B, T, L)) < 0.3).astype(np.float64)
    lens, nts = np.array([20, 7, 13]), np.array([6, 2, 0])
    for objective in DR.OBJECTIVES:
        lq, gm, gv = DR.batch("stable", mus, vars_, rele, objective, lens=lens, ntopics=nts, top_k=5, top_k_axis=1)
        jm, jv, jr = mus.copy(), vars_.copy(), rele.copy()
        for q in range(B):
            jm[q, lens[q]:], jv[q, lens[q]:] = np.nan, np.nan
            jr[q, nts[q]:, :], jr[q, :, lens[q]:] = np.nan, np.nan
        lq2, gm2, gv2 = DR.batch("stable", jm, jv, jr, objective, lens=lens, ntopics=nts, top_k=5, top_k_axis=1)
        assert np.array_equal(lq, lq2) and np.array_equal(gm, gm2) and np.array_equal(gv, gv2)
        assert not gm[1, 7:].any() and not gv[1, 7:].any() and lq[2] == 0.0 and not gm[2].any()
    a0 = DR.loss_and_grads("stable", mus[0], vars_[0], rele[0], "aNDCG", top_k=3, top_k_axis=0)[0]
    a1 = DR.loss_and_grads("stable", mus[0], vars_[0], rele[0], "aNDCG", top_k=3, top_k_axis=1)[0]
    assert abs(a0 - a1) > 1e-3                         # the reference's slice of SUBTOPIC rows is not the document cut-off
    full = [DR.loss_and_grads("stable", mus[0], vars_[0], rele[0], "aNDCG", top_k=k, top_k_axis=0)[0] for k in (None, 6, 10)]
    assert full[0] == full[1] == full[2]               # T = 6 and top_k = 10: the same as no cut-off, bit for bit


# ---------------------------------------------------------------------------------------------------------------- 3. the ABI
def test_abi_stays_v8_and_declares_exports_and_binds_both_entry_points(lib):
    from ptranking_amd import _lib
    src = header_src()
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == _lib.ABI_VERSION == lib.ptr_abi_version()
    assert "ADDITIVE to ABI v8" in open(HEADER).read()
    for name in ENTRY_POINTS:
        proto = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert hasattr(lib, name) and proto.count(",") + 1 == len(_lib.SIGNATURES[name]), name
    for k, name in enumerate(("ANDCG", "ERRIA", "PAIRCLS", "LAMBDAPAIRCLS")):
        assert int(re.search(rf"#define PTR_DIVPROB_{name} (\d+)", src).group(1)) == k
    assert "divprob.hip" in __import__("ptranking_amd.build", fromlist=["SOURCES"]).SOURCES
    import ptranking_amd.functional as F_
    assert {F_.DIVPROB_OBJECTIVES[n] for n in DR.OBJECTIVES} == {0, 1, 2, 3}


def lds_limit(T, K):
    """the largest L with 4 * round_up(L, 4) * (3 + K * Tp) + 16 <= 160 KiB (include/ptranking_amd.h), capped at PTR_MAX_LIST_LEN"""
    Tp = 4 if T <= 4 else 8 if T <= 8 else 16 if T <= 16 else 32
    return min(4096, (160 * 1024 - 16) // (4 * (3 + K * Tp)) // 4 * 4)


TILES = {0: 2, 1: 1, 2: 1, 3: 3}
DOCUMENTED_LIMITS = {1: {4: 4096, 8: 3720, 16: 2152, 32: 1168}, 2: {4: 3720, 8: 2152, 16: 1168, 32: 608}, 3: {4: 2728, 8: 1516, 16: 800, 32: 412}}


def test_argument_errors_need_no_gpu(lib):
    one, f = ctypes.c_void_p(16), ctypes.c_float
    INVALID, UNSUPPORTED = 1001, 1002

    def loss(mus=one, vars_=one, rele=one, B=1, T=4, L=8, objective=0, beta=0.5, top_k=10, axis=0, max_label=1.0, norm=1, loss_q=one, gm=one,
             gv=one):
        return lib.ptr_divprob_fwd_bwd(mus, vars_, rele, None, None, B, T, L, objective, f(beta), top_k, axis, f(max_label), norm, None, loss_q,
                                       gm, gv, None)

    def ranks(mus=one, vars_=one, B=1, L=8, out=one):
        return lib.ptr_divprob_expected_ranks(mus, vars_, None, B, L, out, None)

    for kw in (dict(mus=None), dict(vars_=None), dict(rele=None), dict(loss_q=None), dict(gm=None), dict(gv=None)):
        assert loss(**kw) == INVALID and b"NULL" in lib.ptr_last_error(), kw
    for kw in (dict(mus=None), dict(vars_=None), dict(out=None)):
        assert ranks(**kw) == INVALID and b"NULL" in lib.ptr_last_error(), kw
    for objective in (-1, 4):
        assert loss(objective=objective) == INVALID and b"objective" in lib.ptr_last_error()
    for axis in (-1, 2):
        assert loss(axis=axis) == INVALID and b"top_k_axis" in lib.ptr_last_error()
    for beta in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert loss(beta=beta) == INVALID and b"beta" in lib.ptr_last_error()
    for ml in (-1.0, float("nan")):
        assert loss(objective=1, max_label=ml) == INVALID and b"max_label" in lib.ptr_last_error()
        assert loss(objective=0, max_label=ml, B=0) == 0                                    # only ERR-IA reads it
    assert loss(T=33) == UNSUPPORTED and b"PTR_MAX_SUBTOPICS" in lib.ptr_last_error()
    assert loss(T=0) == INVALID
    assert loss(L=4097) == UNSUPPORTED and b"PTR_MAX_LIST_LEN" in lib.ptr_last_error()
    assert ranks(L=4097) == UNSUPPORTED and b"PTR_MAX_LIST_LEN" in lib.ptr_last_error()
    assert loss(L=0) == INVALID and ranks(L=0) == INVALID
    # a query tile beyond the LDS of a compute unit is refused with the documented limit; the limit itself is served
    for objective, K in TILES.items():
        for T in (4, 8, 16, 32):
            lim = lds_limit(T, K)
            assert lim == DOCUMENTED_LIMITS[K][T]
            assert loss(B=0, T=T, L=lim, objective=objective) == 0
            if lim < 4096:
                assert loss(B=0, T=T, L=lim + 1, objective=objective) == UNSUPPORTED and b"LDS" in lib.ptr_last_error()
    assert loss(mus=None, vars_=None, rele=None, loss_q=None, gm=None, gv=None, B=0) == 0 and ranks(mus=None, vars_=None, out=None, B=0) == 0


def test_the_documented_limits_are_in_the_header():
    doc = open(HEADER).read()
    for K, name in ((1, "1 for ERRIA and PAIRCLS"), (2, "2 for ANDCG"), (3, "3 for LAMBDAPAIRCLS")):
        tail = doc.split(name, 1)[1]
        got = [int(x) for x in re.findall(r"L <= (\d+)", tail)[:4]]
        assert got == [DOCUMENTED_LIMITS[K][T] for T in (4, 8, 16, 32)], (K, got)


def test_cpu_tensors_are_refused():
    import ptranking_amd.functional as F_
    m, v, r = torch.zeros(2, 8), torch.ones(2, 8), torch.zeros(2, 3, 8)
    for objective in DR.OBJECTIVES:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            F_.divprob_loss(m, v, r, objective)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.expected_ranks(m, v)
    with pytest.raises(ValueError, match="objective"):
        F_.divprob_loss(m, v, r, "nDCG")
    with pytest.raises(ValueError, match="top_k_axis"):
        F_.divprob_loss(m, v, r, "aNDCG", top_k_axis="rows")


# ---------------------------------------------------------------------------------------------------------------- 4. the ranker class
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=6, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False, dropout=0.0)}
PARAS = dict(model_id="DivProbRanker", K=1, cluster=False, sort_id="ExpRele", top_k=None, opt_id="SuperSoft", limit_delta=0.01, metric="nERR-IA",
             opt_ideal=True, norm=True)
OWN_METHODS = ("__init__", "uniform_eval_setting", "div_forward", "div_predict", "div_train_op", "div_custom_loss_function")
EVAL_METHODS = ("div_train", "div_validation", "alpha_ndcg_at_k", "alpha_ndcg_at_ks", "err_ia_at_k", "nerr_ia_at_k", "srd_performance_at_ks")


def make(**over):
    import ptranking_amd as pa
    sf = {**SF, "pointsf": dict(SF["pointsf"])}
    return pa.DivProbRanker(sf_para_dict=sf, model_para_dict={**PARAS, **over}, gpu=False, device="cpu"), sf


def test_divprob_ranker_surface_and_scope():
    import ptranking_amd as pa
    assert pa.DIV_RANKER_NAMES == ("DALETOR",) and pa.EXTRA_DIV_RANKER_NAMES == ("DivProbRanker",)
    assert "DivProbRanker" not in pa.RANKER_NAMES + pa.EXTRA_RANKER_NAMES
    assert pa.diversity.DEFAULT_DIV_PARAS["DivProbRanker"] == PARAS                                   # div_prob_ranker.py:387-389
    for m in OWN_METHODS + EVAL_METHODS:
        assert callable(getattr(pa.DivProbRanker, m)), m
    for m in EVAL_METHODS:                                                                              # ONE set of loops for both rankers
        assert getattr(pa.DivProbRanker, m) is getattr(pa.DALETOR, m), m
    r, sf = make()
    assert (r.id, r.K, r.opt_id, r.metric, r.top_k, r.beta, r.b, r.norm) == ("DivProbRanker", 1, "SuperSoft", "nERR-IA", None, 0.5, 0.1, False)
    assert r.sf_para_dict["pointsf"]["num_features"] == 18 and r.sf_para_dict["pointsf"]["out_dim"] == 2
    assert sf["pointsf"]["num_features"] == 6 and "out_dim" not in sf["pointsf"]                        # the caller's dict is left alone
    assert make(K=5)[0].sf_para_dict["pointsf"]["out_dim"] == 15
    lam = make(opt_id="LambdaPairCLS", norm=True)[0]
    assert lam.norm is True and make(opt_id="PairCLS")[0].norm is False
    r.init()
    mus, vars_ = r.div_forward(torch.randn(1, 6), torch.randn(5, 6))
    assert mus.shape == vars_.shape == (1, 5) and bool((vars_ > 0).all()) and bool((vars_ < 0.01).all())
    assert r.div_predict(torch.randn(1, 6), torch.randn(5, 6)).shape == (1, 5)
    with pytest.raises(AssertionError):
        r.div_custom_loss_function(mus, vars_, torch.zeros(2, 5))                                       # presort is required (:305)
    eval_dict = dict(do_validation=True, vali_metric="aNDCG")
    r.uniform_eval_setting(eval_dict=eval_dict)
    assert eval_dict["vali_metric"] == "nERR-IA"
    eval_dict = dict(do_validation=True, vali_metric="aNDCG")
    lam.uniform_eval_setting(eval_dict=eval_dict)
    assert eval_dict["vali_metric"] == "aNDCG"


def test_every_refused_configuration():
    import ptranking_amd as pa
    for sf_id in ("listsf", "listsfco"):
        with pytest.raises(NotImplementedError, match="out of scope"):
            pa.DivProbRanker(sf_para_dict={"sf_id": sf_id, "opt": "Adam", "lr": 1e-3, sf_id: {}}, model_para_dict=dict(PARAS))
    for over in (dict(cluster=True, K=3), dict(opt_ideal=False), dict(opt_id="LambdaPairCLS", opt_ideal=False), dict(opt_id="Portfolio")):
        with pytest.raises(NotImplementedError, match="out of scope"):
            make(**over)
    with pytest.raises(AssertionError):
        make(sort_id="Random")
    with pytest.raises(AssertionError):
        make(opt_id="ListNet")
    with pytest.raises(AssertionError):
        make(metric="nDCG")
    r = make()[0]
    with pytest.raises(NotImplementedError, match="out of scope"):
        r.srd_performance_at_ks(test_data=[], max_label=1.0, generate_div_run=True)
    with pytest.raises(NotImplementedError, match="out of scope"):
        r.div_custom_loss_function(torch.zeros(1, 5), torch.ones(1, 5), torch.zeros(2, 5), presort=True, batch_cocos=torch.zeros(1, 5, 5))
    with pytest.raises(NotImplementedError):
        r.div_validation(vali_metric="nDCG")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "ptranking")), reason="the reference checkout is not on this machine")
def test_divprob_ranker_signatures_match_the_reference():
    import ptranking_amd as pa
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    try:
        from ptranking.ltr_diversification.score_and_sort.div_prob_ranker import DivProbRanker as RefRanker
        for m in OWN_METHODS + EVAL_METHODS:
            assert inspect.signature(getattr(pa.DivProbRanker, m)) == inspect.signature(getattr(RefRanker, m)), m
    finally:
        sys.path.remove(REF)
        for m in [m for m in sys.modules if m == "ptranking" or m.startswith("ptranking.")]:
            del sys.modules[m]


@pytest.mark.parametrize("K,limit_delta", [(1, None), (1, 0.1), (3, None), (3, 0.01)])
def test_heads_against_a_torch_restatement(K, limit_delta):
    r = make(K=K, limit_delta=limit_delta)[0]
    torch.manual_seed(3)
    comp = torch.randn(4, 9, 2 if K == 1 else 3 * K, dtype=torch.float64)
    mus, vars_ = r._head(comp)
    to_var = (lambda s: s.exp()) if limit_delta is None else (lambda s: limit_delta / (1.0 + (-s).exp()))
    if K == 1:
        want_m, want_v = comp[..., 0], to_var(comp[..., 1])
    else:
        w = comp[..., :K].exp() / comp[..., :K].exp().sum(dim=-1, keepdim=True)
        want_m, want_v = (w * comp[..., K:2 * K]).sum(-1), (w * to_var(comp[..., 2 * K:])).sum(-1)
    assert mus.shape == vars_.shape == (4, 9)
    assert torch.allclose(mus, want_m, rtol=1e-12, atol=1e-14) and torch.allclose(vars_, want_v, rtol=1e-12, atol=1e-14)
    r.sort_id = "RiskAware"
    assert torch.equal(r._sort_scores(mus, vars_), mus - 0.1 * vars_)
    r.sort_id = "ExpRele"
    assert r._sort_scores(mus, vars_) is mus


# ---------------------------------------------------------------------------------------------------------------- 5. install
@pytest.fixture
def stand_in_div_module(tmp_path, monkeypatch):
    """A minimal package with the module path install_diversification() binds into; its rankers are placeholders."""
    root = tmp_path / "stand_in"
    files = {"ptranking/__init__.py": "", "ptranking/ltr_diversification/__init__.py": "", "ptranking/ltr_diversification/eval/__init__.py": "",
             "ptranking/ltr_diversification/eval/ltr_diversification.py": "class DALETOR:\n    pass\n\n\nclass DivProbRanker:\n    pass\n"}
    for path, text in files.items():
        p = root / path
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(text)
    monkeypatch.setattr(sys, "dont_write_bytecode", True)
    monkeypatch.syspath_prepend(str(root))
    for m in [m for m in sys.modules if m == "ptranking" or m.startswith("ptranking.")]:
        monkeypatch.delitem(sys.modules, m)
    yield
    for m in [m for m in sys.modules if m == "ptranking" or m.startswith("ptranking.")]:
        del sys.modules[m]


def test_install_diversification_extras_round_trip(stand_in_div_module):
    import ptranking_amd as pa
    import ptranking.ltr_diversification.eval.ltr_diversification as mod
    daletor, divprob = mod.DALETOR, mod.DivProbRanker
    installed = pa.install_diversification(extras=True)
    try:
        assert set(installed) == {"DALETOR", "DivProbRanker"}
        assert mod.DALETOR is pa.DALETOR and mod.DivProbRanker is pa.DivProbRanker is installed["DivProbRanker"]
        r = vars(mod)["DivProbRanker"](sf_para_dict={**SF, "pointsf": dict(SF["pointsf"])}, model_para_dict=dict(PARAS), gpu=False, device="cpu")
        assert type(r) is pa.DivProbRanker
    finally:
        pa.uninstall()
    assert mod.DALETOR is daletor and mod.DivProbRanker is divprob
    only = pa.install_diversification(names=(), extras=True)
    try:
        assert set(only) == {"DivProbRanker"} and mod.DALETOR is daletor and mod.DivProbRanker is pa.DivProbRanker
    finally:
        pa.uninstall()
    assert mod.DivProbRanker is divprob


def test_default_install_is_unchanged(stand_in_div_module):
    import ptranking_amd as pa
    import ptranking.ltr_diversification.eval.ltr_diversification as mod
    daletor, divprob = mod.DALETOR, mod.DivProbRanker
    try:
        assert set(pa.install_diversification()) == {"DALETOR"} and mod.DivProbRanker is divprob
        with pytest.raises(KeyError):
            pa.install_diversification(names=("DivProbRanker",))
        with pytest.raises(KeyError):
            pa.install_diversification(names=("RankNet",), extras=True)
    finally:
        pa.uninstall()
    assert mod.DALETOR is daletor and mod.DivProbRanker is divprob
