"""CPU: the cross-entropy nDCG objective (rank_xendcg) without a GPU — the float64 restatement (tests/xendcg_ref.py) on answers worked by
hand and its invariants, the eager fp32 form under the gate on every input of the GPU tests, planted faults the gate must reject, the
counter stream of the uniforms, the parameter, the model file, the ABI and the Python surface."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import plsample_ref as PR
import tree_ref as TR
import xendcg_ref as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
ENTRY = "ptr_tree_xendcg_grad_hess"


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- 1. the restatement
def test_known_answers_by_hand_for_two_documents():
    """u = 0.  Equal scores, labels (1, 0): rho = 1/2, phi = (2, 1), a = (-1/6, 1/6), x = (-1/3, 1/3), A = 0, b = -a, z = -x, Bs = 0, c = a:
    grad = a, hess = 1/4.  Scores (ln 3, 0), equal labels: rho = (3/4, 1/4), a = (1/4, -1/4), q = (1/4, 3/4), x = (1, -1/3), A = 2/3,
    b = (-1/4, 1/4), z = (-1, 1/3), Bs = -2/3, c = (1/4, -1/4): grad = (1/4, -1/4), hess = 3/16."""
    grad, E, hess, Eh = XR.query([0.0, 0.0], [1.0, 0.0], [0.0, 0.0])
    assert np.allclose(grad, [-1 / 6, 1 / 6], rtol=1e-15) and np.allclose(hess, [0.25, 0.25], rtol=1e-15) and (E > 0).all() and (Eh > 0).all()
    grad, _, hess, _ = XR.query([math.log(3.0), 0.0], [0.0, 0.0], [0.0, 0.0])
    assert np.allclose(grad, [0.25, -0.25], rtol=1e-14) and np.allclose(hess, [3 / 16, 3 / 16], rtol=1e-14)
    eg, eh = XR.eager_query([0.0, 0.0], [1.0, 0.0], [0.0, 0.0])
    assert np.allclose(eg, [-1 / 6, 1 / 6], rtol=1e-6) and np.array_equal(eh, [0.25, 0.25])
    # a uniform moves phi: labels (1, 0) with u = (1/2, 0) give phi = (3/2, 1), a = (1/2 - 3/5, 1/2 - 2/5)
    assert np.allclose(XR.query([0.0, 0.0], [1.0, 0.0], [0.5, 0.0], detail=True)["a"], [-0.1, 0.1], rtol=1e-14)


def test_the_exact_cases_and_the_bad_inputs():
    assert all(v.shape == (0,) for v in XR.query([], [], []))
    assert all((v == 0).all() and v.shape == (1,) for v in XR.query([0.5], [3.0], [0.25]))
    assert all((v == 0).all() for v in XR.eager_query([0.5], [3.0], [0.25]))
    good = ([0.1, 0.2, 0.3], [1.0, 0.0, 2.0], [0.5, 0.25, 0.0])
    assert np.isfinite(XR.query(*good)[0]).all()
    for k, bad in ((0, np.nan), (1, np.nan), (1, -1.0), (2, 1.0), (2, -0.5), (2, np.nan)):
        args = [list(v) for v in good]
        args[k][1] = bad
        res = XR.query(*args)
        assert np.isnan(res[0]).all() and np.isnan(res[2]).all() and (res[1] == 0).all(), (k, bad)
        assert all(np.isnan(v).all() for v in XR.eager_query(*args))
    assert np.isnan(XR.query([np.nan], [1.0], [0.0])[0]).all()                  # a bad input wins over the one-document rule


def test_first_order_terms_sum_to_zero_and_dominant_lists_stay_finite():
    for name in ("straddle", "dominant"):
        s, y, u, group = XR.gpu_inputs()[name]
        off = TR.offsets_of(group)
        for a, b in zip(off[:-1], off[1:]):
            ref = XR.query(s[a:b], y[a:b], u[a:b], detail=True)
            assert abs(ref["a"].sum()) <= ref["E_a"].sum() + 1e-300                                  # rho and phi / P both sum to 1
            fp32 = XR.eager_query(s[a:b], y[a:b], u[a:b], parts=True)[2]
            assert abs(fp32.sum()) <= ref["E_a"].sum() + 1e-300                                      # and within the bound in fp32
            assert (ref["hess"] >= 0).all() and all(np.isfinite(ref[k]).all() for k in ("grad", "E_grad", "hess", "E_hess"))
    s, y, u, group = XR.gpu_inputs()["dominant"]
    grad, hess = XR.eager_batch(s, y, u, group)
    assert np.isfinite(grad).all() and np.isfinite(hess).all() and (hess >= 0).all()
    off = TR.offsets_of(group)
    rho = np.concatenate([np.exp(s[a:b].astype(np.float32) - s[a:b].max()) / np.exp(s[a:b].astype(np.float32) - s[a:b].max()).sum(dtype=np.float32)
                          for a, b in zip(off[:-1], off[1:])])
    assert (rho == 1.0).sum() == 4 and ((1.0 - rho > 0) & (1.0 - rho < 64 * XR.FLOOR)).any()         # the floor is hit, and approached


# ---------------------------------------------------------------------------------------------------------------- 2. the eager form
@pytest.mark.parametrize("name", list(XR.gpu_inputs()))
def test_eager_fp32_passes_the_gate_on_every_gpu_input(name):
    s, y, u, group = XR.gpu_inputs()[name]
    w = XR.gate(*XR.eager_batch(s, y, u, group), XR.reference(name), f"eager {name}")
    print(f"eager fp32 on {name}: worst err/E {w:.3f}: needs C_LIST >= {w * XR.C:.2f}")


@pytest.mark.parametrize("fault", XR.FAULTS)
def test_the_gate_rejects_a_planted_fault(fault):
    caught = []
    for name, (s, y, u, group) in XR.gpu_inputs().items():
        try:
            XR.gate(*XR.eager_batch(s, y, u, group, fault=fault), XR.reference(name), f"{fault} on {name}")
        except AssertionError as e:
            assert "bound failed" in str(e)
            caught.append(name)
    print(f"{fault}: rejected on {caught}")
    assert caught, fault
    if fault in ("hess_floored", "no_floor"):
        assert caught == ["dominant"]                          # the floor shows only where one document holds the softmax mass


# ---------------------------------------------------------------------------------------------------------------- 3. the stream
def test_the_stream_is_keyed_by_seed_draw_and_document():
    d = np.arange(4096)
    base = XR.uniforms(5, 3, d)
    assert np.array_equal(base, XR.uniforms(5, 3, d)) and base.dtype == np.float32
    assert np.array_equal(base[100:200], XR.uniforms(5, 3, d[100:200]))                    # a document's value, whatever is asked beside it
    for other in (XR.uniforms(6, 3, d), XR.uniforms(5, 4, d), XR.uniforms(5, 3, d + 1), XR.uniforms(5 + (1 << 32), 3, d),
                  XR.uniforms(5, 3 + (1 << 32), d), XR.uniforms(5, 3, d + (1 << 32))):
        assert (other != base).mean() > 0.99
    # it is plsample_ref's hash with the round as the query, hi32(d) as the sample and lo32(d) as the index
    assert np.array_equal(base, PR.uniforms_host(1, 4096, 1, 5, q0=3)[0, 0])
    assert np.array_equal(XR.uniforms(5, 3, d[:64] + (2 << 32)), PR.uniforms_host(1, 64, 3, 5, q0=3)[0, 2])
    assert np.array_equal(XR.uniforms(9, (1 << 32) + 1, d[:64]), PR.uniforms_host(1, 64, 1, 9, q0=(1 << 32) + 1)[0, 0])
    assert (base >= 0).all() and (base < 1).all() and np.array_equal(base * 2.0 ** 24, np.round(base * 2.0 ** 24))


def test_the_stream_is_uniform_to_four_standard_errors():
    n = 2 ** 16
    u = XR.uniforms(5, 0, np.arange(n)).astype(np.float64)
    assert abs(u.mean() - 0.5) <= 4.0 * math.sqrt(1.0 / 12.0 / n)
    assert abs((u < 0.5).mean() - 0.5) <= 4.0 * math.sqrt(0.25 / n)


# ---------------------------------------------------------------------------------------------------------------- 4. the ABI
def test_the_symbol_is_declared_exported_and_bound(lib):
    from ptranking_amd import _lib
    import ptranking_amd.functional as F_
    doc = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == _lib.ABI_VERSION == lib.ptr_abi_version()
    proto = re.search(ENTRY + r"\s*\(([^)]*)\)", src).group(1)
    assert hasattr(lib, ENTRY) and proto.count(",") + 1 == len(_lib.SIGNATURES[ENTRY]) == 13
    assert "const float *unif, uint64_t seed, int64_t draw" in proto
    flat = re.sub(r"\s*\n \*\s*", " ", doc)                               # the comment block as running text
    for phrase in ("modelled on LightGBM's RankXENDCG", "compared with nothing of LightGBM's", "no parity with it is claimed", "2^-20",
                   "phi_i = 2^{y_i} - u_i", "UNFLOORED", "pl_sample_keys(pl_query_keys(seed, draw), hi32(d))"):
        assert phrase in flat, phrase
    assert "tree_xendcg_grad_hess" in F_.__all__ and callable(F_.tree_xendcg_grad_hess)
    for name, what in (("COVERAGE.md", "f-22"), ("COVERAGE.md", "rank_xendcg"), ("DESIGN.md", "rank_xendcg")):
        assert what in open(os.path.join(ROOT, name)).read(), (name, what)


def test_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    INVALID, UNSUPPORTED = 1001, 1002

    def call(preds=one, labels=one, offsets=one, B=2, queries=None, nq=2, max_len=8, unif=None, seed=5, draw=0, grad=one, hess=one):
        return getattr(lib, ENTRY)(preds, labels, offsets, B, queries, nq, max_len, unif, seed, draw, grad, hess, None)

    for kw in (dict(preds=None), dict(labels=None), dict(offsets=None), dict(grad=None), dict(hess=None)):
        assert call(**kw) == INVALID and b"NULL" in lib.ptr_last_error(), kw
    for kw in (dict(B=-1, nq=-1), dict(nq=-1, queries=one), dict(max_len=-1)):
        assert call(**kw) == INVALID and b"negative" in lib.ptr_last_error(), kw
    assert call(nq=1) == INVALID and b"nq must equal B" in lib.ptr_last_error()
    for draw in (-1, -2 ** 40):
        assert call(draw=draw) == INVALID and b"draw" in lib.ptr_last_error()
    assert call(max_len=4097) == UNSUPPORTED and b"PTR_MAX_LIST_LEN" in lib.ptr_last_error()
    assert call(max_len=4097, draw=-1) == INVALID                               # an argument error wins over the unsupported length
    assert call(max_len=4096, B=0, nq=0) == 0
    assert call(preds=None, labels=None, offsets=None, grad=None, hess=None, B=0, nq=0) == 0
    assert call(preds=None, labels=None, offsets=None, grad=None, hess=None, B=3, queries=one, nq=0) == 0


def test_the_library_tells_which_form_serves_a_length(lib):
    def form(max_len):
        a, o = (ctypes.c_int64 * 1)(max_len), (ctypes.c_int32 * 4)(-1, -1, -1, -1)
        assert lib.ptr_launch_form(ENTRY.encode(), a, 1, o, 4) == 0
        return list(o)
    # threads per query, queries per workgroup, documents per thread (the fourth value is left alone)
    assert form(16) == [16, 16, 1, -1] and form(17) == [64, 4, 1, -1] and form(128) == [64, 4, 2, -1]
    assert form(129) == [256, 1, 1, -1] and form(4096) == [256, 1, 16, -1]
    assert [form(n)[2] for n in (64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049)] == [1, 2, 1, 2, 2, 4, 4, 8, 8, 16]
    assert all(f[0] * f[2] >= n for n, f in ((n, form(n)) for n in (1, 16, 17, 128, 129, 1251, 4096)))
    a, o = (ctypes.c_int64 * 2)(16, 0), (ctypes.c_int32 * 4)()
    assert lib.ptr_launch_form(ENTRY.encode(), a, 2, o, 4) == 1001


# ---------------------------------------------------------------------------------------------------------------- 5. the Python surface
def test_the_objective_is_listed_last_and_the_seed_is_a_parameter():
    from ptranking_amd import gbdt
    import ptranking_amd as pa
    assert list(pa.tree.OBJECTIVES) == ["ranknet", "lambdarank", "listnet", "lambdarank_ndcg", "rank_xendcg"]
    assert pa.tree.OBJECTIVES["rank_xendcg"] == ("xendcg", None) and pa.tree.OBJECTIVES["lambdarank_ndcg"][0] == "lambdarank_ndcg"
    assert gbdt.DEFAULT_PARAMS["objective_seed"] == 5 and type(gbdt.DEFAULT_PARAMS["objective_seed"]) is int
    assert "objective_seed" not in gbdt.IGNORED_PARAMS and gbdt.GBDT({"objective_seed": 5}).params == gbdt.GBDT().params
    p = gbdt._params({"objective_seed": np.int64(11), "objective": "rank_xendcg"})
    assert p["objective_seed"] == 11 and type(p["objective_seed"]) is int and "objective" not in p
    assert gbdt._params({"objective_seed": 2 ** 64 - 1})["objective_seed"] == 2 ** 64 - 1
    assert len(pa.tree.DROP_IN_NAMES) == 6 and not any("xendcg" in n for n in pa.tree.DROP_IN_NAMES)
    import inspect
    assert inspect.signature(gbdt.LambdaMART.__init__).parameters["objective"].default == "lambdarank"
    assert inspect.signature(gbdt.LambdaMART.grad_hess).parameters["draw"].default == 0


BAD_SEEDS = [-1, 2.5, float("nan"), float("inf"), -float("inf"), True, "5", None, 2 ** 64]


@pytest.mark.parametrize("bad", BAD_SEEDS, ids=repr)
def test_a_bad_objective_seed_raises_before_any_gpu_is_asked_for(bad, monkeypatch):
    from ptranking_amd import gbdt
    import ptranking_amd as pa
    import ptranking_amd.functional as F_
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for build in (lambda: gbdt._params({"objective_seed": bad}), lambda: gbdt.GBDT({"objective_seed": bad}),
                  lambda: gbdt.LambdaMART({"objective_seed": bad}, objective="rank_xendcg"), lambda: gbdt.LambdaMART({"objective_seed": bad}),
                  lambda: pa.TreeObjective(objective="rank_xendcg", objective_seed=bad),
                  lambda: F_.tree_xendcg_grad_hess(torch.zeros(3), torch.zeros(3), torch.tensor([0, 3]), seed=bad)):
        with pytest.raises(ValueError, match="objective_seed"):
            build()
    for draw in (-1, 1.5, True, None, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="draw"):
            F_.tree_xendcg_grad_hess(torch.zeros(3), torch.zeros(3), torch.tensor([0, 3]), draw=draw)


def test_settings_of_the_other_objectives_do_not_apply(monkeypatch):
    from ptranking_amd import gbdt
    import ptranking_amd as pa
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for kw in (dict(weighting=None), dict(weighting="DeltaGain"), dict(hessian="reference"), dict(hessian="constant"), dict(pair_type="NoTies"),
               dict(epsilon=2.0), dict(gain_type="Label")):
        with pytest.raises(ValueError, match=f"{next(iter(kw))}=.*does not apply"):
            gbdt.LambdaMART(objective="rank_xendcg", **kw)
    for kw in (dict(weighting="DeltaNDCG"), dict(hessian="sum"), dict(pair_type="All"), dict(epsilon=0.5), dict(gain_type="Label")):
        with pytest.raises(ValueError, match=f"{next(iter(kw))}=.*does not apply"):
            pa.TreeObjective(objective="rank_xendcg", **kw)
    lazy = pa.TreeObjective(objective="rank_xendcg", objective_seed=9, truncation_level=7, sigmoid=2, norm=False)   # lambdarank's three: ignored
    assert (lazy.kind, lazy.objective_seed, lazy.draw, lazy.uploads) == ("xendcg", 9, 0, 0)
    assert pa.TreeObjective(objective="rank_xendcg").objective_seed == 5
    assert pa.TreeObjective(objective="lambdarank").draw == 0


def test_without_a_gpu_the_new_paths_raise_loudly(monkeypatch):
    from ptranking_amd import gbdt
    import ptranking_amd as pa
    import ptranking_amd.functional as F_
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    labels, group = np.array([1.0, 0.0, 2.0]), np.array([3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gbdt.LambdaMART({"objective_seed": 7}, objective="rank_xendcg")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pa.TreeObjective(labels, group, "rank_xendcg")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pa.TreeObjective(objective="rank_xendcg").sklearn(labels, np.zeros(3), group)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.tree_xendcg_grad_hess(torch.zeros(3), torch.zeros(3), torch.tensor([0, 3]))


def test_the_seed_travels_in_the_model_file_and_an_older_file_loads(tmp_path):
    from ptranking_amd import gbdt
    m = gbdt.GBDT({"objective_seed": 12, "num_leaves": 4, "max_bin": 16})
    m.edges, m.nbins = np.full((2, 15), np.inf, np.float32), np.ones(2, np.int32)
    m.trees = [{"feature": np.array([0], np.int32), "threshold": np.array([0.5], np.float32), "left": np.array([~0], np.int32),
                "right": np.array([~1], np.int32), "value": np.array([-1.0, 1.0], np.float32)}]
    m.save_model(tmp_path / "m.npz")
    back = gbdt.GBDT.load_model(tmp_path / "m.npz")
    assert back.params == m.params and back.params["objective_seed"] == 12
    with np.load(tmp_path / "m.npz", allow_pickle=False) as z:
        store = {k: z[k] for k in z.files}
    assert int(store["format"]) == 1
    old = json.loads(str(store["params"]))
    del old["objective_seed"]                                              # the file as it was written before the key existed
    store["params"] = np.array(json.dumps(old))
    with open(tmp_path / "old.npz", "wb") as fh:
        np.savez(fh, **store)
    parent = gbdt.GBDT.load_model(tmp_path / "old.npz")
    assert parent.params["objective_seed"] == 5 and len(parent.trees) == 1
