"""CPU: ndeval's measures and greedy ideal ranking without a GPU — the float64 restatement (tests/ndeval_ref.py) against what the reference's
own ndeval printed (tests/golden/ndeval.npz, every field of every topic, string for string), the greedy against a brute-force rescan, the
additive ABI symbol (declared, exported, bound, argument errors before any launch) and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import golden_util as GU
import ndeval_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
INVALID, UNSUPPORTED = 1001, 1002


def golden():
    if "ndeval" not in GU._CACHE:
        GU._CACHE["ndeval"] = GU._load("ndeval.npz")
    return GU._CACHE["ndeval"]


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import build, _lib
    build.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("run", sorted(golden()["runs"]))
def test_restatement_reproduces_every_field_ndeval_printed(run):
    g = golden()
    r = g["runs"][run]
    assert tuple(str(x) for x in r["names"]) == NR.FIELD_NAMES
    bad, total = [], 0
    for tid, row in zip(r["topics"], r["field_str"]):
        t = g["topics"][f"t{int(tid):03d}"]
        mine = NR.fields(NR.topic(t["preds"], t["rele"], float(r["alpha"]), float(r["beta"]), int(r["depth_m"]), int(t["lens"]), int(t["ntopics"])))
        for name, a, b in zip(NR.FIELD_NAMES, mine, row):
            total += 1
            if not NR.same_field(a, str(b)):
                bad.append((int(tid), name, a, str(b)))
    assert total == 21 * len(r["topics"]) and not bad, f"{len(bad)} of {total} fields differ: {bad[:5]}"


def test_fixture_holds_the_families_the_issue_lists():
    g = golden()
    T = {k: t["rele"].shape[0] for k, t in g["topics"].items()}
    n = {k: t["rele"].shape[1] for k, t in g["topics"].items()}
    a = [f"t{int(i):03d}" for i in g["runs"]["a"]["topics"]]
    assert len(a) >= 38 and {1, 4, 5, 9, 10, 19, 20, 21} <= {n[k] for k in a} and max(n[k] for k in a) <= 300
    assert min(T[k] for k in a) == 1 and max(T[k] for k in a) == 20
    assert any(g["topics"][k]["rele"].max() == 3 for k in a)                                              # graded judgments
    assert any(len(np.unique(g["topics"][k]["preds"])) < n[k] for k in a)                                 # tied scores
    assert any(not g["topics"][k]["rele"].any() for k in a)                                               # an all-zero topic
    assert any(g["topics"][k]["noline"].any() for k in a)                                                 # a gap in the subtopic indices
    assert any(g["topics"][k]["rele"].any() and not g["topics"][k]["rele"].any(axis=1).all() and not g["topics"][k]["noline"].any() for k in a)
    assert any(g["topics"][k]["rele"].any() and not g["topics"][k]["rele"].any(axis=0).all() for k in a)  # unjudged documents in the run
    dens = sorted(float((g["topics"][k]["rele"] > 0).mean()) for k in a if n[k] * T[k] >= 400)
    assert dens[0] < 0.1 and dens[-1] > 0.4
    flags = {(float(r["alpha"]), float(r["beta"]), int(r["depth_m"])) for r in g["runs"].values()}
    assert {(0.5, 0.5, 0), (0.3, 0.8, 0), (0.9, 0.5, 0), (0.5, 0.5, 10), (0.5, 0.5, 100)} <= flags
    d = [f"t{int(i):03d}" for i in g["runs"]["d_long"]["topics"]]
    assert {n[k] for k in d} == {1024, 1025, 4096} and {T[k] for k in d} == {32}
    assert os.path.getsize(os.path.join(GU.GOLDEN_DIR, "ndeval.npz")) < 512 * 1024
    # nNRBP of the all-zero topics is what ndeval prints for 0 / 0
    r = g["runs"]["a"]
    zero = [i for i, tid in enumerate(r["topics"]) if not g["topics"][f"t{int(tid):03d}"]["rele"].any()]
    assert zero and all("nan" in str(r["field_str"][i][13]) for i in zero) and np.isnan(r["amean_f64"][13])


# ---------------------------------------------------------------------------------------------------------------- 2. the greedy
@pytest.mark.parametrize("alpha", [0.5, 0.3, 0.9])
def test_greedy_order_against_a_brute_force_rescan(alpha):
    rng = np.random.default_rng(int(alpha * 100))
    for trial in range(60):
        T, n = int(rng.integers(1, 9)), int(rng.integers(1, 25))
        rel = (rng.random((n, T)) < rng.choice([0.1, 0.3, 0.7])).astype(np.uint8)
        if trial % 7 == 0:
            rel[rng.integers(0, n, n // 2 + 1)] = rel[0]                  # duplicate columns: exact ties
        order = NR.ideal_order(rel, alpha)
        brute, rounds = NR.ideal_order_bruteforce(rel.tolist(), alpha)
        assert order == brute and sorted(order) == list(range(n))
        for pick, seen in zip(order, rounds):                             # each round: the maximal score, the last index among the ties
            best = max(seen.values())
            assert seen[pick] == best and pick == max(i for i, s in seen.items() if s == best)


def test_greedy_tail_is_the_unjudged_documents_by_descending_index():
    rel = np.zeros((9, 3), np.uint8)
    rel[2, 0] = rel[5, 1] = rel[6, 0] = 1
    assert NR.ideal_order(rel, 0.5) == [6, 5, 2, 8, 7, 4, 3, 1, 0]
    assert NR.ideal_order(np.zeros((4, 2), np.uint8), 0.5) == [3, 2, 1, 0]


def test_restatement_conventions():
    """k = 1 is not divided by S; S == 0 gives zeros and a NaN nNRBP; a run shorter than k freezes the counts and P-IA divides by k S."""
    rele = np.array([[1, 0, 1], [1, 1, 0]], np.uint8)
    r = NR.topic(np.array([3.0, 2.0, 1.0], np.float32), rele)
    assert r["actual_subtopics"] == 2 and r["ERR-IA"][0] == 2.0 and r["alpha-DCG"][0] == 2.0
    assert r["P-IA"][19] == 4.0 / (20 * 2) and r["strec"][19] == 1.0 and r["P-IA"][2] == 4.0 / 6 and r["P-IA"][3] == 4.0 / 8
    z = NR.topic(np.zeros(3, np.float32), np.zeros((2, 3), np.uint8))
    assert z["actual_subtopics"] == 0 and np.isnan(z["nNRBP"]) and z["NRBP"] == 0.0 and not any(z["alpha-nDCG"]) and z["ideal_order"] == [2, 1, 0]
    per_k, per_q, S, ideal = NR.batch(np.zeros((1, 3), np.float32), rele[None].astype(np.float32), lens=[0])
    assert not per_k.any() and np.isnan(per_q[0, 1]) and S[0] == 0 and (ideal == -1).all()
    # NaN scores rank first, then by value descending, ties by index
    assert NR.run_order(np.array([1.0, np.nan, 2.0, 2.0, np.inf, -np.inf, np.nan]), 7).tolist() == [1, 6, 4, 2, 3, 0, 5]


# ---------------------------------------------------------------------------------------------------------------- 3. the ABI symbol
def test_symbol_is_declared_exported_and_bound(lib):
    from ptranking_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == _lib.ABI_VERSION == lib.ptr_abi_version()
    assert int(re.search(r"#define PTR_NDEVAL_DEPTH (\d+)", src).group(1)) == NR.DEPTH == 20
    proto = re.search(r"ptr_ndeval_measures\s*\(([^)]*)\)", src).group(1)
    assert hasattr(lib, "ptr_ndeval_measures") and proto.count(",") + 1 == len(_lib.SIGNATURES["ptr_ndeval_measures"]) == 17
    assert proto.count("double") == 4 and "const int32_t *ks" in proto
    assert "ndeval.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "ndeval.hip"))


def test_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    ks = (ctypes.c_int32 * 40)(*([5, 10, 20] + [1] * 37))

    def call(rele=one, B=1, T=4, L=8, ks=ks, nk=3, alpha=0.5, beta=0.5, depth_m=0, preds=one):
        return lib.ptr_ndeval_measures(preds, rele, None, None, B, T, L, ks, nk, alpha, beta, depth_m, one, one, one, one, None)

    assert call(rele=None) == INVALID and b"NULL" in lib.ptr_last_error()
    for a in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert call(alpha=a) == INVALID and b"alpha" in lib.ptr_last_error()
    for b in (-0.1, 1.1, float("nan")):
        assert call(beta=b) == INVALID and b"beta" in lib.ptr_last_error()
    assert call(depth_m=-1) == INVALID and b"depth_m" in lib.ptr_last_error()
    for bad in (0, 21, -3):
        assert call(ks=(ctypes.c_int32 * 3)(5, bad, 20)) == INVALID and b"cut-off" in lib.ptr_last_error()
    assert call(ks=None) == INVALID
    assert call(T=0) == INVALID and call(L=0) == INVALID and call(B=-1) == INVALID
    assert call(T=33) == UNSUPPORTED and b"PTR_MAX_SUBTOPICS" in lib.ptr_last_error()
    assert call(nk=33) == UNSUPPORTED and b"PTR_MAX_CUTOFFS" in lib.ptr_last_error()
    # the LDS limit coincides with PTR_MAX_LIST_LEN: 32 * 4096 + 1664 bytes fit the 160 KiB of a compute unit, one document more is refused
    assert call(L=4097) == UNSUPPORTED and b"PTR_MAX_LIST_LEN" in lib.ptr_last_error()
    assert 32 * 4096 + 1664 <= 160 * 1024
    for L in (1, 128, 129, 4096):
        assert call(B=0, L=L, T=32) == 0
    assert call(B=0, rele=None, preds=None) == 0                                      # B == 0 succeeds
    assert call(B=0, beta=0.0) == 0 and call(B=0, beta=1.0) == 0 and call(B=0, nk=0, ks=None) == 0
    assert call(B=0, ks=(ctypes.c_int32 * 2)(1, 20), nk=2) == 0


# ---------------------------------------------------------------------------------------------------------------- 4. the Python surface
def test_functional_names_and_cpu_refusal():
    import ptranking_amd.functional as F_
    for name in ("ndeval_measures", "div_ideal_order", "NDEVAL_MEASURES"):
        assert name in F_.__all__ and hasattr(F_, name)
    assert F_.NDEVAL_MEASURES == NR.MEASURES == ("ERR-IA", "nERR-IA", "alpha-DCG", "alpha-nDCG", "NRBP", "nNRBP", "MAP-IA", "P-IA", "strec")
    assert not [n for n in F_.__all__ if ("ndeval" in n or "ideal" in n) and n.endswith("_loss")]
    sig = inspect.signature(F_.ndeval_measures)
    assert list(sig.parameters) == ["preds", "rele", "ks", "alpha", "beta", "depth", "lens", "ntopics", "return_ideal_order"]
    assert (sig.parameters["ks"].default, sig.parameters["alpha"].default, sig.parameters["beta"].default) == ((5, 10, 20), 0.5, 0.5)
    assert list(inspect.signature(F_.div_ideal_order).parameters) == ["rele", "alpha", "lens", "ntopics"]
    p, r = torch.zeros(2, 8), torch.zeros(2, 3, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.ndeval_measures(p, r)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.ndeval_measures(None, r)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.div_ideal_order(r)


def test_ranker_method_exists_and_the_run_file_stays_out():
    import ptranking_amd as pa
    from ptranking_amd.diversity import DivProbRanker
    for cls in (pa.DALETOR, DivProbRanker):
        sig = inspect.signature(cls.ndeval_performance_at_ks)
        assert list(sig.parameters) == ["self", "test_data", "ks", "alpha", "beta", "depth", "need_per_q"]
        assert sig.parameters["ks"].default == [5, 10, 20]
    assert pa.DIV_RANKER_NAMES == ("DALETOR",)
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
          "pointsf": dict(num_features=6, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False, dropout=0.0)}
    r = pa.DALETOR(sf_para_dict=sf, model_para_dict={"rt": 10.0, "top_k": 10}, gpu=False, device="cpu")
    with pytest.raises(NotImplementedError, match="generate_div_run"):
        r.srd_performance_at_ks(test_data=[], max_label=1.0, generate_div_run=True)
