"""CPU: the tree frame's objectives without a GPU — the float64 restatement (tests/tree_ref.py) against the reference's own float64 runs
(tests/golden/tree.npz), the five findings the fixtures prove, the bounds (neither vacuous nor impossible), the two additive ABI v8 entry
points (declared, exported, bound, argument errors before any launch), the Python surface, install_tree() and the length bucketing."""
import ctypes
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import f64_loss_bounds as FB
import golden_util as GU
import tree_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
REF = os.environ.get("PTRANKING_REF") or "/root/reference"
ENTRY_POINTS = ("ptr_tree_pair_grad_hess", "ptr_tree_listnet_grad_hess")
UTIL = "ptranking.ltr_tree.util.lightgbm_util"
USER = "ptranking.ltr_tree.lambdamart.lightgbm_lambdaMART"


def golden():
    return GU._load("tree.npz")


def rows(fam):
    g = golden()[fam]
    return [(case, r) for case in sorted(g, key=lambda k: (len(k), k)) for r in range(len(g[case]["combos"]))]


def combo(c, row):
    p, w, e = (int(v) for v in c["combos"][row])
    return TR.PAIR_TYPES[p], TR.WEIGHTINGS[w], float(e)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.nanmax(np.abs(a - b), initial=0.0)) / max(1.0, float(np.nanmax(np.abs(b), initial=0.0)))


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import build, _lib
    build.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("case,row", rows("pq"))
def test_restatement_reproduces_the_reference_in_float64(case, row):
    c = golden()["pq"][case]
    pt, w, eps = combo(c, row)
    grad, _, hess, _ = TR.pair_query(c["preds"], c["labels"], pt, w, eps, "reference")
    assert rel(grad, c["res"][row, 0]) <= 1e-12 and rel(hess, c["res"][row, 1]) <= 1e-12


@pytest.mark.parametrize("case", sorted(golden()["pq"], key=lambda k: (len(k), k)))
def test_listnet_restatement_reproduces_the_reference(case):
    c = golden()["pq"][case]
    for k, gain_type in enumerate(TR.GAIN_TYPES):
        grad, _, hess, _ = TR.listnet_query(c["preds"], c["labels"], gain_type)
        assert rel(grad, c["listnet"][k, 0]) <= 1e-12 and rel(hess, c["listnet"][k, 1]) <= 1e-12


def test_golden_cases_cover_the_issue_list():
    g = golden()
    assert {len(c["preds"]) for c in g["pq"].values()} == {1, 2, 3, 17, 64, 65, 130}
    for c in g["pq"].values():
        assert {tuple(int(v) for v in r) for r in c["combos"]} == {(p, w, e) for p in range(4) for w in range(3) for e in (1, 2)}
        assert c["preds"].dtype == np.float32 and len(np.unique(c["preds"])) == len(c["preds"])      # distinct: no tie meets the unstable sort
    w = g["wr"]["ragged"]
    assert list(w["group"]) == [12, 1, 18, 64, 3] and w["res"].shape == (6, 2, 98) and len(w["names"]) == 6
    head = 0
    for n in w["group"]:
        assert len(np.unique(w["preds"][head:head + n])) == n
        head += n
    assert set(g["edge"]) == {"equal_labels", "norel", "nanscore"}


@pytest.mark.parametrize("case,row", rows("edge"))
def test_edge_lists_as_the_reference_returns_them(case, row):
    c = golden()["edge"][case]
    pt, w, eps = combo(c, row)
    grad, _, hess, _ = TR.pair_query(c["preds"], c["labels"], pt, w, eps, "reference")
    ref_g, ref_h = c["res"][row]
    if case == "equal_labels":
        assert pt == "NoTies" and not ref_g.any() and not ref_h.any() and not grad.any() and not hess.any()
    elif case == "norel":
        assert w == "DeltaNDCG" and np.isnan(ref_g).all() == (pt != "No00")             # No00 keeps no pair: exactly 0, the 0 / 0 is never read
        assert rel(grad, ref_g) == 0.0 and rel(hess, ref_h) == 0.0
    elif pt == "All":
        assert np.isnan(ref_g).all() and np.isnan(ref_h).all() and np.isnan(grad).all() and np.isnan(hess).all()
    else:
        # NoTies: the reference keeps the documents that never meet the NaN one finite; the product's rule (COVERAGE a9) gives the list NaN
        assert 0 < np.isnan(ref_g).sum() < len(ref_g) and np.isnan(grad).all()


# ---------------------------------------------------------------------------------------------------------------- 2. the findings
def wrapper_case():
    w = golden()["wr"]["ragged"]
    return w, {str(n): w["res"][k] for k, n in enumerate(w["names"])}


def test_finding_1_the_lambdarank_wrappers_apply_no_weight():
    w, res = wrapper_case()
    plain = TR.pair(w["preds"], w["labels"], w["group"], pair_type="NoTies", weighting=None)
    weighted = TR.pair(w["preds"], w["labels"], w["group"], pair_type="NoTies", weighting="DeltaNDCG")
    for name in ("lightgbm_custom_obj_lambdarank", "lightgbm_custom_obj_lambdarank_fobj"):
        assert rel(plain["grad"], res[name][0]) <= 1e-12 and rel(plain["hess"], res[name][1]) <= 1e-12
        assert np.abs(weighted["grad"] - res[name][0]).max() > 1.0          # nowhere near the Delta-nDCG weighted objective
    ranknet = TR.pair(w["preds"], w["labels"], w["group"], pair_type="All")
    listnet = TR.listnet(w["preds"], w["labels"], w["group"], gain_type="Power")
    for name in ("lightgbm_custom_obj_ranknet", "lightgbm_custom_obj_ranknet_fobj"):
        assert rel(ranknet["grad"], res[name][0]) <= 1e-12 and rel(ranknet["hess"], res[name][1]) <= 1e-12
    for name in ("lightgbm_custom_obj_listnet", "lightgbm_custom_obj_listnet_fobj"):
        assert rel(listnet["grad"], res[name][0]) <= 1e-12 and rel(listnet["hess"], res[name][1]) <= 1e-12


def test_finding_2_the_reference_hessian_is_negative_for_low_ranked_documents():
    w, res = wrapper_case()
    assert (res["lightgbm_custom_obj_ranknet"][1] < 0).sum() > 10 and (res["lightgbm_custom_obj_lambdarank"][1] < 0).sum() > 10
    c = golden()["pq"]["n130"]
    for row in range(len(c["combos"])):
        pt, wt, eps = combo(c, row)
        if pt == "All":
            assert c["res"][row, 1].min() < 0
            assert TR.pair_query(c["preds"], c["labels"], pt, wt, eps, "sum")[2].min() > 0              # what LightGBM and XGBoost do
    # the lowest-ranked document has every partner above it: its Hessian is minus the 'sum' one
    s, y = c["preds"], c["labels"]
    last = int(np.argmin(s))
    assert TR.pair_query(s, y, "All", None, 1.0, "reference")[2][last] == -TR.pair_query(s, y, "All", None, 1.0, "sum")[2][last]


def test_finding_3_the_hessian_ignores_epsilon_inside_the_sigmoid():
    c = golden()["pq"]["n17"]
    s, y = c["preds"].astype(np.float64), c["labels"].astype(np.float64)
    r1 = {combo(c, r): c["res"][r] for r in range(len(c["combos"]))}
    assert rel(r1[("All", None, 2.0)][1], 4.0 * r1[("All", None, 1.0)][1]) <= 1e-12           # epsilon^2 outside, epsilon 1 inside
    d = s[:, None] - s[None, :]
    inside = 4.0 * FB._sig(2.0 * d) * (1.0 - FB._sig(2.0 * d))
    sign = np.where(TR.ranks_of(s)[None, :] > TR.ranks_of(s)[:, None], 1.0, -1.0) * ~np.eye(17, dtype=bool)
    assert rel((sign * inside).sum(1), r1[("All", None, 2.0)][1]) > 1e-2


def test_finding_5_equal_scores_rank_by_original_index():
    y = np.array([0.0, 2.0, 1.0, 0.0, 3.0])
    s = np.zeros(5)
    assert list(TR.ranks_of(s)) == [0, 1, 2, 3, 4]
    _, _, hess, _ = TR.pair_query(s, y, "All", None, 1.0, "reference")
    assert list(hess) == [1.0, 0.5, 0.0, -0.5, -1.0]                                            # (below - above) / 4


# ---------------------------------------------------------------------------------------------------------------- 3. the bounds
BOUND_CASES = [(pt, w, eps, h) for pt in TR.PAIR_TYPES for w in TR.WEIGHTINGS for eps in (1.0, 2.0) for h in ("reference", "sum")]


@pytest.fixture(scope="module")
def bound_inputs():
    group = [1, 2, 17, 64, 130]
    out = []
    for offset in (0.0, 1e3):
        s, y = TR.tree_inputs(group, seed=3, offset=offset)
        out.append((group, s, y))
    return out


@pytest.mark.parametrize("pt,w,eps,h", BOUND_CASES)
def test_eager_fp32_passes_the_gate(bound_inputs, pt, w, eps, h):
    """The bounds are not impossible: a plain fp32 evaluation of the closed form (eager torch on the CPU) is inside them, with a common
    offset of 1e3 on the scores as well."""
    for group, s, y in bound_inputs:
        ref = TR.pair(s, y, group, pair_type=pt, weighting=w, eps=eps, hessian=h)
        off = TR.offsets_of(group)
        got = [TR.eager_pair_query(s[a:b], y[a:b], pt, w, eps, h) for a, b in zip(off[:-1], off[1:])]
        TR.gate(np.concatenate([g for g, _ in got]), np.concatenate([hh for _, hh in got]), ref, f"eager fp32 {pt} {w} eps {eps} {h}", FB.C_PAIR)


def test_eager_fp32_listnet_passes_the_gate(bound_inputs):
    for group, s, y in bound_inputs:
        for gain_type in TR.GAIN_TYPES:
            ref = TR.listnet(s, y, group, gain_type=gain_type)
            off = TR.offsets_of(group)
            grad, hess = [], []
            for a, b in zip(off[:-1], off[1:]):
                S, Y = torch.from_numpy(s[a:b]), torch.from_numpy(y[a:b])
                p = torch.softmax(S, 0)
                grad.append((p - torch.softmax(torch.exp2(Y) - 1.0 if gain_type == "Power" else Y, 0)).numpy())
                hess.append((p * (1.0 - p)).numpy())
            TR.gate(np.concatenate(grad), np.concatenate(hess), ref, f"eager fp32 listnet {gain_type}", FB.C_LIST)


@pytest.mark.parametrize("pt,w,eps,h", [c for c in BOUND_CASES if c[0] in ("All", "NoTies")])
def test_a_relative_error_of_1e_5_fails_the_gate(bound_inputs, pt, w, eps, h):
    """The bounds are not vacuous: one gradient element moved by 1e-5 of its sum |terms| fails, and so does a Hessian element — moved by
    1e-4 under DeltaNDCG: the Hessian's largest terms are the pairs of nearly equal scores, hence of adjacent ranks, whose weight |D_i - D_j|
    is the difference of two nearly equal discounts and carries c u (D_i + D_j) (1e-4 of it at rank 100); at 130 documents that alone is
    1.2e-5 of sum |h|."""
    group, s, y = bound_inputs[0]
    ref = TR.pair(s, y, group, pair_type=pt, weighting=w, eps=eps, hessian=h)
    off = TR.offsets_of(group)
    for q in (2, 3, 4):
        a, b = off[q], off[q + 1]
        sumT, sumh = TR.pair_abs_terms(s[a:b], y[a:b], pt, w, eps)
        for key, sums in (("grad", sumT), ("hess", sumh)):
            i = int(np.argmax(sums))
            assert sums[i] > 0
            moved = {k: ref[k].copy() for k in ("grad", "hess")}
            moved[key][a + i] += (1e-4 if key == "hess" and w == "DeltaNDCG" else 1e-5) * sums[i]
            with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
                TR.gate(moved["grad"], moved["hess"], ref, "moved", FB.C_PAIR)


def test_the_signed_hessian_is_bounded_against_the_sum_of_its_terms():
    """A middle-ranked document's signed Hessian cancels to almost nothing; its bound does not shrink with it."""
    c = golden()["pq"]["n130"]
    s, y = c["preds"], c["labels"]
    _, _, hess, E = TR.pair_query(s, y, "All", None, 1.0, "reference")
    _, sumh = TR.pair_abs_terms(s, y, "All", None, 1.0)
    i = int(np.argmin(np.abs(hess)))
    assert abs(hess[i]) < 0.05 * sumh[i] and E[i] >= FB.C_PAIR * TR.U * np.sqrt(129.0) * sumh[i]


# ---------------------------------------------------------------------------------------------------------------- 4. the ABI
def header_src():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_abi_stays_v8_and_declares_exports_and_binds_both_entry_points(lib):
    from ptranking_amd import _lib, build
    import ptranking_amd.functional as F_
    src = header_src()
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == _lib.ABI_VERSION == lib.ptr_abi_version()
    for name in ENTRY_POINTS:
        proto = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert hasattr(lib, name) and proto.count(",") + 1 == len(_lib.SIGNATURES[name]), name
    doc = open(HEADER).read()
    for finding in ("Finding 1", "Finding 2", "Finding 3", "Finding 4", "Finding 5", "lightgbm_util.py:120-183", ":308-330"):
        assert finding in doc, finding
    for prefix, table in (("PAIRS_", {"ALL": "All", "NOTIES": "NoTies", "NO00": "No00", "00": "00"}),
                          ("W_", {"NONE": None, "DELTA_NDCG": "DeltaNDCG", "DELTA_GAIN": "DeltaGain"}),
                          ("HESS_", {"REFERENCE": "reference", "SUM": "sum", "CONSTANT": "constant"}), ("GAIN_", {"POWER": "Power", "LABEL": "Label"})):
        py = {"PAIRS_": F_.TREE_PAIR_TYPES, "W_": F_.TREE_WEIGHTINGS, "HESS_": F_.TREE_HESSIANS, "GAIN_": F_.TREE_GAIN_TYPES}[prefix]
        for cname, pname in table.items():
            assert int(re.search(rf"#define PTR_TREE_{prefix}{cname} (\d+)", src).group(1)) == py[pname]
    assert "tree.hip" in build.SOURCES


def test_argument_errors_need_no_gpu(lib):
    one, f = ctypes.c_void_p(16), ctypes.c_float
    INVALID, UNSUPPORTED = 1001, 1002

    def pair(preds=one, labels=one, offsets=one, B=2, queries=None, nq=2, max_len=8, pair_type=0, weighting=0, eps=1.0, hessian=0, grad=one,
             hess=one):
        return lib.ptr_tree_pair_grad_hess(preds, labels, offsets, B, queries, nq, max_len, pair_type, weighting, f(eps), hessian, grad, hess, None)

    def listnet(preds=one, labels=one, offsets=one, B=2, queries=None, nq=2, max_len=8, gain_type=0, hessian=0, grad=one, hess=one):
        return lib.ptr_tree_listnet_grad_hess(preds, labels, offsets, B, queries, nq, max_len, gain_type, hessian, grad, hess, None)

    for fn in (pair, listnet):
        for kw in (dict(preds=None), dict(labels=None), dict(offsets=None), dict(grad=None), dict(hess=None)):
            assert fn(**kw) == INVALID and b"NULL" in lib.ptr_last_error(), kw
        for kw in (dict(B=-1, nq=-1), dict(nq=-1, queries=one), dict(max_len=-1)):
            assert fn(**kw) == INVALID and b"negative" in lib.ptr_last_error(), kw
        assert fn(nq=1) == INVALID and b"nq must equal B" in lib.ptr_last_error()              # queries == NULL means all B queries
        for hessian in (-1, 3):
            assert fn(hessian=hessian) == INVALID and b"hessian" in lib.ptr_last_error()
        assert fn(max_len=4097) == UNSUPPORTED and b"PTR_MAX_LIST_LEN" in lib.ptr_last_error()
        assert fn(max_len=4096, B=0, nq=0) == 0
        # nothing to launch: no pointer is read
        assert fn(preds=None, labels=None, offsets=None, grad=None, hess=None, B=0, nq=0) == 0
        assert fn(preds=None, labels=None, offsets=None, grad=None, hess=None, B=3, queries=one, nq=0) == 0
    for pair_type in (-1, 4):
        assert pair(pair_type=pair_type) == INVALID and b"pair_type" in lib.ptr_last_error()
    for weighting in (-1, 3):
        assert pair(weighting=weighting) == INVALID and b"weighting" in lib.ptr_last_error()
    for eps in (-1.0, -1e-30, float("nan")):
        assert pair(eps=eps) == INVALID and b"epsilon" in lib.ptr_last_error()
    for gain_type in (-1, 2):
        assert listnet(gain_type=gain_type) == INVALID and b"gain_type" in lib.ptr_last_error()
    # an argument error wins over the unsupported length
    assert pair(max_len=4097, pair_type=9) == INVALID and listnet(max_len=4097, gain_type=9) == INVALID


# ---------------------------------------------------------------------------------------------------------------- 5. the Python surface
def test_cpu_tensors_are_refused():
    import ptranking_amd.functional as F_
    s, y, off = torch.zeros(5), torch.zeros(5), torch.tensor([0, 2, 5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.tree_pair_grad_hess(s, y, off)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.tree_listnet_grad_hess(s, y, off)
    for kw, what in ((dict(pair_type="Ties"), "pair_type"), (dict(weighting=True), "weighting"), (dict(weighting="DeltaMAP"), "weighting"),
                     (dict(hessian="signed"), "hessian")):
        with pytest.raises(ValueError, match=what):
            F_.tree_pair_grad_hess(s, y, off, **kw)
    with pytest.raises(ValueError, match="gain_type"):
        F_.tree_listnet_grad_hess(s, y, off, gain_type="Linear")


def test_tree_objective_without_a_gpu_raises_loudly(monkeypatch):
    import ptranking_amd as pa
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    labels, group, preds = np.array([1.0, 0.0, 2.0]), np.array([3]), np.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pa.TreeObjective(labels, group, "lambdarank")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pa.tree.lightgbm_custom_obj_ranknet(labels=labels, preds=preds, group=group)
    data = types.SimpleNamespace(get_label=lambda: labels, get_group=lambda: group)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pa.tree.lightgbm_custom_obj_listnet_fobj(preds, data)
    lazy = pa.TreeObjective(objective="ranknet")                              # nothing to upload yet
    assert (lazy.pair_type, lazy.weighting, lazy.epsilon, lazy.hessian, lazy.uploads) == ("All", None, 1.0, "reference", 0)
    assert pa.TreeObjective(objective="lambdarank").pair_type == "NoTies"
    with pytest.raises(RuntimeError, match="without labels"):
        lazy(preds)
    for kw, what in ((dict(objective="mart"), "objective"), (dict(objective="ranknet", pair_type="Ties"), "pair_type"),
                     (dict(objective="ranknet", weighting=True), "weighting"), (dict(objective="ranknet", epsilon=-1.0), "epsilon"),
                     (dict(objective="listnet", gain_type="Linear"), "gain_type"), (dict(objective="ranknet", hessian="lightgbm"), "hessian"),
                     (dict(labels=labels), "labels and group")):
        with pytest.raises(ValueError, match=what):
            pa.TreeObjective(**kw)
    assert "fp32-accurate" in pa.TreeObjective.__doc__ and "never negative" in pa.TreeObjective.__doc__


def test_length_bucketing_is_host_code():
    from ptranking_amd.tree import LENGTH_CLASSES, bucket_queries
    assert LENGTH_CLASSES == (16, 128, 256, 512, 1024, 2048, 4096)
    group = [0, 1, 16, 17, 128, 129, 256, 257, 1251, 4096, 3, 0, 2048, 2049]
    got = bucket_queries(np.asarray(group, np.int32))
    assert [(m, list(idx)) for m, idx in got] == [(16, [1, 2, 10]), (128, [3, 4]), (256, [5, 6]), (257, [7]), (2048, [8, 12]), (4096, [9, 13])]
    assert all(idx.dtype == np.int32 for _, idx in got)
    launched = sorted(int(i) for _, idx in got for i in idx)
    assert launched == [q for q, n in enumerate(group) if n > 0]              # every document once; empty queries own no output
    assert bucket_queries([]) == [] and bucket_queries([0, 0]) == []
    assert [(m, list(i)) for m, i in bucket_queries(np.array([5.0, 40.0]))] == [(5, [0]), (40, [1])]     # LightGBM hands group over as floats too
    with pytest.raises(ValueError, match="4097"):
        bucket_queries([3, 4097])
    with pytest.raises(ValueError, match="negative"):
        bucket_queries([3, -1])


# ---------------------------------------------------------------------------------------------------------------- 6. install
def purge():
    for m in [m for m in sys.modules if m == "ptranking" or m.startswith("ptranking.")]:
        del sys.modules[m]


@pytest.fixture
def stand_in_tree_package(tmp_path, monkeypatch):
    """A minimal package with the two module paths install_tree() binds into: placeholder objectives, and a lightgbm_lambdaMART stub that
    imports them BY VALUE as the reference's does (lightgbm itself is not needed)."""
    from ptranking_amd.tree import DROP_IN_NAMES
    root = tmp_path / "stand_in"
    util = "".join(f"def {n}(*args, **kwargs):\n    return '{n}'\n\n\n" for n in DROP_IN_NAMES)
    files = {"ptranking/__init__.py": "", "ptranking/ltr_tree/__init__.py": "", "ptranking/ltr_tree/util/__init__.py": "",
             "ptranking/ltr_tree/lambdamart/__init__.py": "", "ptranking/ltr_tree/util/lightgbm_util.py": util,
             "ptranking/ltr_tree/lambdamart/lightgbm_lambdaMART.py": f"from {UTIL} import \\\n    " + ", ".join(DROP_IN_NAMES) + "\n"}
    for path, text in files.items():
        p = root / path
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(text)
    monkeypatch.setattr(sys, "dont_write_bytecode", True)
    monkeypatch.syspath_prepend(str(root))
    purge()
    yield
    purge()


def test_install_tree_round_trip_on_a_stand_in(stand_in_tree_package):
    import importlib
    import ptranking_amd as pa
    util = importlib.import_module(UTIL)
    before = {n: getattr(util, n) for n in pa.tree.DROP_IN_NAMES}
    installed = pa.install_tree()                                             # the user module is not imported yet: only lightgbm_util is bound
    try:
        assert set(installed) == set(pa.tree.DROP_IN_NAMES) and USER not in sys.modules
        assert all(getattr(util, n) is getattr(pa.tree, n) for n in pa.tree.DROP_IN_NAMES)
        user = importlib.import_module(USER)                                  # imported afterwards: it picks the installed names up by itself
        assert all(getattr(user, n) is getattr(pa.tree, n) for n in pa.tree.DROP_IN_NAMES)
    finally:
        pa.uninstall()
    assert all(getattr(util, n) is before[n] for n in before)
    del sys.modules[USER]
    user = importlib.import_module(USER)                                      # imported BEFORE install_tree(): holds the names by value
    assert all(getattr(user, n) is before[n] for n in before)
    pa.install_tree()
    try:
        assert all(getattr(user, n) is getattr(pa.tree, n) and getattr(util, n) is getattr(pa.tree, n) for n in before)
    finally:
        pa.uninstall()
    assert all(getattr(user, n) is before[n] and getattr(util, n) is before[n] for n in before)
    assert user.lightgbm_custom_obj_ranknet() == "lightgbm_custom_obj_ranknet"


def test_install_and_install_diversification_are_untouched_by_install_tree(stand_in_tree_package):
    import ptranking_amd as pa
    inst = sys.modules["ptranking_amd.install"]                          # (the package attribute `install` is the function)
    pa.install_tree()
    try:
        assert {m for m, _ in inst._saved} == {UTIL}
    finally:
        pa.uninstall()
    assert not inst._saved


needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "ptranking", "ltr_tree")), reason="the reference checkout is not on this machine")


@pytest.fixture
def reference_on_path(monkeypatch):
    monkeypatch.setattr(sys, "dont_write_bytecode", True)
    monkeypatch.syspath_prepend(REF)
    purge()
    yield
    purge()


@needs_reference
def test_drop_in_signatures_match_the_reference(reference_on_path):
    import importlib
    import ptranking_amd as pa
    util = importlib.import_module(UTIL)
    for n in pa.tree.DROP_IN_NAMES:
        assert inspect.signature(getattr(pa.tree, n)) == inspect.signature(getattr(util, n)), n
    assert (pa.tree.FIRST_ORDER, pa.tree.CONSTANT_HESSIAN) == (util.FIRST_ORDER, util.CONSTANT_HESSIAN)
    assert sorted(pa.functional.TREE_GAIN_TYPES) == sorted(util.GAIN_TYPE)
    assert sorted(k for k in pa.functional.TREE_WEIGHTINGS if k) == sorted(util.WEIGHTING_TYPE)


@needs_reference
def test_install_tree_round_trip_on_the_reference(reference_on_path):
    import importlib
    import ptranking_amd as pa
    util = importlib.import_module(UTIL)
    before = {n: getattr(util, n) for n in pa.tree.DROP_IN_NAMES}
    stub = types.ModuleType(USER)                                             # the real module imports lightgbm, which is not installed here
    vars(stub).update(before)
    sys.modules[USER] = stub
    try:
        pa.install_tree()
        try:
            assert all(getattr(util, n) is getattr(pa.tree, n) and getattr(stub, n) is getattr(pa.tree, n) for n in before)
            assert util.per_query_gradient_hessian_lambda.__module__ == UTIL          # nothing else is touched
        finally:
            pa.uninstall()
        assert all(getattr(util, n) is before[n] and getattr(stub, n) is before[n] for n in before)
    finally:
        del sys.modules[USER]
