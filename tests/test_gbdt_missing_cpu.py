"""CPU: missing feature values in the native booster (use_missing=True).  The numpy restatement tests/gbdt_missing_ref.py reproduces
scikit-learn's whole fits on data with NaNs (tests/golden/gbdt_sklearn_missing.npz), the gate constant is measured here from the
restatement alone, and one planted fault per rule makes a comparison fail; the parameter, bin_edges under the switch, both model formats
on host-built trees, and the argument errors of every new entry point, all without a GPU."""
import ctypes as C
import functools
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import gbdt_missing_ref as MR
import gbdt_ref as R
import gbdt_sk as SK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ptr_gbdt_bin_missing", "ptr_gbdt_best_split_missing", "ptr_gbdt_best_split_slots_missing", "ptr_gbdt_partition_missing",
                "ptr_gbdt_partition_segments_missing", "ptr_gbdt_add_tree_binned_missing", "ptr_gbdt_predict_missing")
CASES = ("p", "q", "r", "s", "t")


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def fixture():
    return MR.load()


@functools.lru_cache(maxsize=None)
def unfaulted(name):
    return MR.compare_restatement(fixture()[0][name])


# ---------------------------------------------------------------- the restatement against scikit-learn
def test_fixture_cases_are_the_ones_the_issue_asks_for():
    cases, version = fixture()
    assert tuple(sorted(cases)) == CASES and version
    for name, c in cases.items():
        nanf = c["nan"].any(axis=0)
        assert 2 <= nanf.sum() <= 4 and 0.15 < c["nan"][:, nanf].mean() < 0.35, name
        nodes = np.concatenate(c["nodes"])
        with_missing = nodes[:, 4] > 0
        assert np.isinf(nodes[:, 1]).any() and (with_missing & (nodes[:, 3] == 1)).any(), name          # NaN against the rest; missing-left
        assert (with_missing & (nodes[:, 3] == 0) & np.isfinite(nodes[:, 1])).any(), name                 # missing-right by a learned direction
        bearing = c["fresh_nan"].any(axis=1)
        assert bearing.sum() >= 40 and c["fresh_compared"][bearing].mean() >= 0.9, name
        assert c["fresh_nan"][:, ~nanf].any(), name                                                     # NaNs where training had none
        # of the rows without a NaN, the ones set below and above the training range and those on the threshold of a node with several
        # spellings part ways where the spellings do: 6 + at most 30 of about 65; most of them stay
        assert c["fresh_compared"][~bearing].mean() >= 0.8, name
    edges, nbins, nan_bin = MR.bin_edges(cases["q"]["X"], 255)
    assert nbins[5] == 200 and nan_bin[5] == 200
    edges, nbins, nan_bin = MR.bin_edges(cases["r"]["X"], 256)
    assert cases["r"]["params"]["max_bin"] == 256 and nbins[5] == 255 and nan_bin[5] == 255
    assert cases["r"]["w"] is not None and cases["s"]["w"] is not None and cases["s"]["params"]["max_depth"] == 3
    assert cases["t"]["params"]["depthwise"] == 1 and cases["t"]["params"]["num_leaves"] == 2 ** cases["t"]["params"]["max_depth"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_sklearn_fits_with_nans(name):
    """Every tree equal to sklearn's in canonical form (nodes, the missing rows under them, the direction where it is decided, the leaves'
    row counts), every training score after every round and every compared fresh prediction within the gate."""
    miss, need, leaf_need, margin = unfaulted(name)
    print(f"MEASURED gbdt missing restatement vs sklearn {fixture()[1]}, case {name}: predictions need C >= {need:.2f}, leaf values {leaf_need:.2f}, "
          f"smallest margin {margin:.2e}")
    assert margin >= SK.MIN_MARGIN
    assert miss is None, miss
    assert need <= MR.C_GBDT_SK_MISSING and leaf_need <= MR.C_GBDT_SK_MISSING


def test_the_gate_constant_is_twice_the_restatements_need():
    worst = max(unfaulted(name)[1] for name in CASES)
    print(f"MEASURED gbdt missing restatement vs sklearn: worst need {worst:.2f}, C_GBDT_SK_MISSING {MR.C_GBDT_SK_MISSING}")
    assert round(worst, 2) == MR.NEED_RECORDED and MR.C_GBDT_SK_MISSING == math.ceil(2.0 * worst)


@pytest.mark.parametrize("fault", ("always_right", "no_nan_split", "minority"))
def test_planted_faults_fail_the_sklearn_comparison(fault):
    """Missing always right, NaN-against-the-rest left out, the majority rule inverted: each fails the whole-fit comparison (the two small
    cases are enough)."""
    cases = fixture()[0]
    failed = {name: MR.compare_restatement(cases[name], fault)[0] for name in ("p", "s")}
    print(f"fault {fault}: {failed}")
    assert all(m is not None for m in failed.values())
    if fault == "minority":
        assert all("missing_go_to_left" in m for m in failed.values())


def tie_histogram(max_bin=16, nan_bin=5):
    """One feature of nan_bin value bins whose NaN bin holds rows of zero gradient and zero Hessian: the two directions of every bin tie
    exactly, and the rows (MC > 0) decide.  -> (hist [1, max_bin, 3], nbins, nan_bin, expo)."""
    hist = np.zeros((1, max_bin, 3), np.int64)
    hist[0, :nan_bin] = [(-(1 << 20) * (b < 2) + (1 << 20) * (b >= 2), 1 << 22, 10) for b in range(nan_bin)]
    hist[0, nan_bin] = (0, 0, 7)
    return hist, np.array([nan_bin], np.int32), np.array([nan_bin], np.int32), (20, 20)


def test_a_tie_of_the_two_directions_keeps_missing_right_and_the_planted_fault_shows():
    """The whole fits hold no exact tie of the two directions with missing rows in the node (it takes missing rows of zero Hessian), so this
    fault is planted against a hand-made histogram: the records differ in field 2."""
    hist, nbins, nan_bin, expo = tie_histogram()
    good, bad = (MR.best_split(hist, nbins, nan_bin, expo, min_hess=0.0, fault=f) for f in (None, "tie_left"))
    assert good["gain"] == bad["gain"] > 0 and good["missing"] == 7
    assert (good["bin"], good["default_left"]) == (1, 0) and (bad["bin"], bad["default_left"]) == (1, 1)
    assert not np.array_equal(MR.record(good), MR.record(bad)) and MR.record(good)[2] == 1 and MR.record(bad)[2] == 257
    assert MR.margin(good) == 0.0                                        # two partitions of the rows at one gain: the screen would redraw such a fit
    empty = hist.copy()
    empty[0, 5] = 0                                                      # MC == 0: the two directions are ONE candidate, the margin is to another bin
    assert 0.1 < MR.margin(MR.best_split(empty, nbins, nan_bin, expo, min_hess=0.0)) < np.inf


def test_scan_rules_on_hand_made_histograms():
    expo = (0, 0)
    nbins, nan_bin = np.array([4], np.int32), np.array([4], np.int32)
    base = np.zeros((1, 8, 3), np.int64)
    base[0, :4] = [(-40, 10, 10), (-38, 10, 10), (40, 10, 10), (42, 10, 10)]
    # MC == 0: the candidates of the scan without missing values, bit for bit, and the majority child
    s, old = MR.best_split(base, nbins, nan_bin, expo), R.best_split(base, nbins, expo)
    assert (s["gain"], s["feature"], s["bin"], s["left"], s["right"]) == (old["gain"], old["feature"], old["bin"], old["left"], old["right"])
    assert s["missing"] == 0 and s["default_left"] == 0                  # 20 rows against 20: not more on the left
    lop = base.copy()
    lop[0, 0, 2] = 30
    assert MR.best_split(lop, nbins, nan_bin, expo)["default_left"] == 1 and MR.best_split(lop, nbins, nan_bin, expo, fault="minority")["default_left"] == 0
    # NaN against the rest wins: the values agree with each other, the NaNs do not
    h = base.copy()
    h[0, :4, 0] = 5
    h[0, 4] = (-300, 10, 10)
    s = MR.best_split(h, nbins, nan_bin, expo)
    assert (s["bin"], s["default_left"], s["left"][2], s["right"]) == (3, 0, 40, (-300, 10, 10)) and MR.record(s)[2] == 3
    assert MR.best_split(h, nbins, nan_bin, expo, fault="no_nan_split")["gain"] < s["gain"]
    # missing-left wins: the NaNs look like the low bins
    h = base.copy()
    h[0, 4] = (-80, 10, 10)
    s = MR.best_split(h, nbins, nan_bin, expo)
    assert (s["bin"], s["default_left"], s["left"]) == (1, 1, (-158, 30, 30)) and MR.record(s)[2] == 257
    assert MR.best_split(h, nbins, nan_bin, expo, fault="always_right")["gain"] < s["gain"]
    # equal gains over an empty bin: the lowest bin with the missing rows right, the highest with them left
    h = np.zeros((1, 8, 3), np.int64)
    h[0, :4] = [(-40, 10, 10), (0, 0, 0), (0, 0, 0), (40, 10, 10)]
    h[0, 4] = (60, 10, 10)
    assert (MR.best_split(h, nbins, nan_bin, expo, min_hess=0.0)["bin"], MR.best_split(h, nbins, nan_bin, expo, min_hess=0.0)["default_left"]) == (0, 0)
    h[0, 4] = (-60, 10, 10)
    s = MR.best_split(h, nbins, nan_bin, expo, min_hess=0.0)
    assert (s["bin"], s["default_left"]) == (2, 1)
    # routing and the raw walk
    bins = np.array([[0], [4], [2], [4], [1]], np.uint8)
    out, cl = MR.partition(bins, np.arange(5), 0, 1, also=4)
    assert out.tolist() == [0, 1, 3, 4, 2] and cl == 4
    out, cl = MR.partition(bins, np.arange(5), 0, 1)
    assert out.tolist() == [0, 4, 1, 2, 3] and cl == 2
    tree = {"feature": np.array([0], np.int32), "threshold": np.array([np.inf], np.float32), "left": np.array([~0], np.int32),
            "right": np.array([~1], np.int32), "value": np.array([-1.0, 1.0], np.float32), "default_left": np.array([0], np.uint8)}
    assert MR.predict(np.array([[3.0], [np.nan], [-2.0]], np.float32), [tree]).tolist() == [-1.0, 1.0, -1.0]


# ---------------------------------------------------------------- the parameter and the binning rule
def test_use_missing_parameter():
    from ptranking_amd import gbdt
    assert gbdt.DEFAULT_PARAMS["use_missing"] is False and gbdt.GBDT().params["use_missing"] is False
    assert gbdt.GBDT({"use_missing": True}).params["use_missing"] is True and gbdt._params({"use_missing": np.bool_(True)})["use_missing"] is True
    for bad in (1, 0, "true", None, 1.0):
        with pytest.raises(ValueError, match="use_missing must be True or False"):
            gbdt.GBDT({"use_missing": bad})
    assert gbdt.MODEL_FORMAT == 1 and gbdt.MODEL_FORMAT_MISSING == 2
    assert "LightGBM's own default is True" in gbdt.__doc__


def test_bin_edges_under_the_switch():
    from ptranking_amd import gbdt
    rng = np.random.default_rng(5)
    X = rng.integers(0, 40, (500, 4)).astype(np.float32) / 4
    X[:, 3] = rng.standard_normal(500).astype(np.float32)                   # more distinct values than bins
    Xn = X.copy()
    Xn[rng.random(500) < 0.25, 1] = np.nan
    Xn[rng.random(500) < 0.25, 3] = np.nan
    for mb in (8, 16, 64, 256):
        e0, n0 = gbdt.bin_edges(X, mb)
        e1, n1, nb1 = gbdt.bin_edges(X, mb, use_missing=True)
        assert np.array_equal(e0, e1) and np.array_equal(n0, n1) and (nb1 == -1).all()       # no NaN: exactly as without the switch
        e, nb, nanb = gbdt.bin_edges(Xn, mb, use_missing=True)
        re_, rnb, rnan = MR.bin_edges(Xn, mb)
        assert np.array_equal(e, re_) and np.array_equal(nb, rnb) and np.array_equal(nanb, rnan)
        assert np.array_equal(e[[0, 2]], e0[[0, 2]]) and np.array_equal(nb[[0, 2]], n0[[0, 2]]) and nanb[0] == nanb[2] == -1
        for f in (1, 3):
            assert nanb[f] == nb[f] <= mb - 1 and np.isinf(e[f, nb[f] - 1:]).all()
            ev, nv = gbdt.bin_edges(Xn[~np.isnan(Xn[:, f])][:, f:f + 1], mb - 1)           # the NaNs ignored: the rule under max_bin - 1
            assert nv[0] == nb[f] and np.array_equal(ev[0], e[f, :mb - 2])
        assert nb[3] == mb - 1
    with pytest.raises(ValueError, match="missing values are not handled"):
        gbdt.bin_edges(Xn, 16)
    Xi = Xn.copy()
    Xi[0, 0] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        gbdt.bin_edges(Xi, 16, use_missing=True)
    e, nb, nanb = gbdt.bin_edges(np.full((5, 1), np.nan, np.float32), 16, use_missing=True)    # nothing but NaNs
    assert nb[0] == 1 and nanb[0] == 1


# ---------------------------------------------------------------- the model file
def host_tree(missing):
    t = {"feature": np.array([0, 1], np.int32), "threshold": np.array([0.5, np.inf], np.float32), "left": np.array([1, ~0], np.int32),
         "right": np.array([~2, ~1], np.int32), "value": np.array([-1.0, 1.0, 0.5], np.float32)}
    if missing:
        t["default_left"] = np.array([1, 0], np.uint8)
    return t


def test_model_formats_round_trip(tmp_path):
    from ptranking_amd import gbdt
    edges, nbins = np.full((2, 15), np.inf, np.float32), np.array([2, 1], np.int32)
    edges[0, 0] = 0.5
    # format 1: the file as it was before the switch existed; the switch is not among its parameters
    m = gbdt.GBDT({"num_leaves": 4, "max_bin": 16})
    m.edges, m.nbins, m.trees = edges, nbins, [host_tree(False)]
    m.save_model(tmp_path / "one.npz")
    with np.load(tmp_path / "one.npz", allow_pickle=False) as z:
        assert int(z["format"]) == 1 and "default_left" not in z.files and "nan_bin" not in z.files
        assert sorted(z.files) == sorted(["format", "params", "edges", "nbins", "best_iteration", "feature", "threshold", "left", "right", "value",
                                          "tree_offsets"])
        assert "use_missing" not in json.loads(str(z["params"]))
    back = gbdt.GBDT.load_model(tmp_path / "one.npz")
    assert back.params == m.params and back.nan_bin is None and "default_left" not in back.trees[0] and "default_left" not in back.flat()
    # format 2
    m = gbdt.GBDT({"num_leaves": 4, "max_bin": 16, "use_missing": True})
    m.edges, m.nbins, m.nan_bin, m.trees = edges, nbins, np.array([-1, 1], np.int32), [host_tree(True), host_tree(True)]
    m.best_iteration = 1
    m.save_model(tmp_path / "two.npz")
    with np.load(tmp_path / "two.npz", allow_pickle=False) as z:
        assert int(z["format"]) == 2 and z["default_left"].dtype == np.uint8 and z["default_left"].tolist() == [1, 0, 1, 0]
        assert z["nan_bin"].tolist() == [-1, 1] and json.loads(str(z["params"]))["use_missing"] is True
        store = {k: z[k] for k in z.files}
    back = gbdt.GBDT.load_model(tmp_path / "two.npz")
    assert back.params == m.params and back.best_iteration == 1 and back.nan_bin.tolist() == [-1, 1] and len(back.trees) == 2
    for a, b in zip(back.trees, m.trees):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    for k, v in m.flat().items():
        assert np.array_equal(back.flat()[k], v)
    # a format the reader does not know, and a file whose format and switch disagree
    for fmt, params in ((3, store["params"]), (1, store["params"])):
        with open(tmp_path / "bad.npz", "wb") as fh:
            np.savez(fh, **dict(store, format=np.int64(fmt), params=params))
        with pytest.raises(ValueError, match="model format"):
            gbdt.GBDT.load_model(tmp_path / "bad.npz")


# ---------------------------------------------------------------- the library without a GPU
def test_symbols_are_declared_exported_and_bound(lib):
    from ptranking_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptranking_amd.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        proto = re.search(name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert proto.count(",") + 1 == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name)
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION == lib.ptr_abi_version()


def test_argument_errors_fire_before_any_launch(lib):
    one, two, f64 = C.c_void_p(64), C.c_void_p(128), C.c_double

    def err(rc, code, text):
        assert rc == code and text in lib.ptr_last_error(), (rc, lib.ptr_last_error())

    def binm(X=one, n=4, F=3, edges=one, nbins=one, nan_bin=one, mb=16, stride=16, bins=one):
        return lib.ptr_gbdt_bin_missing(X, n, F, edges, nbins, nan_bin, mb, stride, bins, None)
    for k in ("X", "edges", "nbins", "nan_bin", "bins"):
        err(binm(**{k: None}), 1001, b"NULL")
    err(binm(mb=1), 1001, b"max_bin")
    err(binm(mb=257), 1002, b"max_bin")
    err(binm(n=-1), 1001, b"size")
    err(binm(stride=12), 1001, b"stride")
    err(binm(F=20), 1001, b"stride")
    assert binm(n=0, X=None, edges=None, nbins=None, nan_bin=None, bins=None) == 0

    args = (f64(0.0), C.c_int64(1), f64(1e-3), f64(0.0))

    def split(hist=one, L=2, F=3, mb=16, nbins=one, nan_bin=one, expo=one, a=args, ws=one, rec=one):
        return lib.ptr_gbdt_best_split_missing(hist, L, F, mb, nbins, nan_bin, expo, *a, ws, rec, None)
    for k in ("hist", "nbins", "nan_bin", "expo", "ws", "rec"):
        err(split(**{k: None}), 1001, b"NULL")
    err(split(L=-2), 1001, b"negative")
    err(split(mb=1), 1001, b"max_bin")
    err(split(mb=257), 1002, b"max_bin")
    err(split(a=(f64(-1.0), C.c_int64(1), f64(1e-3), f64(0.0))), 1001, b"lambda_l2")
    err(split(a=(f64(0.0), C.c_int64(1), f64(float("nan")), f64(0.0))), 1001, b"NaN")
    assert split(L=0, hist=None, nbins=None, nan_bin=None, expo=None, ws=None, rec=None) == 0

    def slots(pool=one, ns=4, sl=one, K=2, F=3, mb=16, nbins=one, nan_bin=one, expo=one, a=args, ws=one, rec=one):
        return lib.ptr_gbdt_best_split_slots_missing(pool, ns, sl, K, F, mb, nbins, nan_bin, expo, *a, ws, rec, None)
    for k in ("pool", "sl", "nbins", "nan_bin", "expo", "ws", "rec"):
        err(slots(**{k: None}), 1001, b"NULL")
    err(slots(K=-1), 1001, b"K=-1")
    err(slots(mb=1), 1001, b"max_bin")
    err(slots(mb=257), 1002, b"max_bin")
    err(slots(F=0), 1001, b"F must be >= 1")
    err(slots(ns=-1), 1001, b"nslots=-1")
    err(slots(a=(f64(-1.0), C.c_int64(1), f64(1e-3), f64(0.0))), 1001, b"lambda_l2")
    assert slots(K=0, pool=None, sl=None) == 0

    def part(bins=one, stride=16, n=8, F=3, rows=one, m=4, feature=0, b=0, also=-1, out=two, lc=one, ws=one):
        return lib.ptr_gbdt_partition_missing(bins, stride, n, F, rows, m, feature, b, also, out, lc, ws, None)
    for k in ("bins", "rows", "out", "ws"):
        err(part(**{k: None}), 1001, b"NULL")
    err(part(lc=None), 1001, b"left_count")
    err(part(m=-4), 1001, b"row count")
    err(part(feature=3), 1001, b"feature")
    err(part(b=256), 1001, b"bin")
    err(part(also=-2), 1001, b"also_left")
    err(part(also=256), 1001, b"also_left")
    err(part(stride=12), 1001, b"stride")

    def segs(bins=one, stride=16, n=8, F=3, rows=one, nrows=8, sg=one, K=2, blocks=one, nb=2, out=two, lc=one, ws=one, ws_ints=3):
        return lib.ptr_gbdt_partition_segments_missing(bins, stride, n, F, rows, nrows, sg, K, blocks, nb, out, lc, ws, ws_ints, None)
    for k in ("bins", "rows", "sg", "blocks", "out", "lc", "ws"):
        err(segs(**{k: None}), 1001, b"NULL")
    err(segs(K=-1), 1001, b"K=-1")
    err(segs(F=0), 1001, b"F must be >= 1")
    err(segs(stride=8), 1001, b"stride")
    err(segs(nb=-1), 1001, b"size")
    err(segs(out=one), 1001, b"out must not be rows")
    err(segs(ws_ints=2), 1001, b"workspace too small")

    def walk(scores=one, bins=one, stride=16, n=8, F=3, rows=one, m=8, feature=one, b=one, left=one, right=one, value=one, also=one, nn=3):
        return lib.ptr_gbdt_add_tree_binned_missing(scores, bins, stride, n, F, rows, m, feature, b, left, right, value, also, nn, None)
    for k in ("scores", "bins", "feature", "b", "left", "right", "value", "also"):
        err(walk(**{k: None}), 1001, b"NULL")
    err(walk(stride=12), 1001, b"stride")
    err(walk(m=-1), 1001, b"m=-1")
    err(walk(nn=-1), 1001, b"nnodes=-1")
    err(walk(rows=None, m=9), 1001, b"rows is NULL")
    assert walk(m=0, rows=None) == 0

    def pred(X=one, n=4, F=3, feature=one, thr=one, left=one, right=one, value=one, offs=one, dl=one, nt=1, out=one):
        return lib.ptr_gbdt_predict_missing(X, n, F, feature, thr, left, right, value, offs, dl, nt, out, None)
    for k in ("X", "out"):
        err(pred(**{k: None}), 1001, b"NULL")
    for k in ("feature", "thr", "left", "right", "value", "offs", "dl"):
        err(pred(**{k: None}), 1001, b"NULL tree")
    err(pred(n=-4), 1001, b"negative")
    err(pred(nt=-1), 1001, b"negative")
    assert pred(n=0, X=None, out=None) == 0


def test_python_surface_refuses_to_run_without_a_gpu():
    import ptranking_amd as pa
    Fn = pa.functional
    f32, i32, u8, i64 = (lambda *s: torch.zeros(s, dtype=torch.float32)), (lambda *s: torch.zeros(s, dtype=torch.int32)), \
        (lambda *s: torch.zeros(s, dtype=torch.uint8)), (lambda *s: torch.zeros(s, dtype=torch.int64))
    calls = [lambda: Fn.gbdt_bin(f32(4, 3), f32(3, 15), i32(3), nan_bin=i32(3)),
             lambda: Fn.gbdt_best_split(i64(1, 3, 16, 3), i32(3), i32(2), nan_bin=i32(3)),
             lambda: Fn.gbdt_partition(u8(4, 16), i32(2), 0, 0, 3, also_left=4),
             lambda: Fn.gbdt_predict(f32(4, 3), i32(0), f32(0), i32(0), i32(0), f32(1), i32(2), default_left=u8(0)),
             lambda: Fn.gbdt_add_tree_binned(f32(4), u8(4, 16), 3, None, i32(1), i32(1), i32(1), i32(1), f32(2), also_left=i32(1))]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pa.GBDT({"use_missing": True}, X=np.full((4, 3), np.nan, np.float32))
