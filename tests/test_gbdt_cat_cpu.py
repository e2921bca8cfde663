"""CPU: categorical features in the native booster (categorical_feature, cat_smooth).  The numpy restatement tests/gbdt_cat_ref.py
reproduces scikit-learn's whole fits with categorical_features (tests/golden/gbdt_sklearn_cat.npz), the gate constant is measured here
from the restatement alone, and one planted fault per rule makes a comparison fail; the parameters, bin_edges for categorical columns, the
three model formats on host-built trees, and the argument errors of the six new entry points, all without a GPU."""
import ctypes as C
import functools
import json
import math
import os
import re
import zipfile

import numpy as np
import pytest
import torch

import gbdt_cat_ref as CR
import gbdt_ref as R
import gbdt_sk as SK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ptr_gbdt_best_split_cat", "ptr_gbdt_best_split_slots_cat", "ptr_gbdt_partition_cat", "ptr_gbdt_partition_segments_cat",
                "ptr_gbdt_add_tree_binned_cat", "ptr_gbdt_predict_cat")
CASES = ("a", "b", "c", "d", "e", "f")


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def fixture():
    return CR.load()


@functools.lru_cache(maxsize=None)
def unfaulted(name):
    return CR.compare_restatement(fixture()[0][name])


def left_sizes(nodes):
    return [bin(sum(int(w) << (32 * k) for k, w in enumerate(row[5:]))).count("1") for row in nodes]


# ---------------------------------------------------------------- parameters and binning
def test_parameter_defaults_and_validation():
    from ptranking_amd import gbdt
    p = gbdt._params(None)
    assert p["categorical_feature"] == () and p["cat_smooth"] == 10.0 and gbdt.DEFAULT_PARAMS["categorical_feature"] == ()
    assert gbdt._params({"categorical_feature": [7, 3]})["categorical_feature"] == (3, 7)
    assert gbdt._params({"categorical_feature": (np.int64(2), 0)})["categorical_feature"] == (0, 2)
    assert gbdt._params({"categorical_feature": None})["categorical_feature"] == ()
    assert gbdt._params({"cat_smooth": 0})["cat_smooth"] == 0.0 and isinstance(gbdt._params({"cat_smooth": 3})["cat_smooth"], float)
    for bad in ([1, 1], [-1], [1.5], [True], ["3"], 3, "3,7", [[1], [2]]):
        with pytest.raises(ValueError, match="categorical_feature"):
            gbdt._params({"categorical_feature": bad})
    for bad in (-1.0, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="cat_smooth"):
            gbdt._params({"cat_smooth": bad})
    for k in ("max_cat_to_onehot", "cat_l2", "min_data_per_group", "max_cat_threshold"):
        with pytest.raises(ValueError, match="unknown parameter"):
            gbdt._params({k: 1})
        assert k in gbdt.__doc__
    json.dumps(gbdt._params({"categorical_feature": [2]}))               # a model file carries the parameters as JSON


def test_bin_edges_of_categorical_columns():
    from ptranking_amd import gbdt
    rng = np.random.default_rng(3)
    X = np.stack([rng.integers(0, 9, 200), rng.integers(0, 30, 200) / 4, np.concatenate([[0, 63], rng.integers(0, 64, 198)])], axis=1).astype(np.float32)
    X[X[:, 0] == 4, 0] = 5                                               # code 4 never occurs: its bin stays, empty
    edges, nbins = gbdt.bin_edges(X, 64, categorical=[0, 2])
    plain = gbdt.bin_edges(X, 64)
    assert nbins.tolist() == [9, plain[1][1], 64] and np.array_equal(edges[1], plain[0][1])
    assert np.array_equal(edges[0, :8], np.arange(8) + np.float32(0.5)) and np.isinf(edges[0, 8:]).all()
    assert np.array_equal(edges[2], np.arange(63) + np.float32(0.5))
    ref = CR.bin_edges(X, 64, (0, 2))
    assert np.array_equal(edges, ref[0]) and np.array_equal(nbins, ref[1])
    assert np.array_equal(R.bin_matrix(X, edges, nbins)[:, [0, 2]], X[:, [0, 2]].astype(np.uint8))       # code c lands in bin c
    assert all(np.array_equal(a, b) for a, b in zip(gbdt.bin_edges(X, 64, categorical=()), plain))
    for f, bad in ((0, 2.5), (0, -1.0), (2, 64.0)):
        Y = X.copy()
        Y[5, f] = bad
        with pytest.raises(ValueError, match="integer codes"):
            gbdt.bin_edges(Y, 64, categorical=[0, 2])
    with pytest.raises(ValueError, match="categorical_feature 3"):
        gbdt.bin_edges(X, 64, categorical=[3])
    # under use_missing a NaN is accepted, the limit drops to max_bin - 2 where the column holds one, and the NaN bin stays behind the codes
    Y = X.copy()
    Y[::9, 0] = np.nan
    edges, nbins, nan_bin = gbdt.bin_edges(Y, 64, True, categorical=[0, 2])
    assert nbins.tolist()[::2] == [9, 64] and nan_bin.tolist() == [9, -1, -1]
    ref = CR.bin_edges(Y, 64, (0, 2), True)
    assert np.array_equal(edges, ref[0]) and np.array_equal(nbins, ref[1]) and np.array_equal(nan_bin, ref[2])
    Y[::9, 2] = np.nan
    with pytest.raises(ValueError, match="integer codes"):               # code 63 beside a NaN: no room for the NaN bin
        gbdt.bin_edges(Y, 64, True, categorical=[0, 2])
    Y[Y[:, 2] == 63, 2] = 62
    assert gbdt.bin_edges(Y, 64, True, categorical=[0, 2])[2].tolist() == [9, -1, 63]
    with pytest.raises(ValueError, match="NaN"):
        gbdt.bin_edges(Y, 64, categorical=[0, 2])


# ---------------------------------------------------------------- the restatement against scikit-learn
def test_fixture_cases_are_the_ones_the_issue_asks_for():
    cases, version = fixture()
    assert tuple(sorted(cases)) == CASES and version
    for name, c in cases.items():
        p = c["params"]
        assert c["X"].shape[0] <= 1500 and p["rounds"] <= 6, name
        nodes = np.concatenate(c["nodes"])
        assert (nodes[:, 1] > 0).any(), name
        codes = c["X"][:, :p["ncat"]]
        assert np.array_equal(np.where(np.isnan(codes), 0, codes), np.floor(np.where(np.isnan(codes), 0, codes)))
    a, b, c, d, e, f = (cases[k] for k in CASES)
    assert a["params"]["ncat"] == a["X"].shape[1] and (np.concatenate(a["nodes"])[:, 1] > 0).all()             # every feature categorical
    kinds = np.concatenate(b["nodes"])[:, 1]
    assert 0 < b["params"]["ncat"] < b["X"].shape[1] and (kinds > 0).any() and (kinds == 0).any()               # mixed
    assert c["params"]["use_missing"] and c["nan"][:, 1].any() and not c["nan"][:, [0] + list(range(2, 7))].any()
    cn = np.concatenate(c["nodes"])
    assert ((cn[:, 0] == 1) & (cn[:, 4] > 0)).any() and ((cn[:, 0] == 1) & (cn[:, 4] == 0)).any()                 # NaNs sent left, and right
    assert np.isnan(c["fresh"][:, 1]).any()
    assert d["w"] is not None and np.unique(d["w"]).size == 8 and d["w"].size / d["w"].sum() > 3.0       # TC / TH well above 1
    assert np.unique(e["X"][:, 0]).size == 200 and max(left_sizes(np.concatenate(e["nodes"]))) > 16                # the wide column
    counts = np.bincount(e["X"][:, 0].astype(np.int64))
    assert (counts < CR.CAT_SMOOTH).sum() >= 60 and (counts >= CR.CAT_SMOOTH).sum() >= 60
    assert sum((np.bincount(a["X"][:, k].astype(np.int64)) < CR.CAT_SMOOTH).sum() for k in range(5)) >= 5           # low support
    assert f["params"]["depthwise"] and f["params"]["num_leaves"] == 2 ** f["params"]["max_depth"]
    assert os.path.getsize(CR.FILE) < 256 * 1024


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_sklearn(name):
    """Trees, left sets, staged and fresh predictions; the screen held when the archive was written and holds now."""
    miss, need, leaf_need, margin = unfaulted(name)
    print(f"MEASURED gbdt categorical restatement vs sklearn, case {name}: predictions need C >= {need:.2f}, leaf values {leaf_need:.2f}, margin {margin:.2e}")
    assert miss is None, miss
    assert margin >= SK.MIN_MARGIN
    assert need <= CR.C_GBDT_SK_CAT and leaf_need <= CR.C_GBDT_SK_CAT


def test_gate_constant_is_twice_the_restatements_need():
    worst = max(unfaulted(name)[1] for name in CASES)
    print(f"MEASURED gbdt categorical restatement vs sklearn: worst need {worst:.2f} (recorded {CR.NEED_RECORDED})")
    assert abs(worst - CR.NEED_RECORDED) < 0.01
    assert CR.C_GBDT_SK_CAT == math.ceil(2 * CR.NEED_RECORDED)


@pytest.mark.parametrize("fault,name", [("wrong_middle", "a"), ("unused_left", "a"), ("unused_left", "e"), ("nan_ignored", "c"),
                                        ("support_no_factor", "d")])
def test_planted_faults_are_caught(fault, name):
    assert fault in CR.FAULTS
    miss = CR.compare_restatement(fixture()[0][name], fault)[0]
    print(f"fault {fault} on case {name}: {miss}")
    assert miss is not None


def test_the_rule_on_a_hand_made_node():
    """Five codes and an empty bin, unit Hessians, cat_smooth 2: code 4 (one row) is unused and goes right; sorted by key the codes are
    3, 0, 2, 1; left to right {3}, {3, 0}; right to left {1}."""
    ONE, expo = 1 << 10, (10, 10)
    hist = np.zeros((1, 8, 3), np.int64)
    for code, (g, n) in {0: (-2, 4), 1: (9, 3), 2: (1, 5), 3: (-8, 4), 4: (30, 1)}.items():
        hist[0, code] = (g * ONE, n * ONE, n)
    cands, _ = CR.cat_candidates(hist[0], 6, -1, hist[0].sum(axis=0), expo, 0.0, 1, 1e-3, 0.0, 2.0)
    assert [(k, b) for _, k, _, b in cands] == [(0, 1 << 3), (1, (1 << 3) | 1), (256, 1 << 1)]
    s = CR.best_split(hist, np.array([6]), None, np.array([1]), expo, cat_smooth=2.0)
    rec, words = CR.record(s, False)
    assert s["cat"] and s["set"] in (1 << 3, (1 << 3) | 1, 1 << 1) and rec[2] == bin(s["set"]).count("1") and words[0] == s["set"] and not words[1:].any()
    assert rec[5] + rec[8] == 17 and rec[3] + rec[6] == hist[0, :, 0].sum()
    assert CR.best_split(hist, np.array([6]), None, np.array([1]), expo, cat_smooth=6.0)["feature"] == -1       # no code has six rows: nothing is used
    one = CR.best_split(hist, np.array([6]), None, np.array([1]), expo, cat_smooth=5.0)                           # one used code: no split either
    assert one["feature"] == -1
    tie = hist.copy()
    tie[0, 1] = tie[0, 3]                                                # equal keys order by the lower bin: 1 before 3
    cands, _ = CR.cat_candidates(tie[0], 6, -1, tie[0].sum(axis=0), expo, 0.0, 1, 1e-3, 0.0, 2.0)
    assert cands[0][3] == 1 << 1 and cands[1][3] == (1 << 1) | (1 << 3)


# ---------------------------------------------------------------- the model file on the host
def host_booster(params, cats=True):
    from ptranking_amd import gbdt
    b = gbdt.GBDT(params)
    b.edges = np.full((3, 7), np.inf, np.float32)
    b.edges[0, :4] = np.arange(4) + np.float32(0.5)
    b.edges[1, :3] = [0.25, 0.5, 1.0]
    b.nbins = np.array([5, 4, 1], np.int32)
    if b.params["use_missing"]:
        b.nan_bin = np.array([5, -1, -1], np.int32)
    t0 = {"feature": np.array([0, 1], np.int32), "threshold": np.array([0, 0.5], np.float32), "left": np.array([1, ~0], np.int32),
          "right": np.array([~2, ~1], np.int32), "value": np.array([1, 2, 3], np.float32)}
    t1 = {"feature": np.array([1, 0, 0], np.int32), "threshold": np.array([0.25, 0, 0], np.float32), "left": np.array([1, ~0, ~2], np.int32),
          "right": np.array([2, ~1, ~3], np.int32), "value": np.array([4, 5, 6, 7], np.float32)}
    if cats:
        t0.update(cat_index=np.array([0, -1], np.int32), cat_set=CR.set_words(0b10010)[None])
        t1.update(cat_index=np.array([-1, 0, 1], np.int32), cat_set=np.stack([CR.set_words(0b00101), CR.set_words((1 << 5) | 1)]))
    if b.params["use_missing"]:
        t0["default_left"], t1["default_left"] = np.array([0, 1], np.uint8), np.array([0, 0, 1], np.uint8)
    b.trees = [t0, t1]
    return b


@pytest.mark.parametrize("missing", [False, True])
def test_format_3_round_trip_on_the_host(tmp_path, missing):
    from ptranking_amd import gbdt
    b = host_booster({"categorical_feature": [0], "max_bin": 8, "cat_smooth": 2.5, "use_missing": missing})
    fl = b.flat()
    assert fl["cat_index"].tolist() == [0, -1, -1, 1, 2] and fl["cat_sets"].shape == (3, 4) and fl["cat_sets"].dtype == np.int64
    path = tmp_path / "m.npz"
    b.save_model(path)
    with np.load(path, allow_pickle=False) as z:
        assert int(z["format"]) == gbdt.MODEL_FORMAT_CAT == 3 and z["categorical_feature"].tolist() == [0]
        assert ("nan_bin" in z.files) == ("default_left" in z.files) == missing
        assert json.loads(str(z["params"]))["cat_smooth"] == 2.5
    back = gbdt.GBDT.load_model(path)
    assert back.params == b.params and back.params["categorical_feature"] == (0,)
    for t, u in zip(b.trees, back.trees):
        assert sorted(t) == sorted(u) and all(np.array_equal(t[k], u[k]) and t[k].dtype == u[k].dtype for k in t)
    assert all(np.array_equal(v, back.flat()[k]) for k, v in fl.items())
    # a file whose format and parameters disagree is refused
    with np.load(path, allow_pickle=False) as z:
        members = {k: z[k] for k in z.files}
    for change in ({"format": np.int64(2 if missing else 1)}, {"categorical_feature": np.array([1], np.int32)}):
        np.savez(tmp_path / "bad.npz", **dict(members, **change))
        with pytest.raises(ValueError, match="model format"):
            gbdt.GBDT.load_model(tmp_path / "bad.npz")


@pytest.mark.parametrize("missing", [False, True])
def test_formats_1_and_2_keep_their_bytes_and_still_load(tmp_path, missing):
    """Without categorical features the file is the one written before the two keys existed: they are not among its parameters, whatever
    cat_smooth is; and such a file (a format 1 or 2 file of any age) loads with the defaults."""
    from ptranking_amd import gbdt
    members = []
    for k, extra in enumerate(({}, {"categorical_feature": [], "cat_smooth": 3.0})):
        b = host_booster(dict({"max_bin": 8, "use_missing": missing}, **extra), cats=False)
        b.save_model(tmp_path / f"{k}.npz")
        with zipfile.ZipFile(tmp_path / f"{k}.npz") as z:
            members.append([(i.filename, z.read(i.filename)) for i in z.infolist()])
    assert members[0] == members[1]
    with np.load(tmp_path / "1.npz", allow_pickle=False) as z:
        params = json.loads(str(z["params"]))
        assert int(z["format"]) == (2 if missing else 1) and not set(params) & set(gbdt.CAT_KEYS) and ("use_missing" in params) == missing
        assert "cat_index" not in z.files and "cat_sets" not in z.files and "categorical_feature" not in z.files
    back = gbdt.GBDT.load_model(tmp_path / "1.npz")
    assert back.params["categorical_feature"] == () and back.params["cat_smooth"] == 10.0 and back.params["use_missing"] == missing
    assert "cat_index" not in back.flat() and all("cat_index" not in t for t in back.trees)


# ---------------------------------------------------------------- the library without a GPU
def test_symbols_are_declared_exported_and_bound(lib):
    from ptranking_amd import _lib, functional
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptranking_amd.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        proto = re.search(name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert proto.count(",") + 1 == len(_lib.SIGNATURES[name]), name
        assert "is_cat" in proto and hasattr(lib, name)
        assert name[4:] in functional.__all__ and callable(getattr(functional, name[4:]))
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION == lib.ptr_abi_version()


def test_argument_errors_fire_before_any_launch(lib):
    one, two, f64 = C.c_void_p(64), C.c_void_p(128), C.c_double

    def err(rc, code, text):
        assert rc == code and text in lib.ptr_last_error(), (rc, lib.ptr_last_error())

    args = (f64(0.0), C.c_int64(1), f64(1e-3), f64(0.0), f64(10.0))

    def split(hist=one, L=2, F=3, mb=16, nbins=one, nan_bin=None, is_cat=one, expo=one, a=args, ws=one, rec=one, sets=one):
        return lib.ptr_gbdt_best_split_cat(hist, L, F, mb, nbins, nan_bin, is_cat, expo, *a, ws, rec, sets, None)
    for k in ("hist", "nbins", "is_cat", "expo", "ws", "rec", "sets"):
        err(split(**{k: None}), 1001, b"NULL")
    err(split(L=-2), 1001, b"negative")
    err(split(mb=1), 1001, b"max_bin")
    err(split(mb=257), 1002, b"max_bin")
    err(split(a=(f64(-1.0),) + args[1:]), 1001, b"lambda_l2")
    err(split(a=args[:2] + (f64(float("nan")),) + args[3:]), 1001, b"NaN")
    for bad in (-1.0, float("nan"), float("inf")):
        err(split(a=args[:4] + (f64(bad),)), 1001, b"cat_smooth")
    assert split(L=0, hist=None, nbins=None, is_cat=None, expo=None, ws=None, rec=None, sets=None) == 0

    def slots(pool=one, ns=4, sl=one, K=2, F=3, mb=16, nbins=one, nan_bin=None, is_cat=one, expo=one, a=args, ws=one, rec=one, sets=one):
        return lib.ptr_gbdt_best_split_slots_cat(pool, ns, sl, K, F, mb, nbins, nan_bin, is_cat, expo, *a, ws, rec, sets, None)
    for k in ("pool", "sl", "nbins", "is_cat", "expo", "ws", "rec", "sets"):
        err(slots(**{k: None}), 1001, b"NULL")
    err(slots(K=-1), 1001, b"K=-1")
    err(slots(mb=257), 1002, b"max_bin")
    err(slots(F=0), 1001, b"F must be >= 1")
    err(slots(ns=-1), 1001, b"nslots=-1")
    err(slots(a=args[:4] + (f64(-0.5),)), 1001, b"cat_smooth")
    assert slots(K=0, pool=None, sl=None, is_cat=None, sets=None) == 0

    def part(bins=one, stride=16, n=8, F=3, rows=one, m=4, feature=0, b=0, dl=0, is_cat=one, nan_bin=None, st=one, out=two, lc=one, ws=one):
        return lib.ptr_gbdt_partition_cat(bins, stride, n, F, rows, m, feature, b, dl, is_cat, nan_bin, st, out, lc, ws, None)
    for k in ("bins", "rows", "out", "ws", "is_cat", "st", "lc"):
        err(part(**{k: None}), 1001, b"NULL")
    err(part(m=-4), 1001, b"row count")
    err(part(feature=3), 1001, b"feature")
    err(part(b=256), 1001, b"bin")
    err(part(dl=2), 1001, b"default_left")
    err(part(stride=12), 1001, b"stride")

    def segs(bins=one, stride=16, n=8, F=3, rows=one, nrows=8, sg=one, sets=one, K=2, is_cat=one, nan_bin=None, blocks=one, nb=2, out=two, lc=one,
             ws=one, ws_ints=3):
        return lib.ptr_gbdt_partition_segments_cat(bins, stride, n, F, rows, nrows, sg, sets, K, is_cat, nan_bin, blocks, nb, out, lc, ws, ws_ints, None)
    for k in ("bins", "rows", "sg", "sets", "is_cat", "blocks", "out", "lc", "ws"):
        err(segs(**{k: None}), 1001, b"NULL")
    err(segs(K=-1), 1001, b"K=-1")
    err(segs(F=0), 1001, b"F must be >= 1")
    err(segs(stride=8), 1001, b"stride")
    err(segs(nb=-1), 1001, b"size")
    err(segs(out=one), 1001, b"out must not be rows")
    err(segs(ws_ints=2), 1001, b"workspace too small")

    def walk(scores=one, bins=one, stride=16, n=8, F=3, rows=one, m=8, feature=one, b=one, left=one, right=one, value=one, dl=None, is_cat=one,
             nan_bin=None, ci=one, cs=one, ncat=1, nn=3):
        return lib.ptr_gbdt_add_tree_binned_cat(scores, bins, stride, n, F, rows, m, feature, b, left, right, value, dl, is_cat, nan_bin, ci, cs, ncat, nn, None)
    for k in ("scores", "bins", "feature", "b", "left", "right", "value", "is_cat", "ci", "cs"):
        err(walk(**{k: None}), 1001, b"NULL")
    err(walk(stride=12), 1001, b"stride")
    err(walk(m=-1), 1001, b"m=-1")
    err(walk(nn=-1), 1001, b"nnodes=-1")
    err(walk(ncat=-1), 1001, b"ncat=-1")
    err(walk(rows=None, m=9), 1001, b"rows is NULL")
    assert walk(m=0, rows=None) == 0

    def pred(X=one, n=4, F=3, feature=one, thr=one, left=one, right=one, value=one, offs=one, dl=None, is_cat=one, ci=one, cs=one, ncat=1, nt=1, out=one):
        return lib.ptr_gbdt_predict_cat(X, n, F, feature, thr, left, right, value, offs, dl, is_cat, ci, cs, ncat, nt, out, None)
    for k in ("X", "out", "is_cat", "ci", "cs"):
        err(pred(**{k: None}), 1001, b"NULL")
    for k in ("feature", "thr", "left", "right", "value", "offs"):
        err(pred(**{k: None}), 1001, b"NULL tree")
    err(pred(n=-4), 1001, b"negative")
    err(pred(nt=-1), 1001, b"negative")
    err(pred(ncat=-1), 1001, b"ncat=-1")
    assert pred(n=0, X=None, out=None) == 0


def test_python_surface_refuses_to_run_without_a_gpu():
    import ptranking_amd as pa
    Fn = pa.functional
    f32, i32, u8, i64 = (lambda *s: torch.zeros(s, dtype=torch.float32)), (lambda *s: torch.zeros(s, dtype=torch.int32)), \
        (lambda *s: torch.zeros(s, dtype=torch.uint8)), (lambda *s: torch.zeros(s, dtype=torch.int64))
    calls = [lambda: Fn.gbdt_best_split_cat(i64(1, 3, 16, 3), i32(3), i32(2), u8(3)),
             lambda: Fn.gbdt_best_split_slots_cat(i64(2, 3, 16, 3), [0], i32(3), i32(2), u8(3)),
             lambda: Fn.gbdt_partition_cat(u8(4, 16), i32(2), 0, 0, 3, u8(3), i64(4)),
             lambda: Fn.gbdt_partition_segments_cat(u8(4, 16), i32(4), [[0, 4, 0, 0, 0]], i64(1, 4), 3, u8(3)),
             lambda: Fn.gbdt_add_tree_binned_cat(f32(4), u8(4, 16), 3, None, i32(1), i32(1), i32(1), i32(1), f32(2), u8(3), i32(1), i64(1, 4)),
             lambda: Fn.gbdt_predict_cat(f32(4, 3), i32(0), f32(0), i32(0), i32(0), f32(1), i32(2), u8(3), i32(0), i64(0, 4))]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pa.GBDT({"categorical_feature": [0]}, np.zeros((4, 2), np.float32))
