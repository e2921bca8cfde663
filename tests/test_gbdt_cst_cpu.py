"""CPU: monotone and interaction constraints in the native booster (monotone_constraints, monotone_constraints_method,
interaction_constraints).  The numpy restatement tests/gbdt_cst_ref.py reproduces scikit-learn's whole fits under monotonic_cst and
interaction_cst (tests/golden/gbdt_sklearn_cst.npz), the gate constant is measured here from the restatement alone, and one planted fault
per rule makes a comparison fail; the parameters and every refusal, the model file on host-built trees, and the argument errors of the two
new entry points, all without a GPU."""
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

import gbdt_cst_ref as TR
import gbdt_sk as SK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ptr_gbdt_best_split_cst", "ptr_gbdt_best_split_slots_cst")
CASES = ("a", "b", "c", "d", "e", "f", "g")
MONO_CASES = ("a", "b", "c", "d", "e", "g")


@pytest.fixture(autouse=True, scope="module")
def the_feature():
    """Every test of this module is about the constraints of the package: where it lacks them, none of them says anything."""
    from ptranking_amd import gbdt
    assert set(gbdt.CST_KEYS) <= set(gbdt.DEFAULT_PARAMS) and callable(gbdt.constraints)


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def fixture():
    return TR.load()


@functools.lru_cache(maxsize=None)
def unfaulted(name):
    return TR.compare_restatement(fixture()[0][name])


@functools.lru_cache(maxsize=None)
def restated(name):
    return TR.run_restatement(fixture()[0][name])


# ---------------------------------------------------------------- parameters
def test_parameter_defaults_and_validation():
    from ptranking_amd import gbdt
    p = gbdt._params(None)
    assert p["monotone_constraints"] == () and p["interaction_constraints"] == () and p["monotone_constraints_method"] == "basic"
    assert gbdt.constraints(p) == () and gbdt.constraints(gbdt._params({"monotone_constraints": [0, 0, 0], "interaction_constraints": []})) == ()
    assert gbdt._params({"monotone_constraints": None, "interaction_constraints": None})["monotone_constraints"] == ()
    p = gbdt._params({"monotone_constraints": [1, np.int8(-1), 0], "interaction_constraints": [[1, 0], (2,)]})
    assert p["monotone_constraints"] == (1, -1, 0) and p["interaction_constraints"] == ((0, 1), (2,))
    assert gbdt.constraints(p) == ("monotone", "interaction")
    assert gbdt.constraints(gbdt._params({"monotone_constraints": np.array([0, 1])})) == ("monotone",)
    assert gbdt.constraints(gbdt._params({"interaction_constraints": [{0, 1}, [1, 2]]})) == ("interaction",)
    for bad in ([2], [-2], [1.0], [True], ["1"], 1, "1,0", [[1]]):
        with pytest.raises(ValueError, match="monotone_constraints"):
            gbdt._params({"monotone_constraints": bad})
    for bad in ("intermediate", "advanced", None, 1):
        with pytest.raises(ValueError, match="monotone_constraints_method") as e:
            gbdt._params({"monotone_constraints_method": bad})
        assert repr(bad) in str(e.value)
    for bad in ([[]], [[0], []], [[-1]], [[0.5]], [[True]], [["0"]], [0, 1], 3, "0,1"):
        with pytest.raises(ValueError, match="interaction_constraints"):
            gbdt._params({"interaction_constraints": bad})
    with pytest.raises(ValueError, match="categorical"):
        gbdt._params({"monotone_constraints": [0, 1], "categorical_feature": [1]})
    gbdt._params({"monotone_constraints": [0, 1], "categorical_feature": [0]})          # constraint 0 on the categorical column: fine
    with pytest.raises(ValueError, match="unknown parameter"):
        gbdt._params({"monotone_penalty": 0.0})
    doc = gbdt.__doc__
    assert "monotone_penalty" in doc and "'intermediate'" in doc and "interaction_constraints" in doc
    tail = doc[doc.rindex("Not here:"):]
    assert "monotone constraints" not in tail and all(w in tail for w in ("feature_fraction", "EFB", "DART"))
    json.dumps(p)                                                        # a model file carries the parameters as JSON


def test_column_refusals_come_before_any_device_work():
    """The length of monotone_constraints and the range of interaction_constraints are checked against X in fit_bins, ahead of the device:
    they are ValueErrors with or without a GPU."""
    from ptranking_amd import gbdt
    X = np.zeros((8, 3), np.float32)
    with pytest.raises(ValueError, match="monotone_constraints holds 2 entries"):
        gbdt.GBDT({"monotone_constraints": [1, 0]}).fit_bins(X)
    with pytest.raises(ValueError, match="monotone_constraints holds 4 entries"):
        gbdt.GBDT({"monotone_constraints": [0, 0, 0, 0]}).fit_bins(X)
    with pytest.raises(ValueError, match="interaction_constraints 3 with 3 columns"):
        gbdt.GBDT({"interaction_constraints": [[0, 3]]}).fit_bins(X)
    groups = gbdt._interaction_groups(gbdt._params({"interaction_constraints": [[0, 1], [2, 3]]}), 5)
    assert groups == [frozenset({0, 1}), frozenset({2, 3}), frozenset({4})]           # the unlisted feature forms one more group
    assert gbdt._interaction_groups(gbdt._params({"interaction_constraints": [[0, 1], [1, 2]]}), 3) == [frozenset({0, 1}), frozenset({1, 2})]


# ---------------------------------------------------------------- the restatement against scikit-learn
def test_fixture_cases_are_the_ones_the_issue_asks_for():
    cases, version = fixture()
    assert tuple(sorted(cases)) == CASES and version
    for name, c in cases.items():
        assert c["X"].shape == (600, 5) and c["params"]["rounds"] <= 6, name
        num = c["X"][:, c["params"]["ncat"]:]
        assert np.nanmax(num) <= 23 / 8 and np.array_equal(np.nan_to_num(num * 8), np.floor(np.nan_to_num(num * 8)))
        assert (name in MONO_CASES) == bool(np.any(c["mono"])) == ("sweep" in c)
    a, b, c, d, e, f, g = (cases[k] for k in CASES)
    for x in (a, b):
        assert set(x["mono"].tolist()) == {1, -1, 0} and not x["groups"]
        assert all(lv.shape[0] == x["params"]["num_leaves"] for lv in x["leaves"])       # the cap binds in every round
    assert a["w"] is None and a["params"]["lambda_l2"] == 0.0 and b["w"] is not None and b["params"]["lambda_l2"] > 0.0
    assert c["params"]["depthwise"] and c["params"]["max_depth"] == 4 and c["params"]["num_leaves"] == 16
    assert d["params"]["use_missing"] and d["nan"][:, 0].any() and d["mono"][0] != 0
    assert e["params"]["ncat"] == 1 and e["mono"][0] == 0 and np.any(e["mono"][1:]) and (np.concatenate(e["nodes"])[:, 1] > 0).any()
    assert f["groups"] == [[0, 1], [2, 3]] and not np.any(f["mono"]) and f["X"].shape[1] == 5
    assert g["groups"] and np.any(g["mono"])
    assert os.path.getsize(TR.FILE) < 256 * 1024


def test_sklearn_itself_is_monotone_only_under_the_constraint():
    """The stored sweep of case a: scikit-learn's unconstrained fit steps the wrong way, its constrained fit never does."""
    a = fixture()[0]["a"]
    step = lambda pred: min(float((np.diff(pred[a["sweep_block"] == b]) * a["mono"][a["sweep_feature"][a["sweep_block"] == b][0]]).min())
                            for b in np.unique(a["sweep_block"]))
    print(f"MEASURED sklearn sweep steps, case a: unconstrained {step(a['sweep_free']):.3f}, constrained {step(a['sweep_pred'])}")
    assert step(a["sweep_free"]) < 0.0 and step(a["sweep_pred"]) >= 0.0


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_sklearn(name):
    """Nodes, leaf row counts, leaf values, staged and fresh predictions; the margin held when the archive was written and holds now."""
    miss, need, leaf_need, margin = unfaulted(name)
    print(f"MEASURED gbdt constrained restatement vs sklearn, case {name}: predictions need C >= {need:.2f}, leaf values {leaf_need:.2f}, margin {margin:.2e}")
    assert miss is None, miss
    assert margin >= SK.MIN_MARGIN
    assert need <= TR.C_GBDT_SK_CST and leaf_need <= TR.C_GBDT_SK_CST


def test_gate_constant_is_twice_the_restatements_need():
    worst = max(unfaulted(name)[1] for name in CASES)
    print(f"MEASURED gbdt constrained restatement vs sklearn: worst need {worst:.2f} (recorded {TR.NEED_RECORDED})")
    assert abs(worst - TR.NEED_RECORDED) < 0.01
    assert TR.C_GBDT_SK_CST == math.ceil(2 * TR.NEED_RECORDED)


@pytest.mark.parametrize("name", MONO_CASES)
def test_the_constraints_bind_in_every_monotone_case(name):
    """A rejection decides at least one search, and at least one stored leaf value is a clamped one."""
    stats = restated(name)[3]
    assert sum(s["changed"] for s in stats) > 0 and sum(s["clamped"] for s in stats) > 0


def test_restated_sweeps_are_monotone_and_paths_stay_in_a_group():
    cases = fixture()[0]
    for name in MONO_CASES:
        c = cases[name]
        pred = TR.CR.predict(c["sweep"], [t for t, _ in restated(name)[0]])
        for b in np.unique(c["sweep_block"]):
            sel = c["sweep_block"] == b
            assert (np.diff(pred[sel].astype(np.float64)) * c["mono"][c["sweep_feature"][sel][0]] >= 0).all(), (name, b)
    for name in ("f", "g"):
        c = cases[name]
        assert all(not TR.forbidden_pairs(TR.tree_paths(t), c["groups"], 5) for t, _ in restated(name)[0])
    free = TR.run_restatement(cases["f"], groups=None)[0]
    assert any(TR.forbidden_pairs(TR.tree_paths(t), cases["f"]["groups"], 5) for t, _ in free)       # without the constraint a forbidden pair appears


@pytest.mark.parametrize("fault,name", [("no_clamp", "a"), ("no_clamp", "d"), ("mid_unclamped", "a"), ("mid_unclamped", "c"), ("swapped_neg", "a"),
                                        ("swapped_neg", "g"), ("inherit_all_groups", "f"), ("inherit_all_groups", "g")])
def test_planted_faults_are_caught(fault, name):
    assert fault in TR.FAULTS
    miss = TR.compare_restatement(fixture()[0][name], fault)[0]
    print(f"fault {fault} on case {name}: {miss}")
    assert miss is not None


def test_the_rule_on_a_hand_made_node():
    """One feature, four bins of unit Hessians with gradients that make the unconstrained best split put the larger value on the left."""
    ONE, expo = 1 << 10, (10, 10)
    hist = np.zeros((1, 8, 3), np.int64)
    for b, (g, n) in enumerate([(-6, 2), (-2, 2), (6, 2), (1, 2)]):      # bin values -g / n: 3, 1, -3, -0.5
        hist[0, b] = (g * ONE, n * ONE, n)
    nb, cat = np.array([4]), np.array([0])
    v = TR.node_value(hist[0, :, 0].sum(), hist[0, :, 1].sum(), expo, 0.0)
    inf = (-np.inf, np.inf, v)
    free = TR.best_split(hist, nb, None, cat, expo, mono=np.array([0]), cst=inf)
    assert free["bin"] == 1 and free["vl"] == 2.0 and free["vr"] == -1.75 and not free["changed"]
    assert free["gain"] == ((-1 * v) - (-8 * 2.0)) - (7 * -1.75)       # ((G v) - (GL vL)) - (GR vR)
    up = TR.best_split(hist, nb, None, cat, expo, mono=np.array([1]), cst=inf)
    assert up["feature"] == -1 and not up["gain"] > -np.inf             # every candidate has vL > vR: the record without a split
    down = TR.best_split(hist, nb, None, cat, expo, mono=np.array([-1]), cst=inf)
    assert down["bin"] == 1 and down["gain"] == free["gain"]
    clamp = TR.best_split(hist, nb, None, cat, expo, mono=np.array([-1]), cst=(-1.0, 1.5, v))
    assert clamp["bin"] == 1 and clamp["vl"] == 1.5 and clamp["vr"] == -1.0
    left, right = TR.child_cst((-1.0, 1.5, v), -1, clamp["vl"], clamp["vr"], clamp["left"], hist[0].sum(axis=0), expo, 0.0)
    assert left == (0.25, 1.5, 1.5) and right == (-1.0, 0.25, -1.0)       # under -1 the left child sits above mid
    left, right = TR.child_cst((-1.0, 1.5, v), 1, 0.5, 1.0, clamp["left"], hist[0].sum(axis=0), expo, 0.0)
    assert left == (-1.0, 0.75, 0.5) and right == (0.75, 1.5, 1.0)
    flat = TR.best_split(hist, nb, None, cat, expo, mono=np.array([1]), cst=(0.5, 0.5, 0.5))
    assert flat["feature"] == 0 and flat["vl"] == flat["vr"] == 0.5       # lo == hi: vL == vR passes either order test
    assert TR.best_split(hist, nb, None, cat, expo, mono=np.array([0]), cst=(1.0, 0.0, v))["feature"] == -1       # lo > hi
    assert TR.best_split(hist, nb, None, cat, expo, mono=np.array([0]), cst=(np.nan, 0.0, v))["feature"] == -1
    assert TR.best_split(hist, nb, None, cat, expo, allowed=np.array([False]))["feature"] == -1
    only = TR.best_split(hist, nb, None, cat, expo, allowed=np.array([True]))
    base = TR.CR.best_split(hist, nb, None, cat, expo)
    assert np.array_equal(TR.record(only, False)[0], TR.CR.record(base, False)[0])       # interaction constraints alone: today's record


# ---------------------------------------------------------------- the model file on the host
def host_booster(params):
    from ptranking_amd import gbdt
    b = gbdt.GBDT(params)
    b.edges = np.full((3, 7), np.inf, np.float32)
    b.edges[0, :4] = np.arange(4) + np.float32(0.5)
    b.edges[1, :3] = [0.25, 0.5, 1.0]
    b.nbins = np.array([5, 4, 1], np.int32)
    if b.params["use_missing"]:
        b.nan_bin = np.array([5, -1, -1], np.int32)
    t0 = {"feature": np.array([0, 1], np.int32), "threshold": np.array([0.5, 0.5], np.float32), "left": np.array([1, ~0], np.int32),
          "right": np.array([~2, ~1], np.int32), "value": np.array([1, 2, 3], np.float32)}
    if b.params["use_missing"]:
        t0["default_left"] = np.array([0, 1], np.uint8)
    b.trees = [t0]
    return b


def members(path):
    with zipfile.ZipFile(path) as z:
        return [(i.filename, z.read(i.filename)) for i in z.infolist()]


@pytest.mark.parametrize("missing", [False, True])
def test_the_keys_round_trip_in_the_model_file(tmp_path, missing):
    from ptranking_amd import gbdt
    for k, extra in enumerate(({"monotone_constraints": [1, 0, -1]}, {"interaction_constraints": [[0, 1], [2]]},
                               {"monotone_constraints": [0, -1, 0], "interaction_constraints": [[1, 2]]})):
        b = host_booster(dict({"max_bin": 8, "use_missing": missing}, **extra))
        path = tmp_path / f"{k}.npz"
        b.save_model(path)
        with np.load(path, allow_pickle=False) as z:
            params = json.loads(str(z["params"]))
            assert int(z["format"]) == (2 if missing else 1) and set(gbdt.CST_KEYS) <= set(params)       # the format numbers do not change
        back = gbdt.GBDT.load_model(path)
        assert back.params == b.params and gbdt.constraints(back.params) == gbdt.constraints(b.params) != ()
        assert all(np.array_equal(v, back.flat()[key]) for key, v in b.flat().items())


@pytest.mark.parametrize("missing", [False, True])
def test_inactive_constraints_keep_the_bytes_and_older_files_load(tmp_path, missing):
    """With every constraint 0 and no group the file is the one written before the keys existed: they are not among its parameters; and
    such a file (a file of any age) loads with the defaults."""
    from ptranking_amd import gbdt
    files = []
    for k, extra in enumerate(({}, {"monotone_constraints": [0, 0, 0], "interaction_constraints": [], "monotone_constraints_method": "basic"})):
        host_booster(dict({"max_bin": 8, "use_missing": missing}, **extra)).save_model(tmp_path / f"{k}.npz")
        files.append(members(tmp_path / f"{k}.npz"))
    assert files[0] == files[1]
    with np.load(tmp_path / "1.npz", allow_pickle=False) as z:
        assert not set(json.loads(str(z["params"]))) & set(gbdt.CST_KEYS)
    back = gbdt.GBDT.load_model(tmp_path / "1.npz")
    assert back.params["monotone_constraints"] == () and back.params["interaction_constraints"] == () and back.params["monotone_constraints_method"] == "basic"


# ---------------------------------------------------------------- the library without a GPU
def test_symbols_are_declared_exported_and_bound(lib):
    from ptranking_amd import _lib, functional
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptranking_amd.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        proto = re.search(name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert proto.count(",") + 1 == len(_lib.SIGNATURES[name]) == len(_lib.SIGNATURES[name.replace("_cst", "_cat")]) + 3, name
        assert all(w in proto for w in ("is_cat", "mono", "cst", "allowed")) and hasattr(lib, name)
        assert name[4:] in functional.__all__ and callable(getattr(functional, name[4:]))
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION == lib.ptr_abi_version()


def test_argument_errors_fire_before_any_launch(lib):
    one, f64 = C.c_void_p(64), C.c_double

    def err(rc, code, text):
        assert rc == code and text in lib.ptr_last_error(), (rc, lib.ptr_last_error())

    args = (f64(0.0), C.c_int64(1), f64(1e-3), f64(0.0), f64(10.0))

    def split(hist=one, L=2, F=3, mb=16, nbins=one, nan_bin=None, is_cat=one, expo=one, a=args, ws=one, rec=one, sets=one, mono=one, cst=one, allowed=one):
        return lib.ptr_gbdt_best_split_cst(hist, L, F, mb, nbins, nan_bin, is_cat, expo, *a, ws, rec, sets, mono, cst, allowed, None)
    for k in ("hist", "nbins", "expo", "ws", "rec", "sets", "mono"):
        err(split(**{k: None}), 1001, b"NULL")
    err(split(cst=None, allowed=None), 1001, b"neither cst nor allowed")
    err(split(L=-2), 1001, b"negative")
    err(split(mb=1), 1001, b"max_bin")
    err(split(mb=257), 1002, b"max_bin")
    err(split(a=(f64(-1.0),) + args[1:]), 1001, b"lambda_l2")
    err(split(a=args[:2] + (f64(float("nan")),) + args[3:]), 1001, b"NaN")
    err(split(a=args[:4] + (f64(-1.0),)), 1001, b"cat_smooth")
    assert split(L=0, hist=None, nbins=None, is_cat=None, expo=None, ws=None, rec=None, sets=None, mono=None, cst=None, allowed=None) == 0

    def slots(pool=one, ns=4, sl=one, K=2, F=3, mb=16, nbins=one, nan_bin=None, is_cat=one, expo=one, a=args, ws=one, rec=one, sets=one, mono=one, cst=one,
              allowed=one):
        return lib.ptr_gbdt_best_split_slots_cst(pool, ns, sl, K, F, mb, nbins, nan_bin, is_cat, expo, *a, ws, rec, sets, mono, cst, allowed, None)
    for k in ("pool", "sl", "nbins", "expo", "ws", "rec", "sets", "mono"):
        err(slots(**{k: None}), 1001, b"NULL")
    err(slots(cst=None, allowed=None), 1001, b"neither cst nor allowed")
    err(slots(K=-1), 1001, b"K=-1")
    err(slots(mb=257), 1002, b"max_bin")
    err(slots(F=0), 1001, b"F must be >= 1")
    err(slots(ns=-1), 1001, b"nslots=-1")
    assert slots(K=0, pool=None, sl=None, is_cat=None, sets=None, mono=None, cst=None, allowed=None) == 0


def test_python_surface_refuses_to_run_without_a_gpu():
    import ptranking_amd as pa
    Fn = pa.functional
    i32, u8, i64 = (lambda *s: torch.zeros(s, dtype=torch.int32)), (lambda *s: torch.zeros(s, dtype=torch.uint8)), (lambda *s: torch.zeros(s, dtype=torch.int64))
    i8, f64 = (lambda *s: torch.zeros(s, dtype=torch.int8)), (lambda *s: torch.zeros(s, dtype=torch.float64))
    for call in (lambda: Fn.gbdt_best_split_cst(i64(1, 3, 16, 3), i32(3), i32(2), i8(3), f64(1, 3), u8(1, 3)),
                 lambda: Fn.gbdt_best_split_slots_cst(i64(2, 3, 16, 3), [0], i32(3), i32(2), None, None, u8(1, 3), is_cat=u8(3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call in (lambda: Fn.gbdt_best_split_cst(i64(1, 3, 16, 3), i32(3), i32(2)),
                 lambda: Fn.gbdt_best_split_cst(i64(1, 3, 16, 3), i32(3), i32(2), None, f64(1, 3)),
                 lambda: Fn.gbdt_best_split_slots_cst(i64(2, 3, 16, 3), [0], i32(3), i32(2), i8(3), f64(1, 3), sets=i64(1, 4))):
        with pytest.raises((ValueError, RuntimeError)):
            call()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pa.GBDT({"monotone_constraints": [1, 0]}, np.zeros((4, 2), np.float32))
