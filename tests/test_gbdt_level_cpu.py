"""CPU: depth-wise growth of the native booster (grow_policy='depthwise').  The numpy restatement tests/gbdt_level_ref.py equals the
leaf-wise restatement wherever the leaf cap cannot bind, reproduces scikit-learn's depth-limited trees (tests/golden/gbdt_sklearn_depth.npz),
follows the cap rule where it binds, and every planted fault makes its comparison fail.  The four batched entry points are declared,
exported and bound, every argument error fires before a launch, and the Python surface refuses to run without a GPU."""
import ctypes as C
import functools
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

import gbdt_level_ref as LR
import gbdt_ref as R
import gbdt_sk as SK
from launch_form import launch_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ptr_gbdt_histogram_segments", "ptr_gbdt_hist_sub_segments", "ptr_gbdt_best_split_slots", "ptr_gbdt_partition_segments_ws_ints",
                "ptr_gbdt_partition_segments")
WRAPPERS = ("gbdt_histogram_segments", "gbdt_hist_sub_segments", "gbdt_best_split_slots", "gbdt_partition_segments")
DEPTH_NAMES = ("g", "h", "i", "j")


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def fixtures():
    return SK.load()[0], LR.load()[0]


def cap_cannot_bind(case):
    p = case["params"]
    return (p["max_depth"] > 0 and p["num_leaves"] >= 2 ** p["max_depth"]) or p["num_leaves"] >= case["X"].shape[0]


# ---------------------------------------------------------------- the equivalence, and scikit-learn
def test_fixture_cases_are_the_ones_the_generator_lists():
    leafwise, depth = fixtures()
    assert tuple(sorted(depth)) == DEPTH_NAMES
    shapes = {n: (c["X"].shape, c["params"]["max_bin"], c["params"]["max_depth"], c["params"]["rounds"]) for n, c in depth.items()}
    assert shapes == {"g": ((600, 7), 63, 3, 5), "h": ((1500, 17), 255, 5, 4), "i": ((900, 33), 64, 4, 3), "j": ((257, 1), 16, 2, 2)}
    assert all(cap_cannot_bind(c) for c in depth.values()) and depth["i"]["w"] is not None
    assert [n for n, c in leafwise.items() if cap_cannot_bind(c)] == ["d"]              # the leaf-wise fixture's one depth-limited case
    assert os.path.getsize(LR.FILE) < 200 * 1024


@pytest.mark.parametrize("name", ("d",) + DEPTH_NAMES)
def test_depthwise_equals_leafwise_where_the_cap_cannot_bind(name):
    """Both policies split the same set of leaves from the same integer histograms: the same trees in canonical form, bit-equal fp32 leaf
    values and training scores, bit-equal fresh predictions."""
    leafwise, depth = fixtures()
    case = leafwise[name] if name in leafwise else depth[name]
    assert cap_cannot_bind(case)
    a, fresh_a, _ = LR.run_restatement(case, "leafwise")
    b, fresh_b, _ = LR.run_restatement(case, "depthwise")
    assert LR.same_trees(a, b, case["X"])
    assert np.array_equal(fresh_a.view(np.int32), fresh_b.view(np.int32))


@pytest.mark.parametrize("name", DEPTH_NAMES)
def test_depthwise_restatement_reproduces_sklearn(name):
    """HistGradientBoostingRegressor(max_leaf_nodes=None, max_depth=d): every tree node for node, every prediction within gbdt_sk's gate."""
    case = fixtures()[1][name]
    miss, need, leaf_need, margin = LR.compare_restatement(case)
    print(f"MEASURED depth-wise restatement vs sklearn, case {name}: predictions need C >= {need:.2f}, leaf values {leaf_need:.2f}, margin {margin:.2e}")
    assert miss is None and margin >= SK.MIN_MARGIN and need <= SK.C_GBDT_SK
    if name == "h":
        leaves = [int(t.shape[0]) for t in case["leaves"]]
        assert all(l < 32 for l in leaves) and min(leaves) >= 16                         # ragged levels: some leaves stop early


# ---------------------------------------------------------------- the cap rule
@functools.lru_cache(maxsize=None)
def cap_case():
    """3000 rows, num_leaves 20, no depth limit: 16 leaves after four full levels, so the fifth level has budget 4 for up to 16 candidates."""
    rng = np.random.default_rng(11)
    n, nf, max_bin = 3000, 6, 32
    X = rng.integers(0, 24, (n, nf)).astype(np.float32)
    y = (X[:, 0] * 0.3 + (X[:, 1] > 11) * 2.0 - X[:, 2] * X[:, 0] * 0.02 + np.sin(X[:, 3]) + 0.3 * rng.standard_normal(n)).astype(np.float32)
    edges, nbins = R.bin_edges(X, max_bin)
    bins = R.bin_matrix(X, edges, nbins)
    qg, qh, expo, _ = R.quantize(-y, np.ones(n, np.float32))
    return X, bins, qg, qh, expo, edges, nbins, max_bin


def grow_cap(fault=None, num_leaves=20):
    X, bins, qg, qh, expo, edges, nbins, max_bin = cap_case()
    return LR.grow_tree(bins, qg, qh, expo, edges, nbins, max_bin, num_leaves, lr=0.5, min_data=20, fault=fault)


def test_the_cap_keeps_the_largest_gains_of_the_last_level():
    X, bins, qg, qh, expo, edges, nbins, max_bin = cap_case()
    tree, leaf_rows, margin, levels = grow_cap()
    assert tree["value"].size == 20 == len(leaf_rows) and tree["feature"].size == 19
    assert sorted(np.concatenate(leaf_rows).tolist()) == list(range(3000))
    assert [len(l["kept"]) for l in levels] == [1, 2, 4, 8, 4]
    last = levels[-1]
    assert len(last["candidates"]) > 4
    gains = sorted((g for g, _ in last["candidates"]), reverse=True)
    assert sorted((g for g, _ in last["kept"]), reverse=True) == gains[:4] and gains[3] > gains[4]
    assert [s for _, s in last["kept"]] == sorted(s for _, s in last["kept"])            # numbered in row order
    assert last["searched"] == 0                                                         # a full tree searches no more
    # a policy, not a reordering: the leaf-wise tree of the same data differs
    lw, _, _ = R.grow_tree(bins, qg, qh, expo, edges, nbins, max_bin, 20, lr=0.5, min_data=20)
    a, b = SK.canonical(tree, X), SK.canonical(lw, X)
    assert lw["value"].size == 20 and not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    # with the cap out of the way the two agree again
    free, free_rows, _, _ = grow_cap(num_leaves=4000)
    lw_free, lw_rows, _ = R.grow_tree(bins, qg, qh, expo, edges, nbins, max_bin, 4000, lr=0.5, min_data=20)
    a, b = SK.canonical(free, X), SK.canonical(lw_free, X)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and free["value"].size > 20
    scores = lambda rows, t: R.add_leaf_values(np.zeros(3000, np.float32), rows, t["value"])
    assert np.array_equal(scores(free_rows, free).view(np.int32), scores(lw_rows, lw_free).view(np.int32))


def test_ties_at_the_cap_go_to_the_smaller_start():
    """Two identical halves: every candidate of the right half ties with its twin on the left; the cap takes the left one."""
    rng = np.random.default_rng(5)
    half = rng.integers(0, 8, (200, 3)).astype(np.uint8)
    yh = rng.integers(-40, 40, 200)
    side = np.repeat([0, 7], 200).astype(np.uint8)
    bins = np.concatenate([np.concatenate([half, half]), side[:, None]], axis=1)
    qg = np.concatenate([yh, yh]).astype(np.int32) * 1024 + np.repeat([-2 ** 20, 2 ** 20], 200).astype(np.int32)
    qh = np.full(400, 1 << 20, np.int32)
    nbins = np.full(4, 8, np.int32)
    edges = np.tile(np.arange(7, dtype=np.float32) + 0.5, (4, 1))
    tree, leaf_rows, _, levels = LR.grow_tree(bins, qg, qh, (10, 20), edges, nbins, 8, 3, min_data=5)
    assert tree["feature"][0] == 3 and len(levels) == 2
    (g0, s0), (g1, s1) = levels[1]["candidates"]
    assert g0 == g1 and (s0, s1) == (0, 200) and levels[1]["kept"] == [(g0, 0)]


# ---------------------------------------------------------------- planted faults
def test_planted_faults_fail_their_comparisons():
    X = cap_case()[0]
    good = grow_cap()
    canon = lambda t: SK.canonical(t, X)
    same = lambda t: all(np.array_equal(u, v) for u, v in zip(canon(good[0]), canon(t)))
    assert same(grow_cap()[0])
    assert not same(grow_cap("cap_smallest")[0])                                         # only visible where the cap binds
    # "refused_frontier" cannot fail a comparison, and that is a fact about the policy worth pinning: the cap binds only when the
    # candidates outnumber the budget, the kept ones then use the budget up, and a full tree has no further level for a refused leaf to
    # come back in.  "Stay leaves for good" follows from the cap rule; it is not a second rule.
    refused = grow_cap("refused_frontier")
    assert same(refused[0]) and len(refused[3]) == len(good[3]) and refused[0]["value"].size == 20
    depth = fixtures()[1]
    for fault in ("neighbour_split", "larger_hist"):                                     # visible against sklearn's trees
        miss = [LR.compare_restatement(depth[name], fault)[0] for name in ("g", "h")]
        assert all(m is not None for m in miss), (fault, miss)
    assert set(LR.FAULTS) == {"cap_smallest", "refused_frontier", "neighbour_split", "larger_hist"}


# ---------------------------------------------------------------- the library without a GPU
def test_symbols_are_declared_exported_and_bound(lib):
    from ptranking_amd import _lib
    import ptranking_amd as pa
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptranking_amd.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        proto = re.search(name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert proto.count(",") + 1 == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name)
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION == lib.ptr_abi_version()
    for name in WRAPPERS:
        assert name in pa.functional.__all__ and callable(getattr(pa.functional, name)) and not name.endswith("_loss")


def test_argument_errors_fire_before_any_launch(lib):
    one, f64 = C.c_void_p(64), C.c_double

    def err(rc, code, text):
        assert rc == code and text in lib.ptr_last_error(), (rc, lib.ptr_last_error())

    def hist(bins=one, stride=16, n=8, qg=one, qh=one, rows=one, nrows=8, segs=one, K=2, items=one, nd=1, nl=1, F=3, mb=16, pool=one, slots=4):
        return lib.ptr_gbdt_histogram_segments(bins, stride, n, qg, qh, rows, nrows, segs, K, items, nd, nl, F, mb, pool, slots, None)
    for k in ("bins", "qg", "qh", "rows", "segs", "items", "pool"):
        err(hist(**{k: None}), 1001, b"NULL")
    err(hist(K=-1), 1001, b"K=-1")
    err(hist(mb=1), 1001, b"max_bin")
    err(hist(mb=257), 1002, b"max_bin")
    err(hist(F=0), 1001, b"F must be >= 1")
    err(hist(stride=12), 1001, b"stride")
    err(hist(F=20), 1001, b"stride")
    err(hist(bins=C.c_void_p(72)), 1001, b"aligned")
    err(hist(nd=-1), 1001, b"size")
    err(hist(nrows=-1), 1001, b"size")
    assert hist(K=0, segs=None, items=None) == 0 and hist(nd=0, nl=0, items=None) == 0   # nothing to do

    def sub(pool=one, slots=4, F=3, mb=16, trips=one, K=2):
        return lib.ptr_gbdt_hist_sub_segments(pool, slots, F, mb, trips, K, None)
    err(sub(pool=None), 1001, b"NULL")
    err(sub(trips=None), 1001, b"NULL")
    err(sub(K=-2), 1001, b"K=-2")
    err(sub(mb=1), 1001, b"max_bin")
    err(sub(mb=300), 1002, b"max_bin")
    err(sub(F=0), 1001, b"F must be >= 1")
    assert sub(K=0, trips=None) == 0

    args = (f64(0.0), C.c_int64(1), f64(1e-3), f64(0.0))

    def split(pool=one, slots=4, sl=one, K=2, F=3, mb=16, nbins=one, expo=one, a=args, ws=one, rec=one):
        return lib.ptr_gbdt_best_split_slots(pool, slots, sl, K, F, mb, nbins, expo, *a, ws, rec, None)
    for k in ("pool", "sl", "nbins", "expo", "ws", "rec"):
        err(split(**{k: None}), 1001, b"NULL")
    err(split(K=-1), 1001, b"K=-1")
    err(split(mb=1), 1001, b"max_bin")
    err(split(mb=257), 1002, b"max_bin")
    err(split(F=0), 1001, b"F must be >= 1")
    err(split(a=(f64(-1.0), C.c_int64(1), f64(1e-3), f64(0.0))), 1001, b"lambda_l2")
    err(split(a=(f64(0.0), C.c_int64(1), f64(float("nan")), f64(0.0))), 1001, b"NaN")
    assert split(K=0, sl=None, ws=None, rec=None) == 0

    def part(bins=one, stride=16, n=8, F=3, rows=one, nrows=8, segs=one, K=2, blocks=one, nb=2, out=C.c_void_p(128), lc=one, ws=one, ws_ints=3):
        return lib.ptr_gbdt_partition_segments(bins, stride, n, F, rows, nrows, segs, K, blocks, nb, out, lc, ws, ws_ints, None)
    for k in ("bins", "rows", "segs", "blocks", "out", "lc", "ws"):
        err(part(**{k: None}), 1001, b"NULL")
    err(part(K=-1), 1001, b"K=-1")
    err(part(F=0), 1001, b"F must be >= 1")
    err(part(stride=8), 1001, b"stride")
    err(part(nb=-1), 1001, b"size")
    err(part(out=one), 1001, b"out must not be rows")
    err(part(ws_ints=2), 1001, b"workspace too small")
    assert lib.ptr_gbdt_partition_segments_ws_ints(0) == 1 and lib.ptr_gbdt_partition_segments_ws_ints(7) == 8
    assert part(K=0, nrows=0, segs=None, blocks=None, nb=0) == 0


def test_launch_forms_of_the_batched_entry_points(lib):
    form = lambda m, nf=136, mb=255, total=0: launch_form("ptr_gbdt_histogram_segments", m, nf, mb, total)
    assert form(0)[0] == 0 and form(1)[0] == 1 and form(256)[:3] == (1, 16, 9) and form(257)[:5] == (2, 16, 9, 1, 16 * 255 * 20)
    assert form(257)[5:8] == (2048, 256, 2)                                              # rows per chunk, the direct bound, launches per call
    assert form(2049)[3] == 2 and form(5000, 17, 256)[2:5] == (2, 3, 16 * 256 * 20) and 16 * 256 * 20 <= 160 * 1024 // 2
    for m in (1, 255, 256, 257, 2048, 2049, 5000, 70000):                                # the form by m alone is ptr_gbdt_histogram's
        assert form(m)[0] == launch_form("ptr_gbdt_histogram", m, 136, 255)[0]
    big = form(1_140_000, 136, 255, 1_140_000)                                           # a level of the large shape: about 1024 workgroups
    assert big[5] % 256 == 0 and big[5] >= 2048 and big[3] * big[2] <= 1024 + big[2]
    assert launch_form("ptr_gbdt_hist_sub_segments", 64)[0] == 1 and launch_form("ptr_gbdt_best_split_slots", 64)[0] == 2
    assert launch_form("ptr_gbdt_partition_segments", 1024)[:2] == (3, 1) and launch_form("ptr_gbdt_partition_segments", 1025)[:2] == (3, 2)
    a, out = (C.c_int64 * 4)(1000, 136, 255, 0), (C.c_int32 * 8)()
    assert lib.ptr_launch_form(b"ptr_gbdt_histogram_segments", a, 3, out, 8) == 1001 and b"takes 4" in lib.ptr_last_error()
    assert lib.ptr_launch_form(b"ptr_gbdt_histogram", a, 3, out, 8) == 0                 # the existing arity stays


def test_segment_items_cover_every_row_once(lib):
    from ptranking_amd import functional as Fn
    counts = np.array([0, 1, 255, 256, 257, 2048, 2049, 5000, 0, 300])
    items, nd, nl = Fn.gbdt_segment_items(counts, 17, 255)
    assert nd == 3 and items[:nd, 0].tolist() == [1, 2, 3] and (items[:nd, 2] <= 256).all()
    assert nl == 1 + 1 + 2 + 3 + 1 and set(items[nd:, 0].tolist()) == {4, 5, 6, 7, 9}
    covered = np.zeros((counts.size, 5000), np.int64)
    for k, begin, rows in items:
        covered[k, begin:begin + rows] += 1
    assert all((covered[k, :c] == 1).all() and not covered[k, c:].any() for k, c in enumerate(counts))
    assert Fn.gbdt_segment_items([], 17, 255)[1:] == (0, 0)


def test_python_surface_refuses_to_run_without_a_gpu():
    import ptranking_amd as pa
    Fn = pa.functional
    i32, u8, i64 = (lambda *s: torch.zeros(s, dtype=torch.int32)), (lambda *s: torch.zeros(s, dtype=torch.uint8)), (lambda *s: torch.zeros(s, dtype=torch.int64))
    calls = {"gbdt_histogram_segments": lambda: Fn.gbdt_histogram_segments(u8(4, 16), i32(4), i32(4), i32(4), [[0, 2, 0]], 3, 16, i64(2, 3, 16, 3)),
             "gbdt_hist_sub_segments": lambda: Fn.gbdt_hist_sub_segments(i64(2, 3, 16, 3), [[0, 1, 0]]),
             "gbdt_best_split_slots": lambda: Fn.gbdt_best_split_slots(i64(2, 3, 16, 3), [0], i32(3), i32(2)),
             "gbdt_partition_segments": lambda: Fn.gbdt_partition_segments(u8(4, 16), i32(4), [[0, 4, 0, 0]], 3)}
    assert set(calls) == set(WRAPPERS)
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pa.GBDT({"grow_policy": "depthwise"}, X=np.zeros((4, 3), np.float32))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pa.LambdaMART({"grow_policy": "depthwise"})


# ---------------------------------------------------------------- the parameter
def test_grow_policy_parameter(tmp_path):
    from ptranking_amd import gbdt
    assert gbdt.DEFAULT_PARAMS["grow_policy"] == "leafwise" and gbdt.GBDT().params["grow_policy"] == "leafwise"
    assert "grow_policy" not in gbdt.IGNORED_PARAMS and gbdt.MODEL_FORMAT == 1
    assert gbdt.GBDT({"grow_policy": "depthwise"}).params["grow_policy"] == "depthwise"
    assert gbdt.GBDT().host_reads == 0
    for bad in ("lossguide", "Depthwise", None):
        with pytest.raises(ValueError, match="'leafwise' and 'depthwise'"):
            gbdt.GBDT({"grow_policy": bad})
    with pytest.raises(ValueError, match="'leafwise' and 'depthwise'"):
        gbdt._params({"grow_policy": "lossguide"})                                       # what LambdaMART calls before it looks for a GPU
    with pytest.raises(ValueError, match="unknown parameter"):
        gbdt.GBDT({"feature_fraction": 0.5})
    if torch.cuda.is_available():
        assert gbdt.LambdaMART({"grow_policy": "depthwise"}).params["grow_policy"] == "depthwise"
    # the model file keeps the policy; a file written before the parameter existed loads as leaf-wise
    m = gbdt.GBDT({"grow_policy": "depthwise", "num_leaves": 4, "max_bin": 16})
    m.edges, m.nbins = np.full((2, 15), np.inf, np.float32), np.ones(2, np.int32)
    m.trees = [{"feature": np.array([0], np.int32), "threshold": np.array([0.5], np.float32), "left": np.array([~0], np.int32),
                "right": np.array([~1], np.int32), "value": np.array([-1.0, 1.0], np.float32)}]
    path = tmp_path / "m.npz"
    m.save_model(path)
    back = gbdt.GBDT.load_model(path)
    assert back.params == m.params and back.params["grow_policy"] == "depthwise" and len(back.trees) == 1
    with np.load(path, allow_pickle=False) as z:
        store = {k: z[k] for k in z.files}
    assert int(store["format"]) == 1
    old = json.loads(str(store["params"]))
    del old["grow_policy"]
    store["params"] = np.array(json.dumps(old))
    with open(tmp_path / "old.npz", "wb") as fh:
        np.savez(fh, **store)
    assert gbdt.GBDT.load_model(tmp_path / "old.npz").params["grow_policy"] == "leafwise"


# ---------------------------------------------------------------- the fixture regenerates
def test_the_depth_fixture_regenerates():
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("make_golden_gbdt_sklearn_depth", os.path.join(ROOT, "tests", "golden", "make_golden_gbdt_sklearn_depth.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    store = gen.generate()
    with np.load(LR.FILE, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(store)
        for k in z.files:
            a, b = z[k], np.asarray(store[k])
            if k.endswith(("/staged", "/fresh_pred", "/baseline")) or k.endswith("/leaves"):
                assert a.shape == b.shape and np.allclose(a, b, rtol=0, atol=1e-12), k   # values to 1e-12
            elif a.dtype.kind in "US":
                assert str(a) == str(b) or k == "sklearn_version"
            else:
                assert a.shape == b.shape and np.array_equal(a, b), k                    # inputs and trees exactly
