"""CPU: a trained GBDT carried onto new data (pred_leaf, refit, init_model).  The seven entry points are declared, exported and bound (ABI
still 8) and ptr_launch_form answers for ptr_gbdt_leaf_sums; every argument error of the C entry points and of the Python surface fires
without a GPU; the numpy restatement (tests/gbdt_lifecycle_ref.py) gives its known answers on hand-built trees; decay_rate=0 reproduces
leaf_value exactly; and what stays refused is still refused."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import gbdt_lifecycle_ref as LR
from launch_form import launch_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ptr_gbdt_predict_leaf", "ptr_gbdt_predict_leaf_missing", "ptr_gbdt_predict_leaf_cat", "ptr_gbdt_leaf_sums",
                "ptr_gbdt_leaf_sums_missing", "ptr_gbdt_leaf_sums_cat", "ptr_gbdt_add_by_leaf")
WRAPPERS = ("gbdt_predict_leaf", "gbdt_leaf_sums", "gbdt_add_by_leaf")


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


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
        assert name in pa.functional.__all__ and callable(getattr(pa.functional, name))
    for cls in (pa.GBDT, pa.LambdaMART):
        assert callable(cls.refit) and inspect.signature(cls.refit).parameters["decay_rate"].default == 0.9
        assert inspect.signature(cls.predict).parameters["pred_leaf"].default is False
    assert inspect.signature(pa.GBDT.fit_bins).parameters["init_model"].default is None
    assert inspect.signature(pa.LambdaMART.fit).parameters["init_model"].default is None
    doc = pa.gbdt.__doc__
    tail = doc[doc.rindex("Not here:"):]
    assert all(w in tail for w in ("feature_fraction", "EFB", "DART")) and all(w in doc for w in ("pred_leaf", "refit", "init_model"))


def test_leaf_sums_launch_forms(lib):
    budget = launch_form("ptr_gbdt_leaf_sums", 1, 1)[4]
    assert budget == 1024
    assert launch_form("ptr_gbdt_leaf_sums", 0, 31)[0] == 0
    for nl in (1, 2, 31, budget):
        kind, block, groups, lds, _ = launch_form("ptr_gbdt_leaf_sums", 5000, nl)[:5]
        assert (kind, block, groups, lds) == (1, 256, 5, 20 * nl)
    assert launch_form("ptr_gbdt_leaf_sums", 5000, budget + 1)[:4] == (2, 256, 5, 0)
    assert launch_form("ptr_gbdt_leaf_sums", 5000, 0)[0] == 2                                  # no cell: every row is lost, nothing to sum in LDS
    assert 8 * launch_form("ptr_gbdt_leaf_sums", 1, budget)[3] <= 160 * 1024                   # eight workgroups fit a compute unit's LDS
    assert [launch_form("ptr_gbdt_leaf_sums", n, 31)[2] for n in (1, 1024, 1025, 1024 * 1024, 1024 * 1024 + 1, 2 ** 31 - 1)] == [1, 1, 2, 1024, 1024, 1024]
    a, out = (C.c_int64 * 2)(5, 5), (C.c_int32 * 8)()
    assert lib.ptr_launch_form(b"ptr_gbdt_leaf_sums", a, 1, out, 8) == 1001 and b"takes 2" in lib.ptr_last_error()


def test_argument_errors_fire_before_any_launch(lib):
    one = C.c_void_p(64)

    def err(rc, text):
        assert rc == 1001 and text in lib.ptr_last_error(), (rc, lib.ptr_last_error())

    nodes = (one, one, one, one)                                           # feature, threshold, left, right
    err(lib.ptr_gbdt_predict_leaf(one, -1, 3, *nodes, one, 0, 2, 5, one, None), b"negative")
    err(lib.ptr_gbdt_predict_leaf(one, 4, -3, *nodes, one, 0, 2, 5, one, None), b"negative")
    err(lib.ptr_gbdt_predict_leaf(one, 4, 3, *nodes, one, -1, 2, 5, one, None), b"negative")
    err(lib.ptr_gbdt_predict_leaf(one, 4, 3, *nodes, one, 0, -2, 5, one, None), b"negative")
    err(lib.ptr_gbdt_predict_leaf(one, 4, 3, *nodes, one, 0, 2, -5, one, None), b"negative")
    err(lib.ptr_gbdt_predict_leaf(one, 4, 3, *nodes, one, 0, 2, 5, None, None), b"NULL pointer (X or leaf)")
    err(lib.ptr_gbdt_predict_leaf(None, 4, 3, *nodes, one, 0, 2, 5, one, None), b"NULL pointer (X or leaf)")
    err(lib.ptr_gbdt_predict_leaf(one, 4, 3, *nodes, None, 0, 2, 5, one, None), b"NULL tree")
    err(lib.ptr_gbdt_predict_leaf(one, 4, 3, one, None, one, one, one, 0, 2, 5, one, None), b"NULL tree")
    err(lib.ptr_gbdt_predict_leaf_missing(one, 4, 3, *nodes, one, None, 0, 2, 5, one, None), b"NULL tree")
    err(lib.ptr_gbdt_predict_leaf_cat(one, 4, 3, *nodes, one, None, None, one, one, 1, 0, 2, 5, one, None), b"is_cat")
    err(lib.ptr_gbdt_predict_leaf_cat(one, 4, 3, *nodes, one, None, one, one, one, -1, 0, 2, 5, one, None), b"ncat")
    assert lib.ptr_gbdt_predict_leaf(None, 0, 3, None, None, None, None, None, 0, 2, 0, None, None) == 0       # no rows: nothing to do
    assert lib.ptr_gbdt_predict_leaf(None, 4, 3, None, None, None, None, None, 0, 0, 0, None, None) == 0       # no trees

    tail = (one, one, 3, one, one, None)                                   # qg, qh, nleaves, leaf, sums, stream
    err(lib.ptr_gbdt_leaf_sums(one, -4, 3, *nodes, 2, *tail), b"negative")
    err(lib.ptr_gbdt_leaf_sums(one, 4, -3, *nodes, 2, *tail), b"negative")
    err(lib.ptr_gbdt_leaf_sums(one, 4, 3, *nodes, -2, *tail), b"negative")
    err(lib.ptr_gbdt_leaf_sums(one, 4, 3, *nodes, 2, one, one, -3, one, one, None), b"negative")
    err(lib.ptr_gbdt_leaf_sums(None, 4, 3, *nodes, 2, *tail), b"NULL pointer")
    err(lib.ptr_gbdt_leaf_sums(one, 4, 3, *nodes, 2, None, one, 3, one, one, None), b"NULL pointer")
    err(lib.ptr_gbdt_leaf_sums(one, 4, 3, *nodes, 2, one, None, 3, one, one, None), b"NULL pointer")
    err(lib.ptr_gbdt_leaf_sums(one, 4, 3, *nodes, 2, one, one, 3, None, one, None), b"NULL pointer")
    err(lib.ptr_gbdt_leaf_sums(one, 4, 3, *nodes, 2, one, one, 3, one, None, None), b"NULL pointer")
    err(lib.ptr_gbdt_leaf_sums(one, 4, 3, one, one, None, one, 2, *tail), b"NULL tree")
    err(lib.ptr_gbdt_leaf_sums_missing(one, 4, 3, *nodes, None, 2, *tail), b"NULL tree")
    err(lib.ptr_gbdt_leaf_sums_cat(one, 4, 3, *nodes, None, None, one, one, 1, 2, *tail), b"is_cat")
    err(lib.ptr_gbdt_leaf_sums_cat(one, 4, 3, *nodes, None, one, one, one, -1, 2, *tail), b"ncat")
    assert lib.ptr_gbdt_leaf_sums(None, 0, 3, None, None, None, None, 0, None, None, 1, None, None, None) == 0  # no rows

    err(lib.ptr_gbdt_add_by_leaf(one, -1, one, one, 3, None), b"negative")
    err(lib.ptr_gbdt_add_by_leaf(one, 4, one, one, -3, None), b"negative")
    err(lib.ptr_gbdt_add_by_leaf(None, 4, one, one, 3, None), b"NULL pointer")
    err(lib.ptr_gbdt_add_by_leaf(one, 4, None, one, 3, None), b"NULL pointer")
    err(lib.ptr_gbdt_add_by_leaf(one, 4, one, None, 3, None), b"NULL pointer")
    assert lib.ptr_gbdt_add_by_leaf(None, 0, None, None, 3, None) == 0 and lib.ptr_gbdt_add_by_leaf(one, 4, one, None, 0, None) == 0


def test_the_python_surface_refuses_before_it_needs_a_gpu(tmp_path):
    import ptranking_amd as pa
    X = np.zeros((4, 2), np.float32)
    b = pa.GBDT()
    b.edges, b.nbins = np.zeros((2, 254), np.float32), np.ones(2, np.int32)
    for bad in (-0.1, 1.5, float("nan"), "much"):
        with pytest.raises(ValueError, match="decay_rate"):
            b.refit(X, lambda s: (s, s), decay_rate=bad)
    with pytest.raises(ValueError, match="pred_leaf and pred_contrib"):
        b.predict(X, pred_leaf=True, pred_contrib=True)
    mono = pa.GBDT({"monotone_constraints": [1, 0]})
    mono.edges, mono.nbins = b.edges, b.nbins
    with pytest.raises(ValueError, match="monotone_constraints"):
        mono.refit(X, lambda s: (s, s))
    assert "monotone" not in pa.gbdt.constraints(pa.GBDT({"monotone_constraints": [0, 0]}).params)     # all zero: not active, refit does not refuse it here

    for key, theirs, ours in (("max_bin", {"max_bin": 63}, {}), ("use_missing", {"use_missing": True}, {}),
                              ("categorical_feature", {"categorical_feature": [1]}, {"categorical_feature": [0]}),
                              ("categorical_feature", {}, {"categorical_feature": [1]})):
        model = pa.GBDT(theirs)
        model.edges, model.nbins = np.zeros((2, model.params["max_bin"] - 1), np.float32), np.ones(2, np.int32)
        with pytest.raises(ValueError, match=key):
            pa.GBDT(ours).fit_bins(X, init_model=model)
    with pytest.raises(ValueError, match="init_model must be"):
        pa.GBDT().fit_bins(X, init_model=7)
    with pytest.raises(ValueError, match="no bin edges"):
        pa.GBDT().fit_bins(X, init_model=pa.GBDT())
    # a path is a model too, and its keys are compared the same way
    path = str(tmp_path / "m.npz")
    b.save_model(path)
    with pytest.raises(ValueError, match="max_bin"):
        pa.GBDT({"max_bin": 15}).fit_bins(X, init_model=path)


def test_what_stays_refused_is_still_refused():
    from ptranking_amd import gbdt
    with pytest.raises(ValueError, match="boosting_type"):
        gbdt._params({"boosting_type": "dart"})
    with pytest.raises(ValueError, match="feature_fraction"):
        gbdt._params({"feature_fraction": 0.8})


# ---------------------------------------------------------------- the restatement's own known answers
def test_a_tree_of_no_node_gives_leaf_zero():
    t = LR.chain_tree(1)
    X = np.array([[0.0], [np.nan], [7.5]], np.float32)
    assert LR.leaf_index(t, X).tolist() == [0, 0, 0] == LR.leaf_index_numeric(t, X).tolist()
    assert LR.leaf_sums([0, 0, 0], [3, -5, 7], [1, 1, 2], 1).tolist() == [[5, 4, 3]]
    assert LR.leaf_index(t, X, nleaves=0).tolist() == [-1, -1, -1]


def test_a_single_split():
    t = {"feature": np.array([1], np.int32), "threshold": np.array([0.5], np.float32), "left": np.array([~0], np.int32),
         "right": np.array([~1], np.int32), "value": np.array([-1.0, 2.0], np.float32)}
    X = np.array([[9, 0.5], [9, 0.50001], [-9, -3], [0, np.nan]], np.float32)
    assert LR.leaf_index(t, X).tolist() == [0, 1, 0, 1] == LR.leaf_index_numeric(t, X).tolist()      # x <= threshold goes left; a NaN compares false
    assert LR.leaf_sums([0, 1, 0, 1], [1, 2, 3, 4], [10, 20, 30, 40], 2).tolist() == [[4, 40, 2], [6, 60, 2]]
    assert LR.sum_leaf_values([t, t], np.array([[0, 1], [1, 1]])).tolist() == [1.0, 4.0]


def test_a_nan_follows_default_left():
    t = {"feature": np.array([0, 0], np.int32), "threshold": np.array([0.0, 5.0], np.float32), "left": np.array([~0, ~1], np.int32),
         "right": np.array([1, ~2], np.int32), "value": np.zeros(3, np.float32), "default_left": np.array([0, 1], np.uint8)}
    X = np.array([[np.nan], [-1.0], [3.0], [6.0]], np.float32)
    assert LR.leaf_index(t, X).tolist() == [1, 0, 1, 2]                    # right at node 0 (default_left 0), left at node 1
    t["default_left"] = np.array([1, 0], np.uint8)
    assert LR.leaf_index(t, X).tolist() == [0, 0, 1, 2]


def test_categorical_nodes_and_the_unseen_code():
    sets = np.zeros((1, 4), np.int64)
    sets[0, 0] = (1 << 1) | (1 << 3)                                       # the codes 1 and 3 go left
    sets[0, 1] = 1 << (70 - 64)                                            # and 70
    t = {"feature": np.array([0, 1], np.int32), "threshold": np.array([0.0, 0.5], np.float32), "left": np.array([~0, ~1], np.int32),
         "right": np.array([1, ~2], np.int32), "value": np.zeros(3, np.float32), "cat_index": np.array([0, -1], np.int32), "cat_set": sets,
         "default_left": np.array([1, 0], np.uint8)}
    is_cat = np.array([1, 0], np.uint8)
    X = np.array([[1, 9], [3, 9], [70, 9], [2, 0], [200, 0], [255, 1], [1.5, 0], [-1, 1], [300, 0], [np.nan, 9]], np.float32)
    # in the set: left.  2 was seen and is not in it; 200 and 255 were never seen; 1.5, -1 and 300 are no codes: all right, then x1 <= 0.5
    assert LR.leaf_index(t, X, is_cat).tolist() == [0, 0, 0, 1, 1, 2, 1, 2, 1, 0]
    # a node whose kind is not its feature's, or whose set does not exist, loses the row
    assert LR.leaf_index(t, X[:2], np.array([0, 0], np.uint8)).tolist() == [-1, -1]
    assert LR.leaf_index(dict(t, cat_index=np.array([1, -1], np.int32)), X[:2], is_cat).tolist() == [-1, -1]


def test_malformed_trees_lose_their_rows():
    t = LR.chain_tree(4)
    X = np.array([[-1.0], [0.5], [1.5], [9.0]], np.float32)
    assert LR.leaf_index(t, X).tolist() == [0, 1, 2, 3]
    cyc = dict(t, right=np.array([1, 0, ~3], np.int32))                    # node 1 sends right back to node 0: the walk runs out of steps
    assert LR.leaf_index(cyc, X).tolist() == [0, 1, -1, -1] == LR.leaf_index_numeric(cyc, X).tolist()
    far = dict(t, right=np.array([1, 7, ~3], np.int32))                    # a child out of range
    assert LR.leaf_index(far, X).tolist() == [0, 1, -1, -1] == LR.leaf_index_numeric(far, X).tolist()
    feat = dict(t, feature=np.array([0, 5, 0], np.int32))                  # a feature out of range
    assert LR.leaf_index(feat, X).tolist() == [0, -1, -1, -1] == LR.leaf_index_numeric(feat, X).tolist()
    leafy = dict(t, left=np.array([~0, ~9, ~2], np.int32))                 # a leaf the tree does not have
    assert LR.leaf_index(leafy, X).tolist() == [0, -1, 2, 3] == LR.leaf_index_numeric(leafy, X).tolist()
    assert LR.leaf_index(t, X, nleaves=2).tolist() == [0, 1, -1, -1] == LR.leaf_index_numeric(t, X, nleaves=2).tolist()


def test_the_vectorised_walk_is_the_walk():
    rng = np.random.default_rng(5)
    for nl in (1, 2, 31, 300):
        t = LR.chain_tree(nl, step=0.25)
        X = rng.uniform(-2, nl * 0.25 + 2, (400, 1)).astype(np.float32)
        X[::37] = np.nan
        assert np.array_equal(LR.leaf_index(t, X), LR.leaf_index_numeric(t, X))


def test_an_unreached_leaf_keeps_its_value_and_the_rule_is_the_stated_one():
    expo = (20, 10)
    assert LR.refit_value(np.float32(0.37), 123, 456, 0, expo, 0.0, 0.1, 0.0) == np.float32(0.37)      # no row: old
    assert LR.refit_value(np.float32(0.37), 123, 0, 5, expo, 0.0, 0.1, 0.5) == np.float32(0.37)        # H + lambda_l2 <= 0: old
    assert LR.refit_value(np.float32(0.37), 123, -7, 5, expo, 0.0, 0.1, 0.5) == np.float32(0.37)
    G, H = 123 * 2.0 ** -20, 456 * 2.0 ** -10
    new = -G / (H + 1.5) * 0.1
    assert LR.new_value(123, 456, expo, 1.5, 0.1) == new
    old = np.float32(0.37)
    assert LR.refit_value(old, 123, 456, 5, expo, 1.5, 0.1, 0.9) == np.float32(0.9 * np.float64(old) + (1.0 - 0.9) * new)
    assert LR.refit_value(old, 123, 456, 5, expo, 1.5, 0.1, 1.0) == old                                # decay 1: nothing moves


def test_decay_zero_reproduces_leaf_value_and_the_package_agrees_with_the_restatement():
    from ptranking_amd import gbdt
    rng = np.random.default_rng(11)
    for _ in range(300):
        expo = (int(rng.integers(0, 40)), int(rng.integers(0, 40)))
        g, h, c = int(rng.integers(-2 ** 40, 2 ** 40)), int(rng.integers(1, 2 ** 40)), int(rng.integers(1, 1000))
        l2, lr = float(rng.choice([0.0, 0.5, 3.0])), float(rng.choice([0.05, 0.1, 0.3]))
        old = np.float32(rng.standard_normal())
        want = gbdt.leaf_value(g, h, expo, l2, lr)
        for rule in (LR.refit_value, gbdt.refit_value):
            got = rule(old, g, h, c, expo, l2, lr, 0.0)
            assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
        for decay in (0.3, 0.9, 1.0):
            assert LR.refit_value(old, g, h, c, expo, l2, lr, decay).tobytes() == gbdt.refit_value(old, g, h, c, expo, l2, lr, decay).tobytes()
        for count, hh in ((0, h), (c, 0), (c, -h)):
            assert LR.refit_value(old, g, hh, count, expo, 0.0, lr, 0.5).tobytes() == old.tobytes() == gbdt.refit_value(old, g, hh, count, expo, 0.0, lr, 0.5).tobytes()
    # a leaf whose gradients sum to zero: trained as -0.0, and refit on its own value gives the same bits
    zero = gbdt.leaf_value(0, 5, (3, 3), 0.0, 0.1)
    assert LR.refit_value(zero, 0, 5, 2, (3, 3), 0.0, 0.1, 0.0).tobytes() == zero.tobytes() == gbdt.refit_value(zero, 0, 5, 2, (3, 3), 0.0, 0.1, 0.0).tobytes()


def test_refit_on_the_host_walks_sums_and_adds_in_order():
    t = LR.chain_tree(3)                                                   # leaves: x <= 0, x <= 1, the rest; leaf 1 gets no row below
    t["value"] = np.array([0.5, 0.25, -0.5], np.float32)
    X = np.array([[-1.0], [-2.0], [5.0]], np.float32)
    y = np.array([1.0, 3.0, -4.0], np.float32)
    values, scores = LR.refit([t, t], X, lambda s: (s - y, np.ones_like(s)), 0.0, 0.5, 0.0)
    assert values[0].tolist() == [1.0, 0.25, -2.0]                         # half the mean residual; the unreached leaf keeps 0.25
    assert values[1].tolist() == [0.5, 0.25, -1.0] and scores.tolist() == [1.5, 1.5, -3.0]
