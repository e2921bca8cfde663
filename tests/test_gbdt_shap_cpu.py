"""CPU: TreeSHAP feature contributions of the native booster.  The six entry points are declared, exported and bound (ABI still 8); every
argument error fires before a launch; the host builder of the path tables (gbdt.shap_tables) on hand-built trees; the polynomial
restatement (tests/gbdt_shap_ref.py, the kernel's own order of operations) against the exponential oracle (the Shapley definition) on
trees of M <= 8 features with numeric nodes, NaNs under default_left and categorical sets; the gate constant C_SHAP measured there; and
feature_importance against a count by hand.  All without a GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import gbdt_shap_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ptr_gbdt_leaf_counts", "ptr_gbdt_leaf_counts_missing", "ptr_gbdt_leaf_counts_cat", "ptr_gbdt_shap", "ptr_gbdt_shap_missing",
                "ptr_gbdt_shap_cat")
WRAPPERS = ("gbdt_leaf_counts", "gbdt_shap")
KINDS = (("numeric", ()), ("missing", ()), ("cat", (1, 5)))


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
    assert "shap_tables" in pa.gbdt.__all__ and pa.gbdt.SHAP_MAX_ELEMENTS == 63
    for cls in (pa.GBDT, pa.LambdaMART):
        assert callable(cls.set_background) and "pred_contrib" in cls.predict.__code__.co_varnames
    assert callable(pa.GBDT.feature_importance)
    # the docstring's last "Not here:" sentence still names the three gaps the other tests pin
    doc = pa.gbdt.__doc__
    tail = doc[doc.rindex("Not here:"):]
    assert all(w in tail for w in ("feature_fraction", "EFB", "DART")) and "pred_contrib" in doc and "set_background" in doc


def test_argument_errors_fire_before_any_launch(lib):
    one = C.c_void_p(64)

    def err(rc, code, text):
        assert rc == code and text in lib.ptr_last_error(), (rc, lib.ptr_last_error())

    walk = (one, one, one, one, one)                                       # feature, threshold, left, right, tree_offsets
    err(lib.ptr_gbdt_leaf_counts(one, -4, 3, *walk, 1, 1, 2, one, None), 1001, b"negative")
    err(lib.ptr_gbdt_leaf_counts(one, 4, 3, *walk, -1, 1, 2, one, None), 1001, b"negative")
    err(lib.ptr_gbdt_leaf_counts(one, 4, 3, *walk, 1, -1, 2, one, None), 1001, b"negative")
    err(lib.ptr_gbdt_leaf_counts(one, 4, 3, *walk, 1, 1, -2, one, None), 1001, b"negative")
    err(lib.ptr_gbdt_leaf_counts(one, 4, 3, *walk, 1, 1, 2, None, None), 1001, b"counts")
    err(lib.ptr_gbdt_leaf_counts(None, 4, 3, *walk, 1, 1, 2, one, None), 1001, b"NULL pointer (X)")
    err(lib.ptr_gbdt_leaf_counts(one, 4, 3, None, one, one, one, one, 1, 1, 2, one, None), 1001, b"NULL tree")
    err(lib.ptr_gbdt_leaf_counts(one, 4, 3, None, None, None, None, None, 1, 0, 1, one, None), 1001, b"NULL tree")      # leaf-only trees still have offsets
    err(lib.ptr_gbdt_leaf_counts_missing(one, 4, 3, *walk, None, 1, 1, 2, one, None), 1001, b"NULL tree")
    err(lib.ptr_gbdt_leaf_counts_cat(one, 4, 3, *walk, None, None, one, one, 1, 1, 1, 2, one, None), 1001, b"is_cat")
    err(lib.ptr_gbdt_leaf_counts_cat(one, 4, 3, *walk, None, one, one, one, -1, 1, 1, 2, one, None), 1001, b"ncat")
    assert lib.ptr_gbdt_leaf_counts(None, 0, 3, None, None, None, None, None, 0, 0, 0, None, None) == 0   # no leaves: nothing to do

    tb = (one, one, one, 2, one, one, one, 3, one, one, 2, one, one)      # offsets, offsets, values, nleaves, path x3, npath, elem x2, nelem, quad x2
    err(lib.ptr_gbdt_shap(one, -4, 3, one, one, 1, *tb, one, None), 1001, b"negative")
    err(lib.ptr_gbdt_shap(one, 4, 3, one, one, -1, *tb, one, None), 1001, b"negative")
    err(lib.ptr_gbdt_shap(one, 4, 3, one, one, 1, one, one, one, -2, one, one, one, 3, one, one, 2, one, one, one, None), 1001, b"negative")
    err(lib.ptr_gbdt_shap(one, 4, 3, one, one, 1, one, one, one, 2, one, one, one, 2 ** 31, one, one, 2, one, one, one, None), 1001, b"int32")
    err(lib.ptr_gbdt_shap(one, 4, 8001, one, one, 1, *tb, one, None), 1002, b"LDS")
    err(lib.ptr_gbdt_shap(one, 4, 3, one, one, 1, *tb, None, None), 1001, b"phi")
    err(lib.ptr_gbdt_shap(None, 4, 3, one, one, 1, *tb, one, None), 1001, b"NULL pointer (X or phi)")
    err(lib.ptr_gbdt_shap(one, 4, 3, one, one, 1, None, one, one, 2, one, one, one, 3, one, one, 2, one, one, one, None), 1001, b"leaf table")
    err(lib.ptr_gbdt_shap(one, 4, 3, one, one, 1, one, one, one, 2, one, None, one, 3, one, one, 2, one, one, one, None), 1001, b"path table")
    err(lib.ptr_gbdt_shap(one, 4, 3, None, one, 1, *tb, one, None), 1001, b"tree array")
    err(lib.ptr_gbdt_shap(one, 4, 3, one, one, 1, one, one, one, 2, one, one, one, 3, one, None, 2, one, one, one, None), 1001, b"element table")
    err(lib.ptr_gbdt_shap(one, 4, 3, one, one, 1, one, one, one, 2, one, one, one, 3, one, one, 2, one, None, one, None), 1001, b"quadrature table")
    err(lib.ptr_gbdt_shap_missing(one, 4, 3, one, one, 1, *tb, None, one, None), 1001, b"tree array")
    err(lib.ptr_gbdt_shap_cat(one, 4, 3, one, one, 1, *tb, None, None, one, one, 1, one, None), 1001, b"is_cat")
    err(lib.ptr_gbdt_shap_cat(one, 4, 3, one, one, 1, *tb, None, one, one, one, -1, one, None), 1001, b"ncat")
    assert lib.ptr_gbdt_shap(None, 0, 3, None, None, 0, None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, None) == 0


def test_python_surface_checks_its_arguments_without_a_gpu():
    import ptranking_amd as pa
    Fn = pa.functional
    f32, i32 = (lambda *s: torch.zeros(s, dtype=torch.float32)), (lambda *s: torch.zeros(s, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.gbdt_leaf_counts(f32(4, 3), i32(0), f32(0), i32(0), i32(0), i32(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.gbdt_shap(f32(4, 3), i32(0), f32(0), {k: i32(1) for k in Fn.SHAP_TABLE_KEYS})
    with pytest.raises(TypeError):
        Fn.gbdt_shap(np.zeros((4, 3), np.float32), i32(0), f32(0), {})
    g = pa.GBDT({"num_leaves": 4})
    with pytest.raises(ValueError, match="keep no split gains.*pinned"):
        g.feature_importance("gain")
    with pytest.raises(ValueError, match="importance_type"):
        g.feature_importance("cover")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            g.set_background(np.zeros((4, 3), np.float32))


# ---------------------------------------------------------------- the path tables on hand-built trees
def hand_tree():
    """        node 0: f2 <= 0.5
             /                \\
        node 1: f0 <= 1.0     leaf 1
          /          \\
      leaf 0      node 2: f2 <= -1.0        (f2 again: one element with node 0)
                    /        \\
                 leaf 2     leaf 3"""
    return {"feature": np.array([2, 0, 2], np.int32), "threshold": np.array([0.5, 1.0, -1.0], np.float32), "left": np.array([1, ~0, ~2], np.int32),
            "right": np.array([~1, 2, ~3], np.int32), "value": np.array([1.0, -2.0, 0.5, 4.0], np.float32)}


def test_path_tables_with_feature_reuse():
    from ptranking_amd import gbdt
    tb = gbdt.shap_tables([hand_tree()], [np.array([5, 10, 2, 3])])
    assert tb["covers"][0].tolist() == [20, 10, 5] and tb["tree_leaf_offsets"].tolist() == [0, 4]
    assert tb["path_offsets"].tolist() == [0, 2, 3, 6, 9] and tb["elem_offsets"].tolist() == [0, 2, 3, 5, 7]
    assert tb["path_node"].tolist() == [0, 1, 0, 0, 1, 2, 0, 1, 2]
    assert tb["path_dir"].tolist() == [1, 1, 0, 1, 0, 1, 1, 0, 0]
    assert tb["path_elem"].tolist() == [0, 1, 0, 0, 1, 0, 0, 1, 0]           # leaves 2 and 3: f2 at nodes 0 and 2 is ONE element
    assert tb["elem_feature"].tolist() == [2, 0, 2, 2, 0, 2, 0]
    z = [10 / 20, 5 / 10, 10 / 20, (10 / 20) * (2 / 5), 5 / 10, (10 / 20) * (3 / 5), 5 / 10]
    assert tb["elem_z"].tolist() == z and tb["elem_z"].dtype == np.float64
    assert tb["leaf_value"].tolist() == [1.0, -2.0, 0.5, 4.0] and tb["leaf_value"].dtype == np.float32
    assert [tb[k].dtype for k in ("path_offsets", "elem_offsets", "path_node", "path_dir", "path_elem", "elem_feature")] == \
        [np.int32, np.int32, np.int32, np.uint8, np.uint8, np.int32]
    # a second tree's nodes are indexed over the nodes of all trees
    two = gbdt.shap_tables([hand_tree(), hand_tree()], [np.array([5, 10, 2, 3])] * 2)
    assert two["path_node"][9:].tolist() == [3, 4, 3, 3, 4, 5, 3, 4, 5] and two["tree_leaf_offsets"].tolist() == [0, 4, 8]
    assert two["path_offsets"].tolist() == [0, 2, 3, 6, 9, 11, 12, 15, 18]


def test_path_tables_of_a_leaf_only_tree_and_of_no_tree():
    from ptranking_amd import gbdt
    leaf = {"feature": np.zeros(0, np.int32), "threshold": np.zeros(0, np.float32), "left": np.zeros(0, np.int32), "right": np.zeros(0, np.int32),
            "value": np.array([0.25], np.float32)}
    tb = gbdt.shap_tables([leaf], [np.array([7])])
    assert tb["path_offsets"].tolist() == [0, 0] and tb["elem_offsets"].tolist() == [0, 0] and tb["leaf_value"].tolist() == [0.25]
    assert tb["path_node"].size == tb["elem_z"].size == 0
    X = np.zeros((3, 2), np.float32)
    assert SR.shap_polynomial(tb, [leaf], X, 2).tolist() == [[0.0, 0.0, 0.25]] * 3
    assert SR.shap_exponential([leaf], [np.array([7])], X, 2).tolist() == [[0.0, 0.0, 0.25]] * 3
    none = gbdt.shap_tables([], [])
    assert none["path_offsets"].tolist() == [0] and none["leaf_value"].size == 0 and none["tree_leaf_offsets"].tolist() == [0]
    assert not SR.shap_polynomial(none, [], X, 2).any()


def test_path_tables_take_63_distinct_features_and_refuse_64():
    from ptranking_amd import gbdt
    ok = SR.chain_tree(list(range(63)), [0.0] * 63, np.arange(64))
    tb = gbdt.shap_tables([ok], [np.ones(64, np.int64)])
    assert int(np.diff(tb["elem_offsets"]).max()) == 63 and tb["path_elem"].max() == 62
    with pytest.raises(ValueError, match=r"tree 0: the path to leaf 63 holds 64 distinct features, at most 63"):
        gbdt.shap_tables([SR.chain_tree(list(range(64)), [0.0] * 64, np.arange(65))], [np.ones(65, np.int64)])
    # depth is unbounded: 200 nodes on two features are two elements
    deep = SR.chain_tree([i % 2 for i in range(200)], [0.0] * 200, np.arange(201))
    assert int(np.diff(gbdt.shap_tables([deep], [np.ones(201, np.int64)])["elem_offsets"]).max()) == 2


def test_path_tables_refuse_a_cover_of_zero_and_a_broken_tree():
    from ptranking_amd import gbdt
    with pytest.raises(ValueError, match=r"tree 1: node 2 has cover 0"):
        gbdt.shap_tables([hand_tree(), hand_tree()], [np.array([5, 10, 2, 3]), np.array([5, 10, 0, 0])])
    with pytest.raises(ValueError, match=r"tree 0: node ~1 \(leaf 1\) has cover 0"):
        gbdt.shap_tables([hand_tree()], [np.array([5, 0, 2, 3])])
    with pytest.raises(ValueError, match="leaf counts"):
        gbdt.shap_tables([hand_tree()], [np.array([5, 1, 2])])
    broken = hand_tree()
    broken["right"] = np.array([~1, 2, ~2], np.int32)                        # leaf 2 twice, leaf 3 never
    with pytest.raises(ValueError, match="tree 0: node 2 has the child"):
        gbdt.shap_tables([broken], [np.array([5, 10, 2, 3])])


# ---------------------------------------------------------------- the two restatements against each other
@functools.lru_cache(maxsize=None)
def cases():
    """Per kind 24 models of 1 .. 4 random trees of 2 .. 16 leaves over F = 8 features (M <= 8), covers from a background of 400 rows."""
    from ptranking_amd import gbdt
    out = []
    for kind, cats in KINDS:
        for seed in range(24):
            rng = np.random.default_rng([seed, len(kind)])
            B = SR.random_rows(rng, 400, 8, kind, cats)
            trees = []
            while len(trees) < 1 + seed % 4:
                t = SR.random_tree(rng, 8, int(rng.integers(2, 17)), kind, cats)
                if SR.leaf_counts(t, B).min() > 0:
                    trees.append(t)
            counts = [SR.leaf_counts(t, B) for t in trees]
            X = SR.random_rows(rng, 48, 8, kind, cats)
            out.append((kind, trees, counts, gbdt.shap_tables(trees, counts), X))
    return out


def test_the_polynomial_restatement_is_the_shapley_definition_and_c_shap_comes_from_its_need():
    needs = {kind: 0.0 for kind, _ in KINDS}
    for kind, trees, counts, tb, X in cases():
        exp, pol = SR.shap_exponential(trees, counts, X, 8), SR.shap_polynomial(tb, trees, X, 8)
        needs[kind] = max(needs[kind], SR.need(pol, exp, trees))
        # local accuracy of both in float64, and the selected leaf: every o is 1 at the leaf the walk reaches, so the sums are the prediction
        pred = sum(np.asarray(t["value"], np.float32).astype(np.float64)[SR.leaf_of(t, X)] for t in trees)
        for phi in (exp, pol):
            assert np.abs(phi.sum(axis=1) - pred).max() <= 64 * SR.bound(trees)
        used = set(int(f) for t in trees for f in t["feature"])
        assert all(not pol[:, f].any() and not exp[:, f].any() for f in range(8) if f not in used)      # a dummy gets exactly 0.0
    worst = max(needs.values())
    print(f"need of shap_polynomial against shap_exponential, in 2^-52 sum_t max|v|: {needs}; C_SHAP {SR.C_SHAP} = ceil_half(2 x {worst:.3f})")
    assert all(any(k == kind for k, *_ in cases()) for kind, _ in KINDS)
    assert worst <= SR.NEED_POLYNOMIAL and SR.constant_from_need(SR.NEED_POLYNOMIAL) == SR.C_SHAP
    assert SR.constant_from_need(worst) == SR.C_SHAP, worst


def test_a_planted_fault_fails_the_gate():
    kind, trees, counts, tb, X = next(c for c in cases() if len(c[1]) > 1)
    exp = SR.shap_exponential(trees, counts, X, 8)
    wrong = dict(tb)
    wrong["elem_z"] = tb["elem_z"].copy()
    wrong["elem_z"][0] *= 1 + 2.0 ** -40                                    # one cover off by one part in 2^40
    assert SR.need(SR.shap_polynomial(wrong, trees, X, 8), exp, trees) > SR.C_SHAP
    flipped = dict(tb)
    flipped["path_dir"] = tb["path_dir"] ^ 1
    assert SR.need(SR.shap_polynomial(flipped, trees, X, 8), exp, trees) > SR.C_SHAP


def test_leaf_counts_restatement_sums_to_the_rows():
    for kind, trees, counts, tb, X in cases()[::5]:
        for i, (t, c) in enumerate(zip(trees, counts)):
            assert c.sum() == 400 and (SR.node_covers(t, c)[:1] == 400).all()
            assert np.array_equal(SR.node_covers(t, c), tb["covers"][i])


# ---------------------------------------------------------------- feature_importance
def test_feature_importance_counts_the_splits():
    import ptranking_amd as pa
    g = pa.GBDT({"num_leaves": 4})
    g.edges = np.zeros((5, 3), np.float32)                                 # a model of 5 features
    assert g.feature_importance().tolist() == [0, 0, 0, 0, 0]
    g.trees = [hand_tree(), hand_tree(), SR.chain_tree([4, 4, 0], [0.0] * 3, np.arange(4))]
    imp = g.feature_importance(importance_type="split")
    assert imp.dtype == np.int64 and imp.tolist() == [2 + 1, 0, 4, 0, 2]      # by hand: f0 once per hand tree and once in the chain, f2 twice per hand tree
    with pytest.raises(RuntimeError, match="fit_bins"):
        pa.GBDT().feature_importance()
