"""CPU: row sampling of the native booster (bagging by row or by query, GOSS).  The parameters are accepted with LightGBM's names and
defaults and refused where the rules say so; the four entry points are declared, exported and bound, every argument error fires before a
launch and the Python surface refuses to run without a GPU; the numpy restatement tests/gbdt_sample_ref.py checks itself: the exact select
against a sort on every awkward key family, the stable partition, the binned walk against the raw-feature walk, and the hash's bag size."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import gbdt_ref as R
import gbdt_sample_ref as S
from launch_form import launch_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ptr_gbdt_bag_mask", "ptr_gbdt_goss_ws_ints", "ptr_gbdt_goss", "ptr_gbdt_partition_mask", "ptr_gbdt_add_tree_binned")
WRAPPERS = ("gbdt_bag_mask", "gbdt_goss", "gbdt_partition_mask", "gbdt_add_tree_binned")
NEW_DEFAULTS = {"bagging_fraction": 1.0, "bagging_freq": 0, "bagging_seed": 3, "bagging_by_query": False, "data_sample_strategy": "bagging",
                "top_rate": 0.2, "other_rate": 0.1}


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


# ---------------------------------------------------------------- the parameters
def test_every_new_key_is_accepted_with_its_default():
    from ptranking_amd import gbdt
    for k, v in NEW_DEFAULTS.items():
        assert gbdt.DEFAULT_PARAMS[k] == v and type(gbdt.DEFAULT_PARAMS[k]) is type(v), k
        assert gbdt._params({k: v})[k] == v and gbdt.GBDT({k: v}).params == gbdt.GBDT().params
        assert k not in gbdt.IGNORED_PARAMS
    p = gbdt._params({"bagging_fraction": 0.8, "bagging_freq": 1, "bagging_seed": 7, "bagging_by_query": True})
    assert (p["bagging_fraction"], p["bagging_freq"], p["bagging_seed"], p["bagging_by_query"]) == (0.8, 1, 7, True)
    p = gbdt._params({"data_sample_strategy": "goss", "top_rate": 0.5, "other_rate": 0.5, "bagging_freq": 5})      # fraction 1.0: no bagging
    assert p["data_sample_strategy"] == "goss" and gbdt.MODEL_FORMAT == 1
    assert gbdt._params({"data_sample_strategy": "goss", "bagging_fraction": 0.5})["bagging_freq"] == 0            # freq 0: no bagging either


def test_which_parameters_switch_sampling_on():
    from ptranking_amd import gbdt
    on = lambda d: gbdt.sampling(gbdt._params(d))
    assert on({}) is None and on({"bagging_freq": 5, "bagging_fraction": 1.0}) is None and on({"bagging_fraction": 0.5}) is None
    assert on({"bagging_freq": 1, "bagging_fraction": 0.5}) == "bagging" and on({"data_sample_strategy": "goss"}) == "goss"
    assert on({"bagging_by_query": True}) is None
    for d in ({}, {"bagging_freq": 5, "bagging_fraction": 1.0}, {"bagging_freq": 2, "bagging_fraction": 0.5}, {"data_sample_strategy": "goss"}):
        assert S.sampling(d) == on(d)


@pytest.mark.parametrize("bad", [{"bagging_fraction": 0.0}, {"bagging_fraction": -0.1}, {"bagging_fraction": 1.5}, {"bagging_fraction": float("nan")},
                                 {"bagging_freq": -1}, {"bagging_freq": 1.5}, {"bagging_seed": -1}, {"bagging_by_query": "yes"},
                                 {"data_sample_strategy": "random"}, {"data_sample_strategy": None},
                                 {"top_rate": 0.0}, {"other_rate": 0.0}, {"top_rate": -0.2}, {"top_rate": 0.95}, {"top_rate": 0.6, "other_rate": 0.5},
                                 {"other_rate": float("nan")},
                                 {"data_sample_strategy": "goss", "bagging_freq": 1, "bagging_fraction": 0.5}])
def test_refusals_come_as_value_errors_before_any_device_work(bad):
    from ptranking_amd import gbdt
    with pytest.raises(ValueError) as e:
        gbdt._params(bad)
    assert "unknown parameter" not in str(e.value)
    with pytest.raises(ValueError):
        gbdt.GBDT(bad)                                                                   # no GPU is asked for before the parameters are read


def test_what_stays_out_of_scope_still_raises():
    from ptranking_amd import gbdt
    with pytest.raises(ValueError, match="unknown parameter"):
        gbdt.GBDT({"feature_fraction": 0.5})
    with pytest.raises(ValueError, match="only 'gbdt'"):
        gbdt.GBDT({"boosting_type": "goss"})


def test_parameters_travel_in_the_model_file_and_an_older_file_loads(tmp_path):
    from ptranking_amd import gbdt
    m = gbdt.GBDT({"bagging_fraction": 0.5, "bagging_freq": 2, "bagging_by_query": True, "bagging_seed": 11, "num_leaves": 4, "max_bin": 16})
    m.edges, m.nbins = np.full((2, 15), np.inf, np.float32), np.ones(2, np.int32)
    m.trees = [{"feature": np.array([0], np.int32), "threshold": np.array([0.5], np.float32), "left": np.array([~0], np.int32),
                "right": np.array([~1], np.int32), "value": np.array([-1.0, 1.0], np.float32)}]
    path = tmp_path / "m.npz"
    m.save_model(path)
    back = gbdt.GBDT.load_model(path)
    assert back.params == m.params and back.params["bagging_by_query"] is True and back.params["bagging_seed"] == 11
    with np.load(path, allow_pickle=False) as z:
        store = {k: z[k] for k in z.files}
    assert int(store["format"]) == 1
    old = json.loads(str(store["params"]))
    for k in NEW_DEFAULTS:
        del old[k]
    store["params"] = np.array(json.dumps(old))
    with open(tmp_path / "old.npz", "wb") as fh:
        np.savez(fh, **store)
    parent = gbdt.GBDT.load_model(tmp_path / "old.npz")
    assert {k: parent.params[k] for k in NEW_DEFAULTS} == NEW_DEFAULTS and len(parent.trees) == 1


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
    one, two, f32, f64, u64 = C.c_void_p(64), C.c_void_p(128), C.c_float, C.c_double, C.c_uint64

    def err(rc, code, text):
        assert rc == code and text in lib.ptr_last_error(), (rc, lib.ptr_last_error())

    def bag(n=8, qid=None, seed=3, draw=0, fraction=0.5, mask=one):
        return lib.ptr_gbdt_bag_mask(n, qid, u64(seed), draw, f32(fraction), mask, None)
    err(bag(mask=None), 1001, b"NULL")
    err(bag(n=-1), 1001, b"n=-1")
    err(bag(n=2 ** 31), 1001, b"int32")
    err(bag(draw=-1), 1001, b"draw")
    for bad in (0.0, -0.5, 1.5, float("nan")):
        err(bag(fraction=bad), 1001, b"fraction")
    assert bag(n=0, mask=None) == 0

    def goss(g=one, h=one, n=8, top=0.2, other=0.1, seed=3, draw=0, go=one, ho=one, mask=one, info=one, ws=one):
        return lib.ptr_gbdt_goss(g, h, n, f64(top), f64(other), u64(seed), draw, go, ho, mask, info, ws, None)
    for k in ("g", "h", "go", "ho", "mask", "info", "ws"):
        err(goss(**{k: None}), 1001, b"NULL")
    err(goss(n=-1), 1001, b"n=-1")
    err(goss(draw=-2), 1001, b"draw")
    for top, other in ((0.0, 0.1), (0.2, 0.0), (-0.1, 0.1), (0.6, 0.5), (1.0, 0.1), (float("nan"), 0.1), (0.2, float("nan"))):
        err(goss(top=top, other=other), 1001, b"top_rate")
    assert goss(n=0, g=None, h=None, go=None, ho=None, mask=None, info=None, ws=None) == 0
    assert lib.ptr_gbdt_goss_ws_ints(1) == lib.ptr_gbdt_goss_ws_ints(10 ** 6) == 3 * 2048 + 4

    def part(mask=one, n=8, rows=one, m=8, out=two, lc=one, ws=one):
        return lib.ptr_gbdt_partition_mask(mask, n, rows, m, out, lc, ws, None)
    for k in ("mask", "out", "lc", "ws"):
        err(part(**{k: None}), 1001, b"NULL")
    err(part(n=-1), 1001, b"n=-1")
    err(part(m=-1), 1001, b"m=-1")
    err(part(out=one), 1001, b"out must not be rows")

    def walk(scores=one, bins=one, stride=16, n=8, F=3, rows=one, m=8, feature=one, bin=one, left=one, right=one, value=one, nn=3):
        return lib.ptr_gbdt_add_tree_binned(scores, bins, stride, n, F, rows, m, feature, bin, left, right, value, nn, None)
    for k in ("scores", "bins", "feature", "bin", "left", "right", "value"):
        err(walk(**{k: None}), 1001, b"NULL")
    err(walk(stride=12), 1001, b"stride")
    err(walk(F=20), 1001, b"stride")
    err(walk(n=-1), 1001, b"size")
    err(walk(m=-1), 1001, b"m=-1")
    err(walk(nn=-1), 1001, b"nnodes=-1")
    err(walk(rows=None, m=9), 1001, b"rows is NULL")
    assert walk(m=0, rows=None) == 0 and walk(n=0, m=0) == 0


def test_launch_forms(lib):
    assert launch_form("ptr_gbdt_goss", 0)[:4] == (3, 2048, 0, 0)
    assert launch_form("ptr_gbdt_goss", 1)[:4] == (3, 2048, 1, 5) and launch_form("ptr_gbdt_goss", 4096)[2] == 1
    assert launch_form("ptr_gbdt_goss", 4097)[2] == 2 and launch_form("ptr_gbdt_goss", 70001)[2] == 18
    assert launch_form("ptr_gbdt_goss", 2 ** 31 - 1)[2] == 2048                          # the cap: the workgroups stride over the rows
    assert launch_form("ptr_gbdt_partition_mask", 1024)[:2] == (3, 1) and launch_form("ptr_gbdt_partition_mask", 1025)[:2] == (3, 2)


def test_python_surface_refuses_to_run_without_a_gpu():
    import ptranking_amd as pa
    Fn = pa.functional
    i32, u8, f32 = (lambda *s: torch.zeros(s, dtype=torch.int32)), (lambda *s: torch.zeros(s, dtype=torch.uint8)), (lambda *s: torch.zeros(s))
    calls = {"gbdt_bag_mask": lambda: Fn.gbdt_bag_mask(4, 3, 0, 0.5, device="cpu"),
             "gbdt_goss": lambda: Fn.gbdt_goss(f32(4), f32(4), 0.2, 0.1, 3, 0),
             "gbdt_partition_mask": lambda: Fn.gbdt_partition_mask(u8(4)),
             "gbdt_add_tree_binned": lambda: Fn.gbdt_add_tree_binned(f32(4), u8(4, 16), 3, None, i32(1), i32(1), i32(1), i32(1), f32(2))}
    assert set(calls) == set(WRAPPERS)
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.gbdt_bag_mask(4, 3, 0, 0.5, qid=i32(4))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pa.GBDT({"bagging_fraction": 0.5, "bagging_freq": 1}, X=np.zeros((4, 3), np.float32))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pa.LambdaMART({"data_sample_strategy": "goss"})


# ---------------------------------------------------------------- the restatement checks itself
def test_uniforms_are_the_sampler_stream_without_the_sample_step():
    """u(draw, unit) skips pl_sample_keys: it is NOT ptr_pl_uniforms' value for (query draw, sample 0, item unit), and it is a multiple of
    2^-24 in [0, 1) that differs from draw to draw and from seed to seed."""
    import plsample_ref as P
    u = S.uniforms(3, 5, np.arange(1000))
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2.0 ** 24, np.rint(u * 2.0 ** 24))
    assert not np.array_equal(u, P.uniforms_host(1, 1000, 1, 3, q0=5)[0, 0])
    assert not np.array_equal(u, S.uniforms(3, 6, np.arange(1000))) and not np.array_equal(u, S.uniforms(4, 5, np.arange(1000)))
    assert np.array_equal(S.uniforms(3, 5, [7, 7, 2 ** 32 + 7]), np.repeat(u[7], 3))       # a unit is taken as uint32
    assert np.array_equal(S.uniforms(2 ** 40 + 3, 2 ** 33, [1]), S.uniforms(2 ** 40 + 3, 2 ** 33, [1]))
    assert not np.array_equal(S.uniforms(2 ** 40 + 3, 1, np.arange(50)), S.uniforms(3, 1, np.arange(50)))         # the seed's high word counts


def test_the_bag_size_is_binomial():
    """A condition on the hash: on n = 10^5 units the bag holds n p within 5 sqrt(n p (1 - p)) units (a binomial's standard deviation;
    5 of them are passed with probability 6e-7 per draw by a fair stream).  The thresholds are multiples of 2^-24 after the cast, which
    moves p by less than 1e-7, that is n p by less than 0.01."""
    n = 100_000
    for seed, draw, p in ((3, 0, 0.5), (3, 1, 0.5), (3, 0, 0.8), (12345, 7, 0.1), (0, 0, 0.632), (2 ** 63, 40, 0.05)):
        got = int(S.bag_mask(n, seed, draw, p).sum())
        bound = 5.0 * np.sqrt(n * p * (1.0 - p))
        print(f"MEASURED bag size seed {seed} draw {draw} p {p}: {got} for {n * p:.0f} +- {bound:.0f}")
        assert abs(got - n * p) <= bound
    assert S.bag_mask(1000, 3, 0, 1.0).all()                                             # u < 1 always
    assert S.bag_mask(100_000, 3, 0, 2.0 ** -24).sum() == (S.uniforms(3, 0, np.arange(100_000)) == 0).sum()
    # by query: whole queries, ragged, an empty and a one-document query among them
    group = np.array([5, 0, 1, 17, 3, 0, 40])
    qid = S.group_qid(group)
    m = S.bag_mask(qid.size, 3, 2, 0.5, qid)
    per_query = S.bag_mask(group.size, 3, 2, 0.5)
    assert np.array_equal(m, per_query[qid]) and qid.size == group.sum() and 1 not in qid and 5 not in qid


def _select_cases():
    rng = np.random.default_rng(0)
    n = 5000
    one = np.ones(n, np.float32)
    yield "all equal", np.full(n, 0.37, np.float32), one
    yield "all zero", np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    yield "two values", np.where(rng.random(n) < 0.3, 2.0, -0.5).astype(np.float32), one
    yield "denormal products", (rng.standard_normal(n) * 2.0 ** -80).astype(np.float32), (rng.random(n) * 2.0 ** -60).astype(np.float32)
    yield "overflow to +inf", (rng.standard_normal(n) * 2.0 ** 100).astype(np.float32), np.where(rng.random(n) < 0.5, 2.0 ** 100, 1.0).astype(np.float32)
    yield "gaussian", rng.standard_normal(n).astype(np.float32), rng.random(n).astype(np.float32)


@pytest.mark.parametrize("name,g,h", list(_select_cases()), ids=[c[0] for c in _select_cases()])
def test_the_select_equals_a_sort(name, g, h):
    bits, nan = S.goss_keys(g, h)
    assert not nan.any()
    n = bits.size
    srt = np.sort(bits)[::-1]
    with np.errstate(all="ignore"):
        keys = np.abs(g * h)
    assert np.array_equal(np.argsort(bits, kind="stable"), np.argsort(keys, kind="stable"))       # the bit patterns order as the floats do
    if name == "all zero":
        assert (bits == 0).all() and (g * h == 0).all() and np.signbit(g * h).any()                 # -0.0 products: the key is +0
    if name == "denormal products":
        assert ((keys > 0) & (keys < 2.0 ** -126)).sum() > n // 2
    if name == "overflow to +inf":
        assert np.isinf(keys).sum() > n // 4 and srt[0] == 0x7F800000
    for k in (1, 2, n // 5, n // 2, n - 1, n):
        assert S.select_kth_largest(bits, k) == srt[k - 1], k
    assert S.goss_top_k(n, 1.0 / n) == 1 and S.goss_top_k(n, 1.0) == n and S.goss_top_k(3, 0.2) == 1 and S.goss_top_k(1, 0.2) == 1


def test_goss_rule_on_ties_weights_and_a_nan():
    rng = np.random.default_rng(1)
    n = 1000
    g, h = np.full(n, 0.5, np.float32), np.ones(n, np.float32)
    g2, h2, mask, (tau, ntop, nkeep) = S.goss(g, h, 0.2, 0.1, 3, 4)
    assert ntop == nkeep == n and mask.all() and np.array_equal(g2, g) and tau == np.float32(0.5).view(np.uint32)      # ties at tau are all in
    g, h = rng.standard_normal(n).astype(np.float32), rng.random(n).astype(np.float32)
    g[17] = np.nan
    g2, h2, mask, (tau, ntop, nkeep) = S.goss(g, h, 0.2, 0.1, 3, 4)
    keys = np.abs(g * h)
    assert ntop == 200 and tau == np.sort(keys[~np.isnan(keys)])[::-1][199].view(np.uint32)
    top = keys >= np.uint32(tau).view(np.float32)
    assert top.sum() == 200 and not top[17] and np.isnan(g2[17])                           # the NaN is an "other" row and stays a NaN
    other = mask.astype(bool) & ~top
    w = np.float32(0.8 / 0.1)
    assert np.array_equal(g2[top], g[top]) and np.array_equal(h2[other], h[other] * w) and w == 8.0
    dropped = ~mask.astype(bool)
    assert np.array_equal(g2[dropped & ~np.isnan(g)], g[dropped & ~np.isnan(g)]) and nkeep == mask.sum()
    p = 0.1 / 0.8
    assert abs(other.sum() - 800 * p) <= 5.0 * np.sqrt(800 * p * (1 - p))
    # K = 1 and K = n
    assert S.goss(g, h, 1.0 / n, 0.9, 3, 4)[3][1] == 1
    full = S.goss(np.abs(rng.standard_normal(n)).astype(np.float32) + 1, h + 1, 0.5, 0.5, 3, 4)
    assert full[2].all() and full[3][1] == 500                                             # other_rate / (1 - top_rate) = 1: every row kept


def test_partition_mask_restatement_is_stable():
    rng = np.random.default_rng(2)
    mask = (rng.random(500) < 0.4).astype(np.uint8)
    out, kept = S.partition_mask(mask)
    assert kept == mask.sum() and np.array_equal(out[:kept], np.nonzero(mask)[0]) and np.array_equal(out[kept:], np.nonzero(mask == 0)[0])
    rows = rng.permutation(700)[:300].astype(np.int32) - 100                             # some below 0, some beyond the mask
    out, kept = S.partition_mask(mask, rows)
    inside = (rows >= 0) & (rows < 500)
    keep = inside & (mask[np.clip(rows, 0, 499)] != 0)
    assert np.array_equal(out[:kept], rows[keep]) and np.array_equal(out[kept:], rows[~keep]) and (~inside).any()


def test_binned_walk_is_the_raw_walk_and_sampled_growth_is_growth_on_the_subset():
    rng = np.random.default_rng(3)
    n, nf, max_bin = 1200, 5, 31
    X = rng.standard_normal((n, nf)).astype(np.float32)
    X[:, 2] = np.round(X[:, 2] * 3)
    y = (X[:, 0] + (X[:, 1] > 0.3) * 1.5 - 0.4 * X[:, 2] + 0.2 * rng.standard_normal(n)).astype(np.float32)
    edges, nbins = R.bin_edges(X, max_bin)
    bins = R.bin_matrix(X, edges, nbins)
    params = {"max_bin": max_bin, "num_leaves": 8, "min_data_in_leaf": 10, "learning_rate": 0.5, "bagging_fraction": 0.5, "bagging_freq": 1}
    for policy in ("leafwise", "depthwise"):
        tree, mask, add, _ = S.grow(bins, -y, np.ones(n, np.float32), edges, nbins, dict(params, grow_policy=policy), 0)
        assert 0 < mask.sum() < n and tree["feature"].size == 7
        assert np.array_equal(add.view(np.int32), R.predict(X, [tree]).view(np.int32))       # x <= edge is bin <= b, out of the bag too
    # malformed trees give NaN and a single leaf gives its value
    v = np.array([1.0, 2.0], np.float32)
    assert np.isnan(S.walk_binned(bins, [0], [3], [5], [~1], v)[bins[:, 0] <= 3]).all()
    assert np.isnan(S.walk_binned(bins, [0], [3], [0], [0], v)).all()                      # a cycle
    assert (S.walk_binned(bins, [], [], [], [], v[:1]) == 1.0).all()
    # GOSS warms up on every row
    gp = {"max_bin": max_bin, "num_leaves": 8, "data_sample_strategy": "goss", "learning_rate": 0.5}
    assert S.tree_mask(gp, 1, -y, np.ones(n, np.float32))[2] is None and S.tree_mask(gp, 2, -y, np.ones(n, np.float32))[2] is not None
