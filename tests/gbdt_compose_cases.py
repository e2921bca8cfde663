"""The composed cases of the native GBDT: a written-out table in which every pair of option values that ptranking_amd.gbdt._params accepts
meets in at least one case (test_gbdt_compose_cpu.py proves it from AXES), their data, and the parameters each case hands the booster.
Test infrastructure, never imported by the package; it needs no GPU."""
import functools

import numpy as np

import gbdt_cat_ref as CR
import gbdt_missing_ref as MR
import gbdt_sample_ref as S

AXES = {"grow_policy": ("leafwise", "depthwise"), "use_missing": (False, True), "categorical": (False, True), "monotone": (False, True),
        "interaction": (False, True), "sampling": ("none", "bagging", "by_query", "goss"), "quant": ("off", "on", "renew"), "quant_bins": (4, 16),
        "boosting": ("gbdt", "dart"), "linear": (False, True)}
# what _params refuses today (goss x bagging are two values of ONE axis here, so no case could hold them)
REFUSED = {frozenset(pair) for pair in ((("boosting", "dart"), ("categorical", True)), (("boosting", "dart"), ("linear", True)),
                                        (("linear", True), ("categorical", True)), (("linear", True), ("monotone", True)),
                                        (("linear", True), ("quant", "renew")), (("quant", "renew"), ("monotone", True)))}

N, F_, QUERIES, MAX_BIN, ROUNDS, DART_ROUNDS = 600, 8, 20, 31, 3, 5
CATS, MONO, GROUPS = (1, 4), (1, 0, 0, -1, 0, 0, 0, 0), ((0, 1, 2, 3), (2, 3, 4, 5, 6))      # the groups overlap in 2 and 3; 7 is in none
BASE = {"max_bin": MAX_BIN, "num_leaves": 8, "min_data_in_leaf": 10, "learning_rate": 0.3}
DART = {"drop_rate": 0.5, "drop_seed": 5}                              # test_gbdt_dart_cpu.py: why seed 5

_ = False
# name: (grow_policy, use_missing, categorical, monotone, interaction, sampling, quant, quant_bins, boosting, linear, seed).  The seed draws the
# target's noise; it is the first from 0 under which every honesty condition of test_gbdt_compose_cpu.py holds for the case.
TABLE = {
    "depth_miss_cat_inter":        ("depthwise", True, True, _, True, "none", "off", 4, "gbdt", _, 0),
    "plain":                       ("leafwise", _, _, _, _, "none", "off", 4, "gbdt", _, 0),
    "depth_dart_mono_bag_q16":     ("depthwise", True, _, True, _, "bagging", "on", 16, "dart", _, 1),
    "linear_inter_byquery_q16":    ("leafwise", _, _, _, True, "by_query", "on", 16, "gbdt", True, 0),
    "depth_dart_goss_renew_inter": ("depthwise", _, _, _, True, "goss", "renew", 4, "dart", _, 0),
    "cat_mono_goss_q16":           ("leafwise", _, True, True, _, "goss", "on", 16, "gbdt", _, 1),
    "miss_cat_inter_bag_renew":    ("leafwise", True, True, _, True, "bagging", "renew", 4, "gbdt", _, 0),
    "dart_miss_mono_byquery":      ("leafwise", True, _, True, _, "by_query", "off", 4, "dart", _, 0),
    "depth_linear_miss_goss":      ("depthwise", True, _, _, _, "goss", "off", 16, "gbdt", True, 0),
    "depth_dart_mono_inter_q16":   ("depthwise", _, _, True, True, "none", "on", 16, "dart", _, 0),
    "depth_miss_cat_byquery_r16":  ("depthwise", True, True, _, _, "by_query", "renew", 16, "gbdt", _, 0),
    "depth_linear_bag":            ("depthwise", _, _, _, _, "bagging", "off", 4, "gbdt", True, 0),
    "depth_linear_miss_q4":        ("depthwise", True, _, _, _, "none", "on", 4, "gbdt", True, 0),
    "depth_miss_cat_renew":        ("depthwise", True, True, _, _, "none", "renew", 4, "gbdt", _, 0),
    "all_constraints_miss_cat_q4": ("leafwise", True, True, True, True, "none", "on", 4, "gbdt", _, 0),
    "depth_all_constraints_goss":  ("depthwise", True, True, True, True, "goss", "off", 4, "gbdt", _, 0),
    "linear_miss_inter_bag":       ("leafwise", True, _, _, True, "bagging", "off", 4, "gbdt", True, 0),
    "dart_goss_renew_q16":         ("leafwise", True, _, _, _, "goss", "renew", 16, "dart", _, 0),
}
del _


def axis_values(name):
    return dict(zip(AXES, TABLE[name][:len(AXES)]))


def params_of(values, seed=0):
    """The booster's parameter dict for one value per axis (the `boosting` argument rides in the case, not in the dict)."""
    v = values
    p = dict(BASE, grow_policy=v["grow_policy"], num_grad_quant_bins=v["quant_bins"])
    if v["grow_policy"] == "depthwise":
        p["max_depth"] = 3                                             # num_leaves = 2^max_depth: the cap cannot bind
    if v["use_missing"]:
        p["use_missing"] = True
    if v["categorical"]:
        p.update(categorical_feature=list(CATS), cat_smooth=2.5)
    if v["monotone"]:
        p["monotone_constraints"] = list(MONO)
    if v["interaction"]:
        p["interaction_constraints"] = [list(g) for g in GROUPS]
    if v["sampling"] in ("bagging", "by_query"):
        p.update(bagging_fraction=0.6, bagging_freq=2, bagging_by_query=v["sampling"] == "by_query")
    if v["sampling"] == "goss":
        p.update(data_sample_strategy="goss", top_rate=0.3, other_rate=0.3, learning_rate=0.6)      # floor(1 / 0.6) = 1 warm-up tree
    if v["quant"] != "off":
        p.update(use_quantized_grad=True, quant_seed=5, quant_train_renew_leaf=v["quant"] == "renew")
    if v["boosting"] == "dart":
        p.update(DART)
    if v["linear"]:
        p["linear_tree"] = True
    return p


def minimal_params(pair):
    """The smallest dict that holds just the two axis values of `pair` -> (params, boosting argument)."""
    values = {a: vals[0] for a, vals in AXES.items()}
    values.update(dict(pair))
    full, plain = params_of(values), params_of({a: vals[0] for a, vals in AXES.items()})
    keep = {k: v for k, v in full.items() if k not in plain or plain[k] != v}
    return keep, values["boosting"]


@functools.lru_cache(maxsize=None)
def matrix(use_missing, categorical):
    """One training matrix per (use_missing, categorical), float32 [600, 8]: 0 and 3 carry the monotone constraints, 1 and 4 hold integer
    codes 0 .. 11 (numeric columns where the case names no categories), 2 and 4 hold about 10 % NaN under use_missing, 6 has five distinct
    values, 7 is constant; and 200 fresh rows with NaNs, codes the training data never held and values on bin edges."""
    rng = np.random.default_rng([7, int(use_missing), int(categorical)])
    X = rng.standard_normal((N, F_)).astype(np.float32)
    X[:, 1], X[:, 4] = rng.integers(0, 12, N), rng.integers(0, 12, N)
    X[:, 6], X[:, 7] = rng.integers(0, 5, N) * 0.5, 0.25
    nan = np.zeros((N, F_), bool)
    if use_missing:
        nan[:, [2, 4]] = rng.random((N, 2)) < 0.1
    X[nan] = np.nan
    X.setflags(write=False)
    return X


def target(X, seed):
    """Monotone up in column 0 and down in column 3, an interaction of 0 (group one alone) with 5 (group two alone), effects of the codes of
    1 and 4 and of a NaN in 2 or 4, a step in 2, a slope in 6, and the seed's noise."""
    rng = np.random.default_rng([11, seed])
    z = np.nan_to_num(X.astype(np.float64))
    e1, e4 = np.array([0.0, 1.5, -1.0, 0.5, 2.0, -0.5, 1.0, -1.5, 0.25, 1.25, -0.75, 0.75]), np.array([1.0, -1.0, 0.5, 0.0, 1.5, -0.5, 0.0, 1.0, -1.5, 0.5, 2.0, -2.0])
    y = 1.2 * z[:, 0] - 1.0 * z[:, 3] + 0.9 * z[:, 0] * z[:, 5] + e1[z[:, 1].astype(int)] + 0.8 * (z[:, 2] > 0.3) + 0.4 * z[:, 6]
    y = y + np.where(np.isnan(X[:, 4]), 1.2, 0.6 * e4[z[:, 4].astype(int)]) + np.where(np.isnan(X[:, 2]), -1.0, 0.0)
    return (y + 0.5 * rng.standard_normal(X.shape[0])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def binned(use_missing, categorical):
    X = matrix(use_missing, categorical)
    cats = CATS if categorical else ()
    edges, nbins, nan_bin = CR.bin_edges(X, MAX_BIN, cats, use_missing)
    is_cat = np.zeros(F_, bool)
    is_cat[list(cats)] = True
    bins = MR.bin_matrix(X, edges, nbins, nan_bin)
    for a in (edges, nbins, nan_bin, is_cat, bins):
        a.setflags(write=False)
    return dict(X=X, edges=edges, nbins=nbins, nan_bin=nan_bin if use_missing else None, is_cat=is_cat, bins=bins,
                group=np.full(QUERIES, N // QUERIES), qid=S.group_qid(np.full(QUERIES, N // QUERIES)))


def fresh(use_missing, categorical, edges):
    """200 fresh rows: NaNs in every column under use_missing (in columns whose training data held none too), codes 12 .. 15 the training
    data never held, and values exactly on bin edges."""
    rng = np.random.default_rng([13, int(use_missing), int(categorical)])
    X = rng.standard_normal((200, F_)).astype(np.float32)
    X[:, 1], X[:, 4] = rng.integers(0, 16, 200), rng.integers(0, 16, 200)
    X[:, 6], X[:, 7] = rng.integers(0, 5, 200) * 0.5, 0.25
    for f in (0, 2, 3, 5):
        k = int(np.isfinite(edges[f]).sum())
        X[:40, f] = edges[f, rng.integers(0, k, 40)]
    if use_missing:
        X[rng.random(X.shape) < 0.1] = np.nan
    return X


def case(name, seed=None):
    """dict(name, values, params, boosting, rounds, seed, data): what gbdt_compose_ref.fit drives."""
    values = axis_values(name)
    seed = TABLE[name][-1] if seed is None else seed
    d = dict(binned(values["use_missing"], values["categorical"]))
    d["y"] = target(d["X"], seed)
    d["fresh"] = fresh(values["use_missing"], values["categorical"], d["edges"])
    return dict(name=name, values=values, params=params_of(values), boosting=values["boosting"], rounds=DART_ROUNDS if values["boosting"] == "dart" else ROUNDS,
                seed=seed, data=d)


CASES = list(TABLE)
