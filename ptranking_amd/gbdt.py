"""A native LambdaMART: a histogram gradient-boosted tree trainer on the GPU (csrc/gbdt.hip) under the tree frame's objectives (csrc/tree.hip).

The reference's tree frame (ptranking/ltr_tree/lambdamart/lightgbm_lambdaMART.py) parses files, hands the boosting to LightGBM and predicts the
test set.  LightGBM is not installed where this package is developed or tested, so nothing here is compared with it, and no parity is
claimed: the binning rule, the tie rules and the model file are this project's own.  What is pinned from outside is the
booster's whole fits against scikit-learn's trees (tests/golden/gbdt_sklearn.npz): under squared error, on features of no more distinct
values than bins, every tree equals HistGradientBoostingRegressor's node for node (growth order, sibling subtraction, leaf values,
learning rate, the accumulation over rounds), and one tree equals DecisionTreeRegressor's exact greedy best-first tree.  Not pinned:
LightGBM itself, the quantile binning rule for features of more distinct values than bins, and the ranking objectives inside the booster.

    GBDT(params)       the booster: fit_bins(X) bins the features once and keeps them resident; update(grad, hess) grows ONE tree (leaf-wise, or
                        depth-wise under grow_policy='depthwise') from device gradients and adds its leaf values to the resident training scores; predict / save_model / load_model
    LambdaMART(params)  the ranker: every round computes the gradient and the Hessian per document with tree_pair_grad_hess /
                        tree_listnet_grad_hess / tree_lambdarank_ndcg_grad_hess / tree_xendcg_grad_hess on the resident scores (no host copy), quantizes them and calls update

Growth policies (grow_policy): 'leafwise', the default, splits the leaf of the largest gain and reads the two children's records back after
every split; 'depthwise' splits ALL leaves of a level in one batched pass (partition, histograms of the smaller children, sibling
subtraction, split scan over many leaves at once) and reads once per level; under the leaf cap it keeps the level's largest gains.  Where
the cap cannot bind (num_leaves >= 2^max_depth) the two give the same trees, fp32 leaf values and scores bit for bit; depth-wise whole fits
are pinned to scikit-learn with max_leaf_nodes=None as well (tests/golden/gbdt_sklearn_depth.npz).  GBDT.host_reads counts the reads.

Row sampling (LightGBM's names; the rules are this project's own, stated in include/ptranking_amd.h and restated in
tests/gbdt_sample_ref.py; no parity with LightGBM's random streams is claimed).  bagging_fraction < 1 with bagging_freq = k > 0 grows tree
t on a Bernoulli bag of the rows (of whole queries under bagging_by_query, which needs fit_bins(X, group)), redrawn before the trees
0, k, 2k, ... from the counter stream seeded by bagging_seed.  data_sample_strategy='goss' keeps, after the first floor(1 / learning_rate)
trees, the rows at or above the exact K-th largest |g h| (K = floor(n top_rate)) and any other row with probability
other_rate / (1 - top_rate), its gradient and Hessian times (1 - top_rate) / other_rate; it cannot be combined with bagging.  The mask, the
select, the stable partition that puts the bag at the front of the row list and the walk that gives the rows outside the bag their leaf
value all run on the device; the size of the bag reaches the host in the one read update() makes anyway (it is the root's row count), so
host_reads does not grow, and booster.scores stays predict(X) bit for bit for every row.  Without sampling update() issues exactly the
calls it issued before these parameters existed.

Missing values (use_missing, LightGBM's name).  The default here is False: a NaN raises in bin_edges, in predict and for the eval_set of
LambdaMART.fit, and every call is the one made before the switch existed.  LightGBM's own default is True.  Under use_missing=True a NaN
is a missing value (an infinity still raises): a feature that holds one in the training matrix keeps a NaN bin behind its value bins
(bin_edges gives it at most max_bin - 1 of those), the split scan tries every threshold with the missing rows on the right and, where
the node holds missing rows, also the NaNs against all values and every threshold with them on the left, and each node keeps the
direction that won (default_left), or the side of the larger child where its rows do not decide.  predict sends a NaN along default_left.
The rules are scikit-learn's wherever its are deterministic, and whole fits on data with NaNs are pinned to HistGradientBoostingRegressor
node for node (tests/golden/gbdt_sklearn_missing.npz; include/ptranking_amd.h states the rules, tests/gbdt_missing_ref.py restates
them).  Such a model is saved as format 2 (format 1 with default_left per node and nan_bin per feature); a model without the switch saves
the format-1 file it always did.  Not here: zero_as_missing, and the LETOR loader's absent features, which stay zeros.

The truncated, normalised lambdarank: LambdaMART(objective='lambdarank_ndcg').  The reference's tree frame runs LightGBM's BUILT-IN
objective='lambdarank' by default (lightgbm_lambdaMART.py:170-185); 'lambdarank_ndcg' is this project's own rule modelled on that objective
(LightGBM's LambdarankNDCG), stated in include/ptranking_amd.h and restated in tests/lambdarank_ndcg_ref.py.  It is compared with nothing of
LightGBM's and no parity is claimed.  A pair counts where the labels differ and one of its documents ranks in the first
lambdarank_truncation_level (30); its weight is the Delta-nDCG against maxDCG at that level, divided by 0.01 + |score difference| under
lambdarank_norm (True); lam = sigmoid w p, h = sigmoid^2 w p (1 - p) (sigmoid 1.0); under lambdarank_norm a query's results are scaled by
log2(1 + S) / S, S = 2 sum lam.  The three settings come from the parameter dict under LightGBM's names; the other objectives and the bare
booster ignore them.  The key 'objective' of the dict stays ignored (the objective is LambdaMART's argument, and its default stays
'lambdarank', the reference's CUSTOM all-pairs objective), and label_gain stays unknown (the gain is 2^y - 1).  A model file written before
the three keys existed loads with their defaults.

Cross-entropy nDCG: LambdaMART(objective='rank_xendcg'), LightGBM's other built-in ranking objective (Bruch, "An Alternative Cross Entropy
Loss for Learning-to-Rank"): O(n) per query where lambdarank costs O(n T).  The rule is this project's own, modelled on LightGBM's
RankXENDCG, stated in include/ptranking_amd.h and restated in tests/xendcg_ref.py; it is compared with nothing of LightGBM's and no parity is
claimed (its random stream in particular is not LightGBM's).  rho = softmax(scores) per query, phi = 2^y - u with one uniform u in [0, 1)
per document and round, q = max(1 - rho, 2^-20) (the floor is this project's addition: LightGBM divides by 1 - rho unguarded; here every
output is finite); a = rho - phi / sum phi, b = rho (A - a / q), c = rho (Bs - b / q) with A = sum a / q, Bs = sum b / q; grad = a + b + c,
hess = rho (1 - rho).  The uniforms come from the counter stream bagging uses, keyed by (objective_seed, the tree counter, the document's
row): objective_seed (5, LightGBM's name and default) is read by this objective alone, round t draws with draw = t = the trees grown so
far, so a fit continued through init_model goes on in the stream where the first fit stopped and equals the unsplit fit bit for bit, and
refit re-estimates tree t under draw t.  weighting, hessian, pair_type, epsilon and gain_type do not apply.  A model file written before
the key existed loads with the default.

Categorical features (categorical_feature, a list of 0-based column indices; cat_smooth, default 10.0; LightGBM's names).  Such a column
holds integer codes in 0 .. max_bin - 1 (bin_edges maps code c to bin c), and a node on it sends a SET of codes left.  The rules are
scikit-learn's (HistGradientBoostingRegressor(categorical_features=...)) wherever its are deterministic, stated in
include/ptranking_amd.h and restated in tests/gbdt_cat_ref.py: at a node a category is used iff H_c TC / TH >= cat_smooth, the used
categories are sorted by G_c / (H_c + cat_smooth) (equal keys by the lower code: this project's own tie rule), and the candidates are the
first or the last i + 1 of them up to the middle; unused categories and empty bins go right.  cat_smooth plays both roles of
scikit-learn's MIN_CAT_SUPPORT.  Under use_missing a NaN of such a column is one more category.  Whole fits are pinned to scikit-learn
node for node, left sets included (tests/golden/gbdt_sklearn_cat.npz); LightGBM's own categorical search is not claimed.  A tree then keeps
cat_index per node (-1: numeric) and cat_set [sets, 4] int64, 256 bits per set; the model is saved as format 3.  predict sends a code
the training data never held right (it is in no set).  With categorical_feature empty every call and every model file is the one made
before the keys existed.  Not here: max_cat_to_onehot, cat_l2, min_data_per_group, max_cat_threshold.

Monotone constraints (monotone_constraints, a sequence of -1 / 0 / +1, one per feature; LightGBM's name) and interaction constraints
(interaction_constraints, a sequence of groups of 0-based column indices).  Both are training-time rules: a tree, predict and the model
format numbers do not change.  The rules are scikit-learn's (HistGradientBoostingRegressor(monotonic_cst=..., interaction_cst=...)) wherever
its are deterministic, which is LightGBM's monotone_constraints_method 'basic' (the only method here); include/ptranking_amd.h states them
and tests/gbdt_cst_ref.py restates them.  Every node keeps (lo, hi, v) in float64: the bounds of its children's values and its own value.
Under active monotone constraints every split search of the fit uses the bounded gain on every candidate: vL = clamp(-GL / (HL + l2), lo,
hi) and vR likewise, the candidate rejected where vL > vR under +1 or vL < vR under -1, gain = G v - GL vL - GR vR; the children of a
split on a constrained feature share the bound mid = (vL + vR) / 2, and a leaf stores float32(v * learning_rate) with its clamped v.
predict is then non-decreasing (+1) or non-increasing (-1) in the feature, exactly.  A categorical column takes no monotone constraint.
Under interaction constraints a child of a split on f keeps the groups that contain f and may split on their union only; features in
no group form one more group (scikit-learn's rule: LightGBM's own treatment of unlisted features is not claimed).  The host computes the
children's (lo, hi, v) from the integer sums of the record it has read anyway and uploads small tables before each search, so host_reads
does not grow.  Whole fits are pinned to scikit-learn node for node (tests/golden/gbdt_sklearn_cst.npz).  With all constraints zero and no
groups every call and every model file is the one made before the keys existed.  Not here: the methods 'intermediate' and 'advanced',
monotone_penalty.

Feature contributions (LightGBM's predict(pred_contrib=True) and feature_importance()).  predict(X, pred_contrib=True) returns device
float64 [n, F + 1]: path-dependent TreeSHAP (Lundberg et al., Algorithm 2) per feature and the expected value in the last column, so a
row's entries sum to its score.  The rule is stated in include/ptranking_amd.h and restated twice in tests/gbdt_shap_ref.py (the Shapley
definition itself, exponential in the features of a tree, and the polynomial recurrences in the kernel's order of operations); nothing is
compared with LightGBM or the shap package.  TreeSHAP weighs the two children of a node by their covers, and neither a tree nor the
pinned model files keep row counts: set_background(X) walks a background matrix through every tree in one launch, counts its rows per
leaf with integer atomics, and the host sums them into covers and builds one path-table row per leaf (the path's nodes with their
directions, the distinct features as elements with their zero fractions, the leaf value).  The training matrix gives the counts the trees
were grown on (x <= edge is bin <= b).  The kernel gives a row to one wavefront, one lane per element of a path (at most 63 distinct
features on a path; depth is free), and sums in float64 in LDS in leaf order: no float atomic, and a row's bits do not depend on the
batch.  The covers live in memory only: a loaded or a grown booster calls set_background again, and pred_contrib=True without one raises.
feature_importance('split') counts the splits per feature on the host; 'gain' raises, since the trees keep no gains.  With
pred_contrib=False every call is the one made before the flag existed.

A trained model on new data (LightGBM's init_model, Booster.refit and predict(pred_leaf=True); the rules are this project's own, stated
in include/ptranking_amd.h and restated in tests/gbdt_lifecycle_ref.py; nothing is compared with LightGBM).  predict(X, pred_leaf=True)
returns device int32 [n, trees]: the index of the leaf each tree puts each row in, by the walk predict itself makes
(ptr_gbdt_predict_leaf), so value[leaf] summed in tree order in fp32 is the score.  fit_bins(X, init_model=...) and
LambdaMART.fit(..., init_model=...) continue a GBDT, a LambdaMART or a saved model on X: the bins are the model's (the trainer must share
max_bin, use_missing and categorical_feature with it; a categorical code above the model's largest, or a NaN in a feature the model keeps
no NaN bin for, raises), the trees are copies of those predict uses by default, the resident scores start at predict(X), and the tree
counter goes on (the bagging draws and GOSS's warm-up count all trees; evals_result holds the added rounds and best_iteration counts all
trees).  Since every decision rests on integer sums, a fit split in two (train, save, load, continue) gives the trees, values and scores
of the unsplit fit bit for bit.  refit(X, grad_hess, decay_rate=0.9) returns a NEW booster with the same structures whose leaf values are
re-estimated on X tree by tree: gradients at the running scores, ptr_gbdt_quantize, the per-leaf integer sums of ptr_gbdt_leaf_sums
(LDS cells per workgroup up to 1024 leaves, global integer atomics beyond), one host read per tree, value = float32(decay_rate * old +
(1 - decay_rate) * (-G / (H + lambda_l2) * learning_rate)) in float64, a leaf no row reaches keeping its value, then ptr_gbdt_add_by_leaf;
on the training data with decay_rate=0 an unsampled, unconstrained model gets its own values back bit for bit.  Monotone constraints
refuse refit.  LambdaMART.refit(X, y, group) supplies the ranker's objective.  With init_model=None and pred_leaf=False every call and
every model file is the one made before they existed; a continued or refitted model saves in the same three formats.

Everything a tree decides rests on integer sums (ptr_gbdt_quantize), so two fits of the same data give the same bits.  Not here:
feature_fraction, EFB, DART.  There is no CPU path.
"""
import copy
import json

import numpy as np
import torch

from . import functional as F
from . import letor, tree

__all__ = ["GBDT", "LambdaMART", "bin_edges", "DEFAULT_PARAMS", "IGNORED_PARAMS", "constraints", "shap_tables", "SHAP_MAX_ELEMENTS"]

# LightGBM's names, so the reference's lightgbm_para_dict passes through.  min_sum_hessian_in_leaf = 1e-3 is LightGBM's default too; the
# reference's own dict sets 200, which suits LightGBM's built-in lambdarank Hessians, not the sums of tree.hip.
DEFAULT_PARAMS = {"learning_rate": 0.1, "num_leaves": 31, "num_trees": 100, "min_data_in_leaf": 20, "min_sum_hessian_in_leaf": 1e-3,
                  "lambda_l2": 0.0, "min_gain_to_split": 0.0, "max_bin": 255, "max_depth": -1, "grow_policy": "leafwise",
                  "bagging_fraction": 1.0, "bagging_freq": 0, "bagging_seed": 3, "bagging_by_query": False, "data_sample_strategy": "bagging",
                  "top_rate": 0.2, "other_rate": 0.1, "use_missing": False, "categorical_feature": (), "cat_smooth": 10.0,
                  "monotone_constraints": (), "monotone_constraints_method": "basic", "interaction_constraints": (),
                  # LambdaMART(objective='lambdarank_ndcg') alone reads these three; the other objectives and the bare booster ignore them
                  "lambdarank_truncation_level": 30, "lambdarank_norm": True, "sigmoid": 1.0,
                  "objective_seed": 5}                    # LambdaMART(objective='rank_xendcg') alone reads it
IGNORED_PARAMS = ("num_threads", "verbosity", "metric", "boosting_type", "objective", "eval_at")    # accepted, without a meaning here
MODEL_FORMAT = 1                       # a model trained without use_missing
MODEL_FORMAT_MISSING = 2               # one trained under it: format 1 with default_left per node and nan_bin per feature
MODEL_FORMAT_CAT = 3                   # one with categorical features: format 1 or 2 plus categorical_feature, cat_index per node and cat_sets
CAT_KEYS = ("categorical_feature", "cat_smooth")      # not among the parameters of a format 1 or 2 file
CST_KEYS = ("monotone_constraints", "monotone_constraints_method", "interaction_constraints")   # in a model file only where one is active
MONOTONE_METHODS = ("basic",)
GROW_POLICIES = ("leafwise", "depthwise")
SHAP_MAX_ELEMENTS = 63                 # distinct features on one root-to-leaf path: one lane each, within the quadrature rules of up to 32 nodes
SAMPLE_STRATEGIES = ("bagging", "goss")


def _params(params):
    p = dict(DEFAULT_PARAMS)
    for k, v in (params or {}).items():
        if k == "boosting_type" and v != "gbdt":
            raise ValueError(f"boosting_type {v!r} is not implemented: only 'gbdt'")
        if k in IGNORED_PARAMS:
            continue
        if k not in DEFAULT_PARAMS:
            raise ValueError(f"unknown parameter {k!r} (known: {', '.join(DEFAULT_PARAMS)}; ignored: {', '.join(IGNORED_PARAMS)})")
        p[k] = v
    p["max_depth"] = -1 if p["max_depth"] is None else int(p["max_depth"])
    for k in ("num_leaves", "num_trees", "min_data_in_leaf", "max_bin"):
        p[k] = int(p[k])
    for k in ("learning_rate", "min_sum_hessian_in_leaf", "lambda_l2", "min_gain_to_split"):
        p[k] = float(p[k])
    if p["grow_policy"] not in GROW_POLICIES:
        raise ValueError(f"grow_policy {p['grow_policy']!r} is not implemented: only 'leafwise' and 'depthwise'")
    if not p["learning_rate"] > 0.0:
        raise ValueError(f"learning_rate must be > 0, got {p['learning_rate']}")
    if p["num_leaves"] < 1 or p["num_trees"] < 0 or p["min_data_in_leaf"] < 0:
        raise ValueError("num_leaves must be >= 1, num_trees and min_data_in_leaf >= 0")
    if not 2 <= p["max_bin"] <= F.GBDT_MAX_BIN:
        raise ValueError(f"max_bin must be in 2 .. {F.GBDT_MAX_BIN}, got {p['max_bin']}")
    if not p["lambda_l2"] >= 0.0 or p["min_sum_hessian_in_leaf"] != p["min_sum_hessian_in_leaf"] or p["min_gain_to_split"] != p["min_gain_to_split"]:
        raise ValueError("lambda_l2 must be >= 0 and no threshold may be NaN")
    for k in ("bagging_fraction", "top_rate", "other_rate"):
        p[k] = float(p[k])
    for k in ("bagging_by_query", "use_missing"):
        if isinstance(p[k], (bool, np.bool_)):
            p[k] = bool(p[k])
        else:
            raise ValueError(f"{k} must be True or False, got {p[k]!r}")
    if int(p["bagging_freq"]) != p["bagging_freq"] or int(p["bagging_seed"]) != p["bagging_seed"]:
        raise ValueError("bagging_freq and bagging_seed must be integers")
    p["bagging_freq"], p["bagging_seed"] = int(p["bagging_freq"]), int(p["bagging_seed"])
    if not 0.0 < p["bagging_fraction"] <= 1.0:
        raise ValueError(f"bagging_fraction must be in (0, 1], got {p['bagging_fraction']}")
    if p["bagging_freq"] < 0 or p["bagging_seed"] < 0:
        raise ValueError("bagging_freq and bagging_seed must be >= 0")
    if p["data_sample_strategy"] not in SAMPLE_STRATEGIES:
        raise ValueError(f"data_sample_strategy {p['data_sample_strategy']!r} is not implemented: only 'bagging' and 'goss'")
    if not (p["top_rate"] > 0.0 and p["other_rate"] > 0.0 and p["top_rate"] + p["other_rate"] <= 1.0):
        raise ValueError(f"top_rate and other_rate must be > 0 and sum to at most 1, got {p['top_rate']}, {p['other_rate']}")
    if p["data_sample_strategy"] == "goss" and _bagging(p):
        raise ValueError("data_sample_strategy 'goss' cannot be combined with bagging (bagging_freq > 0 and bagging_fraction < 1)")
    p["categorical_feature"] = _categorical(p["categorical_feature"])
    try:
        p["cat_smooth"] = float(p["cat_smooth"])
    except (TypeError, ValueError):
        raise ValueError(f"cat_smooth must be a number >= 0, got {p['cat_smooth']!r}") from None
    if not 0.0 <= p["cat_smooth"] < np.inf:
        raise ValueError(f"cat_smooth must be a finite number >= 0, got {p['cat_smooth']}")
    p["monotone_constraints"] = _monotone(p["monotone_constraints"])
    if p["monotone_constraints_method"] not in MONOTONE_METHODS:
        raise ValueError(f"monotone_constraints_method {p['monotone_constraints_method']!r} is not implemented: only 'basic'")
    for c in p["categorical_feature"]:
        if c < len(p["monotone_constraints"]) and p["monotone_constraints"][c] != 0:
            raise ValueError(f"monotone_constraints: column {c} is categorical, it takes no monotone constraint")
    p["interaction_constraints"] = _interaction(p["interaction_constraints"])
    p["lambdarank_truncation_level"], p["sigmoid"], p["lambdarank_norm"] = F.lambdarank_ndcg_settings(p["lambdarank_truncation_level"], p["sigmoid"],
                                                                                                   p["lambdarank_norm"])
    p["objective_seed"] = F.objective_seed(p["objective_seed"])
    return p


def _categorical(cat):
    """categorical_feature as a sorted tuple of ints; a duplicate, negative or non-integer entry raises ValueError."""
    if cat is None:
        return ()
    if isinstance(cat, (str, bytes)) or not isinstance(cat, (list, tuple, np.ndarray)):
        raise ValueError(f"categorical_feature must be a list or tuple of 0-based column indices, got {cat!r}")
    out = []
    for c in np.asarray(cat, dtype=object).reshape(-1).tolist() if isinstance(cat, np.ndarray) else cat:
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)):
            raise ValueError(f"categorical_feature must hold integers, got {c!r}")
        if c < 0:
            raise ValueError(f"categorical_feature must hold 0-based column indices, got {c}")
        out.append(int(c))
    if len(set(out)) != len(out):
        raise ValueError(f"categorical_feature holds a column twice: {sorted(out)}")
    return tuple(sorted(out))


def _sequence(name, v, what):
    if v is None:
        return []
    if isinstance(v, (str, bytes)) or not isinstance(v, (list, tuple, np.ndarray)):
        raise ValueError(f"{name} must be a list or tuple of {what}, got {v!r}")
    return np.asarray(v, dtype=object).reshape(-1).tolist() if isinstance(v, np.ndarray) and v.dtype != object else list(v)


def _monotone(mono):
    """monotone_constraints as a tuple of -1 / 0 / +1; anything else raises ValueError."""
    out = []
    for c in _sequence("monotone_constraints", mono, "-1 / 0 / +1, one per feature"):
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) or c not in (-1, 0, 1):
            raise ValueError(f"monotone_constraints must hold -1, 0 or +1, got {c!r}")
        out.append(int(c))
    return tuple(out)


def _interaction(groups):
    """interaction_constraints as a tuple of sorted tuples of ints; an empty group or a negative or non-integer entry raises ValueError."""
    out = []
    for g in (groups if isinstance(groups, np.ndarray) and groups.ndim == 2 else _sequence("interaction_constraints", groups, "groups of 0-based column indices")):
        if isinstance(g, (set, frozenset)):
            g = sorted(g, key=repr)
        members = _sequence("interaction_constraints", g, "groups of 0-based column indices")
        if not members:
            raise ValueError("interaction_constraints holds an empty group")
        for c in members:
            if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)):
                raise ValueError(f"interaction_constraints must hold integers, got {c!r}")
            if c < 0:
                raise ValueError(f"interaction_constraints must hold 0-based column indices, got {c}")
        out.append(tuple(sorted({int(c) for c in members})))
    return tuple(out)


def constraints(p):
    """The constraints the parameters switch on, a tuple out of 'monotone' and 'interaction': () with every monotone constraint 0 (or none
    given) and no group."""
    return (("monotone",) if any(p["monotone_constraints"]) else ()) + (("interaction",) if p["interaction_constraints"] else ())


def _interaction_groups(p, nf):
    """The groups as sets over nf features, the features in no group as one more group (scikit-learn's rule); an index >= nf raises."""
    groups = [frozenset(g) for g in p["interaction_constraints"]]
    for g in groups:
        if max(g) >= nf:
            raise ValueError(f"interaction_constraints {max(g)} with {nf} columns")
    rest = frozenset(range(nf)) - frozenset().union(*groups)
    return groups + ([rest] if rest else [])


def _bagging(p):
    return p["bagging_freq"] > 0 and p["bagging_fraction"] < 1.0


def sampling(p):
    """None, 'bagging' or 'goss': the row sampling the parameters switch on.  bagging_freq > 0 with bagging_fraction 1.0 switches nothing on."""
    return "goss" if p["data_sample_strategy"] == "goss" else "bagging" if _bagging(p) else None


_NONFINITE = "X holds a NaN or an infinity: missing values are not handled, impute them first"
_INFINITE = "X holds an infinity: under use_missing a NaN is a missing value, an infinity is not handled"


def _require_finite(Xd):
    """Raises bin_edges' ValueError for a NaN or an infinity in a device matrix: one reduction (the minimum and the maximum, which a NaN
    poisons) and one host read."""
    if Xd.numel() and not bool(torch.isfinite(torch.stack(torch.aminmax(Xd)).cpu()).all()):
        raise ValueError(_NONFINITE)


def _require_no_infinity(Xd):
    """The check under use_missing, where a NaN passes: raises for an infinity in a device matrix; one reduction and one host read."""
    if Xd.numel() and bool(torch.isinf(Xd).any().cpu()):
        raise ValueError(_INFINITE)


def _not_codes(max_bin):
    return f"a categorical column must hold integer codes in 0 .. {max_bin - 1} (under use_missing a NaN too, and then codes up to max_bin - 2)"


def _require_values(Xd, use_missing, categorical=(), max_bin=F.GBDT_MAX_BIN):
    """The check a device matrix passes before it is walked: no infinity under use_missing, nothing but finite values without it; in a
    categorical column nothing but integer codes in 0 .. max_bin - 1 (a NaN passes under use_missing), for one more reduction and read."""
    _require_no_infinity(Xd) if use_missing else _require_finite(Xd)
    if categorical and Xd.numel():
        if max(categorical) >= Xd.shape[1]:
            raise ValueError(f"categorical_feature {max(categorical)} with {Xd.shape[1]} columns")
        col = Xd[:, list(categorical)]
        ok = (col == torch.floor(col)) & (col >= 0) & (col <= max_bin - 1)
        if use_missing:
            ok |= torch.isnan(col)
        if not bool(ok.all().cpu()):
            raise ValueError(_not_codes(max_bin))


def _device_matrix(X, dev):
    """X (numpy array or tensor) as a contiguous float32 tensor on dev."""
    X = X.detach() if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
    return X.to(dev, torch.float32).contiguous()


def _midpoints(lo, hi):
    """An fp32 edge e with lo <= e < hi for adjacent distinct fp32 values: the midpoint, or lo where the midpoint rounds up to hi."""
    mid = ((lo.astype(np.float64) + hi.astype(np.float64)) * 0.5).astype(np.float32)
    return np.where(mid >= hi, lo, mid)


def bin_edges(X, max_bin, use_missing=False, categorical=()):
    """The binning rule, on the host, once per dataset -> (edges float32 [F, max_bin - 1], padded with +inf; nbins int32 [F]).
    Per feature: at most max_bin distinct values give one bin per value, the edges at the midpoints (binning is then lossless).  Otherwise
    the k-th edge (k = 1 .. max_bin - 1) follows the first distinct value whose cumulative row count reaches k n / max_bin, again at the
    midpoint to the next distinct value; edges that coincide are kept once.  Deterministic: no subsampling.
    use_missing=True -> (edges, nbins, nan_bin int32 [F]): a NaN is a missing value and takes no part in the rule (the distinct values, the
    counts and n are those of the feature's other rows).  A feature that holds one is binned under max_bin - 1 in place of max_bin, and
    its NaNs get the bin behind its value bins, nan_bin[f] = nbins[f] (nbins counts value bins only); a feature without a NaN has
    nan_bin[f] = -1 and the edges it has without the switch.  An infinity raises either way.
    categorical: the columns that hold integer codes.  Such a feature gets the edges 0.5, 1.5, ..., so that code c lands in bin c, and
    nbins[f] = the largest code + 1; a value that is no integer in 0 .. max_bin - 1 raises (0 .. max_bin - 2 where the column holds a NaN,
    whose bin stays behind the value bins)."""
    categorical = _categorical(categorical)
    X = np.asarray(X, dtype=np.float32)
    if X.ndim != 2:
        raise ValueError(f"X must be [rows, features], got {X.shape}")
    if use_missing:
        if np.isinf(X).any():
            raise ValueError(_INFINITE)
    elif not np.isfinite(X).all():
        raise ValueError(_NONFINITE)
    nf = X.shape[1]
    if categorical and categorical[-1] >= nf:
        raise ValueError(f"categorical_feature {categorical[-1]} with {nf} columns")
    edges = np.full((nf, max_bin - 1), np.inf, np.float32)
    nbins = np.ones(nf, np.int32)
    nan_bin = np.full(nf, -1, np.int32)
    for f in range(nf):
        col = X[:, f]
        cap = max_bin
        if use_missing and np.isnan(col).any():
            col, cap = col[~np.isnan(col)], max_bin - 1
        if f in categorical:
            if col.size and not ((col == np.floor(col)) & (col >= 0) & (col <= cap - 1)).all():
                raise ValueError(f"feature {f}: " + _not_codes(max_bin))
            top = int(col.max()) if col.size else 0
            edges[f, :top] = np.arange(top, dtype=np.float32) + np.float32(0.5)
            nbins[f] = top + 1
            if cap < max_bin:
                nan_bin[f] = nbins[f]
            continue
        n = col.size
        vals, counts = np.unique(col, return_counts=True)
        if vals.size > 1:
            if vals.size <= cap:
                cut = np.arange(vals.size - 1)
            else:
                cum = np.cumsum(counts)
                cut = np.unique(np.searchsorted(cum, np.arange(1, cap) * (n / cap), side="left"))
                cut = cut[cut < vals.size - 1]
            e = _midpoints(vals[cut], vals[cut + 1])
            edges[f, :e.size] = e
            nbins[f] = e.size + 1
        if cap < max_bin:
            nan_bin[f] = nbins[f]
    return (edges, nbins, nan_bin) if use_missing else (edges, nbins)


def leaf_value(g_sum, h_sum, expo, lambda_l2, learning_rate):
    """-G / (H + lambda_l2) * learning_rate in float64 from the integer sums, rounded to fp32; 0 where H + lambda_l2 is not positive (only a
    tree that never split can get there: the split scan's Hessian floor keeps every child positive)."""
    G, H = np.ldexp(float(g_sum), -int(expo[0])), np.ldexp(float(h_sum), -int(expo[1]))
    return np.float32(-G / (H + lambda_l2) * learning_rate) if H + lambda_l2 > 0.0 else np.float32(0.0)


def refit_value(old, g_sum, h_sum, count, expo, lambda_l2, learning_rate, decay_rate):
    """The value refit gives a leaf: float32(decay_rate * float64(old) + (1 - decay_rate) * new) with new = -G / (H + lambda_l2) *
    learning_rate in float64 from the integer sums, in leaf_value's order of operations.  A leaf no row reaches (count 0) or one with
    H + lambda_l2 <= 0 keeps old."""
    G, H = np.ldexp(float(g_sum), -int(expo[0])), np.ldexp(float(h_sum), -int(expo[1]))
    if int(count) <= 0 or not H + lambda_l2 > 0.0:
        return np.float32(old)
    new = -G / (H + lambda_l2) * learning_rate
    return np.float32(decay_rate * float(np.float32(old)) + (1.0 - decay_rate) * new)


def _decay_rate(decay_rate):
    try:
        decay = float(decay_rate)
    except (TypeError, ValueError):
        raise ValueError(f"decay_rate must be a number in [0, 1], got {decay_rate!r}") from None
    if not 0.0 <= decay <= 1.0:
        raise ValueError(f"decay_rate must be in [0, 1], got {decay_rate!r}")
    return decay


INIT_MODEL_KEYS = ("max_bin", "use_missing", "categorical_feature")    # what a trainer must share with the model it continues: they fix the bins


def _initial_model(init_model, params, device=None):
    """init_model (a GBDT, a LambdaMART or the path of a saved model) as a GBDT whose bins the parameters `params` can continue on; a
    difference in one of INIT_MODEL_KEYS raises ValueError naming the key.  Runs on the host."""
    model = init_model
    if isinstance(model, LambdaMART):
        model = model.booster
        if model is None:
            raise ValueError("init_model is a LambdaMART that has not been fitted")
    elif not isinstance(model, GBDT):
        if not isinstance(model, (str, bytes)) and not hasattr(model, "__fspath__"):
            raise ValueError(f"init_model must be a GBDT, a LambdaMART or the path of a saved model, got {type(init_model).__name__}")
        model = GBDT.load_model(model, device=device)
    for k in INIT_MODEL_KEYS:
        if params[k] != model.params[k]:
            raise ValueError(f"init_model was trained with {k}={model.params[k]!r}, this trainer has {k}={params[k]!r}: the bins would differ")
    if model.edges is None:
        raise ValueError("init_model holds no bin edges: fit_bins() or load_model() first")
    return model


def _copy_tree(t):
    return {k: np.array(v) for k, v in t.items()}


class _Leaf:
    __slots__ = ("start", "count", "depth", "slot", "parent", "side", "g", "h", "rec", "set", "cst", "groups")

    def __init__(self, start, count, depth, slot, parent, side, g, h, rec, set=None, cst=None, groups=None):
        self.start, self.count, self.depth, self.slot, self.parent, self.side, self.g, self.h, self.rec = start, count, depth, slot, parent, side, g, h, rec
        self.set = set                     # categorical features: the left set of rec, 4 int64 as the host read them
        self.cst = cst                     # monotone constraints: (lo, hi, v) float64, the bounds of the children's values and the leaf's own
        self.groups = groups               # interaction constraints: the indices of the leaf's active groups


def _record(r):
    """A split record as the host reads it: (gain float, feature, bin, left (g, h, count), right (g, h, count))."""
    r = np.asarray(r, np.int64)
    return float(r[:1].view(np.float64)[0]), int(r[1]), int(r[2]), tuple(int(v) for v in r[3:6]), tuple(int(v) for v in r[6:9])


_NO_SPLIT = (-np.inf, -1, -1, (0, 0, 0), (0, 0, 0))


def shap_tables(trees, leaf_counts):
    """The path tables of TreeSHAP (include/ptranking_amd.h documents the layout), numpy, one row per leaf in tree order, then leaf order.
    trees: tree dicts (feature, left, right, value); leaf_counts: per tree the rows of the background per leaf (int64 [nodes + 1]).  The
    cover of a node is the sum over the leaves below it.  z of an element = the product, in path order, of cover(child) / cover(node)
    over the path's nodes on its feature (float64).  Also -> tree_leaf_offsets int64 [trees + 1] and covers (per tree, per node).
    ValueError: a node or a leaf of cover 0, a path of more than SHAP_MAX_ELEMENTS distinct features, a tree that is no tree."""
    path_offsets, elem_offsets, leaf_value = [0], [0], []
    path_node, path_dir, path_elem, elem_feature, elem_z, covers = [], [], [], [], [], []
    base = 0
    for ti, (t, counts) in enumerate(zip(trees, leaf_counts)):
        feature, left, right = (np.asarray(t[k]).astype(np.int64) for k in ("feature", "left", "right"))
        nn = feature.size
        counts = np.asarray(counts).astype(np.int64).reshape(-1)
        if counts.size != nn + 1 or np.asarray(t["value"]).size != nn + 1:
            raise ValueError(f"tree {ti}: {nn} nodes with {np.asarray(t['value']).size} leaf values and {counts.size} leaf counts")
        up_node, up_leaf = np.full((nn, 2), -1, np.int64), np.full((nn + 1, 2), -1, np.int64)      # (parent, went left)
        for i in range(nn):
            for c, d in ((int(left[i]), 1), (int(right[i]), 0)):
                into, j = (up_leaf, ~c) if c < 0 else (up_node, c)
                if not 0 <= j < into.shape[0] or into[j, 0] >= 0 or c == 0:
                    raise ValueError(f"tree {ti}: node {i} has the child {c}, which is out of range or has a parent already")
                into[j] = (i, d)
        cover = np.zeros(nn, np.int64)
        paths = []
        for l in range(nn + 1):
            path, (at, d) = [], up_leaf[l]
            while at >= 0 and len(path) <= nn:
                path.append((int(at), int(d)))
                cover[at] += counts[l]
                at, d = up_node[at]
            if nn and (not path or path[-1][0] != 0 or len(path) > nn):
                raise ValueError(f"tree {ti}: leaf {l} does not hang below the root")
            paths.append(path[::-1])
        for i in np.nonzero(cover <= 0)[0][:1]:
            raise ValueError(f"tree {ti}: node {int(i)} has cover 0: no row of the background reaches it")
        for l in np.nonzero(counts <= 0)[0][:1]:
            raise ValueError(f"tree {ti}: node ~{int(l)} (leaf {int(l)}) has cover 0: no row of the background reaches it")
        covers.append(cover)
        for l, path in enumerate(paths):
            feats, z = [], []
            for k, (at, d) in enumerate(path):
                f = int(feature[at])
                child = counts[l] if k + 1 == len(path) else cover[path[k + 1][0]]
                frac = np.float64(child) / np.float64(cover[at])
                if f not in feats:
                    feats.append(f)
                    z.append(np.float64(1.0))
                e = feats.index(f)
                z[e] = z[e] * frac
                path_node.append(base + at)
                path_dir.append(d)
                path_elem.append(e)
            if len(feats) > SHAP_MAX_ELEMENTS:
                raise ValueError(f"tree {ti}: the path to leaf {l} holds {len(feats)} distinct features, at most {SHAP_MAX_ELEMENTS}")
            elem_feature += feats
            elem_z += z
            path_offsets.append(len(path_node))
            elem_offsets.append(len(elem_feature))
        leaf_value.append(np.asarray(t["value"], np.float32).reshape(-1))
        base += nn
    if max(len(path_node), len(elem_feature), base) >= 2 ** 31:
        raise ValueError("the path tables need int32 indices")
    leaves = np.concatenate([[0], np.cumsum([np.asarray(t["feature"]).size + 1 for t in trees])]).astype(np.int64)
    return {"path_offsets": np.array(path_offsets, np.int32), "elem_offsets": np.array(elem_offsets, np.int32),
            "leaf_value": np.concatenate(leaf_value).astype(np.float32) if leaf_value else np.zeros(0, np.float32),
            "path_node": np.array(path_node, np.int32), "path_dir": np.array(path_dir, np.uint8), "path_elem": np.array(path_elem, np.uint8),
            "elem_feature": np.array(elem_feature, np.int32), "elem_z": np.array(elem_z, np.float64), "quad_t": _SHAP_QUAD[0], "quad_w": _SHAP_QUAD[1],
            "tree_leaf_offsets": leaves, "covers": covers}


def shap_quadrature():
    """The Gauss-Legendre rules of TreeSHAP on [0, 1], float64: the rule of Q nodes (Q = 1 .. 32) at Q (Q - 1) / 2 .. of (t [528], w [528]).
    The rule of Q nodes integrates a polynomial of degree 2 Q - 1 exactly: a path of d elements takes Q = ceil(d / 2)."""
    ts, ws = zip(*(np.polynomial.legendre.leggauss(q) for q in range(1, (SHAP_MAX_ELEMENTS + 1) // 2 + 1)))
    return (np.concatenate(ts) + 1.0) / 2.0, np.concatenate(ws) / 2.0


_SHAP_QUAD = shap_quadrature()


class GBDT:
    """The booster.  GBDT(params, X=None): params under LightGBM's names (DEFAULT_PARAMS; the keys of IGNORED_PARAMS are accepted and
    ignored; boosting_type other than 'gbdt' raises).  Under grow_policy='leafwise' update() costs one host synchronisation per split: the
    host reads the two children's records (72 bytes each) to pick the next leaf; under 'depthwise' one per level.  host_reads counts them."""

    def __init__(self, params=None, X=None, device=None):
        self.params = _params(params)
        self.trees = []                    # per tree: dict(feature, threshold, left, right, value) of numpy arrays
        self.edges = self.nbins = None     # host copies (the model file carries them)
        self.nan_bin = None                # under use_missing: the NaN bin per feature, -1 where training saw no NaN
        self._nan_bin_d = None
        self._is_cat = self._is_cat_d = None   # categorical_feature as a mask over the features: host bool [F], device uint8 [F]
        self._mono = self._mono_d = None       # active monotone constraints: host int8 [F] and its device copy
        self._groups = None                    # active interaction constraints: the groups as sets, the unlisted features' group included
        self.best_iteration = None
        self._device = device
        self._flat = None
        self._shap = None                  # set_background: the path tables of TreeSHAP on the device, for the trees held then
        self.n = 0
        self.host_reads = 0                # device-to-host reads inside update(), over the booster's life: what a growth policy costs
        self._qid = None
        if X is not None:
            self.fit_bins(X)

    # ---- data
    def _dev(self):
        if not torch.cuda.is_available():
            raise RuntimeError("GBDT needs a GPU: ptranking_amd runs on the MI355X HIP path only (no CPU fallback)")
        return torch.device("cuda" if self._device is None else self._device)

    def fit_bins(self, X, group=None, init_model=None):
        """Computes the bin edges of X (numpy array or device tensor [n, F]) on the host, bins X on the device and keeps the bins, the
        training scores (zeros) and the work buffers resident.  group: the documents per query, which bagging_by_query samples by.
        init_model (a GBDT, a LambdaMART or the path of a saved model): continue that model on X.  The edges are the model's (no bin_edges
        call), the trees are copies of those its predict uses by default (best_iteration is cleared), and the resident scores start at
        predict(X) over them, so update() goes on from tree len(trees): a fit split in two gives the bits of the unsplit fit.  The trainer
        must share max_bin, use_missing and categorical_feature with the model, and X must fit its bins (ValueError otherwise)."""
        groups = self._check_constraints(np.shape(X))                      # the refusals of the constraints come before any device work
        model = None if init_model is None else _initial_model(init_model, self.params, self._device)
        dev = self._dev()
        if group is not None:
            group = np.asarray(group).reshape(-1).astype(np.int64)
            if (group < 0).any() or int(group.sum()) != len(X):
                raise ValueError(f"group must hold non-negative counts that sum to the {len(X)} rows of X")
        elif self._by_query():
            raise ValueError("bagging_by_query needs the queries: fit_bins(X, group=...)")
        host = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
        host = np.ascontiguousarray(host, dtype=np.float32)
        p = self.params
        cats = p["categorical_feature"]
        if cats and cats[-1] >= host.shape[1]:
            raise ValueError(f"categorical_feature {cats[-1]} with {host.shape[1]} columns")
        if model is not None:
            self._take_bins(model, host)
        elif p["use_missing"]:
            self.edges, self.nbins, self.nan_bin = bin_edges(host, p["max_bin"], True, **({"categorical": cats} if cats else {}))
        else:
            self.edges, self.nbins = bin_edges(host, p["max_bin"], **({"categorical": cats} if cats else {}))
        Xd = _device_matrix(X if isinstance(X, torch.Tensor) else host, dev)
        self.n, self.F = host.shape
        self._edges_d, self._nbins_d = torch.from_numpy(self.edges).to(dev), torch.from_numpy(self.nbins).to(dev)
        self._nan_bin_d = torch.from_numpy(self.nan_bin).to(dev) if p["use_missing"] else None
        self.bins = F.gbdt_bin(Xd, self._edges_d, self._nbins_d, nan_bin=self._nan_bin_d)
        n = self.n
        self.scores = torch.zeros(n, device=dev, dtype=torch.float32)
        self._arange = torch.arange(n, device=dev, dtype=torch.int32)
        self._rows, self._tmp = torch.empty_like(self._arange), torch.empty_like(self._arange)
        self._qg, self._qh = torch.empty_like(self._arange), torch.empty_like(self._arange)
        self._expo = torch.zeros(2, device=dev, dtype=torch.int32)
        self._flag = torch.zeros(1, device=dev, dtype=torch.int32)
        self._lc = torch.zeros(1, device=dev, dtype=torch.int32)
        self._rec = torch.zeros((2, 9), device=dev, dtype=torch.int64)
        self._lrec = torch.zeros((max(p["num_leaves"], 2), 9), device=dev, dtype=torch.int64)      # a depth-wise level's records
        if cats:
            self._set_is_cat(dev)
            self._sets = torch.zeros((2, 4), device=dev, dtype=torch.int64)                            # the left sets beside _rec and _lrec
            self._lsets = torch.zeros((max(p["num_leaves"], 2), 4), device=dev, dtype=torch.int64)
        self._mono = self._mono_d = self._groups = None
        if "monotone" in constraints(p):
            self._mono = np.array(p["monotone_constraints"], np.int8)
            self._mono_d = torch.from_numpy(self._mono).to(dev)
        if groups is not None:
            self._groups, self._allowed_rows = groups, {}
        self._pool = torch.zeros((max(p["num_leaves"], 1), self.F, p["max_bin"], 3), device=dev, dtype=torch.int64)
        self._qid = None if group is None else torch.from_numpy(np.repeat(np.arange(group.size, dtype=np.int32), group)).to(dev)
        if sampling(p):
            self._mask = torch.empty(n, device=dev, dtype=torch.uint8)
            self._none = torch.full((1,), -1, device=dev, dtype=torch.int32)
            self._bag_draw = None                                      # the draw self._mask holds (bagging_freq > 1 reuses it)
            if sampling(p) == "goss":
                self._gg, self._gh = torch.empty_like(self.scores), torch.empty_like(self.scores)
                self._info = torch.zeros(3, device=dev, dtype=torch.int32)
        if model is not None:
            stop = model.best_iteration or len(model.trees)
            self.trees = [_copy_tree(t) for t in model.trees[:stop]]
            self.best_iteration = None
            self._flat = self._shap = None
            self.scores = self.predict(Xd, check_finite=False)             # the bits predict goes on giving: each new tree is added after them
        return self

    def _take_bins(self, model, host):
        """The edges of an initial model in place of bin_edges(host), with bin_edges' refusals of what the matrix may hold and two more:
        what the model's bins cannot represent."""
        p = self.params
        if host.ndim != 2 or host.shape[1] != model.edges.shape[0]:
            raise ValueError(f"X must be [rows, {model.edges.shape[0]}] as the initial model's, got {host.shape}")
        nan = np.isnan(host)
        if p["use_missing"]:
            if np.isinf(host).any():
                raise ValueError(_INFINITE)
            nan_bin = np.asarray(model.nan_bin).reshape(-1)
            if nan_bin.size != host.shape[1]:
                raise ValueError(f"init_model holds nan_bin for {nan_bin.size} features, X {host.shape[1]} columns")
            for f in np.nonzero(nan.any(axis=0) & (nan_bin < 0))[0][:1]:
                raise ValueError(f"feature {int(f)} holds a NaN, and the initial model keeps no NaN bin for it (nan_bin is -1): its training data held none")
        elif not np.isfinite(host).all():
            raise ValueError(_NONFINITE)
        for f in p["categorical_feature"]:
            col = host[:, f][~nan[:, f]]
            if col.size and not ((col == np.floor(col)) & (col >= 0) & (col <= p["max_bin"] - 1)).all():
                raise ValueError(f"feature {f}: " + _not_codes(p["max_bin"]))
            if col.size and col.max() > int(model.nbins[f]) - 1:
                raise ValueError(f"feature {f} holds the categorical code {int(col.max())}, above the initial model's largest, {int(model.nbins[f]) - 1}: "
                                 f"its bins cannot represent it")
        self.edges, self.nbins = np.array(model.edges, np.float32), np.array(model.nbins, np.int32)
        self.nan_bin = np.array(model.nan_bin, np.int32) if p["use_missing"] else None

    def _check_constraints(self, shape):
        """Checks monotone_constraints and interaction_constraints against the columns of X -> the interaction groups as sets (the unlisted
        features' group included), or None without interaction constraints."""
        p = self.params
        if not p["monotone_constraints"] and not p["interaction_constraints"]:
            return None
        if len(shape) != 2:
            raise ValueError(f"X must be [rows, features], got {tuple(shape)}")
        if p["monotone_constraints"] and len(p["monotone_constraints"]) != shape[1]:
            raise ValueError(f"monotone_constraints holds {len(p['monotone_constraints'])} entries, X {shape[1]} columns")
        return _interaction_groups(p, shape[1]) if p["interaction_constraints"] else None

    def _set_is_cat(self, dev):
        self._is_cat = np.zeros(self.edges.shape[0], bool)
        self._is_cat[list(self.params["categorical_feature"])] = True
        self._is_cat_d = torch.from_numpy(self._is_cat.astype(np.uint8)).to(dev)

    def _by_query(self):
        return sampling(self.params) == "bagging" and self.params["bagging_by_query"]

    def _sample(self, grad, hess):
        """The keep mask of the tree about to be grown, in self._mask -> (grad, hess) to quantize, or None for a tree on every row (GOSS's
        warm-up).  Bagging: tree t uses draw t // bagging_freq and keeps the mask between draws.  GOSS: draw t, its own weighted copies."""
        p, t = self.params, len(self.trees)
        if sampling(p) == "goss":
            if t < int(np.floor(1.0 / p["learning_rate"])):
                return None
            F.gbdt_goss(grad, hess, p["top_rate"], p["other_rate"], p["bagging_seed"], t, out=(self._gg, self._gh), mask=self._mask, info=self._info)
            return self._gg, self._gh
        if p["bagging_by_query"] and self._qid is None:
            raise ValueError("bagging_by_query needs the queries: fit_bins(X, group=...)")
        draw = t // p["bagging_freq"]
        if draw != self._bag_draw:
            F.gbdt_bag_mask(self.n, p["bagging_seed"], draw, p["bagging_fraction"], qid=self._qid if p["bagging_by_query"] else None, out=self._mask)
            self._bag_draw = draw
        return grad, hess

    # ---- one boosting round
    def _allowed(self, groups):
        """The features a leaf of these active groups may split on, uint8 [F] (cached by the groups)."""
        row = self._allowed_rows.get(groups)
        if row is None:
            row = np.zeros(self.F, np.uint8)
            for g in groups:
                row[list(self._groups[g])] = 1
            self._allowed_rows[groups] = row
        return row

    def _cst_tables(self, cst, groups):
        """The device tables of the leaves about to be searched: (cst float64 [k, 3] or None, allowed uint8 [k, F] or None), from the leaves'
        (lo, hi, v) and active groups; one small host-to-device copy each, on the current stream."""
        dev = self.scores.device
        cst_d = None if self._mono is None else torch.from_numpy(np.ascontiguousarray(np.asarray(cst, np.float64).reshape(-1, 3))).to(dev)
        allowed_d = None if self._groups is None else torch.from_numpy(np.stack([self._allowed(g) for g in groups])).to(dev)
        return cst_d, allowed_d

    def _child_cst(self, cst, f, lsum, rsum):
        """(lo, hi, v) of the two children of a split on f (one node, or a level's nodes as arrays) from the parent's and the record's
        integer sums: vL = clamp(-GL / (HL + l2), lo, hi), vR likewise, mid = (vL + vR) / 2 -> ([.., 3] left, [.., 3] right) float64."""
        eg, eh = self._expo_host
        cst, lsum, rsum = np.asarray(cst, np.float64), np.asarray(lsum, np.int64), np.asarray(rsum, np.int64)
        lo, hi = cst[..., 0], cst[..., 1]
        l2 = np.float64(self.params["lambda_l2"])
        value = lambda sums: np.minimum(np.maximum(-np.ldexp(sums[..., 0].astype(np.float64), -eg) / (np.ldexp(sums[..., 1].astype(np.float64), -eh) + l2), lo), hi)
        vl, vr = value(lsum), value(rsum)
        mid = (vl + vr) / np.float64(2.0)
        sign = self._mono[f]
        left = np.stack([np.where(sign < 0, mid, lo), np.where(sign > 0, mid, hi), vl], axis=-1)
        right = np.stack([np.where(sign > 0, mid, lo), np.where(sign < 0, mid, hi), vr], axis=-1)
        return left, right

    def _child_groups(self, groups, f):
        """The active groups of a child of a split on f: the parent's that contain f."""
        return tuple(g for g in groups if f in self._groups[g])

    def _search(self, slot, out_row, tables=None):
        p = self.params
        if tables is not None:                                             # monotone or interaction constraints: row 0 of the tables is this leaf's
            cats = bool(p["categorical_feature"])
            F.gbdt_best_split_cst(self._pool[slot:slot + 1], self._nbins_d, self._expo, self._mono_d, tables[0], tables[1],
                                  self._is_cat_d if cats else None, p["cat_smooth"], p["lambda_l2"], p["min_data_in_leaf"], p["min_sum_hessian_in_leaf"],
                                  p["min_gain_to_split"], out=self._rec[out_row:out_row + 1], sets=self._sets[out_row:out_row + 1] if cats else None,
                                  nan_bin=self._nan_bin_d)
            return
        if p["categorical_feature"]:
            F.gbdt_best_split_cat(self._pool[slot:slot + 1], self._nbins_d, self._expo, self._is_cat_d, p["cat_smooth"], p["lambda_l2"], p["min_data_in_leaf"],
                                  p["min_sum_hessian_in_leaf"], p["min_gain_to_split"], out=self._rec[out_row:out_row + 1],
                                  sets=self._sets[out_row:out_row + 1], nan_bin=self._nan_bin_d)
            return
        F.gbdt_best_split(self._pool[slot:slot + 1], self._nbins_d, self._expo, p["lambda_l2"], p["min_data_in_leaf"], p["min_sum_hessian_in_leaf"],
                          p["min_gain_to_split"], out=self._rec[out_row:out_row + 1], nan_bin=self._nan_bin_d)

    def _splittable(self, count, depth):
        """Whether a leaf of `count` rows at `depth` may split: one leaf, or a level's counts as an array."""
        p = self.params
        return (count >= 2 * max(p["min_data_in_leaf"], 1)) & (p["max_depth"] <= 0 or depth < p["max_depth"])

    def update(self, grad, hess):
        """Grows one tree from device fp32 gradients and Hessians [n]: the leaf with the largest gain is split (ties: the older leaf) until
        num_leaves is reached or no leaf has a valid split (_grow_leafwise; grow_policy='depthwise': level by level, _grow_depthwise); the
        leaf values -G / (H + lambda_l2) * learning_rate are added to the resident training scores.  Returns the tree (a dict of numpy
        arrays).  A NaN or an infinity in grad / hess raises."""
        if self.n == 0 or self.edges is None:
            raise RuntimeError("call fit_bins(X) first")
        p, nf, mb, pool = self.params, self.F, self.params["max_bin"], self._pool
        sampled = self._sample(grad, hess) if sampling(p) else None
        if sampled is not None:
            grad, hess = sampled
        F.gbdt_quantize(grad, hess, flag=self._flag, out=(self._qg, self._qh, self._expo))
        pool[0].zero_()
        if sampled is None:
            F.gbdt_histogram(self.bins, self._qg, self._qh, None, nf, mb, hist=pool[0])
        else:
            # the bag first, in order, then the rest: the tree grows on [0, m).  m is known on the device alone until the head read below (it
            # is the root's count), so the root's histogram runs over all n entries of a list whose out-of-bag entries are -1, which it skips
            F.gbdt_partition_mask(self._mask, out=self._rows, left_count=self._lc)
            torch.where(self._mask != 0, self._arange, self._none, out=self._tmp)
            F.gbdt_histogram(self.bins, self._qg, self._qh, self._tmp, nf, mb, hist=pool[0])
        active = constraints(p)
        self._search(0, 0, self._root_tables() if active else None)
        head = torch.cat([self._rec[0], pool[0, 0].sum(0), self._expo.to(torch.int64), self._flag.to(torch.int64)]
                         + ([self._sets[0]] if p["categorical_feature"] else [])).cpu().numpy()      # the root's left set rides in the same read
        self.host_reads += 1
        if head[14]:
            self._flag.zero_()
            raise FloatingPointError("the gradients or Hessians of this round hold a NaN or an infinity")
        expo = self._expo_host = (int(head[12]), int(head[13]))
        self._leaf_v = None                                                # under monotone constraints: the leaves' clamped v, set by the grower
        bag = self.n if sampled is None else int(head[11])             # the root's row count: the size of the bag
        if sampled is None:
            self._rows.copy_(self._arange)
        grow = self._grow_depthwise if p["grow_policy"] == "depthwise" else self._grow_leafwise
        feature, threshold, left, right, starts, g_sum, h_sum, split_bin, go_left, cat_index, cat_sets = grow(head, bag)
        if self._leaf_v is not None and len(g_sum) > 1:                   # a leaf stores float32(v * learning_rate) with its clamped v
            value = np.array([np.float32(v * p["learning_rate"]) for v in self._leaf_v], np.float32)
        else:
            value = np.array([leaf_value(g, h, expo, p["lambda_l2"], p["learning_rate"]) for g, h in zip(g_sum, h_sum)], np.float32)
        return self._finish(feature, threshold, left, right, starts, value, bag, split_bin, go_left, cat_index, cat_sets)

    def _root_tables(self):
        """The root's tables.  Its sums are known on the device alone before the head read, so its v = -G / (H + lambda_l2) is computed
        there, in float64 from the integer totals: no host read; lo = -inf, hi = +inf, every group active."""
        cst_d = None
        if self._mono is not None:
            tot = self._pool[0, 0].sum(0)
            scale = ((1023 - self._expo.to(torch.int64)) << 52).view(torch.float64)      # 2^-e, built from its bits: exact
            G, H = tot[0].to(torch.float64) * scale[0], tot[1].to(torch.float64) * scale[1]
            den = H + self.params["lambda_l2"]
            v = torch.where(den > 0.0, -G / den, torch.zeros_like(den))
            cst_d = torch.stack([torch.full_like(v, -np.inf), torch.full_like(v, np.inf), v]).reshape(1, 3)
        allowed_d = None if self._groups is None else torch.from_numpy(self._allowed(tuple(range(len(self._groups))))[None]).to(self.scores.device)
        return cst_d, allowed_d

    def _root_cst(self, head):
        """(lo, hi, v) of the root on the host, from the totals of the head read: what _root_tables computed on the device."""
        G, H = np.ldexp(np.float64(int(head[9])), -self._expo_host[0]), np.ldexp(np.float64(int(head[10])), -self._expo_host[1])
        den = H + np.float64(self.params["lambda_l2"])
        return np.array([-np.inf, np.inf, -G / den if den > 0.0 else 0.0], np.float64)

    def _grow_leafwise(self, head, m):
        """Leaf-wise growth from the root's record (head, as update read it) over the first m entries of the row list: the leaf with the
        largest gain is split (ties: the older leaf), the smaller child's histogram is built and the larger one's subtracted, and ONE host
        read per split brings the two children's records.  -> what _grow_depthwise returns."""
        p, nf, mb, pool = self.params, self.F, self.params["max_bin"], self._pool
        root_rec = _record(head[:9]) if self._splittable(m, 0) else _NO_SPLIT
        cats = bool(p["categorical_feature"])
        mono, inter = self._mono is not None, self._groups is not None
        leaves = [_Leaf(0, m, 0, 0, -1, 0, int(head[9]), int(head[10]), root_rec, head[15:19].copy() if cats else None,
                        self._root_cst(head) if mono else None, tuple(range(len(self._groups))) if inter else None)]
        feature, threshold, left, right, split_bin, go_left = [], [], [], [], [], []
        cat_index, cat_sets = ([], []) if cats else (None, None)
        missing = p["use_missing"]
        free = 1                                                       # the next unused histogram slot
        while len(leaves) < p["num_leaves"]:
            li = max(range(len(leaves)), key=lambda i: (leaves[i].rec[0], -i))
            leaf = leaves[li]
            gain, f, b, lsum, rsum = leaf.rec
            if not gain > -np.inf:
                break
            s, m = leaf.start, leaf.count
            is_c = cats and bool(self._is_cat[f])
            if missing:                                                    # field 2 of a record of the missing scan: bin + 256 * default_left
                dl, b = b >> 8, b & 255
                go_left.append(dl)
            if is_c:                                                       # field 2 of a categorical record: left categories + 256 * default_left
                b = 0
            if cats:
                cat_index.append(len(cat_sets) if is_c else -1)
                if is_c:
                    cat_sets.append(leaf.set)
                F.gbdt_partition_cat(self.bins, self._rows[s:s + m], f, b, nf, self._is_cat_d, leaf.set, default_left=dl if missing else 0,
                                     nan_bin=self._nan_bin_d, out=self._tmp[s:s + m], left_count=self._lc)
            else:
                F.gbdt_partition(self.bins, self._rows[s:s + m], f, b, nf, out=self._tmp[s:s + m], left_count=self._lc,
                                 also_left=(int(self.nan_bin[f]) if dl else -1) if missing else None)
            self._rows[s:s + m].copy_(self._tmp[s:s + m])
            node = len(feature)
            feature.append(f); threshold.append(np.float32(0.0) if is_c else self.edges[f, b]); left.append(~li); right.append(~len(leaves)); split_bin.append(b)
            if leaf.parent >= 0:
                (left if leaf.side == 0 else right)[leaf.parent] = node
            lchild = _Leaf(s, lsum[2], leaf.depth + 1, leaf.slot, node, 0, lsum[0], lsum[1], _NO_SPLIT)
            rchild = _Leaf(s + lsum[2], rsum[2], leaf.depth + 1, leaf.slot, node, 1, rsum[0], rsum[1], _NO_SPLIT)
            if mono:
                lchild.cst, rchild.cst = self._child_cst(leaf.cst, f, lsum, rsum)
            if inter:
                lchild.groups = rchild.groups = self._child_groups(leaf.groups, f)
            leaves[li] = lchild
            leaves.append(rchild)
            can = [self._splittable(c.count, c.depth) for c in (lchild, rchild)]
            if len(leaves) < p["num_leaves"] and any(can):
                small, large = (lchild, rchild) if lchild.count <= rchild.count else (rchild, lchild)
                small.slot, free = free, free + 1
                pool[small.slot].zero_()
                F.gbdt_histogram(self.bins, self._qg, self._qh, self._rows[small.start:small.start + small.count], nf, mb, hist=pool[small.slot])
                F.gbdt_hist_sub(pool[large.slot], pool[small.slot], out=pool[large.slot])          # the larger child, in the parent's slot
                tables = self._cst_tables([lchild.cst, rchild.cst], [lchild.groups, rchild.groups]) if (mono or inter) else None
                for k, c in enumerate((lchild, rchild)):
                    if can[k]:
                        self._search(c.slot, k, None if tables is None else tuple(None if t is None else t[k:k + 1] for t in tables))
                recs = (torch.cat([self._rec, self._sets], dim=1) if cats else self._rec).cpu().numpy()      # the one synchronisation of this split
                self.host_reads += 1
                for k, c in enumerate((lchild, rchild)):
                    if can[k]:
                        c.rec = _record(recs[k, :9])
                        c.set = recs[k, 9:13].copy() if cats else None
        if mono:
            self._leaf_v = [float(c.cst[2]) for c in leaves]
        return (feature, threshold, left, right, [c.start for c in leaves], [c.g for c in leaves], [c.h for c in leaves], split_bin, go_left, cat_index,
                cat_sets)

    def _finish(self, feature, threshold, left, right, starts, value, m, split_bin, go_left=(), cat_index=None, cat_sets=None):
        """Adds the leaf values (by leaf index, with the leaves' first positions in the row list) to the training scores; keeps the tree.
        The tree grew on the first m entries of the row list: the rows behind them (outside a sampled tree's bag) are walked through the
        tree on their bins and get the same fp32 leaf value, so the scores stay predict(X) bit for bit.  split_bin, the split bins by node,
        serves that one call and is not part of the model.  go_left (use_missing): default_left by node, kept with the tree; in the walk
        a node's NaN bin goes left with it.  cat_index, cat_sets (categorical features): per node -1 or the index of its left set, and the
        sets, kept with the tree as cat_index and cat_set [sets, 4] int64; a tree without them is the dict it always was."""
        order = sorted(range(len(starts)), key=lambda i: starts[i])
        offsets = np.array([starts[i] for i in order] + [m], np.int32)
        dev = self.scores.device
        F.gbdt_add_leaf_values(self.scores, self._rows, torch.from_numpy(offsets).to(dev), torch.from_numpy(value[order]).to(dev))
        t = {"feature": np.array(feature, np.int32), "threshold": np.array(threshold, np.float32), "left": np.array(left, np.int32),
             "right": np.array(right, np.int32), "value": value}
        also = None
        if self.params["use_missing"]:
            t["default_left"] = np.array(go_left, np.uint8).reshape(-1)
            also = np.where(t["default_left"] != 0, self.nan_bin[t["feature"]], -1)
        if cat_index is not None:
            t["cat_index"] = np.array(cat_index, np.int32).reshape(-1)
            t["cat_set"] = np.array(cat_sets, np.int64).reshape(-1, 4)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        if m < self.n and cat_index is not None:
            F.gbdt_add_tree_binned_cat(self.scores, self.bins, self.F, self._rows[m:], up(t["feature"], np.int32), up(split_bin, np.int32), up(t["left"], np.int32),
                                       up(t["right"], np.int32), up(value, np.float32), self._is_cat_d, up(t["cat_index"], np.int32), up(t["cat_set"], np.int64),
                                       default_left=up(t["default_left"], np.uint8) if "default_left" in t else None, nan_bin=self._nan_bin_d)
        elif m < self.n:
            F.gbdt_add_tree_binned(self.scores, self.bins, self.F, self._rows[m:], up(t["feature"], np.int32), up(split_bin, np.int32), up(t["left"], np.int32),
                                   up(t["right"], np.int32), up(value, np.float32), also_left=None if also is None else up(also, np.int32))
        self.trees.append(t)
        self._flat = self._shap = None
        return t

    def _grow_depthwise(self, head, m):
        """Depth-wise growth from the root's record (head, as update read it): every level is one batched pass over all its leaves
        (partition, histograms of the smaller children, sibling subtraction, split scan) and ONE host read, the records of the level's
        searched children.  The root is the first m entries of the row list (all rows, or a sampled tree's bag, which update has put there).
        -> (feature, threshold, left, right, the leaves' first positions, their sums qg and qh, the split bins, default_left (zeros without
        use_missing)), by node / leaf index."""
        p, nf, mb, cap = self.params, self.F, self.params["max_bin"], self.params["num_leaves"]
        pool = self._pool
        feature, threshold = np.zeros(max(cap - 1, 0), np.int32), np.zeros(max(cap - 1, 0), np.float32)
        left, right, split_bin = np.zeros(max(cap - 1, 0), np.int32), np.zeros(max(cap - 1, 0), np.int32), np.zeros(max(cap - 1, 0), np.int32)
        go_left, missing = np.zeros(max(cap - 1, 0), np.uint8), p["use_missing"]
        cats = bool(p["categorical_feature"])                              # a record then carries its left set in the columns 9 .. 12
        cat_index, cat_sets, ncol = (np.full(max(cap - 1, 0), -1, np.int32), [], 13) if cats else (None, None, 9)
        starts, g_sum, h_sum = np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        g_sum[0], h_sum[0] = head[9], head[10]
        nodes, leaves, free, depth = 0, 1, 1, 0
        # the frontier, in ascending start: leaf index, start, count, histogram slot, parent node, side, split record (gain -inf: none)
        leaf, start, count, slot = np.zeros(1, np.int64), np.zeros(1, np.int64), np.full(1, m, np.int64), np.zeros(1, np.int64)
        parent, side = np.full(1, -1, np.int64), np.zeros(1, np.int64)
        rec = np.concatenate([head[:9], head[15:19]] if cats else [head[:9]]).astype(np.int64).reshape(1, ncol)
        mono, inter = self._mono is not None, self._groups is not None
        cst = self._root_cst(head).reshape(1, 3) if mono else None        # the frontier's (lo, hi, v) and active groups
        groups = [tuple(range(len(self._groups)))] if inter else None
        v_leaf = np.zeros(cap, np.float64)
        if mono:
            v_leaf[0] = cst[0, 2]
        while True:
            gain = rec[:, 0].copy().view(np.float64)
            keep = np.nonzero(self._splittable(count, depth) & (gain > -np.inf))[0]
            budget = cap - leaves
            if keep.size == 0 or budget <= 0:
                break
            if keep.size > budget:                                         # the cap: the largest gains, ties to the smaller start
                keep = np.sort(keep[np.lexsort((start[keep], -gain[keep]))[:budget]])
            k = keep.size
            f, b, lsum, rsum = rec[keep, 1], rec[keep, 2], rec[keep, 3:6], rec[keep, 6:9]
            node = nodes + np.arange(k)
            if missing:                                                    # field 2 of a record of the missing scan: bin + 256 * default_left
                go_left[node], b = b >> 8, b & 255
            if cats:                                                       # field 2 of a categorical record: left categories + 256 * default_left
                is_c = self._is_cat[f]
                b = np.where(is_c, 0, b)
                cat_index[node[is_c]] = len(cat_sets) + np.arange(int(is_c.sum()))
                cat_sets.extend(rec[keep[is_c], 9:13])
            feature[node], threshold[node], split_bin[node] = f, np.where(is_c, np.float32(0.0), self.edges[f, b]) if cats else self.edges[f, b], b
            left[node], right[node] = ~leaf[keep], ~(leaves + np.arange(k))
            has = parent[keep] >= 0
            for arr, sd in ((left, 0), (right, 1)):
                sel = has & (side[keep] == sd)
                arr[parent[keep][sel]] = node[sel]
            also = [np.where(go_left[node] != 0, self.nan_bin[f], -1)] if missing else []       # the fifth column of the missing form
            if cats:
                F.gbdt_partition_segments_cat(self.bins, self._rows, np.stack([start[keep], count[keep], f, b, go_left[node].astype(np.int64)], axis=1),
                                              rec[keep, 9:13], nf, self._is_cat_d, nan_bin=self._nan_bin_d, out=self._tmp)
            else:
                F.gbdt_partition_segments(self.bins, self._rows, np.stack([start[keep], count[keep], f, b] + also, axis=1), nf, out=self._tmp, also_left=missing)
            self._rows, self._tmp = self._tmp, self._rows
            # the children, interleaved (left, right): ascending start again
            c_leaf = np.stack([leaf[keep], leaves + np.arange(k)], axis=1)
            c_start = np.stack([start[keep], start[keep] + lsum[:, 2]], axis=1)
            c_count = np.stack([lsum[:, 2], rsum[:, 2]], axis=1)
            starts[c_leaf], g_sum[c_leaf], h_sum[c_leaf] = c_start, np.stack([lsum[:, 0], rsum[:, 0]], axis=1), np.stack([lsum[:, 1], rsum[:, 1]], axis=1)
            if mono:
                c_cst = np.stack(self._child_cst(cst[keep], f, lsum, rsum), axis=1)          # [k, 2, 3]
                v_leaf[c_leaf] = c_cst[:, :, 2]
            if inter:
                c_groups = [self._child_groups(groups[i], int(fi)) for i, fi in zip(keep, f)]
            nodes, leaves, depth = nodes + k, leaves + k, depth + 1
            can = self._splittable(c_count, depth)
            c_slot = np.repeat(slot[keep][:, None], 2, axis=1)
            c_rec = np.zeros((k, 2, ncol), np.int64)
            c_rec[:, :, 0], c_rec[:, :, 1:3] = np.float64(-np.inf).view(np.int64), -1
            pairs = np.nonzero(can.any(axis=1))[0] if leaves < cap else np.zeros(0, np.int64)
            if pairs.size:
                small = (c_count[pairs, 0] > c_count[pairs, 1]).astype(np.int64)      # the smaller child's side; <= goes left
                fresh = free + np.arange(pairs.size)
                free += pairs.size
                c_slot[pairs, small] = fresh
                pool[int(fresh[0]):int(fresh[-1]) + 1].zero_()
                F.gbdt_histogram_segments(self.bins, self._qg, self._qh, self._rows, np.stack([c_start[pairs, small], c_count[pairs, small], fresh], axis=1),
                                          nf, mb, pool)
                F.gbdt_hist_sub_segments(pool, np.stack([slot[keep][pairs], fresh, slot[keep][pairs]], axis=1))   # the larger child, in the parent's slot
                sp, ss = np.nonzero(can[pairs])
                out = self._lrec[:sp.size]
                if mono or inter:
                    cst_d, allowed_d = self._cst_tables(c_cst[pairs[sp], ss] if mono else None, [c_groups[i] for i in pairs[sp]] if inter else None)
                    F.gbdt_best_split_slots_cst(pool, c_slot[pairs[sp], ss], self._nbins_d, self._expo, self._mono_d, cst_d, allowed_d,
                                                self._is_cat_d if cats else None, p["cat_smooth"], p["lambda_l2"], p["min_data_in_leaf"],
                                                p["min_sum_hessian_in_leaf"], p["min_gain_to_split"], out=out, sets=self._lsets[:sp.size] if cats else None,
                                                nan_bin=self._nan_bin_d)
                    if cats:
                        out = torch.cat([out, self._lsets[:sp.size]], dim=1)
                elif cats:
                    F.gbdt_best_split_slots_cat(pool, c_slot[pairs[sp], ss], self._nbins_d, self._expo, self._is_cat_d, p["cat_smooth"], p["lambda_l2"],
                                                p["min_data_in_leaf"], p["min_sum_hessian_in_leaf"], p["min_gain_to_split"], out=out,
                                                sets=self._lsets[:sp.size], nan_bin=self._nan_bin_d)
                    out = torch.cat([out, self._lsets[:sp.size]], dim=1)
                else:
                    F.gbdt_best_split_slots(pool, c_slot[pairs[sp], ss], self._nbins_d, self._expo, p["lambda_l2"], p["min_data_in_leaf"],
                                            p["min_sum_hessian_in_leaf"], p["min_gain_to_split"], out=out, nan_bin=self._nan_bin_d)
                c_rec[pairs[sp], ss] = out.cpu().numpy()                   # the one synchronisation of this level
                self.host_reads += 1
            leaf, start, count, slot = c_leaf.reshape(-1), c_start.reshape(-1), c_count.reshape(-1), c_slot.reshape(-1)
            parent, side, rec = np.repeat(node, 2), np.tile(np.array([0, 1], np.int64), k), c_rec.reshape(-1, ncol)
            if mono:
                cst = c_cst.reshape(-1, 3)
            if inter:
                groups = [g for g in c_groups for _ in (0, 1)]
        if mono:
            self._leaf_v = v_leaf[:leaves].tolist()
        return (feature[:nodes], threshold[:nodes], left[:nodes], right[:nodes], starts[:leaves].tolist(), g_sum[:leaves].tolist(), h_sum[:leaves].tolist(),
                split_bin[:nodes], go_left[:nodes], cat_index[:nodes] if cats else None, cat_sets)

    # ---- the model
    def flat(self):
        """The flat tree arrays ptr_gbdt_predict reads (numpy): feature, threshold, left, right, value, tree_offsets; under use_missing
        default_left; with categorical features cat_index (per node -1, or the index of its left set among ALL trees' sets) and cat_sets."""
        cat = lambda k, dt: np.concatenate([t[k] for t in self.trees]).astype(dt) if self.trees else np.zeros(0, dt)
        offs = np.concatenate([[0], np.cumsum([t["feature"].size for t in self.trees])]).astype(np.int32)
        out = {"feature": cat("feature", np.int32), "threshold": cat("threshold", np.float32), "left": cat("left", np.int32),
               "right": cat("right", np.int32), "value": cat("value", np.float32), "tree_offsets": offs}
        if self.params["use_missing"]:
            out["default_left"] = cat("default_left", np.uint8)
        if self.params["categorical_feature"]:
            base = np.concatenate([[0], np.cumsum([t["cat_set"].shape[0] for t in self.trees])]).astype(np.int32)
            out["cat_index"] = (np.concatenate([np.where(t["cat_index"] >= 0, t["cat_index"] + b, -1) for t, b in zip(self.trees, base)]).astype(np.int32)
                                if self.trees else np.zeros(0, np.int32))
            out["cat_sets"] = (np.concatenate([t["cat_set"] for t in self.trees]) if self.trees else np.zeros((0, 4))).astype(np.int64).reshape(-1, 4)
        return out

    def feature_importance(self, importance_type="split"):
        """How often the trees split on each feature -> int64 [F] (numpy), counted on the host.  'gain' raises: a tree keeps no gains, and
        the three model file formats are pinned, so there is nowhere to keep them."""
        if importance_type != "split":
            raise ValueError(f"importance_type {importance_type!r}: only 'split'.  'gain' is not available: the trees keep no split gains and the "
                             f"model file formats are pinned, so a loaded model could not report them")
        if self.edges is None:
            raise RuntimeError("fit_bins() or load_model() first: the model has no features yet")
        used = np.concatenate([np.asarray(t["feature"]).reshape(-1) for t in self.trees]).astype(np.int64) if self.trees else np.zeros(0, np.int64)
        return np.bincount(used, minlength=self.edges.shape[0]).astype(np.int64)

    def _flat_device(self, dev):
        if self._flat is None:
            self._flat = {k: torch.from_numpy(v).to(dev) for k, v in self.flat().items()}
        return self._flat

    def _cat_walk(self, Xd):
        """The categorical arguments of a walk over raw rows ({} for a model without categorical features)."""
        if not self.params["categorical_feature"]:
            return {}
        if Xd.shape[1] != self.edges.shape[0]:
            raise ValueError(f"X holds {Xd.shape[1]} columns, the model {self.edges.shape[0]}")
        if self._is_cat_d is None or self._is_cat_d.device != Xd.device:
            self._set_is_cat(Xd.device)
        return {"is_cat": self._is_cat_d, "cat_index": self._flat["cat_index"], "cat_sets": self._flat["cat_sets"]}

    def set_background(self, X, check_finite=True):
        """The background matrix of predict(pred_contrib=True): X (numpy array or device tensor [n, F], raw rows as predict takes them) is
        walked through every tree in one launch (ptr_gbdt_leaf_counts), the rows per leaf are summed into node covers on the host, and the
        path tables of TreeSHAP are built and uploaded.  The trees keep no row counts; under this project's binning x <= edge is bin <= b, so
        the TRAINING matrix as background gives the counts the trees were grown on.  Every node and leaf must be reached by a row
        (ValueError names the tree and the node).  The covers live in memory only: save_model writes what it wrote, a loaded model calls
        set_background again, and so does a booster that has grown since."""
        dev = self._dev()
        fl = self._flat_device(dev)
        Xd = _device_matrix(X, dev)
        if self.edges is not None and Xd.dim() == 2 and Xd.shape[1] != self.edges.shape[0]:
            raise ValueError(f"X holds {Xd.shape[1]} columns, the model {self.edges.shape[0]}")
        cats = self.params["categorical_feature"]
        if check_finite:
            _require_values(Xd, self.params["use_missing"], *((cats, self.params["max_bin"]) if cats else ()))
        counts = F.gbdt_leaf_counts(Xd, fl["feature"], fl["threshold"], fl["left"], fl["right"], fl["tree_offsets"],
                                    default_left=fl.get("default_left"), **self._cat_walk(Xd)).cpu().numpy()
        offs = np.concatenate([[0], np.cumsum([t["feature"].size + 1 for t in self.trees])]).astype(np.int64)
        host = shap_tables(self.trees, [counts[offs[t]:offs[t + 1]] for t in range(len(self.trees))])
        self._shap = {"ntrees": len(self.trees), "tree_leaf_offsets": host["tree_leaf_offsets"], "leaf_counts": counts,
                      "tables": {k: torch.from_numpy(host[k]).to(dev) for k in F.SHAP_TABLE_KEYS}}
        return self

    def _contrib(self, Xd, first_tree, stop):
        """predict(pred_contrib=True): the leaves of the trees first_tree .. stop - 1 of the resident path tables through ptr_gbdt_shap."""
        if self._shap is None or self._shap["ntrees"] != len(self.trees):
            raise RuntimeError("pred_contrib=True needs covers and the trees keep none: call set_background(X) first (after load_model and "
                               "after every update() too; the training matrix gives the counts the trees were grown on)")
        if Xd.shape[1] != self.edges.shape[0]:
            raise ValueError(f"X holds {Xd.shape[1]} columns, the model {self.edges.shape[0]}")
        fl, tb = self._flat, dict(self._shap["tables"])
        lo, hi = int(self._shap["tree_leaf_offsets"][first_tree]), int(self._shap["tree_leaf_offsets"][stop])
        tb["path_offsets"], tb["elem_offsets"], tb["leaf_value"] = tb["path_offsets"][lo:hi + 1], tb["elem_offsets"][lo:hi + 1], tb["leaf_value"][lo:hi]
        return F.gbdt_shap(Xd, fl["feature"], fl["threshold"], tb, default_left=fl.get("default_left"), **self._cat_walk(Xd))

    def predict(self, X, num_iteration=None, first_tree=0, check_finite=True, pred_contrib=False, pred_leaf=False):
        """pred_leaf=True -> device int32 [n, trees]: the index of the leaf each of the same trees puts each row in (LightGBM's layout);
        value[leaf] summed in tree order in fp32 is the score.  It cannot be combined with pred_contrib.
        pred_contrib=True -> device float64 [n, F + 1]: the TreeSHAP contribution of every feature to the score of every row over the
        same trees, and the expected value in the last column (LightGBM's layout); a row's entries sum to its score up to the fp32
        rounding of predict's own sum.  It needs set_background.  Otherwise:
        Scores of raw rows X (numpy array or device tensor [n, F]) -> device float32 [n]: the trees first_tree .. num_iteration - 1
        (default: up to best_iteration when early stopping set it, else all), summed in tree order in fp32 — for a training row the bits of
        its resident training score.  A NaN or an infinity in X raises, as in bin_edges (a NaN would go right at every node, while binning
        puts it left); the check costs one synchronisation, and check_finite=False skips it for a matrix the caller has already checked.
        A model trained under use_missing takes NaNs: at a node a NaN feature follows the node's default_left; an infinity still raises.
        A categorical column must hold integer codes in 0 .. max_bin - 1 (the same check; check_finite=False skips it, and the kernel then
        sends what is no integer code in 0 .. 255 right).  A code the training data never held is legal: it is in no left set and goes right."""
        if pred_leaf and pred_contrib:
            raise ValueError("pred_leaf and pred_contrib cannot be combined: ask for one of them")
        dev = self._dev()
        if self._flat is None:
            self._flat = {k: torch.from_numpy(v).to(dev) for k, v in self.flat().items()}
        fl = self._flat
        stop = (self.best_iteration or len(self.trees)) if num_iteration is None else int(num_iteration)
        if not 0 <= first_tree <= stop <= len(self.trees):
            raise ValueError(f"trees {first_tree} .. {stop} of {len(self.trees)}")
        Xd = _device_matrix(X, dev)
        cats = self.params["categorical_feature"]
        if check_finite:
            _require_values(Xd, self.params["use_missing"], *((cats, self.params["max_bin"]) if cats else ()))
        if pred_contrib:
            return self._contrib(Xd, first_tree, stop)
        if pred_leaf:
            if self.edges is not None and Xd.shape[1] != self.edges.shape[0]:
                raise ValueError(f"X holds {Xd.shape[1]} columns, the model {self.edges.shape[0]}")
            return F.gbdt_predict_leaf(Xd, fl["feature"], fl["threshold"], fl["left"], fl["right"], fl["tree_offsets"], first_tree, stop,
                                       default_left=fl.get("default_left"), **self._cat_walk(Xd))
        if cats:
            return self._predict_cat(Xd, first_tree, stop)
        if first_tree == 0:
            return F.gbdt_predict(Xd, fl["feature"], fl["threshold"], fl["left"], fl["right"], fl["value"], fl["tree_offsets"], stop,
                                  default_left=fl.get("default_left"))
        host = self.flat()
        lo, hi = int(host["tree_offsets"][first_tree]), int(host["tree_offsets"][stop])
        sub = {k: torch.from_numpy(np.ascontiguousarray(host[k][lo:hi])).to(dev) for k in ("feature", "threshold", "left", "right", "default_left") if k in host}
        val = torch.from_numpy(np.ascontiguousarray(host["value"][lo + first_tree:hi + stop])).to(dev)
        offs = torch.from_numpy((host["tree_offsets"][first_tree:stop + 1] - lo).astype(np.int32)).to(dev)
        return F.gbdt_predict(Xd, sub["feature"], sub["threshold"], sub["left"], sub["right"], val, offs, default_left=sub.get("default_left"))

    def _predict_cat(self, Xd, first_tree, stop):
        """predict for a model with categorical features: the trees first_tree .. stop - 1 through ptr_gbdt_predict_cat."""
        dev, fl = Xd.device, self._flat
        if Xd.shape[1] != self.edges.shape[0]:
            raise ValueError(f"X holds {Xd.shape[1]} columns, the model {self.edges.shape[0]}")
        if self._is_cat_d is None or self._is_cat_d.device != dev:
            self._set_is_cat(dev)
        if first_tree == 0:
            return F.gbdt_predict_cat(Xd, fl["feature"], fl["threshold"], fl["left"], fl["right"], fl["value"], fl["tree_offsets"], self._is_cat_d,
                                      fl["cat_index"], fl["cat_sets"], stop, default_left=fl.get("default_left"))
        host = self.flat()
        lo, hi = int(host["tree_offsets"][first_tree]), int(host["tree_offsets"][stop])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        sub = {k: up(host[k][lo:hi]) for k in ("feature", "threshold", "left", "right", "default_left") if k in host}
        ci = host["cat_index"][lo:hi]
        first = int((host["cat_index"][:lo] >= 0).sum())                   # the sets of the trees ahead
        sets = host["cat_sets"][first:first + int((ci >= 0).sum())]
        val = up(host["value"][lo + first_tree:hi + stop])
        offs = up((host["tree_offsets"][first_tree:stop + 1] - lo).astype(np.int32))
        return F.gbdt_predict_cat(Xd, sub["feature"], sub["threshold"], sub["left"], sub["right"], val, offs, self._is_cat_d,
                                  up(np.where(ci >= 0, ci - first, -1).astype(np.int32)), up(sets), default_left=sub.get("default_left"))

    def refit(self, X, grad_hess, decay_rate=0.9, with_tree=False):
        """Keeps the tree structures and re-estimates the leaf values on new data (LightGBM's Booster.refit; the rule is this project's own
        and no parity is claimed) -> a NEW booster with the same structures, edges and parameters and its own value arrays; self is
        untouched.  X: raw rows [n, F] as predict takes them; grad_hess(scores) -> device fp32 (grad, hess) [n] at the running scores, which
        start at zero (with_tree=True: grad_hess(scores, t) with t the index of the tree whose values are re-estimated next, for an
        objective that draws per round).  Per tree, in order: grad_hess, gbdt_quantize (a NaN or an infinity raises, as in update), gbdt_leaf_sums over the
        tree, ONE host read of the sums (host_reads grows by one per tree), refit_value per leaf on the host
        (float32(decay_rate * old + (1 - decay_rate) * new), new = -G / (H + lambda_l2) * learning_rate; a leaf no row reaches or one with
        H + lambda_l2 <= 0 keeps old), gbdt_add_by_leaf with the new values.  The trees are those predict uses by default (up to
        best_iteration when early stopping set it, which the new booster clears), so its .scores are its predict(X) bit for bit.  On the
        training matrix with the training objective and decay_rate=0 an unsampled, unconstrained model gets its own leaf values back bit
        for bit.  Active monotone constraints raise: clamped values cannot be re-estimated leaf by leaf without breaking the guarantee."""
        decay = _decay_rate(decay_rate)
        p = self.params
        if "monotone" in constraints(p):
            raise ValueError("refit is not available under monotone_constraints: the leaf values were clamped between their neighbours', and "
                             "re-estimating them leaf by leaf would break the guarantee")
        if self.edges is None:
            raise RuntimeError("fit_bins() or load_model() first: there is no model to refit")
        dev = self._dev()
        Xd = _device_matrix(X, dev)
        if Xd.dim() != 2 or Xd.shape[1] != self.edges.shape[0]:
            raise ValueError(f"X must be [rows, {self.edges.shape[0]}], got {tuple(Xd.shape)}")
        cats = p["categorical_feature"]
        _require_values(Xd, p["use_missing"], *((cats, p["max_bin"]) if cats else ()))
        stop = self.best_iteration or len(self.trees)
        new = GBDT(p, device=self._device)
        new.edges, new.nbins = np.array(self.edges), np.array(self.nbins)
        new.nan_bin = None if self.nan_bin is None else np.array(self.nan_bin)
        new.trees = [_copy_tree(t) for t in self.trees[:stop]]
        new.host_reads = self.host_reads
        fl = new._flat_device(dev)                                         # the structures on the device; the values are not read from it
        walk = new._cat_walk(Xd)
        n = Xd.shape[0]
        scores = torch.zeros(n, device=dev, dtype=torch.float32)
        qg, qh = torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.int32)
        expo, flag = torch.zeros(2, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int32)
        leaf = torch.empty(n, device=dev, dtype=torch.int32)
        sums = torch.zeros((max([t["value"].size for t in new.trees], default=1), 3), device=dev, dtype=torch.int64)
        offs = np.concatenate([[0], np.cumsum([t["feature"].size for t in new.trees])]).astype(np.int64)
        for ti, t in enumerate(new.trees):
            grad, hess = grad_hess(scores, ti) if with_tree else grad_hess(scores)
            F.gbdt_quantize(grad, hess, flag=flag, out=(qg, qh, expo))
            lo, hi, nl = int(offs[ti]), int(offs[ti + 1]), t["value"].size
            cells = sums[:nl]
            cells.zero_()
            F.gbdt_leaf_sums(Xd, fl["feature"][lo:hi], fl["threshold"][lo:hi], fl["left"][lo:hi], fl["right"][lo:hi], qg, qh, nl,
                             default_left=fl["default_left"][lo:hi] if "default_left" in fl else None, leaf=leaf, sums=cells,
                             **({"is_cat": walk["is_cat"], "cat_index": walk["cat_index"][lo:hi], "cat_sets": walk["cat_sets"]} if walk else {}))
            head = torch.cat([cells.reshape(-1), expo.to(torch.int64), flag.to(torch.int64)]).cpu().numpy()      # the one read of this tree
            new.host_reads += 1
            if head[-1]:
                raise FloatingPointError("the gradients or Hessians of this round hold a NaN or an infinity")
            ex, s = (int(head[-3]), int(head[-2])), head[:-3].reshape(nl, 3)
            t["value"] = np.array([refit_value(t["value"][l], s[l, 0], s[l, 1], s[l, 2], ex, p["lambda_l2"], p["learning_rate"], decay) for l in range(nl)],
                                  np.float32)
            F.gbdt_add_by_leaf(scores, leaf, torch.from_numpy(t["value"]).to(dev))
        new._flat = new._shap = None                                       # the device copy holds the old values
        new.scores = scores                                                # no bins are resident: update() still asks for fit_bins first
        return new

    def save_model(self, path):
        """An .npz of this project's own (not LightGBM's text format): the flat tree arrays, the bin edges, the parameters.  Format 1
        without use_missing (the file this method wrote before the switch existed: neither the switch nor the categorical keys are among its
        parameters); format 2 under it, with default_left per node and nan_bin per feature; format 3 with categorical features: format 1
        or 2 (by use_missing, with every parameter) plus categorical_feature, cat_index per node and cat_sets."""
        own = self.params if constraints(self.params) else {k: v for k, v in self.params.items() if k not in CST_KEYS}      # inactive: today's file
        if self.params["categorical_feature"]:
            head = dict(format=np.int64(MODEL_FORMAT_CAT), params=np.array(json.dumps(own)), edges=self.edges, nbins=self.nbins,
                        categorical_feature=np.array(self.params["categorical_feature"], np.int32))
            if self.params["use_missing"]:
                head["nan_bin"] = np.full(0, -1, np.int32) if self.nan_bin is None else self.nan_bin
        elif self.params["use_missing"]:
            params = {k: v for k, v in own.items() if k not in CAT_KEYS}
            head = dict(format=np.int64(MODEL_FORMAT_MISSING), params=np.array(json.dumps(params)), edges=self.edges, nbins=self.nbins,
                        nan_bin=np.full(0, -1, np.int32) if self.nan_bin is None else self.nan_bin)
        else:
            params = {k: v for k, v in own.items() if k != "use_missing" and k not in CAT_KEYS}
            head = dict(format=np.int64(MODEL_FORMAT), params=np.array(json.dumps(params)), edges=self.edges, nbins=self.nbins)
        with open(path, "wb") as fh:
            np.savez(fh, **head, best_iteration=np.int64(self.best_iteration or 0), **self.flat())

    @classmethod
    def load_model(cls, path, device=None):
        """The booster save_model wrote; it predicts the same bits.  (The binned training data are not part of a model.)"""
        with np.load(path, allow_pickle=False) as z:
            fmt = int(z["format"])
            if fmt not in (MODEL_FORMAT, MODEL_FORMAT_MISSING, MODEL_FORMAT_CAT):
                raise ValueError(f"{path}: model format {fmt}, this version reads {MODEL_FORMAT}, {MODEL_FORMAT_MISSING} and {MODEL_FORMAT_CAT}")
            self = cls(json.loads(str(z["params"])), device=device)
            cats = fmt == MODEL_FORMAT_CAT
            if bool(self.params["categorical_feature"]) != cats or (cats and self.params["categorical_feature"] != tuple(z["categorical_feature"].tolist())):
                raise ValueError(f"{path}: model format {fmt} with categorical_feature={self.params['categorical_feature']}")
            if not cats and self.params["use_missing"] != (fmt == MODEL_FORMAT_MISSING):
                raise ValueError(f"{path}: model format {fmt} with use_missing={self.params['use_missing']}")
            self.edges, self.nbins = z["edges"], z["nbins"]
            if cats and self.params["categorical_feature"][-1] >= self.edges.shape[0]:
                raise ValueError(f"{path}: categorical_feature {self.params['categorical_feature'][-1]} with {self.edges.shape[0]} features")
            missing = self.params["use_missing"]
            if missing:
                self.nan_bin = z["nan_bin"]
            first = 0
            self.best_iteration = int(z["best_iteration"]) or None
            offs = z["tree_offsets"]
            for t in range(offs.size - 1):
                lo, hi = int(offs[t]), int(offs[t + 1])
                self.trees.append({"feature": z["feature"][lo:hi], "threshold": z["threshold"][lo:hi], "left": z["left"][lo:hi],
                                   "right": z["right"][lo:hi], "value": z["value"][lo + t:hi + t + 1]})
                if missing:
                    self.trees[-1]["default_left"] = z["default_left"][lo:hi]
                if cats:
                    ci = z["cat_index"][lo:hi]
                    k = int((ci >= 0).sum())
                    self.trees[-1]["cat_index"] = np.where(ci >= 0, ci - first, -1).astype(np.int32)
                    self.trees[-1]["cat_set"] = z["cat_sets"][first:first + k].astype(np.int64).reshape(-1, 4)
                    first += k
        return self


class LambdaMART:
    """LambdaMART on the native booster.  objective 'lambdarank' (pair_type 'NoTies'), 'ranknet' ('All') or 'listnet', as tree.OBJECTIVES.
    The defaults are real LambdaMART: weighting='DeltaNDCG' (applied to 'lambdarank'; 'ranknet' is the unweighted pairwise loss) and the
    never-negative hessian='sum'.  hessian='reference' (the reference's rank-signed Hessian) is accepted, but its sums are negative for
    low-ranked documents, so leaves can stay unsplittable under the Hessian floor of the split scan.
    objective 'lambdarank_ndcg' is the truncated, normalised lambdarank of the module docstring: it reads lambdarank_truncation_level,
    lambdarank_norm and sigmoid from params, and weighting, hessian, pair_type, epsilon and gain_type do not apply to it (a non-default
    value raises ValueError).
    objective 'rank_xendcg' is the cross-entropy nDCG objective of the module docstring: it reads objective_seed from params, draws round
    t's uniforms under draw = t (the tree counter), and the same five settings do not apply to it."""

    def __init__(self, params=None, objective="lambdarank", weighting="DeltaNDCG", hessian="sum", pair_type=None, epsilon=1.0,
                 gain_type="Power", device=None):
        if objective not in tree.OBJECTIVES:
            raise ValueError(f"objective {objective!r} (supported: {', '.join(map(repr, tree.OBJECTIVES))})")
        self.params = _params(params)
        self.objective = objective
        self.kind, default_pairs = tree.OBJECTIVES[objective]
        self.pair_type = default_pairs if pair_type is None else pair_type
        self.weighting = weighting if objective == "lambdarank" else None
        self.epsilon, self.hessian, self.gain_type = float(epsilon), hessian, gain_type
        if self.kind == "pair":
            F._enum("pair_type", self.pair_type, F.TREE_PAIR_TYPES)
            F._enum("weighting", self.weighting, F.TREE_WEIGHTINGS)
        elif self.kind in ("lambdarank_ndcg", "xendcg"):
            tree.not_applicable(objective, dict(weighting=weighting, hessian=hessian, pair_type=pair_type, epsilon=epsilon, gain_type=gain_type),
                                dict(weighting="DeltaNDCG", hessian="sum", pair_type=None, epsilon=1.0, gain_type="Power"))
        else:
            F._enum("gain_type", gain_type, F.TREE_GAIN_TYPES)
        F._enum("hessian", hessian, F.TREE_HESSIANS)
        if not torch.cuda.is_available():
            raise RuntimeError("LambdaMART needs a GPU: ptranking_amd runs on the MI355X HIP path only (no CPU fallback)")
        self.device = torch.device("cuda" if device is None else device)
        self.booster = None
        self.evals_result = []
        self.best_iteration = self.best_score = None

    def grad_hess(self, scores, res, out=None, draw=0):
        """The round's gradient and Hessian per document, on the device: one launch per length class of tree.bucket_queries, exactly as
        TreeObjective._run launches them.  draw: the round whose uniforms 'rank_xendcg' draws (the other objectives ignore it)."""
        out = (torch.empty_like(scores), torch.empty_like(scores)) if out is None else out
        for max_len, queries in res.buckets:
            if self.kind == "pair":
                F.tree_pair_grad_hess(scores, res.labels, res.offsets, self.pair_type, self.weighting, self.epsilon, self.hessian, queries, max_len, out)
            elif self.kind == "lambdarank_ndcg":
                p = self.params
                F.tree_lambdarank_ndcg_grad_hess(scores, res.labels, res.offsets, p["lambdarank_truncation_level"], p["sigmoid"], p["lambdarank_norm"],
                                                 queries, max_len, out)
            elif self.kind == "xendcg":
                F.tree_xendcg_grad_hess(scores, res.labels, res.offsets, self.params["objective_seed"], draw, None, queries, max_len, out)
            else:
                F.tree_listnet_grad_hess(scores, res.labels, res.offsets, self.gain_type, self.hessian, queries, max_len, out)
        return out

    @staticmethod
    def padded_index(group, device):
        """(index int64 [Q, Lmax] into the flat documents, clamped; lens int32 [Q]) for gathering ragged scores into a padded batch."""
        g = np.asarray(group).reshape(-1).astype(np.int64)
        start = np.concatenate([[0], np.cumsum(g)])[:-1]
        lmax = max(int(g.max()) if g.size else 1, 1)
        idx = start[:, None] + np.minimum(np.arange(lmax)[None, :], np.maximum(g - 1, 0)[:, None])
        idx = np.minimum(idx, max(int(g.sum()) - 1, 0))
        return torch.from_numpy(idx).to(device), torch.from_numpy(g.astype(np.int32)).to(device)

    @classmethod
    def ndcg_at(cls, scores, labels, group, k=5, index=None):
        """Mean nDCG@k over the queries that hold a relevant document, from flat device scores and labels: functional.metrics_at_ks on the
        padded gather."""
        idx, lens = cls.padded_index(group, scores.device) if index is None else index
        lab = labels[idx]
        nd = F.metrics_at_ks(scores[idx].contiguous(), lab.contiguous(), [int(k)], lens=lens, which=("ndcg",))["ndcg"][:, 0]
        pos = torch.arange(idx.shape[1], device=idx.device)[None, :] < lens[:, None]
        keep = ((lab > 0) & pos).any(dim=1)
        return float(nd[keep].mean()) if bool(keep.any()) else 0.0

    def fit(self, X, y, group, eval_set=None, eval_group=None, eval_at=5, early_stopping_rounds=None, num_boost_round=None, verbose=0,
            init_model=None):
        """X [n, F], y [n] relevance grades, group: documents per query.  eval_set = (X_valid, y_valid) with eval_group: nDCG@eval_at on it
        after every round (evals_result); early_stopping_rounds: stop after that many rounds without improvement and let predict use the
        best round (best_iteration), as LightGBM does.
        init_model (a GBDT, a LambdaMART or the path of a saved model): the rounds are ADDED to that model's trees (GBDT.fit_bins): the
        training scores and the validation scores start at its predictions, num_boost_round / num_trees count the added rounds,
        evals_result holds the added rounds, and best_iteration counts all trees."""
        res = tree._Resident(y, group, self.device)
        X = X if isinstance(X, torch.Tensor) else np.asarray(X)
        if X.shape[0] != res.n_docs:
            raise ValueError(f"X holds {X.shape[0]} rows, the groups {res.n_docs}")
        self.booster = GBDT(self.params, device=self.device).fit_bins(X, group=np.asarray(group).reshape(-1),
                                                                      **({} if init_model is None else {"init_model": init_model}))
        base = len(self.booster.trees)                                     # the initial model's trees: the rounds count on from them
        self.evals_result, self.best_iteration, self.best_score = [], None, None
        rounds = self.params["num_trees"] if num_boost_round is None else int(num_boost_round)
        valid = None
        if eval_set is not None:
            Xv, yv = eval_set
            if eval_group is None:
                raise ValueError("eval_set needs eval_group")
            Xv = _device_matrix(Xv, self.device)
            cats = self.params["categorical_feature"]
            _require_values(Xv, self.params["use_missing"], *((cats, self.params["max_bin"]) if cats else ()))   # once, before the first round: the rounds skip it
            yv = torch.from_numpy(np.ascontiguousarray(np.asarray(yv).reshape(-1), dtype=np.float32)).to(self.device)
            sv = self.booster.predict(Xv, check_finite=False) if base else torch.zeros(Xv.shape[0], device=self.device, dtype=torch.float32)
            valid = (Xv, yv, self.padded_index(eval_group, self.device), sv)
        elif early_stopping_rounds is not None:
            raise ValueError("early_stopping_rounds needs an eval_set")
        gh = (torch.empty_like(self.booster.scores), torch.empty_like(self.booster.scores))
        for it in range(base + 1, base + rounds + 1):
            self.grad_hess(self.booster.scores, res, gh, draw=len(self.booster.trees))      # the tree counter, as bagging's draws
            self.booster.update(*gh)
            if valid is None:
                continue
            Xv, yv, index, sv = valid
            sv += self.booster.predict(Xv, num_iteration=it, first_tree=it - 1, check_finite=False)      # the new tree alone: the same fp32 sum
            score = self.ndcg_at(sv, yv, None, eval_at, index=index)
            self.evals_result.append(score)
            if self.best_score is None or score > self.best_score:
                self.best_score, self.best_iteration = score, it
            if verbose and it % verbose == 0:
                print(f"[{it}] valid nDCG@{eval_at} {score:.4f}", flush=True)
            if early_stopping_rounds is not None and it - self.best_iteration >= early_stopping_rounds:
                break
        if early_stopping_rounds is None:
            self.best_iteration = None
        self.booster.best_iteration = self.best_iteration
        return self

    def predict(self, X, num_iteration=None, pred_contrib=False, pred_leaf=False):
        """The booster's scores, or with pred_contrib=True its TreeSHAP contributions float64 [n, F + 1] (set_background first), or with
        pred_leaf=True the leaf index per row and tree, int32 [n, trees]."""
        if self.booster is None:
            raise RuntimeError("fit() first")
        if pred_leaf:
            return self.booster.predict(X, num_iteration, pred_contrib=pred_contrib, pred_leaf=True)
        if pred_contrib:
            return self.booster.predict(X, num_iteration, pred_contrib=True)
        return self.booster.predict(X, num_iteration)

    def refit(self, X, y, group, decay_rate=0.9):
        """GBDT.refit of the fitted booster on new queries under this ranker's objective -> a NEW LambdaMART around the refitted booster (its
        .booster.scores are its predict(X)); self is untouched."""
        decay = _decay_rate(decay_rate)
        if self.booster is None:
            raise RuntimeError("fit() first")
        res = tree._Resident(y, group, self.device)
        if np.shape(X)[0] != res.n_docs:
            raise ValueError(f"X holds {np.shape(X)[0]} rows, the groups {res.n_docs}")
        gh = (torch.empty(res.n_docs, device=self.device, dtype=torch.float32), torch.empty(res.n_docs, device=self.device, dtype=torch.float32))
        new = copy.copy(self)
        new.booster = self.booster.refit(X, lambda scores, t: self.grad_hess(scores, res, gh, draw=t), decay, with_tree=True)      # tree t under draw t
        new.evals_result, new.best_iteration, new.best_score = [], None, None
        return new

    def set_background(self, X):
        """GBDT.set_background on the fitted booster: the covers of predict(pred_contrib=True), usually from the training matrix."""
        if self.booster is None:
            raise RuntimeError("fit() first")
        self.booster.set_background(X)
        return self

    def run_letor(self, file_train, file_vali=None, file_test=None, eval_at=5, early_stopping_rounds=None, **loader_kwargs):
        """The shape of the reference's LightGBMLambdaMART.run() on this project's LETOR parser: trains on file_train (validating on file_vali
        when given) and predicts file_test (file_train when absent) -> (y_test, group_test, y_pred) as numpy arrays."""
        def load(path):
            qs = letor.load_letor_queries(path, **loader_kwargs)
            return (np.concatenate([x for _, x, _ in qs]), np.concatenate([lab for _, _, lab in qs]), np.array([lab.size for _, _, lab in qs], np.int64))
        xt, yt, gt = load(file_train)
        ev = load(file_vali) if file_vali else None
        self.fit(xt, yt, gt, eval_set=None if ev is None else (ev[0], ev[1]), eval_group=None if ev is None else ev[2], eval_at=eval_at,
                 early_stopping_rounds=early_stopping_rounds if ev is not None else None)
        xs, ys, gs = load(file_test) if file_test else (xt, yt, gt)
        if xs.shape[1] != xt.shape[1]:
            raise ValueError(f"{file_test} has {xs.shape[1]} features, {file_train} {xt.shape[1]}")
        return ys, gs, self.predict(xs).cpu().numpy()
