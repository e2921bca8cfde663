"""The tree frame's custom LightGBM objectives on the GPU (the reference's ptranking/ltr_tree/util/lightgbm_util.py).

LightGBM asks a custom objective for a gradient and a Hessian per document every boosting round.  The reference computes them with a
Python loop over document pairs; here one fused kernel (csrc/tree.hip) does, over LightGBM's own ragged layout.  The boosting itself stays
in LightGBM — which is not installed where this package is developed, so the hook below is untested end to end:

    obj = TreeObjective(labels, group, "lambdarank", weighting="DeltaNDCG", hessian="sum")
    booster = lightgbm.train(params, train_set, fobj=obj.fobj)              # LightGBM < 4; from 4.0 on: params["objective"] = obj.fobj
    ranker = lightgbm.LGBMRanker(objective=obj.sklearn)

What reading the reference turned up, and what each mode does about it (DESIGN.md has the details):
  1. its lambdarank wrappers pass weighting=True, which the per-query function never recognises: the reference's "lambdarank" is unweighted
     RankNet over NoTies pairs.  The drop-in functions reproduce that; weighting='DeltaNDCG' (opt-in) is real LambdaMART;
  2. its Hessian is signed by rank order (negative for low-ranked documents): hessian='reference'.  hessian='sum' (opt-in) adds the pair
     term to both documents, as LightGBM and XGBoost do, and is never negative;
  3. its Hessian's sigmoid ignores epsilon: kept, in every mode;
  4. its wrappers call group.astype(np.int), which numpy >= 1.24 refuses: nothing here needs np.int;
  5. its sort is not stable: here equal scores rank by original index (the first boosting round has all scores equal).

objective='lambdarank_ndcg' is none of the reference's custom objectives: it is the truncated, normalised lambdarank that the reference's
tree frame runs by default through LightGBM's BUILT-IN objective='lambdarank' (lightgbm_lambdaMART.py:170-185).  The rule is this project's
own, modelled on LightGBM's LambdarankNDCG and compared with nothing of LightGBM's (include/ptranking_amd.h states it): a pair counts where
the labels differ and one of its documents ranks in the first truncation_level; its weight is the Delta-nDCG against maxDCG@truncation_level,
divided by 0.01 + |score difference| under norm; under norm a query's results are scaled by log2(1 + S) / S, S = 2 sum lam.  Its Hessian is
never negative, and a list without a relevant document is exactly 0 where weighting='DeltaNDCG' gives NaN.

objective='rank_xendcg' is LightGBM's second built-in ranking objective, the cross-entropy nDCG loss of Bruch ("An Alternative Cross Entropy
Loss for Learning-to-Rank"), which costs O(n) per query where lambdarank costs O(n T).  Again the rule is this project's own, modelled on
LightGBM's RankXENDCG and compared with nothing of LightGBM's (include/ptranking_amd.h states it): rho = softmax(scores), phi = 2^y - u with
one uniform u per document and round, q = max(1 - rho, 2^-20) (the floor is this project's addition: every output is finite);
a = rho - phi / sum phi, b = rho (A - a / q), c = rho (Bs - b / q) with A = sum a / q and Bs = sum b / q; grad = a + b + c and
hess = rho (1 - rho).  The uniforms come from a counter stream keyed by (objective_seed, draw, the document's index): TreeObjective counts
its calls in .draw, LightGBM calls the objective once per round, so two objects with one seed replay the same rounds bit for bit.
"""
import weakref

import numpy as np
import torch

from . import _lib
from . import functional as F

__all__ = ["TreeObjective", "bucket_queries", "LENGTH_CLASSES", "OBJECTIVES", "lightgbm_custom_obj_ranknet", "lightgbm_custom_obj_lambdarank",
           "lightgbm_custom_obj_listnet", "lightgbm_custom_obj_ranknet_fobj", "lightgbm_custom_obj_lambdarank_fobj",
           "lightgbm_custom_obj_listnet_fobj", "DROP_IN_NAMES", "FIRST_ORDER", "CONSTANT_HESSIAN"]

# Longest list of each launch class.  The kernel has three forms (16 queries per workgroup up to 16 documents, one wavefront per query up
# to 128, one workgroup per query beyond); the one-workgroup form is split further because its LDS rows are sized by the longest list.
LENGTH_CLASSES = (16, 128, 256, 512, 1024, 2048, _lib.MAX_LIST_LEN)
# objective -> (kind, default pair_type): what the reference's wrappers pass (lightgbm_util.py:203-204, :262-264, :351-352)
OBJECTIVES = {"ranknet": ("pair", "All"), "lambdarank": ("pair", "NoTies"), "listnet": ("listnet", None),
              "lambdarank_ndcg": ("lambdarank_ndcg", None),           # the truncated, normalised lambdarank: no wrapper of the reference's
              "rank_xendcg": ("xendcg", None)}                         # cross-entropy nDCG, LightGBM's other built-in: likewise

FIRST_ORDER = False            # lightgbm_util.py:75: True makes the drop-in functions return the constant Hessian
CONSTANT_HESSIAN = 1.0         # lightgbm_util.py:76 (the only value the kernel fills)


def bucket_queries(group, classes=LENGTH_CLASSES):
    """Host side, once per dataset: [(longest list, int32 query indices)] per non-empty length class, shortest first.  Queries of 0
    documents are in no class (they own no output).  A list beyond the last class raises."""
    g = np.asarray(group)
    if g.ndim != 1:
        raise ValueError(f"group must be one-dimensional, got shape {g.shape}")
    if g.size and (g < 0).any():
        raise ValueError("group holds a negative size")
    g = g.astype(np.int64)
    if g.size and int(g.max()) > classes[-1]:
        raise ValueError(f"a query of {int(g.max())} documents exceeds the supported maximum {classes[-1]}")
    out, lo = [], 0
    for hi in classes:
        idx = np.nonzero((g > lo) & (g <= hi))[0].astype(np.int32)
        if idx.size:
            out.append((int(g[idx].max()), idx))
        lo = hi
    return out


def not_applicable(objective, given, defaults):
    """Raises for a setting that `objective` has no use for and that was given a value other than its default."""
    for k, v in given.items():
        d = defaults[k]
        if (v is None) != (d is None) or v != d:
            raise ValueError(f"{k}={v!r} does not apply to objective {objective!r} (leave it at its default {d!r})")


class _Resident:
    """Labels, offsets and the per-class query lists of one dataset, uploaded once."""

    def __init__(self, labels, group, device):
        labels = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.float32)
        group = np.asarray(group).reshape(-1)
        self.buckets_host = bucket_queries(group)
        offsets = np.concatenate([[0], np.cumsum(group.astype(np.int64))]).astype(np.int64)
        if int(offsets[-1]) != labels.size:
            raise ValueError(f"group sums to {int(offsets[-1])} documents, labels holds {labels.size}")
        self.n_docs, self.n_queries = labels.size, group.size
        self.labels_host, self.group_host = labels, group.copy()
        self.labels = torch.from_numpy(labels).to(device)
        self.offsets = torch.from_numpy(offsets).to(device)
        self.buckets = [(m, torch.from_numpy(idx).to(device)) for m, idx in self.buckets_host]

    def same(self, labels, group):
        labels, group = np.asarray(labels).reshape(-1), np.asarray(group).reshape(-1)
        return labels.size == self.n_docs and group.size == self.n_queries and np.array_equal(group, self.group_host) \
            and np.array_equal(labels.astype(np.float32, copy=False), self.labels_host)


class TreeObjective:
    """A custom LightGBM objective whose labels and groups stay on the GPU across boosting rounds.

    TreeObjective(labels, group, objective, ...) uploads the labels and the offsets ONCE and buckets the queries by length class once; a
    call moves only `preds` to the device and `grad` / `hess` back.  objective: 'ranknet' (pair_type 'All'), 'lambdarank' ('NoTies') or
    'listnet', or 'lambdarank_ndcg' (the truncated, normalised lambdarank of the module docstring, with truncation_level, sigmoid and norm;
    pair_type, weighting, epsilon, hessian and gain_type do not apply to it, and a non-default value raises; the other objectives ignore
    its three settings), or 'rank_xendcg' (the cross-entropy nDCG objective of the module docstring, with objective_seed; the same five
    settings do not apply to it; .draw, which starts at 0 and advances by one per __call__ / fobj / sklearn call, numbers the round whose
    uniforms a call draws).  The defaults are the reference's wrappers: unweighted, epsilon 1, the rank-signed Hessian, gain 'Power'.  Opt-in, and not
    what the reference computes: weighting='DeltaNDCG' (real LambdaMART) or 'DeltaGain', hessian='sum' (never negative) or 'constant'.

    __call__(preds) takes a numpy array of any float dtype and returns (grad, hess) as float64 numpy arrays, like the reference; the
    values are fp32-accurate (the kernel computes in fp32; LightGBM stores gradients in fp32 anyway).  labels=None, group=None builds an
    objective for .fobj / .sklearn alone, which take both from their arguments.  There is no CPU path: without a GPU it raises."""

    def __init__(self, labels=None, group=None, objective="lambdarank", pair_type=None, weighting=None, epsilon=1.0, hessian="reference",
                 gain_type="Power", device=None, truncation_level=30, sigmoid=1.0, norm=True, objective_seed=5):
        if objective not in OBJECTIVES:
            raise ValueError(f"objective {objective!r} (supported: {', '.join(map(repr, OBJECTIVES))})")
        self.objective = objective
        self.kind, default_pairs = OBJECTIVES[objective]
        self.pair_type = default_pairs if pair_type is None else pair_type
        self.weighting, self.epsilon, self.hessian, self.gain_type = weighting, float(epsilon), hessian, gain_type
        self.truncation_level, self.sigmoid, self.norm = F.lambdarank_ndcg_settings(truncation_level, sigmoid, norm)
        self.objective_seed, self.draw = F.objective_seed(objective_seed), 0
        if self.kind == "pair":
            F._enum("pair_type", self.pair_type, F.TREE_PAIR_TYPES)
            F._enum("weighting", weighting, F.TREE_WEIGHTINGS)
            if not self.epsilon >= 0.0:
                raise ValueError(f"epsilon must be >= 0, got {epsilon!r}")
        elif self.kind in ("lambdarank_ndcg", "xendcg"):
            not_applicable(objective, dict(pair_type=pair_type, weighting=weighting, epsilon=epsilon, hessian=hessian, gain_type=gain_type),
                           dict(pair_type=None, weighting=None, epsilon=1.0, hessian="reference", gain_type="Power"))
        else:
            F._enum("gain_type", gain_type, F.TREE_GAIN_TYPES)
        F._enum("hessian", hessian, F.TREE_HESSIANS)
        if (labels is None) != (group is None):
            raise ValueError("labels and group come together (or neither, for .fobj / .sklearn)")
        self._device = device
        self._own = None if labels is None else self._resident(labels, group)
        self._by_dataset = {}          # id(dataset) -> (weak reference or the dataset itself, _Resident)
        self._last = None              # .sklearn: the arrays of the previous round
        self.uploads = 0 if labels is None else 1

    def _resident(self, labels, group):
        if not torch.cuda.is_available():
            raise RuntimeError("TreeObjective needs a GPU: ptranking_amd runs on the MI355X HIP path only (no CPU fallback)")
        return _Resident(labels, group, torch.device("cuda" if self._device is None else self._device))

    def _run(self, res, preds):
        preds = np.asarray(preds)
        if preds.size != res.n_docs:
            raise ValueError(f"preds holds {preds.size} documents, the dataset {res.n_docs}")
        p = torch.from_numpy(np.ascontiguousarray(preds.reshape(-1), dtype=np.float32)).to(res.labels.device)
        out = (torch.empty_like(p), torch.empty_like(p))
        for max_len, queries in res.buckets:
            if self.kind == "pair":
                F.tree_pair_grad_hess(p, res.labels, res.offsets, self.pair_type, self.weighting, self.epsilon, self.hessian, queries, max_len, out)
            elif self.kind == "lambdarank_ndcg":
                F.tree_lambdarank_ndcg_grad_hess(p, res.labels, res.offsets, self.truncation_level, self.sigmoid, self.norm, queries, max_len, out)
            elif self.kind == "xendcg":
                F.tree_xendcg_grad_hess(p, res.labels, res.offsets, self.objective_seed, self.draw, None, queries, max_len, out)
            else:
                F.tree_listnet_grad_hess(p, res.labels, res.offsets, self.gain_type, self.hessian, queries, max_len, out)
        self.draw += 1                                                     # one call per boosting round (rank_xendcg's stream reads it)
        both = torch.stack(out).cpu().numpy().astype(np.float64)           # one copy back; every document belongs to a launched query
        return both[0], both[1]

    def __call__(self, preds):
        if self._own is None:
            raise RuntimeError("this TreeObjective was built without labels and group: use .fobj(preds, train_data) or .sklearn(labels, preds, group)")
        return self._run(self._own, preds)

    def fobj(self, preds, train_data):
        """LightGBM's fobj= form: (preds, train_data) -> (grad, hess).  Labels and groups are read from train_data on first use and stay on
        the device for as long as that dataset object lives."""
        hit = self._by_dataset.get(id(train_data))
        if hit is not None and (hit[0]() if isinstance(hit[0], weakref.ref) else hit[0]) is train_data:
            return self._run(hit[1], preds)
        res = self._resident(train_data.get_label(), train_data.get_group())
        self.uploads += 1
        key = id(train_data)
        try:
            ref = weakref.ref(train_data, lambda _r, k=key, d=self._by_dataset: d.pop(k, None))
        except TypeError:
            ref = train_data
        self._by_dataset[key] = (ref, res)
        return self._run(res, preds)

    def sklearn(self, labels, preds, group):
        """LGBMRanker(objective=callable)'s form: (y_true, y_pred, group) -> (grad, hess).  The upload is reused while labels and group
        hold the values of the previous round."""
        if self._last is None or not self._last.same(labels, group):
            self._last = self._resident(labels, group)
            self.uploads += 1
        return self._run(self._last, preds)


# ---- drop-in replacements of the reference's six functions: same names, signatures and results (findings 1 and 2 included), no np.int
_DROP_IN = {}


def _drop_in(objective):
    hessian = "constant" if FIRST_ORDER else "reference"
    obj = _DROP_IN.get((objective, hessian))
    if obj is None:
        obj = _DROP_IN[(objective, hessian)] = TreeObjective(objective=objective, hessian=hessian)
    return obj


def lightgbm_custom_obj_ranknet(labels=None, preds=None, group=None):
    """lightgbm_util.py:185-211: RankNet over 'All' pairs, epsilon 1, no weights, the rank-signed Hessian."""
    return _drop_in("ranknet").sklearn(labels, preds, group)


def lightgbm_custom_obj_ranknet_fobj(preds, train_data):
    """lightgbm_util.py:213-242."""
    return _drop_in("ranknet").fobj(preds, train_data)


def lightgbm_custom_obj_lambdarank(labels=None, preds=None, group=None):
    """lightgbm_util.py:244-271: as the reference RUNS it — 'NoTies' pairs and NO Delta-nDCG weight (its weighting=True selects none)."""
    return _drop_in("lambdarank").sklearn(labels, preds, group)


def lightgbm_custom_obj_lambdarank_fobj(preds, train_data):
    """lightgbm_util.py:273-302."""
    return _drop_in("lambdarank").fobj(preds, train_data)


def lightgbm_custom_obj_listnet(labels=None, preds=None, group=None):
    """lightgbm_util.py:333-359: gain_type 'Power'."""
    return _drop_in("listnet").sklearn(labels, preds, group)


def lightgbm_custom_obj_listnet_fobj(preds, train_data):
    """lightgbm_util.py:361-389."""
    return _drop_in("listnet").fobj(preds, train_data)


DROP_IN_NAMES = ("lightgbm_custom_obj_ranknet", "lightgbm_custom_obj_lambdarank", "lightgbm_custom_obj_listnet",
                 "lightgbm_custom_obj_ranknet_fobj", "lightgbm_custom_obj_lambdarank_fobj", "lightgbm_custom_obj_listnet_fobj")
