"""Tensor-level API of the fused HIP kernels: differentiable losses and device metrics.

Every loss is a `torch.autograd.Function` whose forward launches ONE fused kernel that produces both the loss and
dLoss/dpreds; backward only multiplies by the incoming scalar.  Inputs must be CUDA float32
tensors — there is no CPU path (the reference's CPU op sequences are what `oracle/` restates for the tests).

Shapes: preds / labels `[B, L]` (padded, row-major), optional `lens` int32 `[B]`.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

__all__ = ["ranknet_loss", "lambdarank_loss", "lambdaloss_loss", "approxndcg_loss", "listnet_loss", "listmle_loss",
           "stlistnet_loss", "rankmse_loss", "rankcosine_loss",
           "softrank_loss", "mdprank_loss", "wassrank_loss", "WASS_COST_TYPES", "alphadcg_loss", "div_metrics_at_ks", "ADCG_TOPK_AXES", "ndeval_measures", "div_ideal_order", "NDEVAL_MEASURES","divprob_loss", "expected_ranks", "DIVPROB_OBJECTIVES", "tree_pair_grad_hess", "tree_listnet_grad_hess", "tree_lambdarank_ndcg_grad_hess", "tree_xendcg_grad_hess", "TREE_PAIR_TYPES", "TREE_WEIGHTINGS", "TREE_HESSIANS",
           "TREE_GAIN_TYPES", "smooth_metric_objective", "SMOOTH_METRICS", "gaussian_metric_objective", "pl_uniforms", "sample_rankings_pl", "PL_DISTRIBUTIONS",
           "irgan_uniforms", "irgan_sample", "irgan_point_generator", "irgan_selected", "IRGAN_SAMPLE_MODES", "IRGAN_SELECTED_MODES", "IRGAN_MAX_SAMPLES",
           "irfgan_uniforms", "irfgan_point_sample", "irfgan_pair_sample", "IRFGAN_MODES", "F_DIVERGENCES",
           "adlist_uniforms", "adlist_sample", "ADLIST_MODES", "ADLIST_PROBS", "ADLIST_FAMILIES", "ADLIST_REWARDS", "shuffle_ties_order", "sort_desc", "metrics_at_ks", "sum_f32", "LAMBDALOSS_TYPES",
           "gbdt_bin", "gbdt_quantize", "gbdt_histogram", "gbdt_hist_sub", "gbdt_best_split", "gbdt_partition", "gbdt_add_leaf_values", "gbdt_predict",
           "gbdt_histogram_segments", "gbdt_hist_sub_segments", "gbdt_best_split_slots", "gbdt_partition_segments", "gbdt_segment_items",
           "gbdt_bag_mask", "gbdt_goss", "gbdt_partition_mask", "gbdt_add_tree_binned",
           "gbdt_best_split_cat", "gbdt_best_split_slots_cat", "gbdt_partition_cat", "gbdt_partition_segments_cat", "gbdt_add_tree_binned_cat",
           "gbdt_predict_cat", "gbdt_best_split_cst", "gbdt_best_split_slots_cst", "gbdt_leaf_counts", "gbdt_shap", "SHAP_TABLE_KEYS", "GBDT_MAX_BIN",
           "GBDT_RECORD", "gbdt_predict_leaf", "gbdt_leaf_sums", "gbdt_add_by_leaf"]

# (mdprank_sampled_loss is public too; the *_loss names of __all__ are the losses that take their inputs as given, one row per loss of the
# launch table, and it draws its own; irfgan_loss and adlist_loss are public too: they take a mode, as irgan_selected does)
LAMBDALOSS_TYPES = {"NDCG_Loss1": 0, "NDCG_Loss2": 1, "NDCG_Loss2++": 2}   # ptranking/ltr_adhoc/listwise/lambdaloss.py:27
ADCG_TOPK_AXES = {"reference": 0, "subtopics": 0, 0: 0, "documents": 1, 1: 1}   # PTR_ADCG_TOPK_*
NDEVAL_MEASURES = ("ERR-IA", "nERR-IA", "alpha-DCG", "alpha-nDCG", "NRBP", "nNRBP", "MAP-IA", "P-IA", "strec")   # ndeval.c:1214-1222, its CSV columns
DIVPROB_OBJECTIVES = {"aNDCG": 0, "nERR-IA": 1, "PairCLS": 2, "LambdaPairCLS": 3, 0: 0, 1: 1, 2: 2, 3: 3}   # PTR_DIVPROB_*
TREE_PAIR_TYPES = {"All": 0, "NoTies": 1, "No00": 2, "00": 3}              # PTR_TREE_PAIRS_*; ptranking/ltr_tree/util/lightgbm_util.py:17-60
TREE_WEIGHTINGS = {None: 0, False: 0, "DeltaNDCG": 1, "DeltaGain": 2}       # PTR_TREE_W_*; lightgbm_util.py:80
TREE_HESSIANS = {"reference": 0, "sum": 1, "constant": 2}                   # PTR_TREE_HESS_*
TREE_GAIN_TYPES = {"Power": 0, "Label": 1}                                  # PTR_TREE_GAIN_*; lightgbm_util.py:306
SMOOTH_METRICS = {"P": 0, "AP": 1, "nERR": 2, "nDCG": 3, 0: 0, 1: 1, 2: 2, 3: 3}   # PTR_SMOOTH_*; metric/smooth_metric/metric_as_opt_objective.py
PL_DISTRIBUTIONS = {"PL": 0, "STPL": 1, 0: 0, 1: 1}   # PTR_PL_DIST_*; ptranking/ltr_adhoc/listwise/mdprank.py:19
IRGAN_SAMPLE_MODES = {"POINT_D": 0, "PAIR_D": 1, "PAIR_G": 2}                # PTR_IRGAN_*; irgan_point.py:130-146, irgan_pair.py:140-161, :207-211
IRGAN_SELECTED_MODES = {"POINT_D": 0, "PAIR_D_SVM": 1, "PAIR_D_LOG": 2, "PAIR_G_SVM": 3, "PAIR_G_LOG": 4}   # PTR_IRGAN_SEL_*
IRGAN_MAX_SAMPLES = 64                                                     # PTR_IRGAN_MAX_SAMPLES
IRFGAN_MODES = {"POINT_D": 0, "PAIR_D": 1, "POINT_G": 2, "PAIR_G": 3}       # PTR_IRFGAN_*; irfgan_point.py:200-220, irfgan_pair.py:141-170
F_DIVERGENCES = {"TVar": 0, "KL": 1, "RKL": 2, "PC": 3, "NC": 4, "SH": 5, "JS": 6, "GAN": 7}   # PTR_FDIV_*; ltr_adversarial/util/f_divergence.py
ADLIST_MODES = {"D": 0, "G": 1}                                              # PTR_ADLIST_D, _G; listwise/irgan_list.py:315-341, :344-395
ADLIST_PROBS = {"PL": 0, "BT": 1}                                            # PTR_ADLIST_PL, _BT; util/list_probability.py (PL_D True | False)
ADLIST_FAMILIES = {"IRGAN": 0, "IRFGAN": 1}                                  # PTR_ADLIST_IRGAN, _IRFGAN
ADLIST_REWARDS = {"neg_exp": 0, "neg_lp": 1, "exp_1m": 2, "log_1m": 3}       # PTR_ADLIST_REWARD_*; irgan_list.py:301-310
GBDT_MAX_BIN = 256                                                         # PTR_GBDT_MAX_BIN
GBDT_RECORD = ("gain", "feature", "bin", "left_g", "left_h", "left_count", "right_g", "right_h", "right_count")   # a split record's 9 int64
WASS_COST_TYPES = {"p1": 0, "p2": 1, "eg": 2, "dg": 3, "ddg": 4}   # PTR_WASS_COST_*; wassrank/wasserstein_cost_mat.py:113-139


def _check(name, t, dtype=torch.float32, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: ptranking_amd runs on the MI355X HIP path only (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def _matrix(name, t):
    """The [B, L] check the batch checkers share: a float32 CUDA matrix -> (contiguous tensor, B, L)."""
    t = _check(name, t)
    if t.dim() != 2:
        raise ValueError(f"{name} must be [batch, ranking_size], got {tuple(t.shape)}")
    return (t, *t.shape)


def _list_len(L):
    if L > _lib.MAX_LIST_LEN:
        raise ValueError(f"ranking_size {L} exceeds the supported maximum {_lib.MAX_LIST_LEN}")


def _counts(name, t, B):
    """An optional int32 [B] tensor (lens, ntopics)."""
    return None if t is None else _check(name, t, torch.int32, (B,))


def _batch(preds, second, lens, second_dtype=torch.float32, second_name="labels"):
    preds, B, L = _matrix("preds", preds)
    _list_len(L)
    second = _check(second_name, second, second_dtype, (B, L))
    if second.device != preds.device:
        raise RuntimeError("preds and labels live on different devices")
    return preds, second, _counts("lens", lens, B), B, L


class _FusedLoss(torch.autograd.Function):
    """forward(launch, *inputs) where launch(*inputs) -> (loss 0-d tensor, one grad [B,L] per input); backward scales the grads."""

    @staticmethod
    def forward(ctx, launch, *inputs):
        loss, *grads = launch(*(x.detach() for x in inputs))
        ctx.save_for_backward(*grads)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        return (None, *(g * grad_out for g in ctx.saved_tensors))


def _reduce(loss_q, B, dev):
    out = torch.empty(1, device=dev, dtype=torch.float32)
    _lib.call("ptr_sum_f32", _lib.ptr(loss_q), B, C.c_float(1.0), _lib.ptr(out), _lib.current_stream(dev))
    return out.reshape(())


def _fused(entry, inputs, checked, args, own_loss=False, slots=(("loss_q", None),), tail=()):
    """The one launch path of the fused losses -> (loss, {slot name: tensor}).  The entry point takes (*inputs, *args, loss_out, *slots,
    one gradient per input, *tail, stream): `tail` are further output pointers (tensor or None) behind the gradients; `inputs` are the differentiable [B, L] tensors as the caller passed them and `checked` their detached,
    validated, contiguous forms; `args` the remaining pointer (tensor or None) and scalar arguments in ABI order; `slots` the per-query
    outputs as (name, size), size None meaning [B].  own_loss: the entry point writes loss_out itself; otherwise loss_out is NULL and the
    first slot is summed by the deterministic reduction."""
    B, L = checked[0].shape
    dev = checked[0].device
    parts = {}

    def launch(*xs):
        new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
        outs = [new(max(B, 1) if n is None else n) for _, n in slots]
        grads = [new(B, L) for _ in xs]
        out = new(1) if own_loss else None
        with torch.cuda.device(dev):
            _lib.call(entry, *map(_lib.ptr, xs), *(_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args), _lib.ptr(out),
                      *map(_lib.ptr, outs), *map(_lib.ptr, grads), *map(_lib.ptr, tail), _lib.current_stream(dev))
            loss = out.reshape(()) if own_loss else _reduce(outs[0], B, dev)
        parts.update((name, t[:B] if n is None else t) for (name, n), t in zip(slots, outs))
        return (loss, *grads)

    if any(x.requires_grad for x in inputs):
        return _FusedLoss.apply(launch, *(x.contiguous() for x in inputs)), parts
    return launch(*checked)[0], parts


def _simple(entry, preds, labels, lens, *params, own_loss=False):
    """The (preds, labels, lens, B, L, <params>, loss_out, loss_q, grad, stream) entry points."""
    preds_c, labels, lens, B, L = _batch(preds.detach(), labels, lens)
    return _fused(entry, [preds], [preds_c], [labels, lens, B, L, *params], own_loss)[0]


def _table_loss(name, preds, labels, lens, **values):
    """A loss of _lib.LOSSES (the ones ptr_train_step also serves): its C arguments come from the table."""
    loss = _lib.LOSSES[name]
    return _simple(loss.entry, preds, labels, lens, *loss.c_args(**values))


def ranknet_loss(preds, labels, sigma=1.0, lens=None):
    """RankNet, ptranking/ltr_adhoc/pairwise/ranknet.py:32-36."""
    return _table_loss("ranknet", preds, labels, lens, sigma=sigma)


def lambdarank_loss(preds, labels, sigma=1.0, lens=None):
    """LambdaRank, ptranking/ltr_adhoc/listwise/lambdarank.py:39-56.  `labels` in ideal (descending) order per query."""
    return _table_loss("lambdarank", preds, labels, lens, sigma=sigma)


def lambdaloss_loss(preds, labels, k=5, sigma=1.0, mu=5.0, loss_type="NDCG_Loss2", presort=True, lens=None):
    """LambdaLoss NDCG_Loss1 / NDCG_Loss2 / NDCG_Loss2++, ptranking/ltr_adhoc/listwise/lambdaloss.py:83-132.
    NDCG_Loss1: the reference's [B,L] weights only broadcast against its [B,L,L] tensors at batch size 1; here every query
    of a batch uses its own weights (identical to the reference at B = 1)."""
    if loss_type not in LAMBDALOSS_TYPES:
        raise NotImplementedError(f"LambdaLoss type {loss_type!r} (supported: {sorted(LAMBDALOSS_TYPES)})")
    return _table_loss("lambdaloss", preds, labels, lens, k=k, sigma=sigma, mu=mu, loss_type=LAMBDALOSS_TYPES[loss_type], presort=bool(presort))


def softrank_loss(preds, labels, delta=2.0, top_k=None, lens=None):
    """SoftRank, ptranking/ltr_adhoc/listwise/softrank.py:47-69.  `labels` in ideal (descending) order per query."""
    return _simple("ptr_softrank_fwd_bwd", preds, labels, lens, C.c_float(float(delta)), int(top_k) if top_k else 0)


def listnet_loss(preds, labels, lens=None):
    """ListNet, ptranking/ltr_adhoc/listwise/listnet.py:39."""
    return _table_loss("listnet", preds, labels, lens)


def rankmse_loss(preds, labels, lens=None):
    """RankMSE, ptranking/ltr_adhoc/pointwise/rank_mse.py:13-22 (mean over queries of the per-query squared error sums)."""
    return _simple("ptr_rankmse_fwd_bwd", preds, labels, lens, own_loss=True)


def wassrank_loss(preds, labels, cost_type="eg", lam=0.1, sh_itr=20, gain_base=4.0, non_rele_gap=100.0, var_penalty=math.e,
                  scale_by_max_label=False, lens=None):
    """WassRank, ptranking/ltr_adhoc/listwise/wassrank/wassRank.py:43-88 (mode 'SinkhornOT', smooth_type 'ST', norm_type 'BothST'):
    mean over queries of the entropic Wasserstein distance between softmax(m * preds) and softmax(labels) under the cost `cost_type`
    ('p1', 'p2', 'eg', 'dg', 'ddg'), sh_itr log-domain Sinkhorn iterations with regulariser lam.  m is the query's maximum label when
    scale_by_max_label, else 1.  The reference runs at batch size 1 only; here every query is independent (B = 1 reproduces it), and
    every log-sum-exp takes its own row's maximum, so the loss stays finite where the reference's fp32 evaluation turns NaN."""
    if cost_type not in WASS_COST_TYPES:
        raise NotImplementedError(f"WassRank cost_type {cost_type!r} (supported: {sorted(WASS_COST_TYPES)})")
    return _simple("ptr_wassrank_fwd_bwd", preds, labels, lens, WASS_COST_TYPES[cost_type], C.c_float(float(gain_base)),
                   C.c_float(float(non_rele_gap)), C.c_float(float(var_penalty)), C.c_float(float(lam)), int(sh_itr),
                   int(bool(scale_by_max_label)), own_loss=True)


def rankcosine_loss(preds, labels, lens=None):
    """RankCosine, ptranking/ltr_adhoc/listwise/rank_cosine.py:32."""
    return _simple("ptr_rankcosine_fwd_bwd", preds, labels, lens)


def stlistnet_loss(preds, labels, temperature=1.0, unif=None, lens=None):
    """STListNet, ptranking/ltr_adhoc/listwise/st_listnet.py:41-49.  `unif` = the uniform draws the Gumbel noise is made of
    (default: torch.rand on the device, as the reference does)."""
    preds_c, labels, lens, B, L = _batch(preds.detach(), labels, lens)
    if unif is None:
        unif = torch.rand((B, L), device=preds_c.device)
    unif = _check("unif", unif, torch.float32, (B, L))
    return _fused("ptr_stlistnet_fwd_bwd", [preds], [preds_c], [labels, unif, lens, B, L, C.c_float(float(temperature))])[0]


def listmle_loss(preds, perm, lens=None):
    """ListMLE, ptranking/ltr_adhoc/listwise/listmle.py:82,92-97; `perm` int64 [B,L] from arg_shuffle_ties / shuffle_ties_order."""
    preds_c, perm, lens, B, L = _batch(preds.detach(), perm, lens, torch.int64, "perm")
    return _fused("ptr_listmle_fwd_bwd", [preds], [preds_c], [perm, lens, B, L])[0]


def mdprank_loss(preds, labels, perm, top_k=10, gamma=1.0, lens=None):
    """MDPRank, ptranking/ltr_adhoc/listwise/mdprank.py:46-75: return-weighted ListMLE on the sampled ranking `perm` (int64 [B,L]).
    `preds` are the action scores by ORIGINAL document index (for 'STPL' the caller passes (preds + gumbel) / temperature)."""
    preds_c, perm, lens, B, L = _batch(preds.detach(), perm, lens, torch.int64, "perm")
    labels = _check("labels", labels, shape=(B, L))
    return _fused("ptr_mdprank_fwd_bwd", [preds], [preds_c], [labels, perm, lens, B, L, int(top_k) if top_k else 0, C.c_float(float(gamma))])[0]


def approxndcg_loss(preds, labels, alpha=10.0, presort=True, couple_batch=True, lens=None, grad_scale_override=0.0,
                    return_parts=False):
    """ApproxNDCG, ptranking/ltr_adhoc/listwise/approxNDCG.py:45-62.  couple_batch=True reproduces the reference's batch
    coupling (loss = -(sum DCG_b)(sum 1/IDCG_a)).  With return_parts also returns (dcg_q [B], inv_idcg_q [B], scale [2])."""
    preds_c, labels, lens, B, L = _batch(preds.detach(), labels, lens)
    loss, parts = _fused("ptr_approxndcg_fwd_bwd", [preds], [preds_c],
                         [labels, lens, B, L, C.c_float(float(alpha)), int(bool(presort)), int(bool(couple_batch)), C.c_float(float(grad_scale_override))],
                         own_loss=True, slots=(("dcg_q", None), ("inv_idcg_q", None), ("scale", 2)))
    return (loss, parts) if return_parts else loss


def smooth_metric_objective(preds, labels, metric, alpha=10.0, top_k=None, opt_ideal=True, max_label=None, lens=None, return_parts=False):
    """A ranking metric as the optimisation objective, on smooth ranks: precision_ / AP_ / nERR_ / nDCG_as_opt_objective of
    ptranking/metric/smooth_metric/metric_as_opt_objective.py:12-257 fed with get_approx_ranks(preds, alpha) (approxNDCG.py:19-27), the sum
    over the queries of the reference's one-query loss (minus the smooth metric).  metric 'P' / 'AP' / 'nERR' / 'nDCG'; `labels` in ideal
    (descending) order per query, as the reference asserts; top_k None = the whole list; opt_ideal=True weighs the documents by their input
    (ideal) position, False by their current rank (score descending, index on ties), where a query without a relevant document among its
    top_k contributes nothing, as the reference filters it.  max_label (nERR): None = the batch maximum, found on the device.
    metric='nDCG', opt_ideal=True, top_k=None is ApproxNDCG's per-query form.  With return_parts also returns
    dict(loss_q [B], valid_q [B] (1.0 where the query contributed), ranks [B, L] (the smooth ranks, 0 on padding), max_label_ws [1])."""
    if metric not in SMOOTH_METRICS:
        raise ValueError(f"metric {metric!r} (supported: 'P', 'AP', 'nERR', 'nDCG')")
    preds_c, labels, lens, B, L = _batch(preds.detach(), labels, lens)
    loss, parts = _fused("ptr_smoothmetric_fwd_bwd", [preds], [preds_c],
                         [labels, lens, B, L, SMOOTH_METRICS[metric], int(bool(opt_ideal)), int(top_k) if top_k else 0, C.c_float(float(alpha)),
                          C.c_float(-1.0 if max_label is None else float(max_label))],
                         slots=(("loss_q", None), ("valid_q", None), ("ranks", max(B, 1) * L), ("max_label_ws", 1)))
    if return_parts:
        parts["ranks"] = parts["ranks"][:B * L].view(B, L)
        return loss, parts
    return loss


def gaussian_metric_objective(mus, vars, labels, metric, top_k=None, opt_ideal=True, max_label=None, lens=None, const_std=None, return_parts=False):
    """A ranking metric as the optimisation objective, on Gaussian expected ranks: precision_ / AP_ / nERR_ / nDCG_as_opt_objective of
    ptranking/metric/smooth_metric/metric_as_opt_objective.py:12-257 fed with get_expected_rank(mus, vars)
    (ptranking/ltr_diversification/util/prob_utils.py:62-80) — every document's score a normal variable with mean mus and variance vars,
    its rank 1 + sum_{j != i} erfc((mu_i - mu_j) / sqrt(2 (v_i + v_j))) / 2 — the sum over the queries of the reference's one-query loss,
    differentiable in mus and vars (one launch, both gradients).  vars=None with const_std > 0: every document has the standard deviation
    const_std (get_expected_rank_const, SoftRank's rank model).  metric, labels, top_k, max_label and lens as smooth_metric_objective;
    opt_ideal=False weighs the documents by their current position in the order of the expected ranks (ascending, index on ties).  With
    return_parts also returns dict(loss_q [B], valid_q [B], ranks [B, L] (0 on padding), pos int32 [B, L] (the positions the weights were
    taken at, -1 on padding), max_label_ws [1])."""
    if metric not in SMOOTH_METRICS:
        raise ValueError(f"metric {metric!r} (supported: 'P', 'AP', 'nERR', 'nDCG')")
    if vars is None:
        if const_std is None or not float(const_std) > 0.0:
            raise ValueError(f"without vars, const_std must be > 0 (got {const_std!r})")
        mus_c, B, L = _matrix("mus", mus.detach() if isinstance(mus, torch.Tensor) else mus)
        _list_len(L)
        lens = _counts("lens", lens, B)
        inputs, checked, head, tail = [mus], [mus_c], [None], (None,)
    else:
        if const_std is not None:
            raise ValueError("give vars or const_std, not both")
        mus_c, vars_c, lens, B, L = _divprob_scores(mus.detach() if isinstance(mus, torch.Tensor) else mus,
                                                    vars.detach() if isinstance(vars, torch.Tensor) else vars, lens)
        inputs, checked, head, tail = [mus, vars], [mus_c, vars_c], [], ()
    labels = _check("labels", labels, shape=(B, L))
    if labels.device != mus_c.device:
        raise RuntimeError("mus and labels live on different devices")
    n = max(B, 1) * L
    loss, parts = _fused("ptr_gaussmetric_fwd_bwd", inputs, checked,
                         [*head, labels, lens, B, L, SMOOTH_METRICS[metric], int(bool(opt_ideal)), int(top_k) if top_k else 0,
                          C.c_float(0.0 if const_std is None else float(const_std)), C.c_float(-1.0 if max_label is None else float(max_label))],
                         slots=(("loss_q", None), ("valid_q", None), ("ranks", n), ("pos", n), ("max_label_ws", 1)), tail=tail)
    if return_parts:
        parts["ranks"] = parts["ranks"][:B * L].view(B, L)
        parts["pos"] = parts["pos"][:B * L].view(torch.int32).view(B, L)
        return loss, parts
    return loss


def _div_batch(preds, rele, lens, ntopics):
    """preds [B, L], rele [B, T, L], lens / ntopics int32 [B] or None — checked, contiguous."""
    preds, B, L = _matrix("preds", preds)
    _list_len(L)
    rele = _check("rele", rele)
    if rele.dim() != 3 or rele.shape[0] != B or rele.shape[2] != L:
        raise ValueError(f"rele must be [batch, num_subtopics, ranking_size] = [{B}, T, {L}], got {tuple(rele.shape)}")
    T = rele.shape[1]
    if T < 1 or T > _lib.MAX_SUBTOPICS:
        raise ValueError(f"{T} subtopics: between 1 and {_lib.MAX_SUBTOPICS} are supported")
    if rele.device != preds.device:
        raise RuntimeError("preds and rele live on different devices")
    return preds, rele, _counts("lens", lens, B), _counts("ntopics", ntopics, B), B, T, L


def alphadcg_loss(preds, rele, rt=10.0, alpha=0.5, top_k=10, top_k_axis="reference", lens=None, ntopics=None, return_loss_q=False):
    """DALETOR's alpha-DCG loss, ptranking/ltr_diversification/score_and_sort/daletor.py:9-38, for a padded batch: preds [B, L], rele [B, T, L]
    (per query the reference's q_doc_rele_mat), the sum over queries of the reference's one-query loss.  top_k_axis="reference" keeps the
    first top_k SUBTOPIC rows as the reference's slice does; "documents" keeps the first top_k documents of the presorted ideal order (the
    alpha-DCG@k its docstring describes); top_k=None: no cut-off.  With return_loss_q also returns the per-query losses [B]."""
    if top_k_axis not in ADCG_TOPK_AXES:
        raise ValueError(f"top_k_axis {top_k_axis!r} (supported: 'reference', 'documents')")
    preds_c, rele, lens, ntopics, B, T, L = _div_batch(preds.detach(), rele, lens, ntopics)
    loss, parts = _fused("ptr_alphadcg_fwd_bwd", [preds], [preds_c], [rele, lens, ntopics, B, T, L, C.c_float(float(rt)), C.c_float(float(alpha)),
                                                                     int(top_k) if top_k else 0, ADCG_TOPK_AXES[top_k_axis]])
    return (loss, parts["loss_q"]) if return_loss_q else loss


def div_metrics_at_ks(preds, rele, ks, alpha=0.5, max_label=None, lens=None, ntopics=None):
    """alpha-nDCG@ks, ERR-IA@ks, nERR-IA@ks and the evaluator's `valid` flag for a padded batch -> (andcg [B, nk], err_ia, nerr_ia, valid int32
    [B]) on the device.  Replaces ptranking/base/ranker.py:269-475 (sort, gather) + ptranking/metric/srd/diversity_metric.py.  The ideal
    ranking is the input order (presort).  max_label=None: the two ERR-IA outputs are not computed and come back as None (the reference
    asserts on it, diversity_metric.py:190) — a maximum is never guessed from the batch."""
    preds, rele, lens, ntopics, B, T, L = _div_batch(preds.detach(), rele, lens, ntopics)
    ks = [int(k) for k in ks]
    if len(ks) > _lib.MAX_CUTOFFS:
        raise ValueError(f"at most {_lib.MAX_CUTOFFS} cut-offs")
    dev = preds.device
    new = lambda: torch.empty((B, len(ks)), device=dev, dtype=torch.float32)
    andcg = new()
    err, nerr = (None, None) if max_label is None else (new(), new())
    valid = torch.empty(B, device=dev, dtype=torch.int32)
    ks_arr = (C.c_int32 * max(len(ks), 1))(*ks)
    with torch.cuda.device(dev):
        _lib.call("ptr_div_metrics_at_ks", _lib.ptr(preds), _lib.ptr(rele), _lib.ptr(lens), _lib.ptr(ntopics), B, T, L, ks_arr, len(ks),
                  C.c_float(float(alpha)), C.c_float(0.0 if max_label is None else float(max_label)), _lib.ptr(andcg), _lib.ptr(err),
                  _lib.ptr(nerr), _lib.ptr(valid), _lib.current_stream(dev))
    return andcg, err, nerr, valid


def _ndeval_batch(preds, rele, lens, ntopics):
    """rele [B, T, L] (and preds [B, L] unless None) for ptr_ndeval_measures — checked, contiguous."""
    if preds is not None:
        return _div_batch(preds.detach(), rele, lens, ntopics)
    rele = _check("rele", rele)
    if rele.dim() != 3:
        raise ValueError(f"rele must be [batch, num_subtopics, ranking_size], got {tuple(rele.shape)}")
    B, T, L = rele.shape
    _list_len(L)
    if T < 1 or T > _lib.MAX_SUBTOPICS:
        raise ValueError(f"{T} subtopics: between 1 and {_lib.MAX_SUBTOPICS} are supported")
    return None, rele, _counts("lens", lens, B), _counts("ntopics", ntopics, B), B, T, L


def ndeval_measures(preds, rele, ks=(5, 10, 20), alpha=0.5, beta=0.5, depth=None, lens=None, ntopics=None, return_ideal_order=False):
    """TREC ndeval's diversity measures (ptranking/metric/srd/ndeval.c, the program DivLTREvaluator.fold_evaluation_reproduce runs) for a
    padded batch, in float64 and bit for bit what the program computes per topic -> dict keyed by NDEVAL_MEASURES: "ERR-IA", "nERR-IA",
    "alpha-DCG", "alpha-nDCG", "P-IA" and "strec" [B, nk] at the cut-offs ks (each in 1..20), "NRBP", "nNRBP" and "MAP-IA" [B]; plus
    "actual_subtopics" int32 [B] (the subtopics with a relevant document: 0 marks a query whose measures are all 0 and whose nNRBP is NaN)
    and, with return_ideal_order, "ideal_order" int64 [B, L] (-1 beyond lens).  Judgments are binarised (rele > 0); the run is preds ranked
    as sort_desc ranks it (preds=None: the input order), cut to `depth` documents when given (ndeval -M); the ideal ranking is ndeval's
    greedy over the whole pool, not the input order — which is how these figures differ from div_metrics_at_ks."""
    preds, rele, lens, ntopics, B, T, L = _ndeval_batch(preds, rele, lens, ntopics)
    ks = [int(k) for k in ks]
    if len(ks) > _lib.MAX_CUTOFFS:
        raise ValueError(f"at most {_lib.MAX_CUTOFFS} cut-offs")
    dev, nk = rele.device, len(ks)
    per_k = torch.empty((B, 6, nk), device=dev, dtype=torch.float64)
    per_q = torch.empty((B, 3), device=dev, dtype=torch.float64)
    subtopics = torch.empty(B, device=dev, dtype=torch.int32)
    ideal = torch.empty((B, L), device=dev, dtype=torch.int32) if return_ideal_order else None
    with torch.cuda.device(dev):
        _lib.call("ptr_ndeval_measures", _lib.ptr(preds), _lib.ptr(rele), _lib.ptr(lens), _lib.ptr(ntopics), B, T, L,
                  (C.c_int32 * max(nk, 1))(*ks), nk, C.c_double(float(alpha)), C.c_double(float(beta)), int(depth) if depth else 0,
                  _lib.ptr(per_k), _lib.ptr(per_q), _lib.ptr(subtopics), _lib.ptr(ideal), _lib.current_stream(dev))
    out = {"ERR-IA": per_k[:, 0], "nERR-IA": per_k[:, 1], "alpha-DCG": per_k[:, 2], "alpha-nDCG": per_k[:, 3], "NRBP": per_q[:, 0],
           "nNRBP": per_q[:, 1], "MAP-IA": per_q[:, 2], "P-IA": per_k[:, 4], "strec": per_k[:, 5], "actual_subtopics": subtopics}
    if return_ideal_order:
        out["ideal_order"] = ideal.long()
    return out


def div_ideal_order(rele, alpha=0.5, lens=None, ntopics=None):
    """The ideal ranking the diversification frame presorts by -> int64 [B, L] document indices (-1 beyond lens): ndeval's greedy
    (ndeval.c:351-400; ptranking/metric/srd/diversity_metric.py:113-141 is the same loop over a Python set) on the binarised judgments —
    each round takes the document with the largest sum of (1 - alpha)^(times its subtopic is covered so far), ties to the larger index.
    Gathering a query's documents, and the document axis of its rele, by this order gives what alphadcg_loss, divprob_loss,
    div_metrics_at_ks and DivQueryBatches expect as the given order."""
    _, rele, lens, ntopics, B, T, L = _ndeval_batch(None, rele, lens, ntopics)
    ideal = torch.empty((B, L), device=rele.device, dtype=torch.int32)
    with torch.cuda.device(rele.device):
        _lib.call("ptr_ndeval_measures", None, _lib.ptr(rele), _lib.ptr(lens), _lib.ptr(ntopics), B, T, L, (C.c_int32 * 1)(1), 0,
                  C.c_double(float(alpha)), C.c_double(0.5), 0, None, None, None, _lib.ptr(ideal), _lib.current_stream(rele.device))
    return ideal.long()


def _divprob_scores(mus, vars, lens):
    mus, B, L = _matrix("mus", mus)
    vars = _check("vars", vars, shape=(B, L))
    if vars.device != mus.device:
        raise RuntimeError("mus and vars live on different devices")
    _list_len(L)
    return mus, vars, _counts("lens", lens, B), B, L


def divprob_loss(mus, vars, rele, objective, beta=0.5, top_k=None, top_k_axis="reference", max_label=1.0, norm=True, lens=None, ntopics=None,
                 return_loss_q=False):
    """DivProbRanker's objectives, ptranking/ltr_diversification/score_and_sort/div_prob_ranker.py:29-202 (opt_ideal), for a padded batch:
    mus / vars [B, L] (the predicted mean and variance per document), rele [B, T, L]; the sum over queries of the reference's one-query loss,
    differentiable in mus and vars (one launch, both gradients).  objective: 'aNDCG' (alpha_dcg_as_a_loss; top_k / top_k_axis as
    alphadcg_loss), 'nERR-IA' (err_ia_as_a_loss; top_k cuts documents, max_label), 'PairCLS', 'LambdaPairCLS' (prob_lambda_loss; norm).
    The pairwise terms are the exact -[t log P + (1 - t) log Q] with each logarithm clamped at -100, not the reference's
    `1 - erfc(x) / 2`, which rounds to 1 from |x| = 3.8 on.  With return_loss_q also returns the per-query losses [B]."""
    if objective not in DIVPROB_OBJECTIVES:
        raise ValueError(f"objective {objective!r} (supported: 'aNDCG', 'nERR-IA', 'PairCLS', 'LambdaPairCLS')")
    if top_k_axis not in ADCG_TOPK_AXES:
        raise ValueError(f"top_k_axis {top_k_axis!r} (supported: 'reference', 'documents')")
    mus_c, rele, lens, ntopics, B, T, L = _div_batch(mus.detach(), rele, lens, ntopics)
    vars_c = _check("vars", vars.detach(), shape=(B, L))
    if vars_c.device != mus_c.device:
        raise RuntimeError("mus and vars live on different devices")
    loss, parts = _fused("ptr_divprob_fwd_bwd", [mus, vars], [mus_c, vars_c],
                         [rele, lens, ntopics, B, T, L, DIVPROB_OBJECTIVES[objective], C.c_float(float(beta)), int(top_k) if top_k else 0,
                          ADCG_TOPK_AXES[top_k_axis], C.c_float(float(max_label)), int(bool(norm))])
    return (loss, parts["loss_q"]) if return_loss_q else loss


def expected_ranks(mus, vars, lens=None):
    """Expected ranks [B, L] of documents with independent normal scores: 1 + sum_{j != i} erfc((mu_i - mu_j) / sqrt(2 (var_i + var_j))) / 2,
    ptranking/ltr_diversification/util/prob_utils.py:62-80; padded documents get 0.  Not differentiable (DivProbRanker's 'RERAR' sort key)."""
    mus, vars, lens, B, L = _divprob_scores(mus.detach(), vars.detach(), lens)
    ranks = torch.empty((B, L), device=mus.device, dtype=torch.float32)
    with torch.cuda.device(mus.device):
        _lib.call("ptr_divprob_expected_ranks", _lib.ptr(mus), _lib.ptr(vars), _lib.ptr(lens), B, L, _lib.ptr(ranks),
                  _lib.current_stream(mus.device))
    return ranks


def _enum(name, value, table):
    if value not in table:
        raise ValueError(f"{name} {value!r} (supported: {', '.join(repr(k) for k in table if k is not False)})")
    return table[value]


def _seed64(seed):
    return C.c_uint64(int(seed) & (2 ** 64 - 1))


def _pl_unif(unif, B, S, L, dev):
    if unif is None:
        return None
    unif = _check("unif", unif, torch.float32, (B, S, L))
    if unif.device != dev:
        raise RuntimeError("preds and unif live on different devices")
    return unif


def _pl_samples(samples):
    if int(samples) < 1:
        raise ValueError(f"samples must be >= 1, got {samples}")
    return int(samples)


def pl_uniforms(B, L, samples=1, seed=0, q0=0, device=None):
    """The uniforms sample_rankings_pl / mdprank_sampled_loss draw for (seed, q0): float32 [B, samples, L], multiples of 2^-24 in [0, 1),
    u(seed, q0 + q, s, i) from a counter hash.  q0 = the global index of the batch's first query."""
    _list_len(L)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"device {dev}: ptranking_amd runs on the MI355X HIP path only (no CPU fallback)")
    S = _pl_samples(samples)
    unif = torch.empty((int(B), S, int(L)), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.call("ptr_pl_uniforms", int(B), int(L), S, _seed64(seed), C.c_int64(int(q0)), _lib.ptr(unif), _lib.current_stream(dev))
    return unif


def sample_rankings_pl(preds, samples=1, temperature=1.0, distribution='PL', seed=0, q0=0, lens=None, unif=None, return_action=False):
    """Rankings sampled on the device from the Plackett-Luce model -> int64 [B, samples, L]: the descending order of preds / T + gumbel
    ('PL': the law of sample_ranking_PL's torch.multinomial without replacement, ptranking/ltr_adhoc/util/sampling_utils.py:31-57, with
    no weight that can underflow) or of preds + gumbel ('STPL': sample_ranking_PL_gumbel_softmax, :60-81, and
    ptranking/ltr_adversarial/util/list_sampling.py:38-67 with samples = num_sample_ranking), ties by index.  Counter-based: the same
    (seed, q0 + q) draws the same rankings in any batch; `unif` float32 [B, samples, L] replaces the generator (e.g. the reference's
    torch.rand draws).  Padded positions (lens) hold their own index.  return_action: also the scores ('PL') or (preds + gumbel) / T
    ('STPL') in sampled order, float32 [B, samples, L].  Not differentiable."""
    preds, B, L = _matrix("preds", preds.detach())
    _list_len(L)
    S = _pl_samples(samples)
    dist = _enum("distribution", distribution, PL_DISTRIBUTIONS)
    lens = _counts("lens", lens, B)
    unif = _pl_unif(unif, B, S, L, preds.device)
    perm = torch.empty((B, S, L), device=preds.device, dtype=torch.int64)
    action = torch.empty((B, S, L), device=preds.device, dtype=torch.float32) if return_action else None
    with torch.cuda.device(preds.device):
        _lib.call("ptr_pl_sample", _lib.ptr(preds), _lib.ptr(lens), B, L, S, C.c_float(float(temperature)), dist, _seed64(seed),
                  C.c_int64(int(q0)), _lib.ptr(unif), _lib.ptr(perm), _lib.ptr(action), _lib.current_stream(preds.device))
    return (perm, action) if return_action else perm


def mdprank_sampled_loss(preds, labels, top_k=10, gamma=1.0, temperature=1.0, distribution='PL', samples=1, seed=0, q0=0, lens=None, unif=None,
                         return_perm=False):
    """MDPRank with the sampling inside the kernel (ptranking/ltr_adhoc/listwise/mdprank.py:36-71): one launch draws `samples` rankings per
    query as sample_rankings_pl does and evaluates the return-weighted ListMLE of each; the loss is the sum over queries of the mean over
    the samples, differentiable in preds.  'PL': the loss sees the raw scores (no 1 / T in the gradient); 'STPL': (preds + gumbel) / T.
    samples=1 is the reference's episode.  return_perm: also the sampled rankings, int64 [B, samples, L]."""
    preds_c, labels, lens, B, L = _batch(preds.detach(), labels, lens)
    S = _pl_samples(samples)
    dist = _enum("distribution", distribution, PL_DISTRIBUTIONS)
    unif = _pl_unif(unif, B, S, L, preds_c.device)
    perm = torch.empty((B, S, L), device=preds_c.device, dtype=torch.int64) if return_perm else None
    loss = _fused("ptr_mdprank_sample_fwd_bwd", [preds], [preds_c],
                  [labels, lens, B, L, S, int(top_k) if top_k else 0, C.c_float(float(gamma)), C.c_float(float(temperature)), dist, _seed64(seed),
                   C.c_int64(int(q0)), unif], own_loss=True, tail=(perm,))[0]
    return (loss, perm) if return_perm else loss


def _irgan_samples(samples_per_query):
    if not 1 <= int(samples_per_query) <= IRGAN_MAX_SAMPLES:
        raise ValueError(f"samples_per_query must be in 1 .. {IRGAN_MAX_SAMPLES}, got {samples_per_query}")
    return int(samples_per_query)


def _irgan_batch(preds, num_pos, lens, streams, unif):
    """preds [B, L], num_pos int32 [B], lens, unif [B, streams, L] — checked, contiguous."""
    preds, B, L = _matrix("preds", preds)
    _list_len(L)
    num_pos = _check("num_pos", num_pos, torch.int32, (B,))
    if num_pos.device != preds.device:
        raise RuntimeError("preds and num_pos live on different devices")
    return preds, num_pos, _counts("lens", lens, B), _pl_unif(unif, B, streams, L, preds.device), B, L


def irgan_uniforms(B, L, streams, seed=0, q0=0, device=None):
    """The uniforms irgan_sample (streams = 2: the keys of the positives by document; the negatives by draw under 'POINT_D', by document under
    the pair modes) and irgan_point_generator (streams = draws_per_pos: draw k sits at flat position k of a query's [streams, L] block) draw
    for (seed, q0): float32 [B, streams, L], the counter hash of pl_uniforms."""
    return pl_uniforms(B, L, samples=streams, seed=seed, q0=q0, device=device)


def irgan_sample(preds, num_pos, samples_per_query, mode, temperature=1.0, seed=0, q0=0, lens=None, unif=None):
    """The documents IRGAN's two players train on, drawn on the device -> (pos_idx int64 [B, S], neg_idx int64 [B, S], nsel int32 [B]):
    per query V = nsel valid columns, 0 beyond.  preds: the generator's raw scores [B, L]; num_pos int32 [B]: the relevant documents of a
    list sit at its front (train_presort).  pos_idx: V distinct documents of 0 .. P-1, uniform (randperm(P)[:V]).  mode 'POINT_D'
    (ptranking/ltr_adversarial/pointwise/irgan_point.py:130-146): V = min(P, S), neg_idx V draws WITH replacement from softmax(preds / T);
    'PAIR_D' (pairwise/irgan_pair.py:140-161): V = min(P, n - P, S), V draws without replacement from softmax(preds / T) over the documents
    i >= P; 'PAIR_G' (:207-211): V draws without replacement with weights sigmoid(preds / T) over all documents.  Counter-based: the same
    (seed, q0 + q) draws the same documents in any batch; `unif` float32 [B, 2, L] replaces the generator (irgan_uniforms).  Not
    differentiable."""
    S = _irgan_samples(samples_per_query)
    mode = _enum("mode", mode, IRGAN_SAMPLE_MODES)
    preds, num_pos, lens, unif, B, L = _irgan_batch(preds.detach(), num_pos, lens, 2, unif)
    dev = preds.device
    pos = torch.empty((B, S), device=dev, dtype=torch.int64)
    neg = torch.empty((B, S), device=dev, dtype=torch.int64)
    nsel = torch.empty(B, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.call("ptr_irgan_sample", _lib.ptr(preds), _lib.ptr(lens), _lib.ptr(num_pos), B, L, S, mode, C.c_float(float(temperature)), _seed64(seed),
                  C.c_int64(int(q0)), _lib.ptr(unif), _lib.ptr(pos), _lib.ptr(neg), _lib.ptr(nsel), _lib.current_stream(dev))
    return pos, neg, nsel


def irgan_point_generator(g_preds, d_preds, num_pos, temperature=1.0, lam=0.5, draws_per_pos=5, seed=0, q0=0, lens=None, unif=None, return_parts=False):
    """The generator step of IRGAN_Point (ptranking/ltr_adversarial/pointwise/irgan_point.py:184-217) for a padded batch, one launch: per
    query K = draws_per_pos * P documents are drawn from q = (1 - lam) softmax(g_preds / T) + lam / P on the P relevant documents, and the
    loss is -(1/K) sum over the draws of reward * log p * p / q with reward = 2 (d_preds - 0.5), d_preds [B, L] the discriminator's
    (detached) outputs; the sum over queries, differentiable in g_preds (the importance weight p / q carries gradient, as in the reference).
    A query without a relevant document contributes nothing; a NaN score makes its loss NaN.  unif float32 [B, draws_per_pos, L] replaces
    the generator.  With return_parts also returns dict(loss_q [B], valid_q [B], counts int32 [B, L] (the times each document was drawn))."""
    g_c, num_pos, lens, unif, B, L = _irgan_batch(g_preds.detach(), num_pos, lens, int(draws_per_pos), unif)
    d_preds = _check("d_preds", d_preds.detach(), shape=(B, L))
    if d_preds.device != g_c.device:
        raise RuntimeError("g_preds and d_preds live on different devices")
    counts = torch.empty((B, L), device=g_c.device, dtype=torch.int32) if return_parts else None
    loss, parts = _fused("ptr_irgan_point_gen_fwd_bwd", [g_preds], [g_c],
                         [d_preds, lens, num_pos, B, L, C.c_float(float(temperature)), C.c_float(float(lam)), int(draws_per_pos), _seed64(seed),
                          C.c_int64(int(q0)), unif], own_loss=True, slots=(("loss_q", None), ("valid_q", None)), tail=(counts,))
    if return_parts:
        parts["counts"] = counts
        return loss, parts
    return loss


def irgan_selected(x, nsel, mode, d_sel=None, neg_idx=None, temperature=1.0, lens=None, return_parts=False):
    """IRGAN's losses on the selected documents, loss and gradient in one launch -> the sum over queries, differentiable in x.  nsel int32
    [B]: the valid pairs per query (irgan_sample).  The discriminator's modes take x = its predictions on the compact batch [B, 2 S],
    positives in columns 0 .. V-1 and negatives in V .. 2V-1: 'POINT_D' BCEWithLogits against labels 1 | 0, the mean over 2 V
    (pointwise/irgan_point.py:161-169); 'PAIR_D_SVM' mean max(0, 1 - (d_pos - d_neg)); 'PAIR_D_LOG' -mean log sigmoid(d_pos - d_neg)
    (pairwise/irgan_pair.py:180-184).  The generator's modes 'PAIR_G_SVM' / 'PAIR_G_LOG' take x = g_preds [B, L], neg_idx int64 [B, S]
    and d_sel [B, 2 S] (the discriminator's predictions on the pairs), form the reward (irgan_pair.py:39-42) and
    -mean_k log sigmoid(g_neg_k / T) reward_k (:216-218).  A query with nsel = 0 contributes nothing.  With return_parts also returns
    dict(loss_q [B], valid_q [B])."""
    m = _enum("mode", mode, IRGAN_SELECTED_MODES)
    x_c, B, W = _matrix("x", x.detach())
    dev = x_c.device
    nsel = _check("nsel", nsel, torch.int32, (B,))
    if m >= IRGAN_SELECTED_MODES["PAIR_G_SVM"]:
        _list_len(W)
        if d_sel is None or neg_idx is None:
            raise ValueError(f"mode {mode!r} needs d_sel and neg_idx")
        neg_idx = _check("neg_idx", neg_idx, torch.int64)
        if neg_idx.dim() != 2 or neg_idx.shape[0] != B:
            raise ValueError(f"neg_idx must be [batch, samples_per_query], got {tuple(neg_idx.shape)}")
        S, L = _irgan_samples(neg_idx.shape[1]), W
        d_sel = _check("d_sel", d_sel.detach(), shape=(B, 2 * S))
        lens = _counts("lens", lens, B)
    else:
        if W % 2:
            raise ValueError(f"x must be [batch, 2 * samples_per_query], got {tuple(x_c.shape)}")
        S, L, d_sel, neg_idx, lens = _irgan_samples(W // 2), 1, None, None, None
    if any(t is not None and t.device != dev for t in (nsel, d_sel, neg_idx, lens)):
        raise RuntimeError("x, nsel, d_sel, neg_idx and lens live on different devices")
    loss, parts = _fused("ptr_irgan_sel_fwd_bwd", [x], [x_c], [d_sel, neg_idx, nsel, lens, B, L, S, m, C.c_float(float(temperature))],
                         own_loss=True, slots=(("loss_q", None), ("valid_q", None)))
    return (loss, parts) if return_parts else loss


def _f_div(f_div):
    if f_div == "JSW":
        raise NotImplementedError("f_div 'JSW': the reference's Jensen-Shannon-weighted pair calls torch.log on the Python float math.pi and "
                                  "raises TypeError at its first use (util/f_divergence.py:62-67): there is no behaviour to reproduce")
    return _enum("f_div", f_div, F_DIVERGENCES)


def irfgan_uniforms(B, L, samples_per_query=None, seed=0, q0=0, device=None):
    """The uniforms the IRFGAN samplers draw for (seed, q0), the counter hash of pl_uniforms.  samples_per_query None: float32 [B, 2, L] for
    irfgan_point_sample (stream 0 the keys of the positives, stream 1 the Gumbel uniforms, both by document).  With samples_per_query = S:
    (unif_draw [B, 2, S], unif_bern [B, L, L]) for irfgan_pair_sample — streams 0 and 1 by draw, streams 2 + i by partner j.  unif_bern is
    the one thing of size L x L here: it exists for tests, the product never allocates it."""
    if samples_per_query is None:
        return pl_uniforms(B, L, samples=2, seed=seed, q0=q0, device=device)
    S = _irgan_samples(samples_per_query)
    _list_len(L)
    u = pl_uniforms(B, max(int(L), S), samples=int(L) + 2, seed=seed, q0=q0, device=device)
    return u[:, :2, :S].contiguous(), u[:, 2:, :L].contiguous()


def irfgan_point_sample(preds, num_pos, samples_per_query, seed=0, q0=0, lens=None, unif=None):
    """The documents IRFGAN_Point's players train on (ptranking/ltr_adversarial/pointwise/irfgan_point.py:179-192), drawn on the device ->
    (pos_idx int64 [B, S], neg_idx int64 [B, S], nsel int32 [B]).  V = nsel = min(P, S): pos_idx V distinct documents of 0 .. P-1, uniform
    (randperm(P)[:V]); neg_idx V draws WITHOUT replacement from softmax(preds) over all n documents, by Gumbel keys.  A list with a NaN
    score or without a relevant document gets nsel = 0.  Counter-based: (seed, q0 + q) names the draws in any batch; `unif` float32
    [B, 2, L] replaces the generator (irfgan_uniforms).  Not differentiable."""
    S = _irgan_samples(samples_per_query)
    preds, num_pos, lens, unif, B, L = _irgan_batch(preds.detach(), num_pos, lens, 2, unif)
    dev = preds.device
    pos = torch.empty((B, S), device=dev, dtype=torch.int64)
    neg = torch.empty((B, S), device=dev, dtype=torch.int64)
    nsel = torch.empty(B, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.call("ptr_irfgan_point_sample", _lib.ptr(preds), _lib.ptr(lens), _lib.ptr(num_pos), B, L, S, _seed64(seed), C.c_int64(int(q0)),
                  _lib.ptr(unif), _lib.ptr(pos), _lib.ptr(neg), _lib.ptr(nsel), _lib.current_stream(dev))
    return pos, neg, nsel


def irfgan_pair_sample(preds, labels, num_pos, samples_per_query, seed=0, q0=0, lens=None, unif_draw=None, unif_bern=None, return_count=False):
    """The document pairs IRFGAN_Pair's players train on, drawn on the device without anything of size n x n ->
    (true_head, true_tail, fake_head, fake_tail int64 [B, S], nsel int32 [B]).  labels [B, L]: every list sorted by label descending, no
    label below 0 (the caller's duty: IRFGAN_Pair.fill_global_buffer checks both).  True pairs (ptranking/ltr_adversarial/util/
    pair_sampling.py:26-77): S draws with replacement from w_ij = max(0, y_i - y_j) / (log2(2 + i) log2(2 + j)), i < P, j < n.  Fake pairs
    (:111-122 on irfgan_pair.py:127-130): a Bernoulli mask with P(b_ij) = sigmoid(s_i - s_j) over all n x n pairs, then S draws with
    replacement, uniform over its set bits.  nsel = S, or 0 (no pair named) for an empty list, a NaN score, a list whose first and last
    labels are equal, no true pair of positive weight, or an empty mask.  Counter-based as irfgan_point_sample; unif_draw [B, 2, S] and
    unif_bern [B, L, L] replace the generator (irfgan_uniforms; tests only).  return_count: also the mask's set bits, int32 [B].  Not
    differentiable."""
    S = _irgan_samples(samples_per_query)
    preds, num_pos, lens, _, B, L = _irgan_batch(preds.detach(), num_pos, lens, 2, None)
    dev = preds.device
    labels = _check("labels", labels, shape=(B, L))
    if unif_draw is not None:
        unif_draw = _check("unif_draw", unif_draw, shape=(B, 2, S))
    if unif_bern is not None:
        unif_bern = _check("unif_bern", unif_bern, shape=(B, L, L))
    if any(t is not None and t.device != dev for t in (labels, unif_draw, unif_bern)):
        raise RuntimeError("preds, labels, unif_draw and unif_bern live on different devices")
    out = [torch.empty((B, S), device=dev, dtype=torch.int64) for _ in range(4)]
    nsel = torch.empty(B, device=dev, dtype=torch.int32)
    count = torch.empty(B, device=dev, dtype=torch.int32) if return_count else None
    with torch.cuda.device(dev):
        _lib.call("ptr_irfgan_pair_sample", _lib.ptr(preds), _lib.ptr(labels), _lib.ptr(lens), _lib.ptr(num_pos), B, L, S, _seed64(seed),
                  C.c_int64(int(q0)), _lib.ptr(unif_draw), _lib.ptr(unif_bern), *map(_lib.ptr, out), _lib.ptr(nsel), _lib.ptr(count),
                  _lib.current_stream(dev))
    return (*out, nsel, count) if return_count else (*out, nsel)


def irfgan_loss(x, nsel, mode, f_div, d_fake=None, idx_a=None, idx_b=None, lens=None, return_parts=False):
    """IRFGAN's losses under the f-divergence `f_div` (F_DIVERGENCES), loss and gradient in one launch -> the sum over queries,
    differentiable in x.  With a = activation_f and c = conjugate_f(activation_f(.)) of ptranking/ltr_adversarial/util/f_divergence.py, c
    evaluated in closed form (include/ptranking_amd.h lists them): the reference's literal composition is inf or NaN in fp32 where these
    are finite.  nsel int32 [B] = V, the valid samples per query.  'POINT_D' (pointwise/irfgan_point.py:205): x = the discriminator's
    predictions on the compact batch [B, 2 S], true documents in columns 0 .. V-1, fake in V .. 2V-1; mean c(x_fake) - mean a(x_true).
    'PAIR_D' (pairwise/irfgan_pair.py:143-150): x [B, 4 S] = true heads | true tails | fake heads | fake tails, v = head - tail.
    'POINT_G' (irfgan_point.py:213-216): x = g_preds [B, L], idx_a [B, S] the fake documents, d_fake [B, S] the discriminator's
    predictions on them; -mean_k log softmax(x)[idx_k] c(d_k).  'PAIR_G' (irfgan_pair.py:157-166): idx_a / idx_b the fake heads / tails,
    d_fake [B, 2 S] = heads | tails; -mean_k log sigmoid(x_h - x_t) c(d_h - d_t).  A query with nsel = 0 contributes nothing.  With
    return_parts also returns dict(loss_q [B], valid_q [B])."""
    m = _enum("mode", mode, IRFGAN_MODES)
    f = _f_div(f_div)
    x_c, B, W = _matrix("x", x.detach())
    dev = x_c.device
    nsel = _check("nsel", nsel, torch.int32, (B,))
    if m >= IRFGAN_MODES["POINT_G"]:
        _list_len(W)
        pair = m == IRFGAN_MODES["PAIR_G"]
        if d_fake is None or idx_a is None or (pair and idx_b is None):
            raise ValueError(f"mode {mode!r} needs d_fake, idx_a" + (" and idx_b" if pair else ""))
        idx_a = _check("idx_a", idx_a, torch.int64)
        if idx_a.dim() != 2 or idx_a.shape[0] != B:
            raise ValueError(f"idx_a must be [batch, samples_per_query], got {tuple(idx_a.shape)}")
        S, L = _irgan_samples(idx_a.shape[1]), W
        idx_b = _check("idx_b", idx_b, torch.int64, (B, S)) if pair else None
        d_fake = _check("d_fake", d_fake.detach(), shape=(B, 2 * S if pair else S))
        lens = _counts("lens", lens, B)
    else:
        k = 4 if m == IRFGAN_MODES["PAIR_D"] else 2
        if W % k:
            raise ValueError(f"x must be [batch, {k} * samples_per_query], got {tuple(x_c.shape)}")
        S, L, d_fake, idx_a, idx_b, lens = _irgan_samples(W // k), 1, None, None, None, None
    if any(t is not None and t.device != dev for t in (nsel, d_fake, idx_a, idx_b, lens)):
        raise RuntimeError("x, nsel, d_fake, idx_a, idx_b and lens live on different devices")
    loss, parts = _fused("ptr_irfgan_fwd_bwd", [x], [x_c], [d_fake, idx_a, idx_b, nsel, lens, B, L, S, m, f], own_loss=True,
                         slots=(("loss_q", None), ("valid_q", None)))
    return (loss, parts) if return_parts else loss


def adlist_reward(repTrick, dropLog):
    """The name in ADLIST_REWARDS of get_reward's branch (listwise/irgan_list.py:301-310) for the reference's two switches."""
    return ("neg_exp" if dropLog else "neg_lp") if repTrick else ("exp_1m" if dropLog else "log_1m")


def _adlist_top_k(top_k, L):
    """-> (the C argument, Kw): None or <= 0 is the whole list."""
    k = 0 if top_k is None else int(top_k)
    if k > _lib.MAX_LIST_LEN:
        raise ValueError(f"top_k {k} exceeds the supported maximum {_lib.MAX_LIST_LEN}")
    return (k, k) if k > 0 else (0, L)


def adlist_uniforms(B, L, samples_per_query, mode="D", seed=0, q0=0, device=None):
    """The uniforms adlist_sample (mode 'D': float32 [B, 2 S, L], streams 0 .. S-1 the Gumbel uniforms of the generated rankings, S .. 2S-1
    the tie keys of the standard ones) and adlist_loss(mode='G') ([B, S, L], the same streams 0 .. S-1) draw for (seed, q0)."""
    S = _irgan_samples(samples_per_query)
    return pl_uniforms(B, L, samples=2 * S if _enum("mode", mode, ADLIST_MODES) == 0 else S, seed=seed, q0=q0, device=device)


def adlist_sample(preds, labels, samples_per_query, top_k=None, seed=0, q0=0, lens=None, unif=None):
    """The rankings the list machines' discriminator trains on (ptranking/ltr_adversarial/listwise/irgan_list.py:230-276), one launch ->
    (std_idx, gen_idx int64 [B, S, Kw], kq int32 [B]); Kw = top_k, or L for the whole list (top_k None); per query Kq = kq = min(top_k, n)
    valid positions, 0 beyond.  gen_idx: the first Kq documents of the descending order of preds + gumbel — the prefix of
    sample_rankings_pl(distribution='STPL') for the same (seed, q0), the order of the reference's gumbel_softmax probabilities.  std_idx:
    the first Kq documents by label, descending, ties in uniformly random order (arg_shuffle_ties); labels of -1 sort last.  A list with a
    NaN score gets kq = 0.  `unif` float32 [B, 2 S, L] replaces the generator (adlist_uniforms).  Not differentiable."""
    S = _irgan_samples(samples_per_query)
    preds, labels, lens, B, L = _batch(preds.detach(), labels, lens)
    k, Kw = _adlist_top_k(top_k, L)
    dev = preds.device
    unif = _pl_unif(unif, B, 2 * S, L, dev)
    std = torch.empty((B, S, Kw), device=dev, dtype=torch.int64)
    gen = torch.empty((B, S, Kw), device=dev, dtype=torch.int64)
    kq = torch.empty(B, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.call("ptr_adlist_sample", _lib.ptr(preds), _lib.ptr(labels), _lib.ptr(lens), B, L, S, k, _seed64(seed), C.c_int64(int(q0)),
                  _lib.ptr(unif), _lib.ptr(std), _lib.ptr(gen), _lib.ptr(kq), _lib.current_stream(dev))
    return std, gen, kq


def adlist_loss(x, mode, prob="PL", family="IRGAN", reward="exp_1m", f_div="KL", std_idx=None, gen_idx=None, kq=None, d_preds=None,
                samples_per_query=None, top_k=None, temperature=1.0, seed=0, q0=0, lens=None, unif=None, return_parts=False):
    """The list machines' losses on ranking probabilities, loss and gradient in one launch -> the sum over queries, differentiable in x.
    prob 'PL' | 'BT': the Plackett-Luce or Bradley-Terry log-probability lp of a ranking's scores (util/list_probability.py).
    mode 'D' (irgan_list.py:315-341, irfgan_list.py:322): x = the discriminator's scores of the whole padded batch [B, L]; std_idx, gen_idx
    [B, S, Kw] and kq [B] from adlist_sample; family 'IRGAN': -sum_s lp(x[std_s]) - sum_s log(1 - lp(x[gen_s])); 'IRFGAN':
    mean_s c(lp(x[gen_s])) - mean_s a(lp(x[std_s])) under f_div (F_DIVERGENCES; a, c as irfgan_loss).
    mode 'G' (irgan_list.py:344-395, irfgan_list.py:328-379): x = the generator's scores, d_preds [B, L] the discriminator's (detached)
    scores; the kernel draws samples_per_query Gumbel-softmax rankings per query from (seed, q0) (or unif [B, S, L]) at `temperature`,
    keeps the top_k largest probabilities, and weighs their Plackett-Luce log-probability by the reward of the discriminator's lp of the
    same documents: 'IRGAN' mean_s A_s R_s with `reward` (ADLIST_REWARDS, adlist_reward); 'IRFGAN' -mean_s A_s c(lp).
    A query with kq = 0 (an empty list, a NaN score) contributes nothing.  With return_parts also returns dict(loss_q [B], valid_q [B],
    and under 'G' gen_idx int64 [B, S, Kw])."""
    m = _enum("mode", mode, ADLIST_MODES)
    pr = _enum("prob", prob, ADLIST_PROBS)
    fam = _enum("family", family, ADLIST_FAMILIES)
    rw = _enum("reward", reward, ADLIST_REWARDS)
    f = _f_div(f_div)
    if m == ADLIST_MODES["D"] and (std_idx is None or gen_idx is None or kq is None):
        raise ValueError("mode 'D' needs std_idx, gen_idx and kq (adlist_sample)")
    if m == ADLIST_MODES["G"] and (d_preds is None or samples_per_query is None):
        raise ValueError("mode 'G' needs d_preds and samples_per_query")
    x_c, B, L = _matrix("x", x.detach())
    _list_len(L)
    dev = x_c.device
    lens = _counts("lens", lens, B)
    gout = None
    if m == ADLIST_MODES["D"]:
        std_idx = _check("std_idx", std_idx, torch.int64)
        if std_idx.dim() != 3 or std_idx.shape[0] != B:
            raise ValueError(f"std_idx must be [batch, samples_per_query, top_k], got {tuple(std_idx.shape)}")
        S, Kw = _irgan_samples(std_idx.shape[1]), int(std_idx.shape[2])
        gen_idx = _check("gen_idx", gen_idx, torch.int64, (B, S, Kw))
        kq = _check("kq", kq, torch.int32, (B,))
        k, want = _adlist_top_k(top_k if top_k is not None else (None if Kw == L else Kw), L)
        if want != Kw:
            raise ValueError(f"std_idx holds {Kw} positions per ranking, top_k={top_k!r} asks for {want}")
        d_preds = unif = None
    else:
        S = _irgan_samples(samples_per_query)
        d_preds = _check("d_preds", d_preds.detach(), shape=(B, L))
        k, Kw = _adlist_top_k(top_k, L)
        unif = _pl_unif(unif, B, S, L, dev)
        std_idx = gen_idx = kq = None
        gout = torch.empty((B, S, Kw), device=dev, dtype=torch.int64) if return_parts else None
    if any(t is not None and t.device != dev for t in (std_idx, gen_idx, kq, d_preds, lens)):
        raise RuntimeError("x, std_idx, gen_idx, kq, d_preds and lens live on different devices")
    loss, parts = _fused("ptr_adlist_fwd_bwd", [x], [x_c],
                         [d_preds, std_idx, gen_idx, kq, lens, B, L, S, k, m, pr, fam, rw, f, C.c_float(float(temperature)), _seed64(seed),
                          C.c_int64(int(q0)), unif], own_loss=True, slots=(("loss_q", None), ("valid_q", None)), tail=(gout,))
    if return_parts:
        if gout is not None:
            parts["gen_idx"] = gout
        return loss, parts
    return loss


def _ragged(entry, preds, labels, offsets, queries, max_len, out, *params):
    """The one launch path of the ragged (LightGBM-layout) entry points: (preds, labels, offsets, B, queries, nq, max_len, <params>, grad,
    hess, stream) -> (grad, hess).  preds / labels: flat float32 [N]; offsets: int64 [B + 1], the running sum of the group sizes; queries:
    int32 [nq] or None (all); max_len: the longest launched list (None: read back from `offsets`, which costs a host sync)."""
    preds = _check("preds", preds)
    if preds.dim() != 1:
        raise ValueError(f"preds must be flat [documents], got {tuple(preds.shape)}")
    dev = preds.device
    labels = _check("labels", labels, shape=preds.shape)
    offsets = _check("offsets", offsets, torch.int64)
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError(f"offsets must be [queries + 1], got {tuple(offsets.shape)}")
    B = offsets.numel() - 1
    nq = B
    if queries is not None:
        queries = _check("queries", queries, torch.int32)
        if queries.dim() != 1:
            raise ValueError(f"queries must be [launched queries], got {tuple(queries.shape)}")
        nq = queries.numel()
    if any(t is not None and t.device != dev for t in (labels, offsets, queries)):
        raise RuntimeError("preds, labels, offsets and queries live on different devices")
    if max_len is None:
        max_len = int((offsets[1:] - offsets[:-1]).max()) if B > 0 else 0
    if int(max_len) > _lib.MAX_LIST_LEN:
        raise ValueError(f"a list of {int(max_len)} documents exceeds the supported maximum {_lib.MAX_LIST_LEN}")
    if out is None:
        # documents of queries that are not launched are not written: they read 0
        new = torch.empty_like if queries is None else torch.zeros_like
        out = (new(preds), new(preds))
    grad, hess = (_check(n, t, shape=preds.shape) for n, t in zip(("grad", "hess"), out))
    with torch.cuda.device(dev):
        _lib.call(entry, _lib.ptr(preds), _lib.ptr(labels), _lib.ptr(offsets), B, _lib.ptr(queries), nq, int(max_len), *params, _lib.ptr(grad),
                  _lib.ptr(hess), _lib.current_stream(dev))
    return grad, hess


def tree_pair_grad_hess(preds, labels, offsets, pair_type="NoTies", weighting=None, epsilon=1.0, hessian="reference", queries=None, max_len=None,
                        out=None):
    """Gradient and Hessian per document of the tree frame's pairwise objectives over LightGBM's ragged layout — what
    per_query_gradient_hessian_lambda (ptranking/ltr_tree/util/lightgbm_util.py:120-183) returns for every query of `group`, in one launch.
    preds / labels flat float32 [N], offsets int64 [B + 1]; returns two float32 [N] tensors.  Not differentiable.
    pair_type 'All' / 'NoTies' / 'No00' / '00'; weighting None / 'DeltaNDCG' / 'DeltaGain' (the reference's lambdarank WRAPPERS never
    apply a weight: None reproduces them, 'DeltaNDCG' is real LambdaMART); hessian 'reference' (signed by rank order, negative for
    low-ranked documents), 'sum' (LightGBM's and XGBoost's: never negative) or 'constant' (1.0, the reference's FIRST_ORDER).
    Equal scores rank by original index.  queries (int32 [nq]) / max_len launch a subset, e.g. one length class; `out` = (grad, hess) to
    write into."""
    return _ragged("ptr_tree_pair_grad_hess", preds, labels, offsets, queries, max_len, out, _enum("pair_type", pair_type, TREE_PAIR_TYPES),
                   _enum("weighting", weighting, TREE_WEIGHTINGS), C.c_float(float(epsilon)), _enum("hessian", hessian, TREE_HESSIANS))


def tree_listnet_grad_hess(preds, labels, offsets, gain_type="Power", hessian="reference", queries=None, max_len=None, out=None):
    """ListNet as a tree objective (per_query_gradient_hessian_listnet, lightgbm_util.py:308-330): grad = softmax(preds) - softmax(gain),
    hess = p (1 - p) per query of the ragged batch; gain 2^label - 1 ('Power') or the label ('Label').  Arguments as tree_pair_grad_hess."""
    return _ragged("ptr_tree_listnet_grad_hess", preds, labels, offsets, queries, max_len, out, _enum("gain_type", gain_type, TREE_GAIN_TYPES),
                   _enum("hessian", hessian, TREE_HESSIANS))


def lambdarank_ndcg_settings(truncation_level=30, sigmoid=1.0, norm=True):
    """The three settings of the truncated, normalised lambdarank, validated -> (int truncation_level >= 1, float sigmoid > 0, bool norm).
    A bool is no truncation level, and norm must be a real bool (LightGBM's lambdarank_truncation_level, sigmoid, lambdarank_norm)."""
    t = truncation_level
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)) or t != t or int(t) != t or t < 1:
        raise ValueError(f"lambdarank_truncation_level must be an integer >= 1, got {truncation_level!r}")
    if isinstance(sigmoid, (bool, np.bool_)) or not isinstance(sigmoid, (int, float, np.integer, np.floating)) or not float(np.float32(sigmoid)) > 0.0 \
            or not np.isfinite(np.float32(sigmoid)):
        raise ValueError(f"sigmoid must be a finite float > 0 (in float32), got {sigmoid!r}")
    if not isinstance(norm, (bool, np.bool_)):
        raise ValueError(f"lambdarank_norm must be True or False, got {norm!r}")
    return int(t), float(sigmoid), bool(norm)


def tree_lambdarank_ndcg_grad_hess(preds, labels, offsets, truncation_level=30, sigmoid=1.0, norm=True, queries=None, max_len=None, out=None):
    """Gradient and Hessian per document of the truncated, normalised lambdarank over LightGBM's ragged layout, in one launch
    (ptr_tree_lambdarank_ndcg_grad_hess; include/ptranking_amd.h states the rule in full).  The rule is this project's own, modelled on
    LightGBM's LambdarankNDCG (the objective the reference's tree frame runs by default); it is compared with nothing of LightGBM's.
    A pair counts where the labels differ and one of the two documents ranks in the first `truncation_level`; it weighs
    (g_hi - g_lo) |D_hi - D_lo| / maxDCG@truncation_level, divided by 0.01 + |s_hi - s_lo| under `norm`; lam = sigmoid w p and
    h = sigmoid^2 w p (1 - p) with p = 1 / (1 + exp(sigmoid (s_hi - s_lo))); under `norm` a query's results are scaled by log2(1 + S) / S,
    S = 2 sum lam.  No Hessian is negative; a list without a relevant document is exactly 0 (not NaN, as weighting='DeltaNDCG' gives).
    Arguments and layout as tree_pair_grad_hess."""
    t, sigma, norm = lambdarank_ndcg_settings(truncation_level, sigmoid, norm)
    return _ragged("ptr_tree_lambdarank_ndcg_grad_hess", preds, labels, offsets, queries, max_len, out, min(t, 2 ** 31 - 1), C.c_float(sigma), int(norm))


def _count(name, v, top=2 ** 63 - 1):
    """A non-negative integer setting (no bool, no fraction) -> int."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 <= v <= top or int(v) != v:
        raise ValueError(f"{name} must be an integer in 0 .. {top}, got {v!r}")
    return int(v)


def objective_seed(seed=5):
    """The seed of rank_xendcg's uniforms, validated -> a non-negative int below 2^64 (LightGBM's objective_seed, default 5)."""
    return _count("objective_seed", seed, 2 ** 64 - 1)


def tree_xendcg_grad_hess(preds, labels, offsets, seed=5, draw=0, unif=None, queries=None, max_len=None, out=None):
    """Gradient and Hessian per document of the cross-entropy nDCG objective (LightGBM's objective='rank_xendcg') over LightGBM's ragged
    layout, in one launch that costs O(n) per query (ptr_tree_xendcg_grad_hess; include/ptranking_amd.h states the rule in full).  The rule
    is this project's own, modelled on LightGBM's RankXENDCG; it is compared with nothing of LightGBM's.  With rho = softmax(preds) per
    query, phi = 2^label - u and q = max(1 - rho, 2^-20):  a = rho - phi / sum phi,  b = rho (A - a / q) with A = sum a / q,
    c = rho (Bs - b / q) with Bs = sum b / q,  grad = a + b + c,  hess = rho (1 - rho).  One uniform u in [0, 1) per document comes from
    the counter stream keyed by (seed, draw, the document's global index) — pass the boosting round as `draw` — or from `unif`, a float32
    [documents] tensor that replaces the stream.  A list of one document is exactly 0; a NaN score or label, a negative label or a uniform
    outside [0, 1) gives NaN on that list alone.  Arguments and layout as tree_pair_grad_hess."""
    seed, draw = objective_seed(seed), _count("draw", draw)
    if unif is not None:
        unif = _check("unif", unif, shape=_check("preds", preds).shape)
        if unif.device != preds.device:
            raise RuntimeError("preds and unif live on different devices")
    return _ragged("ptr_tree_xendcg_grad_hess", preds, labels, offsets, queries, max_len, out, _lib.ptr(unif), _seed64(seed), C.c_int64(draw))


def shuffle_ties_order(labels, seed, lens=None):
    """Device replacement for arg_shuffle_ties (ptranking/ltr_adhoc/util/sampling_utils.py:13-28): int64 [B,L] random
    tie-broken label-descending order.  Same distribution, different random stream (not the torch.randperm one)."""
    labels = _check("labels", labels)
    B, L = labels.shape
    if lens is not None:
        lens = _check("lens", lens, torch.int32, (B,))
    perm = torch.empty((B, L), device=labels.device, dtype=torch.int64)
    with torch.cuda.device(labels.device):
        _lib.call("ptr_shuffle_ties_order", _lib.ptr(labels), _lib.ptr(lens), B, L, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                  _lib.ptr(perm), _lib.current_stream(labels.device))
    return perm


def sort_desc(preds, lens=None):
    """torch.sort(preds, dim=1, descending=True) on device -> (values, int64 indices); ties by original index."""
    preds = _check("preds", preds)
    B, L = preds.shape
    if lens is not None:
        lens = _check("lens", lens, torch.int32, (B,))
    vals = torch.empty_like(preds)
    idx = torch.empty((B, L), device=preds.device, dtype=torch.int64)
    with torch.cuda.device(preds.device):
        _lib.call("ptr_sort_desc", _lib.ptr(preds), _lib.ptr(lens), B, L, _lib.ptr(vals), _lib.ptr(idx),
                  _lib.current_stream(preds.device))
    return vals, idx


def metrics_at_ks(preds, labels, ks, presort=False, max_label=None, lens=None, which=("ndcg", "nerr", "ap", "p"),
                  permutation_labels=False):
    """Evaluator prologue + metrics at cut-offs `ks` for one batch -> dict name -> [B, len(ks)] float32 on device.
    Replaces ptranking/base/ranker.py:220-243 + ptranking/metric/adhoc/adhoc_metric.py @ks functions.
    permutation_labels: LABEL_TYPE.Permutation — nDCG's gain is the label itself; nERR is undefined (NotImplementedError)."""
    if permutation_labels and "nerr" in which:
        raise NotImplementedError("nERR is only defined for LABEL_TYPE.MultiLabel (adhoc_metric.py:157-164)")
    preds, labels, lens, B, L = _batch(preds.detach(), labels, lens)
    ks = [int(k) for k in ks]
    if len(ks) > _lib.MAX_CUTOFFS:
        raise ValueError(f"at most {_lib.MAX_CUTOFFS} cut-offs")
    dev = preds.device
    out = {m: torch.empty((B, len(ks)), device=dev, dtype=torch.float32) for m in which}
    ws = torch.empty(1, device=dev, dtype=torch.float32) if ("nerr" in which and max_label is None) else None
    ks_arr = (C.c_int32 * max(len(ks), 1))(*ks)
    ml = -1.0 if max_label is None else float(max_label)
    with torch.cuda.device(dev):
        _lib.call("ptr_metrics_at_ks", _lib.ptr(preds), _lib.ptr(labels), _lib.ptr(lens), B, L, ks_arr, len(ks),
                  int(bool(presort)), int(bool(permutation_labels)), C.c_float(ml), _lib.ptr(ws), _lib.ptr(out.get("ndcg")), _lib.ptr(out.get("nerr")),
                  _lib.ptr(out.get("ap")), _lib.ptr(out.get("p")), _lib.current_stream(dev))
    return out


def sum_f32(x, scale=1.0):
    """Deterministic device sum -> 1-element tensor."""
    x = _check("x", x).reshape(-1)
    out = torch.empty(1, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _lib.call("ptr_sum_f32", _lib.ptr(x), x.numel(), C.c_float(float(scale)), _lib.ptr(out), _lib.current_stream(x.device))
    return out


# ---- the histogram gradient-boosted tree kernels (csrc/gbdt.hip; include/ptranking_amd.h states every contract).  Thin wrappers: gbdt.py
# holds the trainer.  None of them is differentiable.
def _gbdt_bins(bins, F):
    bins = _check("bins", bins, torch.uint8)
    if bins.dim() != 2 or bins.shape[1] % 16 or bins.shape[1] < F:
        raise ValueError(f"bins must be [rows, round_up(F, 16)] uint8 for F={F}, got {tuple(bins.shape)}")
    return bins


def _gbdt_max_bin(max_bin):
    if not 2 <= int(max_bin) <= GBDT_MAX_BIN:
        raise ValueError(f"max_bin must be in 2 .. {GBDT_MAX_BIN}, got {max_bin}")
    return int(max_bin)


def _gbdt_nan_bin(nan_bin, F):
    return _check("nan_bin", nan_bin, torch.int32, (F,))


def gbdt_bin(X, edges, nbins, nan_bin=None):
    """Bin indices of a feature matrix -> uint8 [n, round_up(F, 16)] (pad columns 0).  X float32 [n, F]; edges float32 [F, max_bin - 1],
    ascending per feature; nbins int32 [F].  bin = the number of the feature's first nbins - 1 edges below x, so x <= edges[f, b] is
    bin <= b.  nan_bin (int32 [F], -1: none): a NaN of feature f gets the bin nan_bin[f] (ptr_gbdt_bin_missing)."""
    X = _check("X", X)
    if X.dim() != 2:
        raise ValueError(f"X must be [rows, features], got {tuple(X.shape)}")
    n, F = X.shape
    edges = _check("edges", edges)
    if edges.dim() != 2 or edges.shape[0] != F:
        raise ValueError(f"edges must be [features, max_bin - 1], got {tuple(edges.shape)}")
    max_bin = _gbdt_max_bin(edges.shape[1] + 1)
    nbins = _check("nbins", nbins, torch.int32, (F,))
    stride = (F + 15) // 16 * 16
    bins = torch.empty((n, stride), device=X.device, dtype=torch.uint8)
    with torch.cuda.device(X.device):
        if nan_bin is None:
            _lib.call("ptr_gbdt_bin", _lib.ptr(X), n, F, _lib.ptr(edges), _lib.ptr(nbins), max_bin, stride, _lib.ptr(bins), _lib.current_stream(X.device))
        else:
            _lib.call("ptr_gbdt_bin_missing", _lib.ptr(X), n, F, _lib.ptr(edges), _lib.ptr(nbins), _lib.ptr(_gbdt_nan_bin(nan_bin, F)), max_bin, stride,
                      _lib.ptr(bins), _lib.current_stream(X.device))
    return bins


def gbdt_quantize(grad, hess, flag=None, out=None):
    """Fixed-point gradients and Hessians of one boosting round -> (qg, qh, expo, flag): int32 [n] each, expo int32 [2] = (e_g, e_h) with
    e the largest integer that keeps max|.| 2^e below 2^30, and flag int32 [1], non-zero once a NaN or an infinity was seen (sticky: pass
    the same tensor every round and read it when convenient).  out = (qg, qh, expo) to write into."""
    grad = _check("grad", grad)
    if grad.dim() != 1:
        raise ValueError(f"grad must be flat [rows], got {tuple(grad.shape)}")
    hess = _check("hess", hess, shape=grad.shape)
    dev, n = grad.device, grad.numel()
    flag = torch.zeros(1, device=dev, dtype=torch.int32) if flag is None else _check("flag", flag, torch.int32, (1,))
    if out is None:
        out = (torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.int32), torch.zeros(2, device=dev, dtype=torch.int32))
    qg, qh = (_check(k, t, torch.int32, (n,)) for k, t in zip(("qg", "qh"), out[:2]))
    expo = _check("expo", out[2], torch.int32, (2,))
    state = torch.empty(2, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_quantize", _lib.ptr(grad), _lib.ptr(hess), n, _lib.ptr(qg), _lib.ptr(qh), _lib.ptr(expo), _lib.ptr(flag), _lib.ptr(state),
                  _lib.current_stream(dev))
    return qg, qh, expo, flag


def gbdt_histogram(bins, qg, qh, rows, F, max_bin, hist=None, m=None):
    """ADDS the rows of `rows` (int32 [m]; None: the first m rows, all by default) into hist, int64 [F, max_bin, 3] = (sum qg, sum qh,
    count) per (feature, bin); hist=None starts from zeros.  Integer sums: the bits do not depend on the row order or the launch form."""
    bins = _gbdt_bins(bins, F)
    n, dev = bins.shape[0], bins.device
    max_bin = _gbdt_max_bin(max_bin)
    qg, qh = _check("qg", qg, torch.int32, (n,)), _check("qh", qh, torch.int32, (n,))
    if rows is not None:
        rows = _check("rows", rows, torch.int32)
        if rows.dim() != 1:
            raise ValueError(f"rows must be flat, got {tuple(rows.shape)}")
    m = (n if rows is None else rows.numel()) if m is None else int(m)
    if m < 0 or m > (n if rows is None else rows.numel()):
        raise ValueError(f"m={m} exceeds the row list")
    hist = torch.zeros((F, max_bin, 3), device=dev, dtype=torch.int64) if hist is None else _check("hist", hist, torch.int64, (F, max_bin, 3))
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_histogram", _lib.ptr(bins), bins.shape[1], n, _lib.ptr(qg), _lib.ptr(qh), _lib.ptr(rows), m, F, max_bin, _lib.ptr(hist),
                  _lib.current_stream(dev))
    return hist


def gbdt_hist_sub(parent, child, out=None):
    """parent - child over one histogram (the larger child from the smaller, exactly); out may be `parent` itself."""
    parent = _check("parent", parent, torch.int64)
    if parent.dim() != 3 or parent.shape[2] != 3:
        raise ValueError(f"a histogram is [F, max_bin, 3], got {tuple(parent.shape)}")
    child = _check("child", child, torch.int64, parent.shape)
    out = torch.empty_like(parent) if out is None else _check("out", out, torch.int64, parent.shape)
    with torch.cuda.device(parent.device):
        _lib.call("ptr_gbdt_hist_sub", _lib.ptr(parent), _lib.ptr(child), parent.shape[0], _gbdt_max_bin(parent.shape[1]), _lib.ptr(out),
                  _lib.current_stream(parent.device))
    return out


def gbdt_best_split(hist, nbins, expo, lambda_l2=0.0, min_data_in_leaf=1, min_sum_hessian_in_leaf=1e-3, min_gain_to_split=0.0, out=None, nan_bin=None):
    """The best split of every leaf histogram of a batch -> int64 [leaves, 9] records (GBDT_RECORD; record[0] is the float64 gain's bit
    pattern: .view(torch.float64), -inf without a valid split).  hist int64 [leaves, F, max_bin, 3] (or one [F, max_bin, 3]); nbins int32
    [F]; expo as gbdt_quantize returned it.  float64, ties to the lowest feature, then the lowest bin.  nan_bin (int32 [F], -1: none):
    the scan with learned directions for the missing rows (ptr_gbdt_best_split_missing); record[2] is then bin + 256 * default_left."""
    hist = _check("hist", hist, torch.int64)
    if hist.dim() == 3:
        hist = hist[None]
    if hist.dim() != 4 or hist.shape[3] != 3:
        raise ValueError(f"hist must be [leaves, F, max_bin, 3], got {tuple(hist.shape)}")
    L, F, max_bin = hist.shape[0], hist.shape[1], _gbdt_max_bin(hist.shape[2])
    nbins = _check("nbins", nbins, torch.int32, (F,))
    expo = _check("expo", expo, torch.int32, (2,))
    dev = hist.device
    rec = torch.empty((L, 9), device=dev, dtype=torch.int64) if out is None else _check("out", out, torch.int64, (L, 9))
    ws = torch.empty((max(L * F, 1), 9), device=dev, dtype=torch.int64)
    tail = (C.c_double(float(lambda_l2)), C.c_int64(int(min_data_in_leaf)), C.c_double(float(min_sum_hessian_in_leaf)),
            C.c_double(float(min_gain_to_split)), _lib.ptr(ws), _lib.ptr(rec), _lib.current_stream(dev))
    with torch.cuda.device(dev):
        if nan_bin is None:
            _lib.call("ptr_gbdt_best_split", _lib.ptr(hist), L, F, max_bin, _lib.ptr(nbins), _lib.ptr(expo), *tail)
        else:
            _lib.call("ptr_gbdt_best_split_missing", _lib.ptr(hist), L, F, max_bin, _lib.ptr(nbins), _lib.ptr(_gbdt_nan_bin(nan_bin, F)), _lib.ptr(expo), *tail)
    return rec


def gbdt_partition(bins, rows, feature, bin, F, out=None, left_count=None, also_left=None):
    """Stable partition of a row list by bins[row, feature] <= bin -> (out int32 [m]: the left rows in their order, then the right rows in
    theirs; left_count int32 [1] on the device).  also_left: one more bin that goes left (the NaN bin of a split whose missing rows go
    left), or -1 (ptr_gbdt_partition_missing)."""
    bins = _gbdt_bins(bins, F)
    dev = bins.device
    rows = _check("rows", rows, torch.int32)
    if rows.dim() != 1:
        raise ValueError(f"rows must be flat, got {tuple(rows.shape)}")
    m = rows.numel()
    out = torch.empty_like(rows) if out is None else _check("out", out, torch.int32, (m,))
    left_count = torch.empty(1, device=dev, dtype=torch.int32) if left_count is None else _check("left_count", left_count, torch.int32, (1,))
    ws = torch.empty(int(_lib.query("ptr_gbdt_partition_ws_ints", m)), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        if also_left is None:
            _lib.call("ptr_gbdt_partition", _lib.ptr(bins), bins.shape[1], bins.shape[0], F, _lib.ptr(rows), m, int(feature), int(bin), _lib.ptr(out),
                      _lib.ptr(left_count), _lib.ptr(ws), _lib.current_stream(dev))
        else:
            _lib.call("ptr_gbdt_partition_missing", _lib.ptr(bins), bins.shape[1], bins.shape[0], F, _lib.ptr(rows), m, int(feature), int(bin),
                      int(also_left), _lib.ptr(out), _lib.ptr(left_count), _lib.ptr(ws), _lib.current_stream(dev))
    return out, left_count


def gbdt_add_leaf_values(scores, rows, offsets, values):
    """scores[rows[i]] += values[l] for offsets[l] <= i < offsets[l + 1], in place: all leaves of a finished tree in one launch.  scores
    float32 [n], rows int32 (the leaves' row lists, concatenated), offsets int32 [leaves + 1], values float32 [leaves]."""
    scores = _check("scores", scores)
    rows = _check("rows", rows, torch.int32)
    values = _check("values", values)
    offsets = _check("offsets", offsets, torch.int32, (values.numel() + 1,))
    if not scores.is_contiguous() or scores.dim() != 1 or rows.dim() != 1:
        raise ValueError("scores and rows must be flat and contiguous")
    with torch.cuda.device(scores.device):
        _lib.call("ptr_gbdt_add_leaf_values", _lib.ptr(scores), scores.numel(), _lib.ptr(rows), _lib.ptr(offsets), _lib.ptr(values), values.numel(),
                  rows.numel(), _lib.current_stream(scores.device))
    return scores


def gbdt_predict(X, feature, threshold, left, right, value, tree_offsets, ntrees=None, default_left=None):
    """Scores of raw rows under flat tree arrays -> float32 [n]: per tree the row goes left on x <= threshold; a negative child is leaf ~i;
    tree t owns the nodes tree_offsets[t] .. tree_offsets[t + 1] and the values value[tree_offsets[t] + t ..].  The leaf values are summed
    in tree order in fp32.  ntrees: only the first trees.  default_left (uint8 [nodes]): a NaN feature goes left where the node's byte is
    set, right otherwise (ptr_gbdt_predict_missing)."""
    X = _check("X", X)
    if X.dim() != 2:
        raise ValueError(f"X must be [rows, features], got {tuple(X.shape)}")
    dev = X.device
    tree_offsets = _check("tree_offsets", tree_offsets, torch.int32)
    total = tree_offsets.numel() - 1
    ntrees = total if ntrees is None else int(ntrees)
    if not 0 <= ntrees <= total:
        raise ValueError(f"ntrees={ntrees} outside 0 .. {total}")
    nodes = feature.numel()
    feature, left, right = (_check(k, t, torch.int32, (nodes,)) for k, t in zip(("feature", "left", "right"), (feature, left, right)))
    threshold = _check("threshold", threshold, shape=(nodes,))
    value = _check("value", value, shape=(nodes + total,))
    out = torch.empty(X.shape[0], device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        if default_left is None:
            _lib.call("ptr_gbdt_predict", _lib.ptr(X), X.shape[0], X.shape[1], _lib.ptr(feature), _lib.ptr(threshold), _lib.ptr(left), _lib.ptr(right),
                      _lib.ptr(value), _lib.ptr(tree_offsets), ntrees, _lib.ptr(out), _lib.current_stream(dev))
        else:
            default_left = _check("default_left", default_left, torch.uint8, (nodes,))
            _lib.call("ptr_gbdt_predict_missing", _lib.ptr(X), X.shape[0], X.shape[1], _lib.ptr(feature), _lib.ptr(threshold), _lib.ptr(left),
                      _lib.ptr(right), _lib.ptr(value), _lib.ptr(tree_offsets), _lib.ptr(default_left), ntrees, _lib.ptr(out), _lib.current_stream(dev))
    return out


# ---- one level of a depth-wise tree in batched passes.  The tables (segs, trips, slots) are small HOST arrays (numpy, or anything
# np.asarray takes): the host knows every count from the split records it has read, builds the work lists and uploads each in one copy.
def _gbdt_table(name, table, cols, device):
    t = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, cols) if cols > 1 else np.asarray(table, dtype=np.int64).reshape(-1))
    if t.size and (t.min() < -2 ** 31 or t.max() >= 2 ** 31):
        raise ValueError(f"{name} must hold int32 values")
    return t, torch.from_numpy(t.astype(np.int32)).to(device)


def _gbdt_pool(pool):
    pool = _check("pool", pool, torch.int64)
    if pool.dim() != 4 or pool.shape[3] != 3 or pool.shape[1] < 1:
        raise ValueError(f"pool must be [slots, F >= 1, max_bin, 3], got {tuple(pool.shape)}")
    _gbdt_max_bin(pool.shape[2])
    return pool


def _gbdt_seg_form(m, F, max_bin, total):
    a, out = (C.c_int64 * 4)(int(m), int(F), int(max_bin), int(total)), (C.c_int32 * 8)()
    if _lib.load().ptr_launch_form(b"ptr_gbdt_histogram_segments", a, 4, out, 8) != 0:
        raise RuntimeError(_lib.load().ptr_last_error().decode())
    return tuple(out)


def gbdt_segment_items(counts, F, max_bin):
    """The work list of gbdt_histogram_segments for segments of `counts` rows, on the host -> (items int64 [n, 3] = (segment, first row
    within it, rows), n_direct, n_lds): the segments of at most 256 rows first, whole; then the longer ones in chunks of the row count
    ptr_launch_form gives for the call's total.  Empty segments get no item."""
    counts = np.asarray(counts, np.int64).reshape(-1)
    direct_rows = _gbdt_seg_form(1, F, max_bin, 0)[6]
    small = np.nonzero((counts > 0) & (counts <= direct_rows))[0]
    large = np.nonzero(counts > direct_rows)[0]
    chunk = _gbdt_seg_form(1, F, max_bin, int(counts[large].sum()))[5]
    nch = (counts[large] + chunk - 1) // chunk
    seg = np.repeat(large, nch)
    begin = (np.arange(seg.size) - np.repeat(np.cumsum(nch) - nch, nch)) * chunk
    items = np.concatenate([np.stack([small, np.zeros_like(small), counts[small]], axis=1),
                            np.stack([seg, begin, np.minimum(chunk, counts[seg] - begin)], axis=1)]).astype(np.int64)
    return items, int(small.size), int(seg.size)


def gbdt_histogram_segments(bins, qg, qh, rows, segs, F, max_bin, pool):
    """ADDS, for every segment (start, count, slot) of the host table segs [K, 3], the rows rows[start : start + count] into pool[slot]
    (int64 [slots, F, max_bin, 3], zeroed by the caller): each slot gets the integers gbdt_histogram gives for that row list.  At most two
    launches however many segments: the short ones in the direct form, the long ones cut into row chunks in the LDS form.  A segment that
    leaves the row list or names a slot outside the pool is skipped."""
    bins = _gbdt_bins(bins, F)
    n, dev = bins.shape[0], bins.device
    max_bin = _gbdt_max_bin(max_bin)
    qg, qh = _check("qg", qg, torch.int32, (n,)), _check("qh", qh, torch.int32, (n,))
    rows = _check("rows", rows, torch.int32)
    if rows.dim() != 1:
        raise ValueError(f"rows must be flat, got {tuple(rows.shape)}")
    pool = _gbdt_pool(pool)
    if pool.shape[1] != F or pool.shape[2] != max_bin:
        raise ValueError(f"pool must be [slots, {F}, {max_bin}, 3], got {tuple(pool.shape)}")
    host, segs_d = _gbdt_table("segs", segs, 3, dev)
    K = host.shape[0]
    if K == 0:
        return pool
    items, n_direct, n_lds = gbdt_segment_items(np.where((host[:, 0] >= 0) & (host[:, 0] + host[:, 1] <= rows.numel()), host[:, 1], 0), F, max_bin)
    _, items_d = _gbdt_table("items", items, 3, dev)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_histogram_segments", _lib.ptr(bins), bins.shape[1], n, _lib.ptr(qg), _lib.ptr(qh), _lib.ptr(rows), rows.numel(),
                  _lib.ptr(segs_d), K, _lib.ptr(items_d), n_direct, n_lds, F, max_bin, _lib.ptr(pool), pool.shape[0], _lib.current_stream(dev))
    return pool


def gbdt_hist_sub_segments(pool, trips):
    """pool[out] = pool[parent] - pool[child] for every (parent, child, out) of the host table trips [K, 3], in one launch; out may be the
    parent.  A triple that names a slot outside the pool is skipped."""
    pool = _gbdt_pool(pool)
    host, trips_d = _gbdt_table("trips", trips, 3, pool.device)
    if host.shape[0]:
        with torch.cuda.device(pool.device):
            _lib.call("ptr_gbdt_hist_sub_segments", _lib.ptr(pool), pool.shape[0], pool.shape[1], pool.shape[2], _lib.ptr(trips_d), host.shape[0],
                      _lib.current_stream(pool.device))
    return pool


def gbdt_best_split_slots(pool, slots, nbins, expo, lambda_l2=0.0, min_data_in_leaf=1, min_sum_hessian_in_leaf=1e-3, min_gain_to_split=0.0, out=None,
                          nan_bin=None):
    """gbdt_best_split over the histograms pool[slots[k]] (slots: a host list) -> int64 [K, 9] records, each bit-identical to gbdt_best_split
    on a copy of that slot.  A slot outside the pool gives the record without a split.  nan_bin: as gbdt_best_split."""
    pool = _gbdt_pool(pool)
    dev, F, max_bin = pool.device, pool.shape[1], pool.shape[2]
    nbins = _check("nbins", nbins, torch.int32, (F,))
    expo = _check("expo", expo, torch.int32, (2,))
    host, slots_d = _gbdt_table("slots", slots, 1, dev)
    K = host.shape[0]
    rec = torch.empty((K, 9), device=dev, dtype=torch.int64) if out is None else _check("out", out, torch.int64, (K, 9))
    ws = torch.empty((max(K * F, 1), 9), device=dev, dtype=torch.int64)
    tail = (C.c_double(float(lambda_l2)), C.c_int64(int(min_data_in_leaf)), C.c_double(float(min_sum_hessian_in_leaf)),
            C.c_double(float(min_gain_to_split)), _lib.ptr(ws), _lib.ptr(rec), _lib.current_stream(dev))
    with torch.cuda.device(dev):
        if nan_bin is None:
            _lib.call("ptr_gbdt_best_split_slots", _lib.ptr(pool), pool.shape[0], _lib.ptr(slots_d), K, F, max_bin, _lib.ptr(nbins), _lib.ptr(expo), *tail)
        else:
            _lib.call("ptr_gbdt_best_split_slots_missing", _lib.ptr(pool), pool.shape[0], _lib.ptr(slots_d), K, F, max_bin, _lib.ptr(nbins),
                      _lib.ptr(_gbdt_nan_bin(nan_bin, F)), _lib.ptr(expo), *tail)
    return rec


def gbdt_partition_segments(bins, rows, segs, F, out=None, left_counts=None, also_left=False):
    """Stable partition of every segment (start, count, feature, bin) of the host table segs [K, 4] (disjoint) inside the row list `rows`, as
    gbdt_partition would do each -> (out int32 like rows: a whole row list, the positions outside every segment copied; left_counts int32
    [K] on the device).  A fixed number of launches however many segments; out must not be rows.  A segment that leaves the row list or
    names a feature or bin out of range is left as it was.  also_left=True: segs is [K, 5], the fifth column one more bin that goes left
    or -1, as gbdt_partition's also_left (ptr_gbdt_partition_segments_missing)."""
    bins = _gbdt_bins(bins, F)
    dev = bins.device
    rows = _check("rows", rows, torch.int32)
    if rows.dim() != 1:
        raise ValueError(f"rows must be flat, got {tuple(rows.shape)}")
    host, segs_d = _gbdt_table("segs", segs, 5 if also_left else 4, dev)
    K = host.shape[0]
    out = torch.empty_like(rows) if out is None else _check("out", out, torch.int32, tuple(rows.shape))
    left_counts = torch.zeros(K, device=dev, dtype=torch.int32) if left_counts is None else _check("left_counts", left_counts, torch.int32, (K,))
    per = 1024                                                               # kGbdtPartRows: the rows one workgroup owns
    nblk = np.where((host[:, 0] >= 0) & (host[:, 1] > 0) & (host[:, 0] + host[:, 1] <= rows.numel()), (host[:, 1] + per - 1) // per, 0)
    seg = np.repeat(np.arange(K), nblk)
    blocks = np.stack([seg, np.arange(seg.size) - np.repeat(np.cumsum(nblk) - nblk, nblk)], axis=1)
    _, blocks_d = _gbdt_table("blocks", blocks, 2, dev)
    ws_ints = int(_lib.query("ptr_gbdt_partition_segments_ws_ints", C.c_int64(int(seg.size))))
    ws = torch.empty(ws_ints, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_partition_segments_missing" if also_left else "ptr_gbdt_partition_segments", _lib.ptr(bins), bins.shape[1], bins.shape[0], F, _lib.ptr(rows), rows.numel(), _lib.ptr(segs_d), K,
                  _lib.ptr(blocks_d), int(seg.size), _lib.ptr(out), _lib.ptr(left_counts), _lib.ptr(ws), ws_ints, _lib.current_stream(dev))
    return out, left_counts


# ---- row sampling for the tree trainer (bagging by row or by query, GOSS): include/ptranking_amd.h states the rules.
def gbdt_bag_mask(n, seed, draw, fraction, qid=None, out=None, device=None):
    """The bag of one draw -> uint8 [n], 1 = in the bag: unit r (the row, or qid[r] with qid int32 [n]: whole queries) is kept iff the
    counter stream's u(draw, unit) < float32(fraction).  A Bernoulli draw per unit; fraction in (0, 1]."""
    n = int(n)
    if qid is not None:
        qid = _check("qid", qid, torch.int32, (n,))
        device = qid.device
    if out is not None:
        out = _check("out", out, torch.uint8, (n,))
        device = out.device
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError(f"gbdt_bag_mask on {device}: ptranking_amd runs on the MI355X HIP path only (no CPU fallback)")
    if not 0.0 < float(fraction) <= 1.0:
        raise ValueError(f"fraction must be in (0, 1], got {fraction}")
    if int(draw) < 0:
        raise ValueError(f"draw must be >= 0, got {draw}")
    device = torch.device(device)
    out = torch.empty(n, device=device, dtype=torch.uint8) if out is None else out
    with torch.cuda.device(device):
        _lib.call("ptr_gbdt_bag_mask", n, _lib.ptr(qid), _seed64(seed), int(draw), C.c_float(float(fraction)), _lib.ptr(out), _lib.current_stream(device))
    return out


def gbdt_goss(grad, hess, top_rate, other_rate, seed, draw, out=None, mask=None, info=None):
    """Gradient-based one-side sampling of one round -> (g', h', mask uint8 [n], info int32 [3] = (the bit pattern of tau, the size of the
    top set, the number kept)).  tau is the exact K-th largest |g h| (K = max(1, floor(n top_rate))); the rows at or above it are kept as
    they are, any other row with probability other_rate / (1 - top_rate), its g and h times (1 - top_rate) / other_rate.  out = (g', h')
    to write into; they may be grad and hess themselves."""
    grad = _check("grad", grad)
    if grad.dim() != 1:
        raise ValueError(f"grad must be flat [rows], got {tuple(grad.shape)}")
    hess = _check("hess", hess, shape=grad.shape)
    top_rate, other_rate = float(top_rate), float(other_rate)
    if not (top_rate > 0.0 and other_rate > 0.0 and top_rate + other_rate <= 1.0):
        raise ValueError(f"top_rate and other_rate must be > 0 and sum to at most 1, got {top_rate}, {other_rate}")
    if int(draw) < 0:
        raise ValueError(f"draw must be >= 0, got {draw}")
    dev, n = grad.device, grad.numel()
    out = (torch.empty_like(grad), torch.empty_like(hess)) if out is None else out
    g_out, h_out = (_check(k, t, torch.float32, (n,)) for k, t in zip(("g_out", "h_out"), out))
    mask = torch.empty(n, device=dev, dtype=torch.uint8) if mask is None else _check("mask", mask, torch.uint8, (n,))
    info = torch.zeros(3, device=dev, dtype=torch.int32) if info is None else _check("info", info, torch.int32, (3,))
    ws = torch.empty(int(_lib.query("ptr_gbdt_goss_ws_ints", n)), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_goss", _lib.ptr(grad), _lib.ptr(hess), n, C.c_double(top_rate), C.c_double(other_rate), _seed64(seed), int(draw),
                  _lib.ptr(g_out), _lib.ptr(h_out), _lib.ptr(mask), _lib.ptr(info), _lib.ptr(ws), _lib.current_stream(dev))
    return g_out, h_out, mask, info


def gbdt_partition_mask(mask, rows=None, m=None, out=None, left_count=None):
    """Stable partition of a row list by mask[row] != 0 -> (out int32 [m]: the kept rows in their order, then the others in theirs;
    left_count int32 [1] on the device).  rows=None is the list 0 .. m - 1 (m: all rows of the mask by default).  A row index outside the
    mask is not kept."""
    mask = _check("mask", mask, torch.uint8)
    if mask.dim() != 1:
        raise ValueError(f"mask must be flat [rows], got {tuple(mask.shape)}")
    dev, n = mask.device, mask.numel()
    if rows is not None:
        rows = _check("rows", rows, torch.int32)
        if rows.dim() != 1 or (m is not None and int(m) != rows.numel()):
            raise ValueError(f"rows must be flat and hold m entries, got {tuple(rows.shape)}")
        m = rows.numel()
    m = n if m is None else int(m)
    if m < 0:
        raise ValueError(f"m={m} is negative")
    out = torch.empty(m, device=dev, dtype=torch.int32) if out is None else _check("out", out, torch.int32, (m,))
    left_count = torch.empty(1, device=dev, dtype=torch.int32) if left_count is None else _check("left_count", left_count, torch.int32, (1,))
    ws = torch.empty(int(_lib.query("ptr_gbdt_partition_ws_ints", m)), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_partition_mask", _lib.ptr(mask), n, _lib.ptr(rows), m, _lib.ptr(out), _lib.ptr(left_count), _lib.ptr(ws),
                  _lib.current_stream(dev))
    return out, left_count


def gbdt_add_tree_binned(scores, bins, F, rows, feature, bin, left, right, value, also_left=None):
    """scores[row] += the leaf value one tree gives the BINNED row, for every row of `rows` (int32, distinct; None: all rows), in place.
    The tree as gbdt_predict takes one, with the split bins (int32 [nodes]) in place of the thresholds: left on bins[row, feature] <= bin,
    which is x <= edges[feature, bin], so the value is gbdt_predict's for the raw row.  value float32 [nodes + 1].  also_left (int32
    [nodes]): per node one more bin that goes left, or -1 (ptr_gbdt_add_tree_binned_missing)."""
    scores = _check("scores", scores)
    bins = _gbdt_bins(bins, F)
    n, dev = bins.shape[0], bins.device
    if scores.dim() != 1 or scores.numel() != n or not scores.is_contiguous():
        raise ValueError(f"scores must be flat and contiguous [{n}], got {tuple(scores.shape)}")
    if rows is not None:
        rows = _check("rows", rows, torch.int32)
        if rows.dim() != 1:
            raise ValueError(f"rows must be flat, got {tuple(rows.shape)}")
    nodes = feature.numel()
    feature, bin, left, right = (_check(k, t, torch.int32, (nodes,)) for k, t in zip(("feature", "bin", "left", "right"), (feature, bin, left, right)))
    value = _check("value", value, shape=(nodes + 1,))
    with torch.cuda.device(dev):
        if also_left is None:
            _lib.call("ptr_gbdt_add_tree_binned", _lib.ptr(scores), _lib.ptr(bins), bins.shape[1], n, F, _lib.ptr(rows), n if rows is None else rows.numel(),
                      _lib.ptr(feature), _lib.ptr(bin), _lib.ptr(left), _lib.ptr(right), _lib.ptr(value), nodes, _lib.current_stream(dev))
        else:
            also_left = _check("also_left", also_left, torch.int32, (nodes,))
            _lib.call("ptr_gbdt_add_tree_binned_missing", _lib.ptr(scores), _lib.ptr(bins), bins.shape[1], n, F, _lib.ptr(rows),
                      n if rows is None else rows.numel(), _lib.ptr(feature), _lib.ptr(bin), _lib.ptr(left), _lib.ptr(right), _lib.ptr(value),
                      _lib.ptr(also_left), nodes, _lib.current_stream(dev))
    return scores


# ---- categorical features: set splits (the *_cat entry points; include/ptranking_amd.h states the rule).  is_cat: uint8 [F] on the
# device, non-zero = categorical.  nan_bin stays optional (None: no missing values).  A left set is 256 bits in 4 int64, bit b in word b // 64.
def _gbdt_is_cat(is_cat, F):
    return _check("is_cat", is_cat, torch.uint8, (F,))


def _gbdt_cat_smooth(cat_smooth):
    cat_smooth = float(cat_smooth)
    if not 0.0 <= cat_smooth < float("inf"):
        raise ValueError(f"cat_smooth must be a finite number >= 0, got {cat_smooth}")
    return cat_smooth


def _gbdt_sets(name, sets, rows, device):
    """An int64 [rows, 4] table of left sets on the device: a tensor as it is, anything else (a host array) uploaded."""
    if not isinstance(sets, torch.Tensor):
        sets = torch.from_numpy(np.ascontiguousarray(np.asarray(sets, dtype=np.int64).reshape(-1, 4))).to(device)
    return _check(name, sets.reshape(-1, 4) if sets.dim() == 1 else sets, torch.int64, (rows, 4))


def gbdt_best_split_cat(hist, nbins, expo, is_cat, cat_smooth=10.0, lambda_l2=0.0, min_data_in_leaf=1, min_sum_hessian_in_leaf=1e-3, min_gain_to_split=0.0,
                        out=None, sets=None, nan_bin=None):
    """gbdt_best_split with categorical features -> (records int64 [leaves, 9], sets int64 [leaves, 4]).  A feature with is_cat != 0 is
    searched over SETS of its bins: the used categories (H_c TC / TH >= cat_smooth) sorted by G_c / (H_c + cat_smooth), the first or the
    last i + 1 of them going left.  record[2] of a categorical winner is the number of left categories + 256 * default_left and its set the
    bins that go left; a numeric winner has gbdt_best_split's record and a zero set (ptr_gbdt_best_split_cat)."""
    hist = _check("hist", hist, torch.int64)
    if hist.dim() == 3:
        hist = hist[None]
    if hist.dim() != 4 or hist.shape[3] != 3:
        raise ValueError(f"hist must be [leaves, F, max_bin, 3], got {tuple(hist.shape)}")
    L, F, max_bin = hist.shape[0], hist.shape[1], _gbdt_max_bin(hist.shape[2])
    nbins = _check("nbins", nbins, torch.int32, (F,))
    expo = _check("expo", expo, torch.int32, (2,))
    is_cat, cat_smooth = _gbdt_is_cat(is_cat, F), _gbdt_cat_smooth(cat_smooth)
    nan_bin = None if nan_bin is None else _gbdt_nan_bin(nan_bin, F)
    dev = hist.device
    rec = torch.empty((L, 9), device=dev, dtype=torch.int64) if out is None else _check("out", out, torch.int64, (L, 9))
    sets = torch.empty((L, 4), device=dev, dtype=torch.int64) if sets is None else _check("sets", sets, torch.int64, (L, 4))
    ws = torch.empty((max(L * F, 1), 13), device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_best_split_cat", _lib.ptr(hist), L, F, max_bin, _lib.ptr(nbins), _lib.ptr(nan_bin), _lib.ptr(is_cat), _lib.ptr(expo),
                  C.c_double(float(lambda_l2)), C.c_int64(int(min_data_in_leaf)), C.c_double(float(min_sum_hessian_in_leaf)),
                  C.c_double(float(min_gain_to_split)), C.c_double(cat_smooth), _lib.ptr(ws), _lib.ptr(rec), _lib.ptr(sets), _lib.current_stream(dev))
    return rec, sets


def gbdt_best_split_slots_cat(pool, slots, nbins, expo, is_cat, cat_smooth=10.0, lambda_l2=0.0, min_data_in_leaf=1, min_sum_hessian_in_leaf=1e-3,
                              min_gain_to_split=0.0, out=None, sets=None, nan_bin=None):
    """gbdt_best_split_cat over the histograms pool[slots[k]] (slots: a host list) -> (records int64 [K, 9], sets int64 [K, 4]), each
    bit-identical to gbdt_best_split_cat on a copy of that slot.  A slot outside the pool gives the record without a split and a zero set."""
    pool = _gbdt_pool(pool)
    dev, F, max_bin = pool.device, pool.shape[1], pool.shape[2]
    nbins = _check("nbins", nbins, torch.int32, (F,))
    expo = _check("expo", expo, torch.int32, (2,))
    is_cat, cat_smooth = _gbdt_is_cat(is_cat, F), _gbdt_cat_smooth(cat_smooth)
    nan_bin = None if nan_bin is None else _gbdt_nan_bin(nan_bin, F)
    host, slots_d = _gbdt_table("slots", slots, 1, dev)
    K = host.shape[0]
    rec = torch.empty((K, 9), device=dev, dtype=torch.int64) if out is None else _check("out", out, torch.int64, (K, 9))
    sets = torch.empty((K, 4), device=dev, dtype=torch.int64) if sets is None else _check("sets", sets, torch.int64, (K, 4))
    ws = torch.empty((max(K * F, 1), 13), device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_best_split_slots_cat", _lib.ptr(pool), pool.shape[0], _lib.ptr(slots_d), K, F, max_bin, _lib.ptr(nbins), _lib.ptr(nan_bin),
                  _lib.ptr(is_cat), _lib.ptr(expo), C.c_double(float(lambda_l2)), C.c_int64(int(min_data_in_leaf)),
                  C.c_double(float(min_sum_hessian_in_leaf)), C.c_double(float(min_gain_to_split)), C.c_double(cat_smooth), _lib.ptr(ws), _lib.ptr(rec),
                  _lib.ptr(sets), _lib.current_stream(dev))
    return rec, sets


# ---- monotone and interaction constraints (the *_cst entry points; include/ptranking_amd.h states the rules).  mono: int8 [F] on the
# device; cst: float64 [leaves, 3] = (lo, hi, v) per leaf or None (interaction constraints alone); allowed: uint8 [leaves, F] or None.
def _gbdt_cst_tables(mono, cst, allowed, leaves, F):
    if cst is None and allowed is None:
        raise ValueError("neither cst nor allowed: the unconstrained search serves that")
    if cst is not None:
        if mono is None:
            raise ValueError("cst needs mono")
        cst = _check("cst", cst, torch.float64, (leaves, 3))
    mono = None if mono is None else _check("mono", mono, torch.int8, (F,))
    allowed = None if allowed is None else _check("allowed", allowed, torch.uint8, (leaves, F))
    return mono, cst, allowed


def gbdt_best_split_cst(hist, nbins, expo, mono=None, cst=None, allowed=None, is_cat=None, cat_smooth=10.0, lambda_l2=0.0, min_data_in_leaf=1,
                        min_sum_hessian_in_leaf=1e-3, min_gain_to_split=0.0, out=None, sets=None, nan_bin=None):
    """gbdt_best_split_cat (is_cat None: gbdt_best_split, sets then stay None) under monotone and interaction constraints -> (records int64
    [leaves, 9], sets int64 [leaves, 4] or None).  With cst every candidate takes the bounded gain: its children's values clamped to the
    leaf's [lo, hi], rejected where they break the order mono[f] asks for, gain = G v - GL vL - GR vR; a feature with allowed == 0 at a leaf
    is not searched there (ptr_gbdt_best_split_cst)."""
    hist = _check("hist", hist, torch.int64)
    if hist.dim() == 3:
        hist = hist[None]
    if hist.dim() != 4 or hist.shape[3] != 3:
        raise ValueError(f"hist must be [leaves, F, max_bin, 3], got {tuple(hist.shape)}")
    L, F, max_bin = hist.shape[0], hist.shape[1], _gbdt_max_bin(hist.shape[2])
    nbins = _check("nbins", nbins, torch.int32, (F,))
    expo = _check("expo", expo, torch.int32, (2,))
    mono, cst, allowed = _gbdt_cst_tables(mono, cst, allowed, L, F)
    is_cat, cat_smooth = None if is_cat is None else _gbdt_is_cat(is_cat, F), _gbdt_cat_smooth(cat_smooth)
    nan_bin = None if nan_bin is None else _gbdt_nan_bin(nan_bin, F)
    dev = hist.device
    rec = torch.empty((L, 9), device=dev, dtype=torch.int64) if out is None else _check("out", out, torch.int64, (L, 9))
    if is_cat is not None:
        sets = torch.empty((L, 4), device=dev, dtype=torch.int64) if sets is None else _check("sets", sets, torch.int64, (L, 4))
    elif sets is not None:
        raise ValueError("sets without is_cat")
    ws = torch.empty((max(L * F, 1), 13 if is_cat is not None else 9), device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_best_split_cst", _lib.ptr(hist), L, F, max_bin, _lib.ptr(nbins), _lib.ptr(nan_bin), _lib.ptr(is_cat), _lib.ptr(expo),
                  C.c_double(float(lambda_l2)), C.c_int64(int(min_data_in_leaf)), C.c_double(float(min_sum_hessian_in_leaf)),
                  C.c_double(float(min_gain_to_split)), C.c_double(cat_smooth), _lib.ptr(ws), _lib.ptr(rec), _lib.ptr(sets), _lib.ptr(mono), _lib.ptr(cst),
                  _lib.ptr(allowed), _lib.current_stream(dev))
    return rec, sets


def gbdt_best_split_slots_cst(pool, slots, nbins, expo, mono=None, cst=None, allowed=None, is_cat=None, cat_smooth=10.0, lambda_l2=0.0,
                              min_data_in_leaf=1, min_sum_hessian_in_leaf=1e-3, min_gain_to_split=0.0, out=None, sets=None, nan_bin=None):
    """gbdt_best_split_cst over the histograms pool[slots[k]] (slots: a host list) -> (records int64 [K, 9], sets int64 [K, 4] or None), each
    bit-identical to gbdt_best_split_cst on a copy of that slot; row k of cst and allowed belongs to slots[k]."""
    pool = _gbdt_pool(pool)
    dev, F, max_bin = pool.device, pool.shape[1], pool.shape[2]
    nbins = _check("nbins", nbins, torch.int32, (F,))
    expo = _check("expo", expo, torch.int32, (2,))
    is_cat, cat_smooth = None if is_cat is None else _gbdt_is_cat(is_cat, F), _gbdt_cat_smooth(cat_smooth)
    nan_bin = None if nan_bin is None else _gbdt_nan_bin(nan_bin, F)
    host, slots_d = _gbdt_table("slots", slots, 1, dev)
    K = host.shape[0]
    mono, cst, allowed = _gbdt_cst_tables(mono, cst, allowed, K, F)
    rec = torch.empty((K, 9), device=dev, dtype=torch.int64) if out is None else _check("out", out, torch.int64, (K, 9))
    if is_cat is not None:
        sets = torch.empty((K, 4), device=dev, dtype=torch.int64) if sets is None else _check("sets", sets, torch.int64, (K, 4))
    elif sets is not None:
        raise ValueError("sets without is_cat")
    ws = torch.empty((max(K * F, 1), 13 if is_cat is not None else 9), device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_best_split_slots_cst", _lib.ptr(pool), pool.shape[0], _lib.ptr(slots_d), K, F, max_bin, _lib.ptr(nbins), _lib.ptr(nan_bin),
                  _lib.ptr(is_cat), _lib.ptr(expo), C.c_double(float(lambda_l2)), C.c_int64(int(min_data_in_leaf)),
                  C.c_double(float(min_sum_hessian_in_leaf)), C.c_double(float(min_gain_to_split)), C.c_double(cat_smooth), _lib.ptr(ws), _lib.ptr(rec),
                  _lib.ptr(sets), _lib.ptr(mono), _lib.ptr(cst), _lib.ptr(allowed), _lib.current_stream(dev))
    return rec, sets


def gbdt_partition_cat(bins, rows, feature, bin, F, is_cat, set, default_left=0, nan_bin=None, out=None, left_count=None):
    """gbdt_partition under a node of either kind -> (out, left_count).  At a categorical feature a row goes left iff bit
    bins[row, feature] of `set` (int64 [4]: a device tensor, or a host array that is uploaded) is set; at any other feature on
    bins[row, feature] <= bin, the NaN bin nan_bin[feature] going left too where default_left is set (ptr_gbdt_partition_cat)."""
    bins = _gbdt_bins(bins, F)
    dev = bins.device
    rows = _check("rows", rows, torch.int32)
    if rows.dim() != 1:
        raise ValueError(f"rows must be flat, got {tuple(rows.shape)}")
    if int(default_left) not in (0, 1):
        raise ValueError(f"default_left must be 0 or 1, got {default_left}")
    m = rows.numel()
    is_cat = _gbdt_is_cat(is_cat, F)
    nan_bin = None if nan_bin is None else _gbdt_nan_bin(nan_bin, F)
    set = _gbdt_sets("set", set, 1, dev)
    out = torch.empty_like(rows) if out is None else _check("out", out, torch.int32, (m,))
    left_count = torch.empty(1, device=dev, dtype=torch.int32) if left_count is None else _check("left_count", left_count, torch.int32, (1,))
    ws = torch.empty(int(_lib.query("ptr_gbdt_partition_ws_ints", m)), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_partition_cat", _lib.ptr(bins), bins.shape[1], bins.shape[0], F, _lib.ptr(rows), m, int(feature), int(bin), int(default_left),
                  _lib.ptr(is_cat), _lib.ptr(nan_bin), _lib.ptr(set), _lib.ptr(out), _lib.ptr(left_count), _lib.ptr(ws), _lib.current_stream(dev))
    return out, left_count


def gbdt_partition_segments_cat(bins, rows, segs, sets, F, is_cat, nan_bin=None, out=None, left_counts=None):
    """gbdt_partition_cat over every segment (start, count, feature, bin, default_left) of the host table segs [K, 5], segment k under the
    set sets[k] (int64 [K, 4], host or device) -> (out, left_counts), as gbdt_partition_segments (ptr_gbdt_partition_segments_cat)."""
    bins = _gbdt_bins(bins, F)
    dev = bins.device
    rows = _check("rows", rows, torch.int32)
    if rows.dim() != 1:
        raise ValueError(f"rows must be flat, got {tuple(rows.shape)}")
    host, segs_d = _gbdt_table("segs", segs, 5, dev)
    K = host.shape[0]
    is_cat = _gbdt_is_cat(is_cat, F)
    nan_bin = None if nan_bin is None else _gbdt_nan_bin(nan_bin, F)
    sets = _gbdt_sets("sets", sets, K, dev)
    out = torch.empty_like(rows) if out is None else _check("out", out, torch.int32, tuple(rows.shape))
    left_counts = torch.zeros(K, device=dev, dtype=torch.int32) if left_counts is None else _check("left_counts", left_counts, torch.int32, (K,))
    per = 1024                                                               # kGbdtPartRows: the rows one workgroup owns
    nblk = np.where((host[:, 0] >= 0) & (host[:, 1] > 0) & (host[:, 0] + host[:, 1] <= rows.numel()), (host[:, 1] + per - 1) // per, 0)
    seg = np.repeat(np.arange(K), nblk)
    blocks = np.stack([seg, np.arange(seg.size) - np.repeat(np.cumsum(nblk) - nblk, nblk)], axis=1)
    _, blocks_d = _gbdt_table("blocks", blocks, 2, dev)
    ws_ints = int(_lib.query("ptr_gbdt_partition_segments_ws_ints", C.c_int64(int(seg.size))))
    ws = torch.empty(ws_ints, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_partition_segments_cat", _lib.ptr(bins), bins.shape[1], bins.shape[0], F, _lib.ptr(rows), rows.numel(), _lib.ptr(segs_d),
                  _lib.ptr(sets), K, _lib.ptr(is_cat), _lib.ptr(nan_bin), _lib.ptr(blocks_d), int(seg.size), _lib.ptr(out), _lib.ptr(left_counts),
                  _lib.ptr(ws), ws_ints, _lib.current_stream(dev))
    return out, left_counts


def _gbdt_cat_nodes(cat_index, cat_sets, nodes, device):
    cat_index = _check("cat_index", cat_index, torch.int32, (nodes,))
    cat_sets = _check("cat_sets", cat_sets, torch.int64)
    if cat_sets.dim() != 2 or cat_sets.shape[1] != 4:
        raise ValueError(f"cat_sets must be [sets, 4] int64, got {tuple(cat_sets.shape)}")
    return cat_index, cat_sets


def gbdt_add_tree_binned_cat(scores, bins, F, rows, feature, bin, left, right, value, is_cat, cat_index, cat_sets, default_left=None, nan_bin=None):
    """gbdt_add_tree_binned for a tree with both node kinds: cat_index int32 [nodes] is -1 at a numeric node (left on
    bins[row, feature] <= bin, the NaN bin nan_bin[feature] too where default_left[node] is set), else the row goes left iff bit
    bins[row, feature] of cat_sets[cat_index] (int64 [sets, 4]) is set.  A malformed tree gives NaN (ptr_gbdt_add_tree_binned_cat)."""
    scores = _check("scores", scores)
    bins = _gbdt_bins(bins, F)
    n, dev = bins.shape[0], bins.device
    if scores.dim() != 1 or scores.numel() != n or not scores.is_contiguous():
        raise ValueError(f"scores must be flat and contiguous [{n}], got {tuple(scores.shape)}")
    if rows is not None:
        rows = _check("rows", rows, torch.int32)
        if rows.dim() != 1:
            raise ValueError(f"rows must be flat, got {tuple(rows.shape)}")
    nodes = feature.numel()
    feature, bin, left, right = (_check(k, t, torch.int32, (nodes,)) for k, t in zip(("feature", "bin", "left", "right"), (feature, bin, left, right)))
    value = _check("value", value, shape=(nodes + 1,))
    is_cat = _gbdt_is_cat(is_cat, F)
    cat_index, cat_sets = _gbdt_cat_nodes(cat_index, cat_sets, nodes, dev)
    default_left = None if default_left is None else _check("default_left", default_left, torch.uint8, (nodes,))
    nan_bin = None if nan_bin is None else _gbdt_nan_bin(nan_bin, F)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_add_tree_binned_cat", _lib.ptr(scores), _lib.ptr(bins), bins.shape[1], n, F, _lib.ptr(rows), n if rows is None else rows.numel(),
                  _lib.ptr(feature), _lib.ptr(bin), _lib.ptr(left), _lib.ptr(right), _lib.ptr(value), _lib.ptr(default_left), _lib.ptr(is_cat),
                  _lib.ptr(nan_bin), _lib.ptr(cat_index), _lib.ptr(cat_sets), cat_sets.shape[0], nodes, _lib.current_stream(dev))
    return scores


def gbdt_predict_cat(X, feature, threshold, left, right, value, tree_offsets, is_cat, cat_index, cat_sets, ntrees=None, default_left=None):
    """gbdt_predict for trees with both node kinds (cat_index, cat_sets as gbdt_add_tree_binned_cat takes them, over the nodes of all
    trees).  At a categorical node a NaN follows default_left (right without one), a value that is no integer in 0 .. 255 goes right, any
    other code goes left iff its bit is set: a code the training data never held is in no set.  A malformed tree gives NaN
    (ptr_gbdt_predict_cat)."""
    X = _check("X", X)
    if X.dim() != 2:
        raise ValueError(f"X must be [rows, features], got {tuple(X.shape)}")
    dev = X.device
    tree_offsets = _check("tree_offsets", tree_offsets, torch.int32)
    total = tree_offsets.numel() - 1
    ntrees = total if ntrees is None else int(ntrees)
    if not 0 <= ntrees <= total:
        raise ValueError(f"ntrees={ntrees} outside 0 .. {total}")
    nodes = feature.numel()
    feature, left, right = (_check(k, t, torch.int32, (nodes,)) for k, t in zip(("feature", "left", "right"), (feature, left, right)))
    threshold = _check("threshold", threshold, shape=(nodes,))
    value = _check("value", value, shape=(nodes + total,))
    is_cat = _gbdt_is_cat(is_cat, X.shape[1])
    cat_index, cat_sets = _gbdt_cat_nodes(cat_index, cat_sets, nodes, dev)
    default_left = None if default_left is None else _check("default_left", default_left, torch.uint8, (nodes,))
    out = torch.empty(X.shape[0], device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.call("ptr_gbdt_predict_cat", _lib.ptr(X), X.shape[0], X.shape[1], _lib.ptr(feature), _lib.ptr(threshold), _lib.ptr(left), _lib.ptr(right),
                  _lib.ptr(value), _lib.ptr(tree_offsets), _lib.ptr(default_left), _lib.ptr(is_cat), _lib.ptr(cat_index), _lib.ptr(cat_sets),
                  cat_sets.shape[0], ntrees, _lib.ptr(out), _lib.current_stream(dev))
    return out


# ---- TreeSHAP feature contributions (include/ptranking_amd.h states the rule and the layout of the path tables)
SHAP_TABLE_KEYS = ("path_offsets", "elem_offsets", "leaf_value", "path_node", "path_dir", "path_elem", "elem_feature", "elem_z", "quad_t", "quad_w")
_SHAP_TABLE_TYPES = (torch.int32, torch.int32, torch.float32, torch.int32, torch.uint8, torch.uint8, torch.int32, torch.float64, torch.float64, torch.float64)
SHAP_QUAD = 528                        # the Gauss-Legendre rules of 1 .. 32 nodes on [0, 1]: the rule of Q nodes at Q (Q - 1) / 2


def _gbdt_walk_kind(X, nodes, default_left, is_cat, cat_index, cat_sets):
    """The form a walk over raw rows takes: '' (plain), '_missing' or '_cat', with the checked optional arrays."""
    if (is_cat is None) != (cat_index is None) or (is_cat is None) != (cat_sets is None):
        raise ValueError("is_cat, cat_index and cat_sets go together")
    default_left = None if default_left is None else _check("default_left", default_left, torch.uint8, (nodes,))
    if is_cat is None:
        return ("" if default_left is None else "_missing"), default_left, None, None, None
    is_cat = _gbdt_is_cat(is_cat, X.shape[1])
    cat_index, cat_sets = _gbdt_cat_nodes(cat_index, cat_sets, nodes, X.device)
    return "_cat", default_left, is_cat, cat_index, cat_sets


def gbdt_leaf_counts(X, feature, threshold, left, right, tree_offsets, default_left=None, is_cat=None, cat_index=None, cat_sets=None):
    """The rows of X (float32 [n, F]) per LEAF of every tree -> int64 [nodes + trees], in the layout of gbdt_predict's leaf values: the
    walk of gbdt_predict (gbdt_predict_cat with is_cat, cat_index, cat_sets), one launch, one integer atomic per (row, tree).  The covers of
    gbdt_shap are these counts, summed into node counts on the host (ptr_gbdt_leaf_counts, _missing, _cat)."""
    X = _check("X", X)
    if X.dim() != 2:
        raise ValueError(f"X must be [rows, features], got {tuple(X.shape)}")
    dev = X.device
    tree_offsets = _check("tree_offsets", tree_offsets, torch.int32)
    if tree_offsets.dim() != 1 or tree_offsets.numel() < 1:
        raise ValueError(f"tree_offsets must be [trees + 1], got {tuple(tree_offsets.shape)}")
    ntrees = tree_offsets.numel() - 1
    nodes = feature.numel()
    feature, left, right = (_check(k, t, torch.int32, (nodes,)) for k, t in zip(("feature", "left", "right"), (feature, left, right)))
    threshold = _check("threshold", threshold, shape=(nodes,))
    kind, default_left, is_cat, cat_index, cat_sets = _gbdt_walk_kind(X, nodes, default_left, is_cat, cat_index, cat_sets)
    counts = torch.empty(nodes + ntrees, device=dev, dtype=torch.int64)
    head = (_lib.ptr(X), X.shape[0], X.shape[1], _lib.ptr(feature), _lib.ptr(threshold), _lib.ptr(left), _lib.ptr(right), _lib.ptr(tree_offsets))
    tail = (ntrees, nodes, counts.numel(), _lib.ptr(counts), _lib.current_stream(dev))
    with torch.cuda.device(dev):
        if kind == "":
            _lib.call("ptr_gbdt_leaf_counts", *head, *tail)
        elif kind == "_missing":
            _lib.call("ptr_gbdt_leaf_counts_missing", *head, _lib.ptr(default_left), *tail)
        else:
            _lib.call("ptr_gbdt_leaf_counts_cat", *head, _lib.ptr(default_left), _lib.ptr(is_cat), _lib.ptr(cat_index), _lib.ptr(cat_sets),
                      cat_sets.shape[0], *tail)
    return counts


def gbdt_shap(X, feature, threshold, tables, default_left=None, is_cat=None, cat_index=None, cat_sets=None):
    """TreeSHAP contributions of raw rows X (float32 [n, F]) -> float64 [n, F + 1]: a column per feature, then the expected value.
    feature, threshold (and default_left, cat_index) over the nodes of ALL trees; tables: the path tables (SHAP_TABLE_KEYS, one row per
    leaf; gbdt.shap_tables builds them).  A sub-range of leaves is served by slicing path_offsets, elem_offsets and leaf_value alone.  A
    row's bits depend on the row and the tables alone; malformed tables give NaN (ptr_gbdt_shap, _missing, _cat)."""
    X = _check("X", X)
    if X.dim() != 2:
        raise ValueError(f"X must be [rows, features], got {tuple(X.shape)}")
    dev = X.device
    missing = [k for k in SHAP_TABLE_KEYS if k not in tables]
    if missing:
        raise ValueError(f"tables lacks {', '.join(missing)}")
    tb = {k: _check(k, tables[k], dt) for k, dt in zip(SHAP_TABLE_KEYS, _SHAP_TABLE_TYPES)}
    if any(t.dim() != 1 for t in tb.values()):
        raise ValueError("every path table must be flat")
    nleaves, npath, nelem = tb["leaf_value"].numel(), tb["path_node"].numel(), tb["elem_feature"].numel()
    for k, size in (("path_offsets", nleaves + 1), ("elem_offsets", nleaves + 1), ("path_dir", npath), ("path_elem", npath), ("elem_z", nelem),
                    ("quad_t", SHAP_QUAD), ("quad_w", SHAP_QUAD)):
        if tb[k].numel() != size:
            raise ValueError(f"{k} must have shape ({size},), got {tuple(tb[k].shape)}")
    nodes = feature.numel()
    feature = _check("feature", feature, torch.int32, (nodes,))
    threshold = _check("threshold", threshold, shape=(nodes,))
    kind, default_left, is_cat, cat_index, cat_sets = _gbdt_walk_kind(X, nodes, default_left, is_cat, cat_index, cat_sets)
    phi = torch.empty((X.shape[0], X.shape[1] + 1), device=dev, dtype=torch.float64)
    args = (_lib.ptr(X), X.shape[0], X.shape[1], _lib.ptr(feature), _lib.ptr(threshold), nodes, _lib.ptr(tb["path_offsets"]),
            _lib.ptr(tb["elem_offsets"]), _lib.ptr(tb["leaf_value"]), nleaves, _lib.ptr(tb["path_node"]), _lib.ptr(tb["path_dir"]),
            _lib.ptr(tb["path_elem"]), npath, _lib.ptr(tb["elem_feature"]), _lib.ptr(tb["elem_z"]), nelem, _lib.ptr(tb["quad_t"]), _lib.ptr(tb["quad_w"]))
    with torch.cuda.device(dev):
        if kind == "":
            _lib.call("ptr_gbdt_shap", *args, _lib.ptr(phi), _lib.current_stream(dev))
        elif kind == "_missing":
            _lib.call("ptr_gbdt_shap_missing", *args, _lib.ptr(default_left), _lib.ptr(phi), _lib.current_stream(dev))
        else:
            _lib.call("ptr_gbdt_shap_cat", *args, _lib.ptr(default_left), _lib.ptr(is_cat), _lib.ptr(cat_index), _lib.ptr(cat_sets), cat_sets.shape[0],
                      _lib.ptr(phi), _lib.current_stream(dev))
    return phi


# ---- a trained model on new data: leaf indices, the per-leaf sums of refit, add by leaf (include/ptranking_amd.h states the rules)
def _gbdt_tree_nodes(X, feature, threshold, left, right):
    X = _check("X", X)
    if X.dim() != 2:
        raise ValueError(f"X must be [rows, features], got {tuple(X.shape)}")
    nodes = feature.numel()
    feature, left, right = (_check(k, t, torch.int32, (nodes,)) for k, t in zip(("feature", "left", "right"), (feature, left, right)))
    return X, nodes, feature, _check("threshold", threshold, shape=(nodes,)), left, right


def gbdt_predict_leaf(X, feature, threshold, left, right, tree_offsets, first_tree=0, stop=None, default_left=None, is_cat=None, cat_index=None,
                      cat_sets=None):
    """The leaf every tree puts every row in -> int32 [n, stop - first_tree] (LightGBM's pred_leaf layout): entry [r, t - first_tree] is the
    index l of the leaf ~l of tree t, found by the walk of gbdt_predict (gbdt_predict_cat with is_cat, cat_index, cat_sets) over the flat
    arrays of ALL trees.  A tree of no node gives 0, a malformed tree -1 (ptr_gbdt_predict_leaf, _missing, _cat)."""
    X, nodes, feature, threshold, left, right = _gbdt_tree_nodes(X, feature, threshold, left, right)
    dev = X.device
    tree_offsets = _check("tree_offsets", tree_offsets, torch.int32)
    if tree_offsets.dim() != 1 or tree_offsets.numel() < 1:
        raise ValueError(f"tree_offsets must be [trees + 1], got {tuple(tree_offsets.shape)}")
    total = tree_offsets.numel() - 1
    stop = total if stop is None else int(stop)
    first_tree = int(first_tree)
    if not 0 <= first_tree <= stop <= total:
        raise ValueError(f"trees {first_tree} .. {stop} of {total}")
    kind, default_left, is_cat, cat_index, cat_sets = _gbdt_walk_kind(X, nodes, default_left, is_cat, cat_index, cat_sets)
    out = torch.empty((X.shape[0], stop - first_tree), device=dev, dtype=torch.int32)
    head = (_lib.ptr(X), X.shape[0], X.shape[1], _lib.ptr(feature), _lib.ptr(threshold), _lib.ptr(left), _lib.ptr(right), _lib.ptr(tree_offsets))
    tail = (first_tree, stop - first_tree, nodes, _lib.ptr(out), _lib.current_stream(dev))
    with torch.cuda.device(dev):
        if kind == "":
            _lib.call("ptr_gbdt_predict_leaf", *head, *tail)
        elif kind == "_missing":
            _lib.call("ptr_gbdt_predict_leaf_missing", *head, _lib.ptr(default_left), *tail)
        else:
            _lib.call("ptr_gbdt_predict_leaf_cat", *head, _lib.ptr(default_left), _lib.ptr(is_cat), _lib.ptr(cat_index), _lib.ptr(cat_sets),
                      cat_sets.shape[0], *tail)
    return out


def gbdt_leaf_sums(X, feature, threshold, left, right, qg, qh, nleaves=None, default_left=None, is_cat=None, cat_index=None, cat_sets=None, leaf=None,
                   sums=None):
    """ONE tree over raw rows -> (leaf int32 [n], sums int64 [nleaves, 3]): leaf[r] is the row's leaf index (-1 where the tree loses it) and
    (qg[r], qh[r], 1) is ADDED into sums[leaf[r]]; sums=None starts from zeros, nleaves defaults to nodes + 1.  feature, threshold, left, right
    (and default_left, cat_index) are the tree's own nodes; cat_index indexes cat_sets as given.  Integer atomics only: the sums do not depend
    on the launch form (ptr_launch_form 'ptr_gbdt_leaf_sums': LDS cells up to 1024 leaves, global atomics beyond)."""
    X, nodes, feature, threshold, left, right = _gbdt_tree_nodes(X, feature, threshold, left, right)
    dev, n = X.device, X.shape[0]
    qg, qh = _check("qg", qg, torch.int32, (n,)), _check("qh", qh, torch.int32, (n,))
    nleaves = nodes + 1 if nleaves is None else int(nleaves)
    if nleaves < 0:
        raise ValueError(f"nleaves={nleaves}")
    kind, default_left, is_cat, cat_index, cat_sets = _gbdt_walk_kind(X, nodes, default_left, is_cat, cat_index, cat_sets)
    leaf = torch.empty(n, device=dev, dtype=torch.int32) if leaf is None else _check("leaf", leaf, torch.int32, (n,))
    sums = torch.zeros((nleaves, 3), device=dev, dtype=torch.int64) if sums is None else _check("sums", sums, torch.int64, (nleaves, 3))
    if not leaf.is_contiguous() or not sums.is_contiguous():
        raise ValueError("leaf and sums must be contiguous")
    head = (_lib.ptr(X), n, X.shape[1], _lib.ptr(feature), _lib.ptr(threshold), _lib.ptr(left), _lib.ptr(right))
    tail = (nodes, _lib.ptr(qg), _lib.ptr(qh), nleaves, _lib.ptr(leaf), _lib.ptr(sums), _lib.current_stream(dev))
    with torch.cuda.device(dev):
        if kind == "":
            _lib.call("ptr_gbdt_leaf_sums", *head, *tail)
        elif kind == "_missing":
            _lib.call("ptr_gbdt_leaf_sums_missing", *head, _lib.ptr(default_left), *tail)
        else:
            _lib.call("ptr_gbdt_leaf_sums_cat", *head, _lib.ptr(default_left), _lib.ptr(is_cat), _lib.ptr(cat_index), _lib.ptr(cat_sets),
                      cat_sets.shape[0], *tail)
    return leaf, sums


def gbdt_add_by_leaf(scores, leaf, values):
    """scores[r] += values[leaf[r]] in place where 0 <= leaf[r] < leaves; other rows are skipped.  scores float32 [n], leaf int32 [n], values
    float32 [leaves] (ptr_gbdt_add_by_leaf)."""
    scores = _check("scores", scores)
    if scores.dim() != 1 or not scores.is_contiguous():
        raise ValueError("scores must be flat and contiguous")
    leaf = _check("leaf", leaf, torch.int32, (scores.numel(),))
    values = _check("values", values)
    if values.dim() != 1:
        raise ValueError(f"values must be flat, got {tuple(values.shape)}")
    with torch.cuda.device(scores.device):
        _lib.call("ptr_gbdt_add_by_leaf", _lib.ptr(scores), scores.numel(), _lib.ptr(leaf), _lib.ptr(values), values.numel(), _lib.current_stream(scores.device))
    return scores
