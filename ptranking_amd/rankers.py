"""The ltr_adhoc rankers of the hot path (the six losses of the north star + the sibling losses of SURVEY.md §8 f-4) as drop-in replacements for the reference classes of the same name.

Each class keeps the reference's constructor signature and `custom_loss_function` contract (consume `batch_preds`
attached to the scorer graph + `batch_std_labels`, do zero_grad -> backward -> optimizer.step itself, return the scalar
loss tensor; ptranking/base/ranker.py:605-613) but computes the loss and dLoss/dpreds with ONE fused HIP kernel.

`make_ranker_classes(base)` builds the classes on top of any base that provides the reference's AdhocNeuralRanker
interface: ptranking_amd.host.PointScorerRanker stand-alone, or the reference's own
ptranking.base.adhoc_ranker.AdhocNeuralRanker when `ptranking_amd.install()` drops them into
ptranking.ltr_adhoc.eval.ltr.
"""
import copy
import ctypes as C
import math
import os

import torch

from . import _lib
from . import dp
from . import functional as F_
from .host import DeviceEvaluator, DeviceTrainLoop, PointScorerRanker, is_multilabel
from .listsf import FusedListScorerMixin
from .scorer import (FLAT_OPTIMIZERS, FlatOptimizer, FusedPointScorer, FusedScorerMixin, alloc_acts, mlp_forward, opt_step_c_values, x6_wimg_for,
                     x6_image_tag, x6_set_image_tag)

RANKER_NAMES = ("RankNet", "LambdaRank", "LambdaLoss", "ApproxNDCG", "ListNet", "ListMLE", "STListNet", "RankCosine", "RankMSE", "SoftRank",
                "WassRank")
# SURVEY.md 2 marks these OUT OF SCOPE (the reference's driver cannot reach them): kept as classes for whoever asks for them by name
# (install(extras=True), pa.DASALC / pa.MDPRank), not part of the default drop-in surface
EXTRA_RANKER_NAMES = ("DASALC", "MDPRank")
# the smooth-rank metric objectives (ptranking/metric/smooth_metric/metric_as_opt_objective.py): the reference has no ranker class around
# them, so this one is opt-in by name (install(names=RANKER_NAMES + METRIC_RANKER_NAMES), pa.SmoothMetric)
METRIC_RANKER_NAMES = ("SmoothMetric",)
# the same objectives on Gaussian expected ranks (prob_utils.get_expected_rank): the scorer predicts a mean and a variance per document.  No
# reference class either: bound only by install(names=RANKER_NAMES + PROB_RANKER_NAMES), pa.ProbSmoothMetric
PROB_RANKER_NAMES = ("ProbSmoothMetric",)
PROB_SORT_IDS = ('ExpRele', 'RiskAware', 'RERAR')       # ptranking/ltr_diversification/base/div_mdn_ranker.py:43

# default hyper-parameters = the reference's `default_para_dict()`s
DEFAULT_PARAS = {
    "RankNet": dict(model_id="RankNet", sigma=1.0),                                    # pairwise/ranknet.py:57
    "LambdaRank": dict(model_id="LambdaRank", sigma=1.0),                              # listwise/lambdarank.py:78
    "LambdaLoss": dict(model_id="LambdaLoss", k=5, sigma=1.0, mu=5.0, loss_type="NDCG_Loss2"),   # listwise/lambdaloss.py:155-158
    "ApproxNDCG": dict(model_id="ApproxNDCG", alpha=10),                               # listwise/approxNDCG.py:131
    "ListNet": dict(model_id="ListNet"),
    "ListMLE": dict(model_id="ListMLE"),
    "STListNet": dict(model_id="STListNet", temperature=1.0),                          # listwise/st_listnet.py:70
    "RankCosine": dict(model_id="RankCosine"),
    "RankMSE": dict(model_id="RankMSE"),
    "SoftRank": dict(model_id="SoftRank", delta=2.0, metric='nDCG', top_k=None),       # listwise/softrank.py:97
    "DASALC": dict(model_id="DASALC"),
    "MDPRank": dict(model_id="MDPRank", temperature=1.0, gamma=1.0, top_k=10, distribution='PL'),   # listwise/mdprank.py:95-96
    "WassRank": dict(model_id="WassRank", mode='SinkhornOT', sh_itr=20, lam=0.1, smooth_type='ST', norm_type='BothST',   # listwise/wassrank/
                     cost_type='eg', non_rele_gap=100, var_penalty=math.e, gain_base=4),                                 # wassRank.py:97-104
    "SmoothMetric": dict(model_id="SmoothMetric", metric='nDCG', alpha=10, top_k=None, opt_ideal=True),   # alpha: listwise/approxNDCG.py:131
    "ProbSmoothMetric": dict(model_id="ProbSmoothMetric", metric='nDCG', top_k=None, opt_ideal=True, limit_delta=0.01, const_std=None,
                             sort_id='ExpRele'),        # limit_delta, sort_id: ltr_diversification/score_and_sort/div_prob_ranker.py:387-389
}


class FusedStepMixin:
    """zero_grad -> backward -> [one all_reduce(SUM) of the flat gradient under data parallelism] -> optimizer.step,
    the tail every reference loss ends with (e.g. lambdarank.py:58-60)."""

    data_parallel = True          # only takes effect when torch.distributed is initialised with world_size > 1
    _grad_bucket = None
    _dp_single = None

    # ---- direct train step: scorer forward -> fused loss kernel -> scorer backward -> [all-reduce] -> Adam as five C-ABI calls
    # One step of the autograd path costs ~0.37 ms of host time (autograd engine, tensor bookkeeping, optimizer hooks): at
    # <= 1024 queries per step that is more than the GPU needs.  When the scorer is the fused pointsf scorer, the optimiser is
    # FlatAdam and the ranker's loss is one of the single-kernel losses below, `DeviceTrainLoop.train_op` takes this path
    # instead: the SAME kernels with the SAME arguments in the SAME order (bit-identical parameters), no autograd graph.
    # A subclass that overrides custom_loss_function (the reference's plugin surface) is detected and keeps the autograd path.
    use_direct_step = True
    fuse_optimizer_step = True    # direct step on one device: optimiser step + loss-slot sum inside ptr_mlp_backward_step
    single_call_step = True       # r6: ... and the whole step as ONE C-ABI call (ptr_train_step: the same three entry points chained in C)
    reuse_weight_image = True     # r6: ... whose optimiser launch refreshes the bf16x6 forward's weight image, so the next step skips the prep launch
    _direct_loss = None           # the _lib.LOSSES entry of the loss — set by the loss mixins that qualify
    _direct_owner = None          # the class whose custom_loss_function the entry point implements

    def _direct_check(self, kwargs):
        """The reference's asserts of the loss (run on the direct path too)."""

    def _loss_values(self, kwargs):
        """The parameters of _direct_loss by name, as plain Python values."""
        return {}

    def _direct_train_op(self, X, Y, kwargs):
        spec = self._direct_loss
        sf = getattr(self, "point_sf", None)
        if (spec is None or not self.use_direct_step or not isinstance(sf, FusedPointScorer) or not isinstance(self.optimizer, FlatOptimizer)
                or type(self).custom_loss_function is not self._direct_owner.custom_loss_function or not sf.training
                or not torch.is_grad_enabled() or not (X.is_cuda and X.dim() == 3 and X.dtype == torch.float32 and X.is_contiguous())
                or not (Y.is_cuda and Y.dtype == torch.float32 and Y.is_contiguous() and Y.shape == X.shape[:2])
                or X.size(2) != sf.num_features or len(self.optimizer.param_groups) != 1):
            return None
        od = self.optimizer.__dict__       # an optimiser whose step / zero_grad were replaced on the instance (gradient accumulation hacks,
        if 'zero_grad' in od or ('step' in od and not getattr(od['step'], '_wrapped_by_lr_sched', False)):   # hooks) keeps its semantics:
            return None                    # autograd path (torch's lr schedulers wrap step() themselves — that wrapper is fine)
        self._direct_check(kwargs)
        lens = kwargs.get('lens')
        B, L, Fd = X.shape
        if L > _lib.MAX_LIST_LEN or (lens is not None and not (lens.is_cuda and lens.dtype == torch.int32 and lens.is_contiguous()
                                                               and lens.shape == (B,))):
            return None                    # the autograd path validates (functional._batch) and raises
        R, NL, dev = B * L, sf.num_layers, X.device
        cache = self.__dict__.setdefault("_direct_buffers", {})
        buf = cache.get((B, L))
        if buf is None:
            if len(cache) >= 4:                      # a few length buckets at most: do not pin scratch for every shape ever seen
                cache.pop(next(iter(cache)))
            ndz = _lib.query("ptr_mlp_backward_dz_floats", R, Fd, NL)
            buf = dict(preds=torch.empty((B, L), device=dev), acts=alloc_acts(R, NL, dev),
                       loss_q=torch.empty(max(B, 1), device=dev), dpreds=torch.empty((B, L), device=dev),
                       ws=torch.empty(_lib.query("ptr_mlp_backward_ws_floats", Fd, NL), device=dev),
                       dz=torch.empty(ndz, device=dev) if ndz else None)
            cache[(B, L)] = buf
        flat = sf.flat
        if flat.grad is None or flat.grad.shape != flat.shape or not flat.grad.is_contiguous():
            flat.grad = torch.empty_like(flat)
        p = sf.dropout
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0.0 else 0      # same CPU-generator draw as FusedPointScorer.forward
        if p > 0.0:
            seed = dp.local_dropout_seed(seed, R, local_queries=B)
        dp.end_step()                            # the recorded query slice described this batch only — with or without dropout (as _fused_step does)
        loss = torch.empty(1, device=dev)
        values = self._loss_values(kwargs)
        distributed = self.data_parallel and dp.is_distributed()
        # single device: the optimiser step and the loss-slot sum ride in the backward's partial reduction (three launches fewer per step,
        # bit-identical results); under data parallelism the all-reduce sits between the gradient and the step
        fuse_step = self.fuse_optimizer_step and not distributed and type(self.optimizer) in FLAT_OPTIMIZERS.values()
        if fuse_step and self.single_call_step:
            # r6: forward -> loss -> backward + step enqueued by ONE foreign call (ptr_train_step chains the very entry points used below:
            # bit-identical parameters); bench.py's per-stage timings (_lib.TIMING) come from events the call records between its stages
            return self._single_call_step(X, Y, lens, buf, flat, B, L, Fd, NL, R, p, seed, spec, values, kwargs, loss, dev)
        with torch.cuda.device(dev):
            st = _lib.current_stream(dev)
            mlp_forward(X, flat, R, Fd, NL, 1, p, seed, buf["preds"], buf["acts"], dev)
            stop_training = False
            if 'epoch_k' in kwargs and kwargs['epoch_k'] % self.stop_check_freq == 0:
                stop_training = self.stop_training(buf["preds"])
            # data parallel with a flat optimiser: backward -> flat gradient -> all-reduce -> ONE launch (optimiser step + loss-slot sum,
            # ptr_opt_step_loss): the single-device launch sequence + one kernel + one collective, nothing returns to autograd in between
            dp_fused = distributed and self.fuse_optimizer_step and type(self.optimizer) in FLAT_OPTIMIZERS.values()
            _lib.call(spec.entry, _lib.ptr(buf["preds"]), _lib.ptr(Y), _lib.ptr(lens), B, L, *spec.c_args(**values),
                      None if (fuse_step or dp_fused) else _lib.ptr(loss), _lib.ptr(buf["loss_q"]), _lib.ptr(buf["dpreds"]), st)
            if fuse_step:
                opt = opt_step_c_values(self.optimizer.fused_step_args(flat)).values()
                try:
                    _lib.call("ptr_mlp_backward_step", _lib.ptr(X), _lib.ptr(flat), _lib.ptr(buf["acts"]), _lib.ptr(buf["dpreds"]), R, Fd, NL, C.c_float(p),
                              C.c_uint64(seed), _lib.ptr(buf["dz"]), _lib.ptr(buf["ws"]), _lib.ptr(flat.grad), *opt, _lib.ptr(buf["loss_q"]), B, _lib.ptr(loss), st)
                except Exception:
                    self.optimizer.undo_step(flat)
                    raise
            else:
                _lib.call("ptr_mlp_backward", _lib.ptr(X), _lib.ptr(flat), _lib.ptr(buf["acts"]), _lib.ptr(buf["dpreds"]), R, Fd, NL, C.c_float(p),
                          C.c_uint64(seed), _lib.ptr(buf["dz"]), _lib.ptr(buf["ws"]), _lib.ptr(flat.grad), st)
                if distributed:
                    dp.all_reduce_sum(flat.grad)
                if dp_fused:
                    opt = opt_step_c_values(self.optimizer.fused_step_args(flat)).values()
                    try:
                        _lib.call("ptr_opt_step_loss", _lib.ptr(flat), _lib.ptr(flat.grad), C.c_int64(flat.numel()), *opt, _lib.ptr(buf["loss_q"]), B,
                                  _lib.ptr(loss), st)
                    except Exception:
                        self.optimizer.undo_step(flat)
                        raise
                else:
                    self.optimizer.step_flat(flat)
        return loss.reshape(()), stop_training

    def _single_call_step(self, X, Y, lens, buf, flat, B, L, Fd, NL, R, p, seed, spec, values, kwargs, loss, dev):
        d = buf.get("desc")
        if d is None:
            d = buf["desc"] = _lib.TrainStepDesc()
            d.struct_bytes = C.sizeof(_lib.TrainStepDesc)
            d.loss_kind = spec.kind
            d.B, d.L, d.F, d.NL = B, L, Fd, NL
            for k in ("preds", "acts", "loss_q", "dpreds", "dz", "ws"):
                setattr(d, k, None if buf[k] is None else buf[k].data_ptr())
        li, lf = spec.desc_arrays(**values)            # the loss parameters, as the separate entry point takes them
        d.loss_i[:len(li)], d.loss_f[:len(lf)] = li, lf
        wimg = x6_wimg_for(X, R, Fd, NL, True, dev)    # the forward mlp_forward would choose for this call
        d.wimg = None if wimg is None else wimg.data_ptr()
        d.X, d.labels, d.lens = X.data_ptr(), Y.data_ptr(), (None if lens is None else lens.data_ptr())
        # is the weight image still the one the previous step left for exactly these parameters?  (tag: scorer.x6_image_tag)
        st_ = self.optimizer.state.get(flat)
        step_before = int(st_["step"]) if st_ else 0
        d.wimg_current = int(wimg is not None and self.reuse_weight_image and os.environ.get("PTR_REUSE_IMG", "1") != "0" and
                             x6_image_tag(dev, Fd, NL) == (flat.data_ptr(), flat._version, step_before, wimg.data_ptr()))
        timing = _lib.TIMING
        evs = None
        if timing is not None:                         # bench.py: HIP events recorded by the call itself between its stages
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            for k, ev in enumerate(evs):
                ev.record()                            # creates the handle; ptr_train_step re-records it at its place in the stream
                d.events[k] = ev.cuda_event
        else:
            for k in range(4):
                d.events[k] = None
        opt = opt_step_c_values(self.optimizer.fused_step_args(flat))
        for name, v in opt.items():
            setattr(d, name, v)
        step = opt["step"]
        d.p_drop, d.seed = p, seed
        d.params, d.grad = flat.data_ptr(), flat.grad.data_ptr()
        d.loss_out = loss.data_ptr()
        if wimg is not None:
            x6_set_image_tag(dev, Fd, NL, None)        # until the call has gone through, nobody may trust the image
        try:
            with torch.cuda.device(dev):
                _lib.TIMING = None                     # (the call's own events time its stages; no bracket around the whole call)
                try:
                    _lib.call("ptr_train_step", C.addressof(d), _lib.current_stream(dev))
                finally:
                    _lib.TIMING = timing
        except Exception:
            self.optimizer.undo_step(flat)
            raise
        if wimg is not None:                           # the optimiser launch rewrote the image for the parameters it has just produced
            x6_set_image_tag(dev, Fd, NL, (flat.data_ptr(), flat._version, step, wimg.data_ptr()))
        if evs is not None:
            timing.setdefault("ptr_mlp_forward_x6" if wimg is not None else "ptr_mlp_forward", []).append((evs[0], evs[1]))
            timing.setdefault(spec.entry, []).append((evs[1], evs[2]))
            timing.setdefault("ptr_mlp_backward_step", []).append((evs[2], evs[3]))
        stop_training = False
        if 'epoch_k' in kwargs and kwargs['epoch_k'] % self.stop_check_freq == 0:
            stop_training = self.stop_training(buf["preds"])      # the scores of THIS step's forward (the reference checks them before the loss; it steps either way)
        return loss.reshape(()), stop_training

    def _bucket(self, extra=0):
        if self._grad_bucket is None or self._grad_bucket.extra != extra:
            if hasattr(self.optimizer, "grad_bucket"):
                # FlatViewAdam: the stack's gradients already live in ONE flat buffer that the optimiser steps on — a FlatGradBucket
                # would re-point every .grad away from it and Adam would step on zeros
                self._grad_bucket = self.optimizer.grad_bucket(extra)
            else:
                self._grad_bucket = dp.FlatGradBucket(list(self.get_parameters()), extra=extra)
        return self._grad_bucket

    def _fused_step(self, loss):
        if self.data_parallel and dp.is_distributed():
            if self._dp_single is None:
                ps = [p for p in self.get_parameters() if p.requires_grad]
                self._dp_single = ps[0] if len(ps) == 1 else False
            if self._dp_single is not False:
                # fused scorer: ONE flat parameter -> backward hands back one flat gradient, reduced in place
                # (no bucket memset, no accumulate-into-view copy)
                self.optimizer.zero_grad()
                loss.backward()
                if self._dp_single.grad is None:          # no gradient on this rank (e.g. an all-padding shard): every rank
                    self._dp_single.grad = torch.zeros_like(self._dp_single)   # must still join the collective
                stack = getattr(self.optimizer, "stack", None)
                if stack is not None:                     # flat-view optimiser: gradients that something re-pointed (module.zero_grad(),
                    stack.reattach_grads()                # a foreign bucket) must be back in the flat buffer BEFORE it is reduced
                dp.all_reduce_sum(self._dp_single.grad)
            else:
                bucket = self._bucket()
                bucket.zero()
                loss.backward()
                bucket.all_reduce()
        else:
            self.optimizer.zero_grad()
            loss.backward()
        self.optimizer.step()
        dp.end_step()                            # a query slice recorded by dp.shard_queries() described this step's batch only
        return loss

    def _batch_mean_step(self, loss, b_local):
        """The step of a loss that is a MEAN over the batch.  Under data parallelism the local gradient (scaled 1/B_local) is turned back
        into a sum, shipped with B_local in the same bucket, and divided by the global batch size after the single all-reduce."""
        if not (self.data_parallel and dp.is_distributed()):
            return self._fused_step(loss)
        b_local = float(b_local)
        bucket = self._bucket(extra=2)
        bucket.zero()
        loss.backward()
        bucket.flat[:bucket.numel].mul_(b_local)
        bucket.extras[0] = b_local
        bucket.extras[1] = loss.detach() * b_local
        bucket.all_reduce()
        b_global = bucket.extras[0].clone()
        bucket.flat[:bucket.numel].div_(b_global)
        self.optimizer.step()
        return bucket.extras[1] / b_global


class RankNetLoss(FusedStepMixin):
    _direct_loss = _lib.LOSSES["ranknet"]

    def _loss_values(self, kwargs):
        return dict(sigma=self.sigma)

    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/pairwise/ranknet.py:25-42"""
        return self._fused_step(F_.ranknet_loss(batch_preds, batch_std_labels, sigma=self.sigma, lens=kwargs.get('lens')))


class LambdaRankLoss(FusedStepMixin):
    _direct_loss = _lib.LOSSES["lambdarank"]

    def _loss_values(self, kwargs):
        return dict(sigma=self.sigma)

    def _direct_check(self, kwargs):
        assert 'label_type' in kwargs and is_multilabel(kwargs['label_type'])
        assert 'presort' in kwargs and kwargs['presort'] is True  # aiming for direct usage of ideal ranking

    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/listwise/lambdarank.py:27-62"""
        self._direct_check(kwargs)
        return self._fused_step(F_.lambdarank_loss(batch_preds, batch_std_labels, sigma=self.sigma, lens=kwargs.get('lens')))


class LambdaLossLoss(FusedStepMixin):
    _direct_loss = _lib.LOSSES["lambdaloss"]

    def _loss_values(self, kwargs):
        return dict(k=self.k, sigma=self.sigma, mu=getattr(self, 'mu', 5.0), loss_type=F_.LAMBDALOSS_TYPES[self.loss_type],
                    presort=bool('presort' in kwargs and kwargs['presort']))

    def _direct_check(self, kwargs):
        assert is_multilabel(kwargs['label_type'])
        if self.loss_type not in F_.LAMBDALOSS_TYPES:
            raise NotImplementedError(f"LambdaLoss type {self.loss_type!r} (supported: {sorted(F_.LAMBDALOSS_TYPES)})")

    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/listwise/lambdaloss.py:73-138"""
        self._direct_check(kwargs)
        presort = bool('presort' in kwargs and kwargs['presort'])
        loss = F_.lambdaloss_loss(batch_preds, batch_std_labels, k=self.k, sigma=self.sigma, mu=getattr(self, 'mu', 5.0),
                                  loss_type=self.loss_type, presort=presort, lens=kwargs.get('lens'))
        return self._fused_step(loss)


class ApproxNDCGLoss(FusedStepMixin):
    couple_batch = True   # the reference's [B]/[B,1] broadcast (SURVEY.md §7 vi); False = per-query normalisation

    def uniform_eval_setting(self, **kwargs):
        """ptranking/ltr_adhoc/listwise/approxNDCG.py:78-81"""
        eval_dict = kwargs['eval_dict']
        if eval_dict["do_validation"] and not eval_dict['vali_metric'] == 'nDCG':
            eval_dict['vali_metric'] = "nDCG"

    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/listwise/approxNDCG.py:83-109"""
        assert is_multilabel(kwargs['label_type'])
        presort = bool('presort' in kwargs and kwargs['presort'])
        if not (self.data_parallel and dp.is_distributed() and self.couple_batch):
            loss = F_.approxndcg_loss(batch_preds, batch_std_labels, alpha=self.alpha, presort=presort,
                                      couple_batch=self.couple_batch, lens=kwargs.get('lens'))
            return self._fused_step(loss)
        # Data parallel + batch coupling: the global loss is -(sum_all DCG)(sum_all 1/IDCG).  Every rank back-propagates
        # with scale 1, ships its local S = sum 1/IDCG and D = sum DCG in the gradient bucket, and rescales by the global S
        # after the single all-reduce (gradients are linear in S) — SURVEY.md §8e.
        loss1, parts = F_.approxndcg_loss(batch_preds, batch_std_labels, alpha=self.alpha, presort=presort,
                                          couple_batch=True, grad_scale_override=1.0, return_parts=True, lens=kwargs.get('lens'))
        bucket = self._bucket(extra=2)
        bucket.zero()
        loss1.backward()
        bucket.extras[0] = parts["scale"][1]
        bucket.extras[1] = -loss1.detach()            # = local sum of DCG (scale 1)
        bucket.all_reduce()
        S, D = bucket.extras[0].clone(), bucket.extras[1].clone()
        bucket.flat[:bucket.numel].mul_(S)
        self.optimizer.step()
        return -(D * S)


class SoftRankLoss(FusedStepMixin):
    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/listwise/softrank.py:33-78"""
        assert 'presort' in kwargs and kwargs['presort'] is True  # aiming for direct usage of ideal ranking
        assert 'nDCG' == self.metric
        assert is_multilabel(kwargs['label_type'])
        return self._fused_step(F_.softrank_loss(batch_preds, batch_std_labels, delta=self.delta_value, top_k=self.top_k,
                                                 lens=kwargs.get('lens')))


class SmoothMetricLoss(FusedStepMixin):
    max_label = None

    def uniform_eval_setting(self, **kwargs):
        """Validate on the metric that is optimised (the pattern of approxNDCG.py:78-81)."""
        eval_dict = kwargs['eval_dict']
        if eval_dict["do_validation"] and not eval_dict['vali_metric'] == self.metric:
            eval_dict['vali_metric'] = self.metric

    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/metric/smooth_metric/metric_as_opt_objective.py on get_approx_ranks (approxNDCG.py:19-27).  The reference's callers skip
        the step of a batch whose every query the top-k filter drops (zero_metric_value); here such a batch still steps, with a zero
        gradient: finding that out would cost a host sync per batch."""
        assert 'presort' in kwargs and kwargs['presort'] is True  # aiming for direct usage of ideal ranking
        assert 'label_type' in kwargs and is_multilabel(kwargs['label_type'])
        if self.metric == 'nERR' and self.max_label is None and self.data_parallel and dp.is_distributed():
            raise ValueError("SmoothMetric nERR under data parallelism needs model_para_dict['max_label']: the batch maximum is rank-local")
        return self._fused_step(F_.smooth_metric_objective(batch_preds, batch_std_labels, self.metric, alpha=self.alpha, top_k=self.top_k,
                                                           opt_ideal=self.opt_ideal, max_label=self.max_label, lens=kwargs.get('lens')))


class ProbSmoothMetricLoss(FusedStepMixin):
    """P / AP / nERR / nDCG on Gaussian expected ranks.  The scorer's outputs are [B, L, 2] (mean, raw variance) or, with const_std, [B, L]."""
    max_label = None
    const_std = None
    limit_delta = 0.01
    sort_id = 'ExpRele'
    risk_b = 0.1                                        # div_mdn_ranker.py:46

    def uniform_eval_setting(self, **kwargs):
        eval_dict = kwargs['eval_dict']
        if eval_dict["do_validation"] and not eval_dict['vali_metric'] == self.metric:
            eval_dict['vali_metric'] = self.metric

    def _head(self, batch_components):
        """Scorer outputs -> (means [B, L], variances [B, L] or None), the K = 1 head of div_mdn_ranker.py:276-294."""
        if self.const_std is not None:
            return batch_components, None
        to_var = torch.exp if self.limit_delta is None else (lambda s: torch.sigmoid(s) * self.limit_delta)     # representing sigma^2
        return batch_components[:, :, 0], to_var(batch_components[:, :, 1])

    def _sort_scores(self, batch_mus, batch_vars, lens=None):
        """The scores a list is ranked by, as diversity.DivProbRanker._sort_scores."""
        if 'ExpRele' == self.sort_id:
            return batch_mus
        if batch_vars is None:
            batch_vars = torch.full_like(batch_mus, float(self.const_std) ** 2)
        if 'RiskAware' == self.sort_id:
            return batch_mus - self.risk_b * batch_vars
        ranks = F_.expected_ranks(batch_mus.contiguous(), batch_vars.contiguous(), lens=lens)     # 'RERAR'
        return torch.where(ranks > 0, 1.0 / ranks, torch.zeros_like(ranks))     # padded documents: 0

    def forward(self, batch_q_doc_vectors):
        B, L = batch_q_doc_vectors.size(0), batch_q_doc_vectors.size(1)
        out = self.point_sf(batch_q_doc_vectors)
        return out.view(B, L) if self.const_std is not None else out.view(B, L, 2)

    def predict(self, batch_q_doc_vectors, lens=None):
        """The scores of sort_id; lens int32 [B]: the list lengths of a padded batch ('RERAR' ranks the valid documents only)."""
        if lens is None:
            lens = getattr(self, '_batch_lens', None)             # set by the evaluation loop around a padded batch
        return self._sort_scores(*self._head(self.forward(batch_q_doc_vectors)), lens=lens)

    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """metric_as_opt_objective.py on get_expected_rank / get_expected_rank_const (prob_utils.py:62-101); batch_preds are the scorer's
        outputs as forward() returns them.  A batch whose every query the top-k filter drops still steps, as SmoothMetric's does."""
        assert 'presort' in kwargs and kwargs['presort'] is True  # aiming for direct usage of ideal ranking
        assert 'label_type' in kwargs and is_multilabel(kwargs['label_type'])
        if self.metric == 'nERR' and self.max_label is None and self.data_parallel and dp.is_distributed():
            raise ValueError("ProbSmoothMetric nERR under data parallelism needs model_para_dict['max_label']: the batch maximum is rank-local")
        batch_mus, batch_vars = self._head(batch_preds)
        return self._fused_step(F_.gaussian_metric_objective(batch_mus, batch_vars, batch_std_labels, self.metric, top_k=self.top_k,
                                                             opt_ideal=self.opt_ideal, max_label=self.max_label, lens=kwargs.get('lens'),
                                                             const_std=self.const_std))


class MDPRankLoss(FusedStepMixin):
    # "torch" (default): the ranking is drawn with torch.multinomial / torch.rand + torch.sort as below; "device": sampling and loss in
    # one launch (functional.mdprank_sampled_loss), samples_per_query rankings per query, from a counter-based generator keyed by a per-call
    # seed and the query's global index.  Both read from model_para_dict ('sampler', 'samples_per_query').
    sampler = "torch"
    samples_per_query = 1
    _pl_seed = 137            # ptranking/ltr_global.py:7
    _pl_calls = 0

    def _query_offset(self, B, kwargs):
        """Global index of this batch's first query: kwargs['q0'] when the caller knows it; under data parallelism the rank's recorded
        slice (dp.shard_queries), else rank * local batch size, so that ranks draw disjoint streams."""
        if kwargs.get('q0') is not None:
            return int(kwargs['q0'])
        if not (self.data_parallel and dp.is_distributed()) or dp.world_size() == 1:
            return 0
        if dp.QUERY_SHARD is not None and dp.QUERY_SHARD[1] == B:
            return int(dp.QUERY_SHARD[0])
        return dp.rank() * B

    def _device_sampled_step(self, batch_preds, batch_std_labels, lens, kwargs):
        if self.distribution not in F_.PL_DISTRIBUTIONS:
            raise NotImplementedError
        self._pl_calls += 1
        loss = F_.mdprank_sampled_loss(batch_preds, batch_std_labels, top_k=self.top_k, gamma=self.gamma, temperature=self.temperature,
                                       distribution=self.distribution, samples=self.samples_per_query,
                                       seed=self._pl_seed * 0x9E3779B1 + self._pl_calls, q0=self._query_offset(batch_preds.size(0), kwargs),
                                       lens=lens)
        return self._fused_step(loss)

    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/listwise/mdprank.py:24-78.  The reference asserts batch size 1 ("aiming for meaningful
        batch-normalization"); every query is an independent episode here, so any batch size works and B = 1 reproduces it."""
        assert 'presort' in kwargs and kwargs['presort'] is True  # aiming for direct usage of ideal ranking
        lens = kwargs.get('lens')
        if self.sampler == 'device':
            return self._device_sampled_step(batch_preds, batch_std_labels, lens, kwargs)
        with torch.no_grad():
            det = batch_preds.detach()
            if lens is not None:      # padded documents must be sampled last: they get (numerically) zero probability mass
                pad = torch.arange(det.size(1), device=det.device)[None, :] >= lens[:, None].to(det.device)
                det = det.masked_fill(pad, -1e30)
            if 'PL' == self.distribution:           # sampling_utils.py:32-58 (torch.multinomial without replacement)
                t = det / self.temperature if 1.0 != self.temperature else det
                probs = torch.exp(t - torch.max(t, dim=1, keepdim=True)[0]).clamp_min(1e-38)
                perm = torch.multinomial(probs, num_samples=det.size(1), replacement=False)
                if lens is not None:  # real documents whose exp() underflowed to the same clamp as the padding may be drawn AFTER a
                    # padded one: stable-partition every sampled ranking so that all real documents come first
                    is_pad = (perm >= lens[:, None].to(perm.device)).to(torch.int8)
                    perm = torch.gather(perm, 1, torch.sort(is_pad, dim=1, stable=True)[1])
                noise = None
            elif 'STPL' == self.distribution:       # sampling_utils.py:61-83 (Gumbel perturbation, then sort)
                unif = torch.rand(det.size(), device=det.device)
                noise = -torch.log(-torch.log(unif + 1e-20) + 1e-20)
                logits = det + noise if 1.0 == self.temperature else (det + noise) / self.temperature
                perm = torch.sort(logits, dim=1, descending=True)[1]
            else:
                raise NotImplementedError
        if noise is None:
            action_preds = batch_preds                                   # gathered in sample order inside the kernel
        else:
            action_preds = batch_preds + noise if 1.0 == self.temperature else (batch_preds + noise) / self.temperature
        loss = F_.mdprank_loss(action_preds, batch_std_labels, perm, top_k=self.top_k, gamma=self.gamma, lens=lens)
        return self._fused_step(loss)


class ListNetLoss(FusedStepMixin):
    _direct_loss = _lib.LOSSES["listnet"]

    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/listwise/listnet.py:22-45"""
        return self._fused_step(F_.listnet_loss(batch_preds, batch_std_labels, lens=kwargs.get('lens')))


class STListNetLoss(FusedStepMixin):
    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/listwise/st_listnet.py:33-55"""
        unif = torch.rand(batch_preds.size(), device=batch_preds.device)  # [batch_size, ranking_size]
        return self._fused_step(F_.stlistnet_loss(batch_preds, batch_std_labels, temperature=self.temperature, unif=unif,
                                                  lens=kwargs.get('lens')))


class RankCosineLoss(FusedStepMixin):
    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/listwise/rank_cosine.py:24-38"""
        return self._fused_step(F_.rankcosine_loss(batch_preds, batch_std_labels, lens=kwargs.get('lens')))


class RankMSELoss(FusedStepMixin):
    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/pointwise/rank_mse.py:29-40.  The loss is a MEAN over the batch (not a sum over queries): under data
        parallelism it takes FusedStepMixin._batch_mean_step's route."""
        loss = F_.rankmse_loss(batch_preds, batch_std_labels, lens=kwargs.get('lens'))
        return self._batch_mean_step(loss, batch_preds.size(0))


class WassRankLoss(FusedStepMixin):
    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/listwise/wassrank/wassRank.py:43-88, mode 'SinkhornOT' (smooth_type 'ST', norm_type 'BothST').  batch_ids,
        lens and label_type are accepted, none is required, and nothing is printed (the reference prints batch_preds on every call).
        The reference squeezes the [B,L,L] cost to 2-D and so only runs at batch size 1; here every query is independent, and the loss
        is the MEAN over the batch, as the reference's .mean(0).sum() — under data parallelism the RankMSE route (_batch_mean_step).

        The predictions are scaled by the query's maximum label when self.TL_AF (= get_tl_af(), read at construction as the reference
        does) is 'S' or 'ST'.  On the reference's own base, AdhocNeuralRanker.get_tl_af() returns None (adhoc_ranker.py:83-87 has no
        `return`), so an installed WassRank never scales, exactly as the reference's driver does not; the stand-alone base returns TL_AF
        from sf_para_dict and does scale for TL_AF 'S'."""
        wd = self.wass_para_dict
        loss = F_.wassrank_loss(batch_preds, batch_std_labels, cost_type=wd['cost_type'], lam=wd['lam'], sh_itr=wd['sh_itr'],
                                gain_base=wd['gain_base'], non_rele_gap=wd['non_rele_gap'], var_penalty=wd['var_penalty'],
                                scale_by_max_label=self.TL_AF in ('S', 'ST'), lens=kwargs.get('lens'))
        return self._batch_mean_step(loss, batch_preds.size(0))


class ListMLELoss(FusedStepMixin):
    # "device" (default): one counter-based HIP kernel shuffles the ties of the whole batch; "torch": the reference's construction, one
    # torch.randperm per query from the global torch RNG (B host-driven calls per step).  Neither reproduces the reference's CPU
    # random stream on a GPU; both draw tie orders uniformly (tests/test_parity_gpu.py::test_tie_shuffle_is_uniform_enough).
    tie_shuffle = "device"
    _tie_seed = 137           # ptranking/ltr_global.py:7
    _tie_calls = 0

    def _shuffle_ties(self, batch_std_labels, lens=None):
        if self.tie_shuffle == "device" or lens is not None:     # padded batches: the device kernel honours `lens`
            self._tie_calls += 1
            return F_.shuffle_ties_order(batch_std_labels, seed=self._tie_seed * 0x9E3779B1 + self._tie_calls, lens=lens)
        # ptranking/ltr_adhoc/util/sampling_utils.py:13-28, batched: one randperm per query from the global torch RNG
        B, L = batch_std_labels.shape
        dev = batch_std_labels.device
        if B > 1:
            rperms = torch.stack([torch.randperm(L, device=dev) for _ in range(B)], dim=0)
        else:
            rperms = torch.randperm(L, device=dev).view(1, -1)
        shuffled = torch.gather(batch_std_labels, dim=1, index=rperms)
        desc = torch.argsort(shuffled, descending=True)
        return torch.gather(rperms, dim=1, index=desc)

    def custom_loss_function(self, batch_preds, batch_std_labels, **kwargs):
        """ptranking/ltr_adhoc/listwise/listmle.py:73-104"""
        lens = kwargs.get('lens')
        perm = self._shuffle_ties(batch_std_labels, lens)   # shuffle per epoch rather than using the same order for a query
        return self._fused_step(F_.listmle_loss(batch_preds, perm, lens=lens))


for _cls in (RankNetLoss, LambdaRankLoss, LambdaLossLoss, ListNetLoss):
    _cls._direct_owner = _cls


def make_ranker_classes(base=PointScorerRanker):
    """Return {name: class} built on `base` (anything with the reference's AdhocNeuralRanker interface)."""

    class RankNet(RankNetLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='RankNet', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
            self.sigma = model_para_dict['sigma']

    class LambdaRank(LambdaRankLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='LambdaRank', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
            self.sigma = model_para_dict['sigma']

    class LambdaLoss(LambdaLossLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='LambdaLoss', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
            self.lambdaloss_dict = model_para_dict
            self.k, self.sigma, self.loss_type = model_para_dict['k'], model_para_dict['sigma'], model_para_dict['loss_type']
            if 'NDCG_Loss2++' == self.loss_type:
                self.mu = model_para_dict['mu']
            if self.loss_type not in F_.LAMBDALOSS_TYPES:
                raise NotImplementedError(f"loss_type {self.loss_type!r}")

    class ApproxNDCG(ApproxNDCGLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='ApproxNDCG', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
            self.alpha = model_para_dict['alpha']

    class ListNet(ListNetLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        def __init__(self, sf_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='ListNet', sf_para_dict=sf_para_dict, gpu=gpu, device=device)

    class ListMLE(ListMLELoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='ListMLE', sf_para_dict=sf_para_dict, gpu=gpu, device=device)

    class STListNet(STListNetLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='STListNet', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
            self.temperature = model_para_dict['temperature']

    class RankCosine(RankCosineLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        def __init__(self, sf_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='RankCosine', sf_para_dict=sf_para_dict, gpu=gpu, device=device)

    class RankMSE(RankMSELoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        def __init__(self, sf_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='RankMSE', sf_para_dict=sf_para_dict, gpu=gpu, device=device)

    class SoftRank(SoftRankLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='SoftRank', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
            self.delta_value = float(model_para_dict['delta'])
            self.delta = torch.tensor([self.delta_value], device=self.device)     # softrank.py:28-29
            self.top_k = model_para_dict['top_k']
            self.metric = model_para_dict['metric']

    class DASALC(ListNetLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        """ptranking/ltr_adhoc/listwise/dasalc.py:7-41: the top-1 ListNet loss on the listwise (listsf) scorer."""

        def __init__(self, sf_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='DASALC', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
            assert 'listsf' == sf_para_dict['sf_id']

    class MDPRank(MDPRankLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='MDPRank', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
            self.gamma = model_para_dict['gamma']
            self.top_k = model_para_dict['top_k']
            self.temperature = model_para_dict['temperature']
            self.distribution = model_para_dict['distribution']  # 'PL', 'STPL'
            self.sampler = model_para_dict.get('sampler', 'torch')                    # 'torch' (the reference's construction) or 'device'
            self.samples_per_query = int(model_para_dict.get('samples_per_query', 1))
            if self.sampler not in ('torch', 'device'):
                raise ValueError(f"MDPRank sampler {self.sampler!r} (supported: 'torch', 'device')")
            if self.samples_per_query < 1 or (self.sampler == 'torch' and self.samples_per_query != 1):
                raise ValueError("MDPRank samples_per_query must be >= 1, and 1 with sampler='torch'")
            self.pg_checking = False

    class WassRank(WassRankLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        """ptranking/ltr_adhoc/listwise/wassrank/wassRank.py:22-41 with the reference's constructor (and the driver's calling convention,
        ltr.py:173-174).  dict_cost_mats / dict_std_dists are kept but never consulted: the ST target histogram is a pure function of the
        labels and the cost is recomputed inside the kernel, so the reference's per-qid caches change no value."""

        def __init__(self, sf_para_dict, wass_para_dict=None, dict_cost_mats=None, dict_std_dists=None, gpu=False, device=None):
            base.__init__(self, id='WassRank', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
            self.TL_AF = self.get_tl_af()
            self.wass_para_dict = dict(DEFAULT_PARAS['WassRank']) if wass_para_dict is None else wass_para_dict
            if dict_cost_mats is not None:
                self.dict_cost_mats = dict_cost_mats
            if dict_std_dists is not None:
                self.dict_std_dists = dict_std_dists
            wd = self.wass_para_dict
            if wd['mode'] != 'SinkhornOT':     # EntropicOT: autograd through every iteration + a batch-global early stop (host sync per iteration)
                raise NotImplementedError(f"WassRank mode {wd['mode']!r}: only mode='SinkhornOT' is served")
            if wd['smooth_type'] != 'ST':      # NG: zero mass on label-0 documents, log(0) — NaN in the reference at any precision
                raise NotImplementedError(f"WassRank smooth_type {wd['smooth_type']!r}: only smooth_type='ST' is served")
            if wd.get('norm_type', 'BothST') != 'BothST':
                raise NotImplementedError(f"WassRank norm_type {wd['norm_type']!r}: only norm_type='BothST' is served")
            if wd['cost_type'] not in F_.WASS_COST_TYPES:
                raise NotImplementedError(f"WassRank cost_type {wd['cost_type']!r} (supported: {sorted(F_.WASS_COST_TYPES)})")

    class SmoothMetric(SmoothMetricLoss, FusedScorerMixin, FusedListScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        """P / AP / nERR / nDCG on smooth ranks as the training objective; model_para_dict: metric, alpha, top_k, opt_ideal, optional max_label."""

        def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
            base.__init__(self, id='SmoothMetric', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
            self.metric = model_para_dict['metric']
            if self.metric not in ('P', 'AP', 'nERR', 'nDCG'):
                raise NotImplementedError(f"metric {self.metric!r} (supported: 'P', 'AP', 'nERR', 'nDCG')")
            self.alpha = model_para_dict['alpha']
            self.top_k = model_para_dict['top_k']
            self.opt_ideal = bool(model_para_dict['opt_ideal'])
            self.max_label = model_para_dict.get('max_label')

    class ProbSmoothMetric(ProbSmoothMetricLoss, FusedScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        """P / AP / nERR / nDCG on Gaussian expected ranks as the training objective: the point scorer predicts a mean and a variance per
        document (out_dim = 2; heads exp, or sigmoid * limit_delta), or a mean alone with model_para_dict['const_std'] (out_dim = 1, every
        document the same standard deviation: SoftRank's rank model).  model_para_dict: metric, top_k, opt_ideal, optional max_label,
        limit_delta, const_std, sort_id ('ExpRele', 'RiskAware', 'RERAR': the scores predict() returns)."""

        def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
            sf_id = sf_para_dict['sf_id']
            if sf_id != 'pointsf':
                raise NotImplementedError(f"ProbSmoothMetric with sf_id={sf_id!r}: the point scorer (sf_id='pointsf') only")
            self.metric = model_para_dict['metric']
            if self.metric not in ('P', 'AP', 'nERR', 'nDCG'):
                raise NotImplementedError(f"metric {self.metric!r} (supported: 'P', 'AP', 'nERR', 'nDCG')")
            self.sort_id = model_para_dict.get('sort_id', 'ExpRele')
            if self.sort_id not in PROB_SORT_IDS:
                raise ValueError(f"sort_id {self.sort_id!r} (supported: {PROB_SORT_IDS})")
            self.const_std = model_para_dict.get('const_std')
            if self.const_std is not None and not float(self.const_std) > 0.0:
                raise ValueError(f"const_std must be > 0 (got {self.const_std!r})")
            sf_para_dict = copy.deepcopy(sf_para_dict)                       # the caller's dict keeps its out_dim
            sf_para_dict[sf_id]['out_dim'] = 1 if self.const_std is not None else 2     # mean | mean and variance, div_mdn_ranker.py:53-56
            base.__init__(self, id='ProbSmoothMetric', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
            self.top_k = model_para_dict['top_k']
            self.opt_ideal = bool(model_para_dict['opt_ideal'])
            self.max_label = model_para_dict.get('max_label')
            self.limit_delta = model_para_dict.get('limit_delta', 0.01)

    out = dict(RankNet=RankNet, LambdaRank=LambdaRank, LambdaLoss=LambdaLoss, ApproxNDCG=ApproxNDCG, ListNet=ListNet,
               ListMLE=ListMLE, STListNet=STListNet, RankCosine=RankCosine, RankMSE=RankMSE, SoftRank=SoftRank, WassRank=WassRank,
               DASALC=DASALC, MDPRank=MDPRank, SmoothMetric=SmoothMetric, ProbSmoothMetric=ProbSmoothMetric)
    for name, cls in out.items():
        cls.__name__ = cls.__qualname__ = name
        cls.__module__ = __name__
    return out


_standalone = make_ranker_classes(PointScorerRanker)
RankNet, LambdaRank, LambdaLoss = _standalone["RankNet"], _standalone["LambdaRank"], _standalone["LambdaLoss"]
ApproxNDCG, ListNet, ListMLE = _standalone["ApproxNDCG"], _standalone["ListNet"], _standalone["ListMLE"]
STListNet, RankCosine, RankMSE = _standalone["STListNet"], _standalone["RankCosine"], _standalone["RankMSE"]
SoftRank, DASALC, MDPRank = _standalone["SoftRank"], _standalone["DASALC"], _standalone["MDPRank"]
WassRank = _standalone["WassRank"]
SmoothMetric = _standalone["SmoothMetric"]
ProbSmoothMetric = _standalone["ProbSmoothMetric"]
