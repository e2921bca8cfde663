"""Search-result diversification (the reference's ltr_diversification frame) on the fused HIP path: DALETOR and the diversity metrics.

  DivQueryBatches   device-resident padded batches of diversification queries — the reference iterates ONE query per step and per
                    evaluation call (ptranking/base/ranker.py:636-669, :269-475) and moves every prediction to the CPU to sort it
  DALETOR           ptranking/ltr_diversification/score_and_sort/daletor.py:41-68 with the method names of
                    ptranking/ltr_diversification/base/diversity_ranker.py and ptranking/base/ranker.py:269-475, :636-695
  DivProbRanker     ptranking/ltr_diversification/score_and_sort/div_prob_ranker.py:234-359 on base/div_mdn_ranker.py:19-337: a mean and a
                    variance per document, four objectives built from the Gaussian pairwise comparison (ptr_divprob_fwd_bwd)

Called with the reference's one-query arguments a ranker behaves like the reference (B = 1); called with a DivQueryBatches it trains and
evaluates in padded batches: one fused loss launch (ptr_alphadcg_fwd_bwd / ptr_divprob_fwd_bwd) per batch, one metric launch
(ptr_div_metrics_at_ks) per batch, no `.cpu()` inside the loops.  Scorer: sf_id 'pointsf' (the point scorer on
[q_repr | q_repr * doc | doc], div_point_ranker.py:14-24).  The listwise scorers of div_list_ranker.py / div_mdn_ranker.py are out of scope
and refused.  Both rankers share one epoch loop and one set of evaluation methods (_DivRanker).
"""
import copy
import math

import numpy as np
import torch

from . import functional as F_
from .host import PointScorerRanker, scorer_lens
from .rankers import FusedStepMixin
from .scorer import FusedScorerMixin

DIV_RANKER_NAMES = ("DALETOR",)
EXTRA_DIV_RANKER_NAMES = ("DivProbRanker",)      # bound by install_diversification(extras=True) only
DEFAULT_DIV_PARAS = {"DALETOR": dict(model_id="DALETOR", rt=10.0, top_k=10),     # daletor.py:90
                     "DivProbRanker": dict(model_id="DivProbRanker", K=1, cluster=False, sort_id="ExpRele", top_k=None, opt_id="SuperSoft",
                                           limit_delta=0.01, metric="nERR-IA", opt_ideal=True, norm=True)}     # div_prob_ranker.py:387-389
SORT_ID = ("ExpRele", "RERAR", "RiskAware")      # div_mdn_ranker.py:17
SRD_METRIC = ("aNDCG", "nERR-IA")                # diversity_metric.py:8


def _np(a, dtype=np.float32):
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=dtype)


def unpack_div_query(item):
    """(qid, q_repr, perm_docs, doc_reprs, alphaDCG, q_doc_subtopics, q_doc_rele_mat) — what the reference's DIVDataset yields — or plain
    (q_repr, doc_reprs, q_doc_rele_mat) -> (qid, q_repr, doc_reprs, q_doc_rele_mat)."""
    if len(item) == 7:
        qid, q_repr, _, doc_reprs, _, _, rele = item
        return qid, q_repr, doc_reprs, rele
    if len(item) == 3:
        return None, item[0], item[1], item[2]
    raise ValueError(f"a diversification query is a 7-tuple or (q_repr, doc_reprs, q_doc_rele_mat), got {len(item)} fields")


class DivQueryBatches:
    """All queries of a split packed ONCE into padded device tensors, bucketed by list length like batching.PaddedQueryBatches.
    Iterating yields (ids, X [B, Lp, 3F], rele [B, Tp, Lp], lens int32 [B], ntopics int32 [B]):
      X      the point-scorer input [q_repr | q_repr * doc | doc] (div_point_ranker.py:14-24), zero rows beyond lens;
      rele   subtopic-by-document relevance, zero beyond lens / ntopics; Tp = the largest subtopic count of the bucket.
    Documents are kept in the given order: the reference's diversification data is presorted into its ideal order (`presort`)."""

    presort = True

    def __init__(self, queries, device, rough_batch_size=4096, pad_to=16, shuffle=False, seed=137):
        self.device = torch.device(device)
        self.shuffle, self._rng = shuffle, np.random.default_rng(seed)
        buckets = {}
        self.num_queries, self.num_features = 0, None
        for k, item in enumerate(queries):
            qid, q_repr, doc_reprs, rele = unpack_div_query(item)
            q, d, r = _np(q_repr).reshape(-1), _np(doc_reprs), _np(rele)
            n, F = d.shape
            if q.shape[0] != F or r.ndim != 2 or r.shape[1] != n:
                raise ValueError(f"query {qid}: q_repr {q.shape}, doc_reprs {d.shape} and q_doc_rele_mat {r.shape} do not fit together")
            if n == 0:
                continue
            if self.num_features is None:
                self.num_features = F
            x = np.concatenate([np.broadcast_to(q, (n, F)), q[None, :] * d, d], axis=1)
            Lp = int(math.ceil(n / pad_to) * pad_to)
            buckets.setdefault(Lp, []).append((k if qid is None else qid, x, r))
            self.num_queries += 1
        self._batches = []
        for Lp in sorted(buckets):
            items = buckets[Lp]
            nq, Tp = len(items), max(r.shape[0] for _, _, r in items)
            X = np.zeros((nq, Lp, 3 * self.num_features), np.float32)
            R = np.zeros((nq, Tp, Lp), np.float32)
            lens, nts, ids = np.empty(nq, np.int32), np.empty(nq, np.int32), []
            for i, (qid, x, r) in enumerate(items):
                n, T = x.shape[0], r.shape[0]
                X[i, :n], R[i, :T, :n], lens[i], nts[i] = x, r, n, T
                ids.append(qid)
            Xd, Rd = torch.from_numpy(X).to(self.device), torch.from_numpy(R).to(self.device)
            Ld, Td = torch.from_numpy(lens).to(self.device), torch.from_numpy(nts).to(self.device)
            per = max(1, rough_batch_size // Lp)
            for lo in range(0, nq, per):
                hi = min(nq, lo + per)
                self._batches.append((ids[lo:hi], Xd[lo:hi], Rd[lo:hi], Ld[lo:hi], Td[lo:hi]))

    def __len__(self):
        return len(self._batches)

    def __iter__(self):
        order = np.arange(len(self._batches))
        if self.shuffle:
            self._rng.shuffle(order)
        for i in order:
            yield self._batches[i]


class _DivRanker(FusedStepMixin, FusedScorerMixin, PointScorerRanker):
    """What the rankers of the diversification frame share: the point scorer on [q_repr | q_repr * doc | doc], the epoch loop
    (ranker.py:636-669) and the evaluation methods (ranker.py:269-475), per query as the reference runs them or over a DivQueryBatches.
    A subclass provides
      _batch_outputs(X, lens)        the scorer's outputs for a padded batch, as the tuple div_custom_loss_function takes before the relevance;
                                     the first one is what the stop check of ranker.py:666-667 looks at
      _batch_sort_scores(X, lens)    the scores [B, L] a padded batch is ranked by
    and the reference's div_forward / div_predict / div_train_op / div_custom_loss_function."""

    def _to_dev(self, t):
        return t.to(self.device, non_blocking=True) if torch.is_tensor(t) and t.device != torch.device(self.device) else t

    def _score_batch(self, X, lens):
        with scorer_lens(self, lens, X):
            return self.forward(X)

    # ---- training (ranker.py:636-669)
    def div_train(self, train_data, epoch_k=None):
        """One epoch.  A DivQueryBatches trains in padded batches (a query without a relevant document adds exactly 0 to the loss and to the
        gradient); anything else is iterated query by query as the reference does, minus its per-query `.item()`."""
        self.train_mode()
        epoch_loss = torch.zeros(1, device=self.device)
        stop_training = False
        if isinstance(train_data, DivQueryBatches):
            # the stop check of ranker.py:666-667 (all-zero or NaN predictions) stays on the device while the batches run — every batch takes
            # its step, as the reference's query does before it breaks (:669, :650) — and is read ONCE after the loop of a check epoch
            check = epoch_k is not None and epoch_k % self.stop_check_freq == 0
            bad = torch.zeros((), dtype=torch.bool, device=self.device)
            for ids, X, rele, lens, ntopics in train_data:
                outs = self._batch_outputs(X, lens)
                if check:
                    p = outs[0].detach()
                    bad |= ~(p != 0).any() | torch.isnan(p).any()
                epoch_loss += self.div_custom_loss_function(*outs, rele, presort=True, lens=lens, ntopics=ntopics).detach().reshape(-1)[:1]
            if check and bool(bad):
                print('All zero or NaN error.\n')
                stop_training = True
            return epoch_loss / max(1, train_data.num_queries), stop_training
        presort = train_data.presort
        for qid, q_repr, perm_docs, doc_reprs, alphaDCG, q_doc_subtopics, q_doc_rele_mat in train_data:
            if torch.sum(q_doc_rele_mat) < 1.0:
                continue      # skip instances that provide no training signal
            q_repr, doc_reprs, q_doc_rele_mat = self._to_dev(q_repr), self._to_dev(doc_reprs), self._to_dev(q_doc_rele_mat)
            batch_loss, stop_training = self.div_train_op(q_repr, doc_reprs, q_doc_rele_mat, qid=qid, alphaDCG=alphaDCG, epoch_k=epoch_k,
                                                          presort=presort)
            if stop_training:
                break
            epoch_loss += batch_loss.detach().reshape(-1)[:1]
        return epoch_loss / len(train_data), stop_training

    # ---- evaluation (ranker.py:269-475)
    def _div_eval(self, test_data, ks, max_label=None, min_len=None, per_q=None):
        """Sums of the three metrics over the queries the reference's loops keep (relevance sum >= 1; at least min_len documents for the
        single-cut-off methods) and their number, all on the device -> averages as CPU tensors [len(ks)]."""
        self.eval_mode()
        dev = torch.device(self.device)
        sums = [torch.zeros(len(ks), device=dev) for _ in range(3)]
        cnt = torch.zeros(1, device=dev)

        def add(preds, rele, lens, ntopics):
            out = F_.div_metrics_at_ks(preds.detach(), rele, ks, alpha=0.5, max_label=max_label, lens=lens, ntopics=ntopics)
            keep = out[3] > 0
            if min_len is not None:
                keep = keep & ((lens >= min_len) if lens is not None else torch.full_like(keep, preds.size(1) >= min_len))
            for s, m in zip(sums, out[:3]):
                if m is not None:
                    s += (m * keep.unsqueeze(1)).sum(dim=0)
            cnt.add_(keep.sum())
            if per_q is not None:
                per_q.append((out[0], keep))

        with torch.no_grad():
            if isinstance(test_data, DivQueryBatches):
                for ids, X, rele, lens, ntopics in test_data:
                    add(self._batch_sort_scores(X, lens), rele, lens, ntopics)
            else:
                assert test_data.presort is True
                for item in test_data:
                    _, q_repr, doc_reprs, rele = unpack_div_query(item)
                    q_repr, doc_reprs, rele = self._to_dev(q_repr), self._to_dev(doc_reprs), self._to_dev(rele)
                    add(self.div_predict(q_repr, doc_reprs), rele.float().unsqueeze(0).contiguous(), None, None)
        return [(s / cnt).cpu() for s in sums]      # no valid query at all: 0 / 0 = NaN, as the reference's sum / cnt (ranker.py:304)

    def alpha_ndcg_at_k(self, test_data=None, k=5, device='cpu'):
        return self._div_eval(test_data, [k], min_len=k)[0]

    def alpha_ndcg_at_ks(self, test_data=None, ks=[1, 5, 10], device='cpu'):
        return self._div_eval(test_data, ks)[0]

    def err_ia_at_k(self, test_data=None, k=5, max_label=None, device='cpu'):
        assert max_label is not None     # it is either query-level or corpus-level (diversity_metric.py:190)
        return self._div_eval(test_data, [k], max_label=max_label, min_len=k)[1]

    def nerr_ia_at_k(self, test_data=None, k=5, max_label=None, device='cpu'):
        assert max_label is not None
        return self._div_eval(test_data, [k], max_label=max_label, min_len=k)[2]

    def div_validation(self, vali_data=None, vali_metric=None, k=5, max_label=None, device='cpu'):
        if 'aNDCG' == vali_metric:
            return self.alpha_ndcg_at_k(test_data=vali_data, k=k, device=device)
        elif 'nERR-IA' == vali_metric:     # nERR-IA is better choice than ERR-IA with no normalization
            return self.nerr_ia_at_k(test_data=vali_data, k=k, max_label=max_label, device=device)
        else:
            raise NotImplementedError

    def srd_performance_at_ks(self, test_data=None, ks=[1, 5, 10], max_label=None, device='cpu', generate_div_run=False, dir=None,
                              fold_k=None, need_per_q_andcg=False):
        if generate_div_run:
            raise NotImplementedError("generate_div_run (the TREC run file for ndeval) is out of scope")
        assert max_label is not None
        per_q = [] if need_per_q_andcg else None
        andcg, err_ia, nerr_ia = self._div_eval(test_data, ks, max_label=max_label, per_q=per_q)
        if need_per_q_andcg:
            return andcg, err_ia, nerr_ia, [row.view(1, -1) for a, keep in per_q for row in a[keep].cpu()]
        return andcg, err_ia, nerr_ia

    def ndeval_performance_at_ks(self, test_data=None, ks=[5, 10, 20], alpha=0.5, beta=0.5, depth=None, need_per_q=False):
        """The figures TREC's ndeval reports for this ranker's run (ptranking/metric/srd/ndeval.c, which
        DivLTREvaluator.fold_evaluation_reproduce shells out to) without the run file: functional.ndeval_measures on the scores of every
        query, summed on the device and read once -> dict of CPU float64 tensors keyed by functional.NDEVAL_MEASURES ([len(ks)] or
        0-d).  The mean is ndeval's `amean`: over every query with at least one document, the nNRBP NaN of a query without a relevant
        document included.  The documents need not be presorted — ndeval builds its own ideal ranking.  With need_per_q also returns the
        per-query dicts (device tensors, "actual_subtopics" included), one per batch."""
        self.eval_mode()
        dev = torch.device(self.device)
        sums = {m: torch.zeros(len(ks) if m in ("ERR-IA", "nERR-IA", "alpha-DCG", "alpha-nDCG", "P-IA", "strec") else (), device=dev,
                               dtype=torch.float64) for m in F_.NDEVAL_MEASURES}
        cnt = torch.zeros((), device=dev, dtype=torch.float64)
        per_q = []

        def add(preds, rele, lens, ntopics):
            out = F_.ndeval_measures(preds.detach(), rele, ks, alpha=alpha, beta=beta, depth=depth, lens=lens, ntopics=ntopics)
            keep = (lens > 0) if lens is not None else torch.ones(preds.size(0), dtype=torch.bool, device=dev)
            for m in F_.NDEVAL_MEASURES:
                x = out[m]
                sums[m] += torch.where(keep if x.dim() == 1 else keep.unsqueeze(1), x, torch.zeros((), dtype=x.dtype, device=dev)).sum(dim=0)
            cnt.add_(keep.sum())
            if need_per_q:
                per_q.append(out)

        with torch.no_grad():
            if isinstance(test_data, DivQueryBatches):
                for ids, X, rele, lens, ntopics in test_data:
                    add(self._batch_sort_scores(X, lens), rele, lens, ntopics)
            else:
                for item in test_data:
                    _, q_repr, doc_reprs, rele = unpack_div_query(item)
                    q_repr, doc_reprs, rele = self._to_dev(q_repr), self._to_dev(doc_reprs), self._to_dev(rele)
                    add(self.div_predict(q_repr, doc_reprs), rele.float().unsqueeze(0).contiguous(), None, None)
        stacked = torch.cat([(sums[m] / cnt).reshape(-1) for m in F_.NDEVAL_MEASURES]).cpu()      # the one host read
        res, o = {}, 0
        for m in F_.NDEVAL_MEASURES:
            k = sums[m].numel()
            res[m] = stacked[o:o + k].reshape(sums[m].shape)
            o += k
        return (res, per_q) if need_per_q else res


class DALETOR(_DivRanker):
    """Le Yan, Zhen Qin, Rama Kumar Pasumarthi, Xuanhui Wang, Mike Bendersky: Diversification-Aware Learning to Rank using Distributed
    Representation, WWW 2021 — the reference's class (daletor.py:41-68) on the fused alpha-DCG loss kernel.

    top_k_axis: "reference" (default) keeps the reference's behaviour, whose top_k slices SUBTOPIC rows; "documents" is the alpha-DCG@k over
    the first top_k documents that its docstring describes.  alpha is 0.5, the value the reference hard-wires in the loss and in every metric."""

    alpha = 0.5
    top_k_axis = "reference"

    def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
        if sf_para_dict['sf_id'] == 'listsf':
            raise NotImplementedError("DALETOR with sf_id='listsf' (div_list_ranker.py: an encoder on 3F features and a second concatenation to "
                                      "6F) is out of scope; use sf_id='pointsf'")
        sf_para_dict = copy.deepcopy(sf_para_dict)      # the reference triples the caller's own dict in place (diversity_ranker.py:22)
        sf_para_dict['pointsf']['num_features'] *= 3    # q_repr + latent cross + doc_repr
        PointScorerRanker.__init__(self, id='DALETOR', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
        self.rt = model_para_dict['rt']
        self.top_k = model_para_dict['top_k']

    # ---- scoring (div_point_ranker.py:14-24)
    def div_forward(self, q_repr, doc_reprs):
        num_docs = doc_reprs.size(0)
        cat_reprs = torch.cat((q_repr.expand(num_docs, -1), q_repr * doc_reprs, doc_reprs), 1)
        return self.point_sf(cat_reprs.unsqueeze(0)).view(-1, num_docs)      # [1, num_docs]

    def div_predict(self, q_repr, doc_reprs):
        return self.div_forward(q_repr, doc_reprs)

    def _batch_outputs(self, X, lens):
        return (self._score_batch(X, lens),)

    def _batch_sort_scores(self, X, lens):
        return self._score_batch(X, lens)

    # ---- training (ranker.py:636-669, daletor.py:53-68)
    def div_custom_loss_function(self, batch_preds, q_doc_rele_mat, **kwargs):
        assert 'presort' in kwargs and kwargs['presort'] is True     # aiming for directly optimising alpha-nDCG over top-k documents
        rele = q_doc_rele_mat if q_doc_rele_mat.dim() == 3 else q_doc_rele_mat.unsqueeze(0)
        loss = F_.alphadcg_loss(batch_preds, rele.float(), rt=self.rt, alpha=self.alpha, top_k=self.top_k, top_k_axis=self.top_k_axis,
                                lens=kwargs.get('lens'), ntopics=kwargs.get('ntopics'))
        return self._fused_step(loss)

    def div_train_op(self, q_repr, doc_reprs, q_doc_rele_mat, **kwargs):
        stop_training = False
        batch_pred = self.div_forward(q_repr, doc_reprs)
        if 'epoch_k' in kwargs and kwargs['epoch_k'] % self.stop_check_freq == 0:
            stop_training = self.stop_training(batch_pred)
        return self.div_custom_loss_function(batch_pred, q_doc_rele_mat, **kwargs), stop_training


class DivProbRanker(_DivRanker):
    """The reference's DivProbRanker (ptranking/ltr_diversification/score_and_sort/div_prob_ranker.py:234-359 on
    ptranking/ltr_diversification/base/div_mdn_ranker.py:19-337): the scorer predicts a mean and a variance per document (for K > 1 a softmax
    mixture of K components), and the loss is one of four objectives built from the Gaussian pairwise comparison, all on ONE fused kernel
    (ptr_divprob_fwd_bwd): opt_id 'SuperSoft' with metric 'aNDCG' or 'nERR-IA', 'PairCLS', 'LambdaPairCLS'.

    Scorer: the point scorer with out_dim = 2 (K = 1) or 3 K on [q_repr | q_repr * doc | doc] — the column order of DivQueryBatches and
    DALETOR; the reference's own order is [q_repr | doc | q_repr * doc] (div_mdn_ranker.py:213-214), a fixed permutation of the input
    columns of a freshly initialised network.  sort_id: 'ExpRele' (the means), 'RiskAware' (mean - 0.1 variance), 'RERAR' (reciprocal
    expected ranks, ptr_divprob_expected_ranks).  Out of scope and refused: the listwise scorers (sf_id 'listsf...', with or without
    batch_cocos), cluster=True, opt_ideal=False, opt_id='Portfolio', generate_div_run.

    top_k_axis: as DALETOR's — "reference" keeps the reference's alpha_dcg_as_a_loss, whose top_k slices SUBTOPIC rows.  The pairwise
    objectives are the exact cross entropy, not the reference's `1 - erfc(x) / 2` arithmetic."""

    top_k_axis = "reference"

    def __init__(self, sf_para_dict=None, model_para_dict=None, gpu=False, device=None):
        sf_id = sf_para_dict['sf_id']
        if sf_id.startswith('listsf'):
            raise NotImplementedError(f"DivProbRanker with sf_id={sf_id!r} (the listwise MDN scorer of div_mdn_ranker.py:103-154, with or without "
                                      "batch_cocos) is out of scope; use sf_id='pointsf'")
        K, cluster = model_para_dict['K'], model_para_dict['cluster']
        assert K >= 1                                                            # div_mdn_ranker.py:39
        if cluster:
            raise NotImplementedError("DivProbRanker with cluster=True (a group of independent scorers, div_mdn_ranker.py:48-51) is out of scope")
        assert model_para_dict['sort_id'] in SORT_ID                             # :43
        self.opt_id = model_para_dict['opt_id']
        assert self.opt_id in ['PairCLS', 'LambdaPairCLS', 'SuperSoft', 'Portfolio']     # div_prob_ranker.py:248
        if self.opt_id == 'Portfolio':
            raise NotImplementedError("DivProbRanker with opt_id='Portfolio' (a cvxpy layer, div_prob_ranker.py:264-286) is out of scope")
        sf_para_dict = copy.deepcopy(sf_para_dict)      # the reference rewrites the caller's own dict in place (div_mdn_ranker.py:35, :53-56)
        sf_para_dict[sf_id]['num_features'] *= 3        # q_repr + latent cross + doc_repr
        sf_para_dict[sf_id]['out_dim'] = 2 if K == 1 else 3 * K      # mu and sigma / mixing coefficient, mu, sigma per component
        PointScorerRanker.__init__(self, id='DivProbRanker', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
        self.K, self.cluster, self.sort_id, self.limit_delta = K, cluster, model_para_dict['sort_id'], model_para_dict['limit_delta']
        self.b = 0.1                                    # :46
        self.beta = 0.5                                 # i.e., alpha in alpha-nDCG (div_prob_ranker.py:250)
        self.norm, self.top_k, self.metric, self.opt_ideal = False, None, None, True
        if 'LambdaPairCLS' == self.opt_id:
            self.opt_ideal, self.norm = model_para_dict['opt_ideal'], model_para_dict['norm']
        elif 'SuperSoft' == self.opt_id:
            self.opt_ideal, self.top_k, self.metric = model_para_dict['opt_ideal'], model_para_dict['top_k'], model_para_dict['metric']
            assert self.metric in SRD_METRIC
        if not self.opt_ideal:
            raise NotImplementedError("DivProbRanker with opt_ideal=False (a re-sort by expected rank, div_prob_ranker.py:55-61, :203-231) is "
                                      "out of scope")

    def uniform_eval_setting(self, **kwargs):
        eval_dict = kwargs['eval_dict']
        if 'SuperSoft' == self.opt_id and eval_dict["do_validation"] and not eval_dict['vali_metric'] == self.metric:
            eval_dict['vali_metric'] = self.metric

    # ---- scoring (div_mdn_ranker.py:248-326)
    def _head(self, batch_components):
        """[B, L, 2] or [B, L, 3 K] scorer outputs -> (means [B, L], variances [B, L]), div_mdn_ranker.py:276-294."""
        to_var = torch.exp if self.limit_delta is None else (lambda s: torch.sigmoid(s) * self.limit_delta)     # representing sigma^2
        if 1 == self.K:
            return batch_components[:, :, 0], to_var(batch_components[:, :, 1])
        batch_weights, batch_mu_i, batch_std_var_i = torch.split(batch_components, split_size_or_sections=self.K, dim=2)
        batch_coefficients = torch.softmax(batch_weights, dim=2)
        return torch.sum(batch_coefficients * batch_mu_i, dim=2), torch.sum(batch_coefficients * to_var(batch_std_var_i), dim=2)

    def _sort_scores(self, batch_mus, batch_vars, lens=None):
        if 'RERAR' == self.sort_id:       # reciprocal_expected_rank_as_relevance
            ranks = F_.expected_ranks(batch_mus.contiguous(), batch_vars.contiguous(), lens=lens)
            return torch.where(ranks > 0, 1.0 / ranks, torch.zeros_like(ranks))     # padded documents: 0
        elif 'ExpRele' == self.sort_id:
            return batch_mus
        elif 'RiskAware' == self.sort_id:
            return batch_mus - self.b * batch_vars
        raise NotImplementedError

    def div_forward(self, q_repr, doc_reprs):
        num_docs = doc_reprs.size(0)
        cat_reprs = torch.cat((q_repr.expand(num_docs, -1), q_repr * doc_reprs, doc_reprs), 1)
        return self._head(self.point_sf(cat_reprs.unsqueeze(0)).view(1, num_docs, -1))      # ([1, num_docs], [1, num_docs])

    def div_predict(self, q_repr, doc_reprs):
        batch_mus, batch_vars = self.div_forward(q_repr, doc_reprs)
        return self._sort_scores(batch_mus, batch_vars)

    def _batch_outputs(self, X, lens):
        with scorer_lens(self, lens, X):
            return self._head(self.point_sf(X).view(X.size(0), X.size(1), -1))       # host.py's forward views ONE output per document

    def _batch_sort_scores(self, X, lens):
        return self._sort_scores(*self._batch_outputs(X, lens), lens=lens)

    # ---- training (div_prob_ranker.py:295-359, div_mdn_ranker.py:329-337)
    def div_custom_loss_function(self, batch_mus, batch_vars, q_doc_rele_mat, **kwargs):
        assert 'presort' in kwargs and kwargs['presort'] is True     # aiming for directly optimising alpha-nDCG over top-k documents
        if kwargs.get('batch_cocos') is not None:
            raise NotImplementedError("batch_cocos (the correlation coefficients of the listwise scorer) is out of scope")
        rele = q_doc_rele_mat if q_doc_rele_mat.dim() == 3 else q_doc_rele_mat.unsqueeze(0)
        objective = self.metric if 'SuperSoft' == self.opt_id else self.opt_id
        loss = F_.divprob_loss(batch_mus, batch_vars, rele.float(), objective, beta=self.beta, top_k=self.top_k, top_k_axis=self.top_k_axis,
                               max_label=1.0, norm=self.norm, lens=kwargs.get('lens'), ntopics=kwargs.get('ntopics'))
        return self._fused_step(loss)

    def div_train_op(self, q_repr, doc_reprs, q_doc_rele_mat, **kwargs):
        stop_training = False
        batch_mus, batch_sigma_sqs = self.div_forward(q_repr, doc_reprs)
        return self.div_custom_loss_function(batch_mus, batch_sigma_sqs, q_doc_rele_mat, **kwargs), stop_training
