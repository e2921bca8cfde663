"""The adversarial frame (the reference's ltr_adversarial) on the fused HIP path: the IRGAN point and pair machines.

  IRGAN_Point   ptranking/ltr_adversarial/pointwise/irgan_point.py:48-232
  IRGAN_Pair    ptranking/ltr_adversarial/pairwise/irgan_pair.py:50-234

Jun Wang, Lantao Yu, Weinan Zhang, Yu Gong, Yinghui Xu, Benyou Wang, Peng Zhang, Dell Zhang: IRGAN — A Minimax Game for Unifying Generative
and Discriminative Information Retrieval Models, SIGIR 2017.

A machine holds two players, both point scorers on the fused kernels (AdversarialPlayer: the reference's ad_player.py, weight_decay 1e-3),
and keeps the reference's method names: fill_global_buffer, mini_max_train, generate_data, train_discriminator, train_generator, reset_* and
get_*.  They work on batching.PaddedQueryBatches: where the reference walks one query per step through torch.multinomial, torch.randperm,
fancy indexing and autograd, a padded batch takes one sampling launch (ptr_irgan_sample), one scorer pass and one fused loss launch
(ptr_irgan_sel_fwd_bwd, ptr_irgan_point_gen_fwd_bwd).

What differs from the reference, on purpose:
  * ONE optimiser step per BATCH on the sum over its queries of the reference's one-query loss, where the reference steps once per query
    (as WassRank and the diversification rankers do here: a batch of one query reproduces the reference's step).
  * The discriminator of IRGAN_Pair scores the positives and the negatives of a query in one compact batch [B, 2 S, F] with lens = 2 nsel;
    the reference scores them in two calls, which only differs under batch normalisation (its statistics see both halves here).
  * The draws come from a counter-based stream keyed by (seed, epoch counter, q0 + q), q0 the global index of a batch's first query — not
    from torch's generator: the same law (tests/test_irgan_gpu.py), another stream, and a shard of a batch draws what the whole batch would.
  * Sampling without replacement orders Gumbel keys instead of calling torch.multinomial: no weight can underflow.
  * NaN scores.  IRGAN_Point: a NaN generator score makes that batch's loss NaN and train_generator returns stop_training = True, as the
    reference's check on the predictions does (irgan_point.py:191-195).  The flag is read once per epoch, not per batch, so no step waits
    for the host; the price is that the optimiser has already stepped on the NaN batch (and on the batches after it) when the flag is
    read: the generator's weights are NaN from then on, where the reference returns before the step and keeps them.  Training stops
    either way; a caller that wants the last finite generator keeps a copy per epoch.  IRGAN_Pair: the reference's pair machine has no
    NaN stop (irgan_pair.py:94-118 ignores train_generator's result), and there is none here: ptr_irgan_sample gives a list with a NaN
    score nsel = 0, so such a query adds loss 0 and gradient 0, and a generator whose scores are all NaN trains nothing without a word.

  IRFGAN_Point  ptranking/ltr_adversarial/pointwise/irfgan_point.py:17-235
  IRFGAN_Pair   ptranking/ltr_adversarial/pairwise/irfgan_pair.py:19-185

Sebastian Nowozin, Botond Cseke, Ryota Tomioka: f-GAN — Training Generative Neural Samplers using Variational Divergence Minimization,
NIPS 2016; the reference's IRFGAN machines put IRGAN's players under its f-divergences.

The IRFGAN machines (EXTRA_AD_RANKER_NAMES) share the players, the buffer, the counter-based draws and the compact batch with the above and
train by train_discriminator_generator_single_step alone: per batch the generator's scores, one sampling launch (ptr_irfgan_point_sample,
ptr_irfgan_pair_sample), one compact batch ([B, 2 S, F] | [B, 4 S, F]), the discriminator's step, its eval-mode scores of the fakes, the
generator's step (ptr_irfgan_fwd_bwd).  What differs from the reference, beyond the list above:
  * conjugate_f(activation_f(v)) is evaluated in closed form: the reference's literal fp32 composition is inf or NaN from |v| of 9 to 17 on
    under RKL, NC, SH, JS and GAN, where the closed forms stay finite.
  * IRFGAN_Pair's fake pairs need no n x n matrix: the Bernoulli mask is recomputed from the counter hash, counted, and never stored.
  * 'JSW' and IRFGAN_Point.mini_max_train(single_step=False) raise NotImplementedError: neither runs in the reference.
  * NaN scores.  A list with a NaN generator score gets nsel = 0 from the samplers: it adds loss 0 and gradient 0 to both players.  The
    flag is accumulated on the device and read once per pass, so the pass trains on the remaining lists and batches before it returns
    stop_training = True, where the reference returns at the first such query (irfgan_point.py:188-190, irfgan_pair.py:120-123); once the
    generator's weights are NaN every list is skipped.  Training stops either way.

  IRGAN_List    ptranking/ltr_adversarial/listwise/irgan_list.py:24-409
  IRFGAN_List   ptranking/ltr_adversarial/listwise/irfgan_list.py:20-393

The list machines (LIST_AD_RANKER_NAMES, install_adversarial_list) play on whole rankings: the discriminator tells standard rankings (by
label, ties shuffled) from the generator's Gumbel-softmax rankings through a Plackett-Luce or Bradley-Terry ranking probability of its own
scores (PL_D), and the generator follows the Plackett-Luce log-probability of its top_k largest stochastic probabilities, weighted by a
reward from the discriminator (repTrick, dropLog; the conjugate of the f-divergence under IRFGAN_List).  Per batch and epoch: the
generator's eval-mode scores, one sampling launch (ptr_adlist_sample), the discriminator's train-mode scores of the padded batch, one loss
launch (ptr_adlist_fwd_bwd, mode D), one step; then the discriminator's eval-mode scores, the generator's train-mode scores, one fused
launch that draws, sorts and differentiates (mode G), one step.  The 'DG' / 'GD' order and the refresh of the rankings when
d_epoch % g_mod == 0 (g_mod = 2 if d_epoches > 1 else 1) are the reference's.  What differs from the reference, on purpose:
  * ONE optimiser step per batch on the sum of the one-query losses; a batch of one query is the reference's step.
  * The discriminator scores each document of a list ONCE and the kernel gathers by index, where the reference scores the gathered
    [S, K, F] copies.  The two agree for point scorers without batch normalisation and dropout; with them, the statistics and the masks
    see each document once here.
  * Rankings are ordered by the logit x + gumbel, not by the fp32 softmax of it: the same order wherever the probabilities differ, and
    a defined one where they underflow to equal zeros.
  * The draws come from the counter stream (seed, epoch counter, q0 + q), not from torch's generator; the label ties are shuffled by
    uniform keys of that stream, the law of arg_shuffle_ties' torch.randperm.
  * Refused with an error: optimal_train=True (NotImplementedError; the reference's driver never sets it, so burn_in is the no-op it is
    there), list-wise scorers (sf_id 'listsf'), mini_max_train(per_query_ad_training=False) (NotImplementedError there too).
  * IRFGAN_List.pre_check runs once top_k is set: the reference calls it a few lines earlier and would raise AttributeError under
    mask_label.
Out of scope: the semi-supervised (-1 label) route of IRFGAN_Pair, the Gaussian pair sampler, AdLTREvaluator's file handling and grid search.
"""
import copy

import torch

from . import functional as F_
from .batching import unpack_batch
from .host import LABEL_TYPE, DeviceEvaluator, PointScorerRanker, scorer_lens
from .rankers import FusedStepMixin
from .scorer import FusedScorerMixin

AD_RANKER_NAMES = ("IRGAN_Point", "IRGAN_Pair")
EXTRA_AD_RANKER_NAMES = ("IRFGAN_Point", "IRFGAN_Pair")       # install_adversarial(extras=True)
LIST_AD_RANKER_NAMES = ("IRGAN_List", "IRFGAN_List")          # install_adversarial_list()
LAMBDA = 0.5                 # irgan_point.py:16
DRAWS_PER_POS = 5            # irgan_point.py:203
DEFAULT_AD_PARAS = {         # irgan_point.py:243-253, irgan_pair.py:244-257
    "IRGAN_Point": dict(model_id="IRGAN_Point", ad_training_order="DG", d_epoches=1, g_epoches=1, temperature=0.5, samples_per_query=5),
    "IRGAN_Pair": dict(model_id="IRGAN_Pair", loss_type="svm", ad_training_order="DG", d_epoches=1, g_epoches=1, temperature=0.5,
                       samples_per_query=5),
    # irfgan_point.py:246-258, irfgan_pair.py:196-208 (the machines read f_div_id and samples_per_query alone)
    "IRFGAN_Point": dict(model_id="IRFGAN_Point", samples_per_query=5, d_epoches=1, g_epoches=1, f_div_id="KL", ad_training_order="DG"),
    "IRFGAN_Pair": dict(model_id="IRFGAN_Pair", d_epoches=1, g_epoches=1, f_div_id="KL", ad_training_order="DG", samples_per_query=5),
    # irgan_list.py:420-433, irfgan_list.py:405-420
    "IRGAN_List": dict(model_id="IRGAN_List", d_epoches=1, g_epoches=1, temperature=0.2, ad_training_order="DG", samples_per_query=10, top_k=2,
                       PL_D=True, repTrick=False, dropLog=True),
    "IRFGAN_List": dict(model_id="IRFGAN_List", d_epoches=1, g_epoches=1, f_div_id="KL", temperature=0.2, ad_training_order="GD",
                        samples_per_query=10, top_k=10, PL_D=True, repTrick=True, dropLog=True),
}


class AdversarialPlayer(FusedStepMixin, FusedScorerMixin, DeviceEvaluator, PointScorerRanker):
    """ptranking/ltr_adversarial/base/ad_player.py: a point-scorer ranker with weight_decay 1e-3; ndcg_at_k(s) and the other metric methods run
    on DeviceEvaluator.  `predict` returns the raw scores: the machines hand the temperature to the kernels."""

    def __init__(self, id=None, sf_para_dict=None, weight_decay=1e-3, gpu=False, device=None):
        PointScorerRanker.__init__(self, id=id, sf_para_dict=sf_para_dict, weight_decay=weight_decay, gpu=gpu, device=device)

    def score(self, X, lens):
        """The scores [B, L] of a padded batch; padded rows stay out of the batch-norm statistics."""
        with scorer_lens(self, lens, X):
            return self.forward(X)


def batch_key(batch):
    """What the global buffer and the generated data are keyed by: a PaddedQueryBatches batch is a fixed view of its bucket's tensor, so
    its address and shape name it for as long as the tensor lives.  The global buffer keeps the tensor itself beside its entry
    (fill_global_buffer), so no address it holds can be handed to another dataset's batch while the buffer is in use."""
    X = batch[1]
    return (X.data_ptr(), tuple(X.shape))


def buffered(global_buffer, batch):
    """(num_pos, q0) of a batch from the global buffer; a batch the buffer was not filled from is a KeyError."""
    num_pos, q0, _ = global_buffer[batch_key(batch)]
    return num_pos, q0


class _IRGANMachine:
    """What the two machines share: the buffer of positives, the mini-max schedule, the compact batch of selected documents."""

    sample_mode = None

    def __init__(self, eval_dict, data_dict, gpu=False, device=None, seed=137):
        self.eval_dict, self.data_dict = eval_dict, data_dict
        self.gpu, self.device = gpu, device
        self.seed, self._draws = int(seed), 0

    def _set_paras(self, ad_para_dict):
        self.d_epoches, self.g_epoches = ad_para_dict['d_epoches'], ad_para_dict['g_epoches']
        self.temperature = ad_para_dict['temperature']
        self.ad_training_order = ad_para_dict['ad_training_order']
        self.samples_per_query = ad_para_dict['samples_per_query']
        if self.ad_training_order not in ('DG', 'GD'):
            raise ValueError(f"ad_training_order {self.ad_training_order!r} ('DG', 'GD')")
        if not 1 <= int(self.samples_per_query) <= F_.IRGAN_MAX_SAMPLES:
            raise ValueError(f"samples_per_query must be in 1 .. {F_.IRGAN_MAX_SAMPLES}, got {self.samples_per_query}")

    def _next_seed(self):
        """(seed, epoch counter): every pass over the data draws from a stream of its own."""
        self._draws += 1
        return (self.seed << 24) + self._draws

    def fill_global_buffer(self, train_data, dict_buffer=None):
        """Per batch: the number of positive documents per query, counted on the device, and the global index of its first query.  Raises
        when a list is not presorted (a positive document behind a non-positive one): the samplers take the positives from the front.
        Nothing is written into dict_buffer before every list has passed that check.  An entry is (num_pos [B] int32, q0, X): the batch's
        tensor is kept so that its address, which is the key, stays its own."""
        assert self.data_dict['train_presort'] is True      # this is required for efficient truth exampling
        q0, unsorted, entries = 0, torch.zeros((), dtype=torch.bool, device=self.device), {}
        for batch in train_data:
            ids, X, Y, lens = unpack_batch(batch)
            key = batch_key(batch)
            if key not in dict_buffer:
                pos = Y > 0
                if lens is not None:
                    pos = pos & (torch.arange(Y.size(1), device=Y.device)[None, :] < lens[:, None])
                unsorted |= (pos[:, 1:] & ~pos[:, :-1]).any()
                entries[key] = (pos.sum(dim=1).to(torch.int32), q0, X)
            q0 += len(ids)
        if bool(unsorted):
            raise ValueError("a list has a relevant document behind a non-relevant one: IRGAN needs presorted training data (train_presort)")
        dict_buffer.update(entries)

    def mini_max_train(self, train_data=None, generator=None, discriminator=None, global_buffer=None):
        """irgan_point.py:87-113 / irgan_pair.py:94-118: 'DG' as the released code, 'GD' as Algorithm 1 of the paper; the generated data is
        refreshed at every 10th discriminator epoch."""
        def d_part():
            generated_data = None
            for d_epoch in range(self.d_epoches):
                if d_epoch % 10 == 0:
                    generated_data = self.generate_data(train_data=train_data, generator=generator, global_buffer=global_buffer)
                self.train_discriminator(train_data=train_data, generated_data=generated_data, discriminator=discriminator)
            return False

        def g_part():
            for g_epoch in range(self.g_epoches):
                if self.train_generator(train_data=train_data, generator=generator, discriminator=discriminator, global_buffer=global_buffer):
                    return True
            return False

        for part in ((d_part, g_part) if self.ad_training_order == 'DG' else (g_part, d_part)):
            if part():
                return True
        return False

    def generate_data(self, train_data=None, generator=None, global_buffer=None):
        """Sampling for training the discriminator: per batch (pos_idx [B, S], neg_idx [B, S], nsel [B]) from the generator's eval-mode scores."""
        generator.eval_mode()
        generated_data = dict()
        seed = self._next_seed()
        with torch.no_grad():
            for batch in train_data:
                ids, X, Y, lens = unpack_batch(batch)
                num_pos, q0 = buffered(global_buffer, batch)
                generated_data[batch_key(batch)] = F_.irgan_sample(generator.score(X, lens), num_pos, self.samples_per_query, self.sample_mode,
                                                                   temperature=self.temperature, seed=seed, q0=q0, lens=lens)
        return generated_data

    @staticmethod
    def selected_batch(X, pos_idx, neg_idx, nsel):
        """The compact padded batch of the selected documents: [B, 2 S, F] with the V positives of a query in rows 0 .. V-1, its V negatives
        in V .. 2V-1 and zero rows beyond, and lens = 2 nsel."""
        S = pos_idx.size(1)
        j = torch.arange(2 * S, device=X.device)[None, :]
        V = nsel.to(torch.int64)[:, None]
        src = torch.where(j < V, pos_idx.gather(1, j.clamp(max=S - 1).expand(X.size(0), -1)), neg_idx.gather(1, (j - V).clamp(0, S - 1)))
        Xs = X.gather(1, src[:, :, None].expand(-1, -1, X.size(2))) * (j < 2 * V)[:, :, None]
        return Xs, (2 * nsel).to(torch.int32)

    def train_discriminator(self, train_data=None, generated_data=None, discriminator=None, **kwargs):
        discriminator.train_mode()
        for batch in train_data:
            key = batch_key(batch)
            if key not in generated_data:
                continue
            ids, X, Y, lens = unpack_batch(batch)
            pos_idx, neg_idx, nsel = generated_data[key]
            Xs, lens_s = self.selected_batch(X, pos_idx, neg_idx, nsel)
            d_sel = discriminator.score(Xs, lens_s)
            discriminator._fused_step(F_.irgan_selected(d_sel, nsel, self.d_loss_mode))

    def reset_generator(self):
        self.generator.init()

    def reset_discriminator(self):
        self.discriminator.init()

    def reset_generator_discriminator(self):
        self.reset_generator()
        self.reset_discriminator()

    def get_generator(self):
        return self.generator

    def get_discriminator(self):
        return self.discriminator


class IRGAN_Point(_IRGANMachine):
    """IRGAN's pointwise machine.  The discriminator ends in a sigmoid (TL_AF 'S') and is trained by BCEWithLogits on its outputs, as the
    reference does; the generator's step draws 5 P documents per query from the importance distribution and weighs log p by the reward
    2 (D - 0.5) and p / q.  One optimiser step per batch on the sum over the queries of the reference's one-query loss."""

    sample_mode = "POINT_D"
    d_loss_mode = "POINT_D"

    def __init__(self, eval_dict, data_dict, sf_para_dict=None, ad_para_dict=None, gpu=False, device=None):
        super().__init__(eval_dict=eval_dict, data_dict=data_dict, gpu=gpu, device=device)
        assert sf_para_dict[sf_para_dict['sf_id']]['apply_tl_af'] == True   # noqa: E712  irgan_point.py:58
        g_sf_para_dict = sf_para_dict
        d_sf_para_dict = copy.deepcopy(g_sf_para_dict)
        d_sf_para_dict[sf_para_dict['sf_id']]['TL_AF'] = 'S'               # as required by the IRGAN model
        self.generator = AdversarialPlayer(id='IRGAN_Point_Generator', sf_para_dict=g_sf_para_dict, gpu=gpu, device=device)
        self.discriminator = AdversarialPlayer(id='IRGAN_Point_Discriminator', sf_para_dict=d_sf_para_dict, gpu=gpu, device=device)
        self._set_paras(ad_para_dict)

    def train_generator(self, train_data=None, generated_data=None, generator=None, discriminator=None, global_buffer=None):
        generator.train_mode()
        discriminator.eval_mode()
        bad = torch.zeros((), dtype=torch.bool, device=self.device)
        seed = self._next_seed()
        for batch in train_data:
            ids, X, Y, lens = unpack_batch(batch)
            num_pos, q0 = buffered(global_buffer, batch)
            with torch.no_grad():
                d_preds = discriminator.score(X, lens)
            loss = F_.irgan_point_generator(generator.score(X, lens), d_preds, num_pos, temperature=self.temperature, lam=LAMBDA,
                                            draws_per_pos=DRAWS_PER_POS, seed=seed, q0=q0, lens=lens)
            bad |= torch.isnan(loss.detach())
            generator._fused_step(loss)
        stop_training = bool(bad)
        if stop_training:
            print('Including NaN error.')
        return stop_training


class IRGAN_Pair(_IRGANMachine):
    """IRGAN's pairwise machine, loss_type 'svm' or 'log'.  The generator (apply_tl_af True) draws the negatives of its own step without
    replacement with weights sigmoid(scores / T); the reward comes from the discriminator (apply_tl_af False) on the pairs.  One optimiser
    step per batch on the sum over the queries of the reference's one-query loss."""

    sample_mode = "PAIR_D"

    def __init__(self, eval_dict, data_dict, sf_para_dict=None, ad_para_dict=None, gpu=False, device=None):
        super().__init__(eval_dict=eval_dict, data_dict=data_dict, gpu=gpu, device=device)
        self.loss_type = ad_para_dict['loss_type']
        if self.loss_type not in ('svm', 'log'):
            raise NotImplementedError(f"loss_type {self.loss_type!r} ('svm', 'log')")
        sf_para_dict[sf_para_dict['sf_id']]['apply_tl_af'] = True          # irgan_pair.py:62, the caller's dict as in the reference
        g_sf_para_dict = sf_para_dict
        d_sf_para_dict = copy.deepcopy(g_sf_para_dict)
        d_sf_para_dict[sf_para_dict['sf_id']]['apply_tl_af'] = False
        self.generator = AdversarialPlayer(id='IRGAN_Pair_Generator', sf_para_dict=g_sf_para_dict, gpu=gpu, device=device)
        self.discriminator = AdversarialPlayer(id='IRGAN_Pair_Discriminator', sf_para_dict=d_sf_para_dict, gpu=gpu, device=device)
        self._set_paras(ad_para_dict)
        self.d_loss_mode = "PAIR_D_SVM" if self.loss_type == 'svm' else "PAIR_D_LOG"
        self.g_loss_mode = "PAIR_G_SVM" if self.loss_type == 'svm' else "PAIR_G_LOG"

    def train_generator(self, train_data=None, generated_data=None, generator=None, discriminator=None, global_buffer=None):
        generator.train_mode()
        discriminator.eval_mode()
        bad = torch.zeros((), dtype=torch.bool, device=self.device)
        seed = self._next_seed()
        for batch in train_data:
            ids, X, Y, lens = unpack_batch(batch)
            num_pos, q0 = buffered(global_buffer, batch)
            g_preds = generator.score(X, lens)
            with torch.no_grad():
                pos_idx, neg_idx, nsel = F_.irgan_sample(g_preds, num_pos, self.samples_per_query, "PAIR_G", temperature=self.temperature, seed=seed,
                                                         q0=q0, lens=lens)
                d_sel = discriminator.score(*self.selected_batch(X, pos_idx, neg_idx, nsel))
            loss = F_.irgan_selected(g_preds, nsel, self.g_loss_mode, d_sel=d_sel, neg_idx=neg_idx, temperature=self.temperature, lens=lens)
            bad |= torch.isnan(loss.detach())
            generator._fused_step(loss)
        stop_training = bool(bad)
        if stop_training:
            print('Including NaN error.')
        return stop_training


class _IRFGANMachine(_IRGANMachine):
    """What IRFGAN_Point and IRFGAN_Pair share: the f-divergence, the single step of both players per batch, the compact batch."""

    model_id = None
    d_mode = g_mode = None
    parts = 2                                    # the compact batch is [B, parts * S, F]

    def _set_f_paras(self, ad_para_dict):
        self.f_div_id = ad_para_dict['f_div_id']
        self.samples_per_query = ad_para_dict['samples_per_query']
        F_._f_div(self.f_div_id)                 # 'JSW' NotImplementedError, an unknown name ValueError
        if not 1 <= int(self.samples_per_query) <= F_.IRGAN_MAX_SAMPLES:
            raise ValueError(f"samples_per_query must be in 1 .. {F_.IRGAN_MAX_SAMPLES}, got {self.samples_per_query}")

    def _players(self, sf_para_dict, d_sf_para_dict, gpu, device):
        self.generator = AdversarialPlayer(id=self.model_id + '_Generator', sf_para_dict=sf_para_dict, gpu=gpu, device=device)
        self.discriminator = AdversarialPlayer(id=self.model_id + '_Discriminator', sf_para_dict=d_sf_para_dict, gpu=gpu, device=device)

    @staticmethod
    def compact_batch(X, idx, nsel):
        """The compact padded batch of the selected documents: idx a list of K index tensors [B, S]; [B, K S, F] with part p of a query in
        rows p V .. (p + 1) V - 1 (V = nsel), zero rows beyond K V, and lens = K nsel."""
        K, S = len(idx), idx[0].size(1)
        j = torch.arange(K * S, device=X.device)[None, :]
        V = nsel.to(torch.int64)[:, None]
        part = torch.div(j, V.clamp(min=1), rounding_mode='floor').clamp(max=K - 1)
        src = torch.cat(idx, dim=1).gather(1, part * S + (j - part * V).clamp(0, S - 1))
        Xs = X.gather(1, src[:, :, None].expand(-1, -1, X.size(2))) * (j < K * V)[:, :, None]
        return Xs, (K * nsel).to(torch.int32)

    def _sample(self, g_preds, batch, seed, global_buffer):
        """-> (the index tensors of the compact batch, the generator loss's idx_a / idx_b, nsel)."""
        raise NotImplementedError

    def generate_data(self, **kwargs):
        """The epoch-wise pieces are reachable only from mini_max_train(single_step=False) of the reference's IRFGAN_Point, which cannot
        run there (see IRFGAN_Point.mini_max_train); IRFGAN_Pair has none."""
        raise NotImplementedError(f"{self.model_id} trains by train_discriminator_generator_single_step only")

    train_discriminator = train_generator = generate_data

    def train_discriminator_generator_single_step(self, train_data=None, generator=None, discriminator=None, global_buffer=None):
        """irfgan_point.py:170-223 / irfgan_pair.py:96-173 per batch: the generator's scores in train mode, one sampling launch, one compact
        batch, the discriminator's step on the summed per-query loss, its eval-mode scores of the fakes, the generator's step."""
        generator.train_mode()
        bad = torch.zeros((), dtype=torch.bool, device=self.device)
        seed = self._next_seed()
        K, fakes = self.parts, self.parts // 2
        for batch in train_data:
            ids, X, Y, lens = unpack_batch(batch)
            g_preds = generator.score(X, lens)
            bad |= torch.isnan(g_preds.detach()).any()
            with torch.no_grad():
                idx, idx_a, idx_b, nsel = self._sample(g_preds, batch, seed, global_buffer)
                Xs, lens_s = self.compact_batch(X, idx, nsel)
            discriminator.train_mode()
            discriminator._fused_step(F_.irfgan_loss(discriminator.score(Xs, lens_s), nsel, self.d_mode, self.f_div_id))
            discriminator.eval_mode()
            with torch.no_grad():
                S = idx_a.size(1)
                V = nsel.to(torch.int64)[:, None]
                cols = (fakes * V + torch.arange(fakes * S, device=X.device)[None, :]).clamp(max=K * S - 1)
                d_fake = discriminator.score(Xs, lens_s).gather(1, cols)     # the fake half, each part V wide
            generator._fused_step(F_.irfgan_loss(g_preds, nsel, self.g_mode, self.f_div_id, d_fake=d_fake, idx_a=idx_a, idx_b=idx_b, lens=lens))
        stop_training = bool(bad)
        if stop_training:
            print('Including NaN error.')
        return stop_training


class IRFGAN_Point(_IRFGANMachine):
    """IRFGAN's pointwise machine (irfgan_point.py:17-235): the discriminator separates relevant documents from the generator's draws under
    an f-divergence (ad_para_dict['f_div_id'], functional.F_DIVERGENCES), the generator follows -mean log p(fake) c(D(fake)).  One optimiser
    step per player per batch on the sum over the queries of the reference's one-query loss."""

    model_id, d_mode, g_mode, parts = "IRFGAN_Point", "POINT_D", "POINT_G", 2

    def __init__(self, eval_dict, data_dict, sf_para_dict=None, ad_para_dict=None, gpu=False, device=None):
        super().__init__(eval_dict=eval_dict, data_dict=data_dict, gpu=gpu, device=device)
        self._set_f_paras(ad_para_dict)
        self._players(sf_para_dict, copy.deepcopy(sf_para_dict), gpu, device)

    def mini_max_train(self, train_data=None, generator=None, discriminator=None, global_buffer=None, single_step=True):
        if not single_step:
            raise NotImplementedError("IRFGAN_Point.mini_max_train(single_step=False): the reference's branch reads self.d_epoches, "
                                      "self.g_epoches and self.ad_training_order, which its constructor never sets (irfgan_point.py:24-26, :57)")
        return self.train_discriminator_generator_single_step(train_data=train_data, generator=generator, discriminator=discriminator,
                                                              global_buffer=global_buffer)

    def _sample(self, g_preds, batch, seed, global_buffer):
        num_pos, q0 = buffered(global_buffer, batch)
        pos_idx, neg_idx, nsel = F_.irfgan_point_sample(g_preds, num_pos, self.samples_per_query, seed=seed, q0=q0, lens=unpack_batch(batch)[3])
        return [pos_idx, neg_idx], neg_idx, None, nsel


class IRFGAN_Pair(_IRFGANMachine):
    """IRFGAN's pairwise machine (irfgan_pair.py:19-185), g_key 'BT': true pairs are drawn by label difference with position discounts,
    fake pairs from a Bernoulli mask of Bradley-Terry probabilities sigmoid(s_i - s_j) of the generator's scores — both on the device,
    nothing of size n x n held; the discriminator (apply_tl_af False) scores head minus tail.  One optimiser step per player per batch."""

    model_id, d_mode, g_mode, parts = "IRFGAN_Pair", "PAIR_D", "PAIR_G", 4

    def __init__(self, eval_dict, data_dict, sf_para_dict=None, ad_para_dict=None, g_key='BT', sigma=1.0, gpu=False, device=None):
        super().__init__(eval_dict=eval_dict, data_dict=data_dict, gpu=gpu, device=device)
        self._set_f_paras(ad_para_dict)
        assert g_key == 'BT'                                                # irfgan_pair.py:30
        self.g_key, self.sigma = g_key, sigma                               # sigma: kept as the reference keeps it, unused under 'BT'
        d_sf_para_dict = copy.deepcopy(sf_para_dict)
        d_sf_para_dict[sf_para_dict['sf_id']]['apply_tl_af'] = False       # :42
        self._players(sf_para_dict, d_sf_para_dict, gpu, device)

    def fill_global_buffer(self, train_data, dict_buffer=None):
        """Per batch (num_pos [B] int32, q0, X, distinct [B] bool): the positives per query, the global index of the batch's first query, the
        batch's tensor (batch_key) and whether a list holds two distinct labels (irfgan_pair.py:81 num_unique_labels; the sampler makes
        the same check on the first and last label).  Raises ValueError on a label below 0 (the semi-supervised route is not built) and on a
        list that is not sorted by label, descending; nothing is written before every list has passed."""
        assert self.data_dict['train_presort'] is True      # this is required for efficient truth exampling
        q0, entries = 0, {}
        negative = torch.zeros((), dtype=torch.bool, device=self.device)
        unsorted = torch.zeros((), dtype=torch.bool, device=self.device)
        for batch in train_data:
            ids, X, Y, lens = unpack_batch(batch)
            key = batch_key(batch)
            if key not in dict_buffer:
                real = torch.ones_like(Y, dtype=torch.bool) if lens is None else torch.arange(Y.size(1), device=Y.device)[None, :] < lens[:, None]
                negative |= ((Y < 0) & real).any()
                unsorted |= ((Y[:, 1:] > Y[:, :-1]) & real[:, 1:]).any()
                n = real.sum(dim=1)
                first, last = Y[:, 0], Y.gather(1, (n - 1).clamp(min=0)[:, None])[:, 0]
                entries[key] = (((Y > 0) & real).sum(dim=1).to(torch.int32), q0, X, (n > 0) & (first != last))
            q0 += len(ids)
        if bool(negative):
            raise ValueError("a label below 0: IRFGAN_Pair's semi-supervised route (MSLETOR_SEMI) is not built")
        if bool(unsorted):
            raise ValueError("a list is not sorted by label, descending: IRFGAN_Pair needs presorted training data (train_presort)")
        dict_buffer.update(entries)

    def mini_max_train(self, train_data=None, generator=None, discriminator=None, global_buffer=None):
        return self.train_discriminator_generator_single_step(train_data=train_data, generator=generator, discriminator=discriminator,
                                                              global_buffer=global_buffer)

    def _sample(self, g_preds, batch, seed, global_buffer):
        ids, X, Y, lens = unpack_batch(batch)
        num_pos, q0 = global_buffer[batch_key(batch)][:2]
        th, tt, fh, ft, nsel = F_.irfgan_pair_sample(g_preds, Y, num_pos, self.samples_per_query, seed=seed, q0=q0, lens=lens)
        return [th, tt, fh, ft], fh, ft, nsel


class _ListMachine(_IRGANMachine):
    """What IRGAN_List and IRFGAN_List share: the players, the per-batch mini-max schedule, the sampling and the two fused losses."""

    model_id, family = None, None
    first_query = 0              # the global index of train_data's first query: a data-parallel shard sets it, so that it draws its rows

    def __init__(self, eval_dict, data_dict, sf_para_dict=None, ad_para_dict=None, optimal_train=False, gpu=False, device=None):
        super().__init__(eval_dict=eval_dict, data_dict=data_dict, gpu=gpu, device=device)
        if optimal_train:
            raise NotImplementedError(f"{self.model_id}(optimal_train=True): the supervised super-players are not built (the reference's driver "
                                      "never sets it)")
        if sf_para_dict['sf_id'] != 'pointsf':
            raise NotImplementedError(f"{self.model_id} plays with point scorers (sf_id 'pointsf'), got {sf_para_dict['sf_id']!r}")
        g_sf_para_dict = sf_para_dict
        d_sf_para_dict = copy.deepcopy(g_sf_para_dict)
        d_sf_para_dict[sf_para_dict['sf_id']]['apply_tl_af'] = True        # irgan_list.py:35-36, irfgan_list.py:31-32
        d_sf_para_dict[sf_para_dict['sf_id']]['TL_AF'] = 'S'
        self.generator = AdversarialPlayer(id=self.model_id + '_Generator', sf_para_dict=g_sf_para_dict, gpu=gpu, device=device)
        self.discriminator = AdversarialPlayer(id=self.model_id + '_Discriminator', sf_para_dict=d_sf_para_dict, gpu=gpu, device=device)
        self.top_k = ad_para_dict['top_k']
        self._set_paras(ad_para_dict)
        self.f_div_id = ad_para_dict.get('f_div_id', 'KL')
        F_._f_div(self.f_div_id)
        if self.top_k is not None and int(self.top_k) < 1:
            raise ValueError(f"top_k must be None (the whole list) or >= 1, got {self.top_k}")
        self.PL_discriminator = ad_para_dict['PL_D']
        self.replace_trick_4_generator = ad_para_dict['repTrick']
        self.drop_discriminator_log_4_reward = ad_para_dict['dropLog']
        self.optimal_train = optimal_train
        self.pre_check()

    def pre_check(self):
        if self.eval_dict is not None and self.eval_dict['mask_label']:
            # it is impossible to generate a standard ranking due to the existence of '-1'
            assert self.top_k is not None

    def burn_in(self, train_data=None):
        """irgan_list.py:64-97 trains the super-players under optimal_train, which is refused here: nothing to do, as in the reference."""

    def fill_global_buffer(self, train_data, dict_buffer=None):
        """For listwise, no particular global information is required (irgan_list.py:99-101)."""
        assert self.data_dict['train_presort'] is True

    @property
    def _loss_kw(self):
        return dict(prob="PL" if self.PL_discriminator else "BT", family=self.family, f_div=self.f_div_id, top_k=self.top_k,
                    reward=F_.adlist_reward(self.replace_trick_4_generator, self.drop_discriminator_log_4_reward))

    def per_query_generation(self, X=None, Y=None, lens=None, generator=None, seed=0, q0=0):
        """irgan_list.py:230-276 for a padded batch: (std_idx, gen_idx [B, S, Kw], kq [B]) from the generator's scores, one launch."""
        with torch.no_grad():
            return F_.adlist_sample(generator.score(X, lens), Y, self.samples_per_query, top_k=self.top_k, seed=seed, q0=q0, lens=lens)

    def train_discriminator(self, discriminator=None, X=None, lens=None, samples=None, **kwargs):
        std_idx, gen_idx, kq = samples
        loss = F_.adlist_loss(discriminator.score(X, lens), "D", std_idx=std_idx, gen_idx=gen_idx, kq=kq, lens=lens, **self._loss_kw)
        discriminator._fused_step(loss)
        return loss

    def train_generator(self, X=None, lens=None, generator=None, discriminator=None, seed=0, q0=0, **kwargs):
        with torch.no_grad():
            d_preds = discriminator.score(X, lens)
        loss = F_.adlist_loss(generator.score(X, lens), "G", d_preds=d_preds, samples_per_query=self.samples_per_query,
                              temperature=self.temperature, seed=seed, q0=q0, lens=lens, **self._loss_kw)
        generator._fused_step(loss)
        return loss

    def mini_max_train(self, train_data=None, generator=None, discriminator=None, global_buffer=None, per_query_ad_training=True):
        """irgan_list.py:103-227 per batch: 'DG' the discriminator's d_epoches steps (the rankings refreshed when d_epoch % g_mod == 0), then
        the generator's g_epoches steps; 'GD' the other way round.  Returns False, as the reference does."""
        if not per_query_ad_training:
            raise NotImplementedError
        g_mod = 2 if self.d_epoches > 1 else 1                              # regarding the generation
        q0 = int(self.first_query)
        for batch in train_data:
            ids, X, Y, lens = unpack_batch(batch)

            def d_part():
                discriminator.train_mode()
                generator.eval_mode()
                samples = None
                for d_epoch in range(self.d_epoches):
                    if d_epoch % g_mod == 0:                                # update generated data
                        samples = self.per_query_generation(X=X, Y=Y, lens=lens, generator=generator, seed=self._next_seed(), q0=q0)
                    self.train_discriminator(discriminator=discriminator, X=X, lens=lens, samples=samples)

            def g_part():
                generator.train_mode()
                discriminator.eval_mode()
                for _ in range(self.g_epoches):
                    self.train_generator(X=X, lens=lens, generator=generator, discriminator=discriminator, seed=self._next_seed(), q0=q0)

            for part in ((d_part, g_part) if self.ad_training_order == 'DG' else (g_part, d_part)):
                part()
            q0 += len(ids)
        stop_training = False
        return stop_training

    generate_data = None

    def get_generator(self, super=False):
        if super:
            raise NotImplementedError(f"{self.model_id}: the super-players exist under optimal_train only, which is not built")
        return self.generator

    def get_discriminator(self, super=False):
        if super:
            raise NotImplementedError(f"{self.model_id}: the super-players exist under optimal_train only, which is not built")
        return self.discriminator


class IRGAN_List(_ListMachine):
    """IRGAN's listwise machine (irgan_list.py:24-409).  ad_para_dict: top_k (None: the whole list), PL_D (the discriminator's ranking
    probability: Plackett-Luce, else Bradley-Terry), repTrick / dropLog (the generator's reward, get_reward), temperature (of the
    Gumbel-softmax), d_epoches, g_epoches, ad_training_order, samples_per_query."""

    model_id, family = "IRGAN_List", "IRGAN"


class IRFGAN_List(_ListMachine):
    """IRFGAN's listwise machine (irfgan_list.py:20-393): IRGAN_List with the discriminator's loss mean c(lp(gen)) - mean a(lp(std)) and the
    generator's reward c(lp) under ad_para_dict['f_div_id'] (functional.F_DIVERGENCES); repTrick and dropLog are read and, as in the
    reference (:295 overrides :283-292), without effect."""

    model_id, family = "IRFGAN_List", "IRFGAN"


def ndcg_at_5(player, data):
    """nDCG@5 of a player over presorted padded batches, as a float."""
    return float(player.ndcg_at_k(test_data=data, k=5, label_type=LABEL_TYPE.MultiLabel, presort=True))
