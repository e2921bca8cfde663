/*
 * ptranking_amd — C ABI of the MI355X-native ltr_adhoc loss / metric hot path.
 *
 * This is the drop-in boundary.  The reference (wildltr/ptranking) is pure Python and has no
 * FFI of its own; each entry point below replaces the ATen op sequence that one reference function executes, and
 * is what a `ctypes` binding on the reference side would bind (INTEGRATION.md shows that stub).  The Python host
 * layer in ptranking_amd/ mirrors the reference's plugin surface (`NeuralRanker.custom_loss_function`,
 * `Evaluator.*`) on top of these calls.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into HBM unless it is marked "host"; the caller owns every buffer,
 *     nothing is allocated, freed or retained by the library; no state survives a call;
 *   - batches are padded row-major (B, L) fp32: `preds[q*L + i]`, `labels[q*L + i]`; `lens` (int32[B], nullable)
 *     gives the number of real documents per query (NULL => L for every query); padded documents are excluded
 *     from every sum and receive gradient 0;
 *   - calls only ENQUEUE work on `stream` (a hipStream_t passed as void*, NULL = the legacy default stream) and
 *     never synchronise the host; results are run-to-run bit-stable (no floating-point atomics across waves);
 *   - return value: 0 on success, a hipError_t (> 0, < 1000) if the HIP runtime failed, or one of PTR_ERR_*;
 *     ptr_last_error() returns a thread-local message for the last non-zero return on this thread;
 *   - list lengths up to PTR_MAX_LIST_LEN are supported (per-query tiles live in LDS).
 */
#ifndef PTRANKING_AMD_H
#define PTRANKING_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTR_ABI_VERSION 8
#define PTR_MAX_LIST_LEN 4096
#define PTR_MAX_CUTOFFS 32
#define PTR_MAX_SUBTOPICS 32
#define PTR_MLP_ACT_LD 112

#define PTR_ERR_INVALID_ARG 1001   /* NULL pointer, negative size, bad enum value               */
#define PTR_ERR_UNSUPPORTED 1002   /* L > PTR_MAX_LIST_LEN, nk > PTR_MAX_CUTOFFS, ...            */

#define PTR_LAMBDALOSS_NDCG_LOSS1 0    /* 'NDCG_Loss1'   (lambdaloss.py:33-34; the reference only runs it at batch size 1: its
                                         [B,L] weights broadcast against [B,L,L]; here every query uses its own w_j)  */
#define PTR_LAMBDALOSS_NDCG_LOSS2 1    /* 'NDCG_Loss2'   (ptranking/ltr_adhoc/listwise/lambdaloss.py:36-45) */
#define PTR_LAMBDALOSS_NDCG_LOSS2PP 2  /* 'NDCG_Loss2++' (ptranking/ltr_adhoc/listwise/lambdaloss.py:47-58) */

int ptr_abi_version(void);
const char *ptr_last_error(void);

/* RankNet — replaces ptranking/ltr_adhoc/pairwise/ranknet.py:32-36 (+ ltr_adhoc/util/lambda_utils.py:5-23) and
 * its autograd backward.  Pairs i<j in INPUT order, unweighted BCE, ties have target 0.5.
 *   loss_q[B] = per-query loss; grad[B,L]; loss_out[1] = sum over queries (nullable: NULL skips the reduction launch,
 *   the caller can run ptr_sum_f32 over loss_q itself).  Same convention for every *_fwd_bwd below. */
int ptr_ranknet_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, float sigma,
                        float *loss_out, float *loss_q, float *grad, void *stream);

/* LambdaRank — replaces ptranking/ltr_adhoc/listwise/lambdarank.py:39-56 (torch.sort, gather,
 * get_pairwise_comp_probs, get_delta_ndcg = ptranking/metric/metric_utils.py:19-45, weighted BCE over the upper
 * triangle) and its backward, fused into one kernel.  `labels` must be in ideal (descending) order per query, as
 * the reference asserts (lambdarank.py:36).  sigma must be >= 0.  Ties in `preds` are ranked by original index. */
int ptr_lambdarank_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, float sigma,
                           float *loss_out, float *loss_q, float *grad, void *stream);

/* LambdaLoss — replaces ptranking/ltr_adhoc/listwise/lambdaloss.py:83-132 and its backward.
 * loss_type: PTR_LAMBDALOSS_*; k = truncation (pairs with both ranks < k); mu only used by NDCG_Loss2++;
 * presort != 0 => labels already in ideal order (lambdaloss.py:83-84), else they are sorted first (:86-87).
 * A list with documents but no relevant one (IDCG = 0): NDCG_Loss1 gives a NaN loss and a NaN gradient on every document,
 * as the reference; NDCG_Loss2 / Loss2++ give loss 0 and gradient 0.  A zero-length list gives 0.  A list that holds a NaN score
 * or label gives a NaN loss and a NaN gradient on every document (the reference ranks a NaN score first and stays finite). */
int ptr_lambdaloss_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, int k,
                           float sigma, float mu, int loss_type, int presort, float *loss_out, float *loss_q,
                           float *grad, void *stream);

/* SoftRank — replaces ptranking/ltr_adhoc/listwise/softrank.py:47-69 and its backward: expected ranks from
 * 0.5*erfc((s_i-s_j)/sqrt(4*delta^2)), loss = -sum_q sum_{i<top_k} (2^l_i-1)/(log2(E[rank_i]+1)*IDCG_q).  Labels must be
 * in ideal order (the reference asserts presort).  top_k <= 0: no truncation (top_k=None).  delta > 0.
 * A zero-length list has loss 0 and a zero gradient; a list without a relevant document is NaN, as the reference
 * (its gradient too, except a one-document list's, which has no pair and is 0). */
int ptr_softrank_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, float delta, int top_k,
                         float *loss_out, float *loss_q, float *grad, void *stream);

/* ApproxNDCG — replaces ptranking/ltr_adhoc/listwise/approxNDCG.py:19-27,45-62 (+ Robust_Sigmoid,
 * ptranking/base/utils.py:57-95) and its backward.  alpha must be > 0.
 * couple_batch != 0 reproduces the reference: loss = -(sum_b DCG_b) * S, S = sum_a 1/IDCG_a, gradients scaled by
 * S (SURVEY.md §7 vi); couple_batch == 0 gives the per-query normalised form -sum_b DCG_b/IDCG_b.
 * Outputs: loss_out[1]; dcg_q[B] (approximate DCG per query); inv_idcg_q[B]; grad[B,L] (fully scaled);
 * scale_out[2] = {factor applied to the gradients, local S}.  With couple_batch != 0 and grad_scale_override > 0 the
 * gradients and loss are scaled with that value instead of the local S (data parallel: pass 1.0, all-reduce the
 * local S with the parameter gradients and rescale them afterwards — they are linear in S). */
int ptr_approxndcg_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, float alpha,
                           int presort, int couple_batch, float grad_scale_override, float *loss_out, float *dcg_q,
                           float *inv_idcg_q, float *scale_out, float *grad, void *stream);

/* ListNet — replaces ptranking/ltr_adhoc/listwise/listnet.py:39 and its backward. */
int ptr_listnet_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, float *loss_out,
                        float *loss_q, float *grad, void *stream);

/* ---- sibling losses served by the same listwise machinery ----
 * STListNet — replaces ptranking/ltr_adhoc/listwise/st_listnet.py:41-49: ListNet on (preds + gumbel)/temperature with
 * gumbel = -log(-log(u + 1e-20) + 1e-20); `unif` [B,L] holds the uniform draws u (the reference: torch.rand). */
int ptr_stlistnet_fwd_bwd(const float *preds, const float *labels, const float *unif, const int32_t *lens, int B, int L,
                          float temperature, float *loss_out, float *loss_q, float *grad, void *stream);
/* RankMSE — replaces ptranking/ltr_adhoc/pointwise/rank_mse.py:13-22: mean over the B queries of sum_i (s_i - y_i)^2
 * (loss_q holds the per-query sums; loss_out and grad carry the 1/B). */
int ptr_rankmse_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, float *loss_out,
                        float *loss_q, float *grad, void *stream);
/* RankCosine — replaces ptranking/ltr_adhoc/listwise/rank_cosine.py:15,32: sum_q (1 - cos(s_q, y_q)) / 0.5,
 * nn.CosineSimilarity(dim=1, eps=1e-8). */
int ptr_rankcosine_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, float *loss_out,
                           float *loss_q, float *grad, void *stream);

/* ListMLE — replaces ptranking/ltr_adhoc/listwise/listmle.py:82,92-97 and its backward.  `perm` (int64[B,L]) is
 * the tie-shuffled label-descending order the reference obtains from arg_shuffle_ties
 * (ptranking/ltr_adhoc/util/sampling_utils.py:13-28); row q holds a permutation of 0..len_q-1 in its first len_q
 * entries. */
int ptr_listmle_fwd_bwd(const float *preds, const int64_t *perm, const int32_t *lens, int B, int L, float *loss_out,
                        float *loss_q, float *grad, void *stream);

/* MDPRank — replaces ptranking/ltr_adhoc/listwise/mdprank.py:46-75 and its backward: ListMLE on a SAMPLED ranking `perm`
 * (int64[B,L], drawn by the caller from the Plackett-Luce model, sampling_utils.py:32-83) whose first top_k positions are
 * weighted with the discounted long-term return G_t = gamma^(t+1) * sum_{t'=t}^{top_k-1} (2^l - 1)/log2(2 + t').
 * top_k <= 0: the whole list (top_k=None).  The reference only accepts batch size 1; here every query is independent. */
int ptr_mdprank_fwd_bwd(const float *preds, const float *labels, const int64_t *perm, const int32_t *lens, int B, int L, int top_k,
                        float gamma, float *loss_out, float *loss_q, float *grad, void *stream);

#define PTR_WASS_COST_P1 0   /* 'p1':  |i - j| (positions)                  wasserstein_cost_mat.py:47-60,121-122 */
#define PTR_WASS_COST_P2 1   /* 'p2':  |i - j|^2                            :124-125 */
#define PTR_WASS_COST_EG 2   /* 'eg':  explicit grouping of label gains     :84-111,127-129 */
#define PTR_WASS_COST_DG 3   /* 'dg':  delta gain |(2^y_i-1) - (2^y_j-1)|   :63-81,131-132 */
#define PTR_WASS_COST_DDG 4  /* 'ddg': dg * |1/log2(i+2) - 1/log2(j+2)|     :63-81,134-135 */

/* WassRank — replaces ptranking/ltr_adhoc/listwise/wassrank/wassRank.py:43-88 in mode 'SinkhornOT' with smooth_type 'ST' and
 * norm_type 'BothST': get_explicit_cost_mat (wasserstein_cost_mat.py:113-139), get_normalized_histograms (:181-208) and OldSinkhornOT
 * (pytorch_wasserstein.py:323-393), forward and backward in one launch.  Per query with n real documents in the given order:
 *   C_ij from labels and positions (cost_type = PTR_WASS_COST_*): eg: g = gain_base^y - 1, g < 1 -> -non_rele_gap, c = |g_i - g_j|,
 *   c < 1 -> var_penalty (any pair closer than 1), diagonal 0; dg ignores gain_base (base 2); positions are 0-based;
 *   b = softmax(labels), a = softmax(m * preds), m = the query's maximum label if scale_by_max_label != 0, else 1;
 *   log u = log v = -log n, then sh_itr times: log v = log b - LSE_i(log u_i - C_ij/lam), log u = log a - LSE_j(log v_j - C_ij/lam);
 *   loss_q = sum_ij C_ij exp(log u_i - C_ij/lam + log v_j); loss_out = mean over the B queries (the reference's .mean(0).sum());
 *   grad = m a_i (G_i - sum_j a_j G_j), G = lam log u centred / B (the reference's grad, then autograd through F.softmax); padded
 *   documents get 0.
 * Every log-sum-exp is taken with its own row's maximum: the same mathematics as the reference's log(K @ exp(v - max v)) + max v with
 * one shift per query, which underflows to log(0) and NaN in fp32; this form is finite whenever the inputs are.  The reference only
 * runs at batch size 1 (it squeezes the [B,L,L] cost to 2-D); here every query is independent and B = 1 reproduces it.
 * Errors: PTR_ERR_INVALID_ARG for a NULL pointer, a bad cost_type, lam <= 0 or sh_itr < 0; PTR_ERR_UNSUPPORTED for L > PTR_MAX_LIST_LEN. */
int ptr_wassrank_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, int cost_type,
                         float gain_base, float non_rele_gap, float var_penalty, float lam, int sh_itr,
                         int scale_by_max_label, float *loss_out, float *loss_q, float *grad, void *stream);

/* ---- search-result diversification (ABI v8, csrc/diversity.hip): the reference's ltr_diversification frame -------------------------------
 * Data model: preds [B,L]; rele [B,T,L] = per query the reference's q_doc_rele_mat (subtopic-by-document relevance, document axis
 * contiguous, values >= 0, graded values allowed); lens int32[B] (nullable: L) real documents, ntopics int32[B] (nullable: T) real
 * subtopics per query.  Padded documents and padded subtopics are never read, contribute nothing, get gradient 0 and count in no
 * denominator.  The reference runs ONE query per call (ptranking/base/ranker.py:636-669); a batch here is B independent reference calls.
 *
 * ptr_alphadcg_fwd_bwd — DALETOR's loss, replaces ptranking/ltr_diversification/score_and_sort/daletor.py:9-38 (get_approx_ranks,
 * alphaDCG_as_a_loss; Robust_Sigmoid ptranking/base/utils.py:57-95) and its autograd backward in one launch; nothing of size L x L or
 * T x L x L is written.  Per query:  ind[i][j] = rs(rt (s_j - s_i)), pi[i] = 0.5 + sum_j ind[i][j], cover[t][i] = sum_j ind[i][j] R[t][j]
 * - R[t][i] / 2, loss_q = - sum over the kept (t, i) of R[t][i] (1 - alpha)^cover[t][i] / log2(1 + pi[i]).
 *   top_k <= 0: every term is kept (top_k=None).  top_k_axis = PTR_ADCG_TOPK_SUBTOPICS reproduces the reference, whose `[0:top_k]` slices the
 *   SUBTOPIC rows (daletor.py:30-35: the sum over dim=1 runs over documents first): kept <=> t < top_k.  PTR_ADCG_TOPK_DOCUMENTS is the
 *   alpha-DCG@k its docstring describes: kept <=> i < top_k, documents in the given (presorted ideal) order.
 *   loss_q [B], grad [B,L], loss_out [1] = sum of loss_q (nullable).  rt > 0 and 0 < alpha < 1, else PTR_ERR_INVALID_ARG;
 *   PTR_ERR_UNSUPPORTED for L > PTR_MAX_LIST_LEN, T > PTR_MAX_SUBTOPICS, or a query tile beyond the LDS of a compute unit:
 *   8 * round_up(L, 4) * (1 + Tp) + 16 bytes <= 160 KiB, Tp = T rounded up to 4, 8, 16 or 32 (T <= 4: L <= 4092; T <= 8: L <= 2272;
 *   T <= 16: L <= 1204; T <= 32: L <= 620). */
#define PTR_ADCG_TOPK_SUBTOPICS 0
#define PTR_ADCG_TOPK_DOCUMENTS 1
int ptr_alphadcg_fwd_bwd(const float *preds, const float *rele, const int32_t *lens, const int32_t *ntopics, int B, int T, int L, float rt,
                         float alpha, int top_k, int top_k_axis, float *loss_out, float *loss_q, float *grad, void *stream);
/* ptr_div_metrics_at_ks — alpha-nDCG@ks, ERR-IA@ks, nERR-IA@ks: replaces the Evaluator prologue of ptranking/base/ranker.py:269-475 (predict
 * -> .cpu() -> torch.sort -> gather) and ptranking/metric/srd/diversity_metric.py:43-82, :189-245, :265-291.  The scores are ranked like
 * ptr_sort_desc (value descending, original index ascending); the ideal ranking is the INPUT order (ranker.py:296, "under the assumption of
 * presort").  ks: HOST int32[nk]; outputs [B,nk], each nullable; a cut-off k > lens[q] yields 0 (the reference's padding); an ideal value
 * <= 0 yields 0; ERR-IA divides by ntopics[q] (empty subtopics count); max_label (2^max_label normalises the satisfaction
 * probability) must be >= 0 when err_ia or nerr_ia is requested.  valid [B] (nullable) = 0 for a query whose relevance sums to less than 1
 * — the evaluator skips it (ranker.py:282, :319) — else 1; the metric rows of such a query are 0. */
int ptr_div_metrics_at_ks(const float *preds, const float *rele, const int32_t *lens, const int32_t *ntopics, int B, int T, int L,
                          const int32_t *ks, int nk, float alpha, float max_label, float *andcg, float *err_ia, float *nerr_ia,
                          int32_t *valid, void *stream);

/* ---- DivProbRanker's objectives (csrc/divprob.hip).  The two symbols below are ADDITIVE to ABI v8: nothing declared before them changed, so
 * PTR_ABI_VERSION stays 8; a v8 library built before them simply lacks the two names.
 * Data model as above, with two score tensors: mus [B,L] and vars [B,L], the mean and the variance the scorer predicts per document.  With
 * x[i][j] = (mu_i - mu_j) / sqrt(2 (var_i + var_j)), Phi[i][j] = erfc(x[i][j]) / 2 for j != i and the expected rank R[i] = 1 + sum_j Phi[i][j]
 * (ptranking/ltr_diversification/util/prob_utils.py:5-26, :62-80).  A variance <= 0 among the first lens[q] documents is the caller's
 * error: the pair argument divides by zero and the query's outputs are NaN (nothing is checked on the device).  A query with
 * ntopics[q] = 0 contributes exactly 0.
 *
 * ptr_divprob_fwd_bwd — one launch for the loss and both gradients of one of the four objectives (opt_ideal: documents in the given, presorted
 * order), replacing the op sequences of ptranking/ltr_diversification/score_and_sort/div_prob_ranker.py and their autograd backward:
 *   PTR_DIVPROB_ANDCG          alpha_dcg_as_a_loss, div_prob_ranker.py:29-79: c[t][i] = sum_j Phi[i][j] r[t][j], loss_q = - sum over the kept
 *                              (t, i) of r[t][i] (1 - beta)^c[t][i] / log2(1 + R[i]); top_k / top_k_axis exactly as ptr_alphadcg_fwd_bwd
 *                              (PTR_ADCG_TOPK_SUBTOPICS reproduces the reference's slice of SUBTOPIC rows, :70-75).
 *   PTR_DIVPROB_ERRIA          err_ia_as_a_loss, :81-165: s = (2^r - 1) / 2^max_label, loss_q = - sum_t sum_i s[t][i] prod_{k<i} (1 - s[t][k])
 *                              / R[i] over the first top_k documents (top_k <= 0 or >= lens: all; top_k_axis is not used).
 *   PTR_DIVPROB_PAIRCLS        prob_lambda_loss('PairCLS'), :167-181 + util/div_lambda_utils.py:26-43: over pairs i < j,
 *                              - [ tb log P + (1 - tb) log Q ], Q = Phi[i][j], P = 1 - Q, tb = mean over the query's subtopics of
 *                              (1 + clamp(r[t][i] - r[t][j], -1, 1)) / 2; each logarithm is clamped at -100 as F.binary_cross_entropy does.
 *   PTR_DIVPROB_LAMBDAPAIRCLS  prob_lambda_loss('LambdaPairCLS', opt_ideal), :182-202: the same term times get_delta_alpha_dcg of the input order
 *                              (ptranking/metric/srd/diversity_metric.py:143-183), | sum_t (g_ti - g_tj)(d_i f_ti - d_j f_tj) | with g = 2^r - 1,
 *                              d_i = 1 / log2(i + 2), f_ti = (1 - beta)^(sum_{k<i} r[t][k]); norm != 0 divides by the input order's alpha-DCG
 *                              (:13-30); an ideal value <= 0 gives weight 0 where the reference divides by zero.
 *   log Q and log P are computed from the scaled complementary error function, never through 1 - Q, so they stay exact where the reference's
 *   fp32 `1 - erfc(x) / 2` has rounded to 1 (|x| >= 3.8); a logarithm at the -100 clamp passes no gradient, elsewhere the gradient
 *   is the exact ratio exp(-x^2) / (sqrt(pi) Q).  top_k, max_label and norm are ignored by the objectives that do not name them.
 *   loss_q [B], grad_mu [B,L], grad_var [B,L], loss_out [1] = sum of loss_q (nullable).  PTR_ERR_INVALID_ARG: a NULL pointer, objective or
 *   top_k_axis out of range, beta outside (0, 1), max_label < 0 for PTR_DIVPROB_ERRIA.  PTR_ERR_UNSUPPORTED: L > PTR_MAX_LIST_LEN,
 *   T > PTR_MAX_SUBTOPICS, or a query tile beyond the LDS of a compute unit: 4 * round_up(L, 4) * (3 + K * Tp) + 16 bytes <= 160 KiB, Tp = T
 *   rounded up to 4, 8, 16 or 32, K = the relevance-sized tiles the objective keeps: 1 for ERRIA and PAIRCLS (T <= 4: L <= 4096; T <= 8:
 *   L <= 3720; T <= 16: L <= 2152; T <= 32: L <= 1168), 2 for ANDCG (T <= 4: L <= 3720; T <= 8: L <= 2152; T <= 16: L <= 1168; T <= 32:
 *   L <= 608), 3 for LAMBDAPAIRCLS (T <= 4: L <= 2728; T <= 8: L <= 1516; T <= 16: L <= 800; T <= 32: L <= 412). */
#define PTR_DIVPROB_ANDCG 0
#define PTR_DIVPROB_ERRIA 1
#define PTR_DIVPROB_PAIRCLS 2
#define PTR_DIVPROB_LAMBDAPAIRCLS 3
int ptr_divprob_fwd_bwd(const float *mus, const float *vars, const float *rele, const int32_t *lens, const int32_t *ntopics, int B, int T, int L,
                        int objective, float beta, int top_k, int top_k_axis, float max_label, int norm, float *loss_out, float *loss_q,
                        float *grad_mu, float *grad_var, void *stream);
/* ptr_divprob_expected_ranks — ranks [B,L] = R[i] (get_expected_rank, prob_utils.py:62-80; the 'RERAR' sort key of
 * ptranking/ltr_diversification/base/div_mdn_ranker.py:314-320 is its reciprocal): the first pass of the kernel above, forward only.
 * Padded documents get 0.  LDS: 12 * round_up(L, 4) bytes per query (48 KiB at L = PTR_MAX_LIST_LEN = 4096; 6 KiB per workgroup of four
 * queries at L = 128): every supported L fits. */
int ptr_divprob_expected_ranks(const float *mus, const float *vars, const int32_t *lens, int B, int L, float *ranks, void *stream);

/* ---- TREC ndeval's diversity measures and its greedy ideal ranking (csrc/ndeval.hip).  The symbol below is ADDITIVE to ABI v8 as well:
 * PTR_ABI_VERSION stays 8.
 * ptr_ndeval_measures — what ptranking/metric/srd/ndeval.c (ndeval 4.4, the one native component of the reference, run by
 * DivLTREvaluator.fold_evaluation_reproduce) prints per topic, in float64 and bit for bit: the same IEEE double operations in the same
 * order.  Data model as above; judgments are binarised (rele > 0 is relevant, ndeval.c:908).  Per query:
 *   pool     the first lens[q] documents (the qrels' document set); nrelSub[j] = the number of documents relevant to subtopic j;
 *            S = actual_subtopics[q] = the number of subtopics with nrelSub > 0 (actualSubtopics, :336-345).
 *   run      the pool ranked as ptr_sort_desc ranks it (value descending, NaN first, original index ascending); preds == NULL: the input
 *            order.  depth_m > 0 keeps the first depth_m ranked documents (ndeval -M, :1000-1020); the ideal side always uses the whole
 *            pool.  A document with an all-zero column is an unjudged document.
 *   ideal    ideal_order [B,L] (nullable; entries beyond lens[q] = -1), idealResult :351-400: lens[q] greedy rounds; a candidate scores the
 *            sum over its subtopics j, ascending, of gain[j]; gain[j] starts at 1 and is multiplied by (1 - alpha) whenever a chosen
 *            document covers j; the largest score wins, ties go to the larger document index (ndeval's "larger docno" with zero-padded
 *            docnos).  Scores are doubles compared for equality, so the tie decisions are ndeval's.
 *   per_k    [B,6,nk] (nullable) at the HOST cut-offs ks[nk], each in 1..PTR_NDEVAL_DEPTH: ERR-IA (computeERR :597-643), nERR-IA, alpha-DCG
 *            (computeDCG :651-698), alpha-nDCG (renormalize :1143-1156: run / ideal, 0 wherever the run's alpha-DCG is 0), P-IA
 *            (computePrecision :736-759) and strec (computeSTRecall :704-730).  The cumulative arrays are divided by the cumulative "ideal
 *            ideal" array (gain S, S (1 - alpha), ...) from index 1 on only: at k = 1 the two raw measures are NOT divided by S — ndeval's
 *            behaviour, kept.  A run shorter than k: the counts freeze and P-IA still divides by k S.
 *   per_q    [B,3] (nullable): NRBP (computeNRBP :531-562, over the whole run), nNRBP = NRBP / the ideal ranking's NRBP, MAP-IA (computeMAP
 *            :484-525, denominators = the pool's nrelSub).
 *   S == 0 (lens[q] == 0 included): every measure is 0 and nNRBP is NaN (0 / 0), as ndeval prints; callers filter on actual_subtopics
 *   [B] (nullable).
 * Padded documents and padded subtopics are never read.  log() is evaluated on the host only (the 20 discounts log 2 / log(i + 2)).
 * One wavefront per query, four queries per workgroup, up to 128 documents; one workgroup per query beyond.  LDS per query:
 * 32 * round_up(L, 4) + 1664 bytes (129.6 KiB at L = PTR_MAX_LIST_LEN = 4096): every supported L fits the 160 KiB of a compute unit, so the
 * LDS limit coincides with PTR_MAX_LIST_LEN.
 * Errors, before any launch: PTR_ERR_INVALID_ARG for a NULL rele, alpha outside (0, 1), beta outside [0, 1] (NaN included), depth_m < 0,
 * a cut-off outside 1..PTR_NDEVAL_DEPTH; PTR_ERR_UNSUPPORTED for L > PTR_MAX_LIST_LEN, T > PTR_MAX_SUBTOPICS, nk > PTR_MAX_CUTOFFS or a
 * query tile beyond the LDS of a compute unit.  B == 0 succeeds. */
#define PTR_NDEVAL_DEPTH 20
int ptr_ndeval_measures(const float *preds, const float *rele, const int32_t *lens, const int32_t *ntopics, int B, int T, int L,
                        const int32_t *ks, int nk, double alpha, double beta, int depth_m, double *per_k, double *per_q,
                        int32_t *actual_subtopics, int32_t *ideal_order, void *stream);

/* ---- The tree frame's custom objectives (csrc/tree.hip).  The two symbols below are ADDITIVE to ABI v8 as well: PTR_ABI_VERSION stays 8.
 * They compute what a LightGBM custom objective returns every boosting round — a gradient and a Hessian per document — and nothing else of
 * the tree frame: the boosting stays in LightGBM.
 * Data model: RAGGED, LightGBM's layout.  preds and labels are flat fp32 arrays over all documents, offsets int64 [B + 1] (device) the
 * running sum of the group sizes: query q owns [offsets[q], offsets[q + 1]).  grad and hess are flat fp32 arrays of the same length.  There
 * is no padding.  queries (int32 [nq], device, nullable) lists the queries to evaluate; NULL means all B of them, and then nq must equal B.
 * max_len is the longest list among the launched queries (the host knows it): it sizes the LDS rows and selects the form — 16 queries per
 * workgroup up to 16 documents, one wavefront per query up to 128, one workgroup per query up to PTR_MAX_LIST_LEN — so a caller with mixed
 * lengths buckets its queries by length once and launches each class through `queries`.  Results do not depend on the form, on the other
 * queries of the launch or on the run: every sum has a fixed order that depends on the query alone.  A launched query longer than max_len is
 * the caller's error and gets NaN; a query of 0 documents writes nothing; documents of queries that are not launched are not written.
 *
 * ptr_tree_pair_grad_hess replaces per_query_gradient_hessian_lambda (ptranking/ltr_tree/util/lightgbm_util.py:120-183, a Python loop over
 * document pairs) with triu_indice (:17-60), get_delta_ndcg / get_delta_gains / ideal_dcg (:82-118), and the loop over `group` of the four
 * RankNet / LambdaRank wrappers (:185-302).  Per document i, over the partners j != i of its query that pass the pair mask, d = s_i - s_j:
 *     grad_i = sum_j w_ij epsilon (sigmoid(epsilon d) - (1 + clip(y_i - y_j, -1, 1)) / 2)
 *     h_ij   = max(epsilon^2 sigmoid(d) (1 - sigmoid(d)), 1e-16) w_ij
 *   pair_type  PTR_TREE_PAIRS_ALL / _NOTIES (labels differ) / _NO00 (not both 0) / _00 (both 0): the four masks of triu_indice.
 *   weighting  PTR_TREE_W_NONE: w = 1.  _DELTA_NDCG: |G_i - G_j| |D_i - D_j|, G = (2^y - 1) / IDCG, D = 1 / log2(rank + 2), rank 0-based in
 *              predicted order.  _DELTA_GAIN: |g_i - g_j|, g = 2^y - 1.
 *              Finding 1: the reference's lambdarank wrappers (:244-302) pass weighting=True, and `True in ['DeltaNDCG', 'DeltaGain']` is
 *              false (:149): its "lambdarank" objective is UNWEIGHTED RankNet over NoTies pairs.  That is PTR_TREE_W_NONE here; the weights
 *              are what the per-query function computes when it is called with weighting='DeltaNDCG' / 'DeltaGain'.
 *   hessian    PTR_TREE_HESS_REFERENCE: hess_i = sum_j h_ij over the partners ranked below i minus the sum over those ranked above it.
 *              Finding 2: the reference adds +h to the higher-ranked document of a pair and -h to the lower one (:175-178), so its
 *              Hessian is negative for low-ranked documents.  _SUM: hess_i = sum_j h_ij, what LightGBM and XGBoost do; never negative.
 *              _CONSTANT: the reference's FIRST_ORDER: hess is filled with 1.0 and no pair Hessian is evaluated.
 *              Finding 3: the Hessian's sigmoid is taken at epsilon 1 whatever epsilon is (:171), and the 1e-16 floor applies before the weight.
 *   Finding 4 (group.astype(np.int), which numpy >= 1.24 refuses) concerns the Python wrappers only: offsets are int64 here.
 *   Finding 5: np.flip(np.argsort(preds)) (:130) breaks ties in an implementation-defined way.  Here a higher score ranks first and equal
 *              scores rank by original index (the rule of ptr_lambdarank_fwd_bwd): it decides D and the Hessian's sign, e.g. on the
 *              all-equal scores of the first boosting round.
 *   Edge rules, as the reference: one document: grad = hess = 0.  No pair passes the mask (all-equal labels under NOTIES): 0 under every
 *   weighting.  No relevant document with pairs under _DELTA_NDCG: NaN (the normalised gains are 0 / 0).  A NaN score or label: NaN grad and
 *   hess on every document of that list and of no other (hess stays 1.0 under _CONSTANT).
 *
 * ptr_tree_listnet_grad_hess replaces per_query_gradient_hessian_listnet (:308-330) and the loop of its two wrappers (:333-389):
 *     grad = softmax(s) - softmax(gain), hess = p (1 - p), p = softmax(s); gain = 2^y - 1 (PTR_TREE_GAIN_POWER) or y (PTR_TREE_GAIN_LABEL).
 *   hessian: _REFERENCE and _SUM coincide; _CONSTANT fills 1.0.  One document: grad 0, hess 0 (p = 1).  Findings 4 and 5 do not reach it
 *   (nothing is sorted), nor do 1 to 3.
 *
 * PTR_ERR_INVALID_ARG (before any launch): a NULL pointer while nq > 0, a negative size, queries == NULL with nq != B, epsilon < 0 or NaN, an
 * enum value out of range.  PTR_ERR_UNSUPPORTED: max_len > PTR_MAX_LIST_LEN.  LDS per query: 4 round_up(max_len, 4) bytes times 2 (no weights),
 * 3 (_DELTA_GAIN, ListNet) or 4 (_DELTA_NDCG): 64 KiB at 4096 documents.
 *
 * ptr_tree_lambdarank_ndcg_grad_hess (ADDITIVE to ABI v8: PTR_ABI_VERSION stays 8) is the truncated, normalised lambdarank that the
 * reference's tree frame runs by default through LightGBM's built-in objective='lambdarank' (lightgbm_lambdaMART.py:170-185).  The rule below
 * is THIS PROJECT'S OWN, modelled on LightGBM's LambdarankNDCG; LightGBM is not available where this library is built and tested, the rule is
 * compared with nothing of LightGBM's, and no parity with it is claimed.  Same ragged layout, `queries` subset list, max_len contract and
 * forms as above.  For one query of n documents, scores s, labels y >= 0, gain g = 2^y - 1, r(i) the 0-based rank of document i in
 * predicted order (a higher score first, equal scores by original index), D(r) = 1 / log2(r + 2), T = truncation_level >= 1,
 * sigma = sigmoid > 0:
 *   1. maxDCG = the sum over the min(T, n) largest gains, in descending order, of g D(position); inv = 1 / maxDCG where maxDCG > 0, else 0.
 *   2. A pair {i, j} counts if and only if y_i != y_j and min(r(i), r(j)) < T.  `hi` is its document of the larger label, `lo` the other,
 *      ds = s_hi - s_lo.
 *   3. delta = (g_hi - g_lo) |D(r(hi)) - D(r(lo))| inv; if norm is set and the query's largest and smallest scores differ,
 *      delta /= (0.01 + |ds|).
 *   4. p = 1 / (1 + exp(sigma ds)), lam = sigma delta p, h = sigma^2 delta p (1 - p).
 *   5. grad[hi] -= lam, grad[lo] += lam, hess[hi] += h, hess[lo] += h, S += 2 lam.
 *   6. If norm is set and S > 0, every grad and hess of the query is multiplied by log2(1 + S) / S.
 *   (Two labels so close that their fp32 gains coincide give delta = 0: such a pair contributes nothing either way.)
 *   The gradients of a query sum to 0 and no Hessian is negative.  One document, equal labels, or NO RELEVANT DOCUMENT: exactly 0 in both
 *   outputs.  The last case DIFFERS from PTR_TREE_W_DELTA_NDCG above, which returns NaN there (its normalised gains are 0 / 0); here inv = 0.
 *   With T >= n, norm = 0 and sigmoid = 1 the result is that of ptr_tree_pair_grad_hess(PTR_TREE_PAIRS_NOTIES, PTR_TREE_W_DELTA_NDCG,
 *   epsilon 1, PTR_TREE_HESS_SUM) on every list that holds a relevant document, up to rounding and that kernel's 1e-16 Hessian floor.
 *   A NaN score or label: NaN on every document of that list and of no other.  A launched query longer than max_len: NaN, as above.
 *   norm: 0 is off, any other value is on.  PTR_ERR_INVALID_ARG as above, and for truncation_level < 1 or a sigmoid that is not > 0 (NaN
 *   included).  No atomics, nothing of size n x n; every sum has an order that depends on the query alone (each document's partners in rank
 *   order; maxDCG and S by a halving tree over n).  LDS per query: 28 round_up(max_len, 4) bytes, 112 KiB at 4096 documents.
 *
 * ptr_tree_xendcg_grad_hess (ADDITIVE to ABI v8: PTR_ABI_VERSION stays 8) is the cross-entropy nDCG objective (Bruch, "An Alternative Cross
 * Entropy Loss for Learning-to-Rank"), LightGBM's second built-in ranking objective, objective='rank_xendcg'.  The rule below is THIS
 * PROJECT'S OWN, modelled on LightGBM's RankXENDCG; LightGBM is not available where this library is built and tested, the rule is compared
 * with nothing of LightGBM's, and no parity with it is claimed (its random stream in particular is not reproduced).  Same ragged layout,
 * `queries` subset list, max_len contract and forms as above.  It costs O(n) per query.  For one query of n documents, scores s, labels
 * y >= 0 and one uniform u_i in [0, 1) per document:
 *   1. n <= 1: grad = hess = 0 exactly.
 *   2. rho_i = exp(s_i - max s) / Z, Z the sum of the numerators (the softmax of ptr_tree_listnet_grad_hess, by the same code).
 *   3. phi_i = 2^{y_i} - u_i (> 0, since u_i < 1); P = sum_j phi_j.
 *   4. q_i = max(1 - rho_i, 2^-20).  The floor is this project's addition: LightGBM divides by 1 - rho unguarded and returns inf / NaN when
 *      one document holds all of the softmax mass in fp32.  With the floor every output is finite for finite inputs.
 *   5. First order:  a_i = rho_i - phi_i / P,  x_i = a_i / q_i,  A = sum_i x_i.
 *   6. Second order: b_i = rho_i (A - x_i),    z_i = b_i / q_i,  Bs = sum_i z_i.
 *   7. Third order:  c_i = rho_i (Bs - z_i).
 *   8. grad_i = (a_i + b_i) + c_i;  hess_i = rho_i (1 - rho_i), UNFLOORED, never negative.
 *   Edge rules: a NaN score or label, a negative label, or a supplied uniform outside [0, 1) (NaN included) gives NaN grad and hess on every
 *   document of that list — a list of one document included — and of no other list.  A launched query longer than max_len: NaN, as above.
 *   The uniforms: unif == NULL draws them from the counter stream of ptr_pl_uniforms' hash (csrc/ptr_plhash.h): for the GLOBAL document
 *   index d = offsets[q] + i, keys = pl_sample_keys(pl_query_keys(seed, draw), hi32(d)) and u = pl_uniform(keys, lo32(d)), a multiple of
 *   2^-24 in [0, 1).  A document's uniform depends on (seed, draw, d) alone, not on the length class, subset or form that launched its query;
 *   a caller passes the boosting round as `draw`.  unif != NULL is a device array of one fp32 uniform per document [documents], read in
 *   place of the stream (seed and draw are then unused).
 *   Every sum (max, Z, P, A, Bs) is a halving tree over n whose shape depends on n alone: the bits of a list do not depend on the form, the
 *   launch or the batch around it.  No atomics, nothing of size n x n.  One thread owns document i (strided where the list is longer than
 *   the group) and keeps rho_i, q_i and its running terms in registers across the three passes.  PTR_ERR_INVALID_ARG as above (`hessian`
 *   does not exist here), and for draw < 0.  LDS per query: 2 rows (the scores | the tree's row), 8 round_up(max_len, 4) bytes, 32 KiB at
 *   4096 documents. */
#define PTR_TREE_PAIRS_ALL 0
#define PTR_TREE_PAIRS_NOTIES 1
#define PTR_TREE_PAIRS_NO00 2
#define PTR_TREE_PAIRS_00 3
#define PTR_TREE_W_NONE 0
#define PTR_TREE_W_DELTA_NDCG 1
#define PTR_TREE_W_DELTA_GAIN 2
#define PTR_TREE_HESS_REFERENCE 0
#define PTR_TREE_HESS_SUM 1
#define PTR_TREE_HESS_CONSTANT 2
#define PTR_TREE_GAIN_POWER 0
#define PTR_TREE_GAIN_LABEL 1
int ptr_tree_pair_grad_hess(const float *preds, const float *labels, const int64_t *offsets, int B, const int32_t *queries, int nq, int max_len,
                            int pair_type, int weighting, float epsilon, int hessian, float *grad, float *hess, void *stream);
int ptr_tree_listnet_grad_hess(const float *preds, const float *labels, const int64_t *offsets, int B, const int32_t *queries, int nq, int max_len,
                               int gain_type, int hessian, float *grad, float *hess, void *stream);
int ptr_tree_lambdarank_ndcg_grad_hess(const float *preds, const float *labels, const int64_t *offsets, int B, const int32_t *queries, int nq,
                                       int max_len, int truncation_level, float sigmoid, int norm, float *grad, float *hess, void *stream);
int ptr_tree_xendcg_grad_hess(const float *preds, const float *labels, const int64_t *offsets, int B, const int32_t *queries, int nq,
                              int max_len, const float *unif, uint64_t seed, int64_t draw, float *grad, float *hess, void *stream);

/* ---- Smooth-rank metric objectives (csrc/smoothmetric.hip).  The symbol below is ADDITIVE to ABI v8 as well: PTR_ABI_VERSION stays 8.
 * ptr_smoothmetric_fwd_bwd — loss and dLoss/dpreds of precision_ / AP_ / nERR_ / nDCG_as_opt_objective
 * (ptranking/metric/smooth_metric/metric_as_opt_objective.py:12-257) on the smooth ranks of get_approx_ranks
 * (ptranking/ltr_adhoc/listwise/approxNDCG.py:19-27), with their autograd backward, in one launch.  The reference knows no padding: the
 * contract is "the reference on the unpadded list, one query at a time", loss_out = the sum over the queries.
 *   labels     in ideal (descending) order per query: the reference asserts presort for nERR, nDCG and every opt_ideal form; there is no
 *              unsorted mode.  Graded (MultiLabel) labels.
 *   top_k      <= 0 means None.  K = n (None) or min(top_k, n); Kdiv = n (None) or top_k (P divides by top_k even on a shorter list).  The
 *              reference's nERR raises for top_k > n; here K is clamped for every metric.
 *   max_label  nERR only (2^max_label normalises the satisfaction probability); < 0 => the batch maximum over the valid documents (the
 *              reference's torch.max(batch_std_labels)) is computed on the device into max_label_ws[1], with no host sync — the convention
 *              of ptr_metrics_at_ks.  max_label_ws may be NULL otherwise.
 *   Per query, n = lens[q]:   r_i = 1 + sum_{j != i} rs(alpha (s_j - s_i));   loss_q = - sum_i W_i phi(r_i), phi(r) = 1 / r (P, AP, nERR) or
 *   1 / log2(1 + r) (nDCG).  pos_i = the input index under opt_ideal, else the 0-based rank by (score descending, index ascending) — the
 *   order of the reference's torch.sort of the smooth ranks whenever those are distinct.  b = clamp(y, 0, 1); yp, bp = labels by position:
 *     P      W_i = [pos_i < K] (pos_i + 1) b_i / Kdiv
 *     AP     W_i = [pos_i < K] (pos_i + 1) (sum_{pos_i <= p < K} bp_p / (p + 1)) / sum_{p < K} bp_p;  opt_ideal == 0 with top_k <= 0 takes the
 *            reference's other formula (:118-123): W_i = b_i #{relevant at positions <= pos_i} / sum b
 *     nERR   sat = (2^yp - 1) / 2^max_label;  W_i = [pos_i < K] sat_{pos_i} prod_{p < pos_i} (1 - sat_p) / idealERR@K, the ideal value the same
 *            expression over the input order with 1 / (p + 1) for 1 / r
 *     nDCG   W_i = [pos_i < K] (2^y_i - 1) / IDCG, the IDCG over the WHOLE list even under top_k (the reference slices a [B, 1] tensor)
 *   Filter (opt_ideal == 0 and top_k > 0, the reference's pos_inds): a query whose top-K positions hold no relevant document (sum of bp for P
 *   and AP, of the labels for nERR, of the gains for nDCG equal to 0) contributes loss 0 and gradient 0, and valid_q = 0.  In every other form
 *   a list without a relevant document gives what the reference gives: 0 for P, 0 / 0 = NaN for AP, nERR and nDCG, confined to that query's
 *   loss_q and gradient row (and loss_out).  n = 0: loss 0, gradient 0, valid 0.  n = 1: no pair, the gradient is exactly 0 — or NaN
 *   where the loss is (the reference's backward passes +c and -c through the diagonal of its difference matrix).
 *   Outputs: loss_q [B], grad [B,L] (padded slots exactly 0), loss_out [1] = sum of loss_q (nullable: the caller sums loss_q with
 *   ptr_sum_f32), valid_q [B] (nullable; 1.0 where the query contributed), ranks [B,L] (nullable; the smooth ranks, 0 on padding).
 *   Lists of up to 512 documents: one wavefront per query out of registers; up to PTR_MAX_LIST_LEN: one workgroup per query (24 KiB of LDS up
 *   to L = 1024, 48 KiB up to 2048, 96 KiB beyond, + 16 bytes).  No atomics.  A query's outputs depend on (its documents, L) alone: the same bits
 *   alone, in any batch of the same padded width L and on every run; another L selects another form and another order of the sums.
 *   PTR_ERR_INVALID_ARG (before any launch): a NULL required pointer, metric outside 0..3, alpha <= 0 or NaN, L <= 0 or L > PTR_MAX_LIST_LEN,
 *   nERR with max_label < 0 and no max_label_ws. */
#define PTR_SMOOTH_P 0
#define PTR_SMOOTH_AP 1
#define PTR_SMOOTH_NERR 2
#define PTR_SMOOTH_NDCG 3
int ptr_smoothmetric_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, int metric, int opt_ideal, int top_k,
                             float alpha, float max_label, float *loss_out, float *loss_q, float *valid_q, float *ranks, float *max_label_ws,
                             float *grad, void *stream);

/* ---- Gaussian expected-rank metric objectives (csrc/gaussmetric.hip).  The symbol below is ADDITIVE to ABI v8 as well: PTR_ABI_VERSION stays 8.
 * ptr_gaussmetric_fwd_bwd — loss, dLoss/dmus and dLoss/dvars of precision_ / AP_ / nERR_ / nDCG_as_opt_objective
 * (ptranking/metric/smooth_metric/metric_as_opt_objective.py:12-257) on the expected ranks of documents whose scores are independent normal
 * variables, get_expected_rank / get_expected_rank_const (ptranking/ltr_diversification/util/prob_utils.py:62-101), with their autograd
 * backward, in one launch.  The contract is that of ptr_smoothmetric_fwd_bwd with the rank source exchanged: metric, labels, top_k (K,
 * Kdiv), max_label / max_label_ws, the weights W_i per form, the filter with valid_q, n = 0, "the reference on the unpadded list, one query
 * at a time" and padded slots exactly 0 are as documented there.
 *   Per query, n = lens[q]:   x_ij = (mu_i - mu_j) / sqrt(2 (v_i + v_j));   r_i = 1 + sum_{j != i} erfc(x_ij) / 2;
 *   loss_q = - sum_i W_i phi(r_i).  With u_i = -W_i phi'(r_i), g = exp(-x^2) / sqrt(pi) and a = 1 / sqrt(2 (v_i + v_j)):
 *   dloss/dmu_i = sum_j g a (u_j - u_i),   dloss/dv_i = sum_j g a (x a) (u_i - u_j).
 *   pos_i = the input index under opt_ideal, else the 0-based rank of the kernel's OWN fp32 r_i ascending with ties by index ascending (the
 *   reference's torch.sort of the ranks).  Expected ranks are not monotone in the mean, so the order is counted from the computed ranks.
 *   vars       [B,L], or NULL: every document then has the variance const_std^2 (rounded once from the double product), const_std > 0 the
 *              reference's `const_var`, which is a standard deviation (prob_utils.py:87); grad_var may then be NULL, and the results are
 *              bit-identical to a call with vars filled with that value.  A variance <= 0 is the caller's error: NaN for that query, as in
 *              ptr_divprob_fwd_bwd.
 *   A list without a relevant document gives what the reference gives (0 for P; NaN for AP, nERR and nDCG in the unfiltered forms, in that
 *   query's loss_q and gradient rows).  n = 1: no pair, both gradients are exactly 0 even where the loss is NaN (the reference masks the
 *   diagonal out of its sum).
 *   Outputs: loss_q [B], grad_mu [B,L], grad_var [B,L] (nullable with vars == NULL), loss_out [1] (nullable), valid_q [B] (nullable),
 *   ranks [B,L] (nullable; r, 0 on padding), pos [B,L] int32 (nullable; the hard positions, -1 on padding).
 *   Lists of up to 512 documents: one wavefront per query out of registers, four queries per workgroup — a ring over the lanes that
 *   evaluates every unordered pair once (8 bytes of LDS per document slot, 1, 2, 3, 4, 6 or 8 x 64 slots, for the rank count and the weight
 *   step); up to PTR_MAX_LIST_LEN: one workgroup per query, every document walks all its partners (16 bytes per slot, 4, 8 or 16 x 256 slots:
 *   64 KiB at L = 4096, + 16 bytes).  No atomics, nothing of size n x n; the sums over the partners are compensated.  A query's outputs
 *   depend on (its documents, L) alone.
 *   PTR_ERR_INVALID_ARG (before any launch): a NULL required pointer, vars == NULL with const_std <= 0 or NaN, vars != NULL with
 *   grad_var == NULL, metric outside 0..3, L <= 0 or L > PTR_MAX_LIST_LEN, nERR with max_label < 0 and no max_label_ws. */
int ptr_gaussmetric_fwd_bwd(const float *mus, const float *vars, const float *labels, const int32_t *lens, int B, int L, int metric,
                            int opt_ideal, int top_k, float const_std, float max_label, float *loss_out, float *loss_q, float *valid_q,
                            float *ranks, int32_t *pos, float *max_label_ws, float *grad_mu, float *grad_var, void *stream);

/* ---- Device Plackett-Luce sampling and the fused multi-sample MDPRank loss (csrc/plsample.hip).  The three symbols below are ADDITIVE to
 * ABI v8 as well: PTR_ABI_VERSION stays 8.
 * A ranking from the Plackett-Luce model with weights exp(s_i / T) is the descending order of s_i / T + g_i, g_i i.i.d. standard Gumbel.
 *   u(seed, q0 + q, s, i)  a multiple of 2^-24 in [0, 1) from a counter hash (32-bit arithmetic); q0 = the GLOBAL index of the batch's first
 *                          query, so a shard of a batch draws what the whole batch would.  g = -log(-log(u + 1e-20) + 1e-20) in fp32
 *                          (ptranking/ltr_adhoc/util/sampling_utils.py:68), so g lies in [-3.83, 16.6].
 *   unif                   nullable [B,S,L] by document: replaces the hash (the parity route: the reference's torch.rand draws).
 *   PTR_PL_DIST_PL         key s_i / T + g_i (s_i at T == 1, sampling_utils.py:41-44) — the law of sample_ranking_PL's torch.multinomial
 *                          without replacement (:49), with no weight that can underflow; action = the raw scores in sampled order (:56).
 *   PTR_PL_DIST_STPL       key s_i + g_i; action = (s_i + g_i) / T in sampled order, no division at T == 1 (sampling_utils.py:60-81,
 *                          ptranking/ltr_adversarial/util/list_sampling.py:38-67 with S = num_sample_ranking).  T does not enter the
 *                          ranking's law there, as in the reference.
 *   Order (key descending, index ascending), as ptr_sort_desc.  Padded documents never enter the sort: perm[q,s,p] = p for p >= lens[q] and
 *   action is 0 there; n = 0 gives the identity; a list with a NaN score gets the identity and NaN action on its real positions.
 * ptr_pl_uniforms writes the uniforms [B,S,L] the two entry points below draw.
 * ptr_pl_sample writes perm int64 [B,S,L] and, when action != NULL, action [B,S,L].
 * ptr_mdprank_sample_fwd_bwd draws the S rankings of every query and evaluates ptranking/ltr_adhoc/listwise/mdprank.py:45-71 on each, in one
 * launch (the maths of ptr_mdprank_fwd_bwd): loss_q[q] = (1/S) sum_s loss(q,s), grad[q,i] = (1/S) sum_s d loss(q,s) / d s_i, loss_out = sum_q
 * loss_q (nullable), perm_out nullable [B,S,L].  Under 'PL' the loss sees the raw scores (no 1/T in the gradient: T only shapes the draw,
 * mdprank.py:37); under 'STPL' it sees (s + g) / T and the gradient carries 1/T (:40-41).  S = 1 is the reference's episode.  n = 0: loss 0,
 * gradient 0.  A NaN score makes the loss and every gradient entry of that list NaN.  top_k <= 0: the whole list.
 * An episode whose action values spread over more than 80 units is evaluated in the log domain: where the reference's log(cumsum(exp)) is
 * -inf the loss and the gradient stay finite.
 *   One wavefront per query up to 1024 documents (register sort), one workgroup per query up to PTR_MAX_LIST_LEN; LDS per query 16 or 24
 *   bytes (sampler / loss) x 64 ceil(L / 64) up to 1024 documents, 12 or 20 bytes x round_up(L, 4) + 16 beyond.  No atomics: a query's bits
 *   depend on (its data, L, S, seed, q0 + q) alone.
 *   PTR_ERR_INVALID_ARG (before any HIP call): B < 0, L <= 0, L > PTR_MAX_LIST_LEN, S < 1, temperature <= 0 or NaN, a distribution other
 *   than the two, gamma <= 0 or NaN, and with B > 0 a NULL preds / labels / perm / loss_q / grad / unif (ptr_pl_uniforms). */
#define PTR_PL_DIST_PL 0
#define PTR_PL_DIST_STPL 1
int ptr_pl_uniforms(int B, int L, int S, uint64_t seed, int64_t q0, float *unif, void *stream);
int ptr_pl_sample(const float *preds, const int32_t *lens, int B, int L, int S, float temperature, int distribution, uint64_t seed, int64_t q0,
                  const float *unif, int64_t *perm, float *action, void *stream);
int ptr_mdprank_sample_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, int S, int top_k, float gamma,
                               float temperature, int distribution, uint64_t seed, int64_t q0, const float *unif, float *loss_out,
                               float *loss_q, float *grad, int64_t *perm_out, void *stream);

/* ---- The adversarial frame's IRGAN point and pair machines (csrc/irgan.hip): sampling documents from the generator's distribution and the
 * two players' losses.  The three symbols below are ADDITIVE to ABI v8 as well: PTR_ABI_VERSION stays 8.
 * Reference: ptranking/ltr_adversarial/pointwise/irgan_point.py, ptranking/ltr_adversarial/pairwise/irgan_pair.py, one query per step there;
 * here a padded batch [B,L] with lens, and num_pos int32 [B] = the number of relevant documents of a list, which sit at its front (the
 * reference's train_presort assert); num_pos is clamped to 0 .. lens.  n = lens[q], P = num_pos[q] below.
 * Uniforms: u(seed, q0 + q, stream, index) of ptr_pl_uniforms; `unif` (nullable) replaces the hash, laid out [B, streams, L] as
 * ptr_pl_uniforms(B, L, streams) writes it.
 * Sampling rules.
 *   with replacement     the inverse CDF on the inclusive prefix sum C of the unnormalised fp32 weights w_i: draw k takes the smallest i with
 *                        u_k * C_{n-1} < C_i, the last document when there is none, and from there the nearest document at or below with
 *                        w_i > 0.
 *   without replacement  V rounds of arg-max over key_i = log-weight_i + gumbel(u_i), order (key descending, index ascending): the law of
 *                        torch.multinomial(replacement=False), with no weight that can underflow (gumbel as in ptr_pl_sample).
 *   positives            the V largest of P uniform keys, (key descending, index ascending): V distinct documents of 0 .. P-1, the law of
 *                        randperm(P)[:V].
 * ptr_irgan_sample — the documents both players train on.  S = samples per query, 1 .. PTR_IRGAN_MAX_SAMPLES.  Writes pos_idx, neg_idx int64
 *   [B,S] (0 beyond the valid count) and nsel int32 [B] = V.  unif [B,2,L]: stream 0, index i = the key of positive i; stream 1 = the
 *   negatives, index k = draw k (with replacement) or index i = document i (without).  z = preds / T.
 *   PTR_IRGAN_POINT_D   V = min(P, S); neg_idx: V i.i.d. draws with replacement, w_i = exp(z_i - max z) over the n documents
 *                       (irgan_point.py:130-146)
 *   PTR_IRGAN_PAIR_D    V = min(P, n - P, S); neg_idx: V draws without replacement, log-weight z_i, documents i >= P only (irgan_pair.py:140-161)
 *   PTR_IRGAN_PAIR_G    V as PAIR_D; neg_idx: V draws without replacement, log-weight log sigmoid(z_i), all n documents (irgan_pair.py:207-211)
 *   A list with a NaN score gets nsel = 0.
 * ptr_irgan_point_gen_fwd_bwd — the generator step of IRGAN_Point (irgan_point.py:184-217), sampling, loss and gradient in one launch.
 *   p = softmax(g_preds / T), q_i = (1 - lambda) p_i + [i < P] lambda / P; K = draws_per_pos * P documents i.i.d. from q by the inverse CDF on
 *   w_i = (1 - lambda) e_i + [i < P] lambda Z / P (e_i = exp(z_i - max z), Z = sum e), draw k from stream k / L, index k % L (unif
 *   [B, draws_per_pos, L]); c_i = the times i was drawn; r_i = 2 (d_preds_i - 0.5) with d_preds [B,L] the discriminator's outputs;
 *   loss_q = -(1/K) sum_i c_i r_i log p_i p_i / q_i (log p the log-softmax; the importance weight p / q carries gradient, as in the reference);
 *   with a_i = [i < P] lambda / P and h_i = -(1/K) c_i r_i (p_i / q_i) (1 + log p_i a_i / q_i):  grad_j = (h_j - p_j sum_i h_i) / T.
 *   Outputs: loss_q [B], valid_q [B] (1.0 where the query trained), grad [B,L] (0 on padding), loss_out [1] = sum of loss_q (nullable),
 *   counts int32 [B,L] (nullable).  P = 0 or n = 0: loss 0, gradient 0, valid 0 (the reference `continue`s), whatever the scores.  A NaN
 *   score in g_preds of a list with P > 0: the loss and every real gradient entry of that list are NaN, valid 1, counts 0 (the reference
 *   stops training there).
 * ptr_irgan_sel_fwd_bwd — the losses on selected documents, loss and gradient in one launch.  nsel int32 [B] = V (clamped to 0 .. S).
 *   The discriminator's forms take x = its predictions on the compact batch [B,2S], positives in columns 0 .. V-1, negatives in V .. 2V-1,
 *   and write grad [B,2S]; d_sel, neg_idx, lens and L are not read (L >= 1):
 *   PTR_IRGAN_SEL_POINT_D     BCEWithLogits against labels 1 | 0, the mean over 2 V (irgan_point.py:161-169), softplus evaluated stably
 *   PTR_IRGAN_SEL_PAIR_D_SVM  mean max(0, 1 - (d_pos - d_neg)) (irgan_pair.py:182); at 1 - (d_pos - d_neg) == 0 half the gradient, as torch.max
 *   PTR_IRGAN_SEL_PAIR_D_LOG  -mean log sigmoid(d_pos - d_neg), through log-sigmoid (:184)
 *   The generator's forms take x = g_preds [B,L], neg_idx [B,S] and d_sel [B,2S] (the discriminator's predictions, laid out as above), form
 *   reward_k = sigmoid(max(0, 1 - (d_pos_k - d_neg_k))) (SVM) or log sigmoid(d_neg_k - d_pos_k) (LOG) (irgan_pair.py:39-42) and
 *   loss_q = -mean_k log sigmoid(g_neg_k / T) reward_k (:216-218); grad [B,L] is non-zero at the named documents only (each named once; an
 *   index outside 0 .. n-1 names nothing):
 *   PTR_IRGAN_SEL_PAIR_G_SVM, PTR_IRGAN_SEL_PAIR_G_LOG
 *   Outputs loss_q [B], valid_q [B], loss_out [1] (nullable).  nsel = 0: loss 0, gradient 0, valid 0.
 * Forms (ptr_launch_form): lists of up to 256 documents one wavefront per query, four queries per workgroup; longer lists one workgroup of
 * 256 threads per query; the discriminator's forms of ptr_irgan_sel_fwd_bwd always one wavefront.  LDS per query: 8 (sample), 12 (generator)
 * or 4 (selected) bytes x round_up(L, 4).  No floating-point atomics; the draw counts are integer LDS atomics.  A query's bits depend on
 * (its data, L, the parameters, seed, q0 + q) alone.
 * PTR_ERR_INVALID_ARG (before any HIP call): B < 0, L <= 0, L > PTR_MAX_LIST_LEN, S outside 1 .. PTR_IRGAN_MAX_SAMPLES, temperature <= 0,
 * infinite or NaN, a mode out of range, lambda outside [0, 1), draws_per_pos outside 1 .. PTR_IRGAN_MAX_DRAWS_PER_POS, and with B > 0 a NULL
 * required pointer (lens, unif, loss_out, counts are optional; d_sel and neg_idx only for the generator's forms). */
#define PTR_IRGAN_MAX_SAMPLES 64
#define PTR_IRGAN_MAX_DRAWS_PER_POS 64
#define PTR_IRGAN_POINT_D 0
#define PTR_IRGAN_PAIR_D 1
#define PTR_IRGAN_PAIR_G 2
#define PTR_IRGAN_SEL_POINT_D 0
#define PTR_IRGAN_SEL_PAIR_D_SVM 1
#define PTR_IRGAN_SEL_PAIR_D_LOG 2
#define PTR_IRGAN_SEL_PAIR_G_SVM 3
#define PTR_IRGAN_SEL_PAIR_G_LOG 4
int ptr_irgan_sample(const float *preds, const int32_t *lens, const int32_t *num_pos, int B, int L, int S, int mode, float temperature,
                     uint64_t seed, int64_t q0, const float *unif, int64_t *pos_idx, int64_t *neg_idx, int32_t *nsel, void *stream);
int ptr_irgan_point_gen_fwd_bwd(const float *g_preds, const float *d_preds, const int32_t *lens, const int32_t *num_pos, int B, int L,
                                float temperature, float lambda, int draws_per_pos, uint64_t seed, int64_t q0, const float *unif,
                                float *loss_out, float *loss_q, float *valid_q, float *grad, int32_t *counts, void *stream);
int ptr_irgan_sel_fwd_bwd(const float *x, const float *d_sel, const int64_t *neg_idx, const int32_t *nsel, const int32_t *lens, int B, int L,
                          int S, int mode, float temperature, float *loss_out, float *loss_q, float *valid_q, float *grad, void *stream);

/* ---- The adversarial frame's IRFGAN point and pair machines (csrc/irfgan.hip): the f-divergence generalisation of the block above.  The
 * three symbols below are ADDITIVE to ABI v8 as well: PTR_ABI_VERSION stays 8, and no entry point or mode above changes.
 * Reference: ptranking/ltr_adversarial/pointwise/irfgan_point.py, pairwise/irfgan_pair.py, util/pair_sampling.py, util/f_divergence.py, one
 * query per step there, with an n x n Bradley-Terry matrix, an n x n Bernoulli mask and a P x n weight matrix per query; here a padded
 * batch [B,L] with lens and num_pos (as above: clamped to 0 .. lens; n = lens[q], P = num_pos[q]) and nothing of size n x n.  Uniforms:
 * u(seed, q0 + q, stream, index) of ptr_pl_uniforms.  S = samples per query, 1 .. PTR_IRGAN_MAX_SAMPLES.
 * ptr_irfgan_point_sample (irfgan_point.py:179-192): V = min(P, S); pos_idx the V largest of P uniform keys (stream 0, index i), as
 *   ptr_irgan_sample; neg_idx V draws WITHOUT replacement from softmax(preds) (no temperature) over all n documents: V rounds of arg-max
 *   over preds_i + gumbel(u(1, i)).  A list with a NaN score or P = 0 gets nsel = 0.  Writes pos_idx, neg_idx int64 [B,S] (0 beyond V), nsel
 *   int32 [B].  unif (nullable) [B,2,L] replaces the hash.
 * ptr_irfgan_pair_sample (pair_sampling.py:26-77, :111-122; irfgan_pair.py:112-130): preds, labels [B,L], every list sorted by label
 *   descending, labels >= 0 (the caller's duty).
 *   True pairs: S draws WITH replacement from w_ij = max(0, y_i - y_j) / (log2(2 + i) log2(2 + j)), i < P, j < n, by the inverse CDF in
 *   row-major order: draw k takes x = u(0, k) W, W the sum of all w; the head is the first row whose running row sum exceeds x (the
 *   with-replacement rule above on the row sums), the tail the first column of that row with w > 0 whose in-row prefix exceeds the remainder.
 *   Fake pairs: b_ij = [u(2 + i, j) < sigmoid(s_i - s_j)] for all n x n pairs, the diagonal included; M = the number of set bits; S draws
 *   WITH replacement, uniform over the set bits: draw k takes r = min(M - 1, floor(floor(u(1, k) 2^24) M / 2^24)), in integers, and names
 *   the r-th set bit in row-major order.  From the comparisons on, integer arithmetic: the draws depend on the bits alone.
 *   nsel = S for a usable list; nsel = 0 (and no pair named) for n = 0, a NaN score, equal first and last label (the reference's
 *   num_unique_labels < 2), W = 0, M = 0.  Writes true_head, true_tail, fake_head, fake_tail int64 [B,S] (0 beyond nsel), nsel int32 [B]
 *   and bern_count int32 [B] (nullable) = M where the mask was counted, else 0.  The parity route: unif_draw (nullable) [B,2,S] replaces
 *   streams 0 and 1, unif_bern (nullable) [B,L,L] replaces streams 2 .. L+1 — the one thing of size L x L, for tests only.
 * ptr_irfgan_fwd_bwd (irfgan_point.py:200-220, irfgan_pair.py:141-170): both players' losses and gradients, one launch.  With
 *   a(v) = activation_f(v) and c(v) = conjugate_f(activation_f(v)) of util/f_divergence.py, c in CLOSED form:
 *     f_div           a(v)                    c(v)
 *     PTR_FDIV_TVAR   0.5 tanh v              0.5 tanh v
 *     PTR_FDIV_KL     v                       exp(v - 1)
 *     PTR_FDIV_RKL    -exp(-v)                v - 1
 *     PTR_FDIV_PC     v                       0.25 v^2 + v
 *     PTR_FDIV_NC     1 - exp(-v)             2 - 2 exp(-v / 2)
 *     PTR_FDIV_SH     1 - exp(-v)             expm1(v)
 *     PTR_FDIV_JS     log 2 - softplus(-v)    softplus(v) - log 2
 *     PTR_FDIV_GAN    -softplus(-v)           softplus(v)
 *   (softplus evaluated stably, 1 - exp through expm1).  nsel int32 [B] = V (clamped to 0 .. S).
 *   PTR_IRFGAN_POINT_D   x = the discriminator's predictions on the compact batch [B,2S], true documents in columns 0 .. V-1, fake in
 *                        V .. 2V-1; loss_q = mean_k c(x_fake,k) - mean_k a(x_true,k); grad [B,2S].  d_fake, idx_a, idx_b, lens, L unread.
 *   PTR_IRFGAN_PAIR_D    x [B,4S] = true heads | true tails | fake heads | fake tails, each V wide, v = head - tail; the same loss;
 *                        grad [B,4S], +g at a head and -g at its tail.
 *   PTR_IRFGAN_POINT_G   x = g_preds [B,L], idx_a [B,S] the fake documents, d_fake [B,S] the discriminator's eval-mode predictions on them
 *                        (constants): loss_q = -(1/V) sum_k log softmax(x)[idx_k] c(d_k), the log-softmax over the n real documents;
 *                        grad_i = -(1/V) (sum_{k: idx_k = i} c_k - p_i sum_k c_k).
 *   PTR_IRFGAN_PAIR_G    x = g_preds, idx_a / idx_b [B,S] the fake heads / tails, d_fake [B,2S] = heads | tails, each V wide,
 *                        v_k = d_head - d_tail: loss_q = -(1/V) sum_k log sigmoid(x_h - x_t) c(v_k), through log-sigmoid.  Pairs may repeat
 *                        and h = t occurs; every document's thread sums its shares in k order (no atomics).
 *   An index outside 0 .. n-1 names nothing (PAIR_G: the pair).  Outputs loss_q [B], valid_q [B], loss_out [1] (nullable), grad (0 on
 *   padding).  nsel = 0: loss 0, gradient 0, valid 0.  A non-finite x or d_fake propagates as in IEEE arithmetic.
 * Forms (ptr_launch_form): as for the IRGAN entry points — the samplers and the generator's modes one wavefront per query up to 256
 * documents, four queries per workgroup, one workgroup of 256 threads per query beyond; the discriminator's modes always one wavefront.
 * LDS per query: 4 (point sampler) or 16 (pair sampler) bytes x round_up(L, 4); the losses 768 bytes or 4 bytes per column of x.  No
 * atomics.  A query's bits depend on (its data, L, S, the parameters, seed, q0 + q) alone, and the samplers' also not on the form.
 * PTR_ERR_INVALID_ARG (before any HIP call): B < 0, L <= 0, L > PTR_MAX_LIST_LEN, S outside 1 .. PTR_IRGAN_MAX_SAMPLES, a mode or f_div out
 * of range, and with B > 0 a NULL required pointer (lens, unif*, bern_count, loss_out are optional; d_fake and idx_a only for the
 * generator's modes, idx_b only for PTR_IRFGAN_PAIR_G). */
#define PTR_IRFGAN_POINT_D 0
#define PTR_IRFGAN_PAIR_D 1
#define PTR_IRFGAN_POINT_G 2
#define PTR_IRFGAN_PAIR_G 3
#define PTR_FDIV_TVAR 0
#define PTR_FDIV_KL 1
#define PTR_FDIV_RKL 2
#define PTR_FDIV_PC 3
#define PTR_FDIV_NC 4
#define PTR_FDIV_SH 5
#define PTR_FDIV_JS 6
#define PTR_FDIV_GAN 7
int ptr_irfgan_point_sample(const float *preds, const int32_t *lens, const int32_t *num_pos, int B, int L, int S, uint64_t seed, int64_t q0,
                            const float *unif, int64_t *pos_idx, int64_t *neg_idx, int32_t *nsel, void *stream);
int ptr_irfgan_pair_sample(const float *preds, const float *labels, const int32_t *lens, const int32_t *num_pos, int B, int L, int S,
                           uint64_t seed, int64_t q0, const float *unif_draw, const float *unif_bern, int64_t *true_head, int64_t *true_tail,
                           int64_t *fake_head, int64_t *fake_tail, int32_t *nsel, int32_t *bern_count, void *stream);
int ptr_irfgan_fwd_bwd(const float *x, const float *d_fake, const int64_t *idx_a, const int64_t *idx_b, const int32_t *nsel, const int32_t *lens,
                       int B, int L, int S, int mode, int f_div, float *loss_out, float *loss_q, float *valid_q, float *grad, void *stream);

/* ---- The adversarial frame's list machines, IRGAN_List and IRFGAN_List (csrc/adlist.hip): the rankings the discriminator trains on and both
 * players' ranking-probability losses.  The two symbols below are ADDITIVE to ABI v8 as well: PTR_ABI_VERSION stays 8, nothing above changes.
 * Reference: ptranking/ltr_adversarial/listwise/irgan_list.py:24-409, listwise/irfgan_list.py:20-393, util/list_probability.py,
 * util/list_sampling.py:16-36 (gumbel_softmax), :70-87 (arg_shuffle_ties) — one query per step there, a Python loop of gathers, one
 * torch.randperm per sample, an [S,K,K] Bradley-Terry matrix and autograd through softmax, sort and LogCumsumExp; here a padded batch
 * [B,L] with lens, one sampling launch and one fused loss launch per player, nothing of size K x K stored.
 * Notation: n = lens[q]; S = samples per query, 1 .. PTR_IRGAN_MAX_SAMPLES; K = top_k, K <= 0 the whole list; Kq = min(K, n), or n for the
 * whole list (the reference's [0:top_k] slice of a shorter list gives n); Kw = K, or L for the whole list.  Uniforms are
 * u(seed, q0 + q, stream, index) of ptr_pl_uniforms, gumbel(u) as in ptr_pl_sample.
 * ptr_adlist_sample (irgan_list.py:230-276) — one launch, top-Kq only.  preds, labels [B,L].
 *   gen_idx[q,s,0..Kq-1] = the first Kq documents in the order (preds_i + gumbel(u(s, i)) descending, index ascending), stream s in
 *   0 .. S-1: the streams of ptr_pl_sample(..., PTR_PL_DIST_STPL), whose perm it is the prefix of, bit for bit, for equal (seed, q0).  The
 *   temperature is a positive scale and does not enter the order: no parameter here.
 *   std_idx[q,s,0..Kq-1] = the first Kq documents in the order (label descending, u(S + s, i) descending, index ascending): uniform
 *   among label ties, the law of arg_shuffle_ties(label, descending=True); labels of -1 sort last.
 *   Outputs: std_idx, gen_idx int64 [B,S,Kw], 0 beyond Kq; kq int32 [B] = Kq, and 0 for n = 0 or a list with a NaN score.  unif (nullable)
 *   [B,2S,L] replaces the hash (the parity route).  Nothing of size [B,S,L] is written when K < L.
 * ptr_adlist_fwd_bwd — loss and gradient of either player, one launch.  With v = the scores of a ranking in ranking order:
 *   PTR_ADLIST_PL  lp(v) = sum_{p<Kq} (v_p - L_p), L_p = log sum_{r>=p} e^{v_r} (max-shifted; the two scans run in double, and in the log
 *                  domain in fp32 where a ranking's scores spread over more than 600);
 *                  d lp / d v_r = 1 - e^{v_r} sum_{p<=r} e^{-L_p}                                  (list_probability.py:24-30)
 *   PTR_ADLIST_BT  lp(v) = sum_{p<r} log sigmoid(v_p - v_r), through log-sigmoid: the reference's e_p / (e_p + e_r) with a batch-wide max
 *                  shift is the same number; d lp / d v_p = sum_{r>p} sigmoid(v_r - v_p) - sum_{r<p} sigmoid(v_p - v_r).  A pair loop,
 *                  nothing of size K x K stored                                                     (list_probability.py:44-62)
 *   mode PTR_ADLIST_D: x = the discriminator's scores of the WHOLE list [B,L]; std_idx, gen_idx [B,S,Kw] and kq [B] as the sampler wrote
 *   them (kq clamped to 0 .. min(n, Kw)); d_preds, temperature, seed, q0, unif, reward unread.
 *     PTR_ADLIST_IRGAN   loss_q = -sum_s lp(x[std_s]) - sum_s log(1 - lp(x[gen_s]))                (irgan_list.py:336-337)
 *     PTR_ADLIST_IRFGAN  loss_q = mean_s c(lp(x[gen_s])) - mean_s a(lp(x[std_s])), f_div one of PTR_FDIV_*, a and c in the closed forms of
 *                        ptr_irfgan_fwd_bwd                                                         (irfgan_list.py:322)
 *     grad [B,L]: the shares of a document are summed over the samples in a fixed order, no floating-point atomics.  A ranking names
 *     a document at most once (the sampler's do); an index outside 0 .. n-1 makes its query invalid (loss 0, gradient 0, valid 0).
 *   mode PTR_ADLIST_G: x = the generator's scores [B,L]; d_preds [B,L] = the discriminator's eval-mode scores, constants; std_idx,
 *   gen_idx, kq unread.  The kernel draws the S rankings itself from (seed, q0), streams 0 .. S-1, or from unif [B,S,L]:
 *     y^s = softmax_i((x_i + gumbel_{s,i}) / T) over the n documents, through the log-softmax (normaliser in double); pi_s = the descending order of the key
 *     x_i + gumbel_{s,i} (the order of the logit); A_s = lp_PL of the Kq largest probabilities — the PL of the PROBABILITIES, as the
 *     reference takes it (irgan_list.py:379); R_s = the reward from lp(d_preds[pi_s(0..Kq-1)]) under `prob`:
 *     PTR_ADLIST_IRGAN   loss_q = (1/S) sum_s A_s R_s, R_s by `reward` (get_reward, irgan_list.py:301-310):
 *                        PTR_ADLIST_REWARD_NEG_EXP -exp(lp) | _NEG_LP -lp | _EXP_1M exp(1 - lp) | _LOG_1M log(1 - lp)
 *     PTR_ADLIST_IRFGAN  loss_q = -(1/S) sum_s A_s c(lp)                                            (irfgan_list.py:295, :375)
 *     With h^s_i = d A_s / d y_i (zero outside the top Kq): grad_j = (1/S) sum_s R_s y^s_j (h^s_j - sum_i y^s_i h^s_i) / T, the sign as
 *     the family's loss.  gen_idx_out (nullable) int64 [B,S,Kw] = ptr_adlist_sample's gen_idx for the same (seed, q0).  Kq = 0 for a list
 *     with a NaN score in x.
 *   Outputs: loss_q [B], valid_q [B], loss_out [1] = sum of loss_q (nullable), grad [B,L] (0 on padding).  Kq = 0: loss 0, gradient 0,
 *   valid 0.  n = 1 is valid: lp = 0 and the gradient is 0; the loss is 0 in every mode except PTR_ADLIST_D under PTR_ADLIST_IRFGAN,
 *   where it is the constant c(0) - a(0) of the divergence (exp(-1) under KL, 2 log 2 under GAN, 0 otherwise), as in the reference.
 *   Non-finite values propagate as in IEEE arithmetic: exp(1 - lp) (PTR_ADLIST_REWARD_EXP_1M) overflows fp32 once lp < -87.7, i.e. for
 *   long rankings, in the reference too.
 * Forms (ptr_launch_form): as the IRGAN entry points — up to 256 documents one wavefront per query, four queries per workgroup; beyond,
 * one workgroup of 256 threads per query.  LDS per query: 8 bytes x round_up(L, 4) (sampler), 8 bytes x round_up(L, 4) + 24 bytes x
 * round_up(min(Kw, L), 4) (losses).  A query's bits depend on (its data, L, S, K, the parameters, seed, q0 + q) alone; the sampler's are
 * integer counts of exact comparisons and do not depend on the form either.
 * PTR_ERR_INVALID_ARG (before any HIP call): B < 0, L <= 0, L > PTR_MAX_LIST_LEN, S outside 1 .. PTR_IRGAN_MAX_SAMPLES, top_k >
 * PTR_MAX_LIST_LEN, temperature <= 0, infinite or NaN, a mode, prob, family, reward or f_div out of range, and with B > 0 a NULL required
 * pointer (lens, unif, loss_out, gen_idx_out are optional; d_preds only for PTR_ADLIST_G; std_idx, gen_idx, kq only for PTR_ADLIST_D). */
#define PTR_ADLIST_D 0
#define PTR_ADLIST_G 1
#define PTR_ADLIST_PL 0
#define PTR_ADLIST_BT 1
#define PTR_ADLIST_IRGAN 0
#define PTR_ADLIST_IRFGAN 1
#define PTR_ADLIST_REWARD_NEG_EXP 0
#define PTR_ADLIST_REWARD_NEG_LP 1
#define PTR_ADLIST_REWARD_EXP_1M 2
#define PTR_ADLIST_REWARD_LOG_1M 3
int ptr_adlist_sample(const float *preds, const float *labels, const int32_t *lens, int B, int L, int S, int top_k, uint64_t seed, int64_t q0,
                      const float *unif, int64_t *std_idx, int64_t *gen_idx, int32_t *kq, void *stream);
int ptr_adlist_fwd_bwd(const float *x, const float *d_preds, const int64_t *std_idx, const int64_t *gen_idx, const int32_t *kq,
                       const int32_t *lens, int B, int L, int S, int top_k, int mode, int prob, int family, int reward, int f_div,
                       float temperature, uint64_t seed, int64_t q0, const float *unif, float *loss_out, float *loss_q, float *valid_q,
                       float *grad, int64_t *gen_idx_out, void *stream);

/* Device tie-shuffled label-descending order (the role of arg_shuffle_ties, sampling_utils.py:13-28) from a
 * counter-based RNG: same distribution, NOT the torch.randperm stream (not parity-checked, statistically tested). */
int ptr_shuffle_ties_order(const float *labels, const int32_t *lens, int B, int L, uint64_t seed, int64_t *perm,
                           void *stream);

/* torch.sort(preds, dim=1, descending=True) as ptranking/base/ranker.py:50 and lambdarank.py:39 call it:
 * vals[B,L] fp32, idx[B,L] int64; order = (value descending, original index ascending); padded tail: 0 / identity.
 * NaN scores sort FIRST (ahead of +inf), among themselves by original index — torch.sort(descending=True, stable=True); -0.0 and +0.0
 * compare equal.  idx is a permutation of [0, lens[q]) on every input. */
int ptr_sort_desc(const float *preds, const int32_t *lens, int B, int L, float *vals, int64_t *idx, void *stream);

/* Evaluator prologue + metrics — replaces ptranking/base/ranker.py:46-60,220-243 (sort, gather, ideal sort) and
 * ptranking/metric/adhoc/adhoc_metric.py:36-62 (P@ks), :91-123 (AP@ks), :127-193 (nERR@ks), :219-260 (nDCG@ks).
 *   ks: HOST int32[nk] cut-offs (nk <= PTR_MAX_CUTOFFS); presort != 0 => labels already ideal-ordered;
 *   max_label: nERR's 2^max_label normaliser; < 0 => the batch maximum is computed on device into max_label_ws[1];
 *   label_type: PTR_LABEL_* (nDCG's gain, adhoc_metric.py:207-212; nERR exists for MultiLabel only, as in the reference);
 *   ndcg/nerr/ap/prec: [B,nk] outputs, each nullable.  Cut-offs larger than the list are zero-filled at the END
 *   of the row exactly like the reference's padded_*_at_ks.
 *   The predicted ranking is ptr_sort_desc's: a NaN score ranks first (index ascending among NaNs), as torch.sort has it.  A list
 *   without a relevant document gives nDCG = nERR = AP = NaN (0 / 0, as the reference) and P = 0 at every fitting cut-off. */
#define PTR_LABEL_MULTILABEL 0    /* LABEL_TYPE.MultiLabel: graded labels, DCG gain 2^l - 1 (data_utils.py:120-126)          */
#define PTR_LABEL_PERMUTATION 1   /* LABEL_TYPE.Permutation: labels = n - rank position, DCG gain = the label itself        */
int ptr_metrics_at_ks(const float *preds, const float *labels, const int32_t *lens, int B, int L, const int32_t *ks,
                      int nk, int presort, int label_type, float max_label, float *max_label_ws, float *ndcg, float *nerr,
                      float *ap, float *prec, void *stream);

/* Deterministic sum of n floats (fixed reduction tree): out[0] = scale * sum(x).  Used for the per-query loss slots
 * and for Evaluator running sums. */
int ptr_sum_f32(const float *x, int n, float scale, float *out, void *stream);

/* ---- pointwise MLP scorer (`pointsf`) --------------------------------------------------------------------------------
 * Replaces ptranking/base/point_ranker.py:45-55 (forward of the stacked feed-forward scorer built by
 * ptranking/base/utils.py:288-356 with AF='R', BN=False, apply_tl_af=False: (Dropout -> Linear -> ReLU) x NL -> Linear), its
 * autograd backward, and the Adam update of ptranking/base/ranker.py:512-525.  Hidden width is 100 (point_ranker.py:30).
 * `params` / `grad` are ONE flat fp32 buffer in PyTorch's own order and layouts:
 *   W1[100][F] b1[100] | W2[100][100] b2[100] | ... (NL hidden layers) | w_out[100] b_out[1]      (ptr_mlp_num_params floats)
 * X is [R][F] row-major (R = B*L documents), preds [R].  train != 0: dropout p_drop from the counter-based generator
 * seeded by `seed`, and the post-dropout activations needed by backward are written to `acts`: ptr_mlp_acts_floats(R, NL) floats,
 * opaque to the caller (ABI v4: TILE-MAJOR [NL][ceil(R / 16)][7][16][16] — every block of 16 rows x 16 of the PTR_MLP_ACT_LD = 112
 * padded features is one contiguous KB, the unit a forward store instruction writes and a backward LDS-DMA piece reads; element
 * (layer, row, col) at layer * ceil16(R) * 112 + (row / 16) * 1792 + (col / 16) * 256 + (row % 16) * 16 + col % 16).
 * SIZE IT WITH ptr_mlp_acts_floats(R, NL): the forward writes WHOLE 16-row tiles, so a buffer allocated as the pre-v4 [NL][R][112] is up to
 * 15 rows per layer too small whenever R % 16 != 0 (an out-of-bounds write).
 * ptr_mlp_backward: dpreds [R] -> grad (every entry overwritten); ws (ptr_mlp_backward_ws_floats) and dz (ptr_mlp_backward_dz_floats
 * floats: [NL][R][PTR_MLP_ACT_LD] for the layer-wise kernels, 0 => may be NULL when the single-pass fused backward serves the
 * configuration — NL = 3, F in {132, 136, 140}) are caller-provided scratch; p_drop / seed must be the forward call's.
 * All calls are deterministic. */
size_t ptr_mlp_num_params(int F, int NL);
size_t ptr_mlp_backward_ws_floats(int F, int NL);
size_t ptr_mlp_backward_dz_floats(int R, int F, int NL);
size_t ptr_mlp_acts_floats(int R, int NL);                       /* ABI v4: NL * ceil16(R) * 112 */
int ptr_mlp_forward(const float *X, const float *params, int R, int F, int NL, int train, float p_drop, uint64_t seed,
                    float *preds, float *acts, void *stream);
int ptr_mlp_backward(const float *X, const float *params, const float *acts, const float *dpreds, int R, int F, int NL,
                     float p_drop, uint64_t seed, float *dz, float *ws, float *grad, void *stream);
/* ptr_mlp_backward + the optimiser step + the loss-slot sum in the SAME launches (ABI v2): the partial-gradient reduction applies the
 * update to each element it has just reduced, and one extra block sums loss_q[nq] into loss_out (nullable) exactly like ptr_sum_f32 — for
 * single-device training, where no all-reduce sits between the gradient and the step (ptranking/base/ranker.py:589-603 does
 * backward -> optimizer.step back to back).  `grad` still receives the gradient.  opt_kind / hyper-parameters:
 *   PTR_OPT_ADAM     hyper1 = beta1, hyper2 = beta2, state1 = exp_avg, state2 = exp_avg_sq      (arithmetic of ptr_adam_step)
 *   PTR_OPT_ADAGRAD  hyper1 = lr_decay, state1 = sum, state2 unused                             (ptr_adagrad_step)
 *   PTR_OPT_RMSPROP  hyper1 = alpha, state1 = square_avg, state2 unused                          (ptr_rmsprop_step)
 * Results are bit-identical to the separate calls. */
#define PTR_OPT_ADAM 1
#define PTR_OPT_ADAGRAD 2
#define PTR_OPT_RMSPROP 3
int ptr_mlp_backward_step(const float *X, float *params, const float *acts, const float *dpreds, int R, int F, int NL, float p_drop,
                          uint64_t seed, float *dz, float *ws, float *grad, int opt_kind, float lr, float hyper1, float hyper2, float eps,
                          float weight_decay, int step, float *state1, float *state2, const float *loss_q, int nq, float *loss_out,
                          void *stream);
/* ABI v4.  The optimiser step of ptr_mlp_backward_step and its loss-slot sum as ONE launch on a gradient that is already complete — the
 * data-parallel step: ptr_mlp_backward -> RCCL all-reduce of `grad` -> this (no reference counterpart: ptranking is single-device,
 * ptranking/ltr_adhoc/eval/ltr.py:44-48; the step itself is ptranking/base/ranker.py:512-525 + the loss accumulation of :589-603).  Same
 * arithmetic as ptr_mlp_backward_step, bit for bit.  loss_out (optional) = sum of the nq loss slots. */
int ptr_opt_step_loss(float *params, const float *grad, int64_t n, int opt_kind, float lr, float hyper1, float hyper2, float eps,
                      float weight_decay, int step, float *state1, float *state2, const float *loss_q, int nq, float *loss_out, void *stream);
/* torch.optim.Adam step (L2 weight decay added to the gradient, bias correction with `step` >= 1) on flat buffers. */
int ptr_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, void *stream);
/* torch.optim.Adagrad (clr = lr / (1 + (step - 1) lr_decay); sum += g^2; p -= clr g / (sqrt(sum) + eps)) and torch.optim.RMSprop
 * (sq = alpha sq + (1 - alpha) g^2; p -= lr g / (sqrt(sq) + eps); no momentum, not centered) on flat buffers, g = grad + weight_decay p:
 * the 'Adagrad' / 'RMS' choices of ptranking/base/ranker.py:518-521. */
int ptr_adagrad_step(float *param, const float *grad, float *state_sum, int64_t n, float lr, float lr_decay, float eps,
                     float weight_decay, int step, void *stream);
int ptr_rmsprop_step(float *param, const float *grad, float *square_avg, int64_t n, float lr, float alpha, float eps,
                     float weight_decay, void *stream);
/* ---- the same scorer on bf16 matrix instructions with fp32 results (ABI v3, csrc/scorer_x6.hip) ---------------------------------
 * Replaces the same reference code as ptr_mlp_forward (ptranking/base/point_ranker.py:45-55, ptranking/base/utils.py:288-356).
 * Every fp32 operand is split exactly into three bf16 pieces and a product is the sum of the six piece products above 2^-24 (six
 * v_mfma_f32_16x16x32_bf16 with fp32 accumulation per 32-deep slice): results agree with the fp32-MFMA entry points to fp32 rounding
 * (error against float64 equal or lower), the arithmetic type of the path stays fp32.  Same operands and `acts` layout as
 * ptr_mlp_forward; `wimg` is caller-provided scratch of ptr_mlp_x6_ws_bytes(F, NL) bytes (16-byte aligned) that receives the
 * pre-split weight image (rebuilt by every call: the weights change every step).  Served: F % 4 == 0, 2 <= NL <= 8 (ws_bytes returns
 * 0 otherwise and the call fails with PTR_ERR_UNSUPPORTED). */
size_t ptr_mlp_x6_ws_bytes(int F, int NL);
int ptr_mlp_forward_x6(const float *X, const float *params, int R, int F, int NL, int train, float p_drop, uint64_t seed,
                       float *preds, float *acts, void *wimg, void *stream);
/* ---- one train step as ONE call (ABI v5, csrc/train_step.hip) ------------------------------------------------------------------------
 * Replaces ptranking/base/ranker.py:589-603 (`NeuralRanker.train_op`: forward -> custom_loss_function = loss, zero_grad, backward,
 * optimizer.step) for the pointsf scorer (ptranking/base/point_ranker.py:45-55) with one of the single-kernel losses: the SAME three
 * entry points a caller would chain — ptr_mlp_forward[_x6] -> ptr_<loss>_fwd_bwd -> ptr_mlp_backward_step — enqueued from C on
 * `stream`, with the same arguments in the same order, so the parameters after the step are bit-identical to the separate calls.
 * What it removes is the host work between the launches (three foreign-function calls with ~60 marshalled arguments: the step was
 * host-bound below ~1024 queries).  The descriptor is caller-owned and may be kept across steps (only seed / step / lr change).
 *   loss_kind      PTR_LOSS_*; loss_f / loss_i carry that loss's parameters:
 *                    RANKNET, LAMBDARANK  loss_f[0] = sigma
 *                    LAMBDALOSS           loss_i[0] = k, loss_i[1] = loss_type (PTR_LAMBDALOSS_*), loss_i[2] = presort; loss_f[0] = sigma, loss_f[1] = mu
 *                    LISTNET              none
 *   X [B*L][F], labels [B][L], lens [B] or NULL; params / grad / state1 / state2: the flat buffers of ptr_mlp_backward_step
 *   scratch        preds [B*L], acts (ptr_mlp_acts_floats), loss_q [B], dpreds [B*L], ws (ptr_mlp_backward_ws_floats), dz
 *                  (ptr_mlp_backward_dz_floats, NULL when 0), wimg (ptr_mlp_x6_ws_bytes; NULL selects the fp32-MFMA forward)
 *   loss_out [1]   sum of the per-query losses (written by the backward's reduction launch)
 *   wimg_current   with the bf16x6 forward the step is FOUR launches: the optimiser launch also writes the updated weights' bf16 planes into `wimg`
 *                  (bit-identical to what the prep launch of ptr_mlp_forward_x6 would build), so the next step needs no prep launch
 * Errors: the first failing stage's code; ptr_last_error() names the stage's entry point. */
#define PTR_LOSS_RANKNET 1
#define PTR_LOSS_LAMBDARANK 2
#define PTR_LOSS_LAMBDALOSS 3
#define PTR_LOSS_LISTNET 4
typedef struct ptr_train_step_desc {
    int32_t struct_bytes;                 /* sizeof(ptr_train_step_desc): a binding built against another layout is refused */
    int32_t loss_kind;
    int32_t B, L, F, NL;
    int32_t opt_kind, step;
    int32_t loss_i[4];
    float loss_f[4];
    float p_drop, lr, hyper1, hyper2, eps, weight_decay;
    uint64_t seed;
    const float *X, *labels;
    const int32_t *lens;
    float *params, *grad, *state1, *state2;
    float *preds, *acts, *loss_q, *dpreds, *dz, *ws;
    void *wimg;
    float *loss_out;
    void *events[4];                      /* optional hipEvent_t handles (NULL: none) recorded on `stream` in front of the forward, between the stages
                                             and behind the backward: events[0..1] bracket the forward, [1..2] the loss kernel, [2..3] the backward + step
                                             (bench.py times the stages of the product path with them) */
    int32_t wimg_current;                 /* != 0: `wimg` already holds the bf16 planes of `params` (left there by the previous ptr_train_step on these
                                             buffers): the forward skips its prep launch.  The call ALWAYS leaves the image current for the updated
                                             parameters — the optimiser launch rewrites it element by element.  0 when in doubt (first call, parameters or
                                             image touched by anything else in between) */
    int32_t reserved;
} ptr_train_step_desc;
int ptr_train_step(const ptr_train_step_desc *d, void *stream);
/* Test helper: the dropout keep-mask (1.0 / 0.0) of dropout site `site` for an [R][n_feat] activation. */
int ptr_mlp_dropout_mask(int R, int n_feat, int site, float p_drop, uint64_t seed, float *out, void *stream);

/* ---- linear layers of the scoring functions (hand-written fp32-MFMA kernels, csrc/linear.hip) -------------------------------
 * Replace the library GEMMs behind the reference's nn.Linear modules: the stacked feed-forward nets of
 * ptranking/base/utils.py:288-356 (pointsf with any activation / batch norm; the listsf head / tail stacks, ff_dims 128/256/512)
 * and the Q|K|V / fc projections of ptranking/base/list_ranker.py:176-254.  Row-major operands with explicit leading dimensions
 * (so packed buffers such as [R][3F] are read / written in place); W is nn.Linear's [N][K] weight.
 *   ptr_linear_forward          Y[R][N] = epi(X[R][K] W^T + bias)   epi: PTR_LINEAR_NONE | _RELU | _RELU_DROPOUT (ReLU, then the
 *                               NEXT layer's dropout from the counter-based generator (seed, site): the stored value is that
 *                               layer's input and `a > 0` encodes "ReLU active and kept")
 *   ptr_linear_backward_input   dX[R][K] = dY[R][N] W, optionally gated: dX *= [gate > 0] / (1 - p_drop)  (gate = the stored
 *                               _RELU_DROPOUT output of the layer below, NULL = no gate)
 *   ptr_linear_backward_weight  dW[N][K] = dY^T X, db[N] = column sums of dY (NULL = skip); ws = ptr_linear_backward_weight_ws_floats
 *                               floats of scratch; deterministic (fixed-order reduction of row chunks)                          */
#define PTR_LINEAR_NONE 0
#define PTR_LINEAR_RELU 1
#define PTR_LINEAR_RELU_DROPOUT 2
#define PTR_LINEAR_GATE 3          /* internal: the epilogue of ptr_linear_backward_input */
int ptr_linear_forward(const float *X, int ldx, const float *W, const float *bias, int R, int K, int N, int act, float p_drop,
                       uint64_t seed, int site, float *Y, int ldy, void *stream);
int ptr_linear_backward_input(const float *dY, int ldy, const float *W, int R, int K, int N, const float *gate, int ldg, float p_drop,
                              float *dX, int ldx, void *stream);
size_t ptr_linear_backward_weight_ws_floats(int R, int K, int N);
int ptr_linear_backward_weight(const float *X, int ldx, const float *dY, int ldy, int R, int K, int N, float *ws, float *dW, float *db,
                               void *stream);
/* nn.Dropout in front of a stack's first Linear (utils.py:299): out = x * keep(seed, site, row, col) / (1 - p); the backward is the
 * same call on the incoming gradient (the mask is recomputed).  C, ldx, ldo multiples of 4, 16-byte aligned pointers. */
int ptr_dropout_apply(const float *x, int ldx, int R, int C, float p_drop, uint64_t seed, int site, float *out, int ldo, void *stream);
/* out = dy * [y > 0]: backward of a trailing ReLU (the `apply_tl_af` activation of the listsf head stack, list_ranker.py:318). */
int ptr_relu_gate(const float *dy, const float *y, int64_t n, float *out, void *stream);

/* ---- batch normalisation + activation + dropout of the stacked feed-forward nets (csrc/bnact.hip) --------------------------
 * One hidden layer of get_stacked_FFNet (ptranking/base/utils.py:296-315) is Dropout -> Linear -> [LTRBatchNorm] -> AF; the default
 * pointsf (ptranking/ltr_adhoc/eval/parameter.py:145-146) is 5 x [.. -> BN(affine) -> GELU] -> Linear -> BN -> Sigmoid.  Around
 * ptr_linear_*:  ptr_bn_stats = LTRBatchNorm's batch statistics (utils.py:201-223: BatchNorm1d without running statistics — batch
 * statistics in training and evaluation, biased variance, two-pass), ptr_bnact_forward = dropout_next(AF(gamma * xhat + beta)),
 * ptr_bnact_backward = the backward of all three (dropout mask and activation derivative recomputed from the stored
 * pre-normalisation z; BatchNorm's two column sums reduced in a fixed order), also yielding dgamma / dbeta.
 * Activations = the working entries of get_AF (utils.py:100-143).  mean == NULL: no batch norm; gamma / beta NULL: no affine. */
#define PTR_AF_NONE 0
#define PTR_AF_RELU 1      /* 'R'  */
#define PTR_AF_LEAKY 2     /* 'LR' */
#define PTR_AF_ELU 3       /* 'E' and 'CE' (alpha = 1) */
#define PTR_AF_SELU 4      /* 'SE' */
#define PTR_AF_GELU 5      /* 'GE' (erf form) */
#define PTR_AF_SIGMOID 6   /* 'S'  */
#define PTR_AF_TANH 7      /* 'T'  */
/* group_rows: 0 = statistics over all R rows (LTRBatchNorm 'BN'); L > 0 = per group of L consecutive rows, i.e. per query (LTRBatchNorm2
 * 'BN2', utils.py:227-286; R % L == 0) — mean / rstd then are [R / L][N]. */
/* lens / rows_per_query (ABI v2; lens nullable): PADDED query batches.  Row r of the [B * rows_per_query] rows is a
 * real document iff (r % rows_per_query) < lens[r / rows_per_query]; only real rows enter the statistics (mean / variance, and the two
 * column sums of the backward, divided by the number of REAL rows — of the batch for 'BN', of the query for 'BN2'), and a padded row's dz
 * is 0, so a padded batch scores and trains exactly like the unpadded lists (the reference batches equal-length lists only,
 * data_utils.py:683-742, so its LTRBatchNorm never sees a padded row).  group_rows > 0 requires group_rows == rows_per_query. */
size_t ptr_bn_ws_floats(int R, int N, int group_rows);
int ptr_bn_stats(const float *z, int ld, int R, int N, int group_rows, const int32_t *lens, int rows_per_query, float eps, float *ws,
                 float *mean, float *rstd, void *stream);
int ptr_bnact_forward(const float *z, int ld, int R, int N, int group_rows, const int32_t *lens, int rows_per_query, const float *mean,
                      const float *rstd, const float *gamma, const float *beta, int af, float p_drop, uint64_t seed, int site, float *out,
                      void *stream);
/* ws: ptr_bn_ws_floats(R, N, group_rows) floats (only read / written with batch norm); dgamma / dbeta: sums over all REAL rows */
int ptr_bnact_backward(const float *z, const float *da, int ld, int R, int N, int group_rows, const int32_t *lens, int rows_per_query,
                       const float *mean, const float *rstd, const float *gamma, const float *beta, int af, float p_drop, uint64_t seed,
                       int site, float *ws, float *dz, float *dgamma, float *dbeta, void *stream);

/* ---- synchronised 'BN' statistics across data-parallel ranks (ABI v7) ---------------------------------------------------------------
 * The whole-batch statistics of ptr_bn_stats and the backward of ptr_bnact_backward, cut where the ranks must talk.  W ranks hold R_w
 * rows each; between the calls the host gathers one fixed-size record per rank (dp.gather_slots), so every rank runs the second half
 * on identical bytes and gets identical statistics whatever the collective backend's reduction order.  group_rows must be 0 in all
 * four (per-query 'BN2' statistics couple no ranks: PTR_ERR_INVALID_ARG); lens / rows_per_query as above; an empty shard (R == 0) is an
 * error, a shard whose rows are all padding is not.
 *   forward   ptr_bn_stats_partial -> gather slots -> ptr_bn_stats_combine -> ptr_bnact_forward(mean, rstd)
 *   backward  ptr_bnact_backward_sums -> gather sums -> ptr_bnact_backward_apply
 * slot  = ptr_bn_slot_floats(N) = 2 N + 4 floats: [ mean[N] | M2[N] | count | 3 unused ] — the mean and the sum of squared deviations
 *         from it of this rank's real rows, and how many they are (0: mean and M2 are 0).  Counts travel as floats: exact while the
 *         ranks hold fewer than 2^24 = 16 777 216 real rows IN TOTAL.
 * combine: mean = sum n_w mean_w / n, var = sum (M2_w + n_w (mean_w - mean)^2) / n (biased), rstd = 1 / sqrt(var + eps), n = sum n_w;
 *         slots taken in rank order 0 .. W-1 (up to 32 ranks: one addition per rank in that order; beyond, ranks w, w + 32, ... are
 *         pre-added — a fixed order either way, no atomics); a slot with count 0 has weight 0 and contributes exactly nothing.
 *         total_count[0] = max(n, 1) stays on the device for ptr_bnact_backward_apply.
 * sums  = 2 N floats: [ sum dy [N] | sum dy xhat [N] ] over this rank's real rows, xhat from the GLOBAL mean / rstd — these are this
 *         rank's dbeta | dgamma (the gradient all-reduce adds them across ranks like every other parameter gradient).
 * apply:  sums[W][2 N] (the gathered records) are added in the same fixed rank order into ws[2 N], then
 *         dz = gamma rstd (dy - sum_dy / n - xhat sum_dyx / n) with n read from total_count; a padded row's dz is 0. */
size_t ptr_bn_slot_floats(int N);
/* ws: ptr_bn_ws_floats(R, N, 0) floats */
int ptr_bn_stats_partial(const float *z, int ld, int R, int N, int group_rows, const int32_t *lens, int rows_per_query, float *ws,
                         float *slot, void *stream);
/* slots: W records, slot_stride (>= 2 N + 1) floats apart */
int ptr_bn_stats_combine(const float *slots, int W, int slot_stride, int N, float eps, float *mean, float *rstd, float *total_count,
                         void *stream);
/* ws: ptr_bn_ws_floats(R, N, 0) floats */
int ptr_bnact_backward_sums(const float *z, const float *da, int ld, int R, int N, int group_rows, const int32_t *lens, int rows_per_query,
                            const float *mean, const float *rstd, const float *gamma, const float *beta, int af, float p_drop,
                            uint64_t seed, int site, float *ws, float *sums, void *stream);
/* ws: 2 N floats (the global sums) */
int ptr_bnact_backward_apply(const float *z, const float *da, int ld, int R, int N, int group_rows, const int32_t *lens, int rows_per_query,
                             const float *mean, const float *rstd, const float *gamma, const float *beta, int af, float p_drop,
                             uint64_t seed, int site, const float *sums, int W, const float *total_count, float *ws, float *dz,
                             void *stream);

/* ---- listsf: the permutation-equivariant scorer's fused pieces (fp32 MFMA attention core, the reference's LayerNorm) ----
 * ptr_mhsa_forward replaces ptranking/base/list_ranker.py:216-240 (Q K^T / sqrt(d_h) -> softmax -> Dropout -> . V, heads = column
 * blocks of width F / n_heads of the [B][L][F] projections Q, K, V; the output O has the same layout, i.e. what
 * `x.permute(0,2,1,3).contiguous().view(bsz,-1,F)` yields at :243-247).  Nothing of size L^2 is written: lse [B*H*L] (log-sum-exp
 * of every score row) is the only side output and lets ptr_mhsa_backward recompute the probabilities.
 * lens (nullable): keys >= lens[b] are excluded from the softmax (padded batches; the reference has no padding).
 * p_drop > 0: dropout on the attention probabilities from the counter generator (seed, site, b, h, row, key); p_drop = 0: eval.
 * ptr_mhsa_backward: dO [B][L][F] -> dQ, dK, dV [B][L][F] (every element written); dvec [B*H*L] is scratch; O, lse, p_drop,
 * seed, site must be the forward call's.  Head dimension F / n_heads <= PTR_MHSA_MAX_HEAD_DIM.
 * ld_qkv = row stride in floats of Q, K, V (and dQ, dK, dV): F for three separate tensors, 3F when they are the column blocks
 * of ONE packed [B][L][3F] projection (pass base, base + F, base + 2F) — one GEMM then produces all three and dQ|dK|dV is
 * directly the gradient of that projection.  O, dO are always [B][L][F].
 * Heads up to 128 wide run the kernels that keep the whole head in registers (csrc/listsf.hip); heads of 129 .. PTR_MHSA_MAX_HEAD_DIM
 * (352 = 22 column tiles of 16: the reference's 2-head default on the 700 Yahoo! features is 350) run the wide forms
 * (csrc/listsf_wide.hip: one workgroup per CU, one operand of head width per wave in registers).  Same contract, same dropout masks; wider heads are refused
 * with PTR_ERR_UNSUPPORTED. */
#define PTR_MHSA_MAX_HEAD_DIM 352
int ptr_mhsa_forward(const float *Q, const float *K, const float *V, int ld_qkv, const int32_t *lens, int B, int L, int F,
                     int n_heads, float p_drop, uint64_t seed, int site, float *O, float *lse, void *stream);
/* ds_ws (ABI v2, nullable): B * n_heads * L * L floats of scratch.  When given, the dK / dV kernel stores the scaled dS it forms and the dQ
 * kernel is ONE GEMM unit dS . K instead of recomputing S = Q K^T and dP = dO V^T (7 -> 5 GEMM units for the backward, at 4 L^2 bytes per
 * (query, head) through HBM); NULL keeps the recomputing dQ kernel (no L^2 scratch). */
int ptr_mhsa_backward(const float *Q, const float *K, const float *V, int ld_qkv, const float *O, const float *dO, const float *lse,
                      const int32_t *lens, int B, int L, int F, int n_heads, float p_drop, uint64_t seed, int site, float *dvec,
                      float *dQ, float *dK, float *dV, float *ds_ws, void *stream);
/* Test helper: the attention dropout keep-mask (1.0 / 0.0), out [B][n_heads][L][L]. */
int ptr_mhsa_dropout_mask(int B, int L, int n_heads, float p_drop, uint64_t seed, int site, float *out, void *stream);
/* LayerNorm of ptranking/base/list_ranker.py:152-174: y = a_2 * (x - mean) / (std + eps) + b_2 over the last axis of X [R][F],
 * std UNBIASED (divides by F-1) and eps added to the std.  stats [R][3] = {mean, 1/(std+eps), std} feeds the backward.
 * ptr_layernorm_backward: dY -> dX [R][F], da2 [F], db2 [F]; ws = ptr_layernorm_backward_ws_floats(F) floats of scratch. */
int ptr_layernorm_forward(const float *X, const float *a2, const float *b2, int64_t R, int F, float eps, float *Y, float *stats,
                          void *stream);
size_t ptr_layernorm_backward_ws_floats(int F);
int ptr_layernorm_backward(const float *X, const float *a2, const float *dY, const float *stats, int64_t R, int F, float *ws,
                           float *dX, float *da2, float *db2, void *stream);

/* Test helper (no GPU, nothing launched): which kernel form the entry point named `entry` launches for a shape.  It calls the very function
 * the entry point's launcher calls, so it reads the same PTR_* switches and the same device (compute units).  args [nargs] in, form [nform]
 * out (nform may exceed the count below; the rest is left alone).  `aligned`: the call's arrays are 16-byte aligned.
 *   entry                                        args                                     form
 *   ptr_lambdarank_fwd_bwd                       B, L, sigma > 0                          kind, G, DPT, QPB      kind: 0 LDS kernel, 1 ring (QPB
 *   ptr_ranknet_fwd_bwd                          B, L                                     kind, G, DPT, QPB        waves), 2 half-wave; QPB: queries
 *                                                                                                                  per workgroup
 *   ptr_approxndcg_fwd_bwd, ptr_softrank_fwd_bwd,
 *   ptr_smoothmetric_fwd_bwd, ptr_gaussmetric_fwd_bwd   L                                 ring, G, DPT           ring: 1 ring form, 0 LDS / walk form
 *   ptr_listnet_fwd_bwd, ptr_listmle_fwd_bwd     L, aligned                               vec, G, V              vec: 1 register kernel (V float4 per
 *                                                                                                                  lane, G lanes per query), 0 LDS kernel
 *   ptr_lambdaloss_fwd_bwd                       L, k, loss_type, presort, aligned        vec, G, V              vec: 1 top-k kernel; 0 generic, (G, DPT)
 *   ptr_mhsa_forward, ptr_mhsa_backward          L, head dim, row stride, ds_ws given,    wide, D, forward row tiles, dK/dV waves, stored dS,
 *                                                alignment of the arrays in bytes           floats per global access
 *   ptr_layernorm_forward, ptr_layernorm_backward   R, F                                  NI, forward workgroups, backward workgroups
 *   ptr_wassrank_fwd_bwd                         L                                        G, DPT
 *   ptr_alphadcg_fwd_bwd                         T, L                                     G, TP
 *   ptr_div_metrics_at_ks                        L                                        G, DPT
 *   ptr_divprob_fwd_bwd                          objective, T, L                          G, TP
 *   ptr_gbdt_histogram                           m, F, max_bin                            kind, features per tile, tiles, row chunks, LDS bytes
 *                                                                                           kind: 0 nothing, 1 direct, 2 LDS tile
 *   ptr_gbdt_histogram_segments                  m, F, max_bin, total                     kind, features per tile, tiles, row chunks, LDS bytes,
 *                                                (m: one segment's rows; total: the rows    rows per chunk, the direct form's row bound, the most
 *                                                of the call's LDS-form segments)           launches of one call
 *   ptr_gbdt_hist_sub_segments                   K                                        launches of one call (1), workgroup rows per triple
 *   ptr_gbdt_best_split_slots                    K                                        launches of one call (2), 0
 *   ptr_gbdt_partition_segments                  m                                        launches of one call (3), workgroups of a segment of m rows
 *   ptr_gbdt_goss                                n                                        counting passes (3), digits per pass (2048), workgroups
 *                                                                                           of a pass, launches of one call (5; 0 for n == 0)
 *   ptr_gbdt_partition_mask                      m                                        launches of one call (3), workgroups of a list of m rows
 *   ptr_gbdt_leaf_sums                           n, nleaves                               kind, threads per workgroup, workgroups, LDS bytes, the
 *                                                                                           most leaves of the LDS form (1024)
 *                                                                                           kind: 0 nothing, 1 LDS cells, 2 global atomics
 *   ptr_irgan_sample, ptr_irgan_point_gen_fwd_bwd   L                                     G, queries per workgroup
 *   ptr_irgan_sel_fwd_bwd                        mode, L                                  G, queries per workgroup
 *   ptr_irfgan_point_sample, ptr_irfgan_pair_sample   L                                   G, queries per workgroup
 *   ptr_irfgan_fwd_bwd                           mode, L                                  G, queries per workgroup
 *   ptr_adlist_sample, ptr_adlist_fwd_bwd        L                                        G, queries per workgroup
 *   ptr_tree_xendcg_grad_hess                    max_len                                  G, queries per workgroup, documents per thread
 * G: threads per query, DPT: documents per thread, TP: subtopic tile.  PTR_ERR_INVALID_ARG for an entry without a form, another nargs, or
 * nform below the count. */
int ptr_launch_form(const char *entry, const int64_t *args, int nargs, int32_t *form, int nform);

/* ---- A histogram gradient-boosted tree trainer (csrc/gbdt.hip).  The symbols below are ADDITIVE to ABI v8 as well: PTR_ABI_VERSION stays 8.
 * The reference's tree frame (ptranking/ltr_tree/lambdamart/lightgbm_lambdaMART.py) hands the boosting to LightGBM; ptranking_amd/gbdt.py
 * grows the trees leaf-wise on these entry points instead.  No parity with LightGBM is claimed: the binning and tie rules are this
 * project's own (the row-sampling rules of the section after next among them), and there is no EFB or categorical handling.  Missing
 * values have entry points of their own, in the last section on the trainer; the ones here take finite features.
 *
 * Common rules: every argument is validated before any launch (PTR_ERR_INVALID_ARG: a NULL pointer that a launch would touch, a negative
 * size, max_bin < 2, a stride that is no multiple of 16 or below F; PTR_ERR_UNSUPPORTED: max_bin > PTR_GBDT_MAX_BIN); an empty input
 * launches nothing; row indices are int32 (n <= 2^31 - 1).  Integer atomics only: every result's bits depend on the data alone.
 *
 * Layouts.  bins [n][stride] uint8, row-major, stride = round_up(F, 16), 16-byte aligned, pad bytes 0.  hist [F][max_bin][3] int64: the
 * sum of qg, the sum of qh and the row count of every (feature, bin).  A split record is 9 int64: the float64 gain's bit pattern (-inf: no
 * valid split), feature, bin (both -1 without a split), then the LEFT child's sum qg, sum qh and count and the RIGHT child's.
 *
 * ptr_gbdt_bin: bins[r][f] = the number of edges[f][0 .. nbins[f] - 1) that are < X[r][f]; X [n][F] fp32 row-major, edges [F][max_bin - 1]
 *   ascending per feature, nbins [F] in 1 .. max_bin.  So x <= edges[f][b] is bin <= b.  Non-finite features are the caller's error.
 * ptr_gbdt_quantize: e_g = the largest integer with max|g| 2^e_g < 2^30 (0 when g is all zero), e_h likewise; qg = rint(g 2^e_g),
 *   qh = rint(h 2^e_h) as int32 (ties to even); expo [2] = {e_g, e_h} in device memory.  A NaN or an infinity in g or h ORs 1 into flag [1]
 *   (the caller zeroes it once and reads it when it likes) and that row is written as 0, 0; nothing is clamped.  state [2]: scratch.
 * ptr_gbdt_histogram: ADDS the rows rows[0 .. m) (rows == NULL: the rows 0 .. m - 1) into a caller-zeroed hist.  A row index outside
 *   [0, n) or a bin >= max_bin is skipped.  Forms, by m alone (ptr_launch_form): m <= 256 adds straight into global memory, one thread per
 *   (row, feature); beyond, a grid of row chunks x tiles of 16 features sums in LDS (20 bytes per (feature, bin)) and flushes the bins it
 *   touched with global integer atomic adds.
 * ptr_gbdt_hist_sub: out = parent - child over one histogram, element-wise (out may alias parent): the larger child from the smaller.
 * ptr_gbdt_best_split: per leaf histogram hist[l] of a batch [nleaf][F][max_bin][3], the best (feature, bin) -> rec [nleaf][9].  float64
 *   throughout, NOT contracted into FMAs (the library is built with -ffp-contract=off), in this order:
 *     G = (double)sum_qg 2^-e_g, H = (double)sum_qh 2^-e_h (exact);  gain = ((GL GL) / (HL + l2) + (GR GR) / (HR + l2)) - (G G) / (H + l2).
 *   A candidate (f, b), b < nbins[f] - 1, sends bins <= b left; it is valid when both children hold >= min_data_in_leaf rows, both Hessian
 *   sums are >= max(min_sum_hessian_in_leaf, 2^-40) and gain >= min_gain_to_split.  Ties: the lowest feature, then the lowest bin.
 *   expo [2] as ptr_gbdt_quantize wrote it; ws: nleaf * F * 9 int64 of scratch.  lambda_l2 < 0 or a NaN threshold: PTR_ERR_INVALID_ARG.
 * ptr_gbdt_partition: out = the rows of rows[0 .. m) with bins[row][feature] <= bin in their order, then the others in theirs;
 *   left_count [1] = how many went left.  ws: ptr_gbdt_partition_ws_ints(m) int32 of scratch.  feature outside 0 .. F - 1 or bin outside
 *   0 .. 255: PTR_ERR_INVALID_ARG.
 * ptr_gbdt_add_leaf_values: scores[rows[i]] += values[l] for offsets[l] <= i < offsets[l + 1], l < nleaves, i < total; the row lists of a
 *   finished tree's leaves are disjoint, so one launch serves them all.
 * ptr_gbdt_predict: out[r] = the fp32 sum, in tree order from 0, of the leaf value each tree gives X[r].  Tree t owns the nodes
 *   tree_offsets[t] .. tree_offsets[t + 1] of feature / threshold / left / right (child indices within the tree, a negative child is leaf
 *   ~i) and the leaf values value[tree_offsets[t] + t ..] (a tree of k nodes has k + 1 leaves; k = 0 is a single leaf).  A row goes left
 *   on x <= threshold.  A malformed tree yields NaN, never a read out of range. */
#define PTR_GBDT_MAX_BIN 256
int ptr_gbdt_bin(const float *X, int64_t n, int F, const float *edges, const int32_t *nbins, int max_bin, int stride, uint8_t *bins,
                 void *stream);
int ptr_gbdt_quantize(const float *g, const float *h, int64_t n, int32_t *qg, int32_t *qh, int32_t *expo, int32_t *flag, uint32_t *state,
                      void *stream);
int ptr_gbdt_histogram(const uint8_t *bins, int stride, int64_t n, const int32_t *qg, const int32_t *qh, const int32_t *rows, int64_t m,
                       int F, int max_bin, int64_t *hist, void *stream);
int ptr_gbdt_hist_sub(const int64_t *parent, const int64_t *child, int F, int max_bin, int64_t *out, void *stream);
int ptr_gbdt_best_split(const int64_t *hist, int nleaf, int F, int max_bin, const int32_t *nbins, const int32_t *expo, double lambda_l2,
                        int64_t min_data_in_leaf, double min_sum_hessian_in_leaf, double min_gain_to_split, int64_t *ws, int64_t *rec,
                        void *stream);
size_t ptr_gbdt_partition_ws_ints(int64_t m);
int ptr_gbdt_partition(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m, int feature, int bin,
                       int32_t *out, int32_t *left_count, int32_t *ws, void *stream);
int ptr_gbdt_add_leaf_values(float *scores, int64_t n, const int32_t *rows, const int32_t *offsets, const float *values, int nleaves,
                             int64_t total, void *stream);
int ptr_gbdt_predict(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                     const int32_t *right, const float *value, const int32_t *tree_offsets, int ntrees, float *out, void *stream);

/* ---- One level of a depth-wise tree in batched passes (csrc/gbdt.hip; grow_policy='depthwise' of ptranking_amd/gbdt.py).  ADDITIVE to ABI
 * v8 too.  Each pass serves K leaves with a fixed number of launches.  The small int32 tables are DEVICE arrays the caller builds on the host
 * (it knows every count from the split records it has read) and uploads.  Host checks before any launch, PTR_ERR_INVALID_ARG: a NULL
 * pointer a launch would touch, K < 0, max_bin < 2 (PTR_ERR_UNSUPPORTED above PTR_GBDT_MAX_BIN, as above), F < 1, the bins layout, a
 * workspace that is too small.  K == 0 succeeds and launches nothing.  In the kernels a table entry that points outside rows, outside the
 * pool's slots or at a feature or bin out of range is skipped, never followed.  pool: int64 [nslots][F][max_bin][3].
 *
 * ptr_gbdt_histogram_segments: segs [K][3] = (start, count, slot) over the row list rows [nrows]; ADDS the rows rows[start .. start + count)
 *   into pool[slot] (the caller zeroes the slots) — exactly the integers ptr_gbdt_histogram gives for that row list.  items
 *   [n_direct + n_lds][3] = (segment, first row within the segment, rows): the work list.  The first n_direct items are whole segments of
 *   at most 256 rows (one launch: a thread per (row, feature), global integer atomics); the n_lds others are row chunks of longer segments
 *   (one launch: grid = items x tiles of 16 features, the LDS tile of ptr_gbdt_histogram).  ptr_launch_form gives the form of a segment of
 *   m rows and the rows per chunk.  Rows listed twice are added twice.
 * ptr_gbdt_hist_sub_segments: trips [K][3] = (parent slot, child slot, out slot): pool[out] = pool[parent] - pool[child] element-wise; out
 *   may be the parent.  One launch.
 * ptr_gbdt_best_split_slots: ptr_gbdt_best_split over the histograms pool[slots[k]], k < K, in place of a contiguous batch -> rec [K][9], each
 *   bit-identical to ptr_gbdt_best_split on a copy of that slot (one shared scan).  A slot outside the pool gives the record without a
 *   split.  ws: K * F * 9 int64 of scratch.
 * ptr_gbdt_partition_segments: segs [K][4] = (start, count, feature, bin), disjoint: out[start .. start + count) = ptr_gbdt_partition of
 *   rows[start .. start + count) by (feature, bin), left_counts [K] = how many went left; every position of rows [nrows] outside the
 *   segments is copied to out unchanged, so out is a whole row list (out must not be rows).  blocks [nblocks][2] = (segment, j): one entry
 *   per 1024 rows of every segment, a segment's entries together in ascending j.  Three launches (count, one scan over all blocks whose
 *   differences within a segment are the segmented scan, scatter) after one device copy; no atomic decides a position.  ws:
 *   ptr_gbdt_partition_segments_ws_ints(nblocks) int32, ws_ints of them given. */
int ptr_gbdt_histogram_segments(const uint8_t *bins, int stride, int64_t n, const int32_t *qg, const int32_t *qh, const int32_t *rows,
                                int64_t nrows, const int32_t *segs, int K, const int32_t *items, int n_direct, int n_lds, int F, int max_bin,
                                int64_t *pool, int nslots, void *stream);
int ptr_gbdt_hist_sub_segments(int64_t *pool, int nslots, int F, int max_bin, const int32_t *trips, int K, void *stream);
int ptr_gbdt_best_split_slots(const int64_t *pool, int nslots, const int32_t *slots, int K, int F, int max_bin, const int32_t *nbins,
                              const int32_t *expo, double lambda_l2, int64_t min_data_in_leaf, double min_sum_hessian_in_leaf,
                              double min_gain_to_split, int64_t *ws, int64_t *rec, void *stream);
size_t ptr_gbdt_partition_segments_ws_ints(int64_t nblocks);
int ptr_gbdt_partition_segments(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t nrows, const int32_t *segs, int K,
                                const int32_t *blocks, int nblocks, int32_t *out, int32_t *left_counts, int32_t *ws, int64_t ws_ints,
                                void *stream);

/* ---- Row sampling for the tree trainer: bagging by row or by query, and GOSS (csrc/gbdt.hip; bagging_fraction, bagging_freq,
 * bagging_by_query and data_sample_strategy='goss' of ptranking_amd/gbdt.py).  ADDITIVE to ABI v8 too.  The rules are this project's own; no
 * parity with LightGBM's random streams is claimed.  tests/gbdt_sample_ref.py restates them in numpy.  Argument rules as above: everything
 * is validated before any launch (PTR_ERR_INVALID_ARG: a NULL pointer a launch would touch, a negative size or draw, n > 2^31 - 1, a rate
 * outside its range, a bad bins layout), and an empty input launches nothing.
 *
 * Uniforms.  u(draw, unit) = pl_uniform(pl_query_keys(seed, draw), (uint32_t)unit) of the counter stream of the device samplers
 *   (csrc/ptr_plhash.h): a multiple of 2^-24 in [0, 1) that depends on (seed, draw, unit) alone.
 * ptr_gbdt_bag_mask: mask[r] = u(draw, unit_r) < fraction, one byte per row, 1 = in the bag; unit_r = r, or qid[r] when qid is given (all
 *   rows of a query share one draw).  A Bernoulli draw per unit, not a fixed count.  fraction in (0, 1]; 1.0 keeps every row.  The
 *   trainer's tree t (from 0) uses draw = t / bagging_freq (integer division) and fraction = (float)bagging_fraction.
 * ptr_gbdt_goss: gradient-based one-side sampling of one round.  key_r = fabsf(g_r * h_r), one fp32 product; K = max(1, floor(n top_rate))
 *   with the product in float64; tau = the K-th largest key, found exactly by a radix select over the keys' uint32 bit patterns (three
 *   counting passes, integer counters only; a NaN key counts as the smallest).  A row with key >= tau is in the top set and keeps g, h: ties
 *   at tau are all in, so the top set may exceed K.  Any other row (a NaN key compares false and is one) is kept iff
 *   u(draw, r) < (float)(other_rate / (1 - top_rate)), and a KEPT other row has g and h multiplied in fp32 by
 *   (float)((1 - top_rate) / other_rate); a dropped row's g and h are copied unchanged (a NaN stays a NaN for ptr_gbdt_quantize's flag).
 *   Writes g_out, h_out [n] (each may be its input), mask [n] (1 = kept) and info [3] = {tau's bit pattern, the size of the top set, the
 *   number kept}.  top_rate, other_rate > 0 with top_rate + other_rate <= 1.  ws: ptr_gbdt_goss_ws_ints(n) int32 of scratch.  The trainer
 *   uses draw = t and leaves the first floor(1 / learning_rate) trees unsampled.
 * ptr_gbdt_partition_mask: ptr_gbdt_partition's stable count / scan / scatter (the same three kernels) under the predicate mask[row] != 0:
 *   out = the rows of rows[0 .. m) with a set mask byte in their order, then the others in theirs; left_count [1] = how many were kept.
 *   rows == NULL is the list 0 .. m - 1.  A row index outside [0, n) is not kept and its mask byte is never read.  out must not be rows.
 *   ws: ptr_gbdt_partition_ws_ints(m) int32.
 * ptr_gbdt_add_tree_binned: scores[rows[i]] += the leaf value ONE tree gives the binned row, i < m (rows == NULL: the rows 0 .. m - 1; a
 *   row index outside [0, n) is skipped).  The tree is in ptr_gbdt_predict's node layout with the split BIN in place of the threshold
 *   (feature, bin, left, right [nnodes], value [nnodes + 1]; nnodes == 0 is a single leaf); a row goes left on bins[row][feature] <= bin,
 *   which is x <= edges[feature][bin] by the binning rule, so the value is the one ptr_gbdt_predict adds for the raw row.  A malformed
 *   tree adds NaN, never a read out of range.  The rows of the list must be distinct.
 * A sampled tree is grown on the front segment [0, left_count) of the partitioned list and its leaf values reach the rows behind it through
 * ptr_gbdt_add_tree_binned, so the resident training scores stay the bits of ptr_gbdt_predict for every row. */
int ptr_gbdt_bag_mask(int64_t n, const int32_t *qid, uint64_t seed, int64_t draw, float fraction, uint8_t *mask, void *stream);
size_t ptr_gbdt_goss_ws_ints(int64_t n);
int ptr_gbdt_goss(const float *g, const float *h, int64_t n, double top_rate, double other_rate, uint64_t seed, int64_t draw, float *g_out,
                  float *h_out, uint8_t *mask, int32_t *info, int32_t *ws, void *stream);
int ptr_gbdt_partition_mask(const uint8_t *mask, int64_t n, const int32_t *rows, int64_t m, int32_t *out, int32_t *left_count, int32_t *ws,
                            void *stream);
int ptr_gbdt_add_tree_binned(float *scores, const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m,
                             const int32_t *feature, const int32_t *bin, const int32_t *left, const int32_t *right, const float *value,
                             int nnodes, void *stream);

/* ---- Missing feature values with learned directions (csrc/gbdt.hip; use_missing=True of ptranking_amd/gbdt.py).  ADDITIVE to ABI v8 too;
 * every symbol above keeps its signature and its results bit for bit (each pair shares one kernel or one template, the older entry point
 * passing "no missing").  A NaN is a missing value; an infinity stays the caller's error.  The rules are scikit-learn's
 * (HistGradientBoostingRegressor) wherever its are deterministic; tests/gbdt_missing_ref.py restates them in numpy.  Out of scope:
 * zero_as_missing, and the LETOR loader's absent features, which stay zeros.  Argument rules as above: everything is validated before any
 * launch, and the int32 tables in device memory (nan_bin, the segment table, also_left by node) are read as untrusted in the kernels.
 *
 * Bins.  nan_bin [F] int32 in device memory: the bin of feature f's NaNs, behind its value bins (nbins[f] <= nan_bin[f] < max_bin; the
 *   trainer uses nan_bin[f] = nbins[f]), or -1 for a feature whose training rows hold no NaN.  nbins keeps counting value bins only, and
 *   the histogram layout [F][max_bin][3] is unchanged: the histogram entry points serve both.  An entry outside that range reads as -1 in
 *   every kernel (a device table cannot be checked before the launch); a scalar also_left outside -1 .. 255 is PTR_ERR_INVALID_ARG.
 * ptr_gbdt_bin_missing: ptr_gbdt_bin, and a NaN of feature f gets the bin nan_bin[f] (bin 0 where that is -1, as ptr_gbdt_bin gives).
 * ptr_gbdt_best_split_missing, ptr_gbdt_best_split_slots_missing: the scan of ptr_gbdt_best_split / _slots with (MG, MH, MC) = the
 *   histogram entry of the NaN bin (zero without one); the node's totals include it.  Candidates per feature: (1) b < nbins - 1, bins <= b
 *   left and the missing rows right; (2) only when MC > 0, b = nbins - 1: every value left, the NaNs right (its threshold is the +inf
 *   padding of the edges); (3) only when MC > 0, b < nbins - 1 with the missing rows LEFT, the left sums being the prefix plus (MG, MH,
 *   MC).  The validity rules and the uncontracted float64 gain are ptr_gbdt_best_split's; one prefix pass serves both directions.  Ties:
 *   the highest gain, then the lowest feature, then missing-right before missing-left, then the lowest bin among missing-right candidates
 *   and the HIGHEST bin among missing-left ones (scikit-learn scans those from the top bin down and keeps the first of equal gains; bins
 *   that are empty in a node make such ties bit-exact and common).  The record stays 9 int64; field 2 is bin + 256 * default_left, and the
 *   sums are the true left and right sums with the missing rows on their side.  default_left is the winning candidate's direction when
 *   MC > 0; otherwise the node's rows do not decide it and default_left = (left count > right count).
 * ptr_gbdt_partition_missing: ptr_gbdt_partition, and the bin also_left goes left as well (-1: none): a row goes left iff
 *   bins[row][feature] <= bin or bins[row][feature] == also_left.  The trainer passes nan_bin[feature] where default_left is set.
 * ptr_gbdt_partition_segments_missing: ptr_gbdt_partition_segments over segs [K][5] = (start, count, feature, bin, also_left); a segment
 *   whose also_left lies outside -1 .. 255 is left as it was.
 * ptr_gbdt_add_tree_binned_missing: ptr_gbdt_add_tree_binned with also_left [nnodes]: at a node the bin also_left[node] goes left too.
 * ptr_gbdt_predict_missing: ptr_gbdt_predict with default_left [nodes of all trees] uint8: at a node a NaN feature goes left where the
 *   byte is set and right otherwise; any other value goes left on x <= threshold.  A malformed tree yields NaN, never a read out of range. */
int ptr_gbdt_bin_missing(const float *X, int64_t n, int F, const float *edges, const int32_t *nbins, const int32_t *nan_bin, int max_bin,
                         int stride, uint8_t *bins, void *stream);
int ptr_gbdt_best_split_missing(const int64_t *hist, int nleaf, int F, int max_bin, const int32_t *nbins, const int32_t *nan_bin,
                                const int32_t *expo, double lambda_l2, int64_t min_data_in_leaf, double min_sum_hessian_in_leaf,
                                double min_gain_to_split, int64_t *ws, int64_t *rec, void *stream);
int ptr_gbdt_best_split_slots_missing(const int64_t *pool, int nslots, const int32_t *slots, int K, int F, int max_bin, const int32_t *nbins,
                                      const int32_t *nan_bin, const int32_t *expo, double lambda_l2, int64_t min_data_in_leaf,
                                      double min_sum_hessian_in_leaf, double min_gain_to_split, int64_t *ws, int64_t *rec, void *stream);
int ptr_gbdt_partition_missing(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m, int feature, int bin,
                               int also_left, int32_t *out, int32_t *left_count, int32_t *ws, void *stream);
int ptr_gbdt_partition_segments_missing(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t nrows,
                                        const int32_t *segs, int K, const int32_t *blocks, int nblocks, int32_t *out, int32_t *left_counts,
                                        int32_t *ws, int64_t ws_ints, void *stream);
int ptr_gbdt_add_tree_binned_missing(float *scores, const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m,
                                     const int32_t *feature, const int32_t *bin, const int32_t *left, const int32_t *right,
                                     const float *value, const int32_t *also_left, int nnodes, void *stream);
int ptr_gbdt_predict_missing(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                             const int32_t *right, const float *value, const int32_t *tree_offsets, const uint8_t *default_left, int ntrees,
                             float *out, void *stream);

/* ---- Categorical features: set splits (csrc/gbdt.hip; categorical_feature of ptranking_amd/gbdt.py).  ADDITIVE to ABI v8 too; every
 * symbol above keeps its signature and its results bit for bit (each pair shares one kernel template, the older entry point passing "no
 * categorical").  The rules are scikit-learn's (HistGradientBoostingRegressor(categorical_features=...), _find_best_bin_to_split_category)
 * wherever its are deterministic, under LightGBM's parameter names; tests/gbdt_cat_ref.py restates them in numpy.  Out of scope:
 * max_cat_to_onehot, cat_l2, min_data_per_group, max_cat_threshold.
 *
 * A categorical column holds integer codes; its edges are 0.5, 1.5, ..., so ptr_gbdt_bin maps code c to bin c and nbins[f] is the largest
 * code plus 1.  is_cat [F] uint8 in device memory: non-zero marks a categorical feature.  nan_bin is as in the section above and may be
 * NULL (no missing values): one _cat family serves both.  A left set is 256 bits in 4 int64, bit b in word b / 64.
 *
 * The rule, for a categorical feature at a node with totals (TG, TH, TC), the NaN bin included:
 *   1. The categories are the value bins 0 .. nbins[f] - 1 and, where nan_bin[f] >= 0, the NaN bin.  G_c, H_c are the exact float64
 *      values ldexp(qsum, -e), as in the numeric scan.
 *   2. A category is USED iff it holds a row and H_c * (TC / TH) >= cat_smooth, in float64 in that order, nothing contracted (and its key
 *      is a number: with cat_smooth = 0 a category of zero Hessian is not used).
 *   3. Its key is v_c = G_c / (H_c + cat_smooth).
 *   4. With u used categories, u <= 1 gives no split on this feature; otherwise the used categories are sorted ascending by v, equal keys
 *      by the lower bin (scikit-learn's qsort leaves that open: the tie rule is this project's own).
 *   5. Candidates.  Left to right: the first i + 1 sorted categories go left, i = 0 .. (u + 1) / 2 - 1.  Right to left: the last i + 1
 *      go left, i = 0 .. (u + 1) / 2 - 2.  Unused categories and empty bins always go right.
 *   6. Validity and gain: those of ptr_gbdt_best_split (min_data_in_leaf, the Hessian floor, min_gain_to_split, the uncontracted float64
 *      gain over integer sums of the categories that go left).  scikit-learn's continue / break walk accepts the same candidates whenever
 *      counts and Hessian sums grow along the scan.
 *   7. Ties: the highest gain, then the lowest feature, then left-to-right before right-to-left, then the candidate with fewer categories
 *      on the left (scikit-learn's first-found).
 *   8. The record stays 9 int64 with the true left and right sums.  Field 2 is the number of left categories (at most 128) plus
 *      256 * default_left; default_left is the NaN bin's bit in the left set, 0 without a NaN bin.  The left set goes to sets [nleaf][4];
 *      a numeric winner, or a leaf without a split, leaves its set zero, and a numeric winner's record is the one ptr_gbdt_best_split
 *      (nan_bin NULL) or ptr_gbdt_best_split_missing writes.
 * ptr_gbdt_best_split_cat, ptr_gbdt_best_split_slots_cat: ws holds nleaf * F * 13 (K * F * 13) int64: the features' records, then their
 *   sets.  cat_smooth must be finite and >= 0.  One wavefront per (leaf, feature) as before; a categorical feature ranks its keys by
 *   counting (each lane's four keys broadcast in turn), permutes the sums through 6 KiB of LDS per wavefront and scans once for both
 *   directions.  Integer sums and vector stores only: the bits depend on the histogram alone.
 * ptr_gbdt_partition_cat: a row goes left iff, at a categorical feature, bit bins[row][feature] of set (4 int64 in device memory) is
 *   set; at any other feature iff bins[row][feature] <= bin, or default_left (0 or 1) is set and the bin is nan_bin[feature].
 * ptr_gbdt_partition_segments_cat: the same over segs [K][5] = (start, count, feature, bin, default_left) with sets [K][4] beside it.
 * ptr_gbdt_add_tree_binned_cat, ptr_gbdt_predict_cat: cat_index [nodes] is -1 at a numeric node, else the node's set cat_sets[cat_index]
 *   (ncat sets; over all trees in ptr_gbdt_predict_cat).  default_left [nodes] uint8 may be NULL (nothing goes left by default).  The
 *   binned walk tests the bin's bit at a categorical node and bin <= bin[node] (or the NaN bin under default_left) at a numeric one.  The
 *   raw walk turns x into a code at a categorical node: a NaN follows default_left; a value that is no integer in 0 .. 255 is in no
 *   set and goes right, and so does a code the training data never held; otherwise the code's bit decides.  ptr_gbdt_predict_cat takes
 *   no nan_bin: raw rows have no bins.  A malformed tree (a cat_index at or past ncat, a node whose kind is not its feature's) yields
 *   NaN, never a read out of range.  Everything is validated before any launch. */
int ptr_gbdt_best_split_cat(const int64_t *hist, int nleaf, int F, int max_bin, const int32_t *nbins, const int32_t *nan_bin,
                            const uint8_t *is_cat, const int32_t *expo, double lambda_l2, int64_t min_data_in_leaf,
                            double min_sum_hessian_in_leaf, double min_gain_to_split, double cat_smooth, int64_t *ws, int64_t *rec,
                            int64_t *sets, void *stream);
int ptr_gbdt_best_split_slots_cat(const int64_t *pool, int nslots, const int32_t *slots, int K, int F, int max_bin, const int32_t *nbins,
                                  const int32_t *nan_bin, const uint8_t *is_cat, const int32_t *expo, double lambda_l2,
                                  int64_t min_data_in_leaf, double min_sum_hessian_in_leaf, double min_gain_to_split, double cat_smooth,
                                  int64_t *ws, int64_t *rec, int64_t *sets, void *stream);
int ptr_gbdt_partition_cat(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m, int feature, int bin,
                           int default_left, const uint8_t *is_cat, const int32_t *nan_bin, const int64_t *set, int32_t *out,
                           int32_t *left_count, int32_t *ws, void *stream);
int ptr_gbdt_partition_segments_cat(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t nrows,
                                    const int32_t *segs, const int64_t *sets, int K, const uint8_t *is_cat, const int32_t *nan_bin,
                                    const int32_t *blocks, int nblocks, int32_t *out, int32_t *left_counts, int32_t *ws, int64_t ws_ints,
                                    void *stream);
int ptr_gbdt_add_tree_binned_cat(float *scores, const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m,
                                 const int32_t *feature, const int32_t *bin, const int32_t *left, const int32_t *right, const float *value,
                                 const uint8_t *default_left, const uint8_t *is_cat, const int32_t *nan_bin, const int32_t *cat_index,
                                 const int64_t *cat_sets, int ncat, int nnodes, void *stream);
int ptr_gbdt_predict_cat(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                         const int32_t *right, const float *value, const int32_t *tree_offsets, const uint8_t *default_left,
                         const uint8_t *is_cat, const int32_t *cat_index, const int64_t *cat_sets, int ncat, int ntrees, float *out,
                         void *stream);

/* ---- Monotone and interaction constraints (csrc/gbdt.hip; monotone_constraints, interaction_constraints of ptranking_amd/gbdt.py).
 * ADDITIVE to ABI v8 too; every symbol above keeps its signature and its results bit for bit (the constrained scan is one more template
 * flag of the same kernels, the older entry points passing "no constraints").  Training-time rules: a tree, prediction and the model
 * formats do not change.  The rules are scikit-learn's (HistGradientBoostingRegressor(monotonic_cst=..., interaction_cst=...)) wherever
 * its are deterministic, which is LightGBM's monotone_constraints_method 'basic'; tests/gbdt_cst_ref.py restates them in numpy.  Out of
 * scope: the methods 'intermediate' and 'advanced', monotone_penalty.
 *
 * Per node the grower keeps (lo, hi, v) as float64: [lo, hi] bounds the values of the node's children, v is the node's own value.  Root:
 * lo = -inf, hi = +inf, v = -G / (H + lambda_l2).
 *
 * The bounded gain.  Under active monotone constraints EVERY split search of the fit uses it on EVERY candidate: numeric features, the
 * three missing-value candidates, categorical set candidates, features whose constraint is 0, nodes whose bounds are infinite.
 *   1. vL = clamp(-GL / (HL + l2), lo, hi) = min(max(., lo), hi), and vR likewise.
 *   2. The candidate is rejected if the feature's constraint is +1 and vL > vR, or -1 and vL < vR (a categorical feature has none).
 *   3. gain = ((G * v) - (GL * vL)) - (GR * vR), float64 in that order, every product and difference rounded, nothing contracted.
 *   4. The validity rules, min_gain_to_split, the tie rules and the record (9 int64) are those of the scans above.
 * When a node splits on feature f, each child takes its clamped vL or vR as its v; with mid = (vL + vR) / 2 its bounds are
 *   constraint 0: left [lo, hi], right [lo, hi];   +1: left [lo, mid], right [mid, hi];   -1: left [mid, hi], right [lo, mid]
 * (scikit-learn's grower.py:574-595).  The host computes vL, vR and mid from the integer sums of the record it has read anyway.  A leaf's
 * stored value is float32(v * learning_rate) with its clamped v.
 *
 * Interaction constraints.  The groups are sets of features; features in no group form one more group (scikit-learn's rule; LightGBM's
 * treatment of unlisted features is not claimed).  The root's active groups are all groups and every feature is allowed; a child of a
 * split on f keeps the active groups that contain f, and its allowed features are their union.  The scan skips a feature that is not
 * allowed; a node with no valid allowed candidate is a leaf.  With interaction constraints alone the gain is that of the scans above,
 * bit for bit, on the allowed features.
 *
 * ptr_gbdt_best_split_cst, ptr_gbdt_best_split_slots_cst: the arguments of the _cat forms plus three tables in device memory, read as
 *   untrusted:  mono [F] int8 (an entry outside -1 .. 1 reads as 0);  cst [nleaf][3] ([K][3], by place in the slot list) float64
 *   (lo, hi, v), or NULL: interaction constraints alone;  allowed [nleaf][F] ([K][F]) uint8, non-zero = allowed, or NULL: every feature.
 *   A NaN among a leaf's (lo, hi, v), or lo > hi, makes that leaf's record "no split".  One of cst and allowed must be given, and cst
 *   needs mono.  is_cat may be NULL here (no categorical feature; sets is then not written and may be NULL, and ws holds 9 int64 per
 *   (leaf, feature) in place of 13).  Everything is validated before any launch. */
int ptr_gbdt_best_split_cst(const int64_t *hist, int nleaf, int F, int max_bin, const int32_t *nbins, const int32_t *nan_bin,
                            const uint8_t *is_cat, const int32_t *expo, double lambda_l2, int64_t min_data_in_leaf,
                            double min_sum_hessian_in_leaf, double min_gain_to_split, double cat_smooth, int64_t *ws, int64_t *rec,
                            int64_t *sets, const int8_t *mono, const double *cst, const uint8_t *allowed, void *stream);
int ptr_gbdt_best_split_slots_cst(const int64_t *pool, int nslots, const int32_t *slots, int K, int F, int max_bin, const int32_t *nbins,
                                  const int32_t *nan_bin, const uint8_t *is_cat, const int32_t *expo, double lambda_l2,
                                  int64_t min_data_in_leaf, double min_sum_hessian_in_leaf, double min_gain_to_split, double cat_smooth,
                                  int64_t *ws, int64_t *rec, int64_t *sets, const int8_t *mono, const double *cst, const uint8_t *allowed,
                                  void *stream);

/* ---- TreeSHAP feature contributions (csrc/gbdt.hip; GBDT.predict(pred_contrib=True), GBDT.set_background of ptranking_amd/gbdt.py).
 * ADDITIVE to ABI v8 too; every symbol above keeps its signature and its results bit for bit.  tests/gbdt_shap_ref.py restates the rule.
 *
 * The rule: path-dependent TreeSHAP (Lundberg, Erion, Lee 2018, Algorithm 2) in its per-leaf closed form.  Take a tree, a leaf l with fp32
 * value v_l, and the set U of DISTINCT features on its root-to-leaf path, d = |U|.  For each k in U:
 *   the zero fraction z_k = the product, over the path's nodes that split on k in path order, of cover(child taken) / cover(node);
 *   the one fraction o_k(x), 0 or 1 = 1 iff row x goes the path's way at every node that splits on k.
 * "Goes the path's way" is the predicate of ptr_gbdt_predict / _missing / _cat on the raw row (x <= threshold, a NaN along default_left, set
 * membership), so a row's o's are all 1 at exactly the leaf predict reaches.  Then
 *   phi_k(x) += v_l (o_k - z_k) sum over S in U \ {k} of |S|! (d - |S| - 1)! / d!  prod_{j in S} o_j  prod_{j not in S, j != k} z_j
 *   phi_F(x) += v_l prod_{k in U} z_k                      (the expected value: the last column)
 * summed in float64 over the leaves in table order (tree order, then leaf order).  The covers are the rows of a BACKGROUND matrix: a tree
 * and the model files keep no counts.  ptr_gbdt_leaf_counts counts the rows per leaf and the host sums them into node covers.
 *
 * How the sum over S is formed.  |S|! (d - |S| - 1)! / d! is the integral over t in [0, 1] of t^|S| (1 - t)^(d - 1 - |S|), so the sum is the
 * integral of prod_{j in U, j != k} (z_j (1 - t) + o_j t), a polynomial of degree d - 1 with positive factors, and the Gauss-Legendre rule of
 * Q = ceil(d / 2) nodes on [0, 1] integrates it exactly.  Nothing cancels, whatever d.  The rules of Q = 1 .. 32 nodes are a table the
 * caller hands in: quad_t, quad_w [528] float64, the rule of Q nodes at Q (Q - 1) / 2 (GBDT builds it with numpy's leggauss).
 *
 * The order of operations (float64, every operation rounded, nothing contracted).  With the elements e = 0 .. d - 1 in table order and
 * the nodes (t_q, w_q), q = 0 .. Q - 1:
 *   P_q = 1, pz = 1;  for j = 0 .. d - 1:  P_q <- P_q * ((z_j * (1 - t_q)) + (o_j ? t_q : 0));  pz <- pz * z_j
 *   sum_e = 0;  for q = 0 .. Q - 1:  sum_e <- sum_e + w_q * (P_q / ((z_e * (1 - t_q)) + (o_e ? t_q : 0)))
 *   phi[feature of e] <- phi[feature of e] + ((sum_e * (o_e - z_e)) * v);   phi[F] <- phi[F] + v * pz.
 *
 * The path tables, one row per leaf, built on the host once per model and background (nleaves leaves, npath path nodes, nelem elements):
 *   path_offsets [nleaves + 1] int32: leaf l owns the entries path_offsets[l] .. path_offsets[l + 1] of
 *     path_node [npath] int32: the node, an index over the nodes of ALL trees (into feature / threshold / default_left / cat_index), root first;
 *     path_dir  [npath] uint8: 1 where the path goes left there;
 *     path_elem [npath] uint8: which of the leaf's elements the node's feature is;
 *   elem_offsets [nleaves + 1] int32: leaf l owns the entries elem_offsets[l] .. elem_offsets[l + 1] (at most 63: one lane each, and the
 *     rules of up to 32 nodes; depth itself is unbounded, a feature used five times is one element) of
 *     elem_feature [nelem] int32, in the order of first use on the path, and elem_z [nelem] float64;
 *   leaf_value [nleaves] float32.
 * A sub-range of leaves is served by offsetting path_offsets, elem_offsets and leaf_value alone: their entries are absolute.
 *
 * ptr_gbdt_leaf_counts (_missing: default_left per node; _cat: the tables of ptr_gbdt_predict_cat): counts [nleaves] int64, nleaves =
 *   nodes + ntrees in the layout of the leaf values, is zeroed and then holds the rows of X [n, F] per leaf: one launch over all trees,
 *   one 64-bit integer atomic per (row, tree).  A row a malformed tree loses counts nowhere; the node arrays hold `nodes` entries and may be
 *   NULL where nodes == 0 (leaf-only trees).
 * ptr_gbdt_shap (_missing, _cat likewise, one kernel body): phi [n, F + 1] float64, every entry written.  One wavefront owns a row for
 *   the whole table and keeps its F + 1 sums in LDS: no float atomic, and a row's bits depend on the row and the tables alone, not on n,
 *   its place or the grid.  F above 8000: PTR_ERR_UNSUPPORTED.  The tables are read as untrusted: an offset, node, feature or element index
 *   out of range, or a leaf of more than 63 elements, makes the row's phi NaN, never an access out of range.  Everything else is
 *   validated before any launch (PTR_ERR_INVALID_ARG: a negative size, a NULL pointer a launch would touch). */
int ptr_gbdt_leaf_counts(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                         const int32_t *right, const int32_t *tree_offsets, int ntrees, int64_t nodes, int64_t nleaves, int64_t *counts,
                         void *stream);
int ptr_gbdt_leaf_counts_missing(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                 const int32_t *right, const int32_t *tree_offsets, const uint8_t *default_left, int ntrees,
                                 int64_t nodes, int64_t nleaves, int64_t *counts, void *stream);
int ptr_gbdt_leaf_counts_cat(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                             const int32_t *right, const int32_t *tree_offsets, const uint8_t *default_left, const uint8_t *is_cat,
                             const int32_t *cat_index, const int64_t *cat_sets, int ncat, int ntrees, int64_t nodes, int64_t nleaves,
                             int64_t *counts, void *stream);
int ptr_gbdt_shap(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, int64_t nodes,
                  const int32_t *path_offsets, const int32_t *elem_offsets, const float *leaf_value, int64_t nleaves,
                  const int32_t *path_node, const uint8_t *path_dir, const uint8_t *path_elem, int64_t npath,
                  const int32_t *elem_feature, const double *elem_z, int64_t nelem, const double *quad_t, const double *quad_w,
        double *phi, void *stream);
int ptr_gbdt_shap_missing(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, int64_t nodes,
                          const int32_t *path_offsets, const int32_t *elem_offsets, const float *leaf_value, int64_t nleaves,
                          const int32_t *path_node, const uint8_t *path_dir, const uint8_t *path_elem, int64_t npath,
                          const int32_t *elem_feature, const double *elem_z, int64_t nelem, const double *quad_t, const double *quad_w,
        const uint8_t *default_left, double *phi,
                          void *stream);
int ptr_gbdt_shap_cat(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, int64_t nodes,
                      const int32_t *path_offsets, const int32_t *elem_offsets, const float *leaf_value, int64_t nleaves,
                      const int32_t *path_node, const uint8_t *path_dir, const uint8_t *path_elem, int64_t npath,
                      const int32_t *elem_feature, const double *elem_z, int64_t nelem, const double *quad_t, const double *quad_w,
        const uint8_t *default_left,
                      const uint8_t *is_cat, const int32_t *cat_index, const int64_t *cat_sets, int ncat, double *phi, void *stream);

/* ---- A trained model on new data (csrc/gbdt.hip; GBDT.predict(pred_leaf=True), GBDT.refit and fit_bins(init_model=...) of
 * ptranking_amd/gbdt.py).  ADDITIVE to ABI v8 too; every symbol above keeps its signature and its results bit for bit.
 * tests/gbdt_lifecycle_ref.py restates the walk, the sums and the refit rule.
 *
 * All three walks take raw fp32 rows X [n][F] and decide at a node exactly as ptr_gbdt_predict / _missing / _cat do (x <= threshold, a NaN
 * along default_left, set membership, an unseen code right); the _missing forms add default_left per node, the _cat forms the tables of
 * ptr_gbdt_predict_cat (default_left may be NULL there).  Validated before any launch (PTR_ERR_INVALID_ARG): a negative size, a NULL
 * pointer a launch would touch.  There is no CPU path.
 *
 * ptr_gbdt_predict_leaf: leaf [n][ntrees] int32 row-major (LightGBM's pred_leaf layout): leaf[r][t - first] = the index l of the leaf ~l
 *   that tree t gives row r, for the trees first .. first + ntrees - 1 of tree_offsets (the node arrays hold `nodes` entries over ALL
 *   trees, and cat_index stays absolute).  A tree of no node gives 0; a malformed tree, or one outside the node arrays, gives -1.  Nothing
 *   is summed.  One thread per (row, tree).
 * ptr_gbdt_leaf_sums: ONE tree of `nodes` nodes (its arrays start at the tree; cat_index still indexes cat_sets of ncat sets).  Writes
 *   leaf [n] int32 (-1 for a row the tree loses or whose leaf index is >= nleaves) and ADDS (qg[r], qh[r], 1) into sums[leaf][3], int64
 *   [nleaves][3] that the caller has zeroed; qg, qh int32 [n] as ptr_gbdt_quantize wrote them.  Integer atomics only: the sums do not depend
 *   on the order of the adds or on the launch shape.  Forms (ptr_launch_form, by n and nleaves): nleaves <= 1024, a workgroup of 256 threads
 *   takes >= 1024 consecutive rows, sums them in LDS cells of (int64, int64, uint32) = 20 bytes (20 KiB at the most: eight workgroups, all
 *   the waves a compute unit holds, fit its 160 KiB) and flushes the cells a row reached with one global atomic per non-zero value; beyond
 *   1024 leaves every row adds into global memory.  At most 1024 workgroups per launch.
 * ptr_gbdt_add_by_leaf: scores[r] += values[leaf[r]] where 0 <= leaf[r] < nleaves; other rows are skipped. */
int ptr_gbdt_predict_leaf(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                          const int32_t *right, const int32_t *tree_offsets, int first, int ntrees, int64_t nodes, int32_t *leaf,
                          void *stream);
int ptr_gbdt_predict_leaf_missing(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                  const int32_t *right, const int32_t *tree_offsets, const uint8_t *default_left, int first, int ntrees,
                                  int64_t nodes, int32_t *leaf, void *stream);
int ptr_gbdt_predict_leaf_cat(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                              const int32_t *right, const int32_t *tree_offsets, const uint8_t *default_left, const uint8_t *is_cat,
                              const int32_t *cat_index, const int64_t *cat_sets, int ncat, int first, int ntrees, int64_t nodes,
                              int32_t *leaf, void *stream);
int ptr_gbdt_leaf_sums(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                       const int32_t *right, int nodes, const int32_t *qg, const int32_t *qh, int nleaves, int32_t *leaf, int64_t *sums,
                       void *stream);
int ptr_gbdt_leaf_sums_missing(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                               const int32_t *right, const uint8_t *default_left, int nodes, const int32_t *qg, const int32_t *qh,
                               int nleaves, int32_t *leaf, int64_t *sums, void *stream);
int ptr_gbdt_leaf_sums_cat(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                           const int32_t *right, const uint8_t *default_left, const uint8_t *is_cat, const int32_t *cat_index,
                           const int64_t *cat_sets, int ncat, int nodes, const int32_t *qg, const int32_t *qh, int nleaves, int32_t *leaf,
                           int64_t *sums, void *stream);
int ptr_gbdt_add_by_leaf(float *scores, int64_t n, const int32_t *leaf, const float *values, int nleaves, void *stream);

/* ---- LETOR / libsvm text input (HOST buffers; the data format feeding the path) ---------------------------------------
 * Replaces the pure-Python tokenizer ptranking/data/data_utils.py:276-387 (iter_lines / parse_letor):
 *   "<label> qid:<id> <fid>:<val> ... [# comment]", feature ids one-indexed unless one_indexed == 0 (Yahoo! sets,
 *   data_utils.py:495-496), absent features = `missing`, width = largest feature id in the file, values rounded
 *   text -> double -> float (the reference's float() + FloatTensor cast, data_utils.py:610).
 * Stateless two-call protocol: ptr_letor_scan sizes the file, the caller allocates, ptr_letor_load fills
 *   X [n_docs][n_features] (float, or double when x_is_f64 — parse_letor's own precision, wanted before feature scaling),
 *   y [n_docs], qids [n_queries], qoff [n_queries+1] (row range of every run of equal qids, in file
 *   order; a non-numeric qid token is reported as a 63-bit FNV-1a hash).  Multi-threaded on the host; no GPU involved. */
int ptr_letor_scan(const char *path, int one_indexed, int64_t *n_docs, int32_t *n_features, int64_t *n_queries);
int ptr_letor_load(const char *path, int one_indexed, float missing, int64_t n_docs, int32_t n_features, int64_t n_queries,
                   void *X, int x_is_f64, float *y, int64_t *qids, int64_t *qoff);

#ifdef __cplusplus
}
#endif
#endif /* PTRANKING_AMD_H */
