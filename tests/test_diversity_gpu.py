"""GPU: the diversification frame on the real kernels — ptr_alphadcg_fwd_bwd against the reference's float64 loss and gradient
(tests/golden/diversity.npz) and against the float64 restatement tests/diversity_ref.py for everything the reference cannot run (batches,
padding, the document cut-off), ptr_div_metrics_at_ks against the reference's metric functions, the DALETOR ranker in one-query and batched
form, and the data-parallel step.

Dispatch forms of the loss kernel (csrc/diversity.hip, ptr_alphadcg_fwd_bwd): threads per query G = 64 (four queries per workgroup, L <= 128) or
256 (L > 128), times the subtopic tile TP = 4 / 8 / 16 / 32 (T rounded up) — eight instantiations, each hit by FORMS below; the metric kernel
follows dispatch_tiling (G, DPT) = (64,1) (64,2) (256,1) (256,2) (256,4) (256,8) (256,16), each hit by METRIC_FORMS.
"""
import copy
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import diversity_ref as DR
import golden_util as GU

pytestmark = pytest.mark.gpu

GOLD = GU._load("diversity.npz")
LOSS_CASES = sorted(k for k in GOLD["daletor"] if not k.startswith("steep_"))
STEEP_CASES = sorted(k for k in GOLD["daletor"] if k.startswith("steep_"))
# (T, L) -> (G, TP) of the loss kernel; the last two sit on the documented LDS limits
FORMS = {(3, 40): (64, 4), (7, 100): (64, 8), (12, 128): (64, 16), (30, 64): (64, 32), (4, 200): (256, 4), (8, 300): (256, 8),
         (16, 513): (256, 16), (32, 620): (256, 32), (8, 2272): (256, 8), (3, 4092): (256, 4)}
METRIC_FORMS = {40: (64, 1), 100: (64, 2), 200: (256, 1), 500: (256, 2), 1000: (256, 4), 2000: (256, 8), 4096: (256, 16)}


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def run_loss(preds, rele, rt=10.0, alpha=0.5, top_k=10, axis=0, lens=None, ntopics=None):
    """ptr_alphadcg_fwd_bwd through the ctypes binding -> (loss_out, loss_q [B], grad [B, L]) as numpy."""
    from ptranking_amd import _lib
    p, r = dev(preds), dev(rele)
    B, T, L = r.shape
    ld, td = dev(lens, torch.int32), dev(ntopics, torch.int32)
    loss, loss_q, grad = torch.full((1,), np.nan).cuda(), torch.full((B,), np.nan).cuda(), torch.full((B, L), np.nan).cuda()
    _lib.call("ptr_alphadcg_fwd_bwd", _lib.ptr(p), _lib.ptr(r), _lib.ptr(ld), _lib.ptr(td), B, T, L, C.c_float(rt), C.c_float(alpha),
              int(top_k or 0), int(axis), _lib.ptr(loss), _lib.ptr(loss_q), _lib.ptr(grad), _lib.current_stream(p.device))
    torch.cuda.synchronize()
    return float(loss.item()), loss_q.cpu().numpy(), grad.cpu().numpy()


def run_metrics(preds, rele, ks, alpha=0.5, max_label=1.0, lens=None, ntopics=None):
    import ptranking_amd.functional as F_
    a, e, ne, v = F_.div_metrics_at_ks(dev(preds), dev(rele), ks, alpha=alpha, max_label=max_label, lens=dev(lens, torch.int32),
                                       ntopics=dev(ntopics, torch.int32))
    torch.cuda.synchronize()
    return a.cpu().numpy(), None if e is None else e.cpu().numpy(), None if ne is None else ne.cpu().numpy(), v.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 6. golden loss cases
@pytest.mark.parametrize("case", LOSS_CASES)
def test_golden_loss_against_the_reference_float64(case):
    """B = 1, top_k_axis = 0, alpha = 0.5 against the reference's float64 loss / gradient under the max-norm and the element-wise 1e-5 gate.
    The generator asserts that the reference's OWN fp32 gradient passes the same gate with need32 <= 0.5."""
    c = GOLD["daletor"][case]
    assert float(c["need32"]) <= 0.5
    loss, loss_q, grad = run_loss(c["preds"], c["rele"][None].astype(np.float32), rt=float(c["rt"]), top_k=int(c["top_k"]))
    print(f"{case}: kernel need {DR.need(grad, c['grad64']):.3f}, reference fp32 need {float(c['need32']):.3f}, "
          f"loss diff {abs(loss - float(c['loss64'])):.2e}")
    GU.assert_close(loss, c["loss64"], f"{case} loss")
    GU.assert_close(loss_q[0], c["loss64"], f"{case} loss_q")
    GU.assert_close(grad, c["grad64"], f"{case} grad")


# ---------------------------------------------------------------------------------------------------------------- 7. steep cases
@pytest.mark.parametrize("case", STEEP_CASES)
def test_steep_cases_stay_within_twice_the_reference_fp32_need(case):
    """rt = 100, T = 7, L = 64, no cut-off: the reference's own fp32 gradient needs need32 = 1.994 (steep_T7_L64_a) and 0.450 (steep_T7_L64_b)
    of the element-wise gate against its float64 gradient (its max-norm error stays below 1e-5).  The kernel must pass the max-norm gate
    and need at most 2 x need32 of the same case.  Measured on the MI355X: the kernel needs 0.009 (steep_T7_L64_a) and 0.030 (steep_T7_L64_b);
    worst need over the ordinary golden cases 0.241, over the ragged dispatch-form cases 0.176 (COVERAGE.md row f-6)."""
    c = GOLD["daletor"][case]
    loss, _, grad = run_loss(c["preds"], c["rele"][None].astype(np.float32), rt=float(c["rt"]), top_k=int(c["top_k"]))
    mine, ref = DR.need(grad, c["grad64"]), float(c["need32"])
    print(f"{case}: kernel need {mine:.3f}, reference fp32 need {ref:.3f}")
    GU.assert_close(loss, c["loss64"], f"{case} loss")
    assert np.max(np.abs(grad - c["grad64"])) <= GU.tol(c["grad64"])
    assert mine <= 2.0 * ref, f"{case}: the kernel needs {mine:.3f} of the element-wise gate, the reference's fp32 {ref:.3f}"


# ---------------------------------------------------------------------------------------------------------------- 8. batches and padding
def _batch(rng, B, T, L, density=0.15, graded=False, sigma=1.0, ragged=True):
    preds = (sigma * rng.standard_normal((B, L))).astype(np.float32)
    rele = (rng.random((B, T, L)) < density).astype(np.float32)
    if graded:
        rele *= rng.integers(1, 4, size=rele.shape).astype(np.float32)
    lens = rng.integers(max(1, L // 3), L + 1, size=B).astype(np.int32) if ragged else np.full(B, L, np.int32)
    nts = rng.integers(1, T + 1, size=B).astype(np.int32) if ragged else np.full(B, T, np.int32)
    lens[0], nts[0] = L, T
    return preds, rele, lens, nts


@pytest.mark.parametrize("T,L", sorted(FORMS))
@pytest.mark.parametrize("axis", [0, 1])
def test_every_dispatch_form_with_ragged_batches(T, L, axis):
    """Ragged lens and ntopics, NaN in every padded slot, graded relevance, B not a multiple of the four queries per workgroup, both
    top_k_axis forms: loss and real gradients equal the float64 restatement, padded gradients are exactly 0."""
    assert FORMS[(T, L)] == (64 if L <= 128 else 256, 4 if T <= 4 else 8 if T <= 8 else 16 if T <= 16 else 32)
    rng = np.random.default_rng(1000 * T + L + axis)
    B = 1 if L > 1000 else 7
    preds, rele, lens, nts = _batch(rng, B, T, L, density=0.15 if L <= 1000 else 0.05, graded=(T + L) % 2 == 0)
    want_q, want_g = DR.alphadcg_batch(preds, rele, rt=10.0, alpha=0.5, top_k=6, top_k_axis=axis, lens=lens, ntopics=nts)
    junk_p, junk_r = preds.copy(), rele.copy()
    for q in range(B):
        junk_p[q, lens[q]:] = np.nan
        junk_r[q, nts[q]:, :] = np.nan
        junk_r[q, :, lens[q]:] = np.nan
    loss, loss_q, grad = run_loss(junk_p, junk_r, top_k=6, axis=axis, lens=lens, ntopics=nts)
    print(f"T={T} L={L} axis={axis}: kernel need {DR.need(grad, want_g):.3f}")
    GU.assert_close(loss_q, want_q, "loss_q")
    GU.assert_close(loss, want_q.sum(), "loss_out")
    GU.assert_close(grad, want_g, "grad")
    for q in range(B):
        assert not grad[q, lens[q]:].any() and np.isfinite(grad[q]).all()
    clean = run_loss(preds, rele, top_k=6, axis=axis, lens=lens, ntopics=nts)
    assert clean[0] == loss and np.array_equal(clean[1], loss_q) and np.array_equal(clean[2], grad)     # garbage changes no bit


@pytest.mark.parametrize("T,L,alpha,rt,top_k", [(5, 48, 0.3, 5.0, None), (9, 160, 0.7, 20.0, 3)])
def test_other_alpha_and_no_cutoff(T, L, alpha, rt, top_k):
    rng = np.random.default_rng(77 + L)
    preds, rele, lens, nts = _batch(rng, 5, T, L)
    a32 = float(np.float32(alpha))
    for axis in (0, 1):
        want_q, want_g = DR.alphadcg_batch(preds, rele, rt=rt, alpha=a32, top_k=top_k, top_k_axis=axis, lens=lens, ntopics=nts)
        _, loss_q, grad = run_loss(preds, rele, rt=rt, alpha=alpha, top_k=top_k, axis=axis, lens=lens, ntopics=nts)
        GU.assert_close(loss_q, want_q, "loss_q")
        GU.assert_close(grad, want_g, "grad")


@pytest.mark.parametrize("T,L", [(6, 96), (6, 320)])
def test_a_query_alone_and_inside_a_batch_is_bit_identical_and_runs_repeat(T, L):
    rng = np.random.default_rng(L)
    preds, rele, lens, nts = _batch(rng, 9, T, L)
    full = run_loss(preds, rele, lens=lens, ntopics=nts)
    again = run_loss(preds, rele, lens=lens, ntopics=nts)
    assert full[0] == again[0] and np.array_equal(full[1], again[1]) and np.array_equal(full[2], again[2])
    for q in (0, 3, 8):
        _, lq, g = run_loss(preds[q:q + 1], rele[q:q + 1], lens=lens[q:q + 1], ntopics=nts[q:q + 1])
        assert lq[0] == full[1][q] and np.array_equal(g[0], full[2][q])
    # lens / ntopics NULL == every slot real
    a = run_loss(preds, rele)
    b = run_loss(preds, rele, lens=np.full(9, L, np.int32), ntopics=np.full(9, T, np.int32))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------------------------- 9. autograd
def test_autograd_scales_the_kernel_gradient():
    import ptranking_amd.functional as F_
    rng = np.random.default_rng(9)
    preds, rele, lens, nts = _batch(rng, 6, 5, 50)
    _, loss_q, grad = run_loss(preds, rele, top_k=4, axis=1, lens=lens, ntopics=nts)
    p = dev(preds).requires_grad_(True)
    loss, lq = F_.alphadcg_loss(p, dev(rele), rt=10.0, alpha=0.5, top_k=4, top_k_axis="documents", lens=dev(lens, torch.int32),
                                ntopics=dev(nts, torch.int32), return_loss_q=True)
    (loss * 3.0).backward()
    assert np.array_equal(lq.cpu().numpy(), loss_q)
    assert np.array_equal(p.grad.cpu().numpy(), grad * np.float32(3.0))
    GU.assert_close(loss.item(), loss_q.astype(np.float64).sum(), "loss")
    assert not F_.alphadcg_loss(dev(preds), dev(rele)).requires_grad


# ---------------------------------------------------------------------------------------------------------------- 10. metrics
@pytest.mark.parametrize("case", sorted(GOLD["metrics"]))
def test_golden_metrics_against_the_reference(case):
    c = GOLD["metrics"][case]
    ks, ml = [int(k) for k in c["ks"]], float(c["max_label"])
    rele = c["rele"].astype(np.float32)
    a, e, ne, v = run_metrics(c["preds"][None], rele[None], ks, max_label=ml)
    assert v.tolist() == [int(c["valid"])]
    GU.assert_close(a[0], c["andcg"], f"{case} alpha-nDCG")
    GU.assert_close(e[0], c["err_ia"], f"{case} ERR-IA")
    GU.assert_close(ne[0], c["nerr_ia"], f"{case} nERR-IA")
    a1, e1, n1, _ = run_metrics(c["preds"][None], rele[None], [int(c["k1"])], max_label=ml)
    GU.assert_close([a1[0, 0], e1[0, 0], n1[0, 0]], [c["andcg_k1"], c["err_ia_k1"], c["nerr_ia_k1"]], f"{case} single cut-off")
    # padded into a wider batch: two NaN subtopic rows and NaN documents behind the real ones, a second (empty-relevance) query
    T, L = rele.shape
    P = np.full((2, L + 5), np.nan, np.float32)
    R = np.full((2, T + 2, L + 5), np.nan, np.float32)
    P[0, :L], R[0, :T, :L] = c["preds"], rele
    P[1, :3], R[1, :1, :3] = [0.3, 0.1, 0.2], 0.0
    a2, e2, n2, v2 = run_metrics(P, R, ks, max_label=ml, lens=[L, 3], ntopics=[T, 1])
    assert np.array_equal(a2[0], a[0]) and np.array_equal(e2[0], e[0]) and np.array_equal(n2[0], ne[0])      # ERR-IA divides by ntopics, not T + 2
    assert v2.tolist() == [int(c["valid"]), 0] and not a2[1].any() and not e2[1].any() and not n2[1].any()
    a3, e3, n3, _ = run_metrics(c["preds"][None], rele[None], ks, max_label=None)
    assert e3 is None and n3 is None and np.array_equal(a3, a)


def test_metric_ties_follow_ptr_sort_desc():
    import ptranking_amd.functional as F_
    rng = np.random.default_rng(11)
    B, T, L = 5, 4, 37
    preds = rng.integers(0, 4, size=(B, L)).astype(np.float32)                  # heavy ties
    rele = (rng.random((B, T, L)) < 0.3).astype(np.float32)
    _, idx = F_.sort_desc(dev(preds))
    assert np.array_equal(idx.cpu().numpy(), np.stack([DR.sort_desc_order(p) for p in preds]))
    ks = [1, 3, 10, 37]
    a, e, ne, v = run_metrics(preds, rele, ks, max_label=1.0)
    wa, we, wn, wv = DR.div_metrics_batch(preds, rele, ks, max_label=1.0)
    GU.assert_close(a, wa, "alpha-nDCG"); GU.assert_close(e, we, "ERR-IA"); GU.assert_close(ne, wn, "nERR-IA")
    assert np.array_equal(v, wv)


@pytest.mark.parametrize("L", sorted(METRIC_FORMS))
def test_metric_dispatch_forms_with_ragged_batches(L):
    rng = np.random.default_rng(L)
    B, T = (3, 5) if L > 1000 else (6, 9)
    preds, rele, lens, nts = _batch(rng, B, T, L, density=0.05, graded=True)
    rele[1] = 0.0                                                                # valid = 0
    lens[2] = 7                                                                  # cut-offs beyond the list: 0
    ks = [1, 5, 10, 20, 7, L]                                                    # unsorted on purpose
    a, e, ne, v = run_metrics(preds, rele, ks, max_label=3.0, lens=lens, ntopics=nts)
    wa, we, wn, wv = DR.div_metrics_batch(preds, rele, ks, max_label=3.0, lens=lens, ntopics=nts)
    GU.assert_close(a, wa, "alpha-nDCG"); GU.assert_close(e, we, "ERR-IA"); GU.assert_close(ne, wn, "nERR-IA")
    assert np.array_equal(v, wv) and v[1] == 0 and not a[1].any()
    assert a[2, 2] == 0.0 and a[2, 3] == 0.0 and a[2, 5] == 0.0 and e[2, 3] == 0.0 and ne[2, 5] == 0.0


# ---------------------------------------------------------------------------------------------------------------- 11. the ranker
F_DIM = 8
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=F_DIM, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False,
                      dropout=0.0)}


def _make(lr=1e-3, seed=21):
    import ptranking_amd as pa
    torch.manual_seed(seed)
    sf = copy.deepcopy(SF)
    sf["lr"] = lr
    r = pa.DALETOR(sf_para_dict=sf, model_para_dict=dict(pa.diversity.DEFAULT_DIV_PARAS["DALETOR"]), gpu=True, device="cuda:0")
    r.init()
    return r


def _query(rng, n, T, density=0.2):
    """One synthetic query in the reference's 7-tuple form: the first T document features carry the (noisy) subtopic relevance."""
    R = (rng.random((T, n)) < density).astype(np.float32)
    R = R[:, np.argsort(-R.sum(axis=0), kind="stable")]                          # presort: most-covering documents first
    d = (0.5 * rng.standard_normal((n, F_DIM))).astype(np.float32)
    d[:, :min(T, F_DIM)] += R.T[:, :F_DIM]
    q = rng.standard_normal((1, F_DIM)).astype(np.float32)
    return (f"q{n}_{T}", torch.from_numpy(q), [f"d{i}" for i in range(n)], torch.from_numpy(d), 0.0, {}, torch.from_numpy(np.ascontiguousarray(R)))


def _query_set(nq=300, seed=5):
    rng = np.random.default_rng(seed)
    data = [_query(rng, int(rng.integers(5, 61)), int(rng.integers(2, 9))) for _ in range(nq)]
    invalid = sum(float(item[6].sum()) < 1.0 for item in data)
    assert invalid <= 0.1 * nq, f"{invalid} of {nq} generated queries have no relevant document"
    return data


class _OneQueryData(list):
    presort = True


def test_one_query_calls_equal_the_batched_path_bit_for_bit():
    """The reference-shaped one-query calls and a DivQueryBatches of that one query (32 documents: a multiple of the padding granule 16, so
    both run the scorer on the same rows) leave bit-identical parameters after three steps."""
    import ptranking_amd as pa
    from ptranking_amd.scorer import FusedPointScorer
    item = _query(np.random.default_rng(3), 32, 5)
    a, b = _make(), _make()
    assert isinstance(a.point_sf, FusedPointScorer) and a.point_sf.num_features == 3 * F_DIM
    assert torch.equal(a.point_sf.flat, b.point_sf.flat)
    batches = pa.DivQueryBatches([item], "cuda:0", pad_to=16)
    a.train_mode()
    losses_a, losses_b = [], []
    for _ in range(3):
        loss, stop = a.div_train_op(item[1].cuda(), item[3].cuda(), item[6].cuda(), presort=True)
        losses_a.append(float(loss))
        ep, stop_b = b.div_train(batches)
        losses_b.append(float(ep))
        assert stop is False and stop_b is False
    assert losses_a == losses_b
    assert torch.equal(a.point_sf.flat, b.point_sf.flat)
    # the reference's epoch loop over one-query data takes the same steps
    c = _make()
    for _ in range(3):
        c.div_train(_OneQueryData([item]), epoch_k=1)
    assert torch.equal(a.point_sf.flat, c.point_sf.flat)
    # evaluation: the one-query form and the batched form agree
    for m in ("alpha_ndcg_at_k", "alpha_ndcg_at_ks"):
        assert torch.equal(getattr(a, m)(_OneQueryData([item])), getattr(a, m)(batches))
    assert torch.equal(a.div_validation(_OneQueryData([item]), "nERR-IA", k=5, max_label=1.0), a.nerr_ia_at_k(batches, k=5, max_label=1.0))


def test_batched_evaluation_equals_the_per_query_average_and_training_improves():
    import ptranking_amd as pa
    data = _query_set()
    batches = pa.DivQueryBatches(data, "cuda:0", rough_batch_size=1024, pad_to=16)
    assert batches.num_queries == len(data) and len(batches) > 4
    r = _make(lr=2e-3)
    ks = [1, 5, 10, 20]

    def per_query_average(min_len=None):
        sums, cnt = np.zeros((3, len(ks))), 0
        r.eval_mode()
        with torch.no_grad():
            for ids, X, rele, lens, nts in batches:
                preds = r._score_batch(X, lens).cpu().numpy()
                for q in range(len(ids)):
                    n, nt = int(lens[q]), int(nts[q])
                    a, e, ne, valid = DR.div_metrics(preds[q, :n], rele[q, :nt, :n].cpu().numpy(), ks, 0.5, 1.0)
                    if valid and (min_len is None or n >= min_len):
                        sums += np.stack([a, e, ne]); cnt += 1
        return sums / cnt, cnt

    want, cnt = per_query_average()
    assert cnt >= 0.9 * len(data)
    got = r.srd_performance_at_ks(test_data=batches, ks=ks, max_label=1.0)
    for g, w, name in zip(got, want, ("alpha-nDCG", "ERR-IA", "nERR-IA")):
        assert g.shape == (len(ks),) and g.device.type == "cpu"
        GU.assert_close(g.numpy(), w, name)
    want10, cnt10 = per_query_average(min_len=10)
    assert cnt10 < cnt                                                           # some queries are shorter than the cut-off
    GU.assert_close(r.alpha_ndcg_at_k(batches, k=10).numpy(), want10[0, 2:3], "alpha-nDCG@10 (queries with >= 10 documents)")
    GU.assert_close(r.err_ia_at_k(batches, k=10, max_label=1.0).numpy(), want10[1, 2:3], "ERR-IA@10")
    before = float(r.alpha_ndcg_at_k(batches, k=10))
    first = None
    for epoch in range(15):
        loss, stop = r.div_train(batches, epoch_k=epoch + 1)
        assert stop is False and torch.isfinite(loss).all()
        first = float(loss) if first is None else first
    after = float(r.alpha_ndcg_at_k(batches, k=10))
    print(f"alpha-nDCG@10 on the training set: {before:.4f} -> {after:.4f}; epoch loss {first:.4f} -> {float(loss):.4f}")
    assert after > before and float(loss) < first


# ---------------------------------------------------------------------------------------------------------------- 12. data parallel
def _dp_batch():
    import ptranking_amd as pa
    data = _query_set(nq=24, seed=8)
    (batch,) = list(pa.DivQueryBatches(data, "cuda:0", rough_batch_size=1 << 20, pad_to=64))
    return batch


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      PTR_DP_BACKEND="gloo")
    from ptranking_amd import dp
    dp.init_from_env()
    ids, X, rele, lens, nts = _dp_batch()
    lo, hi = dp.shard_queries(X.size(0))
    r = _make()
    r.train_mode()
    loss = r.div_custom_loss_function(r._score_batch(X[lo:hi], lens[lo:hi]), rele[lo:hi], presort=True, lens=lens[lo:hi], ntopics=nts[lo:hi])
    torch.save({"grads": r.point_sf.flat.grad.detach().cpu().clone(), "flat": r.point_sf.flat.detach().cpu(), "loss": float(loss)},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_match_the_full_batch(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{i}.pt") for i in range(2))
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["grads"], r1["grads"]), "replicas diverged"
    ids, X, rele, lens, nts = _dp_batch()
    r = _make()
    r.train_mode()
    loss = r.div_custom_loss_function(r._score_batch(X, lens), rele, presort=True, lens=lens, ntopics=nts)
    GU.assert_close(r0["grads"].numpy(), r.point_sf.flat.grad.detach().cpu().numpy(), "all-reduced gradient vs full batch")
    GU.assert_close(r0["loss"] + r1["loss"], float(loss), "loss")
