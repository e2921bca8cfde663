"""GPU: DivProbRanker on the real kernel — ptr_divprob_fwd_bwd against the reference's float64 results (tests/golden/divprob.npz) where the
reference is well conditioned, against the exact definition (tests/divprob_ref.py, `stable`) where its `1 - erfc(x) / 2` arithmetic is not, and
against the same restatement for everything the reference cannot run (batches, padding, the document cut-off); ptr_divprob_expected_ranks; the
DivProbRanker class in one-query and batched form, the data-parallel step and a short training run per objective.

Dispatch forms of the loss kernel (csrc/divprob.hip): threads per query G = 64 (four queries per workgroup: L <= 128 and four tiles fit in
LDS) or 256, times the subtopic tile TP = 4 / 8 / 16 / 32 (T rounded up), times the four objectives — 32 instantiations, each hit by FORMS
below, plus the documented LDS limit of every objective (LIMITS).

Yardstick of the pairwise objectives: the restatement `stable` in float64 is the target; what fp32 arithmetic itself needs of golden_util's
element-wise gate is measured by evaluating the SAME restatement in fp32 with torch on the CPU, and the kernel may need at most
max(1, 2 x that) — per case and per quantity (loss, grad_mu, grad_var).  The yardstick is computed here, never from the kernel.
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

import divprob_ref as DR
import golden_util as GU
from launch_form import group_form

pytestmark = pytest.mark.gpu

GOLD = GU._load("divprob.npz")
NAMES = {0: "aNDCG", 1: "nERR-IA", 2: "PairCLS", 3: "LambdaPairCLS"}


def rows(fams, objectives):
    return [(f, s, r) for f in fams for s in sorted(GOLD[f]) for r, (o, _, _) in enumerate(GOLD[f][s]["combos"]) if int(o) in objectives]


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def run_loss(mus, vars_, rele, objective, beta=0.5, top_k=None, axis=0, max_label=1.0, norm=True, lens=None, ntopics=None):
    """ptr_divprob_fwd_bwd through the ctypes binding -> (loss_out, loss_q [B], grad_mu [B, L], grad_var [B, L]) as numpy."""
    from ptranking_amd import _lib
    import ptranking_amd.functional as F_
    m, v, r = dev(mus), dev(vars_), dev(rele)
    B, T, L = r.shape
    ld, td = dev(lens, torch.int32), dev(ntopics, torch.int32)
    nan = lambda *shape: torch.full(shape, np.nan).cuda()
    loss, loss_q, gm, gv = nan(1), nan(B), nan(B, L), nan(B, L)
    _lib.call("ptr_divprob_fwd_bwd", _lib.ptr(m), _lib.ptr(v), _lib.ptr(r), _lib.ptr(ld), _lib.ptr(td), B, T, L, F_.DIVPROB_OBJECTIVES[objective],
              C.c_float(beta), int(top_k or 0), int(axis), C.c_float(max_label), int(bool(norm)), _lib.ptr(loss), _lib.ptr(loss_q), _lib.ptr(gm),
              _lib.ptr(gv), _lib.current_stream(m.device))
    torch.cuda.synchronize()
    return float(loss.item()), loss_q.cpu().numpy(), gm.cpu().numpy(), gv.cpu().numpy()


def golden_case(fam, shape, row):
    c = GOLD[fam][shape]
    obj, top_k, norm = (int(x) for x in c["combos"][row])
    L = c["mus"].shape[0]
    kw = dict(top_k=top_k or None, norm=bool(norm), max_label=float(c["max_label"]) if fam == "a" else 1.0)
    r64 = c["res64"][row]
    return c, NAMES[obj], kw, (float(r64[0]), r64[1:1 + L], r64[1 + L:])


def check_against_stable(what, got, mus, vars_, rele, objective, lens=None, ntopics=None, **kw):
    """got = (loss_q [B], grad_mu [B, L], grad_var [B, L]) of the kernel against `stable` in float64 under max(1, 2 x the need of `stable` in fp32)."""
    want = DR.batch("stable", mus, vars_, rele, objective, lens=lens, ntopics=ntopics, **kw)
    yard = DR.batch("stable", mus, vars_, rele, objective, lens=lens, ntopics=ntopics, dtype=torch.float32, **kw)
    worst = 0.0
    for name, g, w, y in zip(("loss_q", "grad_mu", "grad_var"), got, want, yard):
        assert np.isfinite(g).all(), f"{what} {name}: not finite"
        mine, fp32 = DR.need(g, w), DR.need(y, w)
        print(f"{what} {name}: kernel need {mine:.3f}, fp32 torch need {fp32:.3f}")
        assert mine <= max(1.0, 2.0 * fp32), f"{what} {name}: the kernel needs {mine:.3f} of the element-wise gate, fp32 arithmetic itself {fp32:.3f}"
        worst = max(worst, mine)
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1. golden cases
@pytest.mark.parametrize("fam,shape,row", rows("a", (0, 1)) + rows("b", (2, 3)))
def test_golden_against_the_reference_float64(fam, shape, row):
    """Family (a) SuperSoft and family (b): B = 1 against the reference's float64 loss and gradients under the max-norm and the element-wise
    1e-5 gate (tests/test_divprob_cpu.py asserts that the reference's OWN fp32 passes that gate on family (b))."""
    c, objective, kw, (l64, gm64, gv64) = golden_case(fam, shape, row)
    loss, loss_q, gm, gv = run_loss(c["mus"][None], c["vars"][None], c["rele"][None], objective, **kw)
    print(f"{shape}[{row}] {objective}: kernel need loss {DR.need([loss], [l64]):.3f} grad_mu {DR.need(gm[0], gm64):.3f} grad_var {DR.need(gv[0], gv64):.3f}")
    GU.assert_close(loss, l64, "loss")
    GU.assert_close(loss_q[0], l64, "loss_q")
    GU.assert_close(gm[0], gm64, "grad_mu")
    GU.assert_close(gv[0], gv64, "grad_var")


@pytest.mark.parametrize("fam,shape,row", rows("a", (2, 3)) + rows("c", (2, 3)))
def test_golden_pairwise_against_the_exact_definition(fam, shape, row):
    """Family (a) pairwise (variances 0.1 sigmoid: saturated) and family (c): the reference's fp32 and float64 are artefacts of the 1e-12 floor
    of F.binary_cross_entropy there, so the target is `stable` in float64.  The needs are printed before they are asserted (COVERAGE.md row f-7)."""
    c, objective, kw, _ = golden_case(fam, shape, row)
    _, loss_q, gm, gv = run_loss(c["mus"][None], c["vars"][None], c["rele"][None], objective, **kw)
    check_against_stable(f"{shape}[{row}] {objective}", (loss_q, gm, gv), c["mus"][None], c["vars"][None], c["rele"][None].astype(np.float64),
                         objective, **kw)


# ---------------------------------------------------------------------------------------------------------------- 2. batches and padding
def _batch(rng, B, T, L, density=0.15, graded=False, ragged=True, var=(0.05, 1.0)):
    mus = rng.standard_normal((B, L)).astype(np.float32)
    vars_ = rng.uniform(var[0], var[1], (B, L)).astype(np.float32)
    rele = (rng.random((B, T, L)) < density).astype(np.float32)
    if graded:
        rele *= rng.integers(1, 4, size=rele.shape).astype(np.float32)
    lens = rng.integers(max(1, L // 3), L + 1, size=B).astype(np.int32) if ragged else np.full(B, L, np.int32)
    nts = rng.integers(1, T + 1, size=B).astype(np.int32) if ragged else np.full(B, T, np.int32)
    lens[0], nts[0] = L, T
    return mus, vars_, rele, lens, nts


# objective -> (T, L) cases: every (G, TP) of every objective; LambdaPairCLS at T = 32, L = 128 is the list of <= 128 documents whose four
# tiles do not fit, served by G = 256
FORMS = [(obj, T, L) for obj in range(4) for T, L in ((3, 40), (7, 100), (12, 128), (30, 64), (4, 200), (8, 300), (16, 260), (32, 140))]
FORMS += [(3, 32, 128)]


def test_forms_cover_every_instantiation():
    form = lambda obj, T, L: group_form("ptr_divprob_fwd_bwd", obj, T, L)           # (G, TP) the entry point launches
    assert {(obj,) + form(obj, T, L) for obj, T, L in FORMS} == {(obj, G, TP) for obj in range(4) for G in (64, 256) for TP in (4, 8, 16, 32)}
    assert form(3, 32, 128) == (256, 32) and form(3, 30, 64) == (64, 32)


def _check_forms_case(obj, T, L, B, axis, seed, density=0.15):
    objective = NAMES[obj]
    rng = np.random.default_rng(seed)
    mus, vars_, rele, lens, nts = _batch(rng, B, T, L, density=density, graded=(T + L) % 2 == 0)
    if B > 2:
        nts[2] = 0                                                               # a query without a subtopic contributes exactly 0
    kw = dict(top_k=6, top_k_axis=axis, max_label=3.0 if (T + L) % 2 == 0 else 1.0, norm=bool((T + L) % 3))
    jm, jv, jr = mus.copy(), vars_.copy(), rele.copy()
    for q in range(B):
        jm[q, lens[q]:], jv[q, lens[q]:] = np.nan, np.nan
        jr[q, nts[q]:, :], jr[q, :, lens[q]:] = np.nan, np.nan
    loss, loss_q, gm, gv = run_loss(jm, jv, jr, objective, top_k=6, axis=axis, max_label=kw["max_label"], norm=kw["norm"], lens=lens, ntopics=nts)
    what = f"{objective} T={T} L={L} axis={axis}"
    if obj < 2:
        want = DR.batch("stable", mus, vars_, rele, objective, lens=lens, ntopics=nts, **kw)
        print(f"{what}: kernel need " + " ".join(f"{DR.need(g, w):.3f}" for g, w in zip((loss_q, gm, gv), want)))
        for name, g, w in zip(("loss_q", "grad_mu", "grad_var"), (loss_q, gm, gv), want):
            GU.assert_close(g, w, f"{what} {name}")
    else:
        check_against_stable(what, (loss_q, gm, gv), mus, vars_, rele, objective, lens=lens, ntopics=nts, **kw)
    GU.assert_close(loss, loss_q.astype(np.float64).sum(), "loss_out")
    for q in range(B):
        assert not gm[q, lens[q]:].any() and not gv[q, lens[q]:].any() and np.isfinite(gm[q]).all() and np.isfinite(gv[q]).all()
    if B > 2:
        assert loss_q[2] == 0.0 and not gm[2].any() and not gv[2].any()
    clean = run_loss(mus, vars_, rele, objective, top_k=6, axis=axis, max_label=kw["max_label"], norm=kw["norm"], lens=lens, ntopics=nts)
    assert clean[0] == loss and all(np.array_equal(a, b) for a, b in zip(clean[1:], (loss_q, gm, gv)))     # garbage changes no bit


@pytest.mark.parametrize("obj,T,L", FORMS)
def test_every_dispatch_form_with_ragged_batches(obj, T, L):
    """Ragged lens and ntopics, NaN in every padded slot, graded relevance, B not a multiple of the four queries per workgroup, the document
    cut-off (the axis only the restatement can run): losses and real gradients equal the float64 restatement, padded gradients are exactly 0."""
    _check_forms_case(obj, T, L, B=7, axis=1 if obj == 0 else 0, seed=1000 * T + L + obj)


# the documented LDS limit of every objective (include/ptranking_amd.h), one subtopic tile each
LIMITS = [(1, 4, 4096), (2, 32, 1168), (0, 32, 608), (0, 8, 2152), (3, 32, 412), (3, 4, 2728)]


@pytest.mark.parametrize("obj,T,L", LIMITS)
def test_one_case_at_each_lds_limit_and_one_beyond(obj, T, L):
    from ptranking_amd import _lib
    _check_forms_case(obj, T, L, B=1, axis=0, seed=L + obj, density=0.04)
    if L < 4096:
        with pytest.raises(RuntimeError, match="LDS"):
            run_loss(np.zeros((1, L + 1), np.float32), np.ones((1, L + 1), np.float32), np.zeros((1, T, L + 1), np.float32), NAMES[obj])
    else:
        with pytest.raises(ValueError, match="exceeds the supported maximum"):
            import ptranking_amd.functional as F_
            F_.divprob_loss(torch.zeros(1, L + 1).cuda(), torch.ones(1, L + 1).cuda(), torch.zeros(1, T, L + 1).cuda(), NAMES[obj])
    assert _lib.MAX_LIST_LEN == 4096


@pytest.mark.parametrize("objective", DR.OBJECTIVES)
@pytest.mark.parametrize("T,L", [(6, 96), (6, 320)])
def test_a_query_alone_and_inside_a_batch_is_bit_identical_and_runs_repeat(objective, T, L):
    rng = np.random.default_rng(L)
    mus, vars_, rele, lens, nts = _batch(rng, 9, T, L)
    full = run_loss(mus, vars_, rele, objective, lens=lens, ntopics=nts)
    again = run_loss(mus, vars_, rele, objective, lens=lens, ntopics=nts)
    assert full[0] == again[0] and all(np.array_equal(a, b) for a, b in zip(full[1:], again[1:]))
    for q in (0, 3, 8):
        _, lq, gm, gv = run_loss(mus[q:q + 1], vars_[q:q + 1], rele[q:q + 1], objective, lens=lens[q:q + 1], ntopics=nts[q:q + 1])
        assert lq[0] == full[1][q] and np.array_equal(gm[0], full[2][q]) and np.array_equal(gv[0], full[3][q])
    a = run_loss(mus, vars_, rele, objective)                                    # lens / ntopics NULL == every slot real
    b = run_loss(mus, vars_, rele, objective, lens=np.full(9, L, np.int32), ntopics=np.full(9, T, np.int32))
    assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_other_beta_and_the_reference_axis_in_a_batch():
    rng = np.random.default_rng(78)
    mus, vars_, rele, lens, nts = _batch(rng, 5, 9, 48)
    b32 = float(np.float32(0.3))
    for axis in (0, 1):
        want = DR.batch("stable", mus, vars_, rele, "aNDCG", lens=lens, ntopics=nts, beta=b32, top_k=3, top_k_axis=axis)
        _, loss_q, gm, gv = run_loss(mus, vars_, rele, "aNDCG", beta=0.3, top_k=3, axis=axis, lens=lens, ntopics=nts)
        for g, w in zip((loss_q, gm, gv), want):
            GU.assert_close(g, w, f"axis {axis}")
    want = DR.batch("stable", mus, vars_, rele, "LambdaPairCLS", lens=lens, ntopics=nts, beta=b32, norm=False)
    _, loss_q, gm, gv = run_loss(mus, vars_, rele, "LambdaPairCLS", beta=0.3, norm=False, lens=lens, ntopics=nts)
    check_against_stable("beta 0.3 LambdaPairCLS", (loss_q, gm, gv), mus, vars_, rele, "LambdaPairCLS", lens=lens, ntopics=nts, beta=b32, norm=False)


# ---------------------------------------------------------------------------------------------------------------- 3. autograd, expected ranks
@pytest.mark.parametrize("objective", DR.OBJECTIVES)
def test_autograd_scales_both_kernel_gradients(objective):
    import ptranking_amd.functional as F_
    rng = np.random.default_rng(9)
    mus, vars_, rele, lens, nts = _batch(rng, 6, 5, 50)
    _, loss_q, gm, gv = run_loss(mus, vars_, rele, objective, top_k=4, axis=1, lens=lens, ntopics=nts)
    m, v = dev(mus).requires_grad_(True), dev(vars_).requires_grad_(True)
    loss, lq = F_.divprob_loss(m, v, dev(rele), objective, top_k=4, top_k_axis="documents", lens=dev(lens, torch.int32), ntopics=dev(nts, torch.int32),
                               return_loss_q=True)
    (loss * 3.0).backward()
    assert np.array_equal(lq.cpu().numpy(), loss_q)
    assert np.array_equal(m.grad.cpu().numpy(), gm * np.float32(3.0)) and np.array_equal(v.grad.cpu().numpy(), gv * np.float32(3.0))
    GU.assert_close(loss.item(), loss_q.astype(np.float64).sum(), "loss")
    assert not F_.divprob_loss(dev(mus), dev(vars_), dev(rele), objective).requires_grad
    # through a head: the variance as exp of a leaf
    raw = dev(np.log(vars_)).requires_grad_(True)
    F_.divprob_loss(dev(mus), raw.exp(), dev(rele), objective, top_k=4, top_k_axis="documents", lens=dev(lens, torch.int32),
                    ntopics=dev(nts, torch.int32)).backward()
    GU.assert_close(raw.grad.cpu().numpy(), gv.astype(np.float64) * vars_.astype(np.float64), "chain rule through exp")


@pytest.mark.parametrize("L", [1, 40, 100, 130, 700, 4096])
def test_expected_ranks_against_float64_and_the_rerar_order(L):
    import ptranking_amd.functional as F_
    rng = np.random.default_rng(L)
    B = 5 if L <= 1000 else 2
    mus, vars_, _, lens, _ = _batch(rng, B, 1, L)
    jm, jv = mus.copy(), vars_.copy()
    for q in range(B):
        jm[q, lens[q]:], jv[q, lens[q]:] = np.nan, np.nan
    got = F_.expected_ranks(dev(jm), dev(jv), lens=dev(lens, torch.int32)).cpu().numpy()
    for q in range(B):
        n = int(lens[q])
        want = DR.expected_ranks(mus[q, :n], vars_[q, :n])
        GU.assert_close(got[q, :n], want, f"query {q}")
        assert not got[q, n:].any()
        assert abs(got[q, :n].astype(np.float64).sum() - n * (n + 1) / 2) <= 1e-5 * n * (n + 1) / 2     # Phi[i][j] + Phi[j][i] = 1
    full = F_.expected_ranks(dev(mus), dev(vars_)).cpu().numpy()
    GU.assert_close(full[0], DR.expected_ranks(mus[0], vars_[0]), "lens NULL")


# ---------------------------------------------------------------------------------------------------------------- 4. the ranker
F_DIM = 8
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=F_DIM, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False,
                      dropout=0.0)}
CONFIGS = {"aNDCG": dict(opt_id="SuperSoft", metric="aNDCG", top_k=10), "nERR-IA": dict(opt_id="SuperSoft", metric="nERR-IA", top_k=None),
           "PairCLS": dict(opt_id="PairCLS"), "LambdaPairCLS": dict(opt_id="LambdaPairCLS", norm=True)}


def _make(lr=1e-3, seed=21, **over):
    import ptranking_amd as pa
    torch.manual_seed(seed)
    sf = copy.deepcopy(SF)
    sf["lr"] = lr
    paras = {**pa.diversity.DEFAULT_DIV_PARAS["DivProbRanker"], "limit_delta": 0.1, **over}
    r = pa.DivProbRanker(sf_para_dict=sf, model_para_dict=paras, gpu=True, device="cuda:0")
    r.init()
    return r


def _params(r):
    return torch.cat([p.detach().reshape(-1) for p in r.get_parameters()])


def _grads(r):
    return torch.cat([p.grad.detach().reshape(-1) for p in r.get_parameters()])


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
    return [_query(rng, int(rng.integers(5, 61)), int(rng.integers(2, 9))) for _ in range(nq)]


class _OneQueryData(list):
    presort = True


@pytest.mark.parametrize("objective,K", [("aNDCG", 1), ("nERR-IA", 3), ("PairCLS", 1), ("LambdaPairCLS", 3)])
def test_one_query_calls_equal_the_batched_path_bit_for_bit(objective, K):
    """The reference-shaped one-query calls and a DivQueryBatches of that one query (32 documents: a multiple of the padding granule 16, so
    both run the scorer on the same rows) leave bit-identical parameters after three steps."""
    import ptranking_amd as pa
    item = _query(np.random.default_rng(3), 32, 5)
    a, b = _make(K=K, **CONFIGS[objective]), _make(K=K, **CONFIGS[objective])
    assert type(a.point_sf).__name__ == "FusedStack"                             # out_dim = 2 / 3 K: the layer-wise stack on the hand-written GEMMs
    assert torch.equal(_params(a), _params(b))
    batches = pa.DivQueryBatches([item], "cuda:0", pad_to=16)
    a.train_mode()
    losses_a, losses_b = [], []
    for _ in range(3):
        loss, stop = a.div_train_op(item[1].cuda(), item[3].cuda(), item[6].cuda(), presort=True)
        losses_a.append(float(loss))
        ep, stop_b = b.div_train(batches)
        losses_b.append(float(ep))
        assert stop is False and stop_b is False
    assert losses_a == losses_b and np.isfinite(losses_a).all()
    assert torch.equal(_params(a), _params(b))
    c = _make(K=K, **CONFIGS[objective])                                         # the reference's epoch loop over one-query data takes the same steps
    for _ in range(3):
        c.div_train(_OneQueryData([item]), epoch_k=1)
    assert torch.equal(_params(a), _params(c))
    for sort_id in ("ExpRele", "RiskAware", "RERAR"):                            # evaluation: the one-query form and the batched form agree
        a.sort_id = sort_id
        for m in ("alpha_ndcg_at_k", "alpha_ndcg_at_ks"):
            assert torch.equal(getattr(a, m)(_OneQueryData([item])), getattr(a, m)(batches))
        assert torch.equal(a.div_validation(_OneQueryData([item]), "nERR-IA", k=5, max_label=1.0), a.nerr_ia_at_k(batches, k=5, max_label=1.0))


def test_rerar_scores_rank_by_expected_rank():
    r = _make(sort_id="RERAR")
    r.eval_mode()
    item = _query(np.random.default_rng(4), 40, 5)
    with torch.no_grad():
        mus, vars_ = r.div_forward(item[1].cuda(), item[3].cuda())
        scores = r.div_predict(item[1].cuda(), item[3].cuda())
    want = DR.expected_ranks(mus.cpu().numpy()[0], vars_.cpu().numpy()[0])
    GU.assert_close(scores.cpu().numpy()[0], 1.0 / want, "1 / expected rank")
    assert np.array_equal(np.argsort(-scores.cpu().numpy()[0], kind="stable"), np.argsort(want, kind="stable"))


def test_batched_evaluation_equals_the_per_query_average():
    import ptranking_amd as pa
    import diversity_ref as MR
    data = _query_set()
    batches = pa.DivQueryBatches(data, "cuda:0", rough_batch_size=1024, pad_to=16)
    assert batches.num_queries == len(data) and len(batches) > 4
    ks = [1, 5, 10, 20]
    for sort_id in ("ExpRele", "RERAR"):
        r = _make(sort_id=sort_id, K=3)
        sums, cnt = np.zeros((3, len(ks))), 0
        r.eval_mode()
        with torch.no_grad():
            for ids, X, rele, lens, nts in batches:
                scores = r._batch_sort_scores(X, lens).cpu().numpy()
                for q in range(len(ids)):
                    n, nt = int(lens[q]), int(nts[q])
                    a, e, ne, valid = MR.div_metrics(scores[q, :n], rele[q, :nt, :n].cpu().numpy(), ks, 0.5, 1.0)
                    if valid:
                        sums += np.stack([a, e, ne]); cnt += 1
        assert cnt >= 0.9 * len(data)
        got = r.srd_performance_at_ks(test_data=batches, ks=ks, max_label=1.0)
        for g, w, name in zip(got, sums / cnt, ("alpha-nDCG", "ERR-IA", "nERR-IA")):
            assert g.shape == (len(ks),) and g.device.type == "cpu"
            GU.assert_close(g.numpy(), w, f"{sort_id} {name}")


@pytest.mark.parametrize("objective", DR.OBJECTIVES)
def test_twenty_training_steps_lower_the_loss(objective):
    """20 steps on ONE padded batch of a synthetic DivQueryBatches: the loss of the batch goes down."""
    import ptranking_amd as pa
    data = _query_set(nq=64, seed=6)
    batches = pa.DivQueryBatches(data, "cuda:0", rough_batch_size=1 << 20, pad_to=64)
    assert len(batches) == 1
    r = _make(lr=2e-3, **CONFIGS[objective])
    losses = []
    for step in range(20):
        loss, stop = r.div_train(batches, epoch_k=step + 1)
        assert stop is False and torch.isfinite(loss).all()
        losses.append(float(loss))
    print(f"{objective}: loss {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert losses[-1] < losses[0]


def test_the_example_runs_and_reports_finite_metrics():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "train_divprob_synthetic.py"), "--queries", "120", "--epochs", "5",
                          "--opt-id", "LambdaPairCLS", "--K", "2", "--sort-id", "RERAR"], cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("alpha-nDCG@")]
    assert len(lines) == 3 and "nan" not in out.stdout.lower(), out.stdout


# ---------------------------------------------------------------------------------------------------------------- 5. data parallel
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
    r = _make(**CONFIGS["LambdaPairCLS"])
    r.train_mode()
    loss = r.div_custom_loss_function(*r._batch_outputs(X[lo:hi], lens[lo:hi]), rele[lo:hi], presort=True, lens=lens[lo:hi], ntopics=nts[lo:hi])
    torch.save({"grads": _grads(r).cpu().clone(), "flat": _params(r).cpu(), "loss": float(loss)}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_match_the_full_batch(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{i}.pt") for i in range(2))
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["grads"], r1["grads"]), "replicas diverged"
    ids, X, rele, lens, nts = _dp_batch()
    r = _make(**CONFIGS["LambdaPairCLS"])
    r.train_mode()
    loss = r.div_custom_loss_function(*r._batch_outputs(X, lens), rele, presort=True, lens=lens, ntopics=nts)
    GU.assert_close(r0["grads"].numpy(), _grads(r).cpu().numpy(), "all-reduced gradient vs full batch")
    GU.assert_close(r0["loss"] + r1["loss"], float(loss), "loss")
