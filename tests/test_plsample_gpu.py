"""GPU: the device Plackett-Luce sampler and the fused multi-sample MDPRank loss (csrc/plsample.hip) through the C ABI — parity with the
reference's own runs (tests/golden/plsample.npz), every dispatch form against the float64 restatement (tests/plsample_ref.py) under the
element-wise bound at C_LIST, fused against composed, the identities of the counter stream, the law of the draws, underflow, the ranker.

The rankings must equal the restatement's EXACTLY; float64 pins a ranking only when no two adjacent sorted keys are closer than 2^-16 max|key|.
The uniforms of the documents that violate it are drawn again on the host before the kernel sees them (plsample_ref.redraw; a whole-list
redraw cannot work from a few hundred documents on: 4096 keys always hold hundreds of pairs closer than that), and each test prints how many."""
import copy
import ctypes as C
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import plsample_ref as PR
from f64_loss_bounds import C_LIST, batch_total, gate_losses, gate_nan
from golden_util import _load, assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST = {"PL": 0, "STPL": 1}


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


def c_sample(preds, lens, S, T, dist, seed=0, q0=0, unif=None, want_action=True):
    """ptr_pl_sample -> (perm int64 [B, S, L], action fp32 [B, S, L] or None) as numpy."""
    from ptranking_amd import _lib
    p, n, u = dev(preds, torch.float32), dev(lens, torch.int32), dev(unif, torch.float32)
    B, L = p.shape
    perm = torch.full((B, S, L), -7, dtype=torch.int64, device="cuda")
    act = torch.full((B, S, L), -7.0, device="cuda") if want_action else None
    _lib.call("ptr_pl_sample", _lib.ptr(p), _lib.ptr(n), B, L, S, C.c_float(T), DIST[dist], C.c_uint64(seed), C.c_int64(q0), _lib.ptr(u),
              _lib.ptr(perm), _lib.ptr(act), _lib.current_stream(p.device))
    return perm.cpu().numpy(), (act.cpu().numpy() if want_action else None)


def c_fused(preds, labels, lens, S, top_k, gamma, T, dist, seed=0, q0=0, unif=None, want_perm=True):
    """ptr_mdprank_sample_fwd_bwd -> (loss_out, loss_q [B], grad [B, L], perm or None) as numpy."""
    from ptranking_amd import _lib
    p, y, n, u = dev(preds, torch.float32), dev(labels, torch.float32), dev(lens, torch.int32), dev(unif, torch.float32)
    B, L = p.shape
    out, lq, grad = torch.full((1,), -7.0, device="cuda"), torch.full((B,), -7.0, device="cuda"), torch.full((B, L), -7.0, device="cuda")
    perm = torch.full((B, S, L), -7, dtype=torch.int64, device="cuda") if want_perm else None
    _lib.call("ptr_mdprank_sample_fwd_bwd", _lib.ptr(p), _lib.ptr(y), _lib.ptr(n), B, L, S, int(top_k or 0), C.c_float(gamma), C.c_float(T),
              DIST[dist], C.c_uint64(seed), C.c_int64(q0), _lib.ptr(u), _lib.ptr(out), _lib.ptr(lq), _lib.ptr(grad), _lib.ptr(perm),
              _lib.current_stream(p.device))
    return float(out.cpu()[0]), lq.cpu().numpy(), grad.cpu().numpy(), (perm.cpu().numpy() if want_perm else None)


def c_uniforms(B, L, S, seed, q0=0):
    import ptranking_amd.functional as F
    return F.pl_uniforms(B, L, samples=S, seed=seed, q0=q0)


# ---------------------------------------------------------------------------------------------------------------- parity with the reference
@pytest.fixture(scope="module")
def golden():
    return _load("plsample.npz")


def test_sampler_reproduces_every_reference_fixture(golden):
    for name, c in sorted(golden["sampler"].items()):
        T = float(c["temperature"])
        perm, act = c_sample(c["preds"], None, c["unif"].shape[0], T, "STPL", unif=c["unif"][None])
        assert np.array_equal(perm[0], c["inds"]), name
        if not int(c["only_indices"]):
            assert_close(act[0], c["logits"], name)


def test_fused_loss_reproduces_every_reference_fixture(golden):
    for name, c in sorted(golden["mdprank"].items()):
        total, lq, grad, perm = c_fused(c["preds"], c["labels"], None, 1, int(c["top_k"]), float(c["gamma"]), float(c["temperature"]), "STPL",
                                        unif=c["unif"][None])
        assert np.array_equal(perm[:, 0], c["perm"]), name
        assert_close(np.array([total]), np.array([c["loss"]]), name + " loss")
        assert_close(lq, np.array([c["loss"]]), name + " loss_q")
        assert_close(grad, c["grad"], name + " grad")


# ---------------------------------------------------------------------------------------------------------------- every dispatch form
LENS17 = [0, 1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1251, 2048, 4096]
# one batch per register-sort width (64, 128, 256, 512, 1024 documents: DPT 1, 2, 4, 8, 16) and per workgroup width (2048, 4096 above),
# plus two widths that are no multiple of 4 (the scalar load / store routes)
WIDTHS = (64, 128, 130, 256, 512, 1024, 1027, 2048)
_BATCHES = {}


def batch(L):
    """(preds, labels, lens) fp32 / int32 on the host, NaN beyond every list's length; the last list holds a NaN SCORE (L != 4096)."""
    if L not in _BATCHES:
        g = np.random.default_rng(1000 + L)
        lens = LENS17 if L == 4096 else [L, L - 1, L // 2 + 1, 3, 0, 1, L // 2]
        B = len(lens)
        preds = (1.5 * g.standard_normal((B, L))).astype(np.float32)
        labels = -np.sort(-g.choice(5, size=(B, L), p=[0.5, 0.3, 0.13, 0.05, 0.02]).astype(np.float32), axis=1)
        for q, n in enumerate(lens):
            preds[q, n:] = np.nan
            labels[q, n:] = np.nan
        if L != 4096:
            preds[B - 1, lens[-1] // 3] = np.nan
        _BATCHES[L] = (preds, labels, np.asarray(lens, np.int32))
    return _BATCHES[L]


COMBOS = [(S, dist, T) for S in (1, 3) for dist in ("PL", "STPL") for T in (1.0, 0.5)]


@pytest.mark.parametrize("S,dist,T", COMBOS, ids=[f"S{S}-{d}-T{T:g}" for S, d, T in COMBOS])
@pytest.mark.parametrize("L", WIDTHS + (4096,))
def test_every_dispatch_form_matches_the_restatement(L, S, dist, T):
    preds, labels, lens = batch(L)
    B = preds.shape[0]
    top_k, gamma = (10, 1.0) if S == 1 else (None, 0.9)
    seed = 77 + L
    unif = c_uniforms(B, L, S, seed).cpu().numpy()
    assert np.array_equal(unif, PR.uniforms_host(B, L, S, seed))            # the host restatement of the counter hash, bit for bit
    lists, draws = PR.redraw(preds, unif, lens, T, dist, seed=L)
    print(f"REDRAWN L={L} S={S} {dist} T={T:g}: {draws} uniforms in {lists} of {B * S} lists")
    perm, act = c_sample(preds, lens, S, T, dist, unif=unif)
    total, lq, grad, perm2 = c_fused(preds, labels, lens, S, top_k, gamma, T, dist, unif=unif)
    rperm, ract, ok, Eact = PR.sample(preds, unif, lens, T, dist)
    ref = PR.mdprank_sampled(preds, labels, unif, lens, top_k, gamma, T, dist)
    assert ok.all() and ref["ok"].all()
    assert np.array_equal(perm, rperm) and np.array_equal(perm2, rperm)     # exact, padded tail and NaN lists (identity) included
    gate_nan(act, ract, Eact, f"action L={L} S={S} {dist} T={T:g}", C_LIST)
    gate_losses(lq, grad, ref, f"L={L} S={S} {dist} T={T:g}", C_LIST, total, batch_total(ref, C_LIST))
    for q, n in enumerate(lens):
        assert (grad[q, n:] == 0).all() and (act[q, :, n:] == 0).all()
        if n == 0:
            assert lq[q] == 0.0


def test_equal_keys_are_ordered_by_index_in_every_form():
    """Ties never reach the packed sort's fast path: equal scores with equal uniforms rank by index, blocks of equal keys stay in order."""
    for L in (64, 100, 256, 1024, 1500):
        preds = np.zeros((2, L), np.float32)
        preds[1, ::2] = 1.0
        unif = np.full((2, 1, L), 0.25, np.float32)
        perm, _ = c_sample(preds, None, 1, 1.0, "PL", unif=unif)
        assert np.array_equal(perm[0, 0], np.arange(L))
        assert np.array_equal(perm[1, 0], np.concatenate([np.arange(0, L, 2), np.arange(1, L, 2)]))


# ---------------------------------------------------------------------------------------------------------------- fused vs composed
@pytest.mark.parametrize("dist,T", [("PL", 0.5), ("STPL", 2.0)])
@pytest.mark.parametrize("L", [100, 1100])
def test_fused_equals_sampler_then_mdprank_loss(L, dist, T):
    import ptranking_amd.functional as F
    g = np.random.default_rng(L)
    B, S, top_k, gamma = 5, 3, 10, 0.9
    preds = g.standard_normal((B, L)).astype(np.float32)
    labels = -np.sort(-g.integers(0, 5, size=(B, L)).astype(np.float32), axis=1)
    lens = np.asarray([L, L - 3, 7, 1, L // 2], np.int32)
    seed, q0 = 4242, 17
    unif = c_uniforms(B, L, S, seed, q0)
    total, lq, grad, perm = c_fused(preds, labels, lens, S, top_k, gamma, T, dist, seed=seed, q0=q0)
    sperm, _ = c_sample(preds, lens, S, T, dist, seed=seed, q0=q0)
    assert np.array_equal(perm, sperm)
    p = dev(preds).requires_grad_(True)
    y, n = dev(labels), dev(lens)
    comp = 0.0
    for s in range(S):
        if dist == "PL":
            a = p
        else:
            noise = -torch.log(-torch.log(unif[:, s] + 1e-20) + 1e-20)
            a = (p + noise) / T
        comp = comp + F.mdprank_loss(a, y, dev(sperm[:, s]), top_k=top_k, gamma=gamma, lens=n) / S
    comp.backward()
    ref = PR.mdprank_sampled(preds, labels, unif.cpu().numpy(), lens, top_k, gamma, T, dist, perm=perm)
    tot = batch_total(ref, C_LIST)
    gate_losses(lq, grad, ref, f"fused L={L} {dist}", C_LIST, total, tot)
    gate_nan(p.grad.cpu().numpy(), ref["grad"], ref["E_grad"], f"composed grad L={L} {dist}", C_LIST)
    gate_nan(np.array([float(comp.detach())]), np.array([tot[0]]), np.array([tot[1] + C_LIST * PR.U * np.abs(ref["loss_s"]).sum()]),
             f"composed loss L={L} {dist}", C_LIST)


# ---------------------------------------------------------------------------------------------------------------- stream identities
@pytest.mark.parametrize("L", [100, 1100])
def test_stream_identities(L):
    g = np.random.default_rng(3)
    B, S, T, dist = 6, 3, 0.5, "PL"
    preds = g.standard_normal((B, L)).astype(np.float32)
    labels = -np.sort(-g.integers(0, 5, size=(B, L)).astype(np.float32), axis=1)
    lens = np.asarray([L, 5, L - 1, 0, L // 2, L], np.int32)
    seed, q0 = 2 ** 35 + 9, 2 ** 32 - 3                                   # a global query index that crosses 2^32 inside the batch
    whole = c_fused(preds, labels, lens, S, 10, 0.9, T, dist, seed=seed, q0=q0)
    unif = c_uniforms(B, L, S, seed, q0).cpu().numpy()
    fed = c_fused(preds, labels, lens, S, 10, 0.9, T, dist, seed=123, q0=0, unif=unif)

    def same(a, b):
        return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))

    assert same(whole, fed)                                                  # the uniforms fed back: the same bits
    assert same(whole, c_fused(preds, labels, lens, S, 10, 0.9, T, dist, seed=seed, q0=q0))      # a repeated call
    lo = c_fused(preds[:2], labels[:2], lens[:2], S, 10, 0.9, T, dist, seed=seed, q0=q0)
    hi = c_fused(preds[2:], labels[2:], lens[2:], S, 10, 0.9, T, dist, seed=seed, q0=q0 + 2)
    for k in (1, 2, 3):
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), whole[k])     # two shards with the right q0: the whole batch
    for q in (0, 4, 5):
        one = c_fused(preds[q:q + 1], labels[q:q + 1], lens[q:q + 1], S, 10, 0.9, T, dist, seed=seed, q0=q0 + q)
        assert all(np.array_equal(one[k][0], whole[k][q]) for k in (1, 2, 3))                    # a query alone
    sp, sa = c_sample(preds, lens, S, T, dist, seed=seed, q0=q0)
    assert np.array_equal(sp, whole[3])
    other, _ = c_sample(preds, lens, S, T, dist, seed=seed + 1, q0=q0)
    assert not np.array_equal(other[0], sp[0]) and not np.array_equal(other[5], sp[5])
    shifted, _ = c_sample(preds, lens, S, T, dist, seed=seed, q0=q0 + 1)
    assert not np.array_equal(shifted[0], sp[0])                             # the stream belongs to the global query index


# ---------------------------------------------------------------------------------------------------------------- the law
def chi2_quantile(df, tail=1e-6):
    """x with P(chi^2_df > x) = tail, from the regularised upper incomplete gamma function by bisection."""
    a = torch.tensor(df / 2.0, dtype=torch.float64)
    lo, hi = 0.0, 50.0 * df + 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if float(torch.special.gammaincc(a, torch.tensor(mid / 2.0, dtype=torch.float64))) > tail:
            lo = mid
        else:
            hi = mid
    return hi


def chi2(counts, probs):
    counts, probs = np.asarray(counts, np.float64), np.asarray(probs, np.float64)
    exp = counts.sum() * probs
    return float(((counts - exp) ** 2 / exp).sum())


def test_chi2_quantile_is_right():
    """Two degrees of freedom have the closed form -2 ln(tail); 3.8415 is the textbook 5 % point of one degree; 70.55 and 44.81 are
    the 1 - 1e-6 points of 23 and 9 degrees from an independent implementation of the inverse survival function."""
    assert abs(chi2_quantile(2) + 2.0 * math.log(1e-6)) < 1e-6 and abs(chi2_quantile(1, 0.05) - 3.8415) < 1e-3
    assert abs(chi2_quantile(23) - 70.55) < 0.01 and abs(chi2_quantile(9) - 44.81) < 0.01


@pytest.mark.parametrize("dist,T", [("PL", 1.0), ("PL", 0.5), ("STPL", 2.0)])
def test_law_of_four_documents(dist, T):
    s = np.array([1.0, 0.5, 0.0, -1.0], np.float32)
    B, S = 4096, 64
    perm, _ = c_sample(np.tile(s, (B, 1)), None, S, T, dist, seed=20261019, want_action=False)
    pr = PR.pl_probabilities(s, T if dist == "PL" else 1.0)                  # 'STPL': T does not enter the ranking's law
    keys = sorted(pr)
    code = (perm * np.array([64, 16, 4, 1])).sum(-1)
    codes = [sum(a * b for a, b in zip(k, (64, 16, 4, 1))) for k in keys]
    probs = [pr[k] for k in keys]
    limit = chi2_quantile(23)
    for what, sub in (("all", code), ("even s", code[:, 0::2]), ("odd s", code[:, 1::2])):
        cnt = [(sub == c).sum() for c in codes]
        assert sum(cnt) == sub.size                                          # every row is a permutation
        x = chi2(cnt, probs)
        print(f"LAW {dist} T={T:g} {what}: chi2_23 = {x:.1f} (limit {limit:.1f})")
        assert x < limit
    first = perm[:, :, 0]
    tab = np.zeros((4, 4))
    np.add.at(tab, (first[:, :-1].ravel(), first[:, 1:].ravel()), 1.0)
    exp = tab.sum(1, keepdims=True) * tab.sum(0, keepdims=True) / tab.sum()
    x = float(((tab - exp) ** 2 / exp).sum())
    print(f"LAW {dist} T={T:g} first documents of samples s, s + 1: chi2_9 = {x:.1f} (limit {chi2_quantile(9):.1f})")
    assert x < chi2_quantile(9)


def test_law_of_the_first_position_at_100_documents():
    g = np.random.default_rng(8)
    s = g.uniform(-1.0, 1.0, size=100).astype(np.float32)
    T = 0.5
    p = dev(np.tile(s, (4096, 1)))
    import ptranking_amd.functional as F
    perm = F.sample_rankings_pl(p, samples=64, temperature=T, distribution="PL", seed=99)
    cnt = torch.bincount(perm[:, :, 0].reshape(-1), minlength=100).cpu().numpy()
    w = np.exp(s.astype(np.float64) / T)
    x = chi2(cnt, w / w.sum())
    print(f"LAW first position of 100 documents: chi2_99 = {x:.1f} (limit {chi2_quantile(99):.1f})")
    assert cnt.sum() == 2 ** 18 and x < chi2_quantile(99)
    assert bool((torch.sort(perm[:64], dim=2)[0] == torch.arange(100, device="cuda")).all())


def test_uniforms_are_uniform_and_uncorrelated():
    u = c_uniforms(4096, 64, 64, seed=31337)                                 # [q, s, i]: 2^24 draws
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0 and bool((u * 2 ** 24 == torch.floor(u * 2 ** 24)).all())
    N = u.numel()
    cnt = torch.bincount((u * 256).long().reshape(-1), minlength=256).cpu().numpy()
    x = chi2(cnt, np.full(256, 1 / 256))
    print(f"UNIFORMS 256 bins over {N} draws: chi2_255 = {x:.1f} (limit {chi2_quantile(255):.1f})")
    assert N == 2 ** 24 and x < chi2_quantile(255)
    z = (u.double() - 0.5)
    var = float((z * z).mean())
    for name, a, b in (("i", z[:, :, :-1], z[:, :, 1:]), ("s", z[:, :-1], z[:, 1:]), ("q", z[:-1], z[1:])):
        r = float((a * b).mean()) / var
        print(f"UNIFORMS lag-1 correlation along {name}: {r:.2e} (limit {4 / math.sqrt(a.numel()):.2e})")
        assert abs(r) < 4 / math.sqrt(a.numel())


# ---------------------------------------------------------------------------------------------------------------- underflow
def test_scores_whose_weights_underflow_still_sample_and_train():
    """exp(-200) and exp(-400) are 0 in fp32: torch.multinomial without replacement fails on such a row (the reference raises; the default
    route clamps at 1e-38).  The Gumbel key needs no weight: document 0 first, then 1, then 2, in every draw (g spans 20.4 < 200)."""
    s = np.array([0.0, -200.0, -400.0], np.float32)
    B, S = 1024, 64
    perm, act = c_sample(np.tile(s, (B, 1)), None, S, 1.0, "PL", seed=5)
    assert perm.shape == (B, S, 3) and (perm == np.array([0, 1, 2])).all() and (act == s).all()
    labels = np.tile(np.array([0.0, 2.0, 1.0], np.float32), (B, 1))
    total, lq, grad, _ = c_fused(np.tile(s, (B, 1)), labels, None, S, 10, 1.0, 1.0, "PL", seed=5)
    assert np.isfinite(total) and np.isfinite(lq).all() and np.isfinite(grad).all()


@pytest.mark.parametrize("L", [100, 1100])
def test_wide_score_spreads_take_the_log_domain_path_inside_the_same_bound(L):
    """Scores spread over a few hundred units: exp(a - m) underflows in fp32 from a - m < -87 on, where the reference's log(cumsum) is
    -inf.  The kernel takes such an episode through log-domain scans; the float64 restatement (no underflow there) and its bound hold as
    they are."""
    g = np.random.default_rng(L)
    B, S, T, dist = 4, 2, 1.0, "PL"
    preds = (40.0 * g.standard_normal((B, L))).astype(np.float32)
    labels = -np.sort(-g.integers(0, 5, size=(B, L)).astype(np.float32), axis=1)
    lens = np.asarray([L, L - 1, 9, L // 2], np.int32)
    unif = c_uniforms(B, L, S, 606).cpu().numpy()
    lists, draws = PR.redraw(preds, unif, lens, T, dist, seed=L)
    print(f"REDRAWN wide L={L}: {draws} uniforms in {lists} of {B * S} lists")
    for top_k, gamma in ((10, 1.0), (None, 0.9)):
        total, lq, grad, perm = c_fused(preds, labels, lens, S, top_k, gamma, T, dist, unif=unif)
        ref = PR.mdprank_sampled(preds, labels, unif, lens, top_k, gamma, T, dist)
        assert ref["ok"].all() and np.array_equal(perm, ref["perm"])
        assert np.isfinite(total) and np.isfinite(grad).all()
        gate_losses(lq, grad, ref, f"wide L={L} top_k={top_k}", C_LIST, total, batch_total(ref, C_LIST))


# ---------------------------------------------------------------------------------------------------------------- the ranker
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=16, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False, dropout=0.0)}


def _data(B=12, L=48, F=16):
    rng = np.random.default_rng(5)
    X = torch.from_numpy(rng.standard_normal((B, L, F)).astype(np.float32))
    Y = rng.choice(5, size=(B, L), p=[0.5, 0.3, 0.15, 0.03, 0.02]).astype(np.float32)
    Y[:, 0] = np.maximum(Y[:, 0], 1)
    lens = torch.from_numpy(rng.integers(3, L + 1, size=B).astype(np.int32))
    return X, torch.from_numpy(-np.sort(-Y, axis=1).copy()), lens


def _make(dist="PL", T=1.0, S=4):
    import ptranking_amd as pa
    torch.manual_seed(21)
    paras = dict(pa.DEFAULT_PARAS["MDPRank"], distribution=dist, temperature=T, sampler="device", samples_per_query=S)
    r = pa.MDPRank(sf_para_dict=copy.deepcopy(SF), model_para_dict=paras, gpu=True, device="cuda:0")
    r.init()
    r.train_mode()
    return r


@pytest.mark.parametrize("with_lens", [False, True], ids=["full", "lens"])
@pytest.mark.parametrize("dist,T", [("PL", 1.0), ("STPL", 2.0)])
def test_ranker_trains_with_the_device_sampler(dist, T, with_lens):
    import ptranking_amd as pa
    X, Y, lens = _data()
    X, Y, lens = X.cuda(), Y.cuda(), (lens.cuda() if with_lens else None)
    r = _make(dist, T)
    before = [p.detach().clone() for p in r.get_parameters()]
    losses = []
    for step in range(20):
        kw = dict(lens=lens) if with_lens else {}
        loss, _ = r.train_op(X, Y, epoch_k=step + 1, presort=True, label_type=pa.LABEL_TYPE.MultiLabel, **kw)
        losses.append(float(loss))
    assert np.isfinite(losses).all() and r._pl_calls == 20
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, r.get_parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in r.get_parameters())


def test_a_one_query_batch_is_the_batched_step_of_that_query():
    X, Y, lens = _data()
    g = torch.Generator().manual_seed(1)
    preds = torch.randn(12, 48, generator=g).cuda()
    Y, lens = Y.cuda(), lens.cuda()
    r = _make("STPL", 2.0)
    r._fused_step = lambda loss: (loss.backward(), loss)[1]

    def step(p, y, n, q0):
        r._pl_calls = 0
        p = p.clone().requires_grad_(True)
        loss = r.custom_loss_function(p, y, presort=True, lens=n, q0=q0)
        return float(loss), p.grad.cpu().numpy()

    _, whole = step(preds, Y, lens, 100)
    for q in (0, 7, 11):
        _, one = step(preds[q:q + 1], Y[q:q + 1], lens[q:q + 1], 100 + q)
        assert np.array_equal(one[0], whole[q])
        _, off = step(preds[q:q + 1], Y[q:q + 1], lens[q:q + 1], 0)
        assert not np.array_equal(off[0], whole[q])


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", PTR_DP_BACKEND="gloo")
    import torch.distributed as dist
    import ptranking_amd as pa
    from ptranking_amd import dp
    dp.init_from_env()
    X, Y, _ = _data()
    lo, hi = dp.shard_queries(X.size(0))
    r = _make("PL", 1.0, 2)
    q0 = r._query_offset(hi - lo, {})
    losses = []
    for step in range(2):
        loss, _ = r.train_op(X[lo:hi].cuda(), Y[lo:hi].cuda(), epoch_k=1, presort=True, label_type=pa.LABEL_TYPE.MultiLabel)
        losses.append(float(loss.detach()))
    torch.save({"flat": r.point_sf.flat.detach().cpu(), "q0": q0, "losses": losses}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_draw_disjoint_streams(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{i}.pt") for i in range(2))
    assert torch.equal(r0["flat"], r1["flat"]), "replicas diverged"
    assert (r0["q0"], r1["q0"]) == (0, 6)
    assert np.isfinite(r0["losses"] + r1["losses"]).all() and bool(torch.isfinite(r0["flat"]).all())


def test_the_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_mdprank_device.py"), "--queries", "64", "--steps", "10"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "before" in out.stdout and "after" in out.stdout and "step  10" in out.stdout, out.stdout
    assert "nan" not in out.stdout.lower()
