"""GPU: the list machines' kernels (csrc/adlist.hip) against the restatement (tests/adlist_ref.py), and the two machines.

Sampler with supplied uniforms: equal index for index; the uniforms are redrawn on the CPU, row by row, until no two Gumbel keys of a list
lie within 1e-4 (asserted, no case left out); the standard rankings compare labels and multiples of 2^-24 exactly and need no screening.
With the hash: ptr_pl_uniforms reproduces the draws, the generated rankings are the prefix of ptr_pl_sample's STPL perm, two calls agree,
a shard with q0 gives the whole batch's rows, L = 256 and L = 257 draw the same.  Laws by chi-square at p = 1e-4, fixed seeds.
Losses: loss_q, loss_out and every gradient element of D x {PL, BT} x {IRGAN, 8 divergences} and of G x {PL, BT} x {4 rewards, 8
divergences} are gated against the float64 restatement, E = C_ADLIST x its first-order bound, which carries the reward's amplification of
the error in lp.  Queries are kept where every float64 value is inside fp32 range: all of them under KL / PC / TVar / GAN and the -lp and
log(1 - lp) rewards, and for the exponential rewards wherever K <= 5 (asserted).  C_ADLIST follows the project's rule for C_METRIC (the
need of the float32 CPU restatement on THESE cases, doubled, rounded up to a half, capped at 4; tests/test_adlist_cpu.py recomputes it).
    MEASURED need at c = 1:  fp32 CPU restatement 0.33 -> C_ADLIST 1.0;  kernels on the MI355X 0.14 (the gradient of D at S = 64; G 0.05)
Shapes: B 5..7; L 1, 2, 3, 63, 64, 65, 130, 256 (wavefront form) and 257, 300 (workgroup form); S 1, 5, 64; K 1, 2, 5, n, > n, whole list;
lens with 0 and 1; labels all equal, labels with -1, a NaN score."""
import copy
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import adlist_ref as AR
from f64_bounds import gate
from golden_util import assert_close
from launch_form import launch_form
from plsample_ref import uniforms_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adlist.npz")
gpu = pytest.mark.gpu
#        B  L    S   K     nan
CASES = ((5, 1, 1, 1, False),
         (6, 2, 5, 2, False),
         (7, 3, 5, None, False),
         (5, 63, 5, 1, False),
         (6, 64, 64, 2, False),
         (7, 65, 5, None, True),
         (5, 130, 64, 5, False),
         (6, 256, 5, 300, True),
         (7, 257, 1, 257, False),
         (6, 300, 5, None, False))
IDS = [f"{c[0]}x{c[1]}-S{c[2]}-K{c[3]}" for c in CASES]
DIVS = tuple(AR.F_DIVS)
REWARDS = tuple(AR.REWARDS)
D_VARIANTS = (("IRGAN", "exp_1m", "KL"),) + tuple(("IRFGAN", "exp_1m", f) for f in DIVS)
G_VARIANTS = tuple(("IRGAN", r, "KL") for r in REWARDS) + tuple(("IRFGAN", "exp_1m", f) for f in DIVS)
ALWAYS_KEPT = {("IRFGAN", f) for f in ("KL", "PC", "TVar", "GAN")} | {("IRGAN", r) for r in ("neg_lp", "log_1m")}
TEMPERATURE = 0.5
CHI2_1E4 = {3: 21.108, 4: 23.513, 5: 25.745, 6: 27.857}        # chi-square quantiles at 1 - 1e-4 by degrees of freedom


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(generator scores s, discriminator scores d in (0, 1), labels y, lens).  Query 0 is full (and holds the NaN score where the case has
    one), 1 is empty, 2 a single document; query 3's labels are all equal, query 4's end in -1 (masked) labels."""
    B, L, S, K, nan = case
    g = np.random.default_rng(5000 * L + B)
    s = (1.5 * g.standard_normal((B, L))).astype(np.float32)
    d = (1.0 / (1.0 + np.exp(-1.5 * g.standard_normal((B, L))))).astype(np.float32)
    lens = g.integers(min(2, L), L + 1, size=B).astype(np.int32)
    lens[0], lens[1], lens[2] = L, 0, min(1, L)
    y = g.integers(0, 5, size=(B, L)).astype(np.float32)
    y[3] = 2.0
    y[4, int(lens[4]) // 2:] = -1.0
    if nan:
        s[0, L // 2] = np.nan
    return s, d, y, lens


def hash_key(case):
    """(seed, q0) of a case's hash route: both beyond 32 bits."""
    return 2 ** 41 + 23 * case[1], 2 ** 33 + 11


@functools.lru_cache(maxsize=None)
def sample_case(case):
    """(unif [B, 2 S, L], std_idx, gen_idx, kq) with every generated ranking pinned (asserted)."""
    B, L, S, K, _ = case
    s, _, y, lens = inputs(case)
    rng = np.random.default_rng(13 + L)
    unif = rng.random((B, 2 * S, L), dtype=np.float32)
    for _ in range(400):
        loose = [(q, k) for q in range(B) for k in range(S)
                 if lens[q] > 0 and not np.isnan(s[q, :lens[q]]).any() and not AR.gen_order(s[q, :lens[q]], unif[q, k, :lens[q]])[1]]
        if not loose:
            break
        for q, k in loose:
            unif[q, k] = rng.random(L, dtype=np.float32)
    std, gen, kq, pinned = AR.sample(s, y, lens, S, K, unif)
    assert pinned.all(), case
    return unif, std, gen, kq


@functools.lru_cache(maxsize=None)
def g_unif(case):
    """unif [B, S, L] of a generator call with every ranking pinned (asserted in the restatement's output)."""
    unif = sample_case(case)[0][:, :case[2]].copy()
    x = g_scores(case)
    s, _, _, lens = inputs(case)
    rng = np.random.default_rng(29 + case[1])
    for _ in range(400):
        loose = [(q, k) for q in range(case[0]) for k in range(case[2]) if lens[q] > 0 and not AR.gen_order(x[q, :lens[q]], unif[q, k, :lens[q]])[1]]
        if not loose:
            break
        for q, k in loose:
            unif[q, k] = rng.random(case[1], dtype=np.float32)
    return unif


def g_scores(case):
    """The generator's scores of a loss call: finite everywhere except query 0 of the NaN cases, which the kernel must skip."""
    return inputs(case)[0]


@functools.lru_cache(maxsize=None)
def loss_ref(case, mode, prob, variant, dtype=torch.float64, c=None):
    family, reward, f_div = variant
    s, d, y, lens = inputs(case)
    if mode == "D":
        _, std, gen, kq = sample_case(case)
        return AR.loss(d, "D", prob, family, reward, f_div, std_idx=std, gen_idx=gen, kq=kq, lens=lens, dtype=dtype, c=c)
    return AR.loss(g_scores(case), "G", prob, family, reward, f_div, d_preds=d, S=case[2], top_k=case[3], T=TEMPERATURE, unif=g_unif(case), lens=lens,
                   dtype=dtype, c=c)


def variants(mode):
    return D_VARIANTS if mode == "D" else G_VARIANTS


def kept(case, mode, prob, variant):
    """The queries of a loss case whose float64 values all lie inside fp32 range; asserted complete where the module's header says so."""
    ref = loss_ref(case, mode, prob, variant)
    keep = ref["inrange"]
    family, reward, f_div = variant
    tag = (family, f_div if family == "IRFGAN" else reward)
    small_k = case[3] is not None and case[3] <= 5
    if tag in ALWAYS_KEPT or (mode == "D" and family == "IRGAN") or (family == "IRGAN" and small_k):
        assert keep.all(), (case, mode, prob, variant)
    return keep


def fp32_restatement_need():
    """The worst err / E (c = 1) of the float32 CPU restatement against the float64 one over every loss case of this module."""
    worst = 0.0
    for case in CASES:
        for mode in ("D", "G"):
            for prob in ("PL", "BT"):
                for variant in variants(mode):
                    r64, r32 = loss_ref(case, mode, prob, variant, c=1.0), loss_ref(case, mode, prob, variant, dtype=torch.float32)
                    keep = r64["inrange"]
                    for k, e in (("loss_q", "E_loss_q"), ("grad", "E_grad")):
                        a, b, E = r32[k][keep], r64[k][keep], r64[e][keep]
                        m = np.isfinite(b) & (E > 0)
                        if m.any():
                            worst = max(worst, float((np.abs(a - b)[m] / E[m]).max()))
    return worst


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_cases_reach_every_form():
    """The case list launches both forms of both entry points, on both sides of the boundary, and holds the shapes the header names."""
    Ls = {c[1] for c in CASES}
    assert {1, 2, 3, 63, 64, 65, 130, 256, 257, 300} == Ls and {c[0] for c in CASES} == {5, 6, 7} and {c[2] for c in CASES} == {1, 5, 64}
    for entry in ("ptr_adlist_sample", "ptr_adlist_fwd_bwd"):
        forms = {L: launch_form(entry, L)[:2] for L in Ls}
        assert {L for L, f in forms.items() if f == (64, 4)} == {1, 2, 3, 63, 64, 65, 130, 256}
        assert {L for L, f in forms.items() if f == (256, 1)} == {257, 300}
    ks = set()
    for B, L, S, K, nan in CASES:
        s, d, y, lens = inputs((B, L, S, K, nan))
        assert lens.min() == 0 and lens.max() == L and (L == 1 or 1 in lens.tolist())
        assert (y[3] == y[3, 0]).all() and (L < 2 or (y[4] == -1).any())
        ks.add("whole" if K is None else K if K < L else "n" if K == L else ">n")
    assert ks == {1, 2, 5, "n", ">n", "whole"} and sum(c[4] for c in CASES) >= 2


# ------------------------------------------------------------------------------------------------------------- the sampler
@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sampler_with_supplied_uniforms_equals_the_restatement(case):
    import ptranking_amd.functional as F
    B, L, S, K, _ = case
    s, _, y, lens = inputs(case)
    unif, std, gen, kq = sample_case(case)
    got = F.adlist_sample(dev(s), dev(y), S, top_k=K, lens=dev(lens), unif=dev(unif))
    assert got[0].shape == got[1].shape == (B, S, AR.kw_of(K, L)) and got[0].dtype == torch.int64 and got[2].dtype == torch.int32
    assert np.array_equal(got[2].cpu().numpy(), kq) and kq[1] == 0 and (not case[4] or kq[0] == 0)
    assert np.array_equal(got[1].cpu().numpy(), gen), "generated rankings"
    assert np.array_equal(got[0].cpu().numpy(), std), "standard rankings"


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sampler_with_the_hash(case):
    import ptranking_amd.functional as F
    B, L, S, K, _ = case
    s, _, y, lens = inputs(case)
    seed, q0 = hash_key(case)
    sd, yd, ld = dev(s), dev(y), dev(lens)
    a = F.adlist_sample(sd, yd, S, top_k=K, seed=seed, q0=q0, lens=ld)
    b = F.adlist_sample(sd, yd, S, top_k=K, seed=seed, q0=q0, lens=ld)
    unif = F.adlist_uniforms(B, L, S, seed=seed, q0=q0)
    assert np.array_equal(unif.cpu().numpy(), uniforms_host(B, L, 2 * S, seed, q0))
    u = F.adlist_sample(sd, yd, S, top_k=K, lens=ld, unif=unif)
    sh = F.adlist_sample(sd[3:], yd[3:], S, top_k=K, seed=seed, q0=q0 + 3, lens=ld[3:])
    for x, z, w, v in zip(a, b, u, sh):
        assert torch.equal(x, z) and torch.equal(x, w) and torch.equal(x[3:], v)
    perm = F.sample_rankings_pl(sd, samples=S, distribution="STPL", seed=seed, q0=q0, lens=ld)
    kq = a[2].cpu().numpy()
    for q in range(B):
        assert torch.equal(a[1][q, :, :kq[q]], perm[q, :, :kq[q]]), q
        assert not a[1][q, :, kq[q]:].any() and not a[0][q, :, kq[q]:].any()
        for k in range(S):                                                    # a standard ranking is a label-descending run of distinct documents
            idx = a[0][q, k, :kq[q]].cpu().numpy()
            assert len(set(idx.tolist())) == kq[q] and (np.diff(y[q, idx]) <= 0).all()
            assert kq[q] == 0 or y[q, idx[-1]] >= np.sort(y[q, :lens[q]])[::-1][kq[q] - 1]


@gpu
def test_the_two_forms_draw_the_same():
    import ptranking_amd.functional as F
    assert launch_form("ptr_adlist_sample", 256)[0] == 64 and launch_form("ptr_adlist_sample", 257)[0] == 256
    case = CASES[7]
    s, d, y, lens = inputs(case)
    seed, q0 = hash_key(case)
    wide = lambda a: np.concatenate([a, np.zeros((a.shape[0], 1), a.dtype)], axis=1)
    for K in (5, None, 256):
        a = F.adlist_sample(dev(s), dev(y), 5, top_k=K, seed=seed, q0=q0, lens=dev(lens))
        b = F.adlist_sample(dev(wide(s)), dev(wide(y)), 5, top_k=K, seed=seed, q0=q0, lens=dev(lens))
        w = a[0].shape[2]
        assert torch.equal(a[0], b[0][:, :, :w]) and torch.equal(a[1], b[1][:, :, :w]) and torch.equal(a[2], b[2])


@gpu
def test_sampler_laws():
    """The top document of the generated rankings follows softmax(preds); the standard ranking is uniform over a tie block."""
    import ptranking_amd.functional as F
    N = 4096
    s7 = np.array([0.3, -1.0, 1.2, 0.0, -0.4, 0.9, 0.1], np.float32)
    y7 = np.array([2, 2, 2, 2, 2, 1, 0], np.float32)
    std, gen, kq = F.adlist_sample(dev(np.tile(s7, (N, 1))), dev(np.tile(y7, (N, 1))), 2, top_k=1, seed=2468)
    assert (kq == 1).all()
    p = np.exp(s7.astype(np.float64))
    p /= p.sum()
    counts = np.bincount(gen.cpu().numpy().reshape(-1), minlength=7)
    chi_g = float(((counts - 2 * N * p) ** 2 / (2 * N * p)).sum())
    tops = np.bincount(std.cpu().numpy().reshape(-1), minlength=7)
    assert tops[5:].sum() == 0
    chi_s = float(((tops[:5] - 2 * N / 5) ** 2 / (2 * N / 5)).sum())
    print(f"MEASURED chi-square: top generated document {chi_g:.2f} at 6 degrees of freedom (bound {CHI2_1E4[6]}), "
          f"top standard document {chi_s:.2f} at 4 ({CHI2_1E4[4]})")
    assert chi_g < CHI2_1E4[6] and chi_s < CHI2_1E4[4]


# ------------------------------------------------------------------------------------------------------------- the losses
def _launch(case, mode, prob, variant, sl=slice(None), **over):
    import ptranking_amd.functional as F
    family, reward, f_div = variant
    s, d, y, lens = inputs(case)
    if mode == "D":
        _, std, gen, kq = sample_case(case)
        x = dev(d[sl]).requires_grad_(True)
        kw = dict(std_idx=dev(std[sl]), gen_idx=dev(gen[sl]), kq=dev(kq[sl]))
    else:
        x = dev(g_scores(case)[sl]).requires_grad_(True)
        kw = dict(d_preds=dev(d[sl]), samples_per_query=case[2], top_k=case[3], temperature=TEMPERATURE, unif=dev(g_unif(case)[sl]))
        kw.update(over)
    loss, parts = F.adlist_loss(x, mode, prob=prob, family=family, reward=reward, f_div=f_div, lens=dev(lens[sl]), return_parts=True, **kw)
    loss.backward()
    return loss.detach().cpu().numpy().reshape(1), parts, x.grad.cpu().numpy()


@gpu
@pytest.mark.parametrize("prob", ("PL", "BT"))
@pytest.mark.parametrize("mode", ("D", "G"))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_losses_against_float64(case, mode, prob):
    worst = 0.0
    B, L, S, K, nan = case
    lens = inputs(case)[3]
    for variant in variants(mode):
        ref = loss_ref(case, mode, prob, variant)
        keep = kept(case, mode, prob, variant)
        loss, parts, grad = _launch(case, mode, prob, variant)
        what = f"adlist {mode} {prob} {variant} {IDS[CASES.index(case)]}"
        assert np.array_equal(parts["valid_q"].cpu().numpy(), ref["valid_q"]), what
        if mode == "G":
            assert ref["pinned"].all() and np.array_equal(parts["gen_idx"].cpu().numpy(), ref["gen_idx"]), what
        worst = max(worst,
                    gate(parts["loss_q"].cpu().numpy()[keep], ref["loss_q"][keep], torch.from_numpy(ref["E_loss_q"][keep]), what + " loss_q", c=AR.C_ADLIST),
                    gate(grad[keep], ref["grad"][keep], torch.from_numpy(ref["E_grad"][keep]), what + " grad", c=AR.C_ADLIST))
        if keep.all():
            worst = max(worst, gate(loss, np.array([ref["loss"]]), torch.tensor([ref["E_loss"]], dtype=torch.float64), what + " loss_out", c=AR.C_ADLIST))
        assert (grad[np.arange(L)[None, :] >= lens[:, None]] == 0).all()
        assert ref["valid_q"][1] == 0 and (L == 1 or (ref["valid_q"][2] == 1 and not grad[2].any()))
        if mode == "G" or variant[0] == "IRGAN":
            assert parts["loss_q"][2] == 0 and parts["loss_q"][1] == 0                 # n = 1: lp = 0
    print(f"MEASURED adlist {mode} {prob} {IDS[CASES.index(case)]}: kernel needs c >= {worst * AR.C_ADLIST:.3f}")


@gpu
@pytest.mark.parametrize("case", (CASES[5], CASES[9]), ids=lambda c: f"L{c[1]}")
def test_a_wide_spread_takes_the_log_domain(case):
    """Discriminator scores that spread over thousands: exp(v - max) underflows for most of a ranking, in double too; the kernel's
    log-domain scans keep every term (the restatement's logcumsumexp does the same)."""
    import ptranking_amd.functional as F
    B, L, S, K, _ = case
    s, d, y, lens = inputs(case)
    _, std, gen, kq = sample_case(case)
    x = (800.0 * np.random.default_rng(3).standard_normal((B, L))).astype(np.float32)
    assert all(np.ptp(x[q, :lens[q]]) > 600 for q in range(B) if lens[q] > 8)
    for family, f_div in (("IRGAN", "KL"), ("IRFGAN", "TVar"), ("IRFGAN", "PC")):
        ref = AR.loss(x, "D", "PL", family, "exp_1m", f_div, std_idx=std, gen_idx=gen, kq=kq, lens=lens)
        assert ref["inrange"].all() and np.isfinite(ref["grad"]).all()
        xd = dev(x).requires_grad_(True)
        loss, parts = F.adlist_loss(xd, "D", prob="PL", family=family, f_div=f_div, std_idx=dev(std), gen_idx=dev(gen), kq=dev(kq), lens=dev(lens),
                                    return_parts=True)
        loss.backward()
        what = f"adlist wide spread {family} {f_div} L{L}"
        gate(parts["loss_q"].cpu().numpy(), ref["loss_q"], torch.from_numpy(ref["E_loss_q"]), what + " loss_q", c=AR.C_ADLIST)
        gate(xd.grad.cpu().numpy(), ref["grad"], torch.from_numpy(ref["E_grad"]), what + " grad", c=AR.C_ADLIST)


@gpu
def test_the_longest_list_takes_its_lds():
    """L = K = PTR_MAX_LIST_LEN: 128 KiB of dynamic LDS per query, beyond the 64 KiB a launch gets unasked.  The discriminator's loss on the
    sampler's own rankings against float64; the generator's whole-list step draws the sampler's rankings, stays finite, leaves padding alone
    and, a function of softmax((x + g) / T), has a gradient that sums to zero over a list."""
    import ptranking_amd.functional as F
    L = 4096
    rng = np.random.default_rng(77)
    s = (1.5 * rng.standard_normal((2, L))).astype(np.float32)
    d = (1.0 / (1.0 + np.exp(-1.5 * rng.standard_normal((2, L))))).astype(np.float32)
    y = rng.integers(0, 5, size=(2, L)).astype(np.float32)
    lens = np.array([L, 3001], np.int32)
    assert launch_form("ptr_adlist_fwd_bwd", L)[:2] == (256, 1)
    std, gen, kq = F.adlist_sample(dev(s), dev(y), 1, seed=5, lens=dev(lens))
    assert kq.tolist() == [L, 3001]
    for q in range(2):
        for idx in (std, gen):
            assert sorted(idx[q, 0, :lens[q]].tolist()) == list(range(lens[q])) and not idx[q, 0, lens[q]:].any()
    ref = AR.loss(d, "D", "PL", "IRFGAN", "exp_1m", "PC", std_idx=std.cpu().numpy(), gen_idx=gen.cpu().numpy(), kq=kq.cpu().numpy(), lens=lens)
    xd = dev(d).requires_grad_(True)
    loss, parts = F.adlist_loss(xd, "D", family="IRFGAN", f_div="PC", std_idx=std, gen_idx=gen, kq=kq, lens=dev(lens), return_parts=True)
    loss.backward()
    gate(parts["loss_q"].cpu().numpy(), ref["loss_q"], torch.from_numpy(ref["E_loss_q"]), "adlist L4096 D loss_q", c=AR.C_ADLIST)
    gate(xd.grad.cpu().numpy(), ref["grad"], torch.from_numpy(ref["E_grad"]), "adlist L4096 D grad", c=AR.C_ADLIST)
    xg = dev(s).requires_grad_(True)
    loss, parts = F.adlist_loss(xg, "G", reward="neg_lp", d_preds=dev(d), samples_per_query=1, temperature=TEMPERATURE, seed=5, lens=dev(lens),
                                return_parts=True)
    loss.backward()
    g = xg.grad.cpu().numpy().astype(np.float64)
    assert torch.equal(parts["gen_idx"], gen) and np.isfinite(g).all() and np.isfinite(parts["loss_q"].cpu().numpy()).all()
    assert not g[1, 3001:].any() and np.abs(g).max() > 0
    assert (np.abs(g.sum(axis=1)) <= 1e-5 * np.abs(g).sum(axis=1)).all()


@gpu
@pytest.mark.parametrize("case", (CASES[3], CASES[5], CASES[7], CASES[9]), ids=lambda c: f"L{c[1]}")
def test_generators_rankings_are_the_samplers(case):
    import ptranking_amd.functional as F
    B, L, S, K, _ = case
    s, d, y, lens = inputs(case)
    seed, q0 = hash_key(case)
    _, gen, kq = F.adlist_sample(dev(s), dev(y), S, top_k=K, seed=seed, q0=q0, lens=dev(lens))
    _, parts = F.adlist_loss(dev(s), "G", d_preds=dev(d), samples_per_query=S, top_k=K, temperature=TEMPERATURE, seed=seed, q0=q0, lens=dev(lens),
                             return_parts=True)
    assert torch.equal(parts["gen_idx"], gen) and torch.equal(parts["valid_q"] > 0, kq > 0)


@gpu
@pytest.mark.parametrize("mode", ("D", "G"))
@pytest.mark.parametrize("case", (CASES[3], CASES[6], CASES[8], CASES[9]), ids=lambda c: f"L{c[1]}")
def test_bits_do_not_depend_on_the_batch(case, mode):
    """A query alone, in the batch, in halves, and a second time: the same bits."""
    for prob, variant in (("PL", variants(mode)[0]), ("BT", variants(mode)[-1])):
        seed, q0 = hash_key(case)
        over = dict(unif=None, seed=seed, q0=q0) if mode == "G" else {}
        full = _launch(case, mode, prob, variant, **over)
        again = _launch(case, mode, prob, variant, **over)
        B = case[0]
        parts = []
        for lo, hi in ((0, 1), (1, B // 2), (B // 2, B)):
            o = dict(over, q0=q0 + lo) if mode == "G" else {}
            parts.append(_launch(case, mode, prob, variant, sl=slice(lo, hi), **o))
        assert np.array_equal(full[2], again[2], equal_nan=True) and np.array_equal(full[0], again[0], equal_nan=True)
        assert np.array_equal(full[2], np.concatenate([p[2] for p in parts]), equal_nan=True)
        assert np.array_equal(full[1]["loss_q"].cpu().numpy(), np.concatenate([p[1]["loss_q"].cpu().numpy() for p in parts]), equal_nan=True)


def golden_cases():
    """[(fields of one case, its slice of the gradient rows, its column of the loss rows)] of tests/golden/adlist.npz."""
    z = np.load(GOLDEN, allow_pickle=False)
    out, at_n, at_u, at_k = [], 0, 0, 0
    for i, (n, S, top_k, K) in enumerate(z["shape"].tolist()):
        f = dict(n=n, S=S, top_k=top_k or None, K=K, x=z["x"][at_n:at_n + n], d=z["d"][at_n:at_n + n], unif=z["unif"][at_u:at_u + S * n].reshape(S, n),
                 gen=z["gen_idx"][at_k:at_k + S * K].reshape(S, K), std=z["std_idx"][at_k:at_k + S * K].reshape(S, K))
        out.append((f, slice(at_n, at_n + n), i))
        at_n, at_u, at_k = at_n + n, at_u + S * n, at_k + S * K
    return z, out


def golden_rows(mode):
    """[(row of the fixture's loss / grad arrays, (family, reward, f_div))]"""
    return list(enumerate(variants(mode)))


def golden_call(f, mode):
    """(x [1, n], keyword arguments of adlist_ref.loss) of one golden case as a batch of one query."""
    n, S, K = f["n"], f["S"], f["K"]
    if mode == "D":
        Kw = AR.kw_of(f["top_k"], n)
        pad = lambda a: np.concatenate([a, np.zeros((S, Kw - K), np.int64)], axis=1)[None]
        return f["d"][None], dict(std_idx=pad(f["std"]), gen_idx=pad(f["gen"]), kq=np.array([K], np.int32))
    return f["x"][None], dict(d_preds=f["d"][None], S=S, top_k=f["top_k"], T=float(np.load(GOLDEN)["temperature"][0]), unif=f["unif"][None])


@gpu
@pytest.mark.parametrize("prob", ("PL", "BT"))
@pytest.mark.parametrize("mode", ("D", "G"))
def test_golden_runs_of_the_reference(mode, prob):
    """The reference's own float64 runs through the C ABI under the project's max-norm plus element-wise gate (golden_util.assert_close):
    every run, all eight divergences and all four rewards, that is finite and inside fp32 range (exp(1 - lp) leaves it from K = 64 on)."""
    import ptranking_amd.functional as F
    z, cases = golden_cases()
    done, failed = 0, []
    for f, cols, i in cases:
        x, kw = golden_call(f, mode)
        for row, (family, reward, f_div) in golden_rows(mode):
            l64, g64 = z[f"{mode}/{prob}/loss64"][row, i], z[f"{mode}/{prob}/grad64"][row, cols]
            if not (np.isfinite(l64) and np.isfinite(g64).all() and max(abs(l64), np.abs(g64).max()) < 1e30):
                continue
            xd = dev(x).requires_grad_(True)
            if mode == "D":
                loss = F.adlist_loss(xd, "D", prob=prob, family=family, f_div=f_div, std_idx=dev(kw["std_idx"]), gen_idx=dev(kw["gen_idx"]), kq=dev(kw["kq"]))
            else:
                loss = F.adlist_loss(xd, "G", prob=prob, family=family, reward=reward, f_div=f_div, d_preds=dev(kw["d_preds"]), samples_per_query=kw["S"],
                                     top_k=kw["top_k"], temperature=kw["T"], unif=dev(kw["unif"]))
            loss.backward()
            what = f"golden {mode} {prob} {family} {reward} {f_div} n{f['n']} S{f['S']} K{f['top_k']}"
            got_l, got_g = loss.detach().cpu().numpy().reshape(1), xd.grad.cpu().numpy()
            try:
                assert_close(got_l, np.array([l64]), what + " loss")
                assert_close(got_g[0], g64, what + " grad")
            except AssertionError as e:
                failed.append(str(e)[:300])
            done += 1
    assert not failed, f"{len(failed)} of {done} runs: " + " | ".join(failed[:6])
    assert done > 0.6 * len(cases) * len(variants(mode))


# ------------------------------------------------------------------------------------------------------------- the machines
def _example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_irgan_list_synthetic as ex
    return ex


def _spied(monkeypatch):
    import ptranking_amd.adversarial as adv
    calls, real_loss, real_sample = [], adv.F_.adlist_loss, adv.F_.adlist_sample

    def loss(x, mode, **kw):
        out = real_loss(x, mode, **kw)
        xg = x.detach().clone().requires_grad_(True)                          # the same call again for the gradient the step is made of
        real_loss(xg, mode, **kw).backward()
        calls.append((mode, x.detach().cpu().numpy(), {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in kw.items()}, float(out),
                      xg.grad.cpu().numpy()))
        return out

    def sample(preds, labels, S, **kw):
        out = real_sample(preds, labels, S, **kw)
        calls.append(("S", preds.cpu().numpy(), dict(kw, labels=labels.cpu().numpy(), S=S), [o.cpu().numpy() for o in out], None))
        return out

    monkeypatch.setattr(adv.F_, "adlist_loss", loss)
    monkeypatch.setattr(adv.F_, "adlist_sample", sample)
    return calls


@gpu
@pytest.mark.parametrize("name", ("IRGAN_List", "IRFGAN_List"))
def test_a_batch_of_one_query_is_the_references_step(name, monkeypatch):
    """One query, one pass, a pointsf scorer without BN and dropout: the sampled rankings are the restatement's for the machine's own draws,
    and each player's loss is the reference's one-query loss of that player's scores — against the float64 restatement, to the gate."""
    import ptranking_amd as pa
    import ptranking_amd.functional as F
    ex = _example()
    data = pa.PaddedQueryBatches(ex.synthetic_queries(1, 8, seed=5, min_docs=23, max_docs=23), "cuda:0", presort=True)
    calls = _spied(monkeypatch)
    for seed in range(137, 147):                                              # the first stream whose 10 rankings float64 pins (gaps above 1e-4)
        del calls[:]
        torch.manual_seed(1)
        machine = ex.build_machine(name, 8, "cuda:0", top_k=5, samples_per_query=5)
        machine.seed = seed
        g, d = machine.get_generator(), machine.get_discriminator()
        before = [[p.detach().clone() for p in pl.get_parameters()] for pl in (g, d)]
        assert machine.mini_max_train(train_data=data, generator=g, discriminator=d, global_buffer={}) is False
        for pl, old in zip((g, d), before):
            assert any(not torch.equal(a, p.detach()) for a, p in zip(old, pl.get_parameters()))
        assert [c[0] for c in calls] == (["S", "D", "G"] if machine.ad_training_order == "DG" else ["G", "S", "D"])
        checked = []
        for mode, x, kw, got, grad in calls:
            lens = kw.get("lens")
            if mode == "S":
                unif = F.adlist_uniforms(1, x.shape[1], 5, seed=kw["seed"], q0=kw["q0"]).cpu().numpy()
                std, gen, kq, pinned = AR.sample(x, kw["labels"], lens, 5, kw["top_k"], unif)
                checked.append(bool(pinned.all()))
                assert np.array_equal(got[0], std) and np.array_equal(got[2], kq) and (not pinned.all() or np.array_equal(got[1], gen))
                continue
            common = dict(prob=kw["prob"], family=kw["family"], reward=kw["reward"], f_div=kw["f_div"], lens=lens)
            if mode == "D":
                ref = AR.loss(x, "D", std_idx=kw["std_idx"], gen_idx=kw["gen_idx"], kq=kw["kq"], **common)
            else:
                unif = F.adlist_uniforms(1, x.shape[1], 5, mode="G", seed=kw["seed"], q0=kw["q0"]).cpu().numpy()
                ref = AR.loss(x, "G", d_preds=kw["d_preds"], S=5, top_k=kw["top_k"], T=kw["temperature"], unif=unif, **common)
                checked.append(bool(ref["pinned"].all()))
                if not checked[-1]:
                    continue
            gate(np.array([got]), np.array([ref["loss"]]), torch.tensor([ref["E_loss"]], dtype=torch.float64), f"{name} {mode} step loss", c=AR.C_ADLIST)
            gate(grad, ref["grad"], torch.from_numpy(ref["E_grad"]), f"{name} {mode} step gradient", c=AR.C_ADLIST)
        if all(checked):
            break
    assert all(checked), "no stream of ten pinned every ranking"


@gpu
@pytest.mark.parametrize("order", ("DG", "GD"))
def test_schedule_follows_the_reference(order, monkeypatch):
    """d_epoches = 3, g_epoches = 2: per batch the discriminator's three steps with the rankings refreshed at d_epoch 0 and 2 (g_mod = 2), the
    generator's two steps before or after them as the order says; every draw takes a seed of its own."""
    import ptranking_amd as pa
    ex = _example()
    data = pa.PaddedQueryBatches(ex.synthetic_queries(12, 8, seed=5), "cuda:0", rough_batch_size=256, presort=True)
    machine = ex.build_machine("IRGAN_List", 8, "cuda:0", ad_training_order=order, d_epoches=3, g_epoches=2)
    calls = _spied(monkeypatch)
    machine.mini_max_train(train_data=data, generator=machine.get_generator(), discriminator=machine.get_discriminator(), global_buffer={})
    d_part, g_part = ["S", "D", "D", "S", "D"], ["G", "G"]
    per_batch = d_part + g_part if order == "DG" else g_part + d_part
    assert [c[0] for c in calls] == per_batch * len(list(data))
    seeds = [c[2]["seed"] for c in calls if c[0] in "SG"]
    assert len(set(seeds)) == len(seeds)
    q0s = [c[2]["q0"] for c in calls if c[0] == "S"]
    assert q0s[0] == 0 and sorted(set(q0s)) == sorted(set(np.cumsum([0] + [len(b[0]) for b in data][:-1]).tolist()))
    one = ex.build_machine("IRGAN_List", 8, "cuda:0", ad_training_order=order, d_epoches=1, g_epoches=1)
    del calls[:]
    one.mini_max_train(train_data=data, generator=one.get_generator(), discriminator=one.get_discriminator(), global_buffer={})
    assert [c[0] for c in calls] == (["S", "D", "G"] if order == "DG" else ["G", "S", "D"]) * len(list(data))


@gpu
@pytest.mark.parametrize("name", ("IRGAN_List", "IRFGAN_List"))
def test_machines_lift_ndcg_on_a_planted_signal(name):
    """30 mini-max rounds on 64 synthetic queries: both players' nDCG@5 stay finite and the discriminator, the player that sees the labels,
    ends above where it started (the generator's figure is printed: on presorted lists a generator that collapses to equal scores reads
    as nDCG 1, so its rise proves nothing)."""
    import ptranking_amd as pa
    ex = _example()
    data = pa.PaddedQueryBatches(ex.synthetic_queries(64, 16, seed=3), "cuda:0", rough_batch_size=256, presort=True)
    machine = ex.build_machine(name, 16, "cuda:0")
    hist = np.array(ex.run(machine, data, 30, log=lambda *_: None))
    print(f"MEASURED {name}: G nDCG@5 {hist[0, 0]:.4f} -> {hist[-1, 0]:.4f}, D nDCG@5 {hist[0, 1]:.4f} -> {hist[-1, 1]:.4f}")
    assert hist.shape == (31, 2) and np.isfinite(hist).all()
    assert hist[-1, 1] > hist[0, 1] + 0.1


def _two_rank_worker(rank, world, port, order, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", PTR_DP_BACKEND="gloo")
    import torch.distributed as dist
    from ptranking_amd import dp
    dp.init_from_env()
    torch.save(_one_step(order, rank, world), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _one_step(order, rank=0, world=1):
    """One mini-max pass of IRGAN_List over this rank's share of 8 queries -> both players' flat parameters and gradients after it."""
    import ptranking_amd as pa
    ex = _example()
    queries = list(ex.synthetic_queries(8, 8, seed=9, min_docs=20, max_docs=20))
    share = len(queries) // world
    data = pa.PaddedQueryBatches(queries[rank * share:(rank + 1) * share], "cuda:0", presort=True)
    torch.manual_seed(21)
    machine = ex.build_machine("IRGAN_List", 8, "cuda:0", lr=1e-2, ad_training_order=order)
    machine.first_query = rank * share
    g, d = machine.get_generator(), machine.get_discriminator()
    machine.mini_max_train(train_data=data, generator=g, discriminator=d, global_buffer={})
    flat = lambda ts: torch.cat([t.detach().reshape(-1).cpu() for t in ts])
    return {"g": flat(g.get_parameters()), "d": flat(d.get_parameters()), "g_grad": flat(p.grad for p in g.get_parameters() if p.grad is not None),
            "d_grad": flat(p.grad for p in d.get_parameters() if p.grad is not None)}


@gpu
@pytest.mark.parametrize("order", ("DG", "GD"))
def test_a_two_rank_step(order, tmp_path):
    """Two ranks on one GPU over gloo, four queries each with their global query indices: the replicas stay bit-identical in parameters and
    gradients, and the exchanged gradient of the player that steps FIRST ('DG' the discriminator, 'GD' the generator: it sees the initial
    players alone) is the single process's over all eight queries (the losses are sums over queries, the draws are keyed by q0 + q).  The
    second player's gradient follows an Adam step of the first and is compared between the replicas only."""
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_two_rank_worker, args=(2, port, order, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{i}.pt") for i in range(2))
    one = _one_step(order)
    for k in ("g", "d", "g_grad", "d_grad"):
        assert torch.equal(r0[k], r1[k]), "replicas diverged"
    first = "d_grad" if order == "DG" else "g_grad"
    assert float(one[first].abs().max()) > 0
    scale = max(1.0, float(one[first].abs().max()))
    assert float((r0[first] - one[first]).abs().max()) <= 2e-5 * scale


@gpu
def test_the_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_irgan_list_synthetic.py"), "--queries", "48", "--epochs", "2"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if " epoch " in l]
    assert len(lines) == 6 and all("G nDCG@5" in l and "D nDCG@5" in l for l in lines), out.stdout
