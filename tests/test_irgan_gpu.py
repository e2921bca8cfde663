"""GPU: the IRGAN point and pair kernels (csrc/irgan.hip) against the restatement (tests/irgan_ref.py), and the two machines.

Loss maths: loss_q, loss_out and every gradient element of ptr_irgan_point_gen_fwd_bwd (on the kernel's own counts) and of every form of
ptr_irgan_sel_fwd_bwd are gated element-wise by tests/f64_bounds.py `gate` against the float64 restatement, E = C_IRGAN x the restatement's
first-order bound.  C_IRGAN follows the project's rule for C_METRIC: the need of the float32 CPU restatement on THESE cases, doubled,
rounded up to a half, capped at 4 (tests/test_irgan_cpu.py recomputes it).
    MEASURED need at c = 1:  fp32 CPU restatement 0.63 (the gradient of PAIR_D_LOG) -> C_IRGAN 1.5;  kernels on the MI355X 0.60 (the same
    gradient; POINT_D 0.54, PAIR_D_SVM 0.44, PAIR_G_* 0.25, the generator step of IRGAN_Point 0.16).
Sampler with supplied uniforms: exact equality of pos_idx, neg_idx, nsel and counts with the restatement; the uniforms are redrawn on the
CPU until no with-replacement draw lies within 2^-12 of a float64 CDF boundary and the competing Gumbel keys are 1e-4 apart, and the
condition is asserted: no case is left out.  Sampler with the hash: irgan_uniforms reproduces the draws, two calls agree, a shard with q0
gives the whole batch's rows, chi-square of each mode against the exact law at p = 1e-4 (fixed seed); the generator step's hash counts
differ from the float64 restatement's on the same uniforms by no more than its unpinned draws can move (a pinned draw lands where float64
puts it; an unpinned one may move one count between two documents: |counts - float64|_1 <= 2 x unpinned per query).
    MEASURED on the MI355X: 0 counts moved on every list up to 257 documents (up to 1 050 draws, 122 of them unpinned); at L = 4096
    the distance is 2 (one draw of 6 825, 3 632 unpinned) and 8 (four draws of 17 735, 9 521 unpinned).
Shapes: B 5..9; L 1, 2, 63, 64, 65, 130, the form boundary 256 and 255 / 257, PTR_MAX_LIST_LEN; ragged lens with 0; S 1, 5, 64; scores
spread over 200 units; a NaN score; T 0.5 and 1.  num_pos 0, 1, n-1, n reach BOTH forms of ptr_irgan_sample (every mode, supplied
uniforms and the hash) and, on the hash route, of ptr_irgan_point_gen_fwd_bwd: its loss gate and hash checks draw 5 P documents with P
up to n (20 475 draws at L = 4096: many passes of the draw loop, streams beyond 0, four waves on the LDS counters).  Only the generator
step's SUPPLIED-uniform equality test caps num_pos, at 3 beyond 130 documents (`few`): the boosted positives sit lambda / P of the total
apart, so with hundreds of them no uniform keeps 2^-12 from every boundary; there it reaches n-1 and n in the wavefront form alone
(test_cases_reach_every_form asserts all of this per entry point)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import irgan_ref as IR
from f64_bounds import gate
from launch_form import launch_form
from plsample_ref import uniforms_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
LAM, DPP = 0.5, 5
#        B  L     S   T    spread  nan
CASES = ((5, 1, 1, 1.0, 0, False),
         (6, 2, 5, 0.5, 0, False),
         (7, 63, 5, 0.5, 0, False),
         (8, 64, 64, 1.0, 0, False),
         (9, 65, 5, 0.5, 200, False),
         (5, 130, 64, 0.5, 0, True),
         (6, 255, 5, 1.0, 200, False),
         (7, 256, 64, 0.5, 200, True),
         (8, 257, 1, 0.5, 200, False),
         (5, 4096, 5, 1.0, 200, False))
IDS = [f"{c[0]}x{c[1]}-S{c[2]}-T{c[3]:g}" for c in CASES]
SAMPLE_MODES = ("POINT_D", "PAIR_D", "PAIR_G")
SEL_MODES = ("POINT_D", "PAIR_D_SVM", "PAIR_D_LOG", "PAIR_G_SVM", "PAIR_G_LOG")
CHI2_1E4 = {4: 23.513, 6: 27.857}        # chi-square quantiles at 1 - 1e-4 by degrees of freedom


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Scores, the discriminator's outputs, ragged lens (a full list, an empty one) and num_pos cycling through n/2, 0, 1, n-1, n, n/3.
    `few` caps num_pos at 3 beyond 130 documents, for the generator step's supplied-uniform equality test alone (gen_case)."""
    B, L, S, T, spread, nan = case
    g = np.random.default_rng(1000 * L + B)
    s = g.standard_normal((B, L)).astype(np.float32)
    if spread:
        s = (s + g.uniform(-spread / 2, spread / 2, size=(B, L))).astype(np.float32)
    d = g.random((B, L), dtype=np.float32)
    lens = g.integers(1, L + 1, size=B).astype(np.int32)
    lens[0] = L
    lens[1] = 0
    if nan:
        s[2, int(lens[2]) // 2] = np.nan
    cyc = lambda n, q: [n // 2, 0, 1, n - 1, n, n // 3][q % 6]
    num_pos = np.array([max(0, min(int(lens[q]), cyc(int(lens[q]), q + B))) for q in range(B)], np.int32)
    few = np.minimum(num_pos, 3) if L > 130 else num_pos
    return s, d, lens, num_pos, few.astype(np.int32)


def _redraw(rng, unif, offenders):
    unif[offenders] = rng.random(int(offenders.sum()), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def sample_case(case, mode):
    """(unif [B, 2, L], pos, neg, nsel) with every draw pinned (asserted)."""
    B, L, S, T, *_ = case
    s, _, lens, P, _ = inputs(case)
    rng = np.random.default_rng(7 + L)
    unif = rng.random((B, 2, L), dtype=np.float32)
    for _ in range(200):
        pos, neg, nsel, pinned = IR.sample(s, P, lens, S, mode, T, unif)
        if pinned.all():
            break
        for q in np.nonzero(~pinned)[0]:
            unif[q, 1] = rng.random(L, dtype=np.float32)
    assert pinned.all(), (case, mode)
    return unif, P, pos, neg, nsel


@functools.lru_cache(maxsize=None)
def gen_case(case):
    """(unif [B, DPP, L], counts) with every draw 2^-12 away from a CDF boundary (asserted)."""
    B, L, S, T, *_ = case
    s, _, lens, _, few = inputs(case)
    rng = np.random.default_rng(13 + L)
    unif = rng.random((B, DPP, L), dtype=np.float32)
    for _ in range(200):
        counts, pinned = IR.gen_counts(s, few, lens, T, LAM, DPP, unif)
        if pinned.all():
            break
        _redraw(rng, unif.reshape(B, -1), ~pinned)
    assert pinned.all(), case
    return unif, counts


def hash_key(case):
    """(seed, q0) of a case's hash route: both beyond 32 bits."""
    return 2 ** 40 + 17 * case[1], 2 ** 33 + 5


@functools.lru_cache(maxsize=None)
def hash_gen_case(case):
    """The generator step on the hash route with the UNCAPPED num_pos, restated on the host: (counts, unpinned draws per query [B]) from
    the host's restatement of the counter hash.  The kernel's counts agree up to the draws that float64 does not pin."""
    B, L, S, T, *_ = case
    s, _, lens, num_pos, _ = inputs(case)
    seed, q0 = hash_key(case)
    counts, pinned = IR.gen_counts(s, num_pos, lens, T, LAM, DPP, uniforms_host(B, L, DPP, seed, q0))
    return counts, (~pinned).sum(axis=1)


@functools.lru_cache(maxsize=None)
def sel_case(case, mode):
    """(x, nsel, d_sel, neg_idx) of a selected-documents call; no hinge within 1e-3 of its kink (asserted)."""
    B, L, S, T, *_ = case
    s, _, lens, num_pos, _ = inputs(case)
    rng = np.random.default_rng(29 + L + len(mode))
    d_sel = (3.0 * rng.standard_normal((B, 2 * S))).astype(np.float32)
    if mode.startswith("PAIR_G"):
        _, _, _, neg, nsel = sample_case(case, "PAIR_G")
        x, neg_idx = s, neg
    else:
        nsel = rng.integers(0, S + 1, size=B).astype(np.int32)
        nsel[0], nsel[1] = S, 0
        x, neg_idx = d_sel, None
    for q in range(B):
        V = int(nsel[q])
        assert (np.abs(1.0 - (d_sel[q, :V] - d_sel[q, V:2 * V])) > 1e-3).all()
    return x, nsel, d_sel, neg_idx


def fp32_restatement_need():
    """The worst err / E (c = 1) of the float32 CPU restatement against the float64 one over every loss case of this module."""
    worst = 0.0

    def judge(a, b, E):
        nonlocal worst
        a, b, E = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(E, np.float64)
        m = np.isfinite(b) & (E > 0)
        if m.any():
            worst = max(worst, float((np.abs(a - b)[m] / E[m]).max()))

    for case in CASES:
        B, L, S, T, *_ = case
        s, d, lens, num_pos, few = inputs(case)
        for P, counts in ((num_pos, hash_gen_case(case)[0]), (few, gen_case(case)[1])):
            r64 = IR.point_generator(s, d, P, lens, T, LAM, counts, c=1.0)
            r32 = IR.point_generator(s, d, P, lens, T, LAM, counts, dtype=torch.float32)
            judge(r32["loss_q"], r64["loss_q"], r64["E_loss_q"])
            judge(r32["grad"], r64["grad"], r64["E_grad"])
        for mode in SEL_MODES:
            x, nsel, d_sel, neg_idx = sel_case(case, mode)
            kw = dict(d_sel=d_sel, neg_idx=neg_idx, lens=lens, T=T) if mode.startswith("PAIR_G") else {}
            r64 = IR.selected(x, nsel, mode, c=1.0, **kw)
            r32 = IR.selected(x, nsel, mode, dtype=torch.float32, **kw)
            judge(r32["loss_q"], r64["loss_q"], r64["E_loss_q"])
            judge(r32["grad"], r64["grad"], r64["E_grad"])
    return worst


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_cases_reach_every_form():
    """The case list launches every form of the three entry points, on both sides of the boundary, and holds the shapes the header names."""
    Ls = {c[1] for c in CASES}
    assert {1, 2, 63, 64, 65, 130, 255, 256, 257, 4096} <= Ls and {c[0] for c in CASES} == {5, 6, 7, 8, 9}
    assert {c[2] for c in CASES} == {1, 5, 64} and {c[3] for c in CASES} == {0.5, 1.0}
    for entry in ("ptr_irgan_sample", "ptr_irgan_point_gen_fwd_bwd"):
        forms = {L: launch_form(entry, L)[:2] for L in Ls}
        assert set(forms.values()) == {(64, 4), (256, 1)}
        assert forms[256] == (64, 4) and forms[257] == (256, 1) and forms[255] == (64, 4) and forms[4096] == (256, 1)
        assert launch_form(entry, 4096) and max(Ls) == 4096               # PTR_MAX_LIST_LEN
    sel = {(m, launch_form("ptr_irgan_sel_fwd_bwd", IR.SEL_MODES[m], L)[:2]) for m in SEL_MODES for L in Ls}
    assert sel == {(m, (64, 4)) for m in SEL_MODES} | {(m, (256, 1)) for m in SEL_MODES[3:]}
    # num_pos per entry point and form.  `num_pos` serves ptr_irgan_sample (every mode, both routes) and the hash route of
    # ptr_irgan_point_gen_fwd_bwd (the loss gate, the hash checks); `few` serves that entry's supplied-uniform equality test alone.
    seen = {(which, G): set() for which in ("num_pos", "few") for G in (64, 256)}
    clip_p, clip_n, clip_s, many = False, False, False, 0
    for case in CASES:
        s, _, lens, num_pos, few = inputs(case)
        assert lens.min() == 0 and lens.max() == case[1]
        G = launch_form("ptr_irgan_point_gen_fwd_bwd", case[1])[0]
        assert G == launch_form("ptr_irgan_sample", case[1])[0]
        for which, Ps in (("num_pos", num_pos), ("few", few)):
            for n, p in zip(lens, Ps):
                seen[which, G] |= {"0"} if p == 0 else set()
                seen[which, G] |= {"1"} if p == 1 else set()
                seen[which, G] |= {"n-1"} if n > 2 and p == n - 1 else set()
                seen[which, G] |= {"n"} if n > 1 and p == n else set()
        for n, p in zip(lens, num_pos):
            V = min(p, n - p, case[2])
            clip_p |= V == p and 0 < p < min(n - p, case[2])
            clip_n |= V == n - p and 0 < n - p < min(p, case[2])
            clip_s |= V == case[2] and case[2] < min(p, n - p)
            if G == 256:
                many = max(many, DPP * int(p))
    assert seen["num_pos", 64] == seen["num_pos", 256] == {"0", "1", "n-1", "n"} and clip_p and clip_n and clip_s
    assert seen["few", 64] == {"0", "1", "n-1", "n"} and seen["few", 256] == {"0", "1"}    # the cap: the header says why
    # the workgroup form's draw loop: many passes of 256 threads, and draws whose stream index k / L is beyond 0
    assert many > 2 * max(Ls) and many > 16 * 256
    assert any(c[4] >= 200 for c in CASES) and sum(c[5] for c in CASES) >= 1
    for case in (c for c in CASES if c[4]):                                   # a plain fp32 softmax underflows on the spread scores
        s, _, lens, *_ = inputs(case)
        z = s[0, :lens[0]] / np.float32(case[3])
        assert (np.exp(z - z.max()) == 0).any()


def test_mini_max_train_calls_the_pieces_in_the_references_order():
    import ptranking_amd as pa
    from ptranking_amd.adversarial import DEFAULT_AD_PARAS
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
          "pointsf": dict(num_features=4, num_layers=2, AF="R", TL_AF="S", apply_tl_af=True, BN=False, bn_type=None, bn_affine=False)}
    for name in pa.AD_RANKER_NAMES:
        for order, want in (("DG", ["gen", "d"] + ["d"] * 9 + ["gen", "d", "g", "g"]), ("GD", ["g", "g", "gen", "d"] + ["d"] * 9 + ["gen", "d"])):
            ad = dict(DEFAULT_AD_PARAS[name], ad_training_order=order, d_epoches=11, g_epoches=2)
            m = getattr(pa, name)(None, dict(train_presort=True), sf_para_dict=dict(sf, pointsf=dict(sf["pointsf"])), ad_para_dict=ad, gpu=False,
                                  device="cpu")
            calls = []
            m.generate_data = lambda **k: calls.append("gen") or {"token": len(calls)}
            m.train_discriminator = lambda **k: calls.append("d") or (k["generated_data"] is not None or pytest.fail("no generated data"))
            m.train_generator = lambda **k: calls.append("g") or False
            assert m.mini_max_train(train_data=[], generator=m.get_generator(), discriminator=m.get_discriminator(), global_buffer={}) is False
            assert calls == want, (name, order, calls)
        # a NaN in the generator's step ends the round at once
        m.train_generator = lambda **k: True
        m.generate_data = lambda **k: pytest.fail("training went on after stop_training")
        assert m.mini_max_train(train_data=[], generator=None, discriminator=None, global_buffer={}) is True


# ------------------------------------------------------------------------------------------------------------- the sampler
@gpu
@pytest.mark.parametrize("mode", SAMPLE_MODES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sampler_with_supplied_uniforms_equals_the_restatement(case, mode):
    import ptranking_amd.functional as F
    B, L, S, T, *_ = case
    s, _, lens, *_ = inputs(case)
    unif, P, pos, neg, nsel = sample_case(case, mode)
    got = F.irgan_sample(dev(s), dev(P), S, mode, temperature=T, lens=dev(lens), unif=dev(unif))
    assert np.array_equal(got[2].cpu().numpy(), nsel)
    assert np.array_equal(got[0].cpu().numpy(), pos) and np.array_equal(got[1].cpu().numpy(), neg)
    for q in range(B):
        V = int(nsel[q])
        assert len(set(pos[q, :V].tolist())) == V and (pos[q, :V] < max(P[q], 1)).all()
        if mode != "POINT_D":
            assert len(set(neg[q, :V].tolist())) == V and (mode != "PAIR_D" or (neg[q, :V] >= P[q]).all())


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sampler_with_the_hash(case):
    import ptranking_amd.functional as F
    B, L, S, T, *_ = case
    s, d, lens, num_pos, few = inputs(case)
    sd, ld = dev(s), dev(lens)
    seed, q0 = hash_key(case)
    for mode in SAMPLE_MODES:
        P = dev(num_pos)
        a = F.irgan_sample(sd, P, S, mode, temperature=T, seed=seed, q0=q0, lens=ld)
        b = F.irgan_sample(sd, P, S, mode, temperature=T, seed=seed, q0=q0, lens=ld)
        u = F.irgan_sample(sd, P, S, mode, temperature=T, lens=ld, unif=F.irgan_uniforms(B, L, 2, seed=seed, q0=q0))
        sh = F.irgan_sample(sd[3:], P[3:], S, mode, temperature=T, seed=seed, q0=q0 + 3, lens=ld[3:])
        for x, y, z, w in zip(a, b, u, sh):
            assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x[3:], w), mode
        pos, neg, nsel = (t.cpu().numpy() for t in a)
        Pn = P.cpu().numpy()
        for q in range(B):
            V = int(nsel[q])
            n = int(lens[q])
            assert V == (min(Pn[q], S) if mode == "POINT_D" else min(Pn[q], n - Pn[q], S)) or np.isnan(s[q, :n]).any()
            assert (pos[q, V:] == 0).all() and (neg[q, V:] == 0).all()
            assert len(set(pos[q, :V].tolist())) == V and (V == 0 or (pos[q, :V].max() < Pn[q] and neg[q, :V].max() < n and neg[q, :V].min() >= 0))
            if mode != "POINT_D":
                assert len(set(neg[q, :V].tolist())) == V and (mode != "PAIR_D" or (neg[q, :V] >= Pn[q]).all())
    kw = dict(temperature=T, lam=LAM, draws_per_pos=DPP, lens=ld, return_parts=True)
    # the generator step with the uncapped num_pos: up to 5 n draws per query
    dd, Pd = dev(d), dev(num_pos)
    a = F.irgan_point_generator(sd, dd, Pd, seed=seed, q0=q0, **kw)[1]["counts"]
    b = F.irgan_point_generator(sd, dd, Pd, seed=seed, q0=q0, **kw)[1]["counts"]
    u = F.irgan_point_generator(sd, dd, Pd, unif=F.irgan_uniforms(B, L, DPP, seed=seed, q0=q0), **kw)[1]["counts"]
    sh = F.irgan_point_generator(sd[3:], dd[3:], Pd[3:], seed=seed, q0=q0 + 3, **dict(kw, lens=ld[3:]))[1]["counts"]
    assert torch.equal(a, b) and torch.equal(a, u) and torch.equal(a[3:], sh)
    nanq = np.array([np.isnan(s[q, :lens[q]]).any() for q in range(B)])
    got = a.cpu().numpy()
    assert (got >= 0).all() and np.array_equal(got.sum(axis=1), np.where(nanq, 0, DPP * num_pos))
    assert (got[np.arange(L)[None, :] >= lens[:, None]] == 0).all()
    # against float64 on the host's restatement of the hash: a pinned draw lands where float64 puts it, an unpinned one may move one count
    # from one document to another
    want, unpinned = hash_gen_case(case)
    moved = np.abs(got.astype(np.int64) - want).sum(axis=1)
    print(f"MEASURED hash counts {case}: draws {want.sum(axis=1).tolist()}, unpinned {unpinned.tolist()}, |counts - float64|_1 {moved.tolist()}")
    assert (moved <= 2 * unpinned).all(), (moved, unpinned)


def _chi_square(counts, p):
    keep = p > 0
    assert counts[~keep].sum() == 0
    e = counts.sum() * p[keep]
    return float(((counts[keep] - e) ** 2 / e).sum()), int(keep.sum()) - 1


@gpu
@pytest.mark.parametrize("mode", SAMPLE_MODES)
def test_sampler_frequencies_follow_the_law(mode):
    """24 000 first draws of one 7-document query (the same list in every row: a row's stream is keyed by its query index) against the exact
    law, chi-square at p = 1e-4; the positives are uniform over 0 .. P-1."""
    import ptranking_amd.functional as F
    N, P, T = 24000, 2, 0.5
    s = np.array([0.8, -0.3, 0.1, 1.2, -1.0, 0.4, -0.1], np.float32)
    rows = dev(np.tile(s, (N, 1)))
    pos, neg, nsel = F.irgan_sample(rows, torch.full((N,), P, dtype=torch.int32, device="cuda"), 1, mode, temperature=T, seed=12345, q0=0)
    assert int(nsel.min()) == 1
    chi, dof = _chi_square(np.bincount(neg[:, 0].cpu().numpy(), minlength=7).astype(np.float64), IR.sample_probabilities(s, P, mode, T))
    print(f"MEASURED chi-square {mode}: {chi:.2f} at {dof} degrees of freedom")
    assert chi < CHI2_1E4[dof], (mode, chi)
    first = np.bincount(pos[:, 0].cpu().numpy(), minlength=P)
    assert abs(first[0] / N - 0.5) < 4.0 * 0.5 / np.sqrt(N)


@gpu
def test_generator_draw_frequencies_follow_the_importance_distribution():
    import ptranking_amd.functional as F
    N, P, T = 5000, 2, 0.5
    s = np.array([0.8, -0.3, 0.1, 1.2, -1.0, 0.4, -0.1], np.float32)
    rows = dev(np.tile(s, (N, 1)))
    _, parts = F.irgan_point_generator(rows, torch.rand(N, 7, device="cuda"), torch.full((N,), P, dtype=torch.int32, device="cuda"), temperature=T,
                                       lam=LAM, draws_per_pos=DPP, seed=99, return_parts=True)
    counts = parts["counts"].sum(dim=0).cpu().numpy().astype(np.float64)
    assert counts.sum() == N * DPP * P
    w = IR.gen_weights(s, P, T, LAM)
    chi, dof = _chi_square(counts, w / w.sum())
    print(f"MEASURED chi-square generator draws: {chi:.2f} at {dof} degrees of freedom")
    assert chi < CHI2_1E4[dof]


# ------------------------------------------------------------------------------------------------------------- the loss maths
def _gate_rows(got, ref, E, what):
    """gate() with the NaN rows of the reference taken out first: they must be NaN in `got`, entry by entry."""
    got, ref, E = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(E, np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    return gate(np.where(nan, 0.0, got), np.where(nan, 0.0, ref), torch.from_numpy(np.where(nan, 0.0, E)), what, c=IR.C_IRGAN)


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_generator_step_of_irgan_point(case):
    """The loss gate on the kernel's own counts, twice: the hash route with the uncapped num_pos (up to 5 n draws per query, every form),
    and the supplied-uniform route (`few`), whose counts must also equal the restatement's."""
    B, L, S, T, *_ = case
    s, d, lens, num_pos, few = inputs(case)
    unif, counts = gen_case(case)
    seed, q0 = hash_key(case)
    for P, route in ((num_pos, dict(seed=seed, q0=q0)), (few, dict(unif=dev(unif)))):
        _gate_generator_step(case, P, route, counts if "unif" in route else None)


def _gate_generator_step(case, P, route, counts):
    import ptranking_amd.functional as F
    B, L, S, T, *_ = case
    s, d, lens, *_ = inputs(case)
    g = dev(s).requires_grad_(True)
    loss, parts = F.irgan_point_generator(g, dev(d), dev(P), temperature=T, lam=LAM, draws_per_pos=DPP, lens=dev(lens), return_parts=True, **route)
    loss.backward()
    got_counts = parts["counts"].cpu().numpy()
    if counts is not None:
        assert np.array_equal(got_counts, counts)
    ref = IR.point_generator(s, d, P, lens, T, LAM, got_counts)
    assert np.array_equal(parts["valid_q"].cpu().numpy(), ref["valid_q"])
    _gate_rows(parts["loss_q"].cpu().numpy(), ref["loss_q"], ref["E_loss_q"], f"irgan point_gen loss_q {case}")
    _gate_rows(g.grad.cpu().numpy(), ref["grad"], ref["E_grad"], f"irgan point_gen grad {case}")
    pad = np.arange(L)[None, :] >= lens[:, None]
    assert (g.grad.cpu().numpy()[pad] == 0).all()
    if np.isnan(ref["loss"]):
        assert torch.isnan(loss)
    else:
        gate(loss.detach().cpu().numpy().reshape(1), np.array([ref["loss"]]), torch.tensor([ref["E_loss"]], dtype=torch.float64), f"irgan point_gen loss_out {case}", c=IR.C_IRGAN)


@gpu
@pytest.mark.parametrize("mode", SEL_MODES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_losses_on_selected_documents(case, mode):
    import ptranking_amd.functional as F
    B, L, S, T, *_ = case
    _, _, lens, *_ = inputs(case)
    x, nsel, d_sel, neg_idx = sel_case(case, mode)
    xd = dev(x).requires_grad_(True)
    if mode.startswith("PAIR_G"):
        loss, parts = F.irgan_selected(xd, dev(nsel), mode, d_sel=dev(d_sel), neg_idx=dev(neg_idx), temperature=T, lens=dev(lens), return_parts=True)
        ref = IR.selected(x, nsel, mode, d_sel=d_sel, neg_idx=neg_idx, lens=lens, T=T)
    else:
        loss, parts = F.irgan_selected(xd, dev(nsel), mode, return_parts=True)
        ref = IR.selected(x, nsel, mode)
    loss.backward()
    assert np.array_equal(parts["valid_q"].cpu().numpy(), ref["valid_q"])
    _gate_rows(parts["loss_q"].cpu().numpy(), ref["loss_q"], ref["E_loss_q"], f"irgan sel {mode} loss_q {case}")
    _gate_rows(xd.grad.cpu().numpy(), ref["grad"], ref["E_grad"], f"irgan sel {mode} grad {case}")
    if np.isnan(ref["loss"]):
        assert torch.isnan(loss)
    else:
        gate(loss.detach().cpu().numpy().reshape(1), np.array([ref["loss"]]), torch.tensor([ref["E_loss"]], dtype=torch.float64), f"irgan sel {mode} loss_out {case}", c=IR.C_IRGAN)


# ------------------------------------------------------------------------------------------------------------- the machines
@gpu
@pytest.mark.parametrize("name,loss_type", [("IRGAN_Point", "svm"), ("IRGAN_Pair", "svm"), ("IRGAN_Pair", "log")])
def test_machines_train_on_a_planted_signal(name, loss_type):
    """20 mini-max rounds on 64 synthetic queries: both players' nDCG@5 stay finite and the discriminator ends above where it started."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_irgan_synthetic as ex
    import ptranking_amd as pa
    data = pa.PaddedQueryBatches(ex.synthetic_queries(64, 16, seed=3), "cuda:0", rough_batch_size=256, presort=True)
    machine = ex.build_machine(name, 16, "cuda:0", loss_type=loss_type)
    hist = np.array(ex.run(machine, data, 20, log=lambda *_: None))
    print(f"MEASURED {name} {loss_type}: G nDCG@5 {hist[0, 0]:.4f} -> {hist[-1, 0]:.4f}, D nDCG@5 {hist[0, 1]:.4f} -> {hist[-1, 1]:.4f}")
    assert hist.shape == (21, 2) and np.isfinite(hist).all()
    assert hist[-1, 1] > hist[0, 1]


@gpu
def test_the_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_irgan_synthetic.py"), "--queries", "48", "--epochs", "2"], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if " epoch " in l]
    assert len(lines) == 6 and all("G nDCG@5" in l and "D nDCG@5" in l for l in lines), out.stdout
