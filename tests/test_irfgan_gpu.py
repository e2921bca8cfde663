"""GPU: the IRFGAN point and pair kernels (csrc/irfgan.hip) against the restatement (tests/irfgan_ref.py), and the two machines.

Samplers with supplied uniforms: exact equality, index for index, of every output with the restatement.  The uniforms are redrawn on the
CPU until float64 pins every draw — no Gumbel key within 1e-4 of its competitor, no true-pair draw within true_margin(n, P) of a boundary
of the flat CDF, no Bernoulli uniform within the sigmoid's fp32 bound of its threshold — and the condition is asserted: no draw is left
out.  Samplers with the hash: irfgan_uniforms reproduces the draws and bern_count bit for bit, two calls agree, a shard with q0 gives the
whole batch's rows, and a list padded to L = 256 (wavefront form) and to L = 257 (workgroup form) draws the same.  Laws by chi-square at
p = 1e-4 with fixed seeds.
Losses: loss_q, loss_out and every gradient element of every mode x every divergence are gated element-wise by tests/f64_bounds.py `gate`
against the float64 restatement, E = C_IRFGAN x its first-order bound; C_IRFGAN follows the project's rule for C_METRIC (the need of the
float32 CPU restatement on THESE cases, doubled, rounded up to a half, capped at 4; tests/test_irfgan_cpu.py recomputes it).
    MEASURED need at c = 1:  fp32 CPU restatement 0.72 (the gradient of PAIR_D under TVar) -> C_IRFGAN 1.5;  kernels on the MI355X 0.73
    (the gradients of POINT_D and PAIR_D; their losses 0.25 / 0.48; POINT_G 0.18 loss, 0.31 gradient; PAIR_G 0.32 / 0.20); on the golden
    steep family 0.45 (the gradient of pair_d), where the reference's fp32 run is inf or NaN under SH, JS, GAN (and NC in point_d, pair_d).
    MEASURED chi-square: point fakes 5.44 and 3.35 at 6 degrees of freedom (bound 27.9), true pairs 4.70 at 7 (29.9), fake pairs 10.40
    at 8 (31.8); bern_count's mean 4.494 against 4.500 at a standard error of 0.009.
Shapes: B 5..7; L 1, 2, 3, 63, 64, 65, 130, 256 (wavefront form, one to four rows per lane) and 257, 300 (workgroup form); lens with 0 and
1; S 1, 5, 64; P = 0, P = n, all-equal labels, a NaN score.  num_pos is capped at 16 beyond 130 documents: the true pairs' flat CDF has
about P n boundaries, and with thousands of them no uniform keeps true_margin away from all (P = n is reached up to 130 documents)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import irfgan_ref as FR
from f64_bounds import gate
from golden_util import _load, assert_close
from launch_form import launch_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
#        B  L    S   nan
CASES = ((5, 1, 1, False),
         (6, 2, 5, False),
         (7, 3, 5, False),
         (5, 63, 5, False),
         (6, 64, 64, False),
         (7, 65, 5, True),
         (5, 130, 64, False),
         (6, 256, 5, True),
         (7, 257, 1, False),
         (6, 300, 5, False))
IDS = [f"{c[0]}x{c[1]}-S{c[2]}" for c in CASES]
MODES = ("POINT_D", "PAIR_D", "POINT_G", "PAIR_G")
DIVS = tuple(FR.F_DIVS)
CHI2_1E4 = {6: 27.857, 7: 29.878, 8: 31.828}        # chi-square quantiles at 1 - 1e-4 by degrees of freedom


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Scores, presorted labels, lens (a full list, an empty one, a single document) and num_pos.  Query q is of kind q % 6: half of the
    list relevant; empty; one document; no relevant document (all labels 0); every document relevant (graded); all labels equal and
    positive.  A NaN score, where the case has one, sits in query 0."""
    B, L, S, nan = case
    g = np.random.default_rng(4000 * L + B)
    s = (1.5 * g.standard_normal((B, L))).astype(np.float32)
    lens = g.integers(min(2, L), L + 1, size=B).astype(np.int32)
    lens[0], lens[1], lens[2] = L, 0, min(1, L)
    y = np.zeros((B, L), np.float32)
    for q in range(B):
        n, kind = int(lens[q]), q % 6
        P = {0: n // 2, 1: 0, 2: n, 3: 0, 4: n, 5: n}[kind]
        if L > 130:
            P = min(P, 16)
        grades = np.full(P, 2.0) if kind == 5 else -np.sort(-g.integers(1, 5, size=P)).astype(np.float64)
        if kind == 4 and P >= 2:
            grades[0], grades[-1] = 4.0, 1.0
        y[q, :P] = grades
    if nan:
        s[0, L // 2] = np.nan
    num_pos = (y > 0).sum(axis=1).astype(np.int32)
    return s, y, lens, num_pos


def hash_key(case):
    """(seed, q0) of a case's hash route: both beyond 32 bits."""
    return 2 ** 41 + 19 * case[1], 2 ** 33 + 7


@functools.lru_cache(maxsize=None)
def point_case(case):
    """(unif [B, 2, L], pos, neg, nsel) with every draw pinned (asserted)."""
    B, L, S, _ = case
    s, _, lens, P = inputs(case)
    rng = np.random.default_rng(11 + L)
    unif = rng.random((B, 2, L), dtype=np.float32)
    for _ in range(200):
        pos, neg, nsel, pinned = FR.point_sample(s, P, lens, S, unif)
        if pinned.all():
            break
        for q in np.nonzero(~pinned)[0]:
            unif[q, 1] = rng.random(L, dtype=np.float32)
    assert pinned.all(), case
    return unif, pos, neg, nsel


def _redraw(rng, unif, offenders):
    unif[offenders] = rng.random(int(offenders.sum()), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def pair_case(case):
    """(unif_draw [B, 2, S], unif_bern [B, L, L], the restatement's outputs) with every draw and every bit pinned (asserted)."""
    B, L, S, _ = case
    s, y, lens, P = inputs(case)
    rng = np.random.default_rng(17 + L)
    ud, ub = rng.random((B, 2, S), dtype=np.float32), rng.random((B, L, L), dtype=np.float32)
    for _ in range(200):
        ref = FR.pair_sample(s, y, P, lens, S, ud, ub)
        if not ref["loose_draw"].any() and not ref["loose_bern"].any():
            break
        _redraw(rng, ud[:, 0], ref["loose_draw"])
        _redraw(rng, ub, ref["loose_bern"])
    assert not ref["loose_draw"].any() and not ref["loose_bern"].any(), case
    return ud, ub, ref


@functools.lru_cache(maxsize=None)
def loss_case(case, mode):
    """(x, nsel, d_fake, idx_a, idx_b) of a loss call: nsel with S and 0 among its rows; the generator's modes with a repeated pair, a pair
    with head = tail and an index outside the list."""
    B, L, S, _ = case
    s, _, lens, _ = inputs(case)
    rng = np.random.default_rng(31 + L + 7 * FR.MODES[mode])
    nsel = rng.integers(0, S + 1, size=B).astype(np.int32)
    nsel[0], nsel[1] = S, 0
    if not mode.endswith("_G"):
        return (3.0 * rng.standard_normal((B, (4 if mode == "PAIR_D" else 2) * S))).astype(np.float32), nsel, None, None, None
    nsel[1], nsel[3] = S, 0                                                   # the empty list names nothing; another row has nsel = 0
    n = np.maximum(lens, 1)[:, None]
    idx_a, idx_b = rng.integers(0, n, size=(B, S)), rng.integers(0, n, size=(B, S))
    if S >= 5:
        idx_a[:, 1], idx_b[:, 1] = idx_a[:, 0], idx_b[:, 0]
        idx_b[:, 2] = idx_a[:, 2]
        idx_a[4, 3] = int(lens[4])                                            # outside the list
        idx_b[0, 4] = -1
    d_fake = (3.0 * rng.standard_normal((B, (2 if mode == "PAIR_G" else 1) * S))).astype(np.float32)
    x = np.where(np.isnan(s), np.float32(0.25), s)                            # the losses have no NaN rule: the scores are finite here
    return x, nsel, d_fake, idx_a.astype(np.int64), idx_b.astype(np.int64) if mode == "PAIR_G" else None


def _loss_ref(case, mode, f_div, **kw):
    x, nsel, d_fake, idx_a, idx_b = loss_case(case, mode)
    return FR.loss(x, nsel, mode, f_div, d_fake=d_fake, idx_a=idx_a, idx_b=idx_b, lens=inputs(case)[2], **kw)


def fp32_restatement_need():
    """The worst err / E (c = 1) of the float32 CPU restatement against the float64 one over every loss case of this module."""
    worst = 0.0
    for case in CASES:
        for mode in MODES:
            for f_div in DIVS:
                r64, r32 = _loss_ref(case, mode, f_div, c=1.0), _loss_ref(case, mode, f_div, dtype=torch.float32)
                for k, e in (("loss_q", "E_loss_q"), ("grad", "E_grad")):
                    a, b, E = r32[k], r64[k], r64[e]
                    m = np.isfinite(b) & (E > 0)
                    if m.any():
                        worst = max(worst, float((np.abs(a - b)[m] / E[m]).max()))
    return worst


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_cases_reach_every_form():
    """The case list launches every form of the three entry points, on both sides of the boundary, and holds the shapes the header names."""
    Ls = {c[1] for c in CASES}
    assert {1, 2, 3, 63, 64, 65, 130, 256, 257, 300} == Ls and {c[0] for c in CASES} == {5, 6, 7} and {c[2] for c in CASES} == {1, 5, 64}
    for entry in ("ptr_irfgan_point_sample", "ptr_irfgan_pair_sample"):
        forms = {L: launch_form(entry, L)[:2] for L in Ls}
        assert {L for L, f in forms.items() if f == (64, 4)} == {1, 2, 3, 63, 64, 65, 130, 256}
        assert {L for L, f in forms.items() if f == (256, 1)} == {257, 300}
    got = {(m, launch_form("ptr_irfgan_fwd_bwd", FR.MODES[m], L)[:2]) for m in MODES for L in Ls}
    assert got == {(m, (64, 4)) for m in MODES} | {(m, (256, 1)) for m in MODES[2:]}
    seen = {64: set(), 256: set()}
    for case in CASES:
        s, y, lens, P = inputs(case)
        assert lens.min() == 0 and lens.max() == case[1] and (case[1] == 1 or 1 in lens.tolist())
        assert (np.diff(y, axis=1) <= 0).all() and (y >= 0).all()
        G = launch_form("ptr_irfgan_pair_sample", case[1])[0]
        for q, (n, p) in enumerate(zip(lens, P)):
            seen[G] |= {"P=0"} if n > 1 and p == 0 else set()
            seen[G] |= {"P=n"} if n > 1 and p == n else set()
            seen[G] |= {"equal"} if n > 1 and y[q, 0] == y[q, n - 1] else set()
            seen[G] |= {"usable"} if n > 1 and y[q, 0] != y[q, n - 1] else set()
    assert seen[64] == {"P=0", "P=n", "equal", "usable"} and {"P=0", "equal", "usable"} <= seen[256]      # the cap: the header says why
    assert sum(c[3] for c in CASES) >= 2


# ------------------------------------------------------------------------------------------------------------- the samplers
@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_point_sampler_with_supplied_uniforms_equals_the_restatement(case):
    import ptranking_amd.functional as F
    B, L, S, _ = case
    s, _, lens, P = inputs(case)
    unif, pos, neg, nsel = point_case(case)
    got = F.irfgan_point_sample(dev(s), dev(P), S, lens=dev(lens), unif=dev(unif))
    assert np.array_equal(got[2].cpu().numpy(), nsel)
    assert np.array_equal(got[0].cpu().numpy(), pos) and np.array_equal(got[1].cpu().numpy(), neg)
    for q in range(B):
        V = int(nsel[q])
        assert V == (0 if np.isnan(s[q, :lens[q]]).any() else min(P[q], S))
        assert len(set(pos[q, :V].tolist())) == V == len(set(neg[q, :V].tolist())) and (V == 0 or (pos[q, :V].max() < P[q] and neg[q, :V].max() < lens[q]))


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pair_sampler_with_supplied_uniforms_equals_the_restatement(case):
    import ptranking_amd.functional as F
    B, L, S, _ = case
    s, y, lens, P = inputs(case)
    ud, ub, ref = pair_case(case)
    got = F.irfgan_pair_sample(dev(s), dev(y), dev(P), S, lens=dev(lens), unif_draw=dev(ud), unif_bern=dev(ub), return_count=True)
    th, tt, fh, ft, nsel, count = (t.cpu().numpy() for t in got)
    assert np.array_equal(nsel, ref["nsel"]) and np.array_equal(count, ref["count"])
    for name, a in (("true_head", th), ("true_tail", tt), ("fake_head", fh), ("fake_tail", ft)):
        assert np.array_equal(a, ref[name]), name
    for q in range(B):
        n = int(lens[q])
        usable = n > 0 and not np.isnan(s[q, :n]).any() and y[q, 0] != y[q, n - 1] and P[q] > 0 and count[q] > 0
        assert nsel[q] == (S if usable else 0)
        if usable:
            assert (y[q, th[q]] > y[q, tt[q]]).all() and th[q].max() < P[q] and max(tt[q].max(), fh[q].max(), ft[q].max()) < n
            assert (ub[q, fh[q], ft[q]] < FR._sg(s[q, fh[q]].astype(np.float64) - s[q, ft[q]])).all()      # every fake pair is a set bit


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_samplers_with_the_hash(case):
    import ptranking_amd.functional as F
    B, L, S, _ = case
    s, y, lens, P = inputs(case)
    sd, yd, ld, Pd = dev(s), dev(y), dev(lens), dev(P)
    seed, q0 = hash_key(case)
    a = F.irfgan_point_sample(sd, Pd, S, seed=seed, q0=q0, lens=ld)
    b = F.irfgan_point_sample(sd, Pd, S, seed=seed, q0=q0, lens=ld)
    u = F.irfgan_point_sample(sd, Pd, S, lens=ld, unif=F.irfgan_uniforms(B, L, seed=seed, q0=q0))
    sh = F.irfgan_point_sample(sd[3:], Pd[3:], S, seed=seed, q0=q0 + 3, lens=ld[3:])
    for x, v, z, w in zip(a, b, u, sh):
        assert torch.equal(x, v) and torch.equal(x, z) and torch.equal(x[3:], w)
    kw = dict(lens=ld, return_count=True)
    ud, ub = F.irfgan_uniforms(B, L, S, seed=seed, q0=q0)
    assert ud.shape == (B, 2, S) and ub.shape == (B, L, L)
    a = F.irfgan_pair_sample(sd, yd, Pd, S, seed=seed, q0=q0, **kw)
    b = F.irfgan_pair_sample(sd, yd, Pd, S, seed=seed, q0=q0, **kw)
    u = F.irfgan_pair_sample(sd, yd, Pd, S, unif_draw=ud, unif_bern=ub, **kw)
    sh = F.irfgan_pair_sample(sd[3:], yd[3:], Pd[3:], S, seed=seed, q0=q0 + 3, lens=ld[3:], return_count=True)
    one = F.irfgan_pair_sample(sd[:1], yd[:1], Pd[:1], S, seed=seed, q0=q0, lens=ld[:1], return_count=True)
    for x, v, z, w, o in zip(a, b, u, sh, one):
        assert torch.equal(x, v) and torch.equal(x, z) and torch.equal(x[3:], w) and torch.equal(x[:1], o)
    th, tt, fh, ft, nsel, count = (t.cpu().numpy() for t in a)
    for q in range(B):
        n = int(lens[q])
        if nsel[q]:
            assert nsel[q] == S and 0 < count[q] <= n * n and (y[q, th[q]] > y[q, tt[q]]).all() and max(fh[q].max(), ft[q].max()) < n
        else:
            assert not (th[q].any() or tt[q].any() or fh[q].any() or ft[q].any())


@gpu
def test_both_forms_draw_the_same():
    """One list of 256 documents, padded to L = 256 (one wavefront per query) and to L = 257 (one workgroup): every draw and bern_count agree."""
    import ptranking_amd.functional as F
    case = next(c for c in CASES if c[1] == 256)
    assert launch_form("ptr_irfgan_pair_sample", 256)[0] == 64 and launch_form("ptr_irfgan_pair_sample", 257)[0] == 256
    s, y, lens, P = inputs(case)
    B, S = case[0], 64
    wide = lambda a: np.concatenate([a, np.zeros((B, 1), a.dtype)], axis=1)
    seed, q0 = hash_key(case)
    for x, z in zip(F.irfgan_point_sample(dev(s), dev(P), S, seed=seed, q0=q0, lens=dev(lens)),
                    F.irfgan_point_sample(dev(wide(s)), dev(P), S, seed=seed, q0=q0, lens=dev(lens))):
        assert torch.equal(x, z)
    a = F.irfgan_pair_sample(dev(s), dev(y), dev(P), S, seed=seed, q0=q0, lens=dev(lens), return_count=True)
    b = F.irfgan_pair_sample(dev(wide(s)), dev(wide(y)), dev(P), S, seed=seed, q0=q0, lens=dev(lens), return_count=True)
    assert int(a[4].max()) == S
    for x, z in zip(a, b):
        assert torch.equal(x, z)


def _chi_square(counts, p):
    keep = p > 0
    assert counts[~keep].sum() == 0
    e = counts.sum() * p[keep]
    return float(((counts[keep] - e) ** 2 / e).sum()), int(keep.sum()) - 1


@gpu
def test_sampler_frequencies_follow_the_laws():
    """24 000 rows of one list (a row's stream is keyed by its query index) against the exact laws, chi-square at p = 1e-4."""
    import ptranking_amd.functional as F
    N = 24000
    s7 = np.array([0.8, -0.3, 0.1, 1.2, -1.0, 0.4, -0.1], np.float32)
    ones = lambda v: torch.full((N,), v, dtype=torch.int32, device="cuda")
    pos, neg, nsel = F.irfgan_point_sample(dev(np.tile(s7, (N, 1))), ones(2), 2, seed=4321)
    assert int(nsel.min()) == 2
    for k in (0, 1):                                                          # the first and the second draw without replacement
        chi, dof = _chi_square(np.bincount(neg[:, k].cpu().numpy(), minlength=7).astype(np.float64), FR.point_fake_law(s7, k + 1))
        print(f"MEASURED chi-square point fakes, draw {k}: {chi:.2f} at {dof} degrees of freedom")
        assert chi < CHI2_1E4[dof]
    y5, s5 = np.array([2, 1, 1, 0, 0], np.float32), np.array([0.3, -0.2, 0.9, 0.0, -0.6], np.float32)
    th, tt, *_ = F.irfgan_pair_sample(dev(np.tile(s5, (N, 1))), dev(np.tile(y5, (N, 1))), ones(3), 1, seed=99)
    w = FR.pair_weights(y5, 3).reshape(-1)
    chi, dof = _chi_square(np.bincount((th[:, 0] * 5 + tt[:, 0]).cpu().numpy(), minlength=15).astype(np.float64), w / w.sum())
    print(f"MEASURED chi-square true pairs: {chi:.2f} at {dof} degrees of freedom")
    assert chi < CHI2_1E4[dof]
    y3, s3 = np.array([1, 0, 0], np.float32), np.array([0.5, -0.4, 0.1], np.float32)
    *_, fh, ft, nsel, count = F.irfgan_pair_sample(dev(np.tile(s3, (N, 1))), dev(np.tile(y3, (N, 1))), ones(1), 1, seed=7, return_count=True)
    law, alive = FR.fake_pair_law(s3)
    ok = (nsel > 0).cpu().numpy()
    assert abs(ok.mean() - alive) <= 4.0 * np.sqrt(alive * (1 - alive) / N) + 1.0 / N
    chi, dof = _chi_square(np.bincount((fh[:, 0] * 3 + ft[:, 0]).cpu().numpy()[ok], minlength=9).astype(np.float64), law)
    print(f"MEASURED chi-square fake pairs: {chi:.2f} at {dof} degrees of freedom")
    assert chi < CHI2_1E4[dof]
    p = FR._sg(s3.astype(np.float64)[:, None] - s3[None, :])
    mean, se = float(count.double().mean()), float(np.sqrt((p * (1 - p)).sum() / N))
    print(f"MEASURED bern_count mean {mean:.4f} against {p.sum():.4f}, standard error {se:.4f}")
    assert abs(mean - p.sum()) <= 4.0 * se


# ------------------------------------------------------------------------------------------------------------- the loss maths
def _launch(x, nsel, mode, f_div, d_fake, idx_a, idx_b, lens):
    import ptranking_amd.functional as F
    xd = dev(x).requires_grad_(True)
    gen = mode.endswith("_G")
    loss, parts = F.irfgan_loss(xd, dev(nsel), mode, f_div, d_fake=dev(d_fake), idx_a=dev(idx_a), idx_b=dev(idx_b), lens=dev(lens) if gen else None,
                                return_parts=True)
    loss.backward()
    return loss.detach().cpu().numpy().reshape(1), parts, xd.grad.cpu().numpy()


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_losses_of_every_divergence(case, mode):
    lens = inputs(case)[2]
    x, nsel, d_fake, idx_a, idx_b = loss_case(case, mode)
    for f_div in DIVS:
        loss, parts, grad = _launch(x, nsel, mode, f_div, d_fake, idx_a, idx_b, lens)
        ref = _loss_ref(case, mode, f_div)
        what = f"irfgan {mode} {f_div} {case}"
        assert np.array_equal(parts["valid_q"].cpu().numpy(), ref["valid_q"]), what
        gate(parts["loss_q"].cpu().numpy(), ref["loss_q"], torch.from_numpy(ref["E_loss_q"]), what + " loss_q", c=FR.C_IRFGAN)
        gate(grad, ref["grad"], torch.from_numpy(ref["E_grad"]), what + " grad", c=FR.C_IRFGAN)
        gate(loss, np.array([ref["loss"]]), torch.tensor([ref["E_loss"]], dtype=torch.float64), what + " loss_out", c=FR.C_IRFGAN)
        if mode.endswith("_G"):
            assert (grad[np.arange(case[1])[None, :] >= lens[:, None]] == 0).all()


def golden_cases(kind, family):
    """[(fields of one case, its slice of the gradient rows, its column of the loss rows)] of tests/golden/irfgan.npz."""
    c = _load("irfgan.npz")[kind][family]
    per_v = {"point_d": ("x_true", "x_fake"), "pair_d": ("th", "tt", "fh", "ft"), "point_g": ("idx", "d_fake"), "pair_g": ("head", "tail", "d_head", "d_tail")}[kind]
    out, at_v, at_n, at_g = [], 0, 0, 0
    for i, row in enumerate(c["shape"]):
        n, V = (int(row[0]), int(row[1])) if row.size == 2 else (0, int(row[0]))
        fields = {k: c[k][at_v:at_v + V] for k in per_v}
        width = n if n else len(per_v) * V
        if n:
            fields["g_preds"] = c["g_preds"][at_n:at_n + n]
        out.append((fields, slice(at_g, at_g + width), i, n, V))
        at_v, at_n, at_g = at_v + V, at_n + n, at_g + width
    return c, out


def golden_call(kind, fields, n, V):
    """(x, nsel, mode, d_fake, idx_a, idx_b) of one golden case as a batch of one query."""
    nsel = np.array([V], np.int32)
    if kind == "point_d":
        return np.concatenate([fields["x_true"], fields["x_fake"]])[None], nsel, "POINT_D", None, None, None
    if kind == "pair_d":
        return np.concatenate([fields[k] for k in ("th", "tt", "fh", "ft")])[None], nsel, "PAIR_D", None, None, None
    if kind == "point_g":
        return fields["g_preds"][None], nsel, "POINT_G", fields["d_fake"][None], fields["idx"][None], None
    return fields["g_preds"][None], nsel, "PAIR_G", np.concatenate([fields["d_head"], fields["d_tail"]])[None], fields["head"][None], fields["tail"][None]


@gpu
@pytest.mark.parametrize("kind", ("point_d", "pair_d", "point_g", "pair_g"))
def test_golden_cases_of_the_reference(kind):
    """Moderate family: the kernel against the reference's own float64 run under the project's 1e-5 max-norm plus element-wise gate.  Steep
    family: wherever the reference's float64 is finite the kernel stays within the float64 bound of the closed form — also where the
    reference's fp32 run is inf or NaN, which it is for SH, JS and GAN (asserted from the fixture)."""
    c, cases = golden_cases(kind, "moderate")
    for fields, cols, i, n, V in cases:
        x, nsel, mode, d_fake, idx_a, idx_b = golden_call(kind, fields, n, V)
        for fi, f_div in enumerate(DIVS):
            loss, parts, grad = _launch(x, nsel, mode, f_div, d_fake, idx_a, idx_b, None)
            assert_close(loss, c["loss64"][fi, i:i + 1], f"{kind} moderate {f_div} n{n} V{V} loss")
            assert_close(grad[0], c["grad64"][fi, cols], f"{kind} moderate {f_div} n{n} V{V} grad")
    c, cases = golden_cases(kind, "steep")
    broken, worst = set(), 0.0
    for fields, cols, i, n, V in cases:
        x, nsel, mode, d_fake, idx_a, idx_b = golden_call(kind, fields, n, V)
        for fi, f_div in enumerate(DIVS):
            if not (np.isfinite(c["loss32"][fi, i]) and np.isfinite(c["grad32"][fi, cols]).all()):
                broken.add(f_div)
            if not (np.isfinite(c["loss64"][fi, i]) and np.isfinite(c["grad64"][fi, cols]).all()):
                continue
            loss, parts, grad = _launch(x, nsel, mode, f_div, d_fake, idx_a, idx_b, None)
            ref = FR.loss(x, nsel, mode, f_div, d_fake=d_fake, idx_a=idx_a, idx_b=idx_b)
            what = f"{kind} steep {f_div} n{n} V{V}"
            worst = max(worst, gate(loss, np.array([ref["loss"]]), torch.tensor([ref["E_loss"]], dtype=torch.float64), what + " loss", c=FR.C_IRFGAN),
                        gate(grad, ref["grad"], torch.from_numpy(ref["E_grad"]), what + " grad", c=FR.C_IRFGAN))
    print(f"MEASURED {kind} steep: the reference's fp32 run is not finite under {sorted(broken)}; kernel worst err/E {worst:.3f}")
    assert {"SH", "JS", "GAN"} <= broken


# ------------------------------------------------------------------------------------------------------------- the machines
def _example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_irfgan_synthetic as ex
    return ex


@gpu
@pytest.mark.parametrize("name", ("IRFGAN_Point", "IRFGAN_Pair"))
def test_a_batch_of_one_query_is_the_references_step(name, monkeypatch):
    """One query, one pass: the documents of the compact batch are the sampled ones, the discriminator steps on mean c(fake) - mean a(true)
    of its train-mode scores, d_fake are its eval-mode scores of the fakes AFTER that step, and the generator steps on the reference's
    one-query loss of its own train-mode scores — each loss against the float64 restatement, to the gate."""
    import ptranking_amd as pa
    import ptranking_amd.adversarial as adv
    ex = _example()
    data = pa.PaddedQueryBatches(ex.synthetic_queries(1, 8, seed=5, min_docs=23, max_docs=23), "cuda:0", presort=True)
    machine = ex.build_machine(name, 8, "cuda:0", f_div="GAN")
    buf = {}
    machine.fill_global_buffer(data, dict_buffer=buf)
    calls, samples, real = [], [], adv.F_.irfgan_loss

    def spy(x, nsel, mode, f_div, **kw):
        out = real(x, nsel, mode, f_div, **kw)
        calls.append((mode, f_div, x.detach().cpu().numpy(), nsel.cpu().numpy(), {k: None if v is None else v.cpu().numpy() for k, v in kw.items()}, float(out)))
        return out

    sample = machine._sample
    monkeypatch.setattr(adv.F_, "irfgan_loss", spy)
    monkeypatch.setattr(machine, "_sample", lambda *a: samples.append(sample(*a)) or samples[-1])
    g, d = machine.get_generator(), machine.get_discriminator()
    before = [[p.detach().clone() for p in pl.get_parameters()] for pl in (g, d)]
    assert machine.mini_max_train(train_data=data, generator=g, discriminator=d, global_buffer=buf) is False
    for pl, old in zip((g, d), before):                                       # both players stepped
        assert any(not torch.equal(a, p.detach()) for a, p in zip(old, pl.get_parameters()))
    (ids, X, Y, lens), = list(data)
    idx, idx_a, idx_b, nsel = samples[0]
    V, S = int(nsel[0]), idx_a.size(1)
    assert V == S == 5 and [c[0] for c in calls] == [machine.d_mode, machine.g_mode] and {c[1] for c in calls} == {"GAN"}
    d.eval_mode()
    with torch.no_grad():
        fakes = [i[:, :V] for i in idx[len(idx) // 2:]]
        want = torch.cat([d.score(X.gather(1, i[:, :, None].expand(-1, -1, X.size(2))), torch.full((1,), V, dtype=torch.int32, device="cuda")) for i in fakes], dim=1)
    kw = calls[1][4]
    assert np.allclose(kw["d_fake"][:, :want.size(1)], want.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert np.array_equal(kw["idx_a"], idx_a.cpu().numpy()) and (idx_b is None or np.array_equal(kw["idx_b"], idx_b.cpu().numpy()))
    for mode, f_div, x, ns, kw, got in calls:
        ref = FR.loss(x, ns, mode, f_div, d_fake=kw.get("d_fake"), idx_a=kw.get("idx_a"), idx_b=kw.get("idx_b"), lens=kw.get("lens"))
        gate(np.array([got]), np.array([ref["loss"]]), torch.tensor([ref["E_loss"]], dtype=torch.float64), f"{name} {mode} step loss", c=FR.C_IRFGAN)


@gpu
@pytest.mark.parametrize("f_div", ("KL", "GAN"))
@pytest.mark.parametrize("name", ("IRFGAN_Point", "IRFGAN_Pair"))
def test_machines_train_on_a_planted_signal(name, f_div):
    """20 mini-max rounds on 64 synthetic queries: both players' nDCG@5 stay finite and the discriminator ends above where it started."""
    import ptranking_amd as pa
    ex = _example()
    data = pa.PaddedQueryBatches(ex.synthetic_queries(64, 16, seed=3), "cuda:0", rough_batch_size=256, presort=True)
    machine = ex.build_machine(name, 16, "cuda:0", f_div=f_div)
    hist = np.array(ex.run(machine, data, 20, log=lambda *_: None))
    print(f"MEASURED {name} {f_div}: G nDCG@5 {hist[0, 0]:.4f} -> {hist[-1, 0]:.4f}, D nDCG@5 {hist[0, 1]:.4f} -> {hist[-1, 1]:.4f}")
    assert hist.shape == (21, 2) and np.isfinite(hist).all()
    assert hist[-1, 1] > hist[0, 1]


@gpu
def test_the_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_irfgan_synthetic.py"), "--queries", "48", "--epochs", "2", "--f-div", "JS"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if " epoch " in l]
    assert len(lines) == 6 and all("G nDCG@5" in l and "D nDCG@5" in l for l in lines), out.stdout
