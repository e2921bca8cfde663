"""CPU: the error model of tests/diversity_bounds.py without a GPU —

  * the two needs that set C_DIV are re-measured: (a) tests/diversity_ref.py evaluated in fp32 torch on every case the GPU tests run,
    (b) the reference's own fp32 loss32 / grad32 of tests/golden/diversity.npz; and the misfit of (b) without the subtraction's term;
  * the restated gradient is the derivative of the restated loss, and the restatement reproduces the reference's float64 results for
    non-finite scores (tests/golden/diversity_edge.npz);
  * planted faults, in an emulation of the kernel's two passes and of its metric walk written here, fail the gate; for each it is
    stated (and for those the old rule cannot see: asserted) whether golden_util.assert_close lets it through;
  * the case lists reach every (G, TP) of the loss kernel and every (G, DPT) of the metric kernel at its smallest and largest length.
"""
import math

import numpy as np
import pytest

import diversity_bounds as DB
import diversity_ref as DR
import golden_util as GU
from launch_form import group_form

C = DB.C_DIV


def ratio(got, ref, E):
    """Worst |got - ref| / E; an element with E = 0 must be equal."""
    got, ref, E = (np.asarray(a, np.float64) for a in (got, ref, E))
    err = np.abs(got - ref)
    assert np.all((E > 0) | (err == 0)), "an exact element differs"
    m = E > 0
    return float((err[m] / E[m]).max()) if m.any() else 0.0


def old_rule_passes(got, ref):
    try:
        GU.assert_close(got, ref, "old rule")
        return True
    except AssertionError:
        return False


# ---------------------------------------------------------------------------------------------------------------- 1. the constant
@pytest.fixture(scope="module")
def needs():
    a_loss, a_met, b, b_loss, misfit = (0.0, ""), (0.0, ""), (0.0, ""), (0.0, ""), (0.0, "")
    for cs in DB.loss_cases():
        ref = DB.loss_case_ref(cs, c=1.0)
        lq, g = DR.alphadcg_batch(cs["preds"], cs["rele"], cs["rt"], cs["alpha"], cs["top_k"], cs["axis"], cs["lens"], cs["ntopics"],
                                  dtype=np.float32, kernel_consts=True)
        a_loss = max(a_loss, (max(ratio(lq, ref["loss_q"], ref["E_loss_q"]), ratio(g, ref["grad"], ref["E_grad"])), cs["name"]))
    for cs in DB.metric_cases() + DB.nan_metric_cases():
        ref = DB.metric_case_ref(cs, c=1.0)
        a, e, ne, v = DR.div_metrics_batch(cs["preds"], cs["rele"], cs["ks"], cs["alpha"], cs["max_label"], cs["lens"], cs["ntopics"],
                                           dtype=np.float32, kernel_consts=True)
        assert np.array_equal(v, ref["valid"])
        w = ratio(a, ref["andcg"], ref["E_andcg"])
        if e is not None:
            w = max(w, ratio(e, ref["err_ia"], ref["E_err_ia"]), ratio(ne, ref["nerr_ia"], ref["E_nerr_ia"]))
        a_met = max(a_met, (w, cs["name"]))
    for name, c in sorted(GU._load("diversity.npz")["daletor"].items()):
        args = (c["preds"], c["rele"][None].astype(np.float32), None, None, float(c["rt"]), 0.5, int(c["top_k"]) or None, 0)
        ref = DB.alphadcg(*args, c=1.0, sub_abs=True)
        wl = ratio([float(c["loss32"])], ref["loss_q"], ref["E_loss_q"])
        b_loss = max(b_loss, (wl, name))
        b = max(b, (max(wl, ratio(c["grad32"], ref["grad"], ref["E_grad"])), name))
        strict = DB.alphadcg(*args, c=1.0)
        misfit = max(misfit, (ratio(c["grad32"], strict["grad"], strict["E_grad"]), name))
    return dict(a_loss=a_loss, a_met=a_met, b=b, b_loss=b_loss, misfit=misfit)


def test_measured_needs_give_the_constant(needs):
    """C_DIV = min(4, 2 x the larger of the two needs, rounded up to a half), and the needs recorded beside it are the measured ones."""
    for k, (w, name) in needs.items():
        print(f"MEASURED need {k} at c = 1: {w:.4g} ({name})")
    a = max(needs["a_loss"][0], needs["a_met"][0])
    assert abs(a - DB.NEED_FP32_TORCH) <= 0.05 and abs(needs["b"][0] - DB.NEED_REFERENCE_FP32) <= 0.05
    assert DB.C_DIV == DB.constant_from_needs(DB.NEED_FP32_TORCH, DB.NEED_REFERENCE_FP32) == DB.constant_from_needs(a, needs["b"][0]) <= DB.C_CAP
    assert a <= DB.C_DIV and needs["b"][0] <= DB.C_DIV
    # without the term of its 1 - ind by subtraction the reference's own fp32 gradient is orders of magnitude outside the model
    assert 0.5 * DB.MISFIT_REFERENCE_FP32 <= needs["misfit"][0] <= 2.0 * DB.MISFIT_REFERENCE_FP32
    assert needs["b_loss"][0] <= 0.2


# ---------------------------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("alpha,top_k,axis,graded", [(0.5, None, 0, False), (0.9, 3, 0, True), (0.1, 4, 1, True), (0.5, 30, 1, False)])
def test_restated_gradient_is_the_derivative_of_the_restated_loss(alpha, top_k, axis, graded):
    g = np.random.default_rng(5)
    T, L = 6, 23
    s = (0.3 * g.standard_normal(L)).astype(np.float32).astype(np.float64)
    R = (g.random((T, L)) < 0.4) * (g.integers(1, 4, size=(T, L)) if graded else 1.0)
    _, grad = DR.alphadcg(s, R, 10.0, alpha, top_k, axis)
    eps = 1e-6
    for j in range(L):
        p, m = s.copy(), s.copy()
        p[j] += eps; m[j] -= eps
        num = (DR.alphadcg(p, R, 10.0, alpha, top_k, axis)[0] - DR.alphadcg(m, R, 10.0, alpha, top_k, axis)[0]) / (2 * eps)
        assert abs(num - grad[j]) <= 2e-7 * max(1.0, float(np.max(np.abs(grad)))), (j, num, grad[j])


@pytest.mark.parametrize("case", sorted(GU._load("diversity_edge.npz")["nonfinite"]))
def test_restatement_reproduces_the_reference_on_non_finite_scores(case):
    """One NaN, two +inf and one -inf score: the reference stays finite (a NaN difference is a tie), and so does the restatement."""
    c = GU._load("diversity_edge.npz")["nonfinite"][case]
    assert not np.isfinite(c["preds"]).all() and np.isfinite(c["grad64"]).all() and np.isfinite(c["grad32"]).all()
    with np.errstate(invalid="ignore"):
        loss, grad = DR.alphadcg(c["preds"][0], c["rele"].astype(np.float64), float(c["rt"]), 0.5, int(c["top_k"]) or None, 0)
    assert abs(loss - float(c["loss64"])) <= 1e-12 * max(1.0, abs(float(c["loss64"])))
    assert np.max(np.abs(grad - c["grad64"][0])) <= 1e-12 * max(1.0, float(np.max(np.abs(c["grad64"]))))
    ref = DB.alphadcg(c["preds"], c["rele"][None].astype(np.float32), rt=float(c["rt"]), top_k=int(c["top_k"]) or None)
    assert np.isfinite(ref["E_grad"]).all() and np.isfinite(ref["E_loss_q"]).all()
    DB.gate_losses(np.array([float(c["loss64"])]), c["grad64"], ref, f"{case}: the fixture's float64", C)


def test_exact_results_carry_no_tolerance():
    cs = DB.loss_case("exact", 5, 30, 9, rele="graded", top_k=3, axis=0, pick=0, seed=1)
    cs["rele"][1, 3:, :] = 2.0
    cs["rele"][1, :3, :] = 0.0                                   # kept relevance all zero, the dropped rows are not
    cs["lens"][1], cs["ntopics"][1] = 30, 5
    cs["rele"][list(cs["lens"]).index(1), 0, 0] = 1.0            # the 1-document query is relevant: a loss, and no gradient
    ref = DB.loss_case_ref(cs)
    lens = [DR.clamp_len(cs["lens"], q, 30) for q in range(9)]
    nts = [DR.clamp_len(cs["ntopics"], q, 5) for q in range(9)]
    assert 0 in lens and 1 in lens and 0 in nts and min(cs["lens"]) < 0 and max(cs["lens"]) > 30 and max(cs["ntopics"]) > 5
    for q in range(9):
        assert not ref["E_grad"][q, lens[q]:].any() and not ref["grad"][q, lens[q]:].any()
        if lens[q] == 0 or nts[q] == 0 or q in (1, 8):
            assert ref["loss_q"][q] == 0 and ref["E_loss_q"][q] == 0 and not ref["grad"][q].any() and not ref["E_grad"][q].any(), q
        elif lens[q] == 1:
            assert ref["E_grad"][q, 0] == 0 and ref["grad"][q, 0] == 0 and ref["E_loss_q"][q] > 0
        else:
            assert (ref["E_grad"][q, :lens[q]] > 0).all() and ref["E_loss_q"][q] > 0


# ---------------------------------------------------------------------------------------------------------------- 3. planted faults: loss
def emulate(s, R, rt, alpha, top_k, axis, dtype, fault=None, at=None):
    """The two passes of alphadcg_kernel for one query in numpy arithmetic of `dtype`, with one planted fault."""
    f = np.dtype(dtype).type
    s, Rt = np.asarray(s).astype(dtype), np.ascontiguousarray(np.asarray(R).T).astype(dtype)
    n, T = Rt.shape
    _, log2_c, ln_c = DR.c_logs(alpha, True)
    rt = f(np.float32(rt))
    x = rt * s[None, :] - rt * s[:, None] if fault == "scaled_x" else rt * (s[None, :] - s[:, None])
    e = np.exp(-np.abs(x))
    r = f(1) / (f(1) + e)
    sm = e * r
    off = ~np.eye(n, dtype=bool)
    ind = np.where(x > 0, r, np.where(x < 0, sm, f(0.5))) * off
    inv = np.where(x > 0, sm, np.where(x < 0, r, f(0.5))) * off
    pi = f(1) + ind.sum(1, dtype=dtype)
    cover = ind @ Rt
    if fault == "self_term":                                     # the reference's form keeps the j = i indicator: 0.5 R - R / 2, here without the second
        cover[at] += f(0.5) * Rt[at]
    lg = np.log2(f(1) + pi)
    Rk = Rt * DR.keep_mask(T, n, top_k, axis).T.astype(dtype)
    g = Rk * np.exp2(cover * f(log2_c)) / lg[:, None]
    if fault == "ln_c_twice":
        ln_c = float(np.float32(0.6931471805599453) * np.float32(log2_c))
    A = g.sum(1, dtype=dtype) / (lg * f(math.log(2.0)) * (f(1) + pi))
    Bc = -g * f(ln_c)
    d = ind * (f(1) - ind) * off if fault == "d_sub" else ind * inv
    D = (A[None, :] - A[:, None]) + Rt @ Bc.T - Bc @ Rt.T
    return float(-g.sum(dtype=dtype)), (rt * (d * D).sum(1, dtype=dtype)).astype(np.float64)


def _one_query(T, L, family, alpha, rele, seed, top_k=None):
    cs = DB.loss_case("fault", T, L, 1, family=family, alpha=alpha, rele=rele, top_k=top_k, seed=seed)
    return cs, DB.loss_case_ref(cs)


def _gate_one(loss, grad, ref, what):
    return DB.gate_losses(np.array([loss]), grad[None], ref, what, C)


def test_the_unfaulted_emulation_passes_the_gate():
    for fam, rt_alpha in (("normal", 0.5), ("steep", 0.5), ("offset+", 0.9)):
        cs, ref = _one_query(7, 100, fam, rt_alpha, "graded", 3)
        for dt in (np.float64, np.float32):
            _gate_one(*emulate(cs["preds"][0], cs["rele"][0], cs["rt"], cs["alpha"], None, 0, dt), ref, f"emulation {fam} {np.dtype(dt).name}")


def test_fault_small_gradient_element_off_by_one_percent():
    """* One element of magnitude <= 1e-4 of the row's largest, 1 % off: the old rule's floor hides it."""
    cs, ref = _one_query(7, 100, "normal", 0.5, "graded", 3)
    loss, grad = emulate(cs["preds"][0], cs["rele"][0], cs["rt"], cs["alpha"], None, 0, np.float64)
    small = np.nonzero((np.abs(grad) <= 1e-4 * np.abs(grad).max()) & (np.abs(grad) > 1e-9 * np.abs(grad).max()))[0]
    assert small.size, "no small gradient element in this list"
    bad = grad.copy()
    bad[small[0]] *= 1.01
    assert old_rule_passes(bad[None], ref["grad"])
    with pytest.raises(AssertionError, match="grad"):
        _gate_one(loss, bad, ref, "planted small element")


def test_fault_d_by_subtraction_in_the_saturated_tail():
    """* d = ya (1 - ya) by subtraction, fp32, rt = 100: where ya rounds to 1 the pair's d is 0 instead of e^-|x|.  The old rule passes."""
    cs, ref = _one_query(7, 100, "steep", 0.5, "graded", 3)
    loss, grad = emulate(cs["preds"][0], cs["rele"][0], cs["rt"], cs["alpha"], None, 0, np.float32, "d_sub")
    assert old_rule_passes(grad[None], ref["grad"])
    with pytest.raises(AssertionError, match="grad"):
        _gate_one(loss, grad, ref, "planted d by subtraction")


def test_fault_ln_c_rounded_twice_is_no_fault_in_fp32():
    """* ln c = ln2 fp32(log2 c).  The issue behind this gate expected it to fail at alpha = 0.9.  It cannot: the fp32 product
    0.6931472f * fp32(log2 c) IS fp32(ln c) at alpha = 0.1, 0.5 and 0.9 (bit for bit: asserted), and over 999 values of alpha it is never
    more than 1 ulp away — 2 u relative on Bc, inside c u |Bc| for every c >= 2.  A gate that refused it would refuse the kernel's own
    constant.  Both rules pass it, at the worst alpha found as well."""
    worst, worst_alpha = 0.0, None
    for a in np.linspace(0.001, 0.999, 999):
        _, l2, ln = DR.c_logs(float(a), True)
        twice = float(np.float32(0.6931471805599453) * np.float32(l2))
        if a in (0.1, 0.5, 0.9) or abs(twice - ln) / abs(ln) > worst:
            worst, worst_alpha = max(worst, abs(twice - ln) / abs(ln)), (float(a) if abs(twice - ln) / abs(ln) >= worst else worst_alpha)
    for a in (0.1, 0.5, 0.9):
        _, l2, ln = DR.c_logs(a, True)
        assert float(np.float32(0.6931471805599453) * np.float32(l2)) == ln
    print(f"MEASURED ln c rounded twice: at most {worst / 2.0 ** -24:.2f} u from fp32(ln c) (alpha = {worst_alpha})")
    assert worst <= 2.0 * 2.0 ** -24
    for a in (0.9, worst_alpha):
        cs, ref = _one_query(7, 100, "normal", a, "graded", 3)
        loss, grad = emulate(cs["preds"][0], cs["rele"][0], cs["rt"], cs["alpha"], None, 0, np.float64, "ln_c_twice")
        assert old_rule_passes(grad[None], ref["grad"])
        _gate_one(loss, grad, ref, f"ln c rounded twice, alpha {a}")


def test_fault_dropped_self_term():
    """The - R / 2 self term of one subtopic dropped for one document (cover too large by R / 2: its gain off by a factor sqrt(c)).
    The old rule sees this one as well."""
    cs, ref = _one_query(7, 100, "normal", 0.5, "graded", 3)
    R = cs["rele"][0]
    i, t = [(i, t) for i in range(100) for t in range(7) if R[t, i] > 0][0]
    loss, grad = emulate(cs["preds"][0], R, cs["rt"], cs["alpha"], None, 0, np.float64, "self_term", at=(i, t))
    print(f"old rule passes the dropped self term: loss {old_rule_passes([loss], ref['loss_q'])}, grad {old_rule_passes(grad[None], ref['grad'])}")
    with pytest.raises(AssertionError):
        _gate_one(loss, grad, ref, "planted dropped self term")


def test_fault_scores_scaled_before_the_difference():
    """x = rt s_j - rt s_i under an offset of 1e3 rounds relative to rt |s|, not to |ds|."""
    cs, ref = _one_query(7, 100, "offset+", 0.5, "graded", 3)
    loss, grad = emulate(cs["preds"][0], cs["rele"][0], cs["rt"], cs["alpha"], None, 0, np.float32, "scaled_x")
    print(f"old rule passes the scaled difference: loss {old_rule_passes([loss], ref['loss_q'])}, grad {old_rule_passes(grad[None], ref['grad'])}")
    with pytest.raises(AssertionError):
        _gate_one(loss, grad, ref, "planted scaled difference")
    _gate_one(*emulate(cs["preds"][0], cs["rele"][0], cs["rt"], cs["alpha"], None, 0, np.float32), ref, "the same list, unfaulted fp32")


def test_fault_one_loss_of_64_off_by_1e_5():
    """* One query's loss out of 64 wrong by 1e-5 relative: exactly what the old rule lets through, per query and in the total."""
    cs = DB.loss_case("batch64", 5, 30, 64, rele="binary30", top_k=None, seed=9, full=True)
    ref = DB.loss_case_ref(cs)
    lq, g = DR.alphadcg_batch(cs["preds"], cs["rele"], cs["rt"], cs["alpha"], None, 0, cs["lens"], cs["ntopics"], kernel_consts=True)
    total = DB.batch_total(ref, C)
    DB.gate_losses(lq, g, ref, "64 queries", C, got_total=lq.sum(), total=total)
    bad = lq.copy()
    bad[17] *= 1.0 + 1e-5
    assert old_rule_passes(bad, ref["loss_q"]) and old_rule_passes(bad.sum(), ref["loss_q"].sum())
    with pytest.raises(AssertionError, match="loss_q"):
        DB.gate_losses(bad, g, ref, "planted loss_q", C)


# ---------------------------------------------------------------------------------------------------------------- 4. planted faults: metrics
def metric_walk(R, order, ks, alpha, max_label, divide_by=None, den_fault=0.0):
    """div_metrics_kernel's walk for one query in float64 numpy with planted faults: ERR-IA divided by `divide_by`, the discount's log2 off
    by den_fault relative with the sign alternating from rank to rank."""
    T, n = R.shape
    _, log2_c, _ = DR.c_logs(alpha, True)
    kmax = min(max(ks), n)
    r = np.arange(kmax, dtype=np.float64)
    den = np.log2(r + 2.0) * (1.0 + den_fault * (-1.0) ** r)

    def lanes(Rk):
        cov = np.cumsum(Rk, 1) - Rk
        dcg = np.cumsum(np.exp2(cov * log2_c) * Rk / den, 1).sum(0)
        sat = (np.exp2(Rk) - 1.0) * 2.0 ** -max_label
        casc = np.concatenate([np.ones((T, 1)), np.cumprod(1.0 - sat, 1)[:, :-1]], 1)
        return dcg, np.cumsum(sat * casc / (r + 1.0), 1).sum(0) / (divide_by or T)
    (ds, es), (di, ei) = lanes(R[:, order][:, :kmax]), lanes(R[:, :kmax])
    out = np.zeros((3, len(ks)))
    for c, k in enumerate(ks):
        if 1 <= k <= n:
            out[:, c] = (ds[k - 1] / di[k - 1] if di[k - 1] > 0 else 0.0, es[k - 1], es[k - 1] / ei[k - 1] if ei[k - 1] > 0 else 0.0)
    return out


def _metric_fault_case(second=False):
    """Query 0: 32 subtopic rows of which 31 count, 256 documents, the only relevant one (document 0, subtopic 0) ranked last — or second;
    query 1: a random one with all 32 subtopics, for company."""
    g = np.random.default_rng(2)
    T, L = 32, 256
    s = g.permutation(2 * L).reshape(2, L).astype(np.float32)
    R = np.zeros((2, T, L), np.float32)
    R[0, 0, 0] = 1.0
    s[0, 0] = np.sort(s[0, 1:])[-1] - 0.5 if second else -1.0
    R[1] = (g.random((T, L)) < 0.05) * g.integers(1, 4, size=(T, L))
    R[0, 31, :] = np.nan                                        # the padded subtopic row
    return dict(preds=s, rele=R, lens=np.array([L, L], np.int32), ntopics=np.array([31, 32], np.int32), ks=[1, 2, 3, 10, L], alpha=0.5,
                max_label=3.0)


def _walk_case(cs, **fault):
    out = np.zeros((3, 2, len(cs["ks"])))
    for q in range(2):
        R = cs["rele"][q, :cs["ntopics"][q]].astype(np.float64)
        out[:, q] = metric_walk(R, DR.sort_desc_order(cs["preds"][q]), cs["ks"], cs["alpha"], cs["max_label"], **fault)
    return out[0], out[1], out[2], np.array([1, 1])


def test_the_unfaulted_walk_passes_the_metric_gate():
    for second in (False, True):
        cs = _metric_fault_case(second)
        DB.gate_metrics(_walk_case(cs), DB.metric_case_ref(cs), "float64 walk", C)


def test_fault_err_ia_divided_by_the_padded_subtopic_count():
    """* ERR-IA / T instead of / ntopics with one padded subtopic row of 32: 3 % — of a value of 1.6e-5, below the old rule's floor."""
    cs = _metric_fault_case()
    ref = DB.metric_case_ref(cs)
    a, e, ne, v = _walk_case(cs, divide_by=32)
    assert old_rule_passes(e, ref["err_ia"]) and abs(e[0, 4] / ref["err_ia"][0, 4] - 31.0 / 32.0) < 1e-9 and np.array_equal(e[1], _walk_case(cs)[1][1])
    with pytest.raises(AssertionError, match="err_ia"):
        DB.gate_metrics((a, e, ne, v), ref, "planted ERR-IA / T", C)


def test_fault_low_precision_discount():
    """* 1 / log2(r + 2) from a log2 that is 1e-6 relative off, the sign alternating with the rank: 2e-6 of alpha-nDCG@2 where the system
    ranks second what the ideal ranks first.  The old rule passes."""
    cs = _metric_fault_case(second=True)
    ref = DB.metric_case_ref(cs)
    a, e, ne, v = _walk_case(cs, den_fault=1e-6)
    assert old_rule_passes(a, ref["andcg"])
    with pytest.raises(AssertionError, match="andcg"):
        DB.gate_metrics((a, e, ne, v), ref, "planted discount", C)


def parent_nan_order(s):
    """The ranking of div_metrics_kernel before its NaN fix: float compares give a NaN score rank 0 beside the true maximum, every other
    document its rank among the non-NaN scores; two documents scatter into order[0] and order[n - 1] keeps its initial 0."""
    s = np.asarray(s, np.float64)
    n = s.size
    with np.errstate(invalid="ignore"):
        gt = (s[None, :] > s[:, None]).sum(1)
        eq_before = np.array([(s[:i] == s[i]).sum() for i in range(n)])
    order = np.zeros(n, np.int64)
    for i in range(n):
        if gt[i] + eq_before[i] < n:
            order[gt[i] + eq_before[i]] = i
    return order


def test_fault_nan_ranking_of_the_parent_commit():
    """A NaN score ranked 'rank 0, last slot = document 0' moves every metric; the restatement ranks NaN first, as torch.sort does."""
    import torch
    cs = DB.nan_metric_cases()[1]
    ref = DB.metric_case_ref(cs)
    B, nk = cs["preds"].shape[0], len(cs["ks"])
    got = [np.zeros((B, nk)) for _ in range(3)]
    moved = 0
    for q in range(B):
        n, nt = DR.clamp_len(cs["lens"], q, cs["preds"].shape[1]), DR.clamp_len(cs["ntopics"], q, cs["rele"].shape[1])
        if n == 0 or nt == 0:
            continue
        s = cs["preds"][q, :n]
        assert np.array_equal(DR.sort_desc_order(s), torch.sort(torch.from_numpy(s.copy()), descending=True, stable=True)[1].numpy())
        order = parent_nan_order(s)
        moved += int(not np.array_equal(order, DR.sort_desc_order(s)))
        a, e, ne, _ = DR.div_metrics(s, cs["rele"][q, :nt, :n], cs["ks"], cs["alpha"], cs["max_label"], kernel_consts=True, order=order)
        got[0][q], got[1][q], got[2][q] = a, e, ne
    assert moved >= 5                                            # the rows with a NaN, and only they
    with pytest.raises(AssertionError):
        DB.gate_metrics((got[0], got[1], got[2], ref["valid"]), ref, "planted parent NaN order", C)


# ---------------------------------------------------------------------------------------------------------------- 5. coverage of the case lists
def loss_form(T, L):
    return group_form("ptr_alphadcg_fwd_bwd", T, L)


def metric_form(L):
    return group_form("ptr_div_metrics_at_ks", L)


def test_the_library_serves_the_forms_the_case_lists_name():
    assert [loss_form(T, 40)[1] for T in (1, 4, 5, 8, 9, 16, 17, 32)] == [4, 4, 8, 8, 16, 16, 32, 32]
    for form, (lo, hi) in DB.METRIC_FORM_L.items():
        assert metric_form(lo) == metric_form(hi) == form and (lo == 1 or metric_form(lo - 1) != form)
        assert hi == 4096 or metric_form(hi + 1) != form


def test_coverage_of_the_case_lists():
    loss = DB.loss_cases()
    forms = {loss_form(c["rele"].shape[1], c["rele"].shape[2]) for c in loss}
    assert forms == {(G, TP) for G in (64, 256) for TP in (4, 8, 16, 32)}
    for (T, L), form in {**DB.LOSS_FORMS, **DB.LOSS_LIMIT_FORMS}.items():
        assert loss_form(T, L) == form and any(c["rele"].shape[1:] == (T, L) for c in loss)
    small = [c for c in loss if c["rele"].shape[2] <= 128 and c["name"].startswith("form_")]
    assert {c["preds"].shape[0] for c in small} == {1, 4, 5, 9}
    lens = {int(v) - c["preds"].shape[1] if v > 2 else int(v) for c in loss for v in c["lens"]}
    assert {0, 1, 2, -3, 7} <= lens                              # 0, 1, 2 documents, the clamped -3 and L + 7 (stored as L + 7 - L)
    nts = {(int(v), c["rele"].shape[1]) for c in loss for v in c["ntopics"]}
    assert any(v == 0 for v, T in nts) and any(v == 1 and T > 1 for v, T in nts) and any(v == T + 2 for v, T in nts)
    assert {c["alpha"] for c in loss} == {0.1, 0.5, 0.9} and {c["rt"] for c in loss} == {10.0, 100.0}
    assert {c["axis"] for c in loss} == {0, 1}
    assert {c["top_k"] for c in loss if c["name"].startswith("topk")} == {None, 1, 6, 7, 8, 24, 29}
    assert all(not c["rele"][-1][np.isfinite(c["rele"][-1])].any() for c in loss if c["preds"].shape[0] >= 2)     # the all-zero query
    deep = [c for c in loss if c["name"].startswith("deep")]
    assert deep and all(c["alpha"] == 0.9 and ((c["rele"][0] > 0).sum(1) >= 40).all() for c in deep)
    met = DB.metric_cases()
    seen = {(metric_form(c["preds"].shape[1]), c["preds"].shape[1]) for c in met}
    for form, (lo, hi) in DB.METRIC_FORM_L.items():
        assert (form, lo) in seen and (form, hi) in seen
    assert {c["rele"].shape[1] for c in met} == {1, 5, 32} and {c["max_label"] for c in met} == {1.0, 3.0, None}
    for c in met:
        ks = c["ks"]
        assert ks != sorted(ks) and len(set(ks)) < len(ks) and 0 in ks and c["preds"].shape[1] in ks and max(ks) > c["preds"].shape[1]
    assert {c["preds"].shape[1] for c in DB.nan_metric_cases()} >= {63, 64, 65}
    for c in DB.nan_metric_cases():
        nan_rows = [q for q in range(c["preds"].shape[0]) if np.isnan(c["preds"][q, :DR.clamp_len(c["lens"], q, c["preds"].shape[1])]).any()]
        assert len(nan_rows) >= 5
        n12 = c["preds"].shape[1]
        assert np.isnan(c["preds"][12, :n12]).all() and np.isnan(c["preds"][9, n12 // 2]) and np.isnan(c["preds"][10, n12 - 1]) and np.isnan(c["preds"][0, 0])
