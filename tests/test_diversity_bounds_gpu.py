"""GPU: the diversification kernels (csrc/diversity.hip) against float64 with ELEMENT-WISE error bounds (tests/diversity_bounds.py, whose
header holds the model), on the case lists tests/test_diversity_bounds_cpu.py measured C_DIV on.

  ptr_alphadcg_fwd_bwd     loss_q, every gradient element and loss_out: all eight (G, TP) forms at their smallest shapes and the two
                           LDS-limit shapes, B in {1, 4, 5, 9} on the four-queries-per-workgroup forms, five score families (N(0, 1), a
                           common offset of +-1e3, ties, rt = 100, a spread that flushes e), alpha 0.1 / 0.5 / 0.9, binary and graded
                           relevance, cover counts that flush c^cover, lens / ntopics at 0, 1, 2, the clamped -3 / L + 7 / T + 2, a
                           query of all-zero relevance in every batch, NaN in every padded slot, top_k at and beyond T and L on both axes,
                           non-finite scores against the reference's own float64 (tests/golden/diversity_edge.npz); run twice and with
                           clean padding bit for bit, a query alone bit for bit
  ptr_div_metrics_at_ks    alpha-nDCG, ERR-IA, nERR-IA per (query, cut-off), `valid` exactly: every (G, DPT) at its smallest and largest
                           L, T in {1, 5, 32}, unsorted cut-offs with a duplicate, a 0, n and beyond, graded labels, ties, +-0.0, +-inf,
                           NaN scores (one, several, all; first, middle, last; 63 / 64 / 65 / 300 documents), the planted relevance
                           totals around the `valid` threshold, n in {0, 1}, ntopics = 0; through functional.div_metrics_at_ks and the C
                           ABI, run twice bit for bit; and the DALETOR evaluation methods on a batch whose predictions hold a NaN

Each gated call prints `MEASURED <what>: worst err/E (c C_DIV: needs c >= k)`; the last test prints the worst k per output.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import diversity_bounds as DB
import diversity_ref as DR
import golden_util as GU
from f64_bounds import U

pytestmark = pytest.mark.gpu
CD = DB.C_DIV
NEEDS = {}
LOSS = {c["name"]: c for c in DB.loss_cases()}
METRIC = {c["name"]: c for c in DB.metric_cases() + DB.nan_metric_cases()}
_REF = {}


def ref_of(cs):
    """One float64 reference per case, shared and left unchanged."""
    if cs["name"] not in _REF:
        _REF[cs["name"]] = DB.loss_case_ref(cs) if "rt" in cs else DB.metric_case_ref(cs)
    return _REF[cs["name"]]


def note(name, worst):
    NEEDS[name] = max(NEEDS.get(name, 0.0), worst * CD)


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def run_loss(preds, rele, rt=10.0, alpha=0.5, top_k=None, axis=0, lens=None, ntopics=None):
    """ptr_alphadcg_fwd_bwd through the ctypes binding -> (loss_out, loss_q [B], grad [B, L]) as numpy; the outputs start as NaN."""
    from ptranking_amd import _lib
    p, r = dev(preds), dev(rele)
    B, T, L = r.shape
    ld, td = dev(lens, torch.int32), dev(ntopics, torch.int32)
    loss, loss_q, grad = torch.full((1,), np.nan).cuda(), torch.full((B,), np.nan).cuda(), torch.full((B, L), np.nan).cuda()
    _lib.call("ptr_alphadcg_fwd_bwd", _lib.ptr(p), _lib.ptr(r), _lib.ptr(ld), _lib.ptr(td), B, T, L, C.c_float(rt), C.c_float(alpha),
              int(top_k or 0), int(axis), _lib.ptr(loss), _lib.ptr(loss_q), _lib.ptr(grad), _lib.current_stream(p.device))
    torch.cuda.synchronize()
    return float(loss.item()), loss_q.cpu().numpy(), grad.cpu().numpy()


def run_case(cs, clean=False):
    p, r = cs["preds"], cs["rele"]
    if clean:
        p, r = np.nan_to_num(p, nan=0.0), np.nan_to_num(r, nan=0.0)
    return run_loss(p, r, cs["rt"], cs["alpha"], cs["top_k"], cs["axis"], cs["lens"], cs["ntopics"])


def same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def gate_loss(got, ref, what):
    loss, loss_q, grad = got
    for name, w in (("loss_q", DB.gate_nan(loss_q[ref["q"]], ref["loss_q"], ref["E_loss_q"], f"{what} loss_q", CD)),
                    ("grad", DB.gate_nan(grad[ref["q"]], ref["grad"], ref["E_grad"], f"{what} grad", CD))):
        note(name, w)
    tot, E = DB.batch_total(ref, CD)
    note("loss_out", DB.gate_nan(np.array([loss]), np.array([tot]), np.array([E]), f"{what} loss_out", CD))


# ---------------------------------------------------------------------------------------------------------------- 1. the loss kernel
@pytest.mark.parametrize("name", sorted(LOSS))
def test_loss_within_the_bounds_and_repeatable(name):
    """Every per-query loss, every gradient element (padded slots, empty queries, the all-zero query: exactly 0) and the batch total; the
    same call again and the call without the NaN garbage in the padded slots give the same bits."""
    cs = LOSS[name]
    got = run_case(cs)
    gate_loss(got, ref_of(cs), name)
    assert same(got, run_case(cs)), "not repeatable"
    assert same(got, run_case(cs, clean=True)), "garbage in padded slots changed a bit"


@pytest.mark.parametrize("name", ["form_T7_L100_B9", "form_T30_L64_B5", "offset-_T16_L260", "steep_T8_L200"])
def test_a_query_alone_equals_the_query_inside_its_batch(name):
    cs = LOSS[name]
    _, loss_q, grad = run_case(cs)
    for q in range(cs["preds"].shape[0]):
        one = run_loss(cs["preds"][q:q + 1], cs["rele"][q:q + 1], cs["rt"], cs["alpha"], cs["top_k"], cs["axis"], cs["lens"][q:q + 1],
                       cs["ntopics"][q:q + 1])
        assert one[1][0] == loss_q[q] and np.array_equal(one[2][0], grad[q]), q


@pytest.mark.parametrize("case", sorted(GU._load("diversity_edge.npz")["nonfinite"]))
def test_non_finite_scores_against_the_reference_float64(case):
    """One NaN, two +inf, one -inf score: the reference's float64 loss and gradient are finite (Robust_Sigmoid takes a NaN difference as
    0.5) and so must the kernel's be — NaN exactly where the fixture has one, the gate everywhere else; alone and as query 1 of a padded
    batch of three."""
    c = GU._load("diversity_edge.npz")["nonfinite"][case]
    rele = c["rele"][None].astype(np.float32)
    rt, top_k = float(c["rt"]), int(c["top_k"]) or None
    ref = DB.alphadcg(c["preds"], rele, rt=rt, top_k=top_k)
    ref["loss_q"], ref["grad"] = np.array([float(c["loss64"])]), c["grad64"].astype(np.float64)       # the fixture is the reference here
    got = run_loss(c["preds"], rele, rt=rt, top_k=top_k)
    gate_loss(got, ref, case)
    assert same(got, run_loss(c["preds"], rele, rt=rt, top_k=top_k))
    T, L = rele.shape[1:]
    P, R = np.full((3, L + 3), np.nan, np.float32), np.full((3, T + 1, L + 3), np.nan, np.float32)
    P[1, :L], R[1, :T, :L] = c["preds"][0], rele[0]
    P[0, :2], R[0, :T, :2], P[2, :1], R[2, :1, :1] = [0.5, -0.5], 1.0, 0.25, 1.0
    _, lq, g = run_loss(P, R, rt=rt, top_k=top_k, lens=[2, L, 1], ntopics=[T, T, 1])
    assert lq[1] == got[1][0] and np.array_equal(g[1, :L], got[2][0]) and not g[1, L:].any() and np.isfinite(g).all()


GOLD = GU._load("diversity.npz")["daletor"]


@pytest.mark.parametrize("case", sorted(GOLD))
def test_golden_loss_cases_under_the_element_wise_gate(case):
    """The inputs of tests/test_diversity_gpu.py's golden cases, the steep (rt = 100) ones included, under the new gate.  The reference is
    the restatement: the fixture's own float64 gradient forms 1 - ind by subtraction and is only good to 1e-16 absolute per pair."""
    c = GOLD[case]
    rele = c["rele"][None].astype(np.float32)
    ref = DB.alphadcg(c["preds"], rele, rt=float(c["rt"]), top_k=int(c["top_k"]) or None)
    gate_loss(run_loss(c["preds"], rele, rt=float(c["rt"]), top_k=int(c["top_k"]) or None), ref, case)


# ---------------------------------------------------------------------------------------------------------------- 2. the metric kernel
def run_metrics(cs, clean=False, abi=False):
    import ptranking_amd.functional as F_
    p, r = cs["preds"], cs["rele"]
    if clean:
        n = [DR.clamp_len(cs["lens"], q, p.shape[1]) for q in range(p.shape[0])]
        p = np.stack([np.concatenate([p[q, :n[q]], np.zeros(p.shape[1] - n[q], np.float32)]) for q in range(p.shape[0])])
        r = np.nan_to_num(r, nan=0.0)
    pd, rd, ld, td = dev(p), dev(r), dev(cs["lens"], torch.int32), dev(cs["ntopics"], torch.int32)
    ml = cs["max_label"]
    if not abi:
        a, e, ne, v = F_.div_metrics_at_ks(pd, rd, cs["ks"], alpha=cs["alpha"], max_label=ml, lens=ld, ntopics=td)
    else:
        from ptranking_amd import _lib
        B, T, L = rd.shape
        nk = len(cs["ks"])
        new = lambda: torch.full((B, nk), np.nan).cuda()
        a, e, ne = new(), (None if ml is None else new()), (None if ml is None else new())
        v = torch.full((B,), -1, dtype=torch.int32).cuda()
        _lib.call("ptr_div_metrics_at_ks", _lib.ptr(pd), _lib.ptr(rd), _lib.ptr(ld), _lib.ptr(td), B, T, L, (C.c_int32 * nk)(*cs["ks"]), nk,
                  C.c_float(cs["alpha"]), C.c_float(0.0 if ml is None else ml), _lib.ptr(a), _lib.ptr(e), _lib.ptr(ne), _lib.ptr(v),
                  _lib.current_stream(pd.device))
    torch.cuda.synchronize()
    f = lambda t: None if t is None else t.cpu().numpy()
    return f(a), f(e), f(ne), f(v)


def same_metrics(x, y):
    return all((a is None and b is None) or np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


@pytest.mark.parametrize("name", sorted(METRIC))
def test_metrics_within_the_bounds_and_repeatable(name):
    """alpha-nDCG, ERR-IA and nERR-IA per (query, cut-off) inside their bounds, `valid` and every exact zero exactly, finite everywhere —
    with NaN scores too, which rank first as in ptr_sort_desc and torch.sort; twice, through the C ABI and with clean padding: the same bits
    (two documents scattered into one rank would show here)."""
    cs = METRIC[name]
    got = run_metrics(cs)
    assert all(np.isfinite(m).all() for m in got[:3] if m is not None)
    DB.gate_metrics(got, ref_of(cs), name, CD, NEEDS)
    for other in (run_metrics(cs), run_metrics(cs, abi=True), run_metrics(cs, clean=True)):
        assert same_metrics(got, other)


def test_nan_scores_follow_ptr_sort_desc():
    """The order the metrics walk is the order of functional.sort_desc on the very rows that hold NaN, +-inf and +-0.0."""
    import ptranking_amd.functional as F_
    for name in ("nan_L65", "T5_inf", "T5_zeros"):
        cs = METRIC[name]
        full = [q for q in range(cs["preds"].shape[0]) if DR.clamp_len(cs["lens"], q, cs["preds"].shape[1]) == cs["preds"].shape[1]]
        rows = cs["preds"][full]
        _, idx = F_.sort_desc(dev(rows))
        assert np.array_equal(idx.cpu().numpy(), np.stack([DR.sort_desc_order(r) for r in rows])), name


# ---------------------------------------------------------------------------------------------------------------- 3. the ranker surface
def test_daletor_evaluation_with_a_nan_prediction():
    """DALETOR.alpha_ndcg_at_k and srd_performance_at_ks on padded batches in which one prediction per batch is NaN: the averages over the
    kept queries equal the restatement's on the very predictions the kernel saw, inside the per-query bounds plus the fp32 mean's."""
    import ptranking_amd as pa
    import test_diversity_gpu as TG
    data = TG._query_set(nq=40, seed=12)
    batches = pa.DivQueryBatches(data, "cuda:0", rough_batch_size=512, pad_to=16)
    r = TG._make()
    seen = []
    inner = r._score_batch

    def with_nan(X, lens):
        preds = inner(X, lens).clone()
        preds[0, 1] = float("nan")
        seen.append(preds.detach().cpu().numpy())
        return preds
    r._score_batch = with_nan
    ks = [1, 5, 10, 20]
    got = r.srd_performance_at_ks(test_data=batches, ks=ks, max_label=1.0)
    preds_by_batch, seen[:] = list(seen), []
    got10 = r.alpha_ndcg_at_k(batches, k=10)
    assert len(preds_by_batch) == len(batches) > 1 and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(preds_by_batch, seen))

    def want(kk, min_len):
        sums, Es, cnt = np.zeros((3, len(kk))), np.zeros((3, len(kk))), 0
        for preds, (ids, X, rele, lens, nts) in zip(preds_by_batch, batches):
            assert np.isnan(preds[0, 1])
            ref = DB.metrics(preds, rele.cpu().numpy(), kk, 0.5, 1.0, lens.cpu().numpy(), nts.cpu().numpy())
            keep = (ref["valid"] > 0) & ((lens.cpu().numpy() >= min_len) if min_len else True)
            for m, name in enumerate(DB.METRIC_OUTPUTS):
                sums[m] += ref[name][keep].sum(0)
                Es[m] += ref["E_" + name][keep].sum(0) + CD * U * np.abs(ref[name][keep]).sum(0)
            cnt += int(keep.sum())
        return sums / cnt, Es / cnt + CD * U * np.abs(sums / cnt)
    w, E = want(ks, None)
    for m, name in enumerate(DB.METRIC_OUTPUTS):
        assert got[m].shape == (len(ks),) and torch.isfinite(got[m]).all()
        note(name, DB.gate_nan(got[m].numpy(), w[m], E[m], f"DALETOR srd_performance_at_ks {name}", CD))
    w10, E10 = want([10], 10)
    note("andcg", DB.gate_nan(got10.numpy(), w10[0], E10[0], "DALETOR alpha_ndcg_at_k", CD))


# ---------------------------------------------------------------------------------------------------------------- 4. the report
def test_zz_report_the_worst_needs():
    """Runs last in this module: the kernel's worst need per output over everything above (diversity_bounds.KERNEL_NEEDS holds the figures
    of the last measurement)."""
    print("MEASURED diversity kernels, worst need per output: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(NEEDS.items())))
    assert all(v <= CD for v in NEEDS.values())
