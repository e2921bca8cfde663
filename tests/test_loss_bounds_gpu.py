"""GPU: the ranking-loss kernels (csrc/pairwise.hip + ptr_ring.h, csrc/approxndcg.hip, csrc/listwise.hip, csrc/lambdaloss.hip) against
float64 with ELEMENT-WISE error bounds (tests/f64_loss_bounds.py) on structured inputs.  The C ABI is called directly, so that every output is gated:
each query's loss_q, the batch total loss_out, every gradient element (padded slots exactly 0), and ApproxNDCG's dcg_q, inv_idcg_q and
scale_out.  Outputs start as NaN, so a slot the kernel never writes fails.

The case lists launch every dispatch form of these entry points (tests/test_abi_cpu.py restates the rules and checks that they do).
Where the O(B L^2) float64 reference of a bench-sized batch is too slow, a sample of queries is gated (`sample_queries`: the first and
the last, both sides of every few workgroup boundaries, random ones); the kernel still runs the whole batch.  Each gate prints its
worst err/E as a MEASURED line (run with -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import f64_loss_bounds as FL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUS = 256                                   # MI355X compute units (the ring kernel's workgroup rule, tests/test_abi_cpu.py)


def _t(a, dtype=torch.float32, unaligned=False):
    a = torch.as_tensor(np.ascontiguousarray(a)).to(dtype)
    if not unaligned:
        return a.to(DEV).contiguous()
    buf = torch.empty(a.numel() + 1, dtype=dtype, device=DEV)        # one element in: 4-byte aligned, not 16
    v = buf[1:].view(a.shape)
    v.copy_(a.to(DEV))
    return v


def _nan(shape, unaligned=False):
    if not unaligned:
        return torch.full(shape, float("nan"), device=DEV)
    buf = torch.full((int(np.prod(shape)) + 1,), float("nan"), device=DEV)
    return buf[1:].view(shape)


def run(name, preds, second, lens, *params, unif=None, unaligned=False, approx=False):
    """One ABI call.  Returns dict(loss_out, loss_q, grad) (ApproxNDCG: loss_out, dcg_q, inv_idcg_q, scale, grad) as float64 numpy."""
    from ptranking_amd import _lib
    B, L = np.asarray(preds).shape
    p = _t(preds, unaligned=unaligned)
    s = _t(second, torch.int64 if name == "ptr_listmle_fwd_bwd" else torch.float32)
    ln = _t(lens, torch.int32)
    out, g = _nan((1,)), _nan((B, L), unaligned)
    st = _lib.current_stream(torch.device(DEV))
    if approx:
        dcg, inv, sc = _nan((B,)), _nan((B,)), _nan((2,))
        _lib.call(name, _lib.ptr(p), _lib.ptr(s), _lib.ptr(ln), B, L, *params, _lib.ptr(out), _lib.ptr(dcg), _lib.ptr(inv), _lib.ptr(sc),
                  _lib.ptr(g), st)
        torch.cuda.synchronize()
        f = lambda t: t.double().cpu().numpy()
        return dict(loss_out=float(out.item()), dcg_q=f(dcg), inv_idcg_q=f(inv), scale=f(sc), grad=f(g))
    lq = _nan((B,))
    args = [_lib.ptr(p), _lib.ptr(s)] + ([_lib.ptr(_t(unif))] if unif is not None else []) + [_lib.ptr(ln), B, L]
    _lib.call(name, *args, *params, _lib.ptr(out), _lib.ptr(lq), _lib.ptr(g), st)
    torch.cuda.synchronize()
    return dict(loss_out=float(out.item()), loss_q=lq.double().cpu().numpy(), grad=g.double().cpu().numpy())


def sample_queries(B, qpb, k=12, seed=0):
    """All queries of a small batch; else the specials (0..5, f64_loss_bounds.pair_inputs), the last, both sides of k workgroup boundaries
    and k random ones."""
    if B <= 96:
        return None
    g = np.random.default_rng(seed)
    nb = (B + qpb - 1) // qpb
    bounds = g.choice(np.arange(1, nb), size=min(k, nb - 1), replace=False) * qpb
    q = np.concatenate([[0, 1, 2, 3, 4, 5, B - 1], bounds - 1, bounds, g.integers(0, B, size=k)])
    return np.unique(q[(q >= 0) & (q < B)])


def ring_qpb(B, L):
    """Queries per workgroup of the LambdaRank ring kernel (pairwise.hip launch_pairwise)."""
    dpt = 1 if L <= 64 else 2 if L <= 128 else 4 if L <= 256 else 8
    qpb = 16
    while qpb > 1 and B < qpb * CUS:
        qpb >>= 1
    return min(qpb, 8) if dpt >= 4 and dpt < 8 else min(qpb, 4) if dpt >= 8 else qpb


def _check(got, ref, what, c, full):
    w = FL.gate_losses(got["loss_q"], got["grad"], ref, what, c)
    if full:
        w = max(w, FL.gate_nan(np.array([got["loss_out"]]), np.array([ref["loss_q"].sum()]),
                               np.array([FL.batch_total(ref, c)[1]]), f"{what} loss_out", c))
    return w


# ---------------------------------------------------------------------------------------------------------------------------- pair losses
# (B, L, sigma, label mix, quantised + offset, lens, PTR_LAMBDARANK_RING, labels sorted as the reference feeds them)
LAMBDARANK_CASES = [
    (37, 20, 1.0, "mslr", False, "ragged", 1, False),          # ring DPT 1, shrunk workgroup, B not a multiple of it
    (300, 64, 1.0, "yahoo", True, "ragged", 1, False),         # DPT 1, quantised ties + 1e3 offset
    (4096, 64, 1.0, "yahoo", False, "ragged", 1, False),       # DPT 1, full 16-wave workgroups
    (70, 128, 1.0, "mslr", False, "full", 1, False),           # DPT 2, no trailing equal slots
    (4096, 128, 1.0, "mslr", False, "ragged", 1, False),       # the bench batch: DPT 2, full 16-wave workgroups
    (50, 256, 2.0, "yahoo", True, "ragged", 1, False),         # DPT 4, shrunk
    (4096, 256, 1.0, "yahoo", False, "full", 1, False),        # DPT 4, full 8-wave workgroups
    (40, 512, 1.0, "mslr", False, "ragged", 1, False),         # DPT 8, shrunk
    (4096, 512, 1.0, "mslr", True, "full", 1, False),          # DPT 8, full 4-wave workgroups, offset
    (33, 64, 1.0, "mslr", False, "ragged", 0, False),          # LDS kernel, tiling (64, 1)
    (33, 128, 1.0, "yahoo", True, "ragged", 0, False),         # (64, 2)
    (21, 256, 1.0, "mslr", False, "ragged", 0, False),         # (256, 1)
    (13, 512, 1.0, "mslr", False, "ragged", 0, False),         # (256, 2)
    (7, 700, 1.0, "yahoo", False, "ragged", 1, False),         # L > 512: LDS (256, 4)
    (5, 1500, 1.0, "mslr", False, "ragged", 1, False),         # (256, 8)
    (3, 2100, 1.0, "mslr", False, "full", 1, False),           # (256, 16)
    (19, 100, 0.0, "mslr", False, "ragged", 1, False),         # sigma 0: LDS (64, 2)
    (70, 128, 1.0, "mslr", False, "full", 1, True),             # DPT 2 on label-sorted lists: real grade-0 slots skipped (Z > 0)
    (4096, 256, 1.0, "mslr", False, "ragged", 1, True),         # DPT 4, sorted, full workgroups (sampled)
    (40, 512, 1.0, "mslr", True, "full", 1, True),              # DPT 8, sorted, offset
]

# (B, L, sigma, label mix, quantised + offset, lens)
RANKNET_CASES = [
    (37, 20, 1.0, "mslr", False, "ragged"),             # L <= 32: two queries per wavefront
    (66, 32, 1.0, "yahoo", True, "full"),
    (33, 64, 1.0, "mslr", False, "ragged"),             # pairwise_bce_kernel (64, 1)
    (33, 128, 1.0, "yahoo", True, "ragged"),            # (64, 2)
    (21, 256, 1.0, "mslr", False, "ragged"),            # (256, 1)
    (13, 512, 1.0, "mslr", False, "full"),              # (256, 2)
    (7, 700, 1.0, "yahoo", False, "ragged"),            # (256, 4)
    (5, 1500, 1.0, "mslr", False, "ragged"),            # (256, 8)
    (3, 2100, 2.0, "mslr", True, "ragged"),             # (256, 16)
]


def _pair_id(c):
    return (f"{c[0]}x{c[1]}-s{c[2]:g}-{c[3]}" + ("-quant-offset" if c[4] else "") + f"-{c[5]}" + (f"-ring{c[6]}" if len(c) > 6 else "")
            + ("-sorted" if len(c) > 7 and c[7] else ""))


def lambdarank_inputs(case):
    """The inputs of a LAMBDARANK_CASES entry (tests/test_abi_cpu.py computes the ring kernel's Z from them)."""
    Bn, L, sigma, mix, qo, lens, ring, srt = case
    return FL.pair_inputs(Bn, L, sigma=sigma if sigma > 0 else 1.0, mix=mix, seed=L + Bn, quantise=qo, offset=1000.0 if qo else 0.0,
                          lens=lens, sort_labels=srt)


@pytest.mark.parametrize("case", LAMBDARANK_CASES, ids=_pair_id)
def test_lambdarank_against_float64(case, monkeypatch):
    Bn, L, sigma, mix, qo, lens, ring, srt = case
    monkeypatch.setenv("PTR_LAMBDARANK_RING", str(ring))
    p, y, n, screened = lambdarank_inputs(case)
    assert screened <= FL.MAX_SCREENED
    got = run("ptr_lambdarank_fwd_bwd", p, y, n, C.c_float(sigma))
    qs = sample_queries(Bn, ring_qpb(Bn, L))
    ref = FL.lambdarank(p, y, n, sigma, FL.C_PAIR, qs)
    _check(got, ref, f"lambdarank {_pair_id(case)}", FL.C_PAIR, qs is None)
    if qs is not None:                                   # padded slots of every query, sampled or not
        pad = np.arange(L)[None, :] >= n[:, None]
        assert (got["grad"][pad] == 0).all()


@pytest.mark.parametrize("L,ring", [(60, 1), (128, 1), (256, 1), (512, 1), (128, 0), (700, 1)])
def test_lambdarank_loss_out_against_float64(L, ring, monkeypatch):
    """The batch total as a value: every query has a relevant document (one without makes loss_out NaN, as the reference)."""
    monkeypatch.setenv("PTR_LAMBDARANK_RING", str(ring))
    p, y, n, _ = FL.pair_inputs(23, L, seed=L + 1, every_relevant=True)
    got = run("ptr_lambdarank_fwd_bwd", p, y, n, C.c_float(1.0))
    ref = FL.lambdarank(p, y, n, 1.0, FL.C_PAIR)
    assert np.isfinite(ref["loss_q"]).all()
    _check(got, ref, f"lambdarank loss_out {L}-ring{ring}", FL.C_PAIR, True)


@pytest.mark.parametrize("case", RANKNET_CASES, ids=_pair_id)
def test_ranknet_against_float64(case):
    Bn, L, sigma, mix, qo, lens = case
    p, y, n, screened = FL.pair_inputs(Bn, L, sigma=sigma, mix=mix, seed=3 * L + Bn, quantise=qo, offset=1000.0 if qo else 0.0, lens=lens)
    assert screened <= FL.MAX_SCREENED
    got = run("ptr_ranknet_fwd_bwd", p, y, n, C.c_float(sigma))
    ref = FL.ranknet(p, y, n, sigma, FL.C_PAIR)
    _check(got, ref, f"ranknet {_pair_id(case)}", FL.C_PAIR, True)


# ---------------------------------------------------------------------------------------------------------------------------- ApproxNDCG
# (B, L, presort, couple_batch, grad_scale_override, PTR_APPROX_RING, quantised + offset)
APPROX_CASES = [
    (37, 50, 1, 1, 0.0, 1, False),        # ring DPT 1, coupled
    (40, 128, 1, 0, 0.0, 1, True),        # DPT 2, per query (NaN on the query without a relevant document), offset
    (21, 192, 0, 1, 0.0, 1, False),       # DPT 3, labels sorted by the kernel
    (4096, 256, 1, 1, 1.0, 1, False),     # DPT 4, the data-parallel form on the bench batch (sampled)
    (4096, 128, 1, 1, 1.0, 1, True),      # DPT 2 bench batch, offset (sampled)
    (13, 384, 0, 0, 0.0, 1, False),       # DPT 6
    (9, 512, 1, 1, 0.0, 1, True),         # DPT 8
    (4096, 512, 1, 1, 1.0, 1, False),     # DPT 8 bench batch (sampled)
    (33, 64, 1, 1, 0.0, 0, False),        # LDS kernel (64, 1)
    (33, 128, 0, 0, 0.0, 0, False),       # (64, 2)
    (17, 256, 1, 1, 1.0, 0, True),        # (256, 1), data parallel
    (9, 512, 1, 0, 0.0, 0, False),        # (256, 2)
    (5, 700, 1, 1, 0.0, 1, False),        # L > 512: LDS (256, 4)
    (3, 1500, 0, 1, 0.0, 1, False),       # (256, 8)
    (2, 2100, 1, 0, 0.0, 1, False),       # (256, 16)
]
ALPHA = 10.0


def _approx_id(c):
    Bn, L, pre, cpl, ov, ring, qo = c
    return f"{Bn}x{L}-pre{pre}-couple{cpl}-ov{ov:g}-ring{ring}" + ("-offset" if qo else "")


@pytest.mark.parametrize("case", APPROX_CASES, ids=_approx_id)
def test_approxndcg_against_float64(case, monkeypatch):
    Bn, L, presort, couple, override, ring, qo = case
    monkeypatch.setenv("PTR_APPROX_RING", str(ring))
    c = FL.C_APPROX
    p, y, n, screened = FL.pair_inputs(Bn, L, sigma=ALPHA, mix="mslr", seed=L + 7 * Bn, quantise=qo, offset=1000.0 if qo else 0.0,
                                       every_relevant=bool(couple))
    assert screened <= FL.MAX_SCREENED
    got = run("ptr_approxndcg_fwd_bwd", p, y, n, C.c_float(ALPHA), presort, couple, C.c_float(override), approx=True)
    qs = sample_queries(Bn, 4)
    what = f"approxndcg {_approx_id(case)}"
    ref = FL.approxndcg(p, y, n, ALPHA, bool(presort), bool(couple), override, c, qs)
    q = ref["q"]
    FL.gate_nan(got["dcg_q"][q], ref["dcg_q"], ref["E_dcg_q"], f"{what} dcg_q", c)
    FL.gate_nan(got["inv_idcg_q"][q], ref["inv_idcg_q"], ref["E_inv_idcg_q"], f"{what} inv_idcg_q", c)
    if qs is None:
        FL.gate_nan(got["grad"], ref["grad"], ref["E_grad"], f"{what} grad", c)
        FL.gate_nan(got["scale"][:1], [ref["scale"]], [ref["E_scale"]], f"{what} scale_out[0]", c)
        FL.gate_nan([got["loss_out"]], [ref["loss"]], [ref["E_loss"]], f"{what} loss_out", c)
    else:                                                 # sampled: only the data-parallel form's grad needs no batch-wide S
        assert couple and override == 1.0
        FL.gate_nan(got["grad"][q], ref["grad"], ref["E_grad"], f"{what} grad", c)
        assert got["scale"][0] == 1.0
        pad = np.arange(L)[None, :] >= n[:, None]
        assert (got["grad"][pad] == 0).all()
    if couple:
        _, _, S, E_S = FL.approx_inv_idcg(y, n, bool(presort), c)
        FL.gate_nan(got["scale"][1:], [S], [E_S], f"{what} scale_out[1] (S)", c)


# ---------------------------------------------------------------------------------------------------------------------------- listwise
# (B, L, quantised offset, unaligned rows)
LISTWISE_CASES = [
    (37, 64, False, False),       # ListNet vector form (16, 1); ListMLE V 1
    (33, 128, True, False),       # (32, 1), offset
    (21, 256, False, False),      # (64, 1)
    (4096, 128, False, False),    # the bench batch (sampled)
    (13, 512, False, False),      # (64, 2); ListMLE V 2
    (4096, 512, False, False),    # bench batch, V 2 (sampled)
    (7, 1024, True, False),       # (64, 4); ListMLE V 4
    (11, 63, False, False),       # L % 4 != 0: the LDS kernels
    (9, 128, False, True),        # unaligned rows: the LDS kernels
    (3, 1500, False, False),      # L > 1024: the LDS kernels
]


def _list_id(c):
    return f"{c[0]}x{c[1]}" + ("-offset" if c[2] else "") + ("-unaligned" if c[3] else "")


@pytest.mark.parametrize("case", LISTWISE_CASES, ids=_list_id)
def test_listwise_against_float64(case):
    Bn, L, off, unal = case
    c = FL.C_LIST
    p, y, n = FL.listwise_inputs(Bn, L, seed=L + Bn, offset=1000.0 if off else 0.0)
    qs = sample_queries(Bn, 4)
    full = qs is None
    got = run("ptr_listnet_fwd_bwd", p, y, n, unaligned=unal)
    _check(got, FL.listnet(p, y, n, c, qs), f"listnet {_list_id(case)}", c, full)
    perm = FL.listmle_perm(y, n, seed=Bn)
    got = run("ptr_listmle_fwd_bwd", p, perm, n, unaligned=unal)
    _check(got, FL.listmle(p, perm, n, c, qs), f"listmle {_list_id(case)}", c, full)
    if Bn <= 96:
        got = run("ptr_rankcosine_fwd_bwd", p, y, n)
        _check(got, FL.rankcosine(p, y, n, c), f"rankcosine {_list_id(case)}", c, True)
        got = run("ptr_rankmse_fwd_bwd", p, y, n)
        ref = FL.rankmse(p, y, n, c)
        FL.gate_losses(got["loss_q"], got["grad"], ref, f"rankmse {_list_id(case)}", c)
        tot, E = FL.batch_total(ref, c, 1.0 / Bn)
        FL.gate_nan([got["loss_out"]], [tot], [E], f"rankmse {_list_id(case)} loss_out", c)


# ---------------------------------------------------------------------------------------------------------------------------- LambdaLoss
# (B, L, k, loss type 0 Loss1 / 1 Loss2 / 2 Loss2++, presort, sigma, flags): q quantised + 1e3 offset, u unaligned rows, c both clamps
# populated (k >= L), x scores x 30 (the top-k kernel's libm route), n NaN scores in three lists (fewer than k documents with a rank by
# score: such a list's outputs are NaN).  tests/test_abi_cpu.py restates ptr_lambdaloss_fwd_bwd's route.
LAMBDALOSS_GENERIC_CASES = [
    (37, 20, 1, 0, 1, 1.0, ""),          # (64, 1): Loss1, k = 1 (the diagonal alone)
    (38, 64, 64, 1, 0, 1.0, "c"),        # (64, 1): k = L, even circulant walk, labels sorted by the kernel
    (33, 128, 2, 2, 0, 2.0, ""),         # (64, 2): k = 2
    (30, 128, 128, 2, 1, 1.0, "c"),      # (64, 2): k = L, Loss2++ with both clamps
    (21, 256, 37, 0, 1, 1.0, "q"),       # (64, 4): Loss1, odd k, ties + offset
    (13, 300, 600, 1, 1, 2.0, ""),       # (256, 2): k = 2 L > n
    (10, 512, 512, 0, 0, 1.0, "c"),      # (256, 2): Loss1 at k = L with both clamps
    (7, 700, 40, 2, 1, 1.0, ""),         # (256, 4): even k
    (9, 1500, 5, 0, 1, 1.0, ""),         # (256, 8): Loss1, k = 5
    (7, 2100, 101, 1, 0, 1.0, ""),       # (256, 16): odd k
    (18, 64, 12, 1, 1, 1.0, ""),         # top-k eligible but k = 12
    (19, 63, 5, 2, 1, 1.0, ""),          # ... but L % 4 != 0
    (17, 128, 5, 1, 1, 1.0, "u"),        # ... but unaligned rows
    (22, 64, 5, 0, 1, 1.0, ""),          # ... but Loss1
    (23, 256, 5, 2, 0, 1.0, ""),         # ... but presort = 0
    (19, 64, 20, 1, 1, 1.0, "n"),        # NaN scores, one wavefront per list
    (13, 300, 7, 2, 0, 1.0, "n"),        # NaN scores, four wavefronts per list, labels sorted by the kernel
]
LAMBDALOSS_TOPK_CASES = [
    (37, 8, 5, 2, 1, 1.0, ""),           # V 1: lists shorter than k (the pair table rebuilt)
    (29, 64, 1, 1, 1, 1.0, ""),          # k = 1: no pair
    (41, 64, 11, 1, 1, 1.0, "q"),        # k = 11 (55 pairs), ties across lanes and inside a lane's four documents
    (26, 256, 2, 2, 1, 2.0, ""),         # full lists (lens == 256: the mask-free path) among ragged ones
    (27, 64, 5, 2, 1, 2.5, "x"),         # |sigma ds| > 80: the libm route and p < eps
    (14, 512, 5, 1, 1, 1.0, ""),         # V 2, with full lists
    (11, 1024, 11, 2, 1, 1.0, "q"),      # V 4
    (21, 8, 5, 1, 1, 1.0, "n"),          # V 1: lists with 2, 0 and n - 1 real scores (the selection ends early)
    (13, 512, 5, 2, 1, 1.0, "n"),        # V 2: the same
]
LAMBDALOSS_PERSISTENT = (3 * 8192 + 17, 8, 5, 2, 1, 1.0, "")      # every wavefront walks >= 3 queries: 8192 is all the device can hold
MU = 5.0


def _ll_id(c):
    return f"{c[0]}x{c[1]}-k{c[2]}-t{c[3]}-pre{c[4]}-s{c[5]:g}" + (f"-{c[6]}" if c[6] else "")


def lambdaloss_inputs(case):
    """The inputs of a LAMBDALOSS_*_CASES entry (tests/test_abi_cpu.py computes the top-k kernel's route from them)."""
    Bn, L, k, lt, pre, sigma, fl = case
    out = FL.lambdaloss_inputs(Bn, L, k, sigma=sigma, mu=MU, loss_type=lt, presort=bool(pre), need_clamps="c" in fl,
                               scale=30.0 if "x" in fl else 1.0, seed=L + 3 * Bn + lt, quantise="q" in fl,
                               offset=1000.0 if "q" in fl else 0.0, mix="yahoo" if (Bn + L) % 2 else "mslr")
    if "n" in fl:
        # three lists beyond the specials with at least four documents: two real scores left (fewer than k), none, all but one
        p, n = out[0], out[2]
        qa, qb, qc = [q for q in range(8, Bn) if n[q] >= 4][:3]
        p[qa, 1:n[qa] - 1] = np.nan
        p[qb, :n[qb]] = np.nan
        p[qc, 1] = np.nan
        assert min(k, int(n[qa])) > 2
    return out


def _run_lambdaloss(case, p, y, n):
    _, _, k, lt, pre, sigma, fl = case
    return run("ptr_lambdaloss_fwd_bwd", p, y, n, k, C.c_float(sigma), C.c_float(MU), lt, pre, unaligned="u" in fl)


@pytest.mark.parametrize("case", LAMBDALOSS_GENERIC_CASES, ids=_ll_id)
def test_lambdaloss_generic_against_float64(case):
    Bn, L, k, lt, pre, sigma, fl = case
    p, y, n, *_ = lambdaloss_inputs(case)
    got = _run_lambdaloss(case, p, y, n)
    ref = FL.lambdaloss(p, y, n, k, sigma, MU, lt, bool(pre), FL.C_LLOSS)
    assert "n" not in fl or np.isnan(ref["loss_q"]).sum() == 3 + (lt == 0)
    _check(got, ref, f"lambdaloss generic {_ll_id(case)}", FL.C_LLOSS, True)


@pytest.mark.parametrize("case", LAMBDALOSS_TOPK_CASES, ids=_ll_id)
def test_lambdaloss_topk_against_float64(case):
    Bn, L, k, lt, pre, sigma, fl = case
    p, y, n, *_ = lambdaloss_inputs(case)
    got = _run_lambdaloss(case, p, y, n)
    ref = FL.lambdaloss(p, y, n, k, sigma, MU, lt, True, FL.C_LLOSS, log_floor=True)
    assert "n" not in fl or np.isnan(ref["loss_q"]).sum() == 3
    _check(got, ref, f"lambdaloss topk {_ll_id(case)}", FL.C_LLOSS, True)


def lambdaloss_persistent_inputs():
    """256 distinct ragged queries (lengths 0..8, so kk changes between a wavefront's consecutive queries) tiled in a shuffled order.
    Returns (preds, labels, lens, order [B]: the distinct query behind each row)."""
    Bn, L, k, lt, pre, sigma, _ = LAMBDALOSS_PERSISTENT
    p, y, n, *_ = FL.lambdaloss_inputs(256, L, k, sigma=sigma, mu=MU, loss_type=lt, presort=True, seed=11)
    g = np.random.default_rng(12)
    n = (np.arange(256) % 9).astype(np.int32)
    g.shuffle(n)
    for q in range(256):                                 # the screen saw other lengths: no entry of the lists as they now are nears a clamp
        assert not FL.lambdaloss_query(p[q, :n[q]], y[q, :n[q]], k, sigma, MU, lt, True, 1.0, detail=True)[4].any(), q
    order = g.permutation(Bn) % 256
    return p[order], y[order], n[order], order


def test_lambdaloss_topk_persistent_walk_against_float64():
    Bn, L, k, lt, pre, sigma, _ = LAMBDALOSS_PERSISTENT
    p, y, n, order = lambdaloss_persistent_inputs()
    got = _run_lambdaloss(LAMBDALOSS_PERSISTENT, p, y, n)
    _, first = np.unique(order, return_index=True)
    assert len(first) == 256
    ref = FL.lambdaloss(p, y, n, k, sigma, MU, lt, True, FL.C_LLOSS, first, log_floor=True)
    _check(got, ref, "lambdaloss topk persistent", FL.C_LLOSS, False)
    src = first[order]                                   # every copy is bit-identical to the first copy of its query
    assert np.array_equal(got["loss_q"], got["loss_q"][src], equal_nan=True)
    assert np.array_equal(got["grad"], got["grad"][src], equal_nan=True)
    assert (got["grad"][np.arange(L)[None, :] >= n[:, None]] == 0).all()
    # the whole batch's total (ptr_sum_f32 at this B): every row's float64 loss and bound are those of the first copy of its query
    lq, E = ref["loss_q"][order], ref["E_loss_q"][order]
    assert np.isfinite(lq).all()
    FL.gate_nan(np.array([got["loss_out"]]), np.array([lq.sum()]), np.array([E.sum() + FL.C_LLOSS * FL.U * np.abs(lq).sum()]),
                "lambdaloss topk persistent loss_out", FL.C_LLOSS)


@pytest.mark.parametrize("L,k,lt", [(64, 5, 2), (64, 64, 0), (300, 40, 1)])
def test_lambdaloss_loss_out_against_float64(L, k, lt):
    """The batch total as a value: every query has a relevant document (one without makes Loss1's total NaN), one has length 0."""
    p, y, n, _ = FL.pair_inputs(23, L, seed=L + 2, every_relevant=True, sort_labels=True)
    n[4] = 0
    got = run("ptr_lambdaloss_fwd_bwd", p, y, n, k, C.c_float(1.0), C.c_float(MU), lt, 1)
    ref = FL.lambdaloss(p, y, n, k, 1.0, MU, lt, True, FL.C_LLOSS, log_floor=k <= 11)
    assert np.isfinite(ref["loss_q"]).all() and ref["loss_q"][4] == 0
    _check(got, ref, f"lambdaloss loss_out {L}-k{k}-t{lt}", FL.C_LLOSS, True)


# ---------------------------------------------------------------------------------------------------------------------------- SoftRank
# (B, L, delta, top_k (0: none), 1e3 offset): one case per dispatch_tiling form
SOFTRANK_CASES = [
    (37, 50, 2.0, 0, False),          # (64, 1)
    (33, 128, 0.3, 10, False),        # (64, 2)
    (21, 256, 2.0, 300, False),       # (256, 1), top_k > n
    (13, 512, 0.3, 0, True),          # (256, 2), offset
    (7, 700, 2.0, 10, False),         # (256, 4)
    (6, 1500, 0.3, 0, False),         # (256, 8)
    (5, 2100, 2.0, 10, False),        # (256, 16)
]


def _soft_id(c):
    return f"{c[0]}x{c[1]}-d{c[2]:g}-k{c[3]}" + ("-offset" if c[4] else "")


def softrank_inputs(Bn, L, delta, off, **kw):
    """Label-sorted lists whose (s_i - s_j) / den spans the indicator's whole range, with the specials of pair_inputs."""
    p, y, n, _ = FL.pair_inputs(Bn, L, sigma=FL.softrank_inv_den(delta), seed=L + 5 * Bn, offset=1000.0 if off else 0.0, sort_labels=True,
                                span=8.0, **kw)
    return p, y, n


@pytest.mark.parametrize("case", SOFTRANK_CASES, ids=_soft_id)
def test_softrank_against_float64(case):
    Bn, L, delta, top_k, off = case
    p, y, n = softrank_inputs(Bn, L, delta, off)
    got = run("ptr_softrank_fwd_bwd", p, y, n, C.c_float(delta), top_k)
    ref = FL.softrank(p, y, n, delta, top_k, FL.C_APPROX)
    assert ref["loss_q"][4] == 0 and (Bn < 6 or np.isnan(ref["loss_q"][2]))
    _check(got, ref, f"softrank {_soft_id(case)}", FL.C_APPROX, True)


def test_softrank_loss_out_with_a_zero_length_query_against_float64():
    """The batch total as a value: every query has a relevant document, one has length 0 (loss 0, not 0 * inf)."""
    p, y, n = softrank_inputs(23, 70, 2.0, False, every_relevant=True)
    n[4] = 0
    got = run("ptr_softrank_fwd_bwd", p, y, n, C.c_float(2.0), 0)
    ref = FL.softrank(p, y, n, 2.0, 0, FL.C_APPROX)
    assert np.isfinite(ref["loss_q"]).all() and ref["loss_q"][4] == 0
    _check(got, ref, "softrank loss_out", FL.C_APPROX, True)


# ---------------------------------------------------------------------------------------------------------------------------- STListNet
# (B, L, temperature, 1e3 offset, unaligned rows); one kernel form (listnet_kernel with the Gumbel prologue)
STLISTNET_CASES = [(37, 64, 1.0, False, False), (11, 63, 2.0, True, False), (9, 128, 0.5, False, True), (6, 1500, 1.0, False, False)]


@pytest.mark.parametrize("case", STLISTNET_CASES, ids=lambda c: f"{c[0]}x{c[1]}-T{c[2]:g}" + ("-offset" if c[3] else "") + ("-unaligned" if c[4] else ""))
def test_stlistnet_against_float64(case):
    Bn, L, T, off, unal = case
    p, y, u, n = FL.stlistnet_inputs(Bn, L, seed=L + Bn, offset=1000.0 if off else 0.0)
    assert n[3] == 1 and n[4] == 0
    got = run("ptr_stlistnet_fwd_bwd", p, y, n, C.c_float(T), unif=u, unaligned=unal)
    ref = FL.stlistnet(p, y, u, n, T, FL.C_LIST)
    _check(got, ref, f"stlistnet {Bn}x{L}-T{T:g}", FL.C_LIST, True)
