"""GPU: the rectangular attention kernels (csrc/xattn.hip) through the C ABI against a float64 restatement of their rule with ELEMENT-WISE
bounds of the form of f64_bounds.mhsa_fwd / mhsa_bwd at C_ATTN (restated below; tests/test_xattn_cpu.py runs the same gate on fp32 torch to
show that it is not vacuous), and the SetRank modules (setrank.py) against a float64 restatement from torch ops on the CPU with the same weights.  Each gate prints its
worst err/E as a MEASURED line (run with -s)."""
import copy
import ctypes as C
import math

import pytest
import torch

import f64_bounds as B
import golden_util as G

pytestmark = pytest.mark.gpu
CPU_REFERENCE_MODULES = True      # tests/conftest.py: the head / tail stacks of the module test are evaluated by torch on the CPU in float64
DEV = "cuda:0"

# (Lq, Lk, head dim, heads, lens: none / q / k / both, Q shared with batch stride 0); B = 3 throughout
CASES = [(70, 20, 4, 3, "none", 0), (70, 20, 20, 1, "both", 0), (130, 64, 128, 1, "k", 0), (130, 64, 20, 3, "q", 0),         # short keys
         (257, 1, 4, 1, "both", 0), (257, 1, 20, 3, "none", 0), (17, 16, 128, 1, "none", 0), (17, 16, 4, 3, "both", 0),
         (20, 70, 20, 3, "both", 1), (20, 70, 4, 1, "none", 0), (64, 130, 128, 1, "k", 1), (64, 130, 20, 3, "q", 0),         # short queries
         (1, 257, 4, 3, "none", 1), (1, 257, 20, 1, "both", 0), (16, 17, 128, 1, "q", 0), (16, 17, 4, 3, "k", 1),
         (20, 20, 20, 3, "both", 0), (20, 20, 4, 1, "none", 0)]                                                             # both short


def case_id(c):
    return f"{c[0]}x{c[1]}-dh{c[2]}-h{c[3]}-lens_{c[4]}" + ("-sharedq" if c[5] else "")


def inputs(case):
    """Structured fp32 inputs (f64_bounds.attn_inputs at the longer side, cut to Lq / Lk) and lens of [0, partial, full]."""
    Lq, Lk, dh, H, mode, shared = case
    Q, K, V, dO, _ = B.attn_inputs(3, max(Lq, Lk), dh * H, H, seed=Lq + Lk + dh)
    Q, K, V, dO = Q[:, :Lq].contiguous(), K[:, :Lk].contiguous(), V[:, :Lk].contiguous(), dO[:, :Lq].contiguous()
    lens = lambda L, flip: torch.tensor([L, (L + 1) // 2, 0] if flip else [0, (L + 1) // 2, L], dtype=torch.int32)
    lq = lens(Lq, False) if mode in ("q", "both") else None
    lk = lens(Lk, mode == "both") if mode in ("k", "both") else None
    return (Q[0].contiguous() if shared else Q), K, V, dO, lq, lk, H


def _mask(Bn, Lq, Lk, lq, lk):
    nq = torch.full((Bn,), Lq) if lq is None else lq.long().clamp(0, Lq)
    nk = torch.full((Bn,), Lk) if lk is None else lk.long().clamp(0, Lk)
    return ((torch.arange(Lq)[None, :] < nq[:, None])[:, None, :, None] & (torch.arange(Lk)[None, :] < nk[:, None])[:, None, None, :])


def reference(Q, K, V, dO, H, lq, lk, O_k, lse_k, c=B.C_ATTN):
    """The rule in float64 with the bounds of f64_bounds.mhsa_fwd / mhsa_bwd: O, lse; dQ, dK, dV given the kernel's own O and lse."""
    Bn, Lk, F = K.shape
    hd = lambda T: B.d64(T).reshape(Bn, -1, H, F // H).permute(0, 2, 1, 3)
    mg = lambda T: T.permute(0, 2, 1, 3).reshape(Bn, -1, F)
    q, k, v, g, o = hd(Q if Q.dim() == 3 else Q.expand(Bn, -1, -1)), hd(K), hd(V), hd(dO), hd(O_k)
    Lq, s, z, tr = q.shape[2], 1.0 / math.sqrt(F // H), torch.zeros(1, dtype=torch.float64), lambda x: x.transpose(-1, -2)
    ok = _mask(Bn, Lq, Lk, lq, lk).expand(Bn, H, Lq, Lk)
    has = ok.any(-1, keepdim=True)
    S, E_S = s * (q @ tr(k)), c * B.U * s * (q.abs() @ tr(k.abs()))
    Sm = S.masked_fill(~ok, -math.inf)
    m, lse = torch.where(has, Sm.amax(-1, keepdim=True), z), torch.where(has, torch.logsumexp(Sm, -1, keepdim=True), z)
    P = torch.exp(Sm - lse)
    e = torch.where(ok, E_S + c * B.U * (1.0 + (S - m).abs()), z)
    Pe = (P * e).sum(-1, keepdim=True)
    E_P = P * (e + Pe) + B.FLT_MIN * ok
    r = dict(O=mg(P @ v), E_O=mg(c * B.U * (P @ v.abs()) + E_P @ v.abs()), lse=lse[..., 0],
             E_lse=torch.where(has, Pe + c * B.U * (lse.abs() + 1.0), z)[..., 0])
    lk_ = B.d64(lse_k).reshape(Bn, H, Lq, 1)
    P = torch.where(ok, torch.exp(S - lk_), z)
    E_P = P * (E_S + c * B.U * (1.0 + (S - lk_).abs())) + B.FLT_MIN * ok
    D, E_D = (o * g).sum(-1, keepdim=True), c * B.U * (o.abs() * g.abs()).sum(-1, keepdim=True)
    dP, E_dP = g @ tr(v), c * B.U * (g.abs() @ tr(v.abs()))
    dS = P * (dP - D) * s
    E_dS = s * (P * (E_dP + E_D + c * B.U * (dP.abs() + D.abs())) + E_P * (dP - D).abs())
    r.update(dQ=mg(dS @ k), E_dQ=mg(c * B.U * (dS.abs() @ k.abs()) + E_dS @ k.abs()),
             dK=mg(tr(dS) @ q), E_dK=mg(c * B.U * (tr(dS.abs()) @ q.abs()) + tr(E_dS) @ q.abs()),
             dV=mg(tr(P) @ g), E_dV=mg(c * B.U * (tr(P) @ g.abs()) + tr(E_P) @ g.abs()))
    return r


def gate_all(got, Q, K, V, dO, H, lq, lk, what):
    """Every output of `got` (O, lse, dQ, dK, dV) within its bound at C_ATTN; E = 0 (padded rows) demands equality.  Returns the needs."""
    r = reference(Q, K, V, dO, H, lq, lk, got["O"], got["lse"])
    return {k: B.C_ATTN * B.gate(got[k], r[k], r["E_" + k], f"{what} {k}", B.C_ATTN) for k in ("O", "lse", "dV", "dK", "dQ")}


def attention64(Q, K, V, H, lq, lk):
    """The rule from differentiable torch ops (float64 [B, L, F] in, O out), for the module reference."""
    Bn, Lq, F = Q.shape
    hd = lambda T: T.reshape(Bn, -1, H, F // H).permute(0, 2, 1, 3)
    ok = _mask(Bn, Lq, K.shape[1], lq, lk)
    dead = ~ok.any(-1, keepdim=True)
    S = (hd(Q) @ hd(K).transpose(-1, -2) / math.sqrt(F // H)).masked_fill(~ok, -math.inf)
    P = torch.softmax(torch.where(dead, torch.zeros_like(S), S), -1) * (~dead)
    return (P @ hd(V)).permute(0, 2, 1, 3).reshape(Bn, Lq, F)


def _run(Q, K, V, dO, H, lq, lk):
    """ptr_xattn_forward + ptr_xattn_backward on NaN-filled outputs; Q [Lq, F] is passed once with batch stride 0."""
    from ptranking_amd import _lib
    Bn, Lk, F = K.shape
    Lq = Q.shape[-2]
    st = _lib.current_stream(torch.device(DEV))
    q, k, v, g = (t.to(DEV) for t in (Q, K, V, dO))
    lqd, lkd = (None if t is None else t.to(DEV) for t in (lq, lk))
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    O, lse, dvec = nan(Bn, Lq, F), nan(Bn, H, Lq), nan(Bn * H * Lq)
    dQ, dK, dV = nan(Bn, Lq, F), nan(Bn, Lk, F), nan(Bn, Lk, F)
    head = (_lib.ptr(q), F, C.c_int64(Lq * F if Q.dim() == 3 else 0), _lib.ptr(k), _lib.ptr(v), F, _lib.ptr(lqd), _lib.ptr(lkd), Bn, Lq, Lk, F, H)
    _lib.call("ptr_xattn_forward", *head, _lib.ptr(O), _lib.ptr(lse), st)
    _lib.call("ptr_xattn_backward", *head, _lib.ptr(O), _lib.ptr(g), _lib.ptr(lse), _lib.ptr(dvec), _lib.ptr(dQ), _lib.ptr(dK), _lib.ptr(dV), st)
    torch.cuda.synchronize()
    return dict(O=O.cpu(), lse=lse.cpu(), dQ=dQ.cpu(), dK=dK.cpu(), dV=dV.cpu())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernels_within_f64_bounds(case):
    Q, K, V, dO, lq, lk, H = inputs(case)
    got = _run(Q, K, V, dO, H, lq, lk)
    gate_all(got, Q, K, V, dO, H, lq, lk, "xattn " + case_id(case))      # padded query rows have E = 0: exact zeros in O, lse, dQ
    again = _run(Q, K, V, dO, H, lq, lk)
    assert all(torch.equal(got[k], again[k]) for k in got), "two calls differ in their bits"


# ---------------------------------------------------------------------------------------------------------------- modules
def _ln(m, x):
    return m.a_2 * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + m.eps) + m.b_2


def _mab64(m, X, Y, lq, lk):
    """setrank.MAB from torch ops on the float64 copy m."""
    a = m.mha
    lin = lambda l, x: x @ l.weight.t() + l.bias
    Xb = X if X.dim() == 3 else X.expand(Y.shape[0], -1, -1)
    kv = lin(a.w_kv, Y)
    att = attention64(lin(a.w_q, Xb), kv[..., :a.hid_dim], kv[..., a.hid_dim:], a.n_heads, lq, lk)
    Hh = _ln(m.norm1, X + lin(a.fc, att))
    return _ln(m.norm2, Hh + lin(m.rff.w2, torch.relu(lin(m.rff.w1, Hh))))


def _imsab64(m, X, lens):
    return _mab64(m.mab_docs, X, _mab64(m.mab_induce, m.I, X, None, lens), lens, None)


def _compare(mods_d, mods_c, out_d, out_c, w):
    (out_d * w.to(DEV)).sum().backward()
    (out_c * w.double()).sum().backward()
    G.assert_close(out_d.detach().cpu().numpy(), out_c.detach().numpy(), "forward")
    for md, mc in zip(mods_d, mods_c):
        for (k, pd), (_, pc) in zip(md.named_parameters(), mc.named_parameters()):
            G.assert_close(pd.grad.cpu().numpy(), pc.grad.numpy(), k)


@pytest.mark.parametrize("with_lens", [False, True], ids=["full", "lens"])
def test_modules_against_float64(with_lens):
    from ptranking_amd import setrank as SR
    torch.manual_seed(5)
    Bn, L, F, H, M = 3, 70, 24, 3, 20
    lens = torch.tensor([70, 33, 1], dtype=torch.int32) if with_lens else None
    real = (torch.arange(L)[None, :] < (lens[:, None] if with_lens else L)).float().expand(Bn, L)
    X = torch.randn(Bn, L, F)
    lens_d = lens.to(DEV) if with_lens else None
    # one IMSAB layer
    layer = SR.IMSAB(F, H, n_induce=M, dropout=0.0)
    ref = copy.deepcopy(layer).double()
    layer.to(DEV)
    w = torch.randn(Bn, L, F) * real[..., None]
    _compare([layer], [ref], layer(X.to(DEV), lens_d), _imsab64(ref, X.double(), lens), w)
    # the whole scorer
    sf = SR.build_setrank(num_features=F, ff_dims=[16, 32], n_heads=H, n_induce=M, encoder_layers=2, dropout=0.0, BN=False)
    sf64 = {k: copy.deepcopy(m).double().eval() for k, m in sf.items()}
    for m in sf.values():
        m.to(DEV).eval()
    x64 = sf64['head_ffnns'](X.double())
    for l in sf64['encoder'].layers:
        x64 = _imsab64(l, x64, lens)
    w = torch.randn(Bn, L) * real
    out = SR.setrank_forward(sf, X.to(DEV), lens_d)
    _compare(list(sf.values()), list(sf64.values()), out, sf64['tail_ffnns'](x64).squeeze(2), w)
    if with_lens:          # other finite features in the padded documents: the real documents' scores and every gradient keep their bits
        X2 = torch.where(real[..., None] > 0, X, 7.0 * torch.randn(Bn, L, F))
        grads = [p.grad.clone() for m in sf.values() for p in m.parameters()]
        for m in sf.values():
            m.zero_grad(set_to_none=True)
        out2 = SR.setrank_forward(sf, X2.to(DEV), lens_d)
        (out2 * w.to(DEV)).sum().backward()
        assert torch.equal(out2[real.to(DEV) > 0], out[real.to(DEV) > 0])
        assert all(torch.equal(a, p.grad) for a, p in zip(grads, (p for m in sf.values() for p in m.parameters())))
