"""No GPU: the argument contract of ptr_xattn_forward / ptr_xattn_backward, their kernel forms, the Python module's refusals, and the proof
that the GPU gate of tests/test_xattn_gpu.py is not vacuous: fp32 torch on the CPU passes the very same bounds on the very same inputs."""
import ctypes as C
import math

import pytest
import torch

from test_xattn_gpu import CASES, case_id, gate_all, inputs, _mask

INVALID, UNSUPPORTED = 1001, 1002      # PTR_ERR_INVALID_ARG, PTR_ERR_UNSUPPORTED


def _call(backward, Lq=20, Lk=70, F=24, H=3, B=2, ld_q=None, ld_kv=None, qbs=0, null=False):
    """Either entry point on host buffers that no kernel ever sees: every case here must fail before a launch."""
    from ptranking_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 16)()
    p = None if null else C.cast(buf, C.c_void_p)
    head = (p, F if ld_q is None else ld_q, C.c_int64(qbs), p, p, F if ld_kv is None else ld_kv, None, None, B, Lq, Lk, F, H)
    if backward:
        return lib.ptr_xattn_backward(*head, p, p, p, p, p, p, p, None)
    return lib.ptr_xattn_forward(*head, p, p, None)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("kw,code", [(dict(Lq=65, Lk=65), UNSUPPORTED), (dict(F=129, H=1), UNSUPPORTED), (dict(F=25), INVALID),
                                     (dict(Lq=0), INVALID), (dict(Lk=-1), INVALID), (dict(B=-1), INVALID), (dict(ld_kv=23), INVALID),
                                     (dict(ld_q=8), INVALID), (dict(qbs=-1), INVALID), (dict(null=True), INVALID)],
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_contract_errors_need_no_device(backward, kw, code):
    assert _call(backward, **kw) == code


@pytest.mark.parametrize("entry", ["ptr_xattn_forward", "ptr_xattn_backward"])
@pytest.mark.parametrize("Lq,Lk,dh,form", [(512, 32, 68, (0, 5, 4, 2)), (32, 512, 68, (1, 5, 4, 2)), (20, 20, 4, (0, 1, 4, 2)),
                                           (1000, 64, 128, (0, 8, 4, 4)), (16, 65, 17, (1, 2, 4, 1))])
def test_kernel_form(entry, Lq, Lk, dh, form):
    from ptranking_amd import _lib
    out = (C.c_int32 * 4)()
    assert _lib.load().ptr_launch_form(entry.encode(), (C.c_int64 * 3)(Lq, Lk, dh), 3, out, 4) == 0
    assert tuple(out) == form          # short side (0 keys / 1 queries), column tiles D, waves, row tiles of the short side


def test_module_refusals():
    from ptranking_amd import _lib, setrank as SR
    with pytest.raises(ValueError, match="n_induce"):
        SR.IMSAB(24, 3, n_induce=65)
    with pytest.raises(_lib.NativeLibraryError):
        SR.cross_attention(torch.randn(20, 24), torch.randn(2, 70, 24), torch.randn(2, 70, 24), 3)
    import ptranking_amd as pa
    assert pa.SetRank is SR.SetRank


def _fp32(Q, K, V, dO, H, lq, lk):
    """The rule and its gradients in fp32 torch on the CPU, the backward from its own O and lse as the kernels' is."""
    Bn, Lk, F = K.shape
    hd = lambda T: T.reshape(Bn, -1, H, F // H).permute(0, 2, 1, 3)
    mg = lambda T: T.permute(0, 2, 1, 3).reshape(Bn, -1, F).contiguous()
    q, k, v, g = hd(Q if Q.dim() == 3 else Q.expand(Bn, -1, -1)), hd(K), hd(V), hd(dO)
    s = torch.tensor(1.0 / math.sqrt(F // H), dtype=torch.float32)
    ok = _mask(Bn, q.shape[2], Lk, lq, lk).expand(Bn, H, -1, -1)
    has = ok.any(-1, keepdim=True)
    S = (q @ k.transpose(-1, -2)) * s
    lse = torch.where(has, torch.logsumexp(S.masked_fill(~ok, -math.inf), -1, keepdim=True), torch.zeros(1))
    P = torch.where(ok, torch.exp(S - lse), torch.zeros(1))
    O = P @ v
    dS = P * (g @ v.transpose(-1, -2) - (O * g).sum(-1, keepdim=True)) * s
    return dict(O=mg(O), lse=lse[..., 0], dQ=mg(dS @ k), dK=mg(dS.transpose(-1, -2) @ q), dV=mg(P.transpose(-1, -2) @ g))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gate_is_not_vacuous(case):
    """fp32 torch passes the GPU gate's bounds on the GPU gate's inputs.  Worst need over the cases: O 1.13, lse 2.14, dQ 2.22, dV 3.30, dK 2.46
    (the kernels on an MI355X: O 1.52, lse 2.11, dQ 2.58, dV 3.25, dK 2.55, and 7.34 where a subnormal probability is flushed: the FLT_MIN floor)."""
    Q, K, V, dO, lq, lk, H = inputs(case)
    gate_all(_fp32(Q, K, V, dO, H, lq, lk), Q, K, V, dO, H, lq, lk, "fp32 torch " + case_id(case))
