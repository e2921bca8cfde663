"""GPU: the listsf attention core and LayerNorm (csrc/listsf.hip) against float64 with ELEMENT-WISE error bounds (tests/f64_bounds.py:
mhsa_fwd / mhsa_bwd, layernorm_fwd / layernorm_bwd) on structured inputs.  The C ABI is called directly so that the kernel's own O and
LSE (LayerNorm: its own stats) feed the backward, and the backward's gate is taken given them.

The case lists hit every dispatch form (tests/test_abi_cpu.py restates the rules and checks that they do): the attention head-dimension
templates D = ceil(dh / 16) = 1..8, the forward's one or two row tiles per wave, the 4- and 8-wave dK / dV kernels with and without the
stored dS, vector and scalar loads, the packed [B, L, 3F] layout; the LayerNorm register forms NI = ceil(F / 64) = 1..4 and the generic
NI = 0, with row loops that take several trips forward (> 32 768 rows) and backward (> 4096 rows).  Each gate prints its worst err/E as a
MEASURED line (run with -s)."""
import ctypes as C

import pytest
import torch

import f64_bounds as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, L, F, heads, mode, dS scratch, packed [B, L, 3F] projection); dh = F / heads
ATTN_CASES = [
    (2, 7, 8, 2, "eval", False, False),                 # dh 4: D 1
    (3, 33, 32, 2, "lens", False, False),               # dh 16
    (2, 129, 64, 4, "dropout", True, False),            # dh 16, two row tiles, stored dS
    (2, 65, 34, 2, "dropout", False, False),            # dh 17: D 2, scalar loads
    (3, 128, 34, 2, "lens", True, False),               # dh 17, stored dS
    (2, 32, 34, 2, "dropout+lens", False, True),        # dh 17 packed: row stride 3F = 102, scalar loads
    (3, 129, 80, 2, "dropout+lens", True, False),       # dh 40: D 3
    (1, 64, 40, 1, "eval", False, False),               # dh 40, one row tile
    (2, 64, 128, 2, "eval", False, False),              # dh 64: D 4
    (3, 257, 128, 2, "lens", True, False),              # dh 64, two row tiles
    (2, 33, 136, 2, "lens", False, False),              # dh 68: D 5 (config 5)
    (3, 256, 136, 2, "dropout+lens", True, False),      # dh 68 at config 5's list length
    (2, 513, 136, 2, "dropout", False, False),          # dh 68, recomputing dQ
    (2, 130, 136, 2, "dropout+lens", True, True),       # dh 68 packed: row stride 408
    (2, 32, 180, 2, "eval", False, False),              # dh 90: D 6, scalar loads
    (3, 128, 180, 2, "dropout+lens", True, False),      # dh 90, stored dS
    (2, 64, 200, 2, "lens", False, False),              # dh 100: D 7, 4-wave dK / dV
    (2, 129, 700, 7, "eval", False, False),             # dh 100 (700 features, 7 heads): 8-wave dK / dV
    (3, 1031, 200, 2, "dropout+lens", True, False),     # dh 100, 8-wave dK / dV storing dS, a long list
    (2, 257, 224, 2, "lens", True, False),              # dh 112: D 7
    (2, 64, 256, 2, "eval", False, False),              # dh 128: D 8, 4-wave dK / dV
    (2, 65, 256, 2, "dropout", False, False),           # dh 128, 8-wave dK / dV
    (2, 256, 256, 2, "dropout+lens", True, False),      # dh 128, 8-wave dK / dV storing dS
]

LN_FS = [2, 24, 64, 65, 128, 136, 200, 256, 257, 700]
LN_CASES = [(1, 2), (1, 136), (1, 700), (262144, 136)] + [(R, F) for F in LN_FS for R in (4099, 32773)]


def _attn_id(c):
    Bn, L, F, H, mode, ds, packed = c
    return f"{Bn}x{L}x{F}-h{H}-{mode}" + ("-ds" if ds else "") + ("-packed" if packed else "")


@pytest.fixture(scope="module")
def LS():
    from ptranking_amd import listsf
    return listsf


@pytest.mark.parametrize("case", ATTN_CASES, ids=[_attn_id(c) for c in ATTN_CASES])
def test_attention_within_f64_bounds(LS, case):
    from ptranking_amd import _lib
    Bn, L, F, H, mode, use_ds, packed = case
    Q, K, V, dO, lens = B.attn_inputs(Bn, L, F, H, seed=L + F)
    p = 0.1 if "dropout" in mode else 0.0
    lens = lens if "lens" in mode else None
    seed, site = 1000 + L, 2
    keep = LS.mhsa_dropout_mask(Bn, L, H, p, seed, site, DEV).cpu() if p else None
    st = _lib.current_stream(torch.device(DEV))
    if packed:
        qkv = torch.cat([Q, K, V], -1).to(DEV)
        ld, ptrs = 3 * F, [LS._voff(qkv, i * F) for i in range(3)]
        dqkv = torch.full_like(qkv, float("nan"))
        gptrs = [LS._voff(dqkv, i * F) for i in range(3)]
    else:
        dev = [t.to(DEV) for t in (Q, K, V)]
        ld, ptrs = F, [_lib.ptr(t) for t in dev]
        grads = [torch.full_like(dev[0], float("nan")) for _ in range(3)]
        gptrs = [_lib.ptr(t) for t in grads]
    lens_d = lens.to(DEV) if lens is not None else None
    O = torch.full((Bn, L, F), float("nan"), device=DEV)
    lse = torch.full((Bn * H * L,), float("nan"), device=DEV)
    _lib.call("ptr_mhsa_forward", *ptrs, ld, _lib.ptr(lens_d), Bn, L, F, H, C.c_float(p), C.c_uint64(seed), site, _lib.ptr(O), _lib.ptr(lse), st)
    dO_d = dO.to(DEV)
    dvec = torch.empty(Bn * H * L, device=DEV)
    ds_ws = torch.full((Bn * H * L * L,), float("nan"), device=DEV) if use_ds else None
    _lib.call("ptr_mhsa_backward", *ptrs, ld, _lib.ptr(O), _lib.ptr(dO_d), _lib.ptr(lse), _lib.ptr(lens_d), Bn, L, F, H, C.c_float(p),
              C.c_uint64(seed), site, _lib.ptr(dvec), *gptrs, _lib.ptr(ds_ws), st)
    torch.cuda.synchronize()
    if packed:
        dQ, dK, dV = (dqkv[..., i * F:(i + 1) * F].cpu() for i in range(3))
    else:
        dQ, dK, dV = (t.cpu() for t in grads)
    O, lse = O.cpu(), lse.cpu()
    what = f"attention {_attn_id(case)}"
    c = B.C_ATTN
    rO, EO, rL, EL = B.mhsa_fwd(Q, K, V, H, keep, p, lens, c)
    B.gate(O, rO, EO, what + " O", c)
    B.gate(lse.reshape(Bn, H, L), rL, EL, what + " LSE", c)
    ref = B.mhsa_bwd(Q, K, V, O, dO, lse, H, keep, p, lens, c)
    B.gate(dV, ref["dV"], ref["E_dV"], what + " dV", c)
    B.gate(dK, ref["dK"], ref["E_dK"], what + " dK", c)
    B.gate(dQ, ref["dQ"], ref["E_dQ"], what + " dQ", c)
    if lens is not None:
        for b in range(Bn):
            n = int(lens[b])
            assert bool((dK[b, n:] == 0).all()) and bool((dV[b, n:] == 0).all()), f"{what}: dK / dV of padded keys of query {b} not 0"


@pytest.mark.parametrize("R,F", LN_CASES)
def test_layernorm_within_f64_bounds(R, F):
    from ptranking_amd import _lib
    x, a2, b2, dy, kinds = B.ln_inputs(R, F, seed=R + F)
    eps = 1e-6
    st = _lib.current_stream(torch.device(DEV))
    xd, ad, bd, dyd = (t.to(DEV) for t in (x, a2, b2, dy))
    y = torch.full((R, F), float("nan"), device=DEV)
    stats = torch.full((R, 3), float("nan"), device=DEV)
    _lib.call("ptr_layernorm_forward", _lib.ptr(xd), _lib.ptr(ad), _lib.ptr(bd), R, F, C.c_float(eps), _lib.ptr(y), _lib.ptr(stats), st)
    ws = torch.full((_lib.query("ptr_layernorm_backward_ws_floats", F),), float("nan"), device=DEV)
    dx = torch.full((R, F), float("nan"), device=DEV)
    da, db = torch.full((F,), float("nan"), device=DEV), torch.full((F,), float("nan"), device=DEV)
    _lib.call("ptr_layernorm_backward", _lib.ptr(xd), _lib.ptr(ad), _lib.ptr(dyd), _lib.ptr(stats), R, F, _lib.ptr(ws), _lib.ptr(dx),
              _lib.ptr(da), _lib.ptr(db), st)
    torch.cuda.synchronize()
    y, stats, dx, da, db = (t.cpu() for t in (y, stats, dx, da, db))
    what = f"layernorm R={R} F={F}"
    c = B.C_LN
    ry, Ey, rst = B.layernorm_fwd(x, a2, b2, eps, c)
    B.gate(stats[:, 0], rst["mean"], rst["E_mean"], what + " mean", c)
    B.gate(stats[:, 2], rst["sd"], rst["E_sd"], what + " sd", c)
    B.gate(stats[:, 1], rst["rinv"], rst["E_rinv"], what + " rinv", c)
    B.gate(y, ry, Ey, what + " y", c)
    ref = B.layernorm_bwd(x, a2, dy, stats, c)
    B.gate(dx, ref["dx"], ref["E_dx"], what + " dx", c)
    B.gate(da, ref["da"], ref["E_da"], what + " da", c)
    B.gate(db, ref["db"], ref["E_db"], what + " db", c)
    zero = kinds == 5
    if bool(zero.any()):
        assert bool((y[zero] == b2).all()), f"{what}: an all-zero row must give y = b2 exactly"
