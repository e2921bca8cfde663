"""GPU: the dense-layer kernels against float64 with ELEMENT-WISE error bounds (tests/f64_bounds.py) on structured LETOR-like data —
every dispatch form forced through its switch: the Linear forward / backward-input (PTR_LIN_X6 = 0 / 1 / 2), the weight gradient
(PTR_LIN_BW_X6), the fused pointsf scorer forward (PTR_MLP_X6) and backward (PTR_BWD_X6, PTR_BWD_FUSED, PTR_BWD_TAIL,
PTR_DW_X6 / PTR_DW_X6_FORM), and batch-norm statistics / bnact forward / backward for every activation, whole-batch and per-query
groups, with and without padded lists, from under 256 rows to 524 288 (more than 128 partials, 512 chunks of more than 64 rows).
Each gate prints its worst err/E as a MEASURED line (run with -s)."""
import ctypes as C

import pytest
import torch

import f64_bounds as B

pytestmark = pytest.mark.gpu

LIN_NONE, LIN_RELU, LIN_RELU_DROPOUT = 0, 1, 2


def _c_lin(mode):
    return B.C_FP32 if mode == "0" else B.C_X6


def _dropout_mask(R, N, p, seed, site):
    """The keep mask of a (seed, site) dropout of the linear / bnact kernels, from the kernels' own generator: ptr_dropout_apply on ones."""
    from ptranking_amd import _lib
    ones = torch.ones(R, N, device="cuda")
    out = torch.empty_like(ones)
    _lib.call("ptr_dropout_apply", _lib.ptr(ones), N, R, N, C.c_float(p), C.c_uint64(seed), site, _lib.ptr(out), N, _lib.current_stream(ones.device))
    return (out > 0).double().cpu()


# ---------------------------------------------------------------------------------------------------------------------------- Linear
LIN_FWD_SHAPES = [(4133, 136, 136), (2049, 136, 408), (70003, 100, 100), (1000, 136, 128), (2000, 512, 136), (1300, 700, 100), (50, 7, 5),
                  (140001, 136, 136), (66000, 36, 200)]
LIN_FWD_CASES = [(s, a) for s in LIN_FWD_SHAPES for a in (LIN_NONE, LIN_RELU, LIN_RELU_DROPOUT) if not (a == LIN_RELU_DROPOUT and s[2] % 4)]


@pytest.mark.parametrize("mode", ["0", "1", "2"])
@pytest.mark.parametrize("shape,act", LIN_FWD_CASES)
def test_linear_forward_within_f64_bounds(shape, act, mode, monkeypatch):
    from ptranking_amd.linear import _fwd
    monkeypatch.setenv("PTR_LIN_X6", mode)
    R, K, N = shape
    X, info = B.structured_inputs(R, K, seed=R + K)
    W, b = B.weights(N, K, seed=N), torch.randn(N)
    p, seed, site = (0.25 if act == LIN_RELU_DROPOUT else 0.0), 4321, 3
    y = _fwd(X.cuda(), K, W.cuda(), b.cuda(), act=act, p=p, seed=seed, site=site)
    torch.cuda.synchronize()
    c = _c_lin(mode)
    Z, EZ = B.gemm_fwd(X, W, b, c)
    what = f"linear fwd R={R} K={K} N={N} act={act} PTR_LIN_X6={mode}"
    if act == LIN_NONE:
        B.gate(y, Z, EZ, what, c)
        return
    s = _dropout_mask(R, N, p, seed, site) / (1 - p) if act == LIN_RELU_DROPOUT else torch.ones_like(Z)
    amb = Z.abs() <= EZ
    assert float(amb.double().mean()) <= B.MAX_AMBIGUOUS, f"{what}: {float(amb.double().mean()):.3%} of the outputs at the ReLU kink"
    ref = Z.clamp(min=0) * s
    E = (EZ * s + B.U * ref.abs()) * ((Z > 0) | amb).double()
    got = B.d64(y)
    accept = amb & ((got == 0) | ((got - Z * s).abs() <= EZ * s + B.U * (Z * s).abs()))
    B.gate(y, ref, E, what, c, accept=accept)


LIN_BWD_SHAPES = [(4133, 136, 136), (1500, 128, 136), (70003, 100, 100), (2049, 136, 408), (1200, 200, 300), (777, 128, 256), (50, 7, 5)]


@pytest.mark.parametrize("mode", ["0", "1", "2"])
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("shape", LIN_BWD_SHAPES)
def test_linear_backward_input_within_f64_bounds(shape, gated, mode, monkeypatch):
    from ptranking_amd.linear import _bwd_input
    monkeypatch.setenv("PTR_LIN_X6", mode)
    R, K, N = shape
    dY, zero_rows = B.structured_grads(R, N, seed=R + N)
    W = B.weights(N, K, seed=K)
    gate, _ = B.structured_inputs(R, K, seed=R) if gated else (None, None)
    p = 0.1 if gated else 0.0
    dx = _bwd_input(dY.cuda(), W.cuda(), gate=None if gate is None else gate.cuda(), p=p)
    torch.cuda.synchronize()
    c = _c_lin(mode)
    G, E = B.gemm_bwd_input(dY, W, c, gate=gate, p=p)
    B.gate(dx, G, E, f"linear bwd-input R={R} K={K} N={N} gated={gated} PTR_LIN_X6={mode}", c)
    assert bool((dx.cpu()[zero_rows] == 0).all()), "a zero dY row must give an exactly-zero dX row"


LIN_BW_SHAPES = [(2049, 136, 408), (40000, 136, 408), (70003, 100, 100), (4097, 140, 1536), (300, 700, 100), (65, 100, 4), (1, 136, 136),
                 (130, 4, 8), (257, 256, 112), (31, 8, 400), (1000, 140, 144)]


@pytest.mark.parametrize("bw_x6", ["0", "2"], ids=["0-None", "2-None"])       # ids as before the form switch was removed
@pytest.mark.parametrize("shape", LIN_BW_SHAPES)
def test_linear_weight_gradient_within_f64_bounds(shape, bw_x6, monkeypatch):
    from ptranking_amd.linear import _bwd_weight
    monkeypatch.setenv("PTR_LIN_BW_X6", bw_x6)
    R, K, N = shape
    X, info = B.structured_inputs(R, K, seed=R * 3 + K)
    dY, _ = B.structured_grads(R, N, seed=N)
    dw = torch.full((N, K), float("nan"), device="cuda")
    db = torch.full((N,), float("nan"), device="cuda")
    _bwd_weight(X.cuda(), K, dY.cuda(), True, dw_out=dw, db_out=db)
    torch.cuda.synchronize()
    c = B.C_FP32 if bw_x6 == "0" else B.C_X6
    rW, EW, rb, Eb = B.gemm_bwd_weight(X, dY, c)
    what = f"linear dW R={R} K={K} N={N} PTR_LIN_BW_X6={bw_x6}"
    B.gate(dw, rW, EW, what, c)
    B.gate(db, rb, Eb, what + " db", c)
    if R > 1:
        assert bool((dw.cpu()[:, info["zero_col"]] == 0).all()), "an all-zero X column must give an exactly-zero dW column"


# ---------------------------------------------------------------------------------------------------------------------------- scorer
SCORER_SHAPES = [(136, 3, 4096 * 128), (136, 3, 1), (136, 3, 4133), (140, 2, 3001), (46, 3, 2049), (256, 4, 5000), (256, 3, 40000),
                 (700, 3, 65536 + 17), (136, 4, 777), (140, 3, 33000)]
BWD_FORMS = [("default", {}), ("fp32 fused", {"PTR_BWD_X6": "0"}), ("layer-wise + tail", {"PTR_BWD_FUSED": "0"}),
             ("layer-wise + fp32 tail", {"PTR_BWD_FUSED": "0", "PTR_BWD_X6": "0"}), ("layer-wise", {"PTR_BWD_FUSED": "0", "PTR_BWD_TAIL": "0"}),
             ("dW x6 off", {"PTR_DW_X6": "0"}), ("dW x6 form 16", {"PTR_DW_X6": "2", "PTR_DW_X6_FORM": "16"}),
             ("dW x6 form 24", {"PTR_DW_X6": "2", "PTR_DW_X6_FORM": "24"})]
BWD_SWITCHES = ("PTR_BWD_X6", "PTR_BWD_FUSED", "PTR_BWD_TAIL", "PTR_DW_X6", "PTR_DW_X6_FORM")


@pytest.mark.parametrize("F,NL,R", SCORER_SHAPES)
def test_scorer_forward_and_backward_within_f64_bounds(F, NL, R, monkeypatch):
    """Train forward (kernel's own dropout masks) and eval forward with PTR_MLP_X6 = 0 / 2; after each train forward, the backward in every
    form of BWD_FORMS on the stored activations.  Rows holding a ReLU unit within its bound of the kink get zero output gradient."""
    from ptranking_amd import _lib
    from ptranking_amd import scorer as S
    from ptranking_amd.scorer import FusedPointScorer
    torch.manual_seed(F + NL + R)
    p, seed = 0.1, 777 + R
    fused = FusedPointScorer(F, num_layers=NL, dropout=p).cuda()
    views = fused.views()
    Ws = [views[f"ff_{l + 2}.weight"].cpu() for l in range(NL + 1)]
    bs = [views[f"ff_{l + 2}.bias"].cpu() for l in range(NL + 1)]
    X, _ = B.structured_inputs(R, F, seed=R + F, scale_exp=(-6, 6))
    Xd = X.cuda()
    masks = [fused.dropout_mask(R, s, seed).cpu() for s in range(NL)]
    c = max(B.C_FP32, B.C_X6)
    ref = B.relu_mlp(X, Ws, bs, c, masks=masks, p=p)
    assert ref["amb_frac"] <= B.MAX_AMBIGUOUS, f"{ref['amb_frac']:.3%} of the hidden units at the ReLU kink"
    dout, _ = B.structured_grads(R, 1, seed=R)
    dout = dout[:, 0].masked_fill(ref["amb_rows"], 0.0)
    ref = B.relu_mlp(X, Ws, bs, c, masks=masks, p=p, dout=dout)
    ref_eval = B.relu_mlp(X, Ws, bs, c)
    layout = fused.layout()
    dev = Xd.device
    st = _lib.current_stream(dev)
    for x6 in ("0", "2"):
        monkeypatch.setenv("PTR_MLP_X6", x6)
        if x6 == "2" and S.x6_wimg_for(Xd, R, F, NL, True, dev) is None:
            continue            # the bf16x6 forward does not serve this shape (F % 4 != 0, ...): "2" would rerun the fp32-MFMA forward
        preds = torch.empty(R, device=dev)
        S.mlp_forward(Xd, fused.flat.data, R, F, NL, False, 0.0, 0, preds, None, dev)
        torch.cuda.synchronize()
        B.gate(preds, ref_eval["out"], ref_eval["E_out"], f"scorer eval fwd F={F} NL={NL} R={R} PTR_MLP_X6={x6}", c)
        acts = S.alloc_acts(R, NL, dev)
        S.mlp_forward(Xd, fused.flat.data, R, F, NL, True, p, seed, preds, acts, dev)
        torch.cuda.synchronize()
        B.gate(preds, ref["out"], ref["E_out"], f"scorer train fwd F={F} NL={NL} R={R} PTR_MLP_X6={x6}", c)
        dpreds = dout.float().cuda()
        for name, env in BWD_FORMS:
            for k in BWD_SWITCHES:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            ndz = _lib.query("ptr_mlp_backward_dz_floats", R, F, NL)
            dz = torch.empty(max(ndz, 1), device=dev)
            ws = torch.empty(_lib.query("ptr_mlp_backward_ws_floats", F, NL), device=dev)
            g = torch.full_like(fused.flat.data, float("nan"))
            _lib.call("ptr_mlp_backward", _lib.ptr(Xd), _lib.ptr(fused.flat.data), _lib.ptr(acts), _lib.ptr(dpreds), R, F, NL, C.c_float(p),
                      C.c_uint64(seed), _lib.ptr(dz) if ndz else None, _lib.ptr(ws), _lib.ptr(g), st)
            torch.cuda.synchronize()
            gc = g.cpu()
            for key, off, shp in layout:
                l = int(key.split(".")[0][3:]) - 2
                n = 1
                for d in shp:
                    n *= d
                got = gc[off:off + n].view(shp)
                if key.endswith("weight"):
                    B.gate(got, ref["dW"][l], ref["E_dW"][l], f"scorer bwd {key} F={F} NL={NL} R={R} x6={x6} form={name}", c)
                else:
                    B.gate(got, ref["db"][l], ref["E_db"][l], f"scorer bwd {key} F={F} NL={NL} R={R} x6={x6} form={name}", c)
        for k in BWD_SWITCHES:
            monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------------------------------------------------------------------- batch norm
# (R, N, group, L for padded lists or 0): under 256 rows; above 8 192 (the backward reduction sums more than 128 partials); 32 768 and up
# (512 chunks of more than 64 rows); 140 001 (512 statistics chunks of 274 rows: the last starts past R); 524 288
BN_CASES = [(200, 100, 0, 0), (200, 7, 0, 0), (240, 24, 24, 24), (8320, 100, 0, 0), (8320, 100, 0, 128), (8320, 36, 128, 128), (9001, 13, 0, 0),
            (40000, 100, 0, 125), (40000, 100, 125, 0), (140001, 100, 0, 0), (131073, 12, 0, 0), (524288, 100, 0, 0), (524288, 100, 128, 128)]
AF_ALL = [B.AF_NONE, B.AF_RELU, B.AF_LEAKY, B.AF_ELU, B.AF_SELU, B.AF_GELU, B.AF_SIGMOID, B.AF_TANH]


@pytest.mark.parametrize("R,N,group,L", BN_CASES)
def test_batch_norm_statistics_forward_backward_within_f64_bounds(R, N, group, L):
    from ptranking_amd.linear import _bn_stats, _bnact_fwd, _bnact_bwd
    z, info = B.structured_inputs(R, N, seed=R + N + group, scale_exp=(-8, 8))
    lens = None
    if L:
        g = torch.Generator().manual_seed(R)
        lens = torch.randint(1, L + 1, (R // L,), generator=g, dtype=torch.int32)
        lens[::3] = L
    zd = z.cuda()
    lens_d = lens.cuda() if lens is not None else None
    tag = f"R={R} N={N} group={group} L={L}"
    mean, rstd = _bn_stats(zd, group, lens_d, L)
    torch.cuda.synchronize()
    rm, rr, Em, Er = B.bn_stats(z, B.C_BNACT, group, lens, L)
    B.gate(mean.view_as(rm), rm, Em, f"bn stats mean {tag}", B.C_BNACT)
    B.gate(rstd.view_as(rr), rr, Er, f"bn stats rstd {tag}", B.C_BNACT)
    # constant column: mean exactly the constant, xhat exactly 0
    xh = _bnact_fwd(zd, group, mean, rstd, None, None, B.AF_NONE, 0.0, 0, 0)
    assert bool((xh[:, info["const_col"]] == 0).all()), "a constant column must normalise to exactly 0"
    gamma, beta = torch.randn(N) * 2, torch.randn(N)
    afs = AF_ALL if R * N <= 4_000_000 else [B.AF_RELU, B.AF_GELU, B.AF_SIGMOID]
    for af in afs:
        p, seed, site = 0.1, 99 + af, 2
        keep = _bnact_fwd(torch.ones_like(zd), 0, None, None, None, None, B.AF_NONE, p, seed, site).cpu().double() * (1 - p)
        keep = (keep > 0.5).double()
        out = _bnact_fwd(zd, group, mean, rstd, gamma.cuda(), beta.cuda(), af, p, seed, site, lens_d, L)
        torch.cuda.synchronize()
        a, Ea, acc = B.bnact_fwd(z, mean.cpu(), rstd.cpu(), gamma, beta, af, B.C_BNACT, group, keep=keep, p=p)
        B.gate(out, a, Ea, f"bnact fwd {B.AF_NAMES[af]} {tag}", B.C_BNACT, accept=B.accept_from(out, acc))
        da, _ = B.structured_grads(R, N, seed=af + R)
        amb = B.bnact_bwd(z, da, mean.cpu(), rstd.cpu(), gamma, beta, af, B.C_BNACT, group, keep, p, lens, L)["amb"]
        assert float(amb.double().mean()) <= B.MAX_AMBIGUOUS
        da = da.masked_fill(amb, 0.0)
        ref = B.bnact_bwd(z, da, mean.cpu(), rstd.cpu(), gamma, beta, af, B.C_BNACT, group, keep, p, lens, L)
        dz, dg, db = _bnact_bwd(zd, da.cuda(), group, mean, rstd, gamma.cuda(), beta.cuda(), af, p, seed, site, lens=lens_d, L=L)
        torch.cuda.synchronize()
        B.gate(dz, ref["dz"], ref["E_dz"], f"bnact bwd dz {B.AF_NAMES[af]} {tag}", B.C_BNACT)
        B.gate(dg, ref["dgamma"], ref["E_dgamma"], f"bnact bwd dgamma {B.AF_NAMES[af]} {tag}", B.C_BNACT)
        B.gate(db, ref["dbeta"], ref["E_dbeta"], f"bnact bwd dbeta {B.AF_NAMES[af]} {tag}", B.C_BNACT)
