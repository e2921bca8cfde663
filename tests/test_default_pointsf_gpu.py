"""GPU: the reference's DEFAULT pointsf — FusedStack, 5 x [Linear -> LTRBatchNorm('BN', affine) -> GELU] with dropout, then Linear ->
BN -> Sigmoid (ptranking/ltr_adhoc/eval/parameter.py:145-146) — end to end at the row counts bench.py --scorer pointsf_default runs,
against the same modules evaluated in float64 on the CPU with the kernels' own dropout masks.

The gate is per column: every column of the output and of dX, and every row (output unit) of each parameter gradient, is compared
with the largest float64 value of that column / row, so a wrong small column cannot hide behind a large one.  140 001 rows: the
whole-batch statistics use 512 chunks of 274 rows and the last chunk starts past the end of the batch (csrc/bnact.hip,
colsum2_reduce_kernel<1>); the features carry an offset of ~20 standard deviations, so the first layer's pre-activations have a mean
far above their spread and a wrong chunk count in the variance shows."""
import copy
import ctypes as C

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
CPU_REFERENCE_MODULES = True      # tests/conftest.py: the reference is the same module objects evaluated by torch on the CPU

DEFAULT = dict(num_layers=5, AF='GE', TL_AF='S', apply_tl_af=True, BN=True, bn_type='BN', bn_affine=True)
# worst per-column (per-row) err / scale measured on an MI355X at both row counts (printed as MEASURED below): output 1.7e-6, dX 5.0e-6,
# weight gradients 6.3e-6 (ff_2.weight), bias / gamma / beta gradients 2.0e-6; the tolerances keep 3x above that.  The batch-norm
# statistics with the empty last chunk counted as negative rows miss by 1.3e-3 at 140 001 rows.
TOL_OUT = 5e-6
TOL_GRAD = 2e-5


def _mask(R, width, p, seed, site):
    from ptranking_amd import _lib
    ones = torch.ones(R, width, device="cuda")
    m = torch.empty_like(ones)
    _lib.call("ptr_dropout_apply", _lib.ptr(ones), width, R, width, C.c_float(p), C.c_uint64(seed), site, _lib.ptr(m), width,
              _lib.current_stream(ones.device))
    return (m > 0).double().cpu()


def _cpu_forward_with_masks(net_cpu, x, p, seed, R):
    site = 0
    for m in net_cpu:
        if isinstance(m, nn.Dropout):
            x = x * _mask(R, x.shape[-1], p, seed, site).view(x.shape) / (1 - p)
            site += 1
        else:
            x = m(x)
    return x


def _per_column(got, ref, tol, what, dim, floor=0.0):
    """max over `dim` of |got - ref| <= tol * max(max over `dim` of |ref|, floor), for every column (dim=0) or row (dim=1)."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.detach().double().cpu()
    if ref.dim() == 1:
        got, ref = got.reshape(-1, 1), ref.reshape(-1, 1)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err = (got - ref).abs().amax(dim=dim)
    scale = ref.abs().amax(dim=dim).clamp(min=floor)
    ratio = err / (scale + 1e-30)
    worst = int(ratio.argmax())
    print(f"MEASURED default pointsf {what}: worst per-{'column' if dim == 0 else 'row'} err/scale {float(ratio[worst]):.3e}")
    bad = err > tol * scale + 1e-30
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} {'columns' if dim == 0 else 'rows'} off; worst {worst}: "
                                 f"max|diff| {float(err[worst]):.3e} > {tol:g} x scale {float(scale[worst]):.3e}")


@pytest.mark.parametrize("B,L", [(1024, 128), (69, 2029)], ids=["131072-rows", "140001-rows"])
def test_default_pointsf_end_to_end_matches_float64_cpu_modules(B, L):
    from ptranking_amd.host import build_pointsf
    from ptranking_amd.linear import FusedStack
    F, p = 136, 0.1
    torch.manual_seed(11 + L)
    net = build_pointsf(num_features=F, dropout=p, **DEFAULT)
    assert isinstance(net, FusedStack)
    with torch.no_grad():                                   # non-trivial affine parameters
        for n_, prm in net.named_parameters():
            if "bn" in n_:
                prm.add_(0.3 * torch.randn_like(prm))
    ref = copy.deepcopy(net).double()                       # CPU tensors: FusedStack.forward is the plain torch modules
    net = net.cuda()
    net.train(); ref.train()
    R = B * L
    g = torch.Generator().manual_seed(R)
    scale = torch.pow(2.0, torch.randint(-3, 4, (F,), generator=g).double())
    x = ((torch.randn(B, L, F, generator=g, dtype=torch.float64) + 20.0) * scale).float()    # feature offsets ~20 standard deviations
    xg = x.cuda().requires_grad_(True)
    out = net(xg)
    assert net._plan and net._plan["kind"] == "bn" and not net._plan["relu_only"]
    gout = torch.randn(B, L, 1, generator=g)
    gout[:, L - L // 8:] = 0.0                              # padded-looking documents: zero gradient rows
    out.backward(gout.cuda())
    xr = x.double().clone().requires_grad_(True)
    outr = _cpu_forward_with_masks(ref, xr, p, net.last_seed, R)
    outr.backward(gout.double())
    _per_column(out.reshape(R, -1), outr.reshape(R, -1), TOL_OUT, "out", 0)
    _per_column(xg.grad.reshape(R, F), xr.grad.reshape(R, F), TOL_GRAD, "dx", 0)
    # weights: per row (output unit).  A Linear bias in front of batch norm has an exactly-zero gradient in float64 (the normalisation
    # removes it), so the vectors (biases, gamma, beta) are measured against the largest weight gradient of their layer
    got = dict(net.named_parameters())
    refs = dict(ref.named_parameters())
    for n_, prm in refs.items():
        if prm.dim() == 2:
            _per_column(got[n_].grad, prm.grad, TOL_GRAD, n_, 1)
        else:
            layer_w = refs["ff_" + n_.split(".")[0].split("_")[1] + ".weight"].grad
            _per_column(got[n_].grad.reshape(1, -1), prm.grad.reshape(1, -1), TOL_GRAD, n_, 1, floor=float(layer_w.abs().max()))
