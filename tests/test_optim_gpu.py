"""GPU: the flat optimisers' ONE update rule (csrc/ptr_optim.h `opt_update`) pinned to a restatement outside the code under test.

`tests/optim_ref.py` restates Adam, Adagrad and RMSprop in numpy float32, one rounded operation per line in the kernel's order, with the host
scalars from libm's powf.  Parameters and state buffers must be bit-equal to it after steps 1, 2 and 3 through every route that reaches the rule:
  (a) the stand-alone entry points ptr_adam_step / ptr_adagrad_step / ptr_rmsprop_step (opt_step_kernel, 256 elements per workgroup),
  (b) ptr_opt_step_loss (reduce_partials_kernel over one partial: 64-lane halves of 128-element workgroups) with its loss-slot sum,
  (c) ptr_mlp_backward_step: the rule applied to the gradient bits ptr_mlp_backward returns for the same inputs.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref

pytestmark = pytest.mark.gpu

KIND = {"Adam": 1, "Adagrad": 2, "RMS": 3}            # PTR_OPT_*
# the defaults of FlatAdam / FlatAdagrad / FlatRMSprop with the reference's weight decay, and a second set without it (Adagrad: a decaying rate)
HYPER = {
    "Adam": [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3), dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0)],
    "Adagrad": [dict(lr=1e-2, lr_decay=0.0, eps=1e-10, weight_decay=1e-3), dict(lr=1e-2, lr_decay=0.1, eps=1e-10, weight_decay=0.0)],
    "RMS": [dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=1e-3), dict(lr=3e-3, alpha=0.9, eps=1e-6, weight_decay=0.0)],
}
# the borders of the 64-lane halves and 128-element workgroups of the reduction and of the 256-thread blocks of the step kernel
SIZES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
CASES = [(kind, hs) for kind in KIND for hs in (0, 1)]


def _abi_hypers(kind, h):
    """(hyper1, hyper2) as the entry points take them."""
    return {"Adam": lambda: tuple(h["betas"]), "Adagrad": lambda: (h["lr_decay"], 0.0), "RMS": lambda: (h["alpha"], 0.0)}[kind]()


def _grad(rng, n, it):
    """randn * 10^(it - 3) with |g| >= 2^-20: no square underflows, so every intermediate is a normal float32."""
    g = (rng.standard_normal(n) * 10.0 ** (it - 3)).astype(np.float32)
    tiny = np.float32(2.0 ** -20)
    return np.where(np.abs(g) < tiny, np.where(g < 0, -tiny, tiny), g).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(t, a):
    return np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))


def _state(kind, n):
    names = optim_ref.RULES[kind][1]
    return tuple(np.zeros(n, np.float32) for _ in names), [torch.zeros(n, device="cuda") for _ in names] + [None] * (2 - len(names))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,hs", CASES)
def test_stand_alone_step_is_the_restated_rule(kind, hs, n):
    from ptranking_amd import _lib
    h = HYPER[kind][hs]
    h1, _h2 = _abi_hypers(kind, h)
    rng = np.random.default_rng(1000 * n + 10 * KIND[kind] + hs)
    p = rng.standard_normal(n).astype(np.float32)
    st, (s1, s2) = _state(kind, n)
    pd = _dev(p)
    stream = _lib.current_stream(pd.device)
    f = C.c_float
    for it in (1, 2, 3):
        g = _grad(rng, n, it)
        gd = _dev(g)
        if kind == "Adam":
            _lib.call("ptr_adam_step", _lib.ptr(pd), _lib.ptr(gd), _lib.ptr(s1), _lib.ptr(s2), C.c_int64(n), f(h["lr"]), f(h["betas"][0]), f(h["betas"][1]),
                      f(h["eps"]), f(h["weight_decay"]), it, stream)
        elif kind == "Adagrad":
            _lib.call("ptr_adagrad_step", _lib.ptr(pd), _lib.ptr(gd), _lib.ptr(s1), C.c_int64(n), f(h["lr"]), f(h1), f(h["eps"]), f(h["weight_decay"]), it, stream)
        else:
            _lib.call("ptr_rmsprop_step", _lib.ptr(pd), _lib.ptr(gd), _lib.ptr(s1), C.c_int64(n), f(h["lr"]), f(h1), f(h["eps"]), f(h["weight_decay"]), stream)
        p, st = optim_ref.step(kind, p, g, st, it, **h)
        assert _same(pd, p), (kind, hs, n, it)
        for k, (dev, ref) in enumerate(zip((s1, s2), st)):
            assert _same(dev, ref), (kind, hs, n, it, optim_ref.RULES[kind][1][k])
        assert _same(gd, g)                                         # the gradient is read, not rewritten


@pytest.mark.parametrize("nq", [1, 1000])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,hs", CASES)
def test_opt_step_loss_is_the_restated_rule(kind, hs, n, nq):
    from ptranking_amd import _lib
    h = HYPER[kind][hs]
    h1, h2 = _abi_hypers(kind, h)
    rng = np.random.default_rng(1000 * n + 10 * KIND[kind] + hs + 7)
    p = rng.standard_normal(n).astype(np.float32)
    st, (s1, s2) = _state(kind, n)
    pd = _dev(p)
    lq = _dev(rng.random(nq).astype(np.float32))
    stream = _lib.current_stream(pd.device)
    f = C.c_float
    want = torch.empty(1, device="cuda")
    _lib.call("ptr_sum_f32", _lib.ptr(lq), nq, f(1.0), _lib.ptr(want), stream)
    for it in (1, 2, 3):
        g = _grad(rng, n, it)
        gd = _dev(g)
        got = torch.full((1,), float("nan"), device="cuda")
        _lib.call("ptr_opt_step_loss", _lib.ptr(pd), _lib.ptr(gd), C.c_int64(n), KIND[kind], f(h["lr"]), f(h1), f(h2), f(h["eps"]), f(h["weight_decay"]), it,
                  _lib.ptr(s1), _lib.ptr(s2), _lib.ptr(lq), nq, _lib.ptr(got), stream)
        p, st = optim_ref.step(kind, p, g, st, it, **h)
        assert _same(pd, p), (kind, hs, n, it)
        for k, (dev, ref) in enumerate(zip((s1, s2), st)):
            assert _same(dev, ref), (kind, hs, n, it, optim_ref.RULES[kind][1][k])
        assert torch.equal(got, want) and _same(gd, g)


# F = 24: the layer-wise backward (partials of two grids: a border inside a reduction workgroup); F = 136: the single-pass backward
@pytest.mark.parametrize("F,NL,R", [(24, 3, 31), (136, 3, 33)])
@pytest.mark.parametrize("kind,hs", CASES)
def test_backward_step_is_the_restated_rule_on_the_backward_s_gradient(kind, hs, F, NL, R):
    """ptr_mlp_backward on the same inputs gives the gradient bits; the restatement applied to them must give the parameters and the state
    ptr_mlp_backward_step leaves (and ptr_mlp_backward_step must return that gradient and the loss-slot sum)."""
    from ptranking_amd import _lib
    from ptranking_amd import scorer as _scorer
    h = HYPER[kind][hs]
    h1, h2 = _abi_hypers(kind, h)
    torch.manual_seed(F + R + KIND[kind] + hs)
    fused = _scorer.FusedPointScorer(F, num_layers=NL, dropout=0.1).cuda()
    params = fused.flat.data
    n = params.numel()
    p = params.cpu().numpy().copy()
    st, (s1, s2) = _state(kind, n)
    X = torch.randn(R, F, device="cuda")
    nq = 7
    lq = torch.rand(nq, device="cuda")
    stream = _lib.current_stream(X.device)
    f = C.c_float
    preds = torch.empty(R, device="cuda")
    acts = _scorer.alloc_acts(R, NL, "cuda")
    ws = torch.empty(_lib.query("ptr_mlp_backward_ws_floats", F, NL), device="cuda")
    ndz = _lib.query("ptr_mlp_backward_dz_floats", R, F, NL)
    dz = torch.empty(ndz, device="cuda") if ndz else None
    want = torch.empty(1, device="cuda")
    _lib.call("ptr_sum_f32", _lib.ptr(lq), nq, f(1.0), _lib.ptr(want), stream)
    for it in (1, 2, 3):
        w = torch.randn(R, device="cuda") * 10.0 ** (it - 3)
        seed = 100 * it + R
        _lib.call("ptr_mlp_forward", _lib.ptr(X), _lib.ptr(params), R, F, NL, 1, f(0.1), C.c_uint64(seed), _lib.ptr(preds), _lib.ptr(acts), stream)
        g = torch.full_like(params, float("nan"))
        _lib.call("ptr_mlp_backward", _lib.ptr(X), _lib.ptr(params), _lib.ptr(acts), _lib.ptr(w), R, F, NL, f(0.1), C.c_uint64(seed), _lib.ptr(dz), _lib.ptr(ws),
                  _lib.ptr(g), stream)
        g2 = torch.full_like(params, float("nan"))
        got = torch.full((1,), float("nan"), device="cuda")
        _lib.call("ptr_mlp_backward_step", _lib.ptr(X), _lib.ptr(params), _lib.ptr(acts), _lib.ptr(w), R, F, NL, f(0.1), C.c_uint64(seed), _lib.ptr(dz),
                  _lib.ptr(ws), _lib.ptr(g2), KIND[kind], f(h["lr"]), f(h1), f(h2), f(h["eps"]), f(h["weight_decay"]), it, _lib.ptr(s1), _lib.ptr(s2),
                  _lib.ptr(lq), nq, _lib.ptr(got), stream)
        gn = g.cpu().numpy()
        assert np.isfinite(gn).all() and _same(g2, gn), (kind, hs, F, it)
        p, st = optim_ref.step(kind, p, gn, st, it, **h)
        assert _same(params, p), (kind, hs, F, it)
        for k, (dev, ref) in enumerate(zip((s1, s2), st)):
            assert _same(dev, ref), (kind, hs, F, it, optim_ref.RULES[kind][1][k])
        assert torch.equal(got, want)
