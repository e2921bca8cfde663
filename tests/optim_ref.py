"""The flat optimisers' update rule (csrc/ptr_optim.h `opt_update`, `make_opt_step`) restated in numpy float32: ONE rounded operation per line, in
the kernel's order, so that a correctly rounded float32 add / multiply / divide / square root reproduces the device bit for bit (the build keeps
-ffp-contract=off; the device divides with v_div_scale / v_div_fmas / v_div_fixup and refines v_sqrt_f32, both correctly rounded).  The host
scalars use libm's powf through ctypes — the library's own bits, as the C side computes them.

Every function takes float32 arrays `p`, `g` and the state, and the hyper-parameters as Python numbers (rounded to float32 here, as the C ABI's
`float` arguments round them); it returns the new parameter and state arrays and changes nothing in place.
"""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def powf(x, y):
    return f32(_libm.powf(float(f32(x)), float(f32(y))))


def _decayed_grad(p, g, wd):
    t = f32(wd) * p
    return g + t


def adam(p, g, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    lr, b1, b2, eps, one = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(1.0)
    t = powf(b1, step)
    bc1 = one - t
    t = powf(b2, step)
    t = one - t
    bc2_sqrt = np.sqrt(t)
    gi = _decayed_grad(p, g, weight_decay)
    a = b1 * m
    c = one - b1
    c = c * gi
    mi = a + c
    a = b2 * v
    c = one - b2
    c = c * gi
    c = c * gi
    vi = a + c
    d = np.sqrt(vi)
    d = d / bc2_sqrt
    denom = d + eps
    s = lr / bc1
    q = mi / denom
    u = s * q
    return p - u, mi, vi


def adagrad(p, g, acc, step, lr=1e-2, lr_decay=0.0, eps=1e-10, weight_decay=0.0):
    lr, lr_decay, eps, one = f32(lr), f32(lr_decay), f32(eps), f32(1.0)
    t = f32(step - 1) * lr_decay
    t = one + t
    clr = lr / t
    gi = _decayed_grad(p, g, weight_decay)
    c = gi * gi
    si = acc + c
    d = np.sqrt(si)
    d = d + eps
    q = gi / d
    u = clr * q
    return p - u, si


def rmsprop(p, g, sq, step, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0):
    lr, alpha, eps, one = f32(lr), f32(alpha), f32(eps), f32(1.0)
    gi = _decayed_grad(p, g, weight_decay)
    a = alpha * sq
    c = one - alpha
    c = c * gi
    c = c * gi
    si = a + c
    d = np.sqrt(si)
    d = d + eps
    q = gi / d
    u = lr * q
    return p - u, si


# kind -> (update, torch's names of the state buffers in ABI order)
RULES = {"Adam": (adam, ("exp_avg", "exp_avg_sq")), "Adagrad": (adagrad, ("sum",)), "RMS": (rmsprop, ("square_avg",))}


def step(kind, p, g, state, t, **hyper):
    """One step of `kind` on float32 arrays: (new p, new state tuple).  `state`: the buffers in RULES' order; t: the step number from 1."""
    fn, _ = RULES[kind]
    assert p.dtype == g.dtype == f32 and all(s.dtype == f32 for s in state)
    out = fn(p, g, *state, t, **hyper)
    assert all(o.dtype == f32 for o in out)
    return out[0], tuple(out[1:])
