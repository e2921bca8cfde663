"""nn.Linear layers and (Dropout -> Linear -> ReLU)* stacks of the scoring functions on the hand-written fp32-MFMA kernels of
csrc/linear.hip — no library GEMM behind any Linear of a scoring function on the GPU.

Reference: ptranking/base/utils.py:288-356 (get_stacked_FFNet), ptranking/base/list_ranker.py:176-254,303-350 (the listsf head /
tail stacks with ff_dims 128/256/512, the Q|K|V and fc projections).

  `linear(x, weight, bias)`   differentiable y = x W^T + b (forward / backward-input / backward-weight kernels)
  `FusedLinear`               nn.Linear (same parameters, initialisation, state_dict) on `linear`
  `ReluStack`                 nn.Sequential with the reference's module names (dr_i / ff_{i+1} / act_{i+1}) whose forward runs the
                              whole stack as one autograd node: ReLU and the NEXT layer's dropout live in the producing kernel's
                              epilogue (counter-based masks, recomputed in backward, never stored), the backward gates ride in
                              the backward-input kernel's epilogue.
CPU tensors take the plain torch ops (host-logic tests only; the product path is the GPU one).
"""
import ctypes as C
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import dp

NONE, RELU, RELU_DROPOUT = 0, 1, 2


def _rows(x):
    """[..., K] -> contiguous-row 2-D view [R, K] and its leading dimension."""
    x2 = x.reshape(-1, x.shape[-1])
    if x2.dtype != torch.float32:
        x2 = x2.float()
    if x2.stride(-1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < x2.shape[1]):
        x2 = x2.contiguous()
    return x2, (x2.stride(0) if x2.shape[0] > 1 else x2.shape[1])


def _fwd(x2, ldx, weight, bias, act=NONE, p=0.0, seed=0, site=0):
    R, K = x2.shape
    N = weight.shape[0]
    y = torch.empty((R, N), device=x2.device, dtype=torch.float32)
    with torch.cuda.device(x2.device):
        _lib.call("ptr_linear_forward", _lib.ptr(x2), ldx, _lib.ptr(weight), _lib.ptr(bias), R, K, N, act, C.c_float(p), C.c_uint64(seed), site,
                  _lib.ptr(y), N, _lib.current_stream(x2.device))
    return y


def _bwd_input(dy2, weight, gate=None, p=0.0):
    R, N = dy2.shape
    K = weight.shape[1]
    dx = torch.empty((R, K), device=dy2.device, dtype=torch.float32)
    with torch.cuda.device(dy2.device):
        _lib.call("ptr_linear_backward_input", _lib.ptr(dy2), N, _lib.ptr(weight), R, K, N, _lib.ptr(gate), K, C.c_float(p), _lib.ptr(dx), K,
                  _lib.current_stream(dy2.device))
    return dx


def _bwd_weight(x2, ldx, dy2, want_bias, dw_out=None, db_out=None):
    """dW, db; dw_out / db_out: contiguous tensors to write them into (gradient sinks of a flattened stack)."""
    R, K = x2.shape
    N = dy2.shape[1]
    dev = x2.device
    ws = torch.empty(_lib.query("ptr_linear_backward_weight_ws_floats", R, K, N), device=dev, dtype=torch.float32)
    dw = dw_out if dw_out is not None else torch.empty((N, K), device=dev, dtype=torch.float32)
    db = (db_out if db_out is not None else torch.empty(N, device=dev, dtype=torch.float32)) if want_bias else None
    with torch.cuda.device(dev):
        _lib.call("ptr_linear_backward_weight", _lib.ptr(x2), ldx, _lib.ptr(dy2), N, R, K, N, _lib.ptr(ws), _lib.ptr(dw), _lib.ptr(db),
                  _lib.current_stream(dev))
    return dw, db


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        x2, ldx = _rows(x)
        w = weight.contiguous()
        y = _fwd(x2, ldx, w, bias)
        ctx.save_for_backward(x2, w)
        ctx.ldx, ctx.has_bias = ldx, bias is not None
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        dx = _bwd_input(dy2, w).view(*dy.shape[:-1], w.shape[1]) if ctx.needs_input_grad[0] else None
        dw, db = _bwd_weight(x2, ctx.ldx, dy2, ctx.has_bias)
        return dx, dw, db


def linear(x, weight, bias=None):
    """nn.functional.linear on the hand-written GEMM kernels for GPU tensors.

    CPU tensors: FusedLinear IS an nn.Linear and FusedStack IS an nn.Sequential, and on a CPU tensor they behave as those torch modules do
    (torch's own F.linear — not the oracle, not a re-implementation of ours).  That is what lets the host-side plumbing the drop-in reuses
    from the reference run where no GPU is (state_dict round trips, the reference's kfold_cv_eval loop on the installed classes in
    tests/test_host_cpu.py, golden-fixture generation).  It is NOT a fallback for the product path: a GPU tensor never takes it, the device
    entry points of _lib refuse CPU tensors, and this branch is an ERROR by default too (r5: strict is the default); the CPU
    tests that exercise the host plumbing opt out with PTR_STRICT_DEVICE=0 (tests/conftest.py sets it for the `not gpu` suite and for the `gpu` test modules that declare CPU_REFERENCE_MODULES)."""
    if not x.is_cuda:
        if os.environ.get("PTR_STRICT_DEVICE", "1") != "0":
            raise _lib.NativeLibraryError(f"linear: tensor on {x.device} — the hand-written kernels run on the GPU only "
                                          f"(PTR_STRICT_DEVICE=0 lets FusedLinear / FusedStack behave as the torch modules they are, for CPU-side tests)")
        return F.linear(x, weight, bias)
    return _LinearFn.apply(x, weight, bias)


class FusedLinear(nn.Linear):
    def forward(self, x):
        return linear(x, self.weight, self.bias)


class _ReluStackFn(torch.autograd.Function):
    """x -> dropout -> (Linear -> ReLU -> dropout)* -> Linear -> ReLU -> Linear [-> ReLU]   (utils.py:296-322 with AF='R', no BN)."""

    @staticmethod
    def forward(ctx, x, p, seed, tail_relu, *params):
        n = len(params) // 2                       # Linear layers; n - 1 of them hidden
        ws, bs = params[0::2], params[1::2]
        x2, ldx = _rows(x)
        dev = x2.device
        R, K0 = x2.shape
        if n > 1 and p > 0.0:
            if K0 % 4 or ldx % 4:
                x2, ldx = x2.contiguous(), K0
                if K0 % 4:
                    raise NotImplementedError("input width must be a multiple of 4 for the fused dropout")
            a = torch.empty((R, K0), device=dev, dtype=torch.float32)
            with torch.cuda.device(dev):
                _lib.call("ptr_dropout_apply", _lib.ptr(x2), ldx, R, K0, C.c_float(p), C.c_uint64(seed), 0, _lib.ptr(a), K0, _lib.current_stream(dev))
            acts, lda = [a], K0
        else:
            acts, lda = [x2], ldx
        for i in range(n - 1):                     # hidden layers: ReLU, and the dropout in front of the next hidden Linear
            last_hidden = i == n - 2
            a = _fwd(acts[-1], lda if i == 0 else acts[-1].shape[1], ws[i], bs[i], RELU if (last_hidden or p == 0.0) else RELU_DROPOUT, p, seed, i + 1)
            acts.append(a)
        out = _fwd(acts[-1], lda if n == 1 else acts[-1].shape[1], ws[-1], bs[-1], RELU if tail_relu else NONE)
        ctx.save_for_backward(out if tail_relu else None, *acts, *ws)
        ctx.meta = (n, p, seed, tail_relu, lda, [b is not None for b in bs])
        return out.view(*x.shape[:-1], ws[-1].shape[0])

    @staticmethod
    def backward(ctx, dout):
        n, p, seed, tail_relu, lda, has_b = ctx.meta
        saved = ctx.saved_tensors
        out, acts, ws = saved[0], saved[1:1 + n], saved[1 + n:]
        dev = dout.device
        dz = dout.reshape(-1, dout.shape[-1]).contiguous()
        if tail_relu:
            g = torch.empty_like(dz)
            with torch.cuda.device(dev):
                _lib.call("ptr_relu_gate", _lib.ptr(dz), _lib.ptr(out), C.c_int64(dz.numel()), _lib.ptr(g), _lib.current_stream(dev))
            dz = g
        grads = [None] * (2 * n)
        for i in range(n - 1, -1, -1):
            a_in = acts[i]
            dw, db = _bwd_weight(a_in, lda if i == 0 else a_in.shape[1], dz, has_b[i])
            grads[2 * i], grads[2 * i + 1] = dw, db
            if i > 0:                               # gate by the stored ReLU (+ dropout) output of the layer below
                dropped = p > 0.0 and i < n - 1     # acts[i] carries dropout unless it feeds the last Linear
                dz = _bwd_input(dz, ws[i], gate=a_in, p=p if dropped else 0.0)
            elif ctx.needs_input_grad[0]:
                dx = _bwd_input(dz, ws[0])
                if n > 1 and p > 0.0:
                    dxd = torch.empty_like(dx)
                    with torch.cuda.device(dev):
                        _lib.call("ptr_dropout_apply", _lib.ptr(dx), dx.shape[1], dx.shape[0], dx.shape[1], C.c_float(p), C.c_uint64(seed), 0,
                                  _lib.ptr(dxd), dx.shape[1], _lib.current_stream(dev))
                    dx = dxd
                return (dx.view(*dout.shape[:-1], ws[0].shape[1]), None, None, None, *grads)
        return (None, None, None, None, *grads)


AF_CODE = {nn.ReLU: 1, nn.LeakyReLU: 2, nn.ELU: 3, nn.CELU: 3, nn.SELU: 4, nn.GELU: 5, nn.Sigmoid: 6, nn.Tanh: 7}   # PTR_AF_*
BN_EPS = 1e-5            # nn.BatchNorm1d's default, what LTRBatchNorm builds (utils.py:214)


def _af_code(m):
    code = AF_CODE.get(type(m))
    if code is None:
        return None
    if isinstance(m, nn.LeakyReLU) and m.negative_slope != 0.01:
        return None
    if isinstance(m, (nn.ELU, nn.CELU)) and m.alpha != 1.0:
        return None
    if isinstance(m, nn.GELU) and getattr(m, "approximate", "none") != "none":
        return None
    return code


def _bn_stats(z, group=0, lens=None, L=0):
    """lens / L: padded query batches — int32 [B] real lengths and the padded list length; only real rows enter the statistics."""
    R, N = z.shape
    dev = z.device
    G = R // group if group else 1
    ws = torch.empty(_lib.query("ptr_bn_ws_floats", R, N, group), device=dev, dtype=torch.float32)
    mean = torch.empty(G * N, device=dev, dtype=torch.float32)
    rstd = torch.empty(G * N, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.call("ptr_bn_stats", _lib.ptr(z), N, R, N, group, _lib.ptr(lens), L, C.c_float(BN_EPS), _lib.ptr(ws), _lib.ptr(mean), _lib.ptr(rstd),
                  _lib.current_stream(dev))
    return mean, rstd


def _bnact_fwd(z, group, mean, rstd, gamma, beta, af, p, seed, site, lens=None, L=0):
    R, N = z.shape
    out = torch.empty_like(z)
    with torch.cuda.device(z.device):
        _lib.call("ptr_bnact_forward", _lib.ptr(z), N, R, N, group, _lib.ptr(lens), L, _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma), _lib.ptr(beta),
                  af, C.c_float(p), C.c_uint64(seed), site, _lib.ptr(out), _lib.current_stream(z.device))
    return out


def _bnact_bwd(z, da, group, mean, rstd, gamma, beta, af, p, seed, site, dg_out=None, db_out=None, lens=None, L=0):
    R, N = z.shape
    dev = z.device
    has_bn = mean is not None
    ws = torch.empty(_lib.query("ptr_bn_ws_floats", R, N, group), device=dev, dtype=torch.float32) if has_bn else None
    dz = torch.empty_like(z)
    dg = (dg_out if dg_out is not None else torch.empty(N, device=dev, dtype=torch.float32)) if (has_bn and gamma is not None) else None
    db = (db_out if db_out is not None else torch.empty(N, device=dev, dtype=torch.float32)) if (has_bn and beta is not None) else None
    with torch.cuda.device(dev):
        _lib.call("ptr_bnact_backward", _lib.ptr(z), _lib.ptr(da), N, R, N, group, _lib.ptr(lens), L, _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma),
                  _lib.ptr(beta), af, C.c_float(p), C.c_uint64(seed), site, _lib.ptr(ws), _lib.ptr(dz), _lib.ptr(dg), _lib.ptr(db),
                  _lib.current_stream(dev))
    return dz, dg, db


def _bn_stats_sync(z, lens=None, L=0):
    """Whole-batch statistics over the documents of ALL data-parallel ranks: this rank's (mean, M2, count) slot -> gathered slots of every
    rank (one collective, dp.gather_slots) -> the rank-order combination, run by every rank on identical bytes.  Returns mean, rstd and the
    global document count [1], which stays on the device for the backward."""
    R, N = z.shape
    dev = z.device
    S = _lib.query("ptr_bn_slot_floats", N)
    slots, own = dp.new_slots(S, dev)
    ws = torch.empty(_lib.query("ptr_bn_ws_floats", R, N, 0), device=dev, dtype=torch.float32)
    mean = torch.empty(N, device=dev, dtype=torch.float32)
    rstd = torch.empty(N, device=dev, dtype=torch.float32)
    cnt = torch.empty(1, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.call("ptr_bn_stats_partial", _lib.ptr(z), N, R, N, 0, _lib.ptr(lens), L, _lib.ptr(ws), _lib.ptr(own), _lib.current_stream(dev))
        dp.gather_slots(slots)
        _lib.call("ptr_bn_stats_combine", _lib.ptr(slots), slots.shape[0], S, N, C.c_float(BN_EPS), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(cnt),
                  _lib.current_stream(dev))
    return mean, rstd, cnt


def _bnact_bwd_sync(z, da, mean, rstd, cnt, gamma, beta, af, p, seed, site, dg_out=None, db_out=None, lens=None, L=0):
    """The backward of a layer normalised with synchronised statistics: local column sums (with the global mean / rstd) -> gathered sums
    of every rank (one collective) -> their fixed-order total and dz.  dgamma / dbeta are the LOCAL sums: the gradient all-reduce adds
    them across ranks like every other parameter gradient (the global sums would be counted once per rank)."""
    R, N = z.shape
    dev = z.device
    sums, own = dp.new_slots(2 * N, dev)
    ws = torch.empty(_lib.query("ptr_bn_ws_floats", R, N, 0), device=dev, dtype=torch.float32)
    dz = torch.empty_like(z)
    with torch.cuda.device(dev):
        st = _lib.current_stream(dev)
        _lib.call("ptr_bnact_backward_sums", _lib.ptr(z), _lib.ptr(da), N, R, N, 0, _lib.ptr(lens), L, _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma),
                  _lib.ptr(beta), af, C.c_float(p), C.c_uint64(seed), site, _lib.ptr(ws), _lib.ptr(own), st)
        db = dg = None
        if beta is not None:
            db = own[:N].clone() if db_out is None else db_out.copy_(own[:N].view_as(db_out))
        if gamma is not None:
            dg = own[N:].clone() if dg_out is None else dg_out.copy_(own[N:].view_as(dg_out))
        dp.gather_slots(sums)
        _lib.call("ptr_bnact_backward_apply", _lib.ptr(z), _lib.ptr(da), N, R, N, 0, _lib.ptr(lens), L, _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma),
                  _lib.ptr(beta), af, C.c_float(p), C.c_uint64(seed), site, _lib.ptr(sums), sums.shape[0], _lib.ptr(cnt), _lib.ptr(ws), _lib.ptr(dz), st)
    return dz, dg, db


def _stack_forward(x, p, seed, spec, params, fixed_stats=None, sink=None, lens=None, L=0, sync=False):
    """Forward of the general stack.  spec = (n_linear, hidden af codes, tail af or 0, has_bn, group): group = 0 — statistics over the
    whole batch ('BN'), L — per query ('BN2').  fixed_stats: per-layer (mean, rstd) to use instead of the batch statistics (BN2 under
    torch.no_grad(): its moving statistics).  sink: list receiving (layer, mean, rstd) of the statistics computed here.  sync ('BN' under data parallelism,
    FusedStack.sync_batch_norm): the statistics of every layer are those of the documents of ALL ranks; the 6th result then holds each
    layer's global document count (a device scalar the backward divides by), else None."""
    n, afs, tail_af, has_bn, group = spec
    per = 4 if has_bn else 2
    x2, ldx = _rows(x)
    dev = x2.device
    R, K0 = x2.shape
    if n > 1 and p > 0.0:
        if K0 % 4 or ldx % 4:
            raise NotImplementedError("input width must be a multiple of 4 for the fused dropout")
        a = torch.empty((R, K0), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.call("ptr_dropout_apply", _lib.ptr(x2), ldx, R, K0, C.c_float(p), C.c_uint64(seed), 0, _lib.ptr(a), K0, _lib.current_stream(dev))
        ins, lda = [a], K0
    else:
        ins, lda = [x2], ldx
    zs, stats, cnts = [], [], []
    out = None
    for i in range(n):
        W, b = params[per * i], params[per * i + 1]
        gamma, beta = (params[per * i + 2], params[per * i + 3]) if has_bn else (None, None)
        z = _fwd(ins[-1], lda if i == 0 else ins[-1].shape[1], W, b)
        hidden = i < n - 1
        af = afs[i] if hidden else tail_af
        if not hidden and af == 0:
            out = z
            zs.append(None); stats.append((None, None)); cnts.append(None)
            break
        gi = group
        cnt = None
        if not has_bn:
            mean, rstd = None, None
        elif sync:
            mean, rstd, cnt = _bn_stats_sync(z, lens, L)
        elif fixed_stats is not None:
            (mean, rstd), gi = fixed_stats[i], 0
        else:
            mean, rstd = _bn_stats(z, group, lens, L)
            if sink is not None:
                sink.append((i, mean, rstd))
        pd = p if (hidden and i < n - 2) else 0.0          # the dropout in front of the NEXT hidden Linear
        a = _bnact_fwd(z, gi, mean, rstd, gamma, beta, af, pd, seed, i + 1, lens, L)
        zs.append(z); stats.append((mean, rstd)); cnts.append(cnt)
        if hidden:
            ins.append(a)
        else:
            out = a
    return out, ins, zs, stats, lda, (cnts if sync else None)


class _StackFn(torch.autograd.Function):
    """The general stack of get_stacked_FFNet (utils.py:288-356): [Dropout -> Linear -> [BN] -> AF]* -> Linear [-> [BN] -> TL_AF], layer by
    layer on our kernels: linear -> column statistics -> (normalise, activate, next layer's dropout).  Only the pre-normalisation z
    and the layer inputs are kept for backward."""

    @staticmethod
    def forward(ctx, x, p, seed, spec, sink, gsinks, lens, sync, *params):
        L = x.shape[-2] if (lens is not None and x.dim() == 3) else 0
        out, ins, zs, stats, lda, ctx.sync_counts = _stack_forward(x, p, seed, spec, params, sink=sink, lens=lens, L=L, sync=sync)
        flat_stats = [t for ms in stats for t in ms]
        ctx.save_for_backward(*ins, *zs, *flat_stats, *params)
        ctx.meta = (spec[0], p, seed, spec, lda)
        ctx.lens, ctx.L = lens, L
        ctx.gsinks = gsinks            # per parameter: the tensor its gradient is WRITTEN into (flattened stack), or None
        return out.view(*x.shape[:-1], out.shape[1])

    @staticmethod
    def backward(ctx, dout):
        n, p, seed, spec, lda = ctx.meta
        _, afs, tail_af, has_bn, group = spec
        per = 4 if has_bn else 2
        sv = ctx.saved_tensors
        ins, zs, fs, params = sv[:n], sv[n:2 * n], sv[2 * n:4 * n], sv[4 * n:]
        dev = dout.device
        d = dout.reshape(-1, dout.shape[-1]).contiguous()
        grads = [None] * len(params)
        gs = ctx.gsinks() if ctx.gsinks is not None else None      # claimed once per zero_grad(): a second backward accumulates
        if gs is None:
            gs = [None] * len(params)
        ret = lambda g, k: None if gs[k] is not None else g        # sunk gradients are not handed to autograd
        for i in range(n - 1, -1, -1):
            W = params[per * i]
            gamma, beta = (params[per * i + 2], params[per * i + 3]) if has_bn else (None, None)
            hidden = i < n - 1
            af = afs[i] if hidden else tail_af
            if hidden or af != 0:
                pd = p if (hidden and i < n - 2) else 0.0
                if ctx.sync_counts is not None:    # synchronised statistics: one collective per layer here too, on every rank alike
                    d, dg, dbt = _bnact_bwd_sync(zs[i], d, fs[2 * i], fs[2 * i + 1], ctx.sync_counts[i], gamma, beta, af, pd, seed, i + 1,
                                                 gs[per * i + 2], gs[per * i + 3], ctx.lens, ctx.L)
                else:
                    d, dg, dbt = _bnact_bwd(zs[i], d, group, fs[2 * i], fs[2 * i + 1], gamma, beta, af, pd, seed, i + 1,
                                            gs[per * i + 2] if has_bn else None, gs[per * i + 3] if has_bn else None, ctx.lens, ctx.L)
                if has_bn:
                    grads[per * i + 2], grads[per * i + 3] = ret(dg, per * i + 2), ret(dbt, per * i + 3)
            a_in = ins[i]
            dw, db = _bwd_weight(a_in, lda if i == 0 else a_in.shape[1], d, params[per * i + 1] is not None, gs[per * i], gs[per * i + 1])
            grads[per * i], grads[per * i + 1] = ret(dw, per * i), ret(db, per * i + 1)
            if i > 0:
                d = _bwd_input(d, W)
            elif ctx.needs_input_grad[0]:
                dx = _bwd_input(d, W)
                if n > 1 and p > 0.0:
                    dxd = torch.empty_like(dx)
                    with torch.cuda.device(dev):
                        _lib.call("ptr_dropout_apply", _lib.ptr(dx), dx.shape[1], dx.shape[0], dx.shape[1], C.c_float(p), C.c_uint64(seed), 0,
                                  _lib.ptr(dxd), dx.shape[1], _lib.current_stream(dev))
                    dx = dxd
                return (dx.view(*dout.shape[:-1], W.shape[1]), None, None, None, None, None, None, None, *grads)
        return (None, None, None, None, None, None, None, None, *grads)


class FusedStack(nn.Sequential):
    """The Sequential get_stacked_FFNet builds (module names and state_dict as the reference's: dr_i / ff_{i+1} / bn_{i+1} / act_{i+1}),
    evaluated on the GPU as ONE autograd node on the hand-written kernels:
      * AF='R' without batch norm: ReLU and the next layer's dropout in the producing GEMM's epilogue (`_ReluStackFn`);
      * any other working activation of get_AF and / or batch norm — bn_type='BN' (statistics over all documents of the batch; the
        reference's DEFAULT pointsf: 5 x [BN(affine) -> GELU], Sigmoid tail) or 'BN2' (per-query statistics, moving statistics under
        torch.no_grad(), LTRBatchNorm2's quirks): layer-wise linear -> statistics -> normalise / activate / dropout (`_StackFn`).
    A structure it does not recognise (RReLU, ...) runs module by module (FusedLinear GEMMs + torch elementwise)."""

    tail_relu = False        # kept for the pure-ReLU fast path
    _plan = None
    _flat = None             # (flat parameter buffer, flat gradient buffer) once flatten_parameters() has re-homed the parameters
    _grads_fresh = False     # set by the owning optimiser's zero_grad(): the next backward may WRITE the gradients (no accumulation)
    batch_lens = None        # padded query batch: int32 [B] real list lengths, set by the ranker around forward (host.scorer_lens)
    sync_batch_norm = False  # 'BN' statistics over the documents of ALL data-parallel ranks in training (dp.sync_batch_norm switches it)

    def _sync_wanted(self):
        """Synchronised statistics apply: switched on, training mode with gradients (evaluation and torch.no_grad() scoring keep
        rank-local statistics — ranks need not make the same number of forward calls there), under data parallelism."""
        return self.sync_batch_norm and self.training and torch.is_grad_enabled() and dp.is_distributed()

    def _refuse_unsynced(self, reason):
        """The module-by-module route would normalise a 'BN' layer with this rank's own statistics: an error while the switch is on."""
        if self._sync_wanted() and any(type(c).__name__ in ("_BatchNormOverDocs", "LTRBatchNorm") for c in self.children()):
            raise NotImplementedError(f"sync_batch_norm is on under data parallelism, but this batch-norm stack runs module by module ({reason}): "
                                      f"its 'BN' layers would use rank-local statistics")

    def handles_padding(self, x):
        """True when a padded batch (batch_lens) is scored exactly like the unpadded lists on this input: the fused GPU path masks the
        padded rows out of the batch-norm statistics; the module-by-module fallbacks (CPU tensors, unrecognised structures) do not."""
        if not x.is_cuda:
            return False
        if self._plan is None:
            self._plan = self._make_plan() or False
        plan = self._plan
        if plan is False:
            return False
        if plan["kind"] is None:
            return True                                   # no batch norm: rows are independent
        if x.dim() != 3:
            return False
        p = plan["p"] if self.training else 0.0
        return not (p > 0.0 and len(plan["lins"]) > 1 and x.shape[-1] % 4)

    def flatten_parameters(self):
        """Re-home every parameter in ONE flat fp32 buffer and its gradient in one flat gradient buffer (parameters and `.grad`s
        become views; names, shapes and state_dict are unchanged): one optimiser kernel and one all-reduce for the whole stack, and
        the general stack's backward writes dW / db / dgamma / dbeta straight into the gradient buffer.  Call after .cuda()."""
        if self._flat is not None:
            return self._flat
        ps = list(self.parameters())
        dev = ps[0].device
        sizes = [(p.numel() + 3) // 4 * 4 for p in ps]                 # 16-byte aligned slices (float4 kernels)
        flat = torch.zeros(sum(sizes), device=dev, dtype=torch.float32)
        self._gbuf = torch.zeros(sum(sizes) + 4, device=dev, dtype=torch.float32)    # 4 spare floats: scalars that ride in the DP all-reduce
        gflat = self._gbuf[:sum(sizes)]
        off = 0
        with torch.no_grad():
            for p, sz in zip(ps, sizes):
                n = p.numel()
                flat[off:off + n].copy_(p.data.reshape(-1))
                p.data = flat[off:off + n].view(p.shape)
                p.grad = gflat[off:off + n].view(p.shape)
                off += sz
        self._flat = (flat, gflat)
        return self._flat

    def reattach_grads(self):
        """Every parameter's .grad must alias its slice of the flat gradient buffer (what FlatViewAdam steps on).  module.zero_grad(),
        a foreign optimiser's zero_grad(set_to_none=True) or a gradient bucket re-point it: a gradient found elsewhere is moved into
        its slice (the slice was zeroed by the last zero_grad), a missing one leaves the zeroed slice.  Returns how many were re-homed."""
        if self._flat is None:
            return 0
        gflat = self._flat[1]
        slots = self.__dict__.get("_grad_slots")
        if slots is None:                       # (parameter, offset, expected address of its gradient slice): built once
            slots, off, base = [], 0, gflat.data_ptr()
            for p in self.parameters():
                slots.append((p, off, base + 4 * off))
                off += (p.numel() + 3) // 4 * 4
            self.__dict__["_grad_slots"] = slots
        moved = 0
        for p, off, addr in slots:              # the per-step cost is one data_ptr() compare per parameter (no tensor views)
            g = p.grad
            if g is None or g.data_ptr() != addr:
                view = gflat[off:off + p.numel()].view(p.shape)
                if g is not None:
                    view.copy_(g)
                p.grad = view
                moved += 1
        return moved

    def _claim_sinks(self, params):
        """Gradient sinks for one backward: each leaf parameter's `.grad` view, handed out only for the FIRST backward after the
        optimiser's zero_grad() (a second backward before the next zero_grad accumulates through autograd as usual)."""
        if self._flat is None:
            return None

        def claim():
            if not self._grads_fresh:
                return None
            self._grads_fresh = False
            return [p.grad if (isinstance(p, nn.Parameter) and p.grad is not None and p.grad.is_contiguous()) else None for p in params]
        return claim

    def _make_plan(self):
        mods = list(self)
        lins, drops = [], []
        cur = None
        for m in mods:
            if isinstance(m, nn.Dropout):
                drops.append(m)
            elif isinstance(m, nn.Linear):
                cur = {"lin": m, "bn": None, "bn2": None, "af": 0}
                lins.append(cur)
            elif type(m).__name__ in ("_BatchNormOverDocs", "LTRBatchNorm"):
                if cur is None or cur["bn"] is not None or cur["bn2"] is not None or cur["af"] != 0:
                    return None
                cur["bn"] = m.bn
            elif type(m).__name__ in ("_BatchNormPerQuery", "LTRBatchNorm2"):
                if cur is None or cur["bn"] is not None or cur["bn2"] is not None or cur["af"] != 0:
                    return None
                cur["bn2"] = m
            elif _af_code(m) is not None:
                if cur is None or cur["af"] != 0:
                    return None
                cur["af"] = _af_code(m)
            else:
                return None
        if not lins or any(l["af"] == 0 for l in lins[:-1]):
            return None
        kinds = {("bn" if l["bn"] is not None else "bn2" if l["bn2"] is not None else None) for l in lins[:-1]}
        if lins[-1]["af"] != 0:
            kinds.add("bn" if lins[-1]["bn"] is not None else "bn2" if lins[-1]["bn2"] is not None else None)
        elif lins[-1]["bn"] is not None or lins[-1]["bn2"] is not None:
            return None
        if len(lins) == 1 and lins[0]["af"] == 0:
            kinds = {None}
        if len(kinds) != 1:
            return None                                 # batch norm on some layers only, or mixed kinds: not the reference's constructions
        kind = kinds.pop()
        if kind == "bn" and any(l["bn"] is not None and (l["bn"].track_running_stats or l["bn"].eps != BN_EPS) for l in lins):
            return None
        if len(drops) not in (0, len(lins) - 1) or len({d.p for d in drops}) > 1:
            return None
        relu_only = kind is None and all(l["af"] == 1 for l in lins[:-1]) and lins[-1]["af"] in (0, 1)
        return dict(lins=lins, kind=kind, relu_only=relu_only, p=drops[0].p if drops else 0.0)

    def forward(self, x):
        if not x.is_cuda:
            self._refuse_unsynced(f"tensor on {x.device}")
            return super().forward(x)
        if self._plan is None:
            self._plan = self._make_plan() or False
        plan = self._plan
        if plan is False or (plan["kind"] == "bn2" and x.dim() != 3):
            self._refuse_unsynced("a structure the fused stack does not recognise")
            return super().forward(x)
        lins = plan["lins"]
        p = plan["p"] if self.training else 0.0
        if p > 0.0 and len(lins) > 1 and x.shape[-1] % 4:
            # the fused input dropout works on float4 feature groups: other widths (46-feature MQ2007/2008 data in front of a listsf
            # head / tail stack or a GELU pointsf) run module by module — FusedLinear GEMMs take any K, nn.Dropout / torch activations
            if getattr(self, "batch_lens", None) is not None and plan["kind"] is not None:
                raise NotImplementedError("a padded batch (batch_lens) reached a batch-norm stack on its module-by-module path: the padded "
                                          "rows would enter the BN statistics (host.scorer_lens should have refused this configuration)")
            self._refuse_unsynced(f"input width {x.shape[-1]} is not a multiple of 4 and the stack has dropout")
            return super().forward(x)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0.0 else 0      # CPU generator: no device sync
        if p > 0.0:
            seed = dp.local_dropout_seed(seed, x.numel() // x.shape[-1])           # data-parallel replicas draw the masks of THEIR global rows
        self.last_seed = seed
        if plan["relu_only"]:
            params = []
            for l in lins:
                params += [l["lin"].weight, l["lin"].bias]
            return _ReluStackFn.apply(x, float(p), seed, lins[-1]["af"] == 1, *params)
        kind = plan["kind"]
        params = []
        for l in lins:
            params += [l["lin"].weight, l["lin"].bias]
            if kind == "bn":
                bn = l["bn"]
                params += [bn.weight if bn is not None else None, bn.bias if bn is not None else None]
            elif kind == "bn2":
                m = l["bn2"]                      # LTRBatchNorm2 (utils.py:266-284): y = (gamma * xhat + beta) [* weight + bias] — folded into one
                if m is None:                     # effective scale / shift per feature by tiny autograd-tracked vector ops
                    params += [None, None]
                else:
                    N = l["lin"].weight.shape[0]
                    g, b = m.gamma.reshape(N), m.beta.reshape(N)
                    if m.affine:
                        g, b = g * m.weight.reshape(N), b * m.weight.reshape(N) + m.bias.reshape(N)
                    params += [g, b]
        has_bn = kind is not None
        group = x.shape[-2] if kind == "bn2" else 0
        spec = (len(lins), tuple(l["af"] for l in lins[:-1]), lins[-1]["af"], has_bn, group)
        if kind == "bn2" and not torch.is_grad_enabled():
            # prediction mode of ltr_batch_norm (utils.py:229-231): the moving statistics instead of the query's own
            fixed = []
            for l in lins:
                m = l["bn2"]
                if m is None:
                    fixed.append((None, None))
                else:
                    N = l["lin"].weight.shape[0]
                    fixed.append((m.moving_mean.to(x.device).reshape(N).contiguous(),
                                  torch.rsqrt(m.moving_var.to(x.device).reshape(N) + BN_EPS).contiguous()))
            out = _stack_forward(x, float(p), seed, spec, [t.detach() if t is not None else None for t in params], fixed_stats=fixed)[0]
            return out.view(*x.shape[:-1], out.shape[1])
        sink = [] if kind == "bn2" else None
        lens = self.batch_lens if (has_bn and x.dim() == 3) else None       # padded batch: real rows only in the statistics
        if lens is not None and not (lens.is_cuda and lens.dtype == torch.int32 and lens.is_contiguous() and lens.shape == (x.shape[0],)):
            raise ValueError("batch_lens must be a contiguous CUDA int32 tensor [B]")
        sync = kind == "bn" and self._sync_wanted()
        out = _StackFn.apply(x, float(p), seed, spec, sink, self._claim_sinks(params), lens, sync, *params)
        if sink:                                   # moving statistics, averaged over the queries of the batch (utils.py:242-245)
            with torch.no_grad():
                for i, mean, rstd in sink:
                    m = lins[i]["bn2"]
                    N = lins[i]["lin"].weight.shape[0]
                    mq = mean.view(-1, N)
                    vq = 1.0 / (rstd.view(-1, N) ** 2) - BN_EPS
                    mom = m.momentum
                    m.moving_mean = ((1.0 - mom) * m.moving_mean.to(x.device).reshape(1, N) + mom * mq).mean(dim=0).reshape(1, 1, N)
                    m.moving_var = ((1.0 - mom) * m.moving_var.to(x.device).reshape(1, N) + mom * vq).mean(dim=0).reshape(1, 1, N)
        return out


ReluStack = FusedStack
