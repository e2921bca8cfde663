// The flat optimisers of the pointsf scorer: the deterministic reduction of the backward's per-block partial gradients with the optimiser step,
// the loss-slot sum and the weight-image refresh as its tail, and the stand-alone step entry points.  The update rule itself is ptr_optim.h's.
//
// Reference: ptranking/base/ranker.py:512-525 (Adam / Adagrad / RMSprop with weight_decay 1e-3), :589-603 (backward -> optimizer.step).
#include "ptr_mlp.h"
#include "ptr_optim.h"

namespace ptr {

// grad[i] = sum_b ws[b][i], fixed order.  A 1024-thread workgroup owns 128 consecutive i, every lane two of them (i and i + 64): wave w sums
// the partials b = w, w+16, ... of both (4 independent accumulators each: 8 loads in flight), then waves 0 / 1 add the 16 wave totals of the
// first / second 64 elements in order — per element the additions of the one-element-per-lane form this replaces, bit for bit.  Two elements per
// lane halve the grid: (n + 127) / 128 (+ 1) workgroups — 267 at 34 001 parameters — are resident at once on 256 CUs x 2 workgroups, where
// the 533 of the 64-element form ran a second, nearly empty round of the whole chain partials -> barrier -> optimiser state -> stores.
// Entries i >= tail_begin (d w_out, d b_out: written by the dZ kernel's smaller grid) only have nblk_tail partials.
constexpr int kRedElems = 128;               // elements per workgroup of reduce_partials_kernel
inline unsigned reduce_grid(size_t n, bool loss_block) { return (unsigned)((n + kRedElems - 1) / kRedElems) + (loss_block ? 1u : 0u); }
__global__ void __launch_bounds__(1024)
reduce_partials_kernel(const float *__restrict__ ws, int nblk, int nblk_tail, size_t tail_begin, size_t stride, size_t n,
                       float *__restrict__ grad, OptStep o) {
    __shared__ float part[16][kRedElems];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (o.loss_out && blockIdx.x == gridDim.x - 1) {
        // one extra block: the loss slots of the batch, summed by the function sum_f32_kernel calls (ptr_device.h block1024_sum): the fused
        // step returns the same bits as the separate call
        const float tot = block1024_sum(o.loss_q, o.nq, &part[0][0]);
        if (threadIdx.x == 0) o.loss_out[0] = tot;
        return;
    }
    // the two elements of this lane (clamped to n - 1 past the end: loaded, never stored)
    const size_t ia = (size_t)blockIdx.x * kRedElems + lane, ib = ia + 64;
    const size_t ica = ia < n ? ia : n - 1, icb = ib < n ? ib : n - 1;
    const int nba = ica >= tail_begin ? nblk_tail : nblk, nbb = icb >= tail_begin ? nblk_tail : nblk;
    const int nbc = nba < nbb ? nba : nbb;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    int b = w;
    for (; b + 48 < nbc; b += 64) {              // both elements: 8 independent loads
        a0 += ws[(size_t)b * stride + ica];
        a1 += ws[(size_t)(b + 16) * stride + ica];
        a2 += ws[(size_t)(b + 32) * stride + ica];
        a3 += ws[(size_t)(b + 48) * stride + ica];
        b0 += ws[(size_t)b * stride + icb];
        b1 += ws[(size_t)(b + 16) * stride + icb];
        b2 += ws[(size_t)(b + 32) * stride + icb];
        b3 += ws[(size_t)(b + 48) * stride + icb];
    }
    // what is left of either element, in the same order.  The two 4-accumulator loops run no iteration unless the elements' counts differ: only
    // in the ONE workgroup that straddles tail_begin, and only on the layer-wise path (every other caller passes tail_begin = n)
    int ba = b, bb = b;
    for (; ba + 48 < nba; ba += 64) {
        a0 += ws[(size_t)ba * stride + ica];
        a1 += ws[(size_t)(ba + 16) * stride + ica];
        a2 += ws[(size_t)(ba + 32) * stride + ica];
        a3 += ws[(size_t)(ba + 48) * stride + ica];
    }
    for (; bb + 48 < nbb; bb += 64) {
        b0 += ws[(size_t)bb * stride + icb];
        b1 += ws[(size_t)(bb + 16) * stride + icb];
        b2 += ws[(size_t)(bb + 32) * stride + icb];
        b3 += ws[(size_t)(bb + 48) * stride + icb];
    }
    for (; ba < nba; ba += 16) a0 += ws[(size_t)ba * stride + ica];
    for (; bb < nbb; bb += 16) b0 += ws[(size_t)bb * stride + icb];
    part[w][lane] = (a0 + a1) + (a2 + a3);
    part[w][64 + lane] = (b0 + b1) + (b2 + b3);
    __syncthreads();
    const int col = 64 * w + lane;                                  // waves 0 / 1: the first / second 64 elements
    const size_t i = (size_t)blockIdx.x * kRedElems + col;
    if (w < 2 && i < n) {
        float s = part[0][col];
#pragma unroll
        for (int k = 1; k < 16; ++k) s += part[k][col];
        if (grad) grad[i] = s;                          // (ptr_opt_step_loss: ws IS the gradient, one "partial" — nothing to write back)
        if (o.kind) {                                   // fused optimiser step on the element just reduced
            const float pn = opt_update(o, i, s);
            if (o.wimg) x6_img_put(o.wimg, o.F, o.NL, i, pn);
        }
    }
}

int launch_reduce_partials(const float *ws, int nblk, int nblk_tail, size_t tail_begin, size_t stride, size_t n, float *grad, const OptStep &o,
                           hipStream_t st, const char *who) {
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(reduce_grid(n, o.loss_out != nullptr)), dim3(1024), 0, st, ws, nblk, nblk_tail, tail_begin,
                       stride, n, grad, o);
    return check_hip(hipGetLastError(), who);
}

// The step on a gradient that is already complete, one element per thread
__global__ void __launch_bounds__(256)
opt_step_kernel(const float *__restrict__ grad, size_t n, OptStep o) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) opt_update(o, i, grad[i]);
}

// ptr_adam_step / ptr_adagrad_step / ptr_rmsprop_step
static int opt_step_alone(const char *who, int opt_kind, float *param, const float *grad, float *state1, float *state2, int64_t n, float lr, float hyper1,
                          float hyper2, float eps, float weight_decay, int step, void *stream) {
    if (n < 0 || (n > 0 && (!param || !grad))) { set_error("%s: bad arguments", who); return PTR_ERR_INVALID_ARG; }
    OptStep o;
    if (int rc = make_opt_step(o, who, opt_kind, lr, hyper1, hyper2, eps, weight_decay, step, param, state1, state2, n > 0, nullptr, 0, nullptr)) return rc;
    if (n == 0) return 0;
    hipLaunchKernelGGL(opt_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), grad, (size_t)n, o);
    return check_hip(hipGetLastError(), who);
}

}  // namespace ptr

extern "C" int ptr_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int step, void *stream) {
    return ptr::opt_step_alone("ptr_adam_step", PTR_OPT_ADAM, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, stream);
}

extern "C" int ptr_adagrad_step(float *param, const float *grad, float *state_sum, int64_t n, float lr, float lr_decay, float eps,
                                float weight_decay, int step, void *stream) {
    return ptr::opt_step_alone("ptr_adagrad_step", PTR_OPT_ADAGRAD, param, grad, state_sum, nullptr, n, lr, lr_decay, 0.0f, eps, weight_decay, step, stream);
}

extern "C" int ptr_rmsprop_step(float *param, const float *grad, float *square_avg, int64_t n, float lr, float alpha, float eps,
                                float weight_decay, void *stream) {
    return ptr::opt_step_alone("ptr_rmsprop_step", PTR_OPT_RMSPROP, param, grad, square_avg, nullptr, n, lr, alpha, 0.0f, eps, weight_decay, 1, stream);
}

// The optimiser step + the loss-slot sum as ONE launch on a gradient that is already reduced (data parallelism: backward -> flat gradient ->
// RCCL all-reduce -> this): reduce_partials_kernel over ONE "partial" — the gradient itself — so the arithmetic is ptr_mlp_backward_step's,
// bit for bit, and the data-parallel step is the single-device launch sequence + one kernel + one collective.
extern "C" int ptr_opt_step_loss(float *params, const float *grad, int64_t n, int opt_kind, float lr, float hyper1, float hyper2, float eps,
                                 float weight_decay, int step, float *state1, float *state2, const float *loss_q, int nq, float *loss_out,
                                 void *stream) {
    using namespace ptr;
    const char *who = "ptr_opt_step_loss";
    OptStep o;
    if (int rc = make_opt_step(o, who, opt_kind, lr, hyper1, hyper2, eps, weight_decay, step, params, state1, state2, n > 0, loss_q, nq, loss_out)) return rc;
    if (n < 0 || (n > 0 && (!params || !grad))) { set_error("%s: bad optimiser / loss arguments", who); return PTR_ERR_INVALID_ARG; }
    if (n == 0 && !loss_out) return 0;
    const size_t nn = (size_t)n;
    return launch_reduce_partials(grad, 1, 1, nn, nn, nn, nullptr, o, as_stream(stream), who);
}
