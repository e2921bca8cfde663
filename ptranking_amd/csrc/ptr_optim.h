// The flat optimisers (torch.optim.Adam / Adagrad / RMSprop on ONE flat fp32 buffer, ptranking/base/ranker.py:512-525): the update rule, the
// host-side step descriptor and the launcher of the partial reduction that carries the step (optim.hip).
#pragma once
#include <math.h>

#include "ptr_device.h"

namespace ptr {

// Optional epilogue of the partial reduction: the optimiser step on the element just reduced (single-device training: no all-reduce sits
// between gradient and step) and the sum of the loss slots of the batch — three launches fewer per train step.
struct OptStep {
    int kind;                      // 0 = none, PTR_OPT_ADAM / _ADAGRAD / _RMSPROP
    float lr, h1, h2, eps, wd, bc1, bc2_sqrt;
    float *param, *s1, *s2;
    const float *loss_q; int nq; float *loss_out;
    uint8_t *wimg; int F, NL;      // r6: the bf16x6 forward's weight image, refreshed element by element behind the step (NULL: none)
};

// Validates the optimiser and loss arguments of a step entry point and fills `o` (wimg / F / NL stay unset: no image).  `need_state`: the
// state buffers are dereferenced (false for an empty parameter vector).  Host scalars as torch computes them in fp32:
//   Adam     hyper1 = beta1, hyper2 = beta2, state1 = exp_avg, state2 = exp_avg_sq; bias corrections 1 - beta1^t and sqrt(1 - beta2^t)
//   Adagrad  hyper1 = lr_decay, state1 = sum; lr is the decayed clr = lr / (1 + (t - 1) lr_decay)
//   RMSprop  hyper1 = alpha, state1 = square_avg
inline int make_opt_step(OptStep &o, const char *who, int opt_kind, float lr, float hyper1, float hyper2, float eps, float weight_decay, int step,
                         float *params, float *state1, float *state2, bool need_state, const float *loss_q, int nq, float *loss_out) {
    if (opt_kind < PTR_OPT_ADAM || opt_kind > PTR_OPT_RMSPROP) { set_error("%s: unknown optimiser %d", who, opt_kind); return PTR_ERR_INVALID_ARG; }
    if (step < 1 || nq < 0 || (need_state && (!state1 || (opt_kind == PTR_OPT_ADAM && !state2))) || (loss_out && nq > 0 && !loss_q)) {
        set_error("%s: bad optimiser / loss arguments", who);
        return PTR_ERR_INVALID_ARG;
    }
    o = OptStep{};
    o.kind = opt_kind; o.lr = lr; o.h1 = hyper1; o.h2 = hyper2; o.eps = eps; o.wd = weight_decay;
    o.param = params; o.s1 = state1; o.s2 = state2; o.loss_q = loss_q; o.nq = nq; o.loss_out = loss_out;
    if (opt_kind == PTR_OPT_ADAM) { o.bc1 = 1.0f - powf(hyper1, (float)step); o.bc2_sqrt = sqrtf(1.0f - powf(hyper2, (float)step)); }
    else if (opt_kind == PTR_OPT_ADAGRAD) o.lr = lr / (1.0f + (float)(step - 1) * hyper1);
    return 0;
}

// grad[i] = sum_b ws[b][i] over the per-block partials (entries i >= tail_begin only have nblk_tail of them), then the step `o` on every
// element and the loss-slot sum (o.kind == 0 / o.loss_out == NULL: none).  grad == NULL: `ws` is the gradient itself (one partial).
int launch_reduce_partials(const float *ws, int nblk, int nblk_tail, size_t tail_begin, size_t stride, size_t n, float *grad, const OptStep &o,
                           hipStream_t st, const char *who);

#if defined(__HIPCC__)
// THE update rule: the step `o` on element i whose (reduced) gradient is g; writes the state and the parameter and returns the new parameter.
//   Adam     g += wd p; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
//   Adagrad  g += wd p; sum += g g;                                      p -= clr * g / (sqrt(sum) + eps)
//   RMSprop  g += wd p; sq = alpha sq + (1 - alpha) g g;                 p -= lr * g / (sqrt(sq) + eps)      (no momentum, not centered)
// One rounded operation per operator, in this order (the build keeps -ffp-contract=off): tests/optim_ref.py restates it line by line.
__device__ __forceinline__ float opt_update(const OptStep &o, size_t i, float g) {
    const float pi = o.param[i];
    const float gi = g + o.wd * pi;
    float upd;
    if (o.kind == PTR_OPT_ADAM) {
        const float mi = o.h1 * o.s1[i] + (1.0f - o.h1) * gi;
        const float vi = o.h2 * o.s2[i] + (1.0f - o.h2) * gi * gi;
        o.s1[i] = mi; o.s2[i] = vi;
        const float denom = sqrtf(vi) / o.bc2_sqrt + o.eps;
        upd = (o.lr / o.bc1) * (mi / denom);
    } else {
        const float si = o.kind == PTR_OPT_ADAGRAD ? o.s1[i] + gi * gi : o.h1 * o.s1[i] + (1.0f - o.h1) * gi * gi;
        o.s1[i] = si;
        upd = o.lr * (gi / (sqrtf(si) + o.eps));         // Adagrad: o.lr = the decayed clr
    }
    const float pn = pi - upd;
    o.param[i] = pn;
    return pn;
}
#endif

}  // namespace ptr
