// C-ABI plumbing: thread-local error text, argument checks, the deterministic slot reduction.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "ptr_attn.h"
#include "ptr_device.h"
#include "ptr_div.h"
#include "ptr_gbdt.h"

namespace ptr {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return 0;
    set_error("%s: HIP error %d (%s)", what, (int)e, hipGetErrorString(e));
    return (int)e;
}

int check_batch(const void *preds, const void *second, int B, int L, const char *who) {
    if (B < 0 || L <= 0) { set_error("%s: bad shape B=%d L=%d", who, B, L); return PTR_ERR_INVALID_ARG; }
    if (B > 0 && (!preds || !second)) { set_error("%s: NULL input pointer", who); return PTR_ERR_INVALID_ARG; }
    if (L > PTR_MAX_LIST_LEN) {
        set_error("%s: list length %d exceeds PTR_MAX_LIST_LEN=%d", who, L, PTR_MAX_LIST_LEN);
        return PTR_ERR_UNSUPPORTED;
    }
    return 0;
}

// out[0] = scale * sum(x[0..n)) with a fixed tree (ptr_device.h block1024_sum): one workgroup of 1024 threads, sixteen loads in flight
// per thread.  n is a batch size (<= a few 10^5): ~4 us at 65 536 slots.
__global__ void __launch_bounds__(1024) sum_f32_kernel(const float *__restrict__ x, int n, float scale, float *__restrict__ out) {
    __shared__ float red[16];
    const float tot = block1024_sum(x, n, red);
    if (threadIdx.x == 0) out[0] = scale * tot;
}

// ptr_launch_form: each entry point's arguments -> the form function its launcher calls.  A form struct is ints only and goes out as it is.
struct FormQuery { const char *entry; int nargs, nform; void (*ask)(const int64_t *a, int32_t *out); };
template <class T> static void put(int32_t *out, const T &form) {
    static_assert(sizeof(T) % sizeof(int32_t) == 0);
    memcpy(out, &form, sizeof(T));
}
static void ask_attention(const int64_t *a, int32_t *out) {         // (L, dh, ld, store_ds, align_bytes)
    const int dh = (int)a[1], stride = (int)a[2];
    const uintptr_t address = (uintptr_t)a[4];
    const AttnForm f = attn_form(dh, (int)a[0], a[3] != 0);
    put(out, f);
    out[5] = f.wide ? wide_access_width(dh, stride, address) : ATTN_FLOAT4_ROWS(dh, stride, address) ? 4 : 1;
}
static void ask_layernorm(const int64_t *a, int32_t *out) { put(out, layernorm_form(a[0], (int)a[1])); }
static void ask_ring(const int64_t *a, int32_t *out) { put(out, ring_form((int)a[0])); }
static void ask_listnet(const int64_t *a, int32_t *out) { put(out, listnet_form((int)a[0], a[1] != 0)); }
static const FormQuery kFormQueries[] = {
    {"ptr_lambdarank_fwd_bwd", 3, 4, [](const int64_t *a, int32_t *out) { put(out, pairwise_form(true, (int)a[0], (int)a[1], a[2] != 0)); }},
    {"ptr_ranknet_fwd_bwd", 2, 4, [](const int64_t *a, int32_t *out) { put(out, pairwise_form(false, (int)a[0], (int)a[1], true)); }},
    {"ptr_approxndcg_fwd_bwd", 1, 3, [](const int64_t *a, int32_t *out) { put(out, approxndcg_form((int)a[0])); }},
    {"ptr_softrank_fwd_bwd", 1, 3, [](const int64_t *a, int32_t *out) { put(out, ring_form((int)a[0], false)); }},
    {"ptr_smoothmetric_fwd_bwd", 1, 3, ask_ring},
    {"ptr_gaussmetric_fwd_bwd", 1, 3, ask_ring},
    {"ptr_listnet_fwd_bwd", 2, 3, ask_listnet},
    {"ptr_listmle_fwd_bwd", 2, 3, [](const int64_t *a, int32_t *out) { put(out, listmle_form((int)a[0], a[1] != 0)); }},
    {"ptr_lambdaloss_fwd_bwd", 5, 3,
     [](const int64_t *a, int32_t *out) { put(out, lambdaloss_form((int)a[0], (int)a[1], (int)a[2], (int)a[3], a[4] != 0)); }},
    {"ptr_mhsa_forward", 5, 6, ask_attention},
    {"ptr_mhsa_backward", 5, 6, ask_attention},
    {"ptr_layernorm_forward", 2, 3, ask_layernorm},
    {"ptr_layernorm_backward", 2, 3, ask_layernorm},
    {"ptr_wassrank_fwd_bwd", 1, 2, [](const int64_t *a, int32_t *out) { put(out, wassrank_form((int)a[0])); }},
    {"ptr_alphadcg_fwd_bwd", 2, 2, [](const int64_t *a, int32_t *out) { put(out, div_form((int)a[0], (int)a[1])); }},
    {"ptr_div_metrics_at_ks", 1, 2, [](const int64_t *a, int32_t *out) { put(out, pick_tiling((int)a[0])); }},
    {"ptr_divprob_fwd_bwd", 3, 2, [](const int64_t *a, int32_t *out) { put(out, divprob_form((int)a[0], (int)a[1], (int)a[2])); }},
    {"ptr_gbdt_histogram", 3, 5, [](const int64_t *a, int32_t *out) { put(out, gbdt_hist_form(a[0], (int)a[1], (int)a[2])); }},
    {"ptr_gbdt_histogram_segments", 4, 8, [](const int64_t *a, int32_t *out) { put(out, gbdt_hist_segments_form(a[0], (int)a[1], (int)a[2], a[3])); }},
    // the other batched level passes have one form each: (launches per call, entries of the table one workgroup serves or 0)
    {"ptr_gbdt_hist_sub_segments", 1, 2, [](const int64_t *, int32_t *out) { out[0] = 1; out[1] = 1; }},
    {"ptr_gbdt_best_split_slots", 1, 2, [](const int64_t *, int32_t *out) { out[0] = 2; out[1] = 0; }},
    {"ptr_gbdt_partition_segments", 1, 2, [](const int64_t *a, int32_t *out) { out[0] = 3; out[1] = (int32_t)((a[0] + kGbdtPartRows - 1) / kGbdtPartRows); }},
    {"ptr_gbdt_goss", 1, 4, [](const int64_t *a, int32_t *out) { put(out, gbdt_goss_form(a[0])); }},
    {"ptr_gbdt_partition_mask", 1, 2, [](const int64_t *a, int32_t *out) { out[0] = 3; out[1] = (int32_t)((a[0] + kGbdtPartRows - 1) / kGbdtPartRows); }},
    {"ptr_gbdt_leaf_sums", 2, 5, [](const int64_t *a, int32_t *out) { put(out, gbdt_leaf_sums_form(a[0], a[1])); }},
    {"ptr_irgan_sample", 1, 2, [](const int64_t *a, int32_t *out) { put(out, irgan_form((int)a[0])); }},
    {"ptr_irgan_point_gen_fwd_bwd", 1, 2, [](const int64_t *a, int32_t *out) { put(out, irgan_form((int)a[0])); }},
    {"ptr_irgan_sel_fwd_bwd", 2, 2, [](const int64_t *a, int32_t *out) { put(out, irgan_sel_form((int)a[0], (int)a[1])); }},
    {"ptr_irfgan_point_sample", 1, 2, [](const int64_t *a, int32_t *out) { put(out, irgan_form((int)a[0])); }},
    {"ptr_irfgan_pair_sample", 1, 2, [](const int64_t *a, int32_t *out) { put(out, irgan_form((int)a[0])); }},
    {"ptr_irfgan_fwd_bwd", 2, 2, [](const int64_t *a, int32_t *out) { put(out, irfgan_loss_form((int)a[0], (int)a[1])); }},
    {"ptr_adlist_sample", 1, 2, [](const int64_t *a, int32_t *out) { put(out, adlist_form((int)a[0])); }},
    {"ptr_adlist_fwd_bwd", 1, 2, [](const int64_t *a, int32_t *out) { put(out, adlist_form((int)a[0])); }},
    {"ptr_tree_xendcg_grad_hess", 1, 3, [](const int64_t *a, int32_t *out) { put(out, tree_form((int)a[0])); }},
};

}  // namespace ptr

extern "C" int ptr_launch_form(const char *entry, const int64_t *args, int nargs, int32_t *form, int nform) {
    if (!entry || !args || !form) { ptr::set_error("ptr_launch_form: NULL pointer"); return PTR_ERR_INVALID_ARG; }
    for (const ptr::FormQuery &q : ptr::kFormQueries) {
        if (strcmp(entry, q.entry) != 0) continue;
        if (nargs != q.nargs || nform < q.nform) {
            ptr::set_error("ptr_launch_form: %s takes %d arguments and gives %d form values (got %d, room for %d)", entry, q.nargs, q.nform, nargs, nform);
            return PTR_ERR_INVALID_ARG;
        }
        q.ask(args, form);
        return 0;
    }
    ptr::set_error("ptr_launch_form: no form is defined for entry point '%s'", entry);
    return PTR_ERR_INVALID_ARG;
}

extern "C" int ptr_abi_version(void) { return PTR_ABI_VERSION; }

extern "C" const char *ptr_last_error(void) { return ptr::g_err; }

extern "C" int ptr_sum_f32(const float *x, int n, float scale, float *out, void *stream) {
    if (n < 0 || !out || (n > 0 && !x)) { ptr::set_error("ptr_sum_f32: bad arguments"); return PTR_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(ptr::sum_f32_kernel, dim3(1), dim3(1024), 0, ptr::as_stream(stream), x, n, scale, out);
    return ptr::check_hip(hipGetLastError(), "ptr_sum_f32");
}
