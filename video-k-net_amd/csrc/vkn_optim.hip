// vkn_optim.hip — AdamW behind a global L2 gradient clip over the flat gradient buckets of dist.BucketedGradAllReducer: the
// optimizer of every shipped schedule (configs/det/_base_/schedules/schedule_1x.py:1-8 — AdamW lr 1e-4, weight_decay 0.05,
// grad_clip max_norm 1, norm_type 2), which the reference runs through mmcv's OptimizerHook as torch's clip_grad_norm_ followed by
// torch.optim.AdamW.step() (external/train.py:67, 98-104).
// One step of one device = three launches, no host read:
//   k_adamw_sqnorm  one workgroup per work item (a <= 16 K-element chunk of one parameter): sum of grad^2, one partial per item;
//   k_adamw_finish  one workgroup: the partials merged in fp64 -> total norm, clip coefficient, step counters;
//   k_adamw_update  one workgroup per work item: torch's single-tensor AdamW (torch/optim/adam.py, decoupled_weight_decay=True).
// Every sum runs in a fixed order (lane -> wave -> workgroup -> items) and no atomics are used: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/vkn.h"
#include "vkn_common.h"

namespace {

constexpr int ADAMW_THREADS = 256;
constexpr size_t ADAMW_WS_HEAD = 256;   // [0, 256): the clip coefficient (float at 0); the per-item partials (double) follow

// the item table holds generic pointers: tell the compiler they address global memory (global_load / global_store, not flat_*)
typedef __attribute__((address_space(1))) f32x4 gf32x4;
__device__ __forceinline__ gf32x4* adamw_global(float* p) { return (gf32x4*)(p); }
__device__ __forceinline__ const gf32x4* adamw_global(const float* p) { return (const gf32x4*)(p); }

// an item the kernels may touch: indices in range, a positive multiple of 4 elements, four 16-byte aligned pointers
__device__ __forceinline__ bool adamw_item_ok(const VknAdamwItem& it, int n_params, int n_groups) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(it.param) | reinterpret_cast<uintptr_t>(it.grad) |
                        reinterpret_cast<uintptr_t>(it.exp_avg) | reinterpret_cast<uintptr_t>(it.exp_avg_sq);
    return it.param && it.grad && it.exp_avg && it.exp_avg_sq && (a & 15) == 0 && it.n > 0 && (it.n & 3) == 0 &&
           it.param_index >= 0 && it.param_index < n_params && it.group_index >= 0 && it.group_index < n_groups;
}

// workgroup sum of one double per thread, fixed order: shuffles down inside each wave, then the four wave sums in wave order
__device__ __forceinline__ double adamw_block_sum(double v, double* lds4) {
#pragma unroll
    for (int off = VKN_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, VKN_WAVE);
    const int lane = threadIdx.x & (VKN_WAVE - 1), wave = threadIdx.x / VKN_WAVE;
    if (lane == 0) lds4[wave] = v;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

__global__ __launch_bounds__(ADAMW_THREADS) void k_adamw_sqnorm(const VknAdamwItem* __restrict__ items, int n_params, int n_groups,
                                                                const unsigned char* __restrict__ active, double* __restrict__ partial) {
    __shared__ double lds4[ADAMW_THREADS / VKN_WAVE];
    const VknAdamwItem it = items[blockIdx.x];
    double acc = 0.0;
    if (adamw_item_ok(it, n_params, n_groups) && active[it.param_index]) {     // an inactive parameter contributes nothing
        const gf32x4* __restrict__ g4 = adamw_global(it.grad);
        const int n4 = it.n >> 2;
#pragma unroll 4
        for (int i = threadIdx.x; i < n4; i += ADAMW_THREADS) {
            const f32x4 g = g4[i];
            acc = fma((double)g[0], (double)g[0], acc);
            acc = fma((double)g[1], (double)g[1], acc);
            acc = fma((double)g[2], (double)g[2], acc);
            acc = fma((double)g[3], (double)g[3], acc);
        }
    }
    const double s = adamw_block_sum(acc, lds4);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(ADAMW_THREADS) void k_adamw_finish(const double* __restrict__ partial, int n_items, int clip, float max_norm,
                                                                int* __restrict__ steps, const unsigned char* __restrict__ active,
                                                                int n_params, float* __restrict__ total_norm_out, float* __restrict__ coef,
                                                                float* __restrict__ coef_out) {
    __shared__ double red[ADAMW_THREADS];
    double s = 0.0;
    if (clip)
        for (int i = threadIdx.x; i < n_items; i += ADAMW_THREADS) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = ADAMW_THREADS / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float c = 1.f;
        if (clip) {
            const float tn = (float)sqrt(red[0]);
            if (total_norm_out) *total_norm_out = tn;
            // torch: clip_coef = max_norm / (total_norm + 1e-6); clamp(clip_coef, max=1.0).  torch.clamp keeps a NaN (fminf would
            // return 1); an inf norm gives 0.
            const float q = max_norm / (tn + 1e-6f);
            c = q > 1.f ? 1.f : q;
        }
        *coef = c;
        if (coef_out) *coef_out = c;
    }
    for (int i = threadIdx.x; i < n_params; i += ADAMW_THREADS)
        if (active[i]) steps[i] += 1;
}

__global__ __launch_bounds__(ADAMW_THREADS) void k_adamw_update(const VknAdamwItem* __restrict__ items, int n_params, int n_groups,
                                                                const double* __restrict__ rows, const int* __restrict__ steps,
                                                                const unsigned char* __restrict__ active, const float* __restrict__ coef_p) {
    const VknAdamwItem it = items[blockIdx.x];
    if (!adamw_item_ok(it, n_params, n_groups) || !active[it.param_index]) return;
    const double* r = rows + (size_t)it.group_index * VKN_ADAMW_GROUP_ROW;
    const double lr = r[0], wd = r[1], b1 = r[2], b2 = r[3], eps = r[4];
    const double step = (double)steps[it.param_index];
    // torch's scalars are Python floats (fp64) that enter the fp32 tensor ops rounded to float
    const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
    const float decay = (float)(1.0 - lr * wd);
    const float w1 = (float)(1.0 - b1);
    const float b2f = (float)b2, omb2 = (float)(1.0 - b2);
    const float neg_step = (float)(-(lr / bc1));
    const float bc2_sqrt = (float)sqrt(bc2);
    const float epsf = (float)eps;
    const float coef = *coef_p;
    const bool w1_small = fabsf(w1) < 0.5f;     // torch's lerp: two forms, chosen by the size of the weight
    gf32x4* __restrict__ p4 = adamw_global(it.param);
    const gf32x4* __restrict__ g4 = adamw_global(it.grad);
    gf32x4* __restrict__ m4 = adamw_global(it.exp_avg);
    gf32x4* __restrict__ v4 = adamw_global(it.exp_avg_sq);
    const int n4 = it.n >> 2;
#pragma unroll 2
    for (int i = threadIdx.x; i < n4; i += ADAMW_THREADS) {
        f32x4 p = p4[i], m = m4[i], v = v4[i];
        const f32x4 gr = g4[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float g = gr[e] * coef;                                  // the clipped gradient (grad itself is not written)
            const float pd = p[e] * decay;                                 // param.mul_(1 - lr * weight_decay)
            const float d = g - m[e];
            const float me = w1_small ? m[e] + w1 * d : g - d * (1.f - w1);   // exp_avg.lerp_(grad, 1 - beta1)
            const float ve = v[e] * b2f + omb2 * (g * g);                  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
            const float denom = sqrtf(ve) / bc2_sqrt + epsf;               // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
            p[e] = pd + neg_step * (me / denom);                           // param.addcdiv_(exp_avg, denom, value=-step_size)
            m[e] = me;
            v[e] = ve;
        }
        p4[i] = p;
        m4[i] = m;
        v4[i] = v;
    }
}

}  // namespace

extern "C" {

size_t vkn_sizeof_adamw_item(void) { return sizeof(VknAdamwItem); }

size_t vkn_adamw_workspace_bytes(int n_items, int n_params, int n_groups) {
    if (n_items <= 0 || n_params <= 0 || n_groups <= 0) return 0;
    return ADAMW_WS_HEAD + ((size_t)n_items * sizeof(double) + 255) / 256 * 256;
}

int vkn_adamw_flat_f32(const VknAdamwItem* items, int n_items, int n_params, const double* group_rows, int n_groups, int* steps,
                       const unsigned char* active, float max_norm, float* total_norm_out, float* coef_out, void* ws, size_t ws_bytes,
                       void* stream) {
    if (!items || !group_rows || !steps || !active || n_items <= 0 || n_params <= 0 || n_groups <= 0) return VKN_E_ARG;
    if (max_norm != max_norm) return VKN_E_ARG;                      // a NaN max_norm
    const size_t need = vkn_adamw_workspace_bytes(n_items, n_params, n_groups);
    if (!ws || ws_bytes < need) return VKN_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(ws) & 15) || (reinterpret_cast<uintptr_t>(items) & 7) || (reinterpret_cast<uintptr_t>(group_rows) & 7) ||
        (reinterpret_cast<uintptr_t>(steps) & 3) || (reinterpret_cast<uintptr_t>(total_norm_out) & 3) ||
        (reinterpret_cast<uintptr_t>(coef_out) & 3))
        return VKN_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* coef = static_cast<float*>(ws);
    double* partial = reinterpret_cast<double*>(static_cast<char*>(ws) + ADAMW_WS_HEAD);
    const int clip = max_norm > 0.f;
    if (clip) {
        hipLaunchKernelGGL(k_adamw_sqnorm, dim3((unsigned)n_items), dim3(ADAMW_THREADS), 0, st, items, n_params, n_groups, active, partial);
        VKN_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_adamw_finish, dim3(1), dim3(ADAMW_THREADS), 0, st, partial, n_items, clip, max_norm, steps, active, n_params,
                       total_norm_out, coef, coef_out);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_adamw_update, dim3((unsigned)n_items), dim3(ADAMW_THREADS), 0, st, items, n_params, n_groups, group_rows, steps,
                       active, coef);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

}  // extern "C"
