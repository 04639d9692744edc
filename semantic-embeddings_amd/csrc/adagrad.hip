// adagrad.hip -- Keras 2.2's Adagrad update of a flat float32 parameter buffer in one launch, with the gradient scale (the mean over
// the data-parallel ranks) and the L2 kernel regulariser folded in.
//
// Replaces keras.optimizers.Adagrad.get_updates [third party, not in the reference tree] as learn_devise.py:87,114 uses it, and the
// passes engine.Trainer.apply_update would otherwise run in front of it (g *= scale; g += l2 * p).  Per element, every operation a
// separately rounded float32 operation (no contraction; '/' and sqrtf are hipcc's correctly rounded ones):
//     g1 = grad_scale == 1 ? g : g * grad_scale
//     g2 = l2 ? g1 + l2 * p : g1                          l2 holds 2 lambda (FlatState.flat_l2)
//     a' = a + g2 * g2
//     p' = p - (lr * g2) / (sqrt(a') + epsilon)           Keras: p - lr * g / (K.sqrt(new_a) + epsilon)
// g is only read.  A streaming kernel: 3 (4 with l2) streams in, 2 out, nothing shared between elements, so no LDS, no barrier, no
// atomics and the same bits whatever the launch geometry.  16-byte accesses when all pointers are 16-byte aligned (the n % 4 tail
// elements are taken one by one), 4-byte accesses otherwise; int64 indices; a grid-stride loop under a capped grid.
#include "se_common.h"

#pragma clang fp contract(off)

namespace se {

constexpr int AG_THREADS = 256;
constexpr int AG_VEC = 4;

template <bool L2>
__device__ __forceinline__ void ag_update(float &p, float &a, float g, float l2, float lr, float grad_scale, float epsilon)
{
    const float g1 = grad_scale == 1.0f ? g : g * grad_scale;
    float g2 = g1;
    if constexpr (L2) {
        const float r = l2 * p;
        g2 = g1 + r;
    }
    const float sq = g2 * g2;
    const float an = a + sq;
    const float den = sqrtf(an) + epsilon;
    const float num = lr * g2;
    const float step = num / den;
    a = an;
    p = p - step;
}

template <bool VEC, bool L2>
__global__ __launch_bounds__(AG_THREADS) void adagrad_step_kernel(float *__restrict__ p, float *__restrict__ accum,
                                                                  const float *__restrict__ g, const float *__restrict__ l2, int64_t n,
                                                                  float lr, const float *__restrict__ lr_dev, float grad_scale,
                                                                  float epsilon)
{
    if (lr_dev) lr = lr_dev[0];
    const int64_t tid = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * AG_THREADS;
    if constexpr (VEC) {
        const int64_t units = n / AG_VEC;
        for (int64_t u = tid; u < units; u += stride) {
            float4 pv = ((const float4 *)p)[u], av = ((const float4 *)accum)[u];
            const float4 gv = ((const float4 *)g)[u];
            float4 lv = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (L2) lv = ((const float4 *)l2)[u];
            ag_update<L2>(pv.x, av.x, gv.x, lv.x, lr, grad_scale, epsilon);
            ag_update<L2>(pv.y, av.y, gv.y, lv.y, lr, grad_scale, epsilon);
            ag_update<L2>(pv.z, av.z, gv.z, lv.z, lr, grad_scale, epsilon);
            ag_update<L2>(pv.w, av.w, gv.w, lv.w, lr, grad_scale, epsilon);
            ((float4 *)accum)[u] = av;
            ((float4 *)p)[u] = pv;
        }
        const int64_t i = units * AG_VEC + tid;             // the n % 4 tail: threads 0 .. 2 of the first workgroup
        if (i < n) {
            float pi = p[i], ai = accum[i];
            ag_update<L2>(pi, ai, g[i], L2 ? l2[i] : 0.f, lr, grad_scale, epsilon);
            accum[i] = ai;
            p[i] = pi;
        }
    } else {
        for (int64_t i = tid; i < n; i += stride) {
            float pi = p[i], ai = accum[i];
            ag_update<L2>(pi, ai, g[i], L2 ? l2[i] : 0.f, lr, grad_scale, epsilon);
            accum[i] = ai;
            p[i] = pi;
        }
    }
}

}  // namespace se

using namespace se;

extern "C" int se_adagrad_step(float *p, float *accum, const float *g, const float *l2, int64_t n, float lr, const float *lr_dev,
                               float grad_scale, float epsilon, se_stream_t stream)
{
    if (n < 0) return fail(SE_ERR_INVALID, "se_adagrad_step: bad length n=%lld", (long long)n);
    if (!(epsilon >= 0.f)) return fail(SE_ERR_INVALID, "se_adagrad_step: epsilon %g must be >= 0", (double)epsilon);
    if (n == 0) return SE_OK;
    if (!p || !accum || !g) return fail(SE_ERR_INVALID, "se_adagrad_step: null pointer");
    const bool vec = n >= AG_VEC && aligned16(p) && aligned16(accum) && aligned16(g) && (!l2 || aligned16(l2));
    const int64_t per_block = (int64_t)AG_THREADS * (vec ? AG_VEC : 1);
    int64_t blocks = (n + per_block - 1) / per_block;
    if (blocks > SE_ADAGRAD_MAX_BLOCKS) blocks = SE_ADAGRAD_MAX_BLOCKS;
    const dim3 grid((unsigned)blocks), block(AG_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (vec) {
        if (l2) hipLaunchKernelGGL((adagrad_step_kernel<true, true>), grid, block, 0, s, p, accum, g, l2, n, lr, lr_dev, grad_scale, epsilon);
        else hipLaunchKernelGGL((adagrad_step_kernel<true, false>), grid, block, 0, s, p, accum, g, l2, n, lr, lr_dev, grad_scale, epsilon);
    } else {
        if (l2) hipLaunchKernelGGL((adagrad_step_kernel<false, true>), grid, block, 0, s, p, accum, g, l2, n, lr, lr_dev, grad_scale, epsilon);
        else hipLaunchKernelGGL((adagrad_step_kernel<false, false>), grid, block, 0, s, p, accum, g, l2, n, lr, lr_dev, grad_scale, epsilon);
    }
    SE_LAUNCH_CHECK();
    return SE_OK;
}
