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
#include "flat_update.h"

#pragma clang fp contract(off)

namespace se {

template <bool L2>
__device__ __forceinline__ void ag_update(float &p, float &a, float g, float l2, float lr, float grad_scale, float epsilon)
{
    const float g2 = reg_grad<L2>(g, p, l2, grad_scale);
    const float sq = g2 * g2;
    const float an = a + sq;
    const float den = sqrtf(an) + epsilon;
    const float num = lr * g2;
    const float step = num / den;
    a = an;
    p = p - step;
}

template <bool VEC, bool L2>
__global__ __launch_bounds__(FLAT_THREADS) void adagrad_step_kernel(float *__restrict__ p, float *__restrict__ accum,
                                                                    const float *__restrict__ g, const float *__restrict__ l2, int64_t n,
                                                                    float lr, const float *__restrict__ lr_dev, float grad_scale,
                                                                    float epsilon)
{
    if (lr_dev) lr = lr_dev[0];
    flat_stream<VEC>(n, [&](auto width, int64_t i) {
        constexpr int W = decltype(width)::value;
        FlatVal<W> pv = flat_load<W>(p + i), av = flat_load<W>(accum + i), lv{};
        const FlatVal<W> gv = flat_load<W>(g + i);
        if constexpr (L2) lv = flat_load<W>(l2 + i);
#pragma unroll
        for (int k = 0; k < W; k++) ag_update<L2>(pv.e[k], av.e[k], gv.e[k], lv.e[k], lr, grad_scale, epsilon);
        flat_store(accum + i, av);
        flat_store(p + i, pv);
    });
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
    const bool vec = flat_vec_ok(n, p, accum, g, l2);
    const dim3 grid(flat_blocks(n, vec, SE_ADAGRAD_MAX_BLOCKS)), block(FLAT_THREADS);
    hipStream_t s = (hipStream_t)stream;
    dispatch_bools(vec, l2 != nullptr, [&](auto V, auto L) {
        hipLaunchKernelGGL((adagrad_step_kernel<V(), L()>), grid, block, 0, s, p, accum, g, l2, n, lr, lr_dev, grad_scale, epsilon);
    });
    SE_LAUNCH_CHECK();
    return SE_OK;
}
