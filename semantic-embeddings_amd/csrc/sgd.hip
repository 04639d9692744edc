// sgd.hip -- Keras 2.2's SGD update of a flat float32 parameter buffer with a deterministic global-norm clip: the norm of the
// regularised gradient and its clip factor (se_grad_clip_factor: a partials launch and a one-wave finalising launch), then the whole
// update in one launch (se_sgd_step), with the gradient scale (the mean over the data-parallel ranks), the L2 kernel regulariser,
// the clip factor, the learning rate, momentum and Nesterov folded in.
//
// Replaces keras.optimizers.SGD.get_updates with clipnorm [third party, not in the reference tree] as the trainers of
// learn_image_embeddings.py / learn_classifier.py / learn_center_loss.py / learn_labelembedding.py compile it, and the whole-buffer
// passes engine.Trainer.apply_update otherwise runs (g *= scale; g += l2 * p; norm; g *= factor; v = m v - lr g; p += v).  Per element,
// every operation a separately rounded float32 operation (no contraction; '/' is hipcc's correctly rounded one):
//     g1 = grad_scale == 1 ? g : g * grad_scale
//     g2 = l2 ? g1 + l2 * p : g1                          l2 holds 2 lambda (FlatState.flat_l2)
//     S  = sum of (double)g2 * (double)g2                 float64; norm = (float)sqrt(S); factor = min(clipnorm / (norm + 1e-12f), 1)
//     g3 = clip ? g2 * factor : g2
//     step = lr * g3
//     v' = momentum * v - step                            Keras: v = self.momentum * m - lr * g
//     p' = nesterov ? (p + momentum * v') - step : p + v' Keras: p + self.momentum * v - lr * g
// g is only read.  Streaming kernels: the norm reads 1 (3 with l2) streams, the update reads 3 (4 with l2) and writes 2.  The sum's
// order is fixed by n and the alignment class alone (include/sehip.h): per-thread chains in ascending order, a xor butterfly over each
// wave, the four waves in order, one float64 partial per workgroup, and one wave that adds the partials the same way -- no atomics.
// 16-byte accesses when all pointers are 16-byte aligned (the n % 4 tail elements are taken one by one), 4-byte accesses otherwise;
// int64 indices; a grid-stride loop under a capped grid.
#include "flat_update.h"

#pragma clang fp contract(off)

namespace se {

template <bool L2>
__device__ __forceinline__ void sq_add(double &s, float g, float p, float l2, float grad_scale)
{
    const double g2 = (double)reg_grad<L2>(g, p, l2, grad_scale);
    const double sq = g2 * g2;
    s = s + sq;
}

// workspace[blockIdx.x] = this workgroup's float64 sum of squares
template <bool VEC, bool L2>
__global__ __launch_bounds__(FLAT_THREADS) void grad_sqsum_kernel(const float *__restrict__ g, const float *__restrict__ p,
                                                                  const float *__restrict__ l2, int64_t n, float grad_scale,
                                                                  double *__restrict__ partials)
{
    __shared__ double wave_part[FLAT_THREADS / WAVE];
    double s = 0.0;
    flat_stream<VEC>(n, [&](auto width, int64_t i) {
        constexpr int W = decltype(width)::value;
        const FlatVal<W> gv = flat_load<W>(g + i);
        FlatVal<W> pv{}, lv{};
        if constexpr (L2) {
            pv = flat_load<W>(p + i);
            lv = flat_load<W>(l2 + i);
        }
#pragma unroll
        for (int k = 0; k < W; k++) sq_add<L2>(s, gv.e[k], pv.e[k], lv.e[k], grad_scale);
    });
    s = wave_sum(s);
    if (lane_id() == 0) wave_part[threadIdx.x / WAVE] = s;
    wg_barrier();
    if (threadIdx.x == 0) {
        double t = wave_part[0];
#pragma unroll
        for (int w = 1; w < FLAT_THREADS / WAVE; w++) t = t + wave_part[w];
        partials[blockIdx.x] = t;
    }
}

// one wave: stats[0] = (float)sqrt(sum of the partials), stats[1] = the clip factor
__global__ __launch_bounds__(WAVE) void grad_clip_final_kernel(const double *__restrict__ partials, int nparts, float clipnorm,
                                                               float *__restrict__ stats)
{
    // all loads first (one latency, not one per partial), then the additions in index order; a missing partial adds +0, which
    // changes no sum of non-negative terms
    constexpr int PER_LANE = SE_SGD_MAX_BLOCKS / WAVE;
    static_assert(SE_SGD_MAX_BLOCKS % WAVE == 0, "the finalising wave takes SE_SGD_MAX_BLOCKS / 64 partials per lane");
    double part[PER_LANE];
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) {
        const int i = k * WAVE + (int)threadIdx.x;
        part[k] = i < nparts ? partials[i] : 0.0;
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) s = s + part[k];
    s = wave_sum(s);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        const float den = norm + 1e-12f;
        const float q = clipnorm / den;
        stats[0] = norm;
        stats[1] = q > 1.0f ? 1.0f : q;                     // a NaN q stays (fminf would drop it)
    }
}

template <bool L2, bool CLIP, bool NESTEROV>
__device__ __forceinline__ void sgd_update(float &p, float &v, float g, float l2, float lr, float grad_scale, float factor, float momentum)
{
    const float g2 = reg_grad<L2>(g, p, l2, grad_scale);
    float g3 = g2;
    if constexpr (CLIP) g3 = g2 * factor;
    const float step = lr * g3;
    const float mv = momentum * v;
    const float vn = mv - step;
    if constexpr (NESTEROV) {
        const float look = momentum * vn;
        const float ahead = p + look;
        p = ahead - step;
    } else {
        p = p + vn;
    }
    v = vn;
}

template <bool VEC, bool L2, bool CLIP, bool NESTEROV>
__global__ __launch_bounds__(FLAT_THREADS) void sgd_step_kernel(float *__restrict__ p, float *__restrict__ v, const float *__restrict__ g,
                                                                const float *__restrict__ l2, int64_t n, float lr,
                                                                const float *__restrict__ lr_dev, float grad_scale,
                                                                const float *__restrict__ clip_dev, float momentum)
{
    if (lr_dev) lr = lr_dev[0];
    float factor = 1.0f;
    if constexpr (CLIP) factor = clip_dev[0];
    flat_stream<VEC>(n, [&](auto width, int64_t i) {
        constexpr int W = decltype(width)::value;
        FlatVal<W> pv = flat_load<W>(p + i), vv = flat_load<W>(v + i), lv{};
        const FlatVal<W> gv = flat_load<W>(g + i);
        if constexpr (L2) lv = flat_load<W>(l2 + i);
#pragma unroll
        for (int k = 0; k < W; k++) sgd_update<L2, CLIP, NESTEROV>(pv.e[k], vv.e[k], gv.e[k], lv.e[k], lr, grad_scale, factor, momentum);
        flat_store(v + i, vv);
        flat_store(p + i, pv);
    });
}

}  // namespace se

using namespace se;

extern "C" size_t se_grad_clip_workspace_bytes(void) { return (size_t)SE_SGD_MAX_BLOCKS * sizeof(double); }

extern "C" int se_grad_clip_factor(const float *g, const float *p, const float *l2, int64_t n, float grad_scale, float clipnorm,
                                   void *workspace, float *stats, se_stream_t stream)
{
    if (n < 0) return fail(SE_ERR_INVALID, "se_grad_clip_factor: bad length n=%lld", (long long)n);
    if (!(clipnorm > 0.f) || !(clipnorm <= 3.402823466e+38f))
        return fail(SE_ERR_INVALID, "se_grad_clip_factor: clipnorm %g must be finite and > 0", (double)clipnorm);
    if (n == 0) return SE_OK;
    if (!g || !workspace || !stats) return fail(SE_ERR_INVALID, "se_grad_clip_factor: null pointer");
    if (l2 && !p) return fail(SE_ERR_INVALID, "se_grad_clip_factor: l2 needs p");
    if (((uintptr_t)workspace) & 7) return fail(SE_ERR_INVALID, "se_grad_clip_factor: the workspace must be 8-byte aligned");
    const bool vec = flat_vec_ok(n, g, l2 ? p : nullptr, l2);   // p is a buffer of the call only with l2
    const unsigned blocks = flat_blocks(n, vec, SE_SGD_MAX_BLOCKS);
    const dim3 grid(blocks), block(FLAT_THREADS);
    hipStream_t s = (hipStream_t)stream;
    double *partials = (double *)workspace;
    dispatch_bools(vec, l2 != nullptr, [&](auto V, auto L) {
        hipLaunchKernelGGL((grad_sqsum_kernel<V(), L()>), grid, block, 0, s, g, p, l2, n, grad_scale, partials);
    });
    SE_LAUNCH_CHECK();
    hipLaunchKernelGGL(grad_clip_final_kernel, dim3(1), dim3(WAVE), 0, s, (const double *)partials, (int)blocks, clipnorm, stats);
    SE_LAUNCH_CHECK();
    return SE_OK;
}

extern "C" int se_sgd_step(float *p, float *v, const float *g, const float *l2, int64_t n, float lr, const float *lr_dev,
                           float grad_scale, const float *clip_dev, float momentum, int nesterov, se_stream_t stream)
{
    if (n < 0) return fail(SE_ERR_INVALID, "se_sgd_step: bad length n=%lld", (long long)n);
    if (!(momentum >= 0.f)) return fail(SE_ERR_INVALID, "se_sgd_step: momentum %g must be >= 0", (double)momentum);
    if (n == 0) return SE_OK;
    if (!p || !v || !g) return fail(SE_ERR_INVALID, "se_sgd_step: null pointer");
    const bool vec = flat_vec_ok(n, p, v, g, l2);
    const dim3 grid(flat_blocks(n, vec, SE_SGD_MAX_BLOCKS)), block(FLAT_THREADS);
    hipStream_t s = (hipStream_t)stream;
    dispatch_bools(vec, [&](auto V) {                       // 16 instantiations: VEC x L2 x CLIP x NESTEROV
        dispatch_bools(l2 != nullptr, clip_dev != nullptr, nesterov != 0, [&](auto L, auto C, auto N) {
            hipLaunchKernelGGL((sgd_step_kernel<decltype(V)::value, L(), C(), N()>), grid, block, 0, s, p, v, g, l2, n, lr, lr_dev,
                               grad_scale, clip_dev, momentum);
        });
    });
    SE_LAUNCH_CHECK();
    return SE_OK;
}
