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
#include "se_common.h"

#pragma clang fp contract(off)

namespace se {

constexpr int SGD_THREADS = 256;
constexpr int SGD_VEC = 4;

// the regularised gradient of one element: the first two lines of ag_update (adagrad.hip)
template <bool L2>
__device__ __forceinline__ float sgd_grad(float g, float p, float l2, float grad_scale)
{
    const float g1 = grad_scale == 1.0f ? g : g * grad_scale;
    float g2 = g1;
    if constexpr (L2) {
        const float r = l2 * p;
        g2 = g1 + r;
    }
    return g2;
}

template <bool L2>
__device__ __forceinline__ void sq_add(double &s, float g, float p, float l2, float grad_scale)
{
    const double g2 = (double)sgd_grad<L2>(g, p, l2, grad_scale);
    const double sq = g2 * g2;
    s = s + sq;
}

// workspace[blockIdx.x] = this workgroup's float64 sum of squares
template <bool VEC, bool L2>
__global__ __launch_bounds__(SGD_THREADS) void grad_sqsum_kernel(const float *__restrict__ g, const float *__restrict__ p,
                                                                 const float *__restrict__ l2, int64_t n, float grad_scale,
                                                                 double *__restrict__ partials)
{
    __shared__ double wave_part[SGD_THREADS / WAVE];
    const int64_t tid = (int64_t)blockIdx.x * SGD_THREADS + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * SGD_THREADS;
    double s = 0.0;
    if constexpr (VEC) {
        const int64_t units = n / SGD_VEC;
        for (int64_t u = tid; u < units; u += stride) {
            const float4 gv = ((const float4 *)g)[u];
            float4 pv = make_float4(0.f, 0.f, 0.f, 0.f), lv = pv;
            if constexpr (L2) {
                pv = ((const float4 *)p)[u];
                lv = ((const float4 *)l2)[u];
            }
            sq_add<L2>(s, gv.x, pv.x, lv.x, grad_scale);
            sq_add<L2>(s, gv.y, pv.y, lv.y, grad_scale);
            sq_add<L2>(s, gv.z, pv.z, lv.z, grad_scale);
            sq_add<L2>(s, gv.w, pv.w, lv.w, grad_scale);
        }
        const int64_t i = units * SGD_VEC + tid;            // the n % 4 tail: threads 0 .. 2 of the first workgroup
        if (i < n) sq_add<L2>(s, g[i], L2 ? p[i] : 0.f, L2 ? l2[i] : 0.f, grad_scale);
    } else {
        for (int64_t i = tid; i < n; i += stride) sq_add<L2>(s, g[i], L2 ? p[i] : 0.f, L2 ? l2[i] : 0.f, grad_scale);
    }
    s = wave_sum(s);
    if (lane_id() == 0) wave_part[threadIdx.x / WAVE] = s;
    wg_barrier();
    if (threadIdx.x == 0) {
        double t = wave_part[0];
#pragma unroll
        for (int w = 1; w < SGD_THREADS / WAVE; w++) t = t + wave_part[w];
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
    const float g2 = sgd_grad<L2>(g, p, l2, grad_scale);
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
__global__ __launch_bounds__(SGD_THREADS) void sgd_step_kernel(float *__restrict__ p, float *__restrict__ v, const float *__restrict__ g,
                                                               const float *__restrict__ l2, int64_t n, float lr,
                                                               const float *__restrict__ lr_dev, float grad_scale,
                                                               const float *__restrict__ clip_dev, float momentum)
{
    if (lr_dev) lr = lr_dev[0];
    float factor = 1.0f;
    if constexpr (CLIP) factor = clip_dev[0];
    const int64_t tid = (int64_t)blockIdx.x * SGD_THREADS + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * SGD_THREADS;
    if constexpr (VEC) {
        const int64_t units = n / SGD_VEC;
        for (int64_t u = tid; u < units; u += stride) {
            float4 pv = ((const float4 *)p)[u], vv = ((const float4 *)v)[u];
            const float4 gv = ((const float4 *)g)[u];
            float4 lv = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (L2) lv = ((const float4 *)l2)[u];
            sgd_update<L2, CLIP, NESTEROV>(pv.x, vv.x, gv.x, lv.x, lr, grad_scale, factor, momentum);
            sgd_update<L2, CLIP, NESTEROV>(pv.y, vv.y, gv.y, lv.y, lr, grad_scale, factor, momentum);
            sgd_update<L2, CLIP, NESTEROV>(pv.z, vv.z, gv.z, lv.z, lr, grad_scale, factor, momentum);
            sgd_update<L2, CLIP, NESTEROV>(pv.w, vv.w, gv.w, lv.w, lr, grad_scale, factor, momentum);
            ((float4 *)v)[u] = vv;
            ((float4 *)p)[u] = pv;
        }
        const int64_t i = units * SGD_VEC + tid;            // the n % 4 tail: threads 0 .. 2 of the first workgroup
        if (i < n) {
            float pi = p[i], vi = v[i];
            sgd_update<L2, CLIP, NESTEROV>(pi, vi, g[i], L2 ? l2[i] : 0.f, lr, grad_scale, factor, momentum);
            v[i] = vi;
            p[i] = pi;
        }
    } else {
        for (int64_t i = tid; i < n; i += stride) {
            float pi = p[i], vi = v[i];
            sgd_update<L2, CLIP, NESTEROV>(pi, vi, g[i], L2 ? l2[i] : 0.f, lr, grad_scale, factor, momentum);
            v[i] = vi;
            p[i] = pi;
        }
    }
}

// workgroups of a streaming launch over n elements: ceil(n / (256 * elements per thread)), capped
inline unsigned sgd_blocks(int64_t n, bool vec)
{
    const int64_t per_block = (int64_t)SGD_THREADS * (vec ? SGD_VEC : 1);
    const int64_t blocks = (n + per_block - 1) / per_block;
    return (unsigned)(blocks > SE_SGD_MAX_BLOCKS ? SE_SGD_MAX_BLOCKS : blocks);
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
    const bool vec = n >= SGD_VEC && aligned16(g) && (!l2 || (aligned16(l2) && aligned16(p)));
    const unsigned blocks = sgd_blocks(n, vec);
    const dim3 grid(blocks), block(SGD_THREADS);
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
    const bool vec = n >= SGD_VEC && aligned16(p) && aligned16(v) && aligned16(g) && (!l2 || aligned16(l2));
    const dim3 grid(sgd_blocks(n, vec)), block(SGD_THREADS);
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
