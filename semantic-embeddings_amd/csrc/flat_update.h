// flat_update.h -- what the optimizer kernels over a flat float32 buffer share (adagrad.hip, sgd.hip): the streaming loop with its
// value type, the regularised gradient of one element, and the host's launch geometry and 16-byte decision.  The order in which
// se_grad_clip_factor adds is promised in include/sehip.h and is the order of flat_stream, so that loop exists once.
#pragma once
#include "se_common.h"

#pragma clang fp contract(off)

namespace se {

constexpr int FLAT_THREADS = 256;
constexpr int FLAT_VEC = 4;             // floats per 16-byte unit

// W consecutive floats moved by one access: 16 bytes for W = 4 (the address must be 16-byte aligned), 4 bytes for W = 1
template <int W>
struct alignas(4 * W) FlatVal {
    float e[W];
};
template <int W>
__device__ __forceinline__ FlatVal<W> flat_load(const float *at) { return *(const FlatVal<W> *)at; }
template <int W>
__device__ __forceinline__ void flat_store(float *at, const FlatVal<W> &v) { *(FlatVal<W> *)at = v; }

// The streaming loop of a launch of FLAT_THREADS-wide workgroups over n elements: f(std::integral_constant<int, W>{}, i) for W
// elements from index i on, in ascending order within a thread.  VEC: W = 4 for the units u = tid, tid + stride, ... of n / 4, then
// W = 1 for the n % 4 tail on threads 0 .. 2 of the first workgroup.  Otherwise W = 1 for i = tid, tid + stride, ...
template <bool VEC, class F>
__device__ __forceinline__ void flat_stream(int64_t n, F f)
{
    const int64_t tid = (int64_t)blockIdx.x * FLAT_THREADS + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * FLAT_THREADS;
    constexpr std::integral_constant<int, 1> one{};
    if constexpr (VEC) {
        const int64_t units = n / FLAT_VEC;
        for (int64_t u = tid; u < units; u += stride) f(std::integral_constant<int, FLAT_VEC>{}, u * FLAT_VEC);
        const int64_t i = units * FLAT_VEC + tid;
        if (i < n) f(one, i);
    } else {
        for (int64_t i = tid; i < n; i += stride) f(one, i);
    }
}

// the regularised gradient of one element: g2 = g1 + l2 * p (g1 without L2), g1 = g * grad_scale (g when the scale is 1)
template <bool L2>
__device__ __forceinline__ float reg_grad(float g, float p, float l2, float grad_scale)
{
    const float g1 = grad_scale == 1.0f ? g : g * grad_scale;
    float g2 = g1;
    if constexpr (L2) {
        const float r = l2 * p;
        g2 = g1 + r;
    }
    return g2;
}

// ---- host ----
// workgroups of a streaming launch over n elements: ceil(n / (256 * elements per thread)), at most cap
inline unsigned flat_blocks(int64_t n, bool vec, int64_t cap) { return row_blocks(n, FLAT_THREADS * (vec ? FLAT_VEC : 1), cap); }

// whether a call takes 16-byte accesses: n >= 4 and every buffer it was given is 16-byte aligned (a null pointer is no buffer, and passes as address 0)
template <class... P>
inline bool flat_vec_ok(int64_t n, const P *...buf)
{
    return n >= FLAT_VEC && (aligned16(buf) && ...);
}

}  // namespace se
