// se_common.h -- shared helpers for the gfx950 kernels behind include/sehip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <type_traits>

#include "../../include/sehip.h"

namespace se {

// thread-local last-error text (se_last_error)
char *err_buf();
int fail(int code, const char *fmt, ...);

// compute units of the current device (256 when the query fails), read once per process: one process drives one GPU model.
// (Hidden: an internal helper, not part of the library's exported symbols.)
__attribute__((visibility("hidden"))) int num_cus();

// out[0] = mean of v[0 .. n) in a fixed order (one 256-thread block; +0 for n = 0), on stream s (loss_kernels.hip; hidden like num_cus)
__attribute__((visibility("hidden"))) void launch_mean(const float *v, int64_t n, float *out, hipStream_t s);

// Phase timing (se_phase_timing / se_phase_timing_read, include/sehip.h): when switched on, multi-kernel entry points record a HIP
// event on their stream behind each phase.  Off (the default): one relaxed atomic load per mark.
void phase_mark(const char *name, hipStream_t s);
bool phase_timing_on();
void phase_note_counters(const unsigned *dev_counters, long long rows, hipStream_t s);   // se_retrieve_topk: its 4 statistics words, copied on stream s into a library-owned pinned buffer

#define SE_HIP_CHECK(expr)                                                                     \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess)                                                                 \
            return se::fail(SE_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                            __FILE__, __LINE__);                                               \
    } while (0)

#define SE_LAUNCH_CHECK()                                                                      \
    do {                                                                                       \
        hipError_t e__ = hipGetLastError();                                                    \
        if (e__ != hipSuccess)                                                                 \
            return se::fail(SE_ERR_HIP, "kernel launch failed: %s (%s:%d)",                    \
                            hipGetErrorString(e__), __FILE__, __LINE__);                       \
    } while (0)

constexpr int WAVE = 64;

// Tuning / test switches (environment variables that pin a kernel variant, print phase profiles or make a kernel skip work)
// exist only in the -DSE_TUNING build (sehip/libsehip_tuning.so, loaded by tests / tools through SEHIP_LIB): the product
// library ignores them all, so no environment variable can change what an entry point computes.  Product switches that stay:
// SE_RANK_SAFE=1 (guaranteed-order ranking kernel) and SE_RANK_VERBOSE=1 (says which ranking kernel the probe selected).
#ifdef SE_TUNING
inline const char *tuning_env(const char *name) { return getenv(name); }
constexpr bool kTuning = true;
#else
inline const char *tuning_env(const char *) { return nullptr; }
constexpr bool kTuning = false;
#endif

// Phase timer of the kernels that profile themselves in the tuning build: the cycles since the previous mark go to t_acc[i] when `on`
// (the kernel declares `uint64_t t_acc[], t_last` under the same #ifdef)
#ifdef SE_TUNING
#define SE_PHASE_T(on, i) if (on) { const uint64_t now = __builtin_amdgcn_s_memtime(); t_acc[i] += now - t_last; t_last = now; }
#else
#define SE_PHASE_T(on, i)
#endif

// Work-group barrier of every kernel in this library: drain this wave's LDS queue, THEN barrier.
// __syncthreads() alone is not enough on gfx950 with this compiler: for a barrier at a loop header the waitcnt pass can leave
// the back edge without an s_waitcnt lgkmcnt(0) between the previous stage's ds_write and the s_barrier (seen in the ISA of the
// LDS bitonic sort of topk_rows_kernel).  The stores are then still queued when the wave signals the barrier; the next stage's
// reader on another SIMD normally loses that race, but not when a second kernel's waves share the SIMD's LDS queue --
// se_topk_rows returned the right k entries in the wrong order in ~1 of 5 calls with another stream busy.
__device__ __forceinline__ void wg_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

// Order-preserving float32 -> uint32 key of the canonical ranking order:
// ascending value, -0.0 == +0.0, every NaN maps to 0xFFFFFFFF (sorted last).
__device__ __forceinline__ uint32_t canon_key(float f)
{
    uint32_t u = __float_as_uint(f);
    if (f != f) return 0xFFFFFFFFu;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }

// round-to-nearest-even float32 -> bf16 (NaN preserved)
__device__ __forceinline__ uint16_t f32_to_bf16(float f)
{
    uint32_t u = __float_as_uint(f);
    if (f != f) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// Wave-wide butterflies (every lane gets the result); T = float / int / int64_t / double
template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <class T>
__device__ __forceinline__ T wave_max(T v)      // floating point: fmax (a NaN loses against a number)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

template <class T>
__device__ __forceinline__ T wave_min(T v)      // integers
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// Inclusive prefix sum over the 64 lanes with data-parallel primitives (DPP), T = int / uint32_t / double: four row_shr steps scan
// each row of 16 lanes, row_bcast15 / row_bcast31 carry the row totals on -- six VALU instructions per 32-bit half instead of six
// ds_bpermute round trips (__shfl_up), and no LDS traffic.  Lane 63 holds the wave's total.
template <int CTRL, int ROWS, class T>
__device__ __forceinline__ T dpp_or_zero(T v)      // v of the lane that CTRL names; 0 where there is none or the row is masked out
{
    static_assert(std::is_same<T, int>::value || std::is_same<T, uint32_t>::value || std::is_same<T, double>::value, "int, uint32_t or double");
    if constexpr (sizeof(T) == 8) {
        const int lo = dpp_or_zero<CTRL, ROWS>(__double2loint(v)), hi = dpp_or_zero<CTRL, ROWS>(__double2hiint(v));
        return __hiloint2double(hi, lo);
    } else {
        return (T)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, true);
    }
}

template <class T>
__device__ __forceinline__ T wave_incl_scan(T v)
{
    v += dpp_or_zero<0x111, 0xf>(v);   // row_shr:1
    v += dpp_or_zero<0x112, 0xf>(v);   // row_shr:2
    v += dpp_or_zero<0x114, 0xf>(v);   // row_shr:4
    v += dpp_or_zero<0x118, 0xf>(v);   // row_shr:8
    v += dpp_or_zero<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
    v += dpp_or_zero<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
    return v;
}

// number of set bits of a wave mask (a ballot; or its two halves) below this lane
__device__ __forceinline__ uint32_t wave_prefix_count(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u)); }
__device__ __forceinline__ uint32_t wave_prefix_count(uint64_t ballot) { return wave_prefix_count((uint32_t)ballot, (uint32_t)(ballot >> 32)); }

// Sum of one value per thread of a 256-thread workgroup in a fixed order (thread t adds part[t + off], off = 128 ... 1); every thread
// gets the total.  part: 256 floats of LDS.
__device__ __forceinline__ float block_sum_256(float v, float *part)
{
    part[threadIdx.x] = v;
    wg_barrier();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        wg_barrier();
    }
    return part[0];
}

// element i of a float32 / bf16 array as float32, and its store (bf16: round to nearest even)
template <bool BF16>
__device__ __forceinline__ float ld_elem(const void *p, int64_t i)
{
    if constexpr (BF16) return bf16_to_f32(((const uint16_t *)p)[i]);
    else return ((const float *)p)[i];
}

template <bool BF16>
__device__ __forceinline__ void st_elem(void *p, int64_t i, float v)
{
    if constexpr (BF16) ((uint16_t *)p)[i] = f32_to_bf16(v);
    else ((float *)p)[i] = v;
}

// the 8 bf16 values of one 16-byte load, in memory order
__device__ __forceinline__ void unpack_bf16x8(uint4 p, float *v)
{
    const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[2 * k] = __uint_as_float(w[k] << 16);
        v[2 * k + 1] = __uint_as_float(w[k] & 0xFFFF0000u);
    }
}

// class label as a safe gather index: clamped to [0, C - 1] (the hosts validate; the kernels never read out of bounds).  C: int or int64_t
template <class TC>
__device__ __forceinline__ int64_t clamp_label(int64_t y, TC C) { return y < 0 ? 0 : (y >= C ? C - 1 : y); }

// ---- host helpers of the entry points ----
inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
inline bool aligned16(const void *p, int64_t ld, int elem_bytes) { return aligned16(p) && (ld * elem_bytes) % 16 == 0; }   // base and row pitch
inline bool is_float_dtype(int code) { return code == SE_DTYPE_F32 || code == SE_DTYPE_BF16; }
// grid of a kernel whose workgroups take rows_per_block rows at a time and stride over the rest: ceil(B / rows_per_block), capped
inline unsigned row_blocks(int64_t B, int rows_per_block, int64_t cap)
{
    const int64_t blocks = (B + rows_per_block - 1) / rows_per_block;
    return (unsigned)(blocks > cap ? cap : blocks);
}
// f(std::bool_constant<b0>{}, ...): run-time flags to template arguments, every combination instantiated
template <class F>
inline void dispatch_bools(bool b0, F f)
{
    if (b0) f(std::true_type{});
    else f(std::false_type{});
}
template <class F>
inline void dispatch_bools(bool b0, bool b1, F f)
{
    dispatch_bools(b0, [&](auto c0) { dispatch_bools(b1, [&](auto c1) { f(c0, c1); }); });
}
template <class F>
inline void dispatch_bools(bool b0, bool b1, bool b2, F f)
{
    dispatch_bools(b0, [&](auto c0) { dispatch_bools(b1, b2, [&](auto c1, auto c2) { f(c0, c1, c2); }); });
}

// f(std::integral_constant<int, clsw>{}) for the class-table width clsw = 0 / 1 / 2 of the ranking consumers (rank_stream.h); returns
// what f returns
template <class F>
inline auto dispatch_clsw(int clsw, F f)
{
    if (clsw == 1) return f(std::integral_constant<int, 1>{});
    if (clsw == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 0>{});
}

// K-block list of the canonical dot product: the FMA chain restarts per block, block sums are added in order
constexpr int SE_MAX_KB = 16;
struct KBlocks {
    int n;
    int len[SE_MAX_KB];
};
// metric epilogue of a canonical dot product: v = a.b, sa = |a|^2, sb = |b|^2 (Euclidean only)
template <int METRIC>
__device__ __forceinline__ float dist_finish(float v, float sa, float sb)
{
    if (METRIC == SE_METRIC_COSINE) return -v;
    if (METRIC == SE_METRIC_EUCLID) return (sa + sb) - 2.0f * v;
    return v;
}
// host: validate a caller's K-block list into `kbs`; *multi = more than one block.  SE_OK or an error code (text set).
int make_kblocks(const char *who, const int32_t *kblocks, int nkb, int64_t d, KBlocks &kbs, bool &multi);

// ---- fused distance + top-k (se_retrieve_topk): the two passes that run on the tile loop of pdist_mfma.hip ----
// Both take the GALLERY as the row operand and the QUERIES as the column operand of the MFMA tiles, so that a lane owns ONE
// query per 32-column block and sees 16 gallery rows of it per tile.
constexpr int EPI_STORE = 0;      // se_pairwise_dist: the tile goes to the distance matrix
constexpr int EPI_GROUPMIN = 1;   // sample pass: min over each lane's 16 values -> gm[query, group]
constexpr int EPI_FILTER = 2;     // main pass: values <= tau[query] are appended to the query's candidate list
constexpr int FUSED_GROUP = 16;   // values per group minimum (one lane, one 32 x 32 accumulator block)
struct FusedArgs {
    float *gm;             // EPI_GROUPMIN: [queries, gm_ld] group minima; group = 8 * (tile row index) + 2 * wave row + lane half
    int64_t gm_ld;
    const float *tau;      // EPI_FILTER: [queries] thresholds
    unsigned *rowcnt;      // EPI_FILTER: [queries] candidates appended so far (may exceed cap: the row is then redone)
    uint2 *lists;          // EPI_FILTER: [queries, cap] (float bits of the distance, gallery row)
    int64_t cap;
    int64_t sqa_stride;    // Euclidean epilogue: |a|^2 of row r is sqa[r * sqa_stride] (the sample pass strides through the gallery)
};
// host: one pass over (gallery rows [n_a, d] with pitch lda) x (queries [n_q, d]); metric SE_METRIC_COSINE / SE_METRIC_EUCLID
int launch_fused_pass(int epi, const float *gallery, int64_t lda, const float *queries, int64_t ldq, const float *sqg, const float *sqq,
                      int64_t n_a, int64_t n_q, int64_t d, int metric, const KBlocks &kbs, bool multi, const FusedArgs &fa, hipStream_t s);
int64_t pdist_max_ld();

// ---- bf16 pre-filter of the fused distance + top-k (prefilter.hip; driver and exact refinement: topk.hip) ----
constexpr int PF_EPI_GROUPMIN = 1, PF_EPI_FILTER = 2, PF_EPI_STORE = 3;
struct PfPassArgs {
    float *gm; int64_t gm_ld;          // sample pass: [queries, gm_ld] group minima of d~ (d~: the half-precision distance)
    const float *thr;                  // filter pass: [queries] thresholds (NaN: only NaN values pass)
    unsigned *rowcnt; uint2 *lists; int64_t cap;     // cap: entries per (query, sub-list)
    int spill; uint2 *spill_lists; unsigned *spill_cnt;   // filter pass: sub-list slots of every query's shared spill region, [queries][spill * cap]; fill counters [queries]
    int64_t sqa_stride;
    float *out; int64_t ldo;           // PF_EPI_STORE (tuning build): d~ matrix [gallery rows, queries]
    int d_valid;                       // columns that are not zero padding (0: all kp): the 128 x 128 kernel skips the all-zero k = 16 steps of its last chunk
};
int pf_padded_dim(int64_t d);
// fp32 rows -> scaled fp16 rows [n, pf_padded_dim(d)] + per-row norm of the image / of the rounding residual (upper bounds; NaN for
// irregular rows, whose image is all NaN) + ctl[0..4] = max image norm bits, max residual norm bits, irregular rows, largest regular
// magnitude bits, scale exponent (caller zeroes the 8-word ctl block)
int pf_convert(const float *x, int64_t ldx, int64_t n, int64_t d, uint16_t *out, float *nrm, float *res, unsigned *ctl, hipStream_t s);
// ctl_g / ctl_q: the ctl blocks pf_convert filled for the two operand matrices (word 4 = the image's scale exponent)
// geometry of a pass (prefilter.hip): the workgroups resident on an XCD form a gi x gj grid and take (gi query tiles) x (one of `parts`
// contiguous gallery ranges of `tpp` tiles) at a time, workgroup (i, j) walking the range's tiles j, j + gj, ...  A query's candidates of
// (range p, sequence j) go to sub-list p * gj + j:  lists[(query * nsub + sub) * cap ...], their number to rowcnt[query * nsub + sub],
// nsub = parts * gj.  want_parts = 0: as many ranges as keep every XCD busy for >= ~4 rounds.
struct PfGeom { int gi, gj, parts, tpp, big; };      // big: the 256 x 256 filter kernel (long rows) instead of the 128 x 128 one
PfGeom pf_geometry(int64_t n_a, int64_t n_q, int want_parts, int kp);    // kp: padded columns of the FILTER pass this is for; 0: sample pass
// filter pass with a spill region: counters [queries][nsub + spill] -> per-sub-list counts as the refinement reads them (prefilter.hip)
int pf_spill_counts(unsigned *rowcnt, const unsigned *spill_cnt, int64_t queries, int nsub, int spill, int64_t cap, hipStream_t s);
int pf_pass(int epi, const PfGeom *geom, int metric, const uint16_t *gallery, int64_t lda, const uint16_t *queries, int64_t ldq, const float *sqg,
            const float *sqq, int64_t n_a, int64_t n_q, int kp, const unsigned *ctl_g, const unsigned *ctl_q, const PfPassArgs &pa, hipStream_t s);

}  // namespace se
