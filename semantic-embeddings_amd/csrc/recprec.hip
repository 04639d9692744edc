// recprec.hip -- recall-precision curves and mAP on the device (the second consumer of the rankings, next to hprec.hip).
//
// Replaces the per-query loop of plot_recall_precision.py:52-79: for every query, the relevance of its ranking with the query
// itself removed, average precision, and the (recall, max precision) points that are averaged into the curve.  Everything the
// reference computes there is a function of ONE list of integers per query: p_j, the 1-based position (self removed) of the j-th
// item of the query's class.  Two steps:
//
// * relpos_kernel (se_relevant_positions) writes those positions.  Persistent 256-thread workgroups take one query at a time and
//   walk its ranking in 2048-rank chunks (thread t owns two runs of 4 consecutive ranks, one 16-byte load each, requested a chunk
//   ahead): rank -> class through a byte / 16-bit copy of the gallery's classes in LDS (filled once per workgroup), relevance by a
//   compare with the query's class, the query's own position by a ballot on its gallery index.  The index j of a hit is a wave
//   prefix count (one ballot + mbcnt per rank slot) plus the per-wave totals of the chunk, exchanged through LDS behind the ONE
//   barrier of the chunk (double-buffered).  A row stops streaming once its R_q hits are found: the tail of a ranking behind the
//   last relevant item changes nothing the reference computes.
// * se_recall_precision_reduce turns the positions of a tile of queries into per-query AP and per-class sums, in a fixed order
//   (no float atomics: the same inputs give the same bits).  Queries of one class share R, so all their unbinned recall levels are
//   j / R: one thread per (class, j) sums j / p_j over the class's queries, in query order, on top of what earlier tiles left in
//   the buffer -- tiling does not change a bit.  Binned curves: one wave per (class, bin) takes the max of j / p_j over the bin's j
//   for every query of the class (max is exact in any order) and adds it to the bin's sum.
// float64 throughout; every j / p_j is an IEEE (correctly rounded) division, like the reference's tp / arange.
#include "rank_stream.h"

#include <limits.h>

namespace se {

constexpr int RP_THREADS = 256;
constexpr int RP_WAVES = RP_THREADS / WAVE;
constexpr int RP_VEC = 4;                          // consecutive ranks per thread and group (one 16-byte / 8-byte load)
constexpr int RP_GROUPS = 2;                       // groups per chunk: position of (group g, thread t, element k) = g * 1024 + 4 t + k
constexpr int RP_GSPAN = RP_THREADS * RP_VEC;
constexpr int RP_CHUNK = RP_GSPAN * RP_GROUPS;
constexpr int RP_HEAD_INTS = 2 * (RP_GROUPS + 1) * RP_WAVES;     // [2][RP_GROUPS][RP_WAVES] hit counts, [2][RP_WAVES] self positions
constexpr int RP_MAX_BINS = 1 << 20;

// CLSW: where the class of a ranked gallery item comes from (rank_stream.h) -- 1 / 2: a byte / 16-bit copy of `cls` in LDS; 0: global gathers.
// RT: element type of the rankings -- int32_t, or uint16_t (se_rank_rows with idx64 == 2).
template <int CLSW, typename RT>
__global__ __launch_bounds__(RP_THREADS) void relpos_kernel(const RT *__restrict__ rank, int64_t ldr, int64_t Q, int64_t L,
                                                            const int32_t *__restrict__ cls, int64_t gallery,
                                                            const int32_t *__restrict__ qcls, const int32_t *__restrict__ qidx,
                                                            const int64_t *__restrict__ hit_off, int32_t *__restrict__ hit_pos, int vec_ok)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rp_raw[];
    int *s_cnt = reinterpret_cast<int *>(rp_raw);
    int *s_self = s_cnt + 2 * RP_GROUPS * RP_WAVES;
    unsigned char *s_cls = rp_raw + RP_HEAD_INTS * sizeof(int);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- once per workgroup: the gallery's classes into LDS ----
    fill_class_table<CLSW, RP_THREADS, 2>(cls, gallery, s_cls, tid);
    wg_barrier();

    const int Li = (int)L;                 // positions are int32 (checked at the entry point)
    int par = 0;
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        const int64_t off = hit_off[q];
        const int R = (int)(hit_off[q + 1] - off);
        if (R <= 0) continue;                                         // uniform: no relevant item, nothing to find
        const int qc = qcls[q];
        const int self = qidx ? qidx[q] : -1;
        const RT *row = rank + q * ldr;
        int32_t *out = hit_pos + off;
        int r[RP_GROUPS][RP_VEC];
#pragma unroll
        for (int g = 0; g < RP_GROUPS; g++) load_ranks(r[g], row, g * RP_GSPAN + tid * RP_VEC, Li, vec_ok);
        int carry = 0;                                                // hits in the chunks before this one (the same in every thread)
        bool self_before = false;                                     // the query itself was met in an earlier chunk
        for (int base = 0; base < Li; base += RP_CHUNK) {
            unsigned bits[RP_GROUPS];                                 // bit k of group g: position g * 1024 + 4 tid + k is a hit
            bool mine_self = false;
            int self_at = 0;
#pragma unroll
            for (int g = 0; g < RP_GROUPS; g++) {
                bits[g] = 0;
#pragma unroll
                for (int k = 0; k < RP_VEC; k++) {
                    const int pos = base + g * RP_GSPAN + tid * RP_VEC + k;
                    const bool live = pos < Li;
                    const int v = r[g][k];
                    const int c = class_of<CLSW>(s_cls, cls, v, live, -1);
                    const bool is_self = live && v == self;
                    bits[g] |= (live && !is_self && c == qc) ? (1u << k) : 0u;
                    if (is_self) { mine_self = true; self_at = pos; }
                }
            }
            // the rank registers are free: the next chunk's ranks are requested here, in front of the counts and the barrier
#pragma unroll
            for (int g = 0; g < RP_GROUPS; g++) load_ranks(r[g], row, base + RP_CHUNK + g * RP_GSPAN + tid * RP_VEC, Li, vec_ok);
            // ---- hit index: ballot + mbcnt inside the wave, per-wave totals through LDS ----
            int below[RP_GROUPS];
            int *cnt = s_cnt + par * RP_GROUPS * RP_WAVES;
#pragma unroll
            for (int g = 0; g < RP_GROUPS; g++) {
                int n = 0;
                below[g] = 0;
#pragma unroll
                for (int k = 0; k < RP_VEC; k++) {
                    const uint64_t m = __ballot((bits[g] >> k) & 1u);
                    below[g] += (int)wave_prefix_count(m);
                    n += __popcll(m);
                }
                if (lane == 0) cnt[g * RP_WAVES + wave] = n;
            }
            const uint64_t sm = __ballot(mine_self);
            if (sm == 0) {
                if (lane == 0) s_self[par * RP_WAVES + wave] = INT_MAX;
            } else if (mine_self) {
                s_self[par * RP_WAVES + wave] = self_at;
            }
            wg_barrier();   // the only barrier of a chunk: the other half of s_cnt / s_self is written next time
            int start[RP_GROUPS];
            int total = 0, chunk_self = INT_MAX;
#pragma unroll
            for (int g = 0; g < RP_GROUPS; g++) {
                start[g] = carry + total + below[g];
#pragma unroll
                for (int w = 0; w < RP_WAVES; w++) {
                    const int n = cnt[g * RP_WAVES + w];
                    if (w < wave) start[g] += n;
                    total += n;
                }
            }
#pragma unroll
            for (int w = 0; w < RP_WAVES; w++) chunk_self = min(chunk_self, s_self[par * RP_WAVES + w]);
            // ---- write the positions of this thread's hits (about one rank in C) ----
#pragma unroll
            for (int g = 0; g < RP_GROUPS; g++)
                for (unsigned m = bits[g]; m; m &= m - 1) {
                    const int k = __ffs(m) - 1;
                    const int j = start[g] + __popc(bits[g] & ((1u << k) - 1u)) + 1;
                    const int pos = base + g * RP_GSPAN + tid * RP_VEC + k;
                    if (j <= R) out[j - 1] = pos + 1 - ((self_before || chunk_self < pos) ? 1 : 0);
                }
            carry += total;
            self_before = self_before || chunk_self != INT_MAX;
            par ^= 1;
            if (carry >= R) break;                                    // uniform: every relevant item is found
        }
        // fewer hits than hit_off promised (classes inconsistent with hit_off): the missing positions read 0
        for (int j = carry + tid; j < R; j += RP_THREADS) out[j] = 0;
    }
}

// AP of every query: (1 / R) sum_j j / p_j -- one wave per query, a fixed butterfly
__global__ __launch_bounds__(RP_THREADS) void rp_ap_kernel(const int32_t *__restrict__ hit_pos, const int64_t *__restrict__ hit_off, int64_t Q,
                                                           double *__restrict__ ap)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t q = (int64_t)blockIdx.x * RP_WAVES + wave; q < Q; q += (int64_t)gridDim.x * RP_WAVES) {
        const int64_t off = hit_off[q];
        const int R = (int)(hit_off[q + 1] - off);
        double s = 0.0;
        for (int j = lane + 1; j <= R; j += WAVE) s += (double)j / (double)hit_pos[off + j - 1];
        s = wave_sum(s);
        if (lane == 0) ap[q] = R > 0 ? s / (double)R : 0.0;
    }
}

// Unbinned sums: thread per (class c, j = 1 .. R_c) -- element class_off[c] + j - 1 of prec_sum -- over the class's queries in order
__global__ __launch_bounds__(RP_THREADS) void rp_sum_kernel(const int32_t *__restrict__ hit_pos, const int64_t *__restrict__ hit_off,
                                                            const int32_t *__restrict__ order, const int32_t *__restrict__ cstart,
                                                            const int64_t *__restrict__ class_off, int C, int64_t class_len,
                                                            double *__restrict__ prec_sum, int64_t *__restrict__ first_miss)
{
    const int64_t total = class_off[C] < class_len ? class_off[C] : class_len;
    for (int64_t g = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x; g < total; g += (int64_t)gridDim.x * RP_THREADS) {
        int lo = 0, hi = C;                       // the class whose range holds g: class_off[lo] <= g < class_off[lo + 1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (class_off[mid] <= g) lo = mid; else hi = mid;
        }
        const int j = (int)(g - class_off[lo]) + 1;
        double s = prec_sum[g];
        int64_t miss = 0;
        for (int k = cstart[lo]; k < cstart[lo + 1]; k++) {
            const int q = order[k];
            const int64_t off = hit_off[q];
            if (j <= hit_off[q + 1] - off) {
                const int p = hit_pos[off + j - 1];
                s += (double)j / (double)p;
                miss += p > 1 ? 1 : 0;
            }
        }
        prec_sum[g] = s;
        if (j == 1) first_miss[lo] += miss;
    }
}

// bin of hit j of R: int((j / R) * B), with Python's float64 operations (IEEE division, then multiplication)
__device__ __forceinline__ int rp_bin(int j, int R, int B) { return (int)(((double)j / (double)R) * (double)B); }

// smallest j in [1, R] with rp_bin(j) >= t, R + 1 if none (rp_bin is non-decreasing in j)
__device__ __forceinline__ int rp_first_bin_at_least(int t, int R, int B)
{
    int64_t e = (int64_t)t * R / B;
    int j = (int)(e < 1 ? 1 : (e > R + 1 ? R + 1 : e));
    while (j > 1 && rp_bin(j - 1, R, B) >= t) j--;
    while (j <= R && rp_bin(j, R, B) < t) j++;
    return j;
}

// Binned sums: one wave per (class, bin b = 0 .. B): per query of the class the max of j / p_j over the j of the bin (a first-position
// miss adds 0.0 to bin 0), added in query order to bin_sum; bin_count counts the queries that have the bin
__global__ __launch_bounds__(RP_THREADS) void rp_bin_kernel(const int32_t *__restrict__ hit_pos, const int64_t *__restrict__ hit_off,
                                                            const int32_t *__restrict__ order, const int32_t *__restrict__ cstart,
                                                            const int64_t *__restrict__ class_off, int C, int B, double *__restrict__ bin_sum,
                                                            int64_t *__restrict__ bin_count)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nw = (int64_t)C * (B + 1);
    for (int64_t w = (int64_t)blockIdx.x * RP_WAVES + wave; w < nw; w += (int64_t)gridDim.x * RP_WAVES) {
        const int c = (int)(w / (B + 1)), b = (int)(w % (B + 1));
        const int Rc = (int)(class_off[c + 1] - class_off[c]);
        if (Rc <= 0) continue;
        const int jlo = rp_first_bin_at_least(b, Rc, B), jhi = rp_first_bin_at_least(b + 1, Rc, B);
        if (jhi == jlo && b != 0) continue;                          // no query of the class has this bin
        double sum = bin_sum[w];
        int64_t count = bin_count[w];
        for (int k = cstart[c]; k < cstart[c + 1]; k++) {
            const int q = order[k];
            const int64_t off = hit_off[q];
            const int Rq = (int)(hit_off[q + 1] - off);
            const int end = jhi <= Rq ? jhi : Rq + 1;
            double v = 0.0;
            for (int j = jlo + lane; j < end; j += WAVE) v = fmax(v, (double)j / (double)hit_pos[off + j - 1]);
            v = wave_max(v);
            const bool has = (end > jlo) || (b == 0 && Rq > 0 && hit_pos[off] > 1);
            if (has) { sum += v; count++; }
        }
        if (lane == 0) { bin_sum[w] = sum; bin_count[w] = count; }
    }
}

}  // namespace se

using namespace se;

template <typename RT>
static int rp_positions(const char *who, const RT *rank, int64_t ldr, int64_t q, int64_t list_len, const int32_t *cls, int64_t gallery,
                        const int32_t *qcls, const int32_t *qidx, int num_classes, const int64_t *hit_off, int32_t *hit_pos, se_stream_t stream)
{
    if (sizeof(RT) == 2 && gallery > 65536) return fail(SE_ERR_INVALID, "%s: a gallery of %lld items does not fit 16-bit ranks", who, (long long)gallery);
    if (q < 0 || list_len <= 0 || gallery <= 0 || num_classes <= 0 || q > 0x7FFFFFFF || list_len > 0x7FFFFFFF - 2 * RP_CHUNK)
        return fail(SE_ERR_INVALID, "%s: bad shape q=%lld len=%lld gallery=%lld classes=%d", who, (long long)q, (long long)list_len,
                    (long long)gallery, num_classes);
    if (!rank || !cls || !qcls || !hit_off || !hit_pos) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if (ldr < list_len) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    if (q == 0) return SE_OK;
    const ClassTable ct = choose_class_table(list_len, q, gallery, num_classes, RP_HEAD_INTS * sizeof(int));
    const int vec_ok = ranks_vec_ok<RT, RP_VEC>(rank, ldr);
    return dispatch_clsw(ct.clsw, [&](auto w) -> int {
        const auto kernel = relpos_kernel<decltype(w)::value, RT>;
        int64_t grid = 0;
        SE_HIP_CHECK(persistent_grid(kernel, RP_THREADS, ct.lds_bytes, q, &grid));
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(RP_THREADS), ct.lds_bytes, (hipStream_t)stream, rank, ldr, q, list_len, cls, gallery,
                           qcls, qidx, hit_off, hit_pos, vec_ok);
        SE_LAUNCH_CHECK();
        return SE_OK;
    });
}

extern "C" int se_relevant_positions(const int32_t *rank, int64_t ldr, int64_t q, int64_t list_len, const int32_t *cls, int64_t gallery,
                                     const int32_t *qcls, const int32_t *qidx, int num_classes, const int64_t *hit_off, int32_t *hit_pos,
                                     se_stream_t stream)
{
    return rp_positions<int32_t>("se_relevant_positions", rank, ldr, q, list_len, cls, gallery, qcls, qidx, num_classes, hit_off, hit_pos, stream);
}

extern "C" int se_relevant_positions_r16(const uint16_t *rank, int64_t ldr, int64_t q, int64_t list_len, const int32_t *cls, int64_t gallery,
                                         const int32_t *qcls, const int32_t *qidx, int num_classes, const int64_t *hit_off, int32_t *hit_pos,
                                         se_stream_t stream)
{
    return rp_positions<uint16_t>("se_relevant_positions_r16", rank, ldr, q, list_len, cls, gallery, qcls, qidx, num_classes, hit_off, hit_pos, stream);
}

extern "C" int se_recall_precision_reduce(const int32_t *hit_pos, const int64_t *hit_off, int64_t q, const int32_t *order,
                                          const int32_t *class_start, int num_classes, const int64_t *class_off, int64_t class_len,
                                          int bins, double *ap, double *prec_sum, int64_t *first_miss, double *bin_sum,
                                          int64_t *bin_count, se_stream_t stream)
{
    if (q < 0 || q > 0x7FFFFFFF || num_classes <= 0 || class_len < 0 || bins < 0 || bins > RP_MAX_BINS)
        return fail(SE_ERR_INVALID, "se_recall_precision_reduce: bad shape q=%lld classes=%d class_len=%lld bins=%d", (long long)q,
                    num_classes, (long long)class_len, bins);
    if (!hit_pos || !hit_off || !order || !class_start || !class_off || !ap || !prec_sum || !first_miss || (bins > 0 && (!bin_sum || !bin_count)))
        return fail(SE_ERR_INVALID, "se_recall_precision_reduce: null pointer");
    if (q == 0) return SE_OK;
    hipStream_t s = (hipStream_t)stream;
    int64_t g = (q + RP_WAVES - 1) / RP_WAVES;
    hipLaunchKernelGGL(rp_ap_kernel, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(RP_THREADS), 0, s, hit_pos, hit_off, q, ap);
    SE_LAUNCH_CHECK();
    if (class_len > 0) {
        g = (class_len + RP_THREADS - 1) / RP_THREADS;
        hipLaunchKernelGGL(rp_sum_kernel, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(RP_THREADS), 0, s, hit_pos, hit_off, order, class_start,
                           class_off, num_classes, class_len, prec_sum, first_miss);
        SE_LAUNCH_CHECK();
    }
    if (bins > 0) {
        g = ((int64_t)num_classes * (bins + 1) + RP_WAVES - 1) / RP_WAVES;
        hipLaunchKernelGGL(rp_bin_kernel, dim3((unsigned)(g < 8192 ? g : 8192)), dim3(RP_THREADS), 0, s, hit_pos, hit_off, order, class_start,
                           class_off, num_classes, bins, bin_sum, bin_count);
        SE_LAUNCH_CHECK();
    }
    return SE_OK;
}
