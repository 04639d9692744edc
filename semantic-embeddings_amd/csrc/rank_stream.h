// rank_stream.h -- what the kernels that stream rankings share (hprec.hip, ndcg.hip, recprec.hip): persistent workgroups that walk
// the rows `se_rank_rows` wrote, N consecutive ranks per thread and load, and turn every rank into the class of that gallery item.
// One copy of: the class table in LDS and its look-up, the vector load of a thread's ranks with its alignment rule, the host rule
// that picks the table, and the launch of a persistent grid; for the metric kernels also the sorted cut-off list and the search
// for the query's own entry (ndcg.hip calls them; hprec_kernel keeps the forms it was measured with).
#pragma once
#include "se_common.h"

namespace se {

// ---- device ----

// CLSW: where the class of a ranked gallery item comes from -- 1 / 2: a byte / 16-bit copy of `cls` in LDS, filled once per
// (persistent) workgroup; 0: gathered from global memory (galleries too large for LDS, or too little work to pay for the fill).
// The random 4-byte gather costs a 128-byte L2 -> L1 line per rank, 32x the ranking itself.
// The fill, by the THREADS threads of the workgroup (tid: threadIdx.x; no barrier: the caller's); lds: 16-byte aligned,
// choose_class_table's bytes.  DEPTH: loads a thread keeps in flight -- what the kernel's registers allow without costing it a
// resident wave: 8 under hprec_kernel's 256-register bound, 2 in relpos_kernel (45 - 47 VGPRs, eight waves per SIMD).
template <int CLSW, int THREADS, int DEPTH = 8>
__device__ __forceinline__ void fill_class_table(const int32_t *__restrict__ cls, int64_t gallery, unsigned char *lds, const int tid)
{
    unsigned *w = reinterpret_cast<unsigned *>(lds);
    if constexpr (CLSW == 1) {
        const int64_t quads = (reinterpret_cast<uintptr_t>(cls) % 16 == 0) ? gallery / 4 : 0;     // 16-byte loads when `cls` allows
        const int4 *c4 = reinterpret_cast<const int4 *>(cls);
#pragma unroll DEPTH
        for (int64_t g = tid; g < quads; g += THREADS) {
            const int4 v = c4[g];
            w[g] = ((unsigned)v.x & 0xFFu) | (((unsigned)v.y & 0xFFu) << 8) | (((unsigned)v.z & 0xFFu) << 16) | (((unsigned)v.w & 0xFFu) << 24);
        }
        for (int64_t i = quads * 4 + (int64_t)tid * 4; i < gallery; i += THREADS * 4) {
            unsigned v = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) v |= (i + e < gallery ? (unsigned)cls[i + e] & 0xFFu : 0u) << (8 * e);
            w[i >> 2] = v;
        }
    } else if constexpr (CLSW == 2) {
#pragma unroll DEPTH
        for (int64_t i = (int64_t)tid * 2; i < gallery; i += THREADS * 2)
            w[i >> 1] = ((unsigned)cls[i] & 0xFFFFu) | ((i + 1 < gallery ? (unsigned)cls[i + 1] & 0xFFFFu : 0u) << 16);
    }
}

// class of gallery item v; a dead slot (live == false: v is not a rank) reads table entry v (v = 0 there) or, without a table, `dead`
template <int CLSW>
__device__ __forceinline__ int class_of(const unsigned char *lds, const int32_t *__restrict__ cls, int v, bool live, int dead)
{
    if constexpr (CLSW == 1) return lds[v];
    else if constexpr (CLSW == 2) return reinterpret_cast<const unsigned short *>(lds)[v];
    else return live ? cls[v] : dead;
}

// dst = row[at .. at + N) (0 from `bound` on).  vec_ok (ranks_vec_ok<RT, N>) and a full run: int32_t ranks by N / 4 16-byte loads,
// uint16_t ranks by one 8-byte load (N = 4) or N / 8 16-byte loads; otherwise element by element.
template <class RT, int N>
__device__ __forceinline__ void load_ranks(int (&dst)[N], const RT *__restrict__ row, int at, int bound, int vec_ok)
{
    static_assert((sizeof(RT) == 4 && N % 4 == 0) || (sizeof(RT) == 2 && (N == 4 || N % 8 == 0)), "int32_t or uint16_t ranks, whole vector loads");
    if (vec_ok && at + N <= bound) {
        if constexpr (sizeof(RT) == 2 && N == 4) {
            const uint2 a = *reinterpret_cast<const uint2 *>(row + at);
            dst[0] = (int)(a.x & 0xFFFFu); dst[1] = (int)(a.x >> 16); dst[2] = (int)(a.y & 0xFFFFu); dst[3] = (int)(a.y >> 16);
        } else if constexpr (sizeof(RT) == 2) {
#pragma unroll
            for (int v = 0; v < N / 8; v++) {
                const uint4 a = *reinterpret_cast<const uint4 *>(row + at + 8 * v);
                dst[8 * v] = (int)(a.x & 0xFFFFu); dst[8 * v + 1] = (int)(a.x >> 16); dst[8 * v + 2] = (int)(a.y & 0xFFFFu); dst[8 * v + 3] = (int)(a.y >> 16);
                dst[8 * v + 4] = (int)(a.z & 0xFFFFu); dst[8 * v + 5] = (int)(a.z >> 16); dst[8 * v + 6] = (int)(a.w & 0xFFFFu); dst[8 * v + 7] = (int)(a.w >> 16);
            }
        } else {
#pragma unroll
            for (int v = 0; v < N / 4; v++) {
                const int4 a = *reinterpret_cast<const int4 *>(row + at + 4 * v);
                dst[4 * v] = a.x; dst[4 * v + 1] = a.y; dst[4 * v + 2] = a.z; dst[4 * v + 3] = a.w;
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < N; e++) dst[e] = (at + e < bound) ? (int)row[at + e] : 0;
    }
}

// The cut-offs of a metric kernel, once per workgroup: s_ks[0 .. nk) = ks ascending (ties keep the caller's order), s_perm = the
// slot of each in the caller's order.  Returns whether ks is 1, 2, ..., nk in that order (the CLI's case: effective rank j then IS
// slot j and nothing is looked up).  nk <= MAX_KS; s_flag: one int of LDS.  Holds barriers: every thread of the workgroup calls it.
template <int THREADS, int MAX_KS>
__device__ __forceinline__ bool sort_cutoffs(const int32_t *__restrict__ ks, int nk, int *s_ks, int *s_perm, int *s_flag, const int tid)
{
    constexpr int PER = (MAX_KS + THREADS - 1) / THREADS;
    for (int s = tid; s < nk; s += THREADS) s_perm[s] = ks[s];      // raw copy, ranked by counting below
    if (tid == 0) *s_flag = 1;
    wg_barrier();
    int mine[PER], at[PER];
#pragma unroll
    for (int v = 0; v < PER; v++) {
        const int s = tid + v * THREADS;
        mine[v] = s < nk ? s_perm[s] : 0;
        at[v] = 0;
        if (s < nk)
            for (int u = 0; u < nk; u++) { const int o = s_perm[u]; at[v] += (o < mine[v] || (o == mine[v] && u < s)) ? 1 : 0; }
    }
    wg_barrier();
#pragma unroll
    for (int v = 0; v < PER; v++) {
        const int s = tid + v * THREADS;
        if (s < nk) {
            s_ks[at[v]] = mine[v]; s_perm[at[v]] = s;
            if (mine[v] != s + 1) *s_flag = 0;
        }
    }
    wg_barrier();
    return *s_flag != 0;
}

// Position of the first entry of row[0 .. len) equal to `self`, or len: what a kernel that drops the query from its own ranking
// needs before it walks the row.  The common answers cost no pass -- self < 0 (not a gallery item) and self first in its own row;
// otherwise block by block with a uniform early exit.  s_pos: one int of LDS.  Holds barriers: every thread of the workgroup calls it.
template <int THREADS, class RT>
__device__ __forceinline__ int find_own_entry(const RT *__restrict__ row, int len, int32_t self, int *s_pos, const int tid)
{
    const int32_t first = (self >= 0 && len > 0) ? (int32_t)row[0] : -1;
    if (tid == 0) *s_pos = (self >= 0 && first == self) ? 0 : 0x7FFFFFFF;
    wg_barrier();
    if (self >= 0 && first != self) {
        for (int b0 = 0; b0 < len; b0 += 4 * THREADS) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int i = b0 + e * THREADS + tid;
                if (i < len && (int32_t)row[i] == self) atomicMin(s_pos, i);
            }
            wg_barrier();
            const int found = *s_pos;       // into a register before the second barrier: no wave may start the next block's atomicMin
            wg_barrier();                   // while another has yet to read the flag (they would leave the loop at different blocks)
            if (found != 0x7FFFFFFF) break;
        }
    }
    const int pos = *s_pos;
    return pos == 0x7FFFFFFF ? len : pos;
}

// ---- host ----

// load_ranks<RT, N> may use its vector loads: base and row pitch are multiples of the load's bytes
template <class RT, int N>
inline int ranks_vec_ok(const RT *rank, int64_t ldr)
{
    constexpr int64_t bytes = N * sizeof(RT) < 16 ? N * sizeof(RT) : 16;
    return ((ldr * (int64_t)sizeof(RT)) % bytes == 0) && (reinterpret_cast<uintptr_t>(rank) % bytes == 0);
}

// The class table of a launch and the dynamic LDS of a workgroup: the gallery's classes as bytes / shorts in LDS when they fit next
// to the kernel's own `fixed_lds_bytes`, else gathered (clsw = 0).
constexpr size_t CLASS_TABLE_LDS_CAP = 160 * 1024;
struct ClassTable { int clsw; size_t lds_bytes; };
inline ClassTable choose_class_table(int64_t list_len, int64_t q, int64_t gallery, int num_classes, size_t fixed_lds_bytes)
{
    const size_t tab8 = ((size_t)gallery + 15) / 16 * 16, tab16 = ((size_t)gallery * 2 + 15) / 16 * 16;
    if (list_len * (q < 4096 ? q : 4096) < 8 * gallery) return {0, fixed_lds_bytes};   // short lists / few queries: filling the table would cost more than the gathers
    if (num_classes <= 256 && fixed_lds_bytes + tab8 <= CLASS_TABLE_LDS_CAP) return {1, fixed_lds_bytes + tab8};
    if (num_classes <= 65536 && fixed_lds_bytes + tab16 <= CLASS_TABLE_LDS_CAP) return {2, fixed_lds_bytes + tab16};
    return {0, fixed_lds_bytes};
}

// Grid of persistent workgroups that each take one of q rows at a time: as many as are resident at once, q at the most.  Also allows
// the kernel its `lds` bytes of dynamic LDS.
template <class K>
inline hipError_t persistent_grid(K kernel, int threads, size_t lds, int64_t q, int64_t *grid)
{
    int per_cu = 0;
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds);
    const int64_t resident = (int64_t)(per_cu < 1 ? 1 : per_cu) * num_cus();
    *grid = q < resident ? q : resident;
    return e;
}

}  // namespace se
