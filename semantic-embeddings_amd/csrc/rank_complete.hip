// rank_complete.hip -- completion of given (possibly partial) ranked lists to whole-gallery rankings: se_complete_rankings.
//
// Replaces: `ret = ret + [id for id in all_ids if id not in sret]` (class_hierarchy.py:262-264), the per-query Python set and list
// comprehension over all_ids of ClassHierarchy.hierarchical_precision, for a tile of queries at once.
//
// complete_rankings_kernel: a capped grid of 256-thread workgroups, each looping over rows.  Per row:
//   clear    a membership bitmap of `gallery` bits -- in LDS for galleries up to SE_COMPLETE_LDS_ITEMS (32 KB), above that in the
//            workgroup's own slice of the workspace -- and the row's flag word.  EVERY row clears it: a workgroup handles many rows.
//   phase 1  stride over the list's valid entries: an entry is range-checked, THEN used as a bit position of a returning integer OR
//            (the old bit tells of a duplicate), and stored to the front of the output row (bounded by `gallery`).  Range failures
//            and duplicates OR their bit into the workgroup's flag word.
//   phase 2  flag set: the row is overwritten with `order` (nothing of the list is kept, so the result does not depend on which
//            lane met a duplicate first).  A clean list of `gallery` entries is complete already.  Otherwise each wave owns a contiguous segment of `order` (whole 64-element chunks),
//            counts its absent elements (order == NULL: a popcount over the bitmap's words), one barrier exchanges the four counts,
//            and each wave writes its segment's absent elements at its offset, a ballot / mbcnt prefix per 64-element chunk.
// Integers only; the bitmap operations are integer atomics whose combined result does not depend on their order, and every output
// position is a function of the inputs alone: the same inputs give the same bits on every launch geometry.  Nothing here rests on
// the lane-order property that se_rank_rows_init probes.
//
// The workspace bitmap is written and read with agent-scope atomic operations only: its OR runs in L2, so a plain load could hit
// a line that the vector L1 kept from the previous row of the same workgroup.
#include "se_common.h"

namespace se {

constexpr int CR_THREADS = 256;
constexpr int CR_WAVES = CR_THREADS / WAVE;
constexpr int CR_BLOCKS_PER_CU = 8;              // grid cap of the LDS form
constexpr int64_t CR_WS_BLOCKS = 1024;           // grid cap of the workspace form: one bitmap slice each
constexpr int CR_BAD_RANGE = 1, CR_BAD_DUP = 2;  // status bits

inline int64_t cr_slice_words(int64_t gallery) { return ((gallery + 31) / 32 + 63) / 64 * 64; }      // 256-byte slices

template <bool WS>
__device__ __forceinline__ void bm_clear(uint32_t *bm, int w)
{
    if constexpr (WS) __hip_atomic_store(bm + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else bm[w] = 0u;
}

template <bool WS>
__device__ __forceinline__ uint32_t bm_or(uint32_t *bm, int w, uint32_t bit)
{
    if constexpr (WS) return __hip_atomic_fetch_or(bm + w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return atomicOr(bm + w, bit);
}

template <bool WS>
__device__ __forceinline__ uint32_t bm_load(const uint32_t *bm, int w)
{
    if constexpr (WS) return __hip_atomic_load(bm + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return bm[w];
}

// phase 1 for one entry: range check, then the bit; returns the entry's status bits
template <bool WS>
__device__ __forceinline__ int cr_mark(uint32_t *bm, int32_t g, int gallery)
{
    if ((uint32_t)g >= (uint32_t)gallery) return CR_BAD_RANGE;
    const uint32_t bit = 1u << (g & 31);
    return (bm_or<WS>(bm, g >> 5, bit) & bit) ? CR_BAD_DUP : 0;
}

// WS: bitmap in the workspace.  VEC: list and output rows are 16-byte aligned (base and pitch).  ORD: order != NULL.
template <bool WS, bool VEC, bool ORD>
__global__ __launch_bounds__(CR_THREADS) void complete_rankings_kernel(const int32_t *__restrict__ lists, int64_t ldl, const int32_t *__restrict__ len,
                                                                       int64_t Q, int list_len, const int32_t *__restrict__ order, int gallery,
                                                                       int32_t *__restrict__ rank, int64_t ldr, int32_t *__restrict__ status,
                                                                       uint32_t *__restrict__ ws, int64_t slice_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t cr_lds[];
    __shared__ int flag;
    __shared__ int wave_cnt[CR_WAVES];
    uint32_t *bm = WS ? ws + (int64_t)blockIdx.x * slice_words : cr_lds;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const int words = (gallery + 31) >> 5;
    const int chunks = (gallery + WAVE - 1) / WAVE;                 // 64-element chunks of `order`
    const int cpw = (chunks + CR_WAVES - 1) / CR_WAVES;             // chunks per wave
    const int c0 = wave * cpw < chunks ? wave * cpw : chunks, c1 = c0 + cpw < chunks ? c0 + cpw : chunks;

    for (int64_t row = blockIdx.x; row < Q; row += gridDim.x) {
        for (int w = tid; w < words; w += CR_THREADS) bm_clear<WS>(bm, w);
        if (tid == 0) flag = 0;
        wg_barrier();

        int n = len ? len[row] : list_len;
        n = n < 0 ? 0 : (n > list_len ? list_len : n);              // nothing is read beyond the row, whatever len says
        const int32_t *list = lists + row * ldl;
        int32_t *out = rank + row * ldr;
        int bad = 0;
        if constexpr (VEC) {
            const int n4 = n & ~3;
            for (int e = tid * 4; e < n4; e += CR_THREADS * 4) {
                const int4 v = *(const int4 *)(list + e);
                bad |= cr_mark<WS>(bm, v.x, gallery) | cr_mark<WS>(bm, v.y, gallery) | cr_mark<WS>(bm, v.z, gallery) | cr_mark<WS>(bm, v.w, gallery);
                if (e + 4 <= gallery) {
                    *(int4 *)(out + e) = v;
                } else {                                            // (a list longer than the gallery: the row is flagged anyway)
                    if (e < gallery) out[e] = v.x;
                    if (e + 1 < gallery) out[e + 1] = v.y;
                    if (e + 2 < gallery) out[e + 2] = v.z;
                }
            }
            for (int e = n4 + tid; e < n; e += CR_THREADS) {
                const int32_t g = list[e];
                bad |= cr_mark<WS>(bm, g, gallery);
                if (e < gallery) out[e] = g;
            }
        } else {
            for (int e = tid; e < n; e += CR_THREADS) {
                const int32_t g = list[e];
                bad |= cr_mark<WS>(bm, g, gallery);
                if (e < gallery) out[e] = g;
            }
        }
        if (bad) atomicOr(&flag, bad);
        wg_barrier();

        const int st = flag;
        if (tid == 0) status[row] = st;
        if (st) {
            // a bad row as a whole becomes `order`: a valid permutation that means nothing
            for (int e = tid; e < gallery; e += CR_THREADS) out[e] = ORD ? order[e] : e;
        } else if (n < gallery) {       // (n is the same in every thread; a clean row of `gallery` entries is complete as it stands)
            // a clean row: n distinct entries of [0, gallery) are in place, gallery - n elements of `order` are absent
            int cnt = 0;
            if constexpr (ORD) {
                for (int c = c0; c < c1; c++) {
                    const int e = c * WAVE + lane;
                    const int32_t o = e < gallery ? order[e] : -1;
                    const bool in = (uint32_t)o < (uint32_t)gallery;
                    const bool absent = in && !((bm_load<WS>(bm, in ? o >> 5 : 0) >> (o & 31)) & 1u);
                    cnt += __popcll(__ballot(absent));
                }
            } else {
                const int w1 = 2 * c1 < words ? 2 * c1 : words;
                for (int w = 2 * c0 + lane; w < w1; w += WAVE) {
                    const int left = gallery - w * 32;              // valid bits of the last word
                    const uint32_t valid = left >= 32 ? 0xFFFFFFFFu : ((1u << left) - 1u);
                    cnt += __popc(~bm_load<WS>(bm, w) & valid);
                }
                cnt = wave_sum(cnt);
            }
            if (lane == 0) wave_cnt[wave] = cnt;
            wg_barrier();
            int off = n;
            for (int w = 0; w < wave; w++) off += wave_cnt[w];
            for (int c = c0; c < c1; c++) {
                const int e = c * WAVE + lane;
                const int32_t o = e < gallery ? (ORD ? order[e] : e) : -1;
                const bool in = (uint32_t)o < (uint32_t)gallery;    // (an element of `order` outside [0, gallery) is never written)
                const bool absent = in && !((bm_load<WS>(bm, in ? o >> 5 : 0) >> (o & 31)) & 1u);
                const uint64_t ballot = __ballot(absent);
                const int pos = off + (int)wave_prefix_count(ballot);
                if (absent && pos < gallery) out[pos] = o;
                off += __popcll(ballot);
            }
        }
        wg_barrier();       // the bitmap, the flag and the counts are read to here; the next row clears them
    }
}

}  // namespace se

using namespace se;

extern "C" int64_t se_complete_rankings_workspace_bytes(int64_t q, int64_t gallery)
{
    if (q <= 0 || gallery <= SE_COMPLETE_LDS_ITEMS) return 0;
    return (q < CR_WS_BLOCKS ? q : CR_WS_BLOCKS) * cr_slice_words(gallery) * (int64_t)sizeof(uint32_t);
}

extern "C" int se_complete_rankings(const int32_t *lists, int64_t ldl, const int32_t *len, int64_t q, int64_t list_len, const int32_t *order,
                                    int64_t gallery, int32_t *rank, int64_t ldr, int32_t *status, void *workspace, int64_t workspace_bytes,
                                    se_stream_t stream)
{
    if (q < 0 || list_len < 0 || gallery < 0 || workspace_bytes < 0 || list_len > SE_COMPLETE_MAX_ITEMS || gallery > SE_COMPLETE_MAX_ITEMS)
        return fail(SE_ERR_INVALID, "se_complete_rankings: bad shape q=%lld list_len=%lld gallery=%lld workspace_bytes=%lld", (long long)q,
                    (long long)list_len, (long long)gallery, (long long)workspace_bytes);
    if (q == 0 || gallery == 0) return SE_OK;
    if ((!lists && list_len > 0) || !rank || !status) return fail(SE_ERR_INVALID, "se_complete_rankings: null pointer");
    if (ldl < list_len) return fail(SE_ERR_INVALID, "se_complete_rankings: leading dimension ldl=%lld below list_len=%lld", (long long)ldl, (long long)list_len);
    if (ldr < gallery) return fail(SE_ERR_INVALID, "se_complete_rankings: leading dimension ldr=%lld below gallery=%lld", (long long)ldr, (long long)gallery);
    const bool in_ws = gallery > SE_COMPLETE_LDS_ITEMS;
    const int64_t need = se_complete_rankings_workspace_bytes(q, gallery);
    if (in_ws && (!workspace || workspace_bytes < need || (((uintptr_t)workspace) & 3) != 0))
        return fail(SE_ERR_INVALID, "se_complete_rankings: the workspace holds %lld bytes, %lld are needed (4-byte aligned)", (long long)workspace_bytes,
                    (long long)need);
    const int64_t cap = in_ws ? CR_WS_BLOCKS : (int64_t)num_cus() * CR_BLOCKS_PER_CU;
    const unsigned blocks = row_blocks(q, 1, cap);
    const size_t lds = in_ws ? 0 : (size_t)((gallery + 31) / 32) * sizeof(uint32_t);
    const bool vec = list_len > 0 && aligned16(lists, ldl, 4) && aligned16(rank, ldr, 4);
    dispatch_bools(in_ws, vec, order != nullptr, [&](auto cws, auto cvec, auto cord) {
        hipLaunchKernelGGL((complete_rankings_kernel<cws.value, cvec.value, cord.value>), dim3(blocks), dim3(CR_THREADS), lds, (hipStream_t)stream,
                           lists, ldl, len, q, (int)list_len, order, (int)gallery, rank, ldr, status, (uint32_t *)workspace, cr_slice_words(gallery));
    });
    SE_LAUNCH_CHECK();
    return SE_OK;
}
