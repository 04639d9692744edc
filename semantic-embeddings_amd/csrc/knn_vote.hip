// knn_vote.hip -- k-nearest-neighbour classification: the vote over the neighbour lists of se_retrieve_topk / se_topk_merge.
//
// Replaces the host composition sklearn.neighbors.KNeighborsClassifier(weights='uniform').predict / predict_proba on brute-force
// neighbour lists (the reference has no k-NN line): for every query and every cut-off k, the classes of its first k neighbours are
// counted and the `top` classes with the most votes are written, ties in ascending class index.
//
// knn_vote_kernel: ONE WAVE per query, up to 4 queries per workgroup.  A query's votes live in a wave-private open-addressing table
// in LDS -- `slots` (class, votes) pairs, slots = the power of two >= 2 * list_len (at least 64) -- so the LDS a query needs follows
// the list length (8 bytes per slot: 4 KB for 200 neighbours, 32 KB for SE_TOPK_MAX), not the number of classes, which is
// unlimited.  The list is walked ONCE, 64 entries per step: a ballot of the entries that count as neighbours gives every lane its
// entry's ordinal among them, lanes whose ordinal lies below the current cut-off insert their class (integer LDS compare-and-swap
// on the key, integer add on the votes; linear probing; the table is at most half full), and whenever a step completes a cut-off
// the ranking of the table is written before the walk goes on: `top` arg-max passes over the slots, each a wave reduction of the
// packed key (votes << 32) | ~class among the keys below the previous pass's.  Classes without a vote fill the tail in ascending
// class index.  Everything is an integer and nothing depends on which slot a class landed in, so the same inputs give the same
// bits on every launch geometry.  The table is private to its wave and a wave's LDS operations execute in order: the kernel has no
// workgroup barrier.
#include "se_common.h"

namespace se {

constexpr int KV_MAX_QUERIES = 4;                  // waves (queries) per workgroup
constexpr int KV_LDS_MAX = 64 * 1024;              // dynamic LDS a workgroup may own without a function attribute
constexpr int KV_MIN_SLOTS = 64;
constexpr int32_t KV_EMPTY = -1;

struct KnnCuts {
    int n;
    int k[SE_KNN_KS_MAX];
};

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// The ranking of the wave's table for cut-off j of query `row`: lane t < top writes entry t of out_cls / out_votes.
__device__ __forceinline__ void knn_emit(const int32_t *keys, const int32_t *votes, int slots, int top, int num_classes, int lane,
                                         int32_t *__restrict__ oc, int32_t *__restrict__ ov)
{
    uint64_t below = ~0ull;         // keys of this pass lie strictly below the previous pass's
    int32_t my_cls = 0, my_votes = 0;
    int found = 0;
    for (; found < top; found++) {
        uint64_t best = 0;          // (a voted class has votes >= 1: its key is never 0)
        for (int s = lane; s < slots; s += WAVE) {
            const int32_t c = keys[s];
            if (c == KV_EMPTY) continue;
            const uint64_t key = ((uint64_t)(uint32_t)votes[s] << 32) | (uint32_t)~c;
            if (key < below && key > best) best = key;
        }
        best = wave_max_u64(best);
        if (best == 0) break;       // every voted class is out
        if (lane == found) {
            my_cls = (int32_t)~(uint32_t)best;
            my_votes = (int32_t)(best >> 32);
        }
        below = best;
    }
    if (found < top) {
        // zero-vote tail: the smallest classes that are not among the `found` < top <= 16 voted ones, all of which are in lanes
        // 0 .. found - 1.  At most `found` of the classes 0 .. 31 are voted, so 32 candidates always hold top - found free ones.
        bool is_free = lane < 32 && lane < num_classes;         // lane l stands for class l
        for (int t = 0; t < found; t++) {
            const int32_t voted = __shfl(my_cls, t, 64);        // (every lane takes part: no shuffle behind a lane's own condition)
            is_free = is_free && voted != lane;
        }
        uint64_t free_classes = __ballot(is_free);
        if (lane >= found && lane < top) {                      // entry `lane` is the (lane - found)-th free class
            for (int r = found; r < lane; r++) free_classes &= free_classes - 1;
            my_cls = __ffsll((unsigned long long)free_classes) - 1;
            my_votes = 0;
        }
    }
    if (lane < top) {
        oc[lane] = my_cls;
        ov[lane] = my_votes;
    }
}

__global__ __launch_bounds__(KV_MAX_QUERIES * WAVE) void knn_vote_kernel(const int32_t *__restrict__ idx, int64_t ldi, int64_t Q, int list_len,
                                                                         const int32_t *__restrict__ cls, int64_t gallery, int num_classes,
                                                                         const int32_t *__restrict__ qidx, KnnCuts cuts, int top, int slots,
                                                                         int32_t *__restrict__ out_cls, int32_t *__restrict__ out_votes)
{
    extern __shared__ __attribute__((aligned(16))) int32_t kv_lds[];
    const int lane = lane_id(), wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    int32_t *keys = kv_lds + (size_t)wave * 2 * slots, *votes = keys + slots;
    const uint32_t mask = (uint32_t)slots - 1u;
    const int shift = 1 + __builtin_clz((unsigned)slots);      // 32 - log2(slots) <= 26: the hash keeps the top bits of the product
    const int nk = cuts.n;

    for (int64_t row = (int64_t)blockIdx.x * waves + wave; row < Q; row += (int64_t)gridDim.x * waves) {
        for (int s = lane; s < slots; s += WAVE) {
            keys[s] = KV_EMPTY;
            votes[s] = 0;
        }
        __builtin_amdgcn_wave_barrier();
        const int32_t self = qidx ? qidx[row] : -1;       // (an entry < 0 is never a neighbour: -1 skips nothing else)
        const int32_t *list = idx + row * ldi;
        int32_t *oc = out_cls + row * (int64_t)nk * top, *ov = out_votes + row * (int64_t)nk * top;
        int j = 0;
        int base = 0;       // neighbours before this step
        int done = 0;       // neighbours that have voted
        for (int pos = 0; pos < list_len && j < nk; pos += WAVE) {
            const int e = pos + lane;
            const int32_t g = e < list_len ? list[e] : -1;
            const bool voter = g >= 0 && (int64_t)g < gallery && g != self;
            const uint64_t ballot = __ballot(voter);
            const int ord = base + (int)wave_prefix_count(ballot);
            const int total = base + __popcll(ballot);
            const int32_t c = voter ? cls[g] : -1;
            const bool votes_ok = voter && c >= 0 && c < num_classes;
            while (j < nk) {
                const int kj = cuts.k[j];
                if (votes_ok && ord >= done && ord < kj) {
                    uint32_t h = ((uint32_t)c * 2654435761u) >> shift;
                    for (;;) {
                        const int32_t prev = atomicCAS(&keys[h], KV_EMPTY, c);
                        if (prev == KV_EMPTY || prev == c) {
                            atomicAdd(&votes[h], 1);
                            break;
                        }
                        h = (h + 1u) & mask;
                    }
                }
                done = total < kj ? total : kj;
                if (total < kj) break;
                __builtin_amdgcn_wave_barrier();
                knn_emit(keys, votes, slots, top, num_classes, lane, oc + (int64_t)j * top, ov + (int64_t)j * top);
                j++;
            }
            base = total;
        }
        // the list holds fewer neighbours than the remaining cut-offs: all of them have voted
        __builtin_amdgcn_wave_barrier();
        for (; j < nk; j++) knn_emit(keys, votes, slots, top, num_classes, lane, oc + (int64_t)j * top, ov + (int64_t)j * top);
    }
}

}  // namespace se

using namespace se;

extern "C" int se_knn_vote(const int32_t *idx, int64_t ldi, int64_t q, int64_t list_len, const int32_t *cls, int64_t gallery, int num_classes,
                           const int32_t *qidx, const int32_t *ks, int nk, int top, int32_t *out_cls, int32_t *out_votes,
                           se_stream_t stream)
{
    if (q < 0 || nk < 0 || list_len < 0 || gallery < 0)
        return fail(SE_ERR_INVALID, "se_knn_vote: bad shape q=%lld list_len=%lld gallery=%lld nk=%d", (long long)q, (long long)list_len,
                    (long long)gallery, nk);
    if (q == 0 || nk == 0) return SE_OK;
    if (!idx || !cls || !ks || !out_cls || !out_votes) return fail(SE_ERR_INVALID, "se_knn_vote: null pointer");
    if (list_len < 1 || list_len > SE_TOPK_MAX)
        return fail(SE_ERR_INVALID, "se_knn_vote: list_len=%lld outside [1, %d]", (long long)list_len, SE_TOPK_MAX);
    if (ldi < list_len) return fail(SE_ERR_INVALID, "se_knn_vote: leading dimension %lld below list_len=%lld", (long long)ldi, (long long)list_len);
    if (num_classes < 1) return fail(SE_ERR_INVALID, "se_knn_vote: num_classes=%d", num_classes);
    if (top < 1 || top > SE_KNN_TOP_MAX || top > num_classes)
        return fail(SE_ERR_INVALID, "se_knn_vote: top=%d outside [1, min(%d, num_classes=%d)]", top, SE_KNN_TOP_MAX, num_classes);
    if (nk > SE_KNN_KS_MAX) return fail(SE_ERR_UNSUPPORTED, "se_knn_vote: %d cut-offs, at most %d per call", nk, SE_KNN_KS_MAX);
    KnnCuts cuts;
    cuts.n = nk;
    for (int j = 0; j < nk; j++) {
        if (ks[j] < 1 || ks[j] > list_len || (j > 0 && ks[j] <= ks[j - 1]))
            return fail(SE_ERR_INVALID, "se_knn_vote: cut-offs must ascend within [1, list_len=%lld] (ks[%d]=%d)", (long long)list_len, j, ks[j]);
        cuts.k[j] = ks[j];
    }
    for (int j = nk; j < SE_KNN_KS_MAX; j++) cuts.k[j] = 0;
    int slots = KV_MIN_SLOTS;
    while (slots < 2 * list_len) slots *= 2;
    const int bytes_per_query = slots * 2 * (int)sizeof(int32_t);
    int per_block = KV_LDS_MAX / bytes_per_query;        // >= 2: 32 KB per query at SE_TOPK_MAX
    if (per_block > KV_MAX_QUERIES) per_block = KV_MAX_QUERIES;
    const unsigned blocks = row_blocks(q, per_block, (int64_t)num_cus() * 16);
    hipLaunchKernelGGL(knn_vote_kernel, dim3(blocks), dim3(per_block * WAVE), (size_t)per_block * bytes_per_query, (hipStream_t)stream, idx, ldi, q,
                       (int)list_len, cls, gallery, num_classes, qidx, cuts, top, slots, out_cls, out_votes);
    SE_LAUNCH_CHECK();
    return SE_OK;
}
