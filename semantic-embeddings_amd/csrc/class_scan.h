// class_scan.h -- the fixed-order scan over the batch rows of one class, for the gradients that sum over {i : label_i = k} "from +0 in
// INCREASING i" (center_loss.hip: the centroids; labelembed.hip: the label-embedding table).  One wave owns class k: it reads the
// labels 64 at a time, ballots the lanes whose row belongs to k and walks the set bits in ascending order, so every element of the
// owner's row sees its class's rows in batch order and the rows of other classes are never read.  No hand-off between waves, no
// atomics, no workspace, no LDS; WAVES such owners per workgroup, COLS columns of the row per lane.  labelembed_table_grad_kernel calls
// scan(); center_loss_centroid_grad_kernel shares the constants and keeps the same loop written out (slower through the helper:
// profiles/loss_head_dedup.txt section 3) -- a change of the order here belongs there too.
#pragma once
#include "se_common.h"

namespace se {
namespace class_scan {

constexpr int WAVES = 4;        // owners (one wave each) per 256-thread workgroup
constexpr int COLS = 4;         // columns per lane: a wave holds 256 columns of its row in registers
constexpr int CHUNKS = 4;       // 64-label chunks whose loads are in flight together
constexpr int ROWS = 4;         // matched batch rows handed over together, so that the caller's loads of them are in flight together

// up to ROWS matched rows of one 64-label chunk, ascending: lane[q] held row[q]'s label.  Slots q >= n name the chunk's first row
// (lane 0; it is < B), so that the caller may load all ROWS slots unconditionally and must accumulate only q < n.
struct Group {
    int n, lane[ROWS];
    int64_t row[ROWS];
};

// For wave-uniform k: pred(i, mine) -> bool per lane, called once per chunk with the lane's row i and mine = (i < B && clamp(label_i)
// == k); it may load what the lane's row contributes and narrow the predicate.  A chunk with matches: on_hits(lowest matching lane)
// once, then on_group(g) for every group, in ascending row order.
template <class Pred, class OnHits, class OnGroup>
__device__ __forceinline__ void scan(const int64_t *__restrict__ labels, int64_t B, int64_t C, int64_t k, Pred pred, OnHits on_hits,
                                     OnGroup on_group)
{
    const int lane = lane_id();
    for (int64_t i0 = 0; i0 < B; i0 += 64 * CHUNKS) {
        int64_t lab[CHUNKS];
#pragma unroll
        for (int j = 0; j < CHUNKS; j++) {
            const int64_t i = i0 + j * 64 + lane;
            lab[j] = i < B ? labels[i] : -1;
        }
#pragma unroll
        for (int j = 0; j < CHUNKS; j++) {
            const int64_t i = i0 + j * 64 + lane;
            const int64_t y = clamp_label(lab[j], C);      // the gathers' clamp
            uint64_t hit = __ballot(pred(i, i < B && y == k));
            if (hit) on_hits(__builtin_ctzll(hit));
            while (hit) {
                Group g;
                g.n = 0;
#pragma unroll
                for (int q = 0; q < ROWS; q++) {
                    g.lane[q] = __builtin_ctzll(hit ? hit : 1ull);
                    g.row[q] = i0 + j * 64 + g.lane[q];
                    g.n += hit ? 1 : 0;
                    hit &= hit - 1;
                }
                on_group(g);
            }
        }
    }
}

}  // namespace class_scan
}  // namespace se
