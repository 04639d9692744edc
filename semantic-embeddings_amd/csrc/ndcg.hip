// ndcg.hip -- normalised discounted cumulative gain on the device: the graded, position-discounted measure next to hprec.hip's
// hierarchical precision, read from the same rank tiles (se_ndcg, include/sehip.h).
//
// Per query and gain table: DCG@k = sum over the first k ranked items (the query's own entry dropped) of
// gain[query class][item class] * disc[position - 1], divided by the ideal DCG the caller built from the gallery's class counts
// (sehip.ndcg_ideal).  Persistent 256-thread workgroups take one query at a time and walk its ranking in chunks of
// SE_NDCG_CHUNK = 2048 ranks: two groups of 1024, in each of which thread t owns ranks 4 t .. 4 t + 3 (one 16-byte load per group,
// contiguous across the wave).  rank -> class (rank_stream.h's LDS table) -> the query class's gain pair (LDS) -> two FMAs with
// the position's discount into per-thread float64 accumulators.  That is ALL an interior chunk does -- one behind the query's own
// position and past the largest cut-off, every rank live: no scan, no barrier, nothing tested per rank.  The other chunks mask the
// dead positions (the query, the list's end) with a gain of exactly 0 -- the accumulators then take the same FMAs with the same
// bits, so a result does not depend on which form a chunk took -- and, where a cut-off can fall into the chunk, scan the products
// (DPP wave scan, wave totals double-buffered in LDS, one barrier) to give every position its running DCG.
// What the memory system sees per rank: 4 B of the ranking (requested a chunk ahead) and 8 B of `disc`, the one array every
// query shares (400 KB at 50,000 positions: L2-resident).  No best curve per class is needed at every rank -- the ideal enters
// at the cut-offs only -- so there is no class-order workspace, and a row's bits depend on that row alone: the whole-list sum is
// the fixed-order reduction of the 256 threads' accumulators, the cut-offs are carry + scan, whatever the grid.
#include "rank_stream.h"

namespace se {

constexpr int ND_THREADS = 256;
constexpr int ND_WAVES = ND_THREADS / WAVE;
constexpr int ND_ITEMS = 4;                                  // consecutive ranks per thread and load
constexpr int ND_GROUPS = 2;                                 // loads per thread and chunk
constexpr int ND_GROUP_RANKS = ND_THREADS * ND_ITEMS;
constexpr int ND_CHUNK = ND_GROUPS * ND_GROUP_RANKS;
constexpr int ND_MAX_KS = 512;
static_assert(ND_CHUNK == SE_NDCG_CHUNK, "the header states the chunk");

// LDS of a workgroup in front of the class table: [C] gain pairs, [2][ND_GROUPS][ND_WAVES][2] scan totals, [ND_WAVES][2] final sums,
// [nk] + [nk] cut-offs and slots, 4 ints (own position, iota flag); rounded so that the class table starts 16-byte aligned
inline size_t nd_fixed_lds(int num_classes, int nk)
{
    return (size_t)num_classes * sizeof(double2) + (size_t)(2 * ND_GROUPS * ND_WAVES * 2 + ND_WAVES * 2) * sizeof(double) +
           (size_t)((2 * nk + 4 + 3) / 4 * 4) * sizeof(int);
}

// out row layout: [NDCG@k a x nk][NDCG@k b x nk][NDCG a][NDCG b]
template <int CLSW>
__global__ __launch_bounds__(ND_THREADS) void ndcg_kernel(const int32_t *__restrict__ rank, int64_t ldr, int64_t Q, int64_t L,
                                                          const int32_t *__restrict__ cls, int64_t gallery,
                                                          const int32_t *__restrict__ qcls, const int32_t *__restrict__ qidx,
                                                          const double *__restrict__ gain_a, const double *__restrict__ gain_b, int C,
                                                          const double *__restrict__ disc, const double *__restrict__ ideal,
                                                          const int32_t *__restrict__ ks, int nk, int want_full,
                                                          double *__restrict__ out, int64_t ldo, int vec_ok)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char nd_raw[];
    double2 *s_gain = reinterpret_cast<double2 *>(nd_raw);         // [C] (a, b) gain of every class for the query's class
    double *s_part = reinterpret_cast<double *>(s_gain + C);       // [2][ND_GROUPS][ND_WAVES][2] wave totals of the scans, double-buffered
    double *s_fin = s_part + 2 * ND_GROUPS * ND_WAVES * 2;         // [ND_WAVES][2] end-of-query reduction
    int *s_ks = reinterpret_cast<int *>(s_fin + ND_WAVES * 2);     // [nk] the cut-offs, ascending
    int *s_perm = s_ks + nk;                                       // [nk] their slots in the output row
    int *s_misc = s_perm + nk;                                     // own position, iota flag
    unsigned char *s_cls = reinterpret_cast<unsigned char *>(s_ks + (2 * nk + 4 + 3) / 4 * 4);   // class of every gallery item (CLSW 1 / 2)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- once per workgroup: the gallery's classes into LDS, the cut-offs sorted ----
    fill_class_table<CLSW, ND_THREADS>(cls, gallery, s_cls, tid);
    const bool ks_iota = sort_cutoffs<ND_THREADS, ND_MAX_KS>(ks, nk, s_ks, s_perm, s_misc + 1, tid);   // (its barriers cover the fill)
    const int kmax = nk > 0 ? s_ks[nk - 1] : 0;                    // cut-offs live at original positions <= kmax
    const int Li = (int)L;                                         // positions are int32 (list_len < 2^31 - 8192 is checked at the entry point)
    const int len = want_full ? Li : min(Li, kmax + 1);            // entries of a row that are read at all
    const int64_t ld_ideal = nk + 1;

    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        const int32_t *row = rank + q * ldr;
        double *orow = out + q * ldo;
        const int qc = qcls[q];
        const int32_t self = qidx ? qidx[q] : -1;
        const double *idl = ideal + ((int64_t)qc * 2 + (self >= 0 ? 1 : 0)) * 2 * ld_ideal;    // [table][slot] of this query
        // the first chunk's ranks are requested together with everything else a query starts with
        int r[ND_GROUPS][ND_ITEMS];
#pragma unroll
        for (int g = 0; g < ND_GROUPS; g++) load_ranks(r[g], row, g * ND_GROUP_RANKS + tid * ND_ITEMS, len, vec_ok);
        for (int c = tid; c < C; c += ND_THREADS) s_gain[c] = make_double2(gain_a[(int64_t)qc * C + c], gain_b[(int64_t)qc * C + c]);
        const int qpos = find_own_entry<ND_THREADS>(row, len, self, s_misc, tid);   // len if nothing is dropped (its barrier covers s_gain)
        const int n_eff = (qpos < len) ? len - 1 : len;            // n_i: entries that are scored

        double car_a = 0.0, car_b = 0.0;        // DCG in front of the current chunk (every thread holds it); kept through the cut-off chunks only
        double acc_a[2] = {0.0, 0.0}, acc_b[2] = {0.0, 0.0};       // this thread's share of the whole sum, two chains per table
        int par = 0;
        for (int base = 0; base < len; base += ND_CHUNK) {
            const bool cuts = (nk > 0) && (base <= kmax);           // uniform: a cut-off may fall into this chunk
            // uniform: every position of the chunk is live and lies behind the query, and no cut-off does
            const bool interior = !cuts && base > qpos && base + ND_CHUNK <= len;
            if (interior) {
                double d[ND_GROUPS][ND_ITEMS];
#pragma unroll
                for (int g = 0; g < ND_GROUPS; g++)
#pragma unroll
                    for (int e = 0; e < ND_ITEMS; e++) d[g][e] = disc[base + g * ND_GROUP_RANKS + tid * ND_ITEMS + e - 1];
                double2 v[ND_GROUPS][ND_ITEMS];
#pragma unroll
                for (int g = 0; g < ND_GROUPS; g++)
#pragma unroll
                    for (int e = 0; e < ND_ITEMS; e++) v[g][e] = s_gain[class_of<CLSW>(s_cls, cls, r[g][e], true, 0)];
                // the rank registers are free again: the next chunk's ranks are requested in front of the arithmetic
#pragma unroll
                for (int g = 0; g < ND_GROUPS; g++) load_ranks(r[g], row, base + ND_CHUNK + g * ND_GROUP_RANKS + tid * ND_ITEMS, len, vec_ok);
#pragma unroll
                for (int g = 0; g < ND_GROUPS; g++)
#pragma unroll
                    for (int e = 0; e < ND_ITEMS; e++) {
                        acc_a[e & 1] = fma(v[g][e].x, d[g][e], acc_a[e & 1]);
                        acc_b[e & 1] = fma(v[g][e].y, d[g][e], acc_b[e & 1]);
                    }
                continue;
            }
            // ---- general form: dead positions (the query itself, the list's end) take a gain of exactly 0 and discount slot 0 ----
            double pa[ND_GROUPS][ND_ITEMS], pb[ND_GROUPS][ND_ITEMS];     // inclusive sums of the products inside the thread's group
#pragma unroll
            for (int g = 0; g < ND_GROUPS; g++) {
                double ta = 0.0, tb = 0.0;
#pragma unroll
                for (int e = 0; e < ND_ITEMS; e++) {
                    const int i = base + g * ND_GROUP_RANKS + tid * ND_ITEMS + e;
                    const bool live = (i < len) && (i != qpos);
                    const int j = (i < qpos) ? i : i - 1;                   // effective rank, 0-based
                    const double de = disc[live ? j : 0];
                    double2 ve = s_gain[class_of<CLSW>(s_cls, cls, r[g][e], live, 0)];
                    ve.x = live ? ve.x : 0.0; ve.y = live ? ve.y : 0.0;
                    acc_a[e & 1] = fma(ve.x, de, acc_a[e & 1]);
                    acc_b[e & 1] = fma(ve.y, de, acc_b[e & 1]);
                    ta += ve.x * de; tb += ve.y * de;
                    pa[g][e] = ta; pb[g][e] = tb;
                }
            }
#pragma unroll
            for (int g = 0; g < ND_GROUPS; g++) load_ranks(r[g], row, base + ND_CHUNK + g * ND_GROUP_RANKS + tid * ND_ITEMS, len, vec_ok);
            if (!cuts) continue;
            // ---- workgroup scan of the group totals: DPP inside the wave, wave totals through LDS, one barrier ----
            double ia[ND_GROUPS], ib[ND_GROUPS];
            double *part = s_part + par * (ND_GROUPS * ND_WAVES * 2);
#pragma unroll
            for (int g = 0; g < ND_GROUPS; g++) {
                ia[g] = wave_incl_scan(pa[g][ND_ITEMS - 1]); ib[g] = wave_incl_scan(pb[g][ND_ITEMS - 1]);
                if (lane == 63) { part[(g * ND_WAVES + wave) * 2] = ia[g]; part[(g * ND_WAVES + wave) * 2 + 1] = ib[g]; }
            }
            wg_barrier();       // the only barrier of a chunk: the other half of s_part is written next time
            par ^= 1;
#pragma unroll
            for (int g = 0; g < ND_GROUPS; g++) {
                double ca = car_a + (ia[g] - pa[g][ND_ITEMS - 1]), cb = car_b + (ib[g] - pb[g][ND_ITEMS - 1]);   // DCG in front of this thread's group
#pragma unroll
                for (int w = 0; w < ND_WAVES; w++) {
                    const double wa = part[(g * ND_WAVES + w) * 2], wb = part[(g * ND_WAVES + w) * 2 + 1];
                    if (w < wave) { ca += wa; cb += wb; }
                    car_a += wa; car_b += wb;
                }
#pragma unroll
                for (int e = 0; e < ND_ITEMS; e++) {
                    const int i = base + g * ND_GROUP_RANKS + tid * ND_ITEMS + e;
                    if (i >= len || i == qpos) continue;
                    const int j = (i < qpos) ? i : i - 1;
                    if (j >= kmax) continue;                            // DCG@(j + 1), if that is a cut-off
                    const double da = ca + pa[g][e], db = cb + pb[g][e];
                    if (ks_iota) {
                        const double za = idl[j], zb = idl[ld_ideal + j];
                        orow[j] = za > 0.0 ? da / za : 0.0; orow[nk + j] = zb > 0.0 ? db / zb : 0.0;
                    } else {
                        int at = 0, hi = nk;                            // lower bound of j + 1 among the sorted cut-offs, then its duplicates
                        while (at < hi) {
                            const int mid = (at + hi) >> 1;
                            if (s_ks[mid] < j + 1) at = mid + 1; else hi = mid;
                        }
                        for (; at < nk && s_ks[at] == j + 1; at++) {
                            const int s = s_perm[at];
                            const double za = idl[s], zb = idl[ld_ideal + s];
                            orow[s] = za > 0.0 ? da / za : 0.0; orow[nk + s] = zb > 0.0 ? db / zb : 0.0;
                        }
                    }
                }
            }
        }
        // ---- finish: the whole sum in a fixed order; it scores the whole list and every cut-off beyond the list's end ----
        const double fa = wave_incl_scan(acc_a[0] + acc_a[1]), fb = wave_incl_scan(acc_b[0] + acc_b[1]);     // lane 63: the wave's sums
        if (lane == 63) { s_fin[wave * 2] = fa; s_fin[wave * 2 + 1] = fb; }
        wg_barrier();
        double all_a = 0.0, all_b = 0.0;
#pragma unroll
        for (int w = 0; w < ND_WAVES; w++) { all_a += s_fin[w * 2]; all_b += s_fin[w * 2 + 1]; }
        for (int at = tid; at < nk; at += ND_THREADS)
            if (s_ks[at] > n_eff) {
                const int s = s_perm[at];
                const double za = idl[s], zb = idl[ld_ideal + s];
                orow[s] = za > 0.0 ? all_a / za : 0.0; orow[nk + s] = zb > 0.0 ? all_b / zb : 0.0;
            }
        if (want_full && tid == 0) {
            const double za = idl[nk], zb = idl[ld_ideal + nk];
            orow[2 * nk] = za > 0.0 ? all_a / za : 0.0; orow[2 * nk + 1] = zb > 0.0 ? all_b / zb : 0.0;
        }
        wg_barrier();       // s_fin, s_gain and the own position are rewritten by the next query
    }
}

}  // namespace se

using namespace se;

extern "C" int se_ndcg(const int32_t *rank, int64_t ldr, int64_t q, int64_t list_len, const int32_t *cls, int64_t gallery,
                       const int32_t *qcls, const int32_t *qidx, const double *gain_a, const double *gain_b, int num_classes,
                       const double *disc, int64_t disc_len, const double *ideal, const int32_t *ks, int nk, int want_full,
                       double *out, int64_t ldo, se_stream_t stream)
{
    if (q < 0 || list_len < 0 || gallery < 0 || disc_len < 0 || ldr < 0 || ldo < 0)
        return fail(SE_ERR_INVALID, "se_ndcg: negative size q=%lld len=%lld gallery=%lld disc_len=%lld ldr=%lld ldo=%lld", (long long)q,
                    (long long)list_len, (long long)gallery, (long long)disc_len, (long long)ldr, (long long)ldo);
    if (nk < 0 || nk > ND_MAX_KS) return fail(SE_ERR_INVALID, "se_ndcg: nk=%d cut-offs, 0 .. %d are taken", nk, ND_MAX_KS);
    if (num_classes < 1) return fail(SE_ERR_INVALID, "se_ndcg: num_classes=%d", num_classes);
    if (nk == 0 && !want_full) return fail(SE_ERR_INVALID, "se_ndcg: nothing to compute (nk == 0 and want_full == 0)");
    if (list_len >= 0x7FFFFFFF - 8192 || q > 0x7FFFFFFF)
        return fail(SE_ERR_INVALID, "se_ndcg: q=%lld len=%lld: positions and rows are 32-bit", (long long)q, (long long)list_len);
    if (ldr < list_len) return fail(SE_ERR_INVALID, "se_ndcg: ldr=%lld is smaller than list_len=%lld", (long long)ldr, (long long)list_len);
    if (disc_len < list_len) return fail(SE_ERR_INVALID, "se_ndcg: disc covers %lld positions, the rankings have %lld", (long long)disc_len, (long long)list_len);
    if (ldo < 2 * (int64_t)nk + 2) return fail(SE_ERR_INVALID, "se_ndcg: ldo=%lld is smaller than 2 nk + 2 = %d", (long long)ldo, 2 * nk + 2);
    if (q == 0 || list_len == 0) return SE_OK;
    if (!rank || !cls || !qcls || !gain_a || !gain_b || !disc || !ideal || !out || (nk > 0 && !ks)) return fail(SE_ERR_INVALID, "se_ndcg: null pointer");
    if (gallery == 0) return fail(SE_ERR_INVALID, "se_ndcg: rankings over an empty gallery");
    const size_t fixed = nd_fixed_lds(num_classes, nk);
    if (fixed > CLASS_TABLE_LDS_CAP) return fail(SE_ERR_UNSUPPORTED, "se_ndcg: %d classes exceed the LDS gain rows", num_classes);
    const ClassTable ct = choose_class_table(list_len, q, gallery, num_classes, fixed);
    const int vec_ok = ranks_vec_ok<int32_t, ND_ITEMS>(rank, ldr);
    return dispatch_clsw(ct.clsw, [&](auto w) -> int {
        const auto kernel = ndcg_kernel<decltype(w)::value>;
        int64_t grid = 0;      // persistent workgroups: the class table is loaded once each
        SE_HIP_CHECK(persistent_grid(kernel, ND_THREADS, ct.lds_bytes, q, &grid));
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(ND_THREADS), ct.lds_bytes, (hipStream_t)stream, rank, ldr, q, list_len, cls, gallery,
                           qcls, qidx, gain_a, gain_b, num_classes, disc, ideal, ks, nk, want_full, out, ldo, vec_ok);
        SE_LAUNCH_CHECK();
        return SE_OK;
    });
}
