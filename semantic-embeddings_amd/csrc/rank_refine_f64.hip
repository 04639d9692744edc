// rank_refine_f64.hip -- se_rank_refine_f64: turns the canonical ranking of the float32 IMAGES of a float64 distance matrix
// (se_rank_rows on img = (float)out64) into the canonical ranking of the float64 distances themselves.
//
// The cast is monotone non-decreasing, so the image ranking already has every pair of columns with different images in the right
// order; only inside a maximal run of adjacent ranks whose images are equal (==, so +-0 are one run; all NaNs are one run) can the
// float64 order differ.  Every such run is sorted in place by (float64 canonical key, column index): NaN last, -0 == +0, equal
// values index-ascending -- the order of se_rank_rows, one level down.
//
// One workgroup walks a row one rank per thread at a time and asks whether a rank starts a run.  Gathering the image through the
// ranks costs a memory line per rank (50,000 x 50,000: 42 ms, six times the ranking itself; profiles/float64_retrieval_bench.txt),
// so rows of up to RF_TOK_MAX_N columns are first staged in LDS as 16-bit TOKENS -- the low half of the image's bits, 0 for a
// NaN: equal images have equal tokens, and neighbours in sorted order differ in their low bits first -- with one coalesced pass
// over the image row.  A rank whose token differs from both neighbours' (theirs come from the neighbouring lanes) is in no run;
// only the others gather the three images that decide (20 ms).  Longer rows gather every rank's image from memory.
// Three sizes of run:
//   * 2 .. RF_SHORT ranks (nearly all of them: Gaussian cosine rows of 50,000 columns have 17 pairs of adjacent ranks with equal
//     images): the thread that owns the run's first rank sorts it in registers (odd-even transposition network) and writes it back;
//   * up to RF_LDS ranks: a second walk over the row, only made when the first saw such a run; the workgroup stages (key, index)
//     in LDS and every element counts the elements in front of it;
//   * longer (up to the whole row): the row is flagged, and a second launch of few workgroups, each with a slice of the workspace
//     as large as a row, sorts the run in chunks of RF_LDS (the same counting, from LDS, into the slice) and then ranks every
//     element by binary search in every other chunk: L / RF_LDS searches per element.  It is the fallback.
// No atomics; workgroups synchronise through wg_barrier() only.  Nothing rests on the order in which the hardware serves lanes.
//
// Concurrent access inside a row: while one thread rewrites a short run, its neighbours may read ranks of that run to decide
// whether THEIR rank starts a run.  Every word of a run holds, at every moment, the index of some column of that run (a store
// replaces one member by another), and all of them have the same image -- so those decisions do not depend on the moment of the
// read.  A run has exactly one writer (the owner of its first rank, or the whole workgroup between two barriers).
#include "se_common.h"

namespace se {

constexpr int RF_THREADS = 256;              // workgroup of the direct (gathering) kernels
constexpr int RF_TOK_THREADS = 1024;         // workgroup of the token kernel: its LDS allows one or two per CU, so they are large
constexpr int RF_MAX_WAVES = RF_TOK_THREADS / WAVE;
constexpr int64_t RF_TOK_MAX_N = 65536;      // longest row whose tokens (2 bytes each) fit the LDS next to the sort's 12 KB
constexpr int RF_SHORT = 8;                 // longest run one thread sorts in registers
constexpr int RF_LDS = 1024;                // longest run sorted from LDS
constexpr int RF_MAX_BLOCKS = 2048;         // grid cap of the main launch
constexpr int RF_FALLBACK_BLOCKS = 64;      // workgroups (and row-sized workspace slices) of the fallback launch

// Order-preserving float64 -> uint64 key of the canonical order: ascending value, -0.0 == +0.0, every NaN last.
__device__ __forceinline__ uint64_t canon_key64(double f)
{
    uint64_t u = (uint64_t)__double_as_longlong(f);
    if (f != f) return ~0ull;
    if (u == 0x8000000000000000ull) u = 0ull;
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ bool same_image(float x, float y) { return x == y || (x != x && y != y); }

// same_image(x, y) implies image_token(x) == image_token(y): +0 and -0 share their low half, every NaN maps to 0
__device__ __forceinline__ uint16_t image_token(float x) { return x != x ? (uint16_t)0 : (uint16_t)__float_as_uint(x); }

template <bool I64>
__device__ __forceinline__ int64_t rf_ld(const void *rank, int64_t i)
{
    if constexpr (I64) return ((const volatile int64_t *)rank)[i];
    else return ((const volatile int32_t *)rank)[i];
}

template <bool I64>
__device__ __forceinline__ void rf_st(void *rank, int64_t i, int64_t v)
{
    if constexpr (I64) ((volatile int64_t *)rank)[i] = v;
    else ((volatile int32_t *)rank)[i] = (int32_t)v;
}

// column index at rank r of the row, forced into [0, n): a ranking that is not a permutation must not make the gathers leave the row
template <bool I64>
__device__ __forceinline__ int64_t rf_col(const void *rank, int64_t r, int64_t n)
{
    const int64_t c = rf_ld<I64>(rank, r);
    return (uint64_t)c < (uint64_t)n ? c : 0;
}

__device__ __forceinline__ bool pair_less(uint64_t ka, int32_t ia, uint64_t kb, int32_t ib) { return ka < kb || (ka == kb && ia < ib); }

// Sort the run of L <= RF_LDS ranks that starts at rank s by counting: element e goes to s + (number of elements in front of it).
// keys / idx (LDS, L entries) are filled here; the (key, index) pairs are distinct, so the destinations are a permutation.
template <bool I64>
__device__ void rf_count_sort(void *rank, const double *__restrict__ d64, int64_t n, int64_t s, int64_t L, uint64_t *keys, int32_t *idx)
{
    const int tid = threadIdx.x, threads = blockDim.x;
    for (int64_t e = tid; e < L; e += threads) {
        const int64_t c = rf_col<I64>(rank, s + e, n);
        keys[e] = canon_key64(d64[c]);
        idx[e] = (int32_t)c;
    }
    wg_barrier();
    for (int64_t e = tid; e < L; e += threads) {
        const uint64_t k = keys[e];
        const int32_t c = idx[e];
        int64_t before = 0;
        for (int64_t j = 0; j < L; j++) before += pair_less(keys[j], idx[j], k, c) ? 1 : 0;
        rf_st<I64>(rank, s + before, c);
    }
    wg_barrier();
}

// The run of L > RF_LDS ranks that starts at rank s: chunks of RF_LDS are sorted through LDS into g_keys / g_idx (L entries of this
// workgroup's workspace slice); the place of an element is its place in its own chunk plus, for every other chunk, the number of
// that chunk's elements in front of it (a binary search: the pairs are distinct).
template <bool I64>
__device__ void rf_chunk_sort(void *rank, const double *__restrict__ d64, int64_t n, int64_t s, int64_t L, uint64_t *g_keys, int32_t *g_idx,
                              uint64_t *s_keys, int32_t *s_idx)
{
    const int tid = threadIdx.x, threads = blockDim.x;
    for (int64_t b0 = 0; b0 < L; b0 += RF_LDS) {
        const int len = (int)(L - b0 < RF_LDS ? L - b0 : RF_LDS);
        for (int e = tid; e < len; e += threads) {
            const int64_t c = rf_col<I64>(rank, s + b0 + e, n);
            s_keys[e] = canon_key64(d64[c]);
            s_idx[e] = (int32_t)c;
        }
        wg_barrier();
        for (int e = tid; e < len; e += threads) {
            const uint64_t k = s_keys[e];
            const int32_t c = s_idx[e];
            int before = 0;
            for (int j = 0; j < len; j++) before += pair_less(s_keys[j], s_idx[j], k, c) ? 1 : 0;
            g_keys[b0 + before] = k;
            g_idx[b0 + before] = c;
        }
        wg_barrier();
    }
    __threadfence_block();
    wg_barrier();
    for (int64_t e = tid; e < L; e += threads) {
        const uint64_t k = g_keys[e];
        const int32_t c = g_idx[e];
        const int64_t own = e / RF_LDS * RF_LDS;
        int64_t place = e - own;
        for (int64_t b0 = 0; b0 < L; b0 += RF_LDS) {
            if (b0 == own) continue;
            int64_t lo = b0, hi = L - b0 < RF_LDS ? L : b0 + RF_LDS;     // first entry of the chunk that is not in front of (k, c)
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (pair_less(g_keys[mid], g_idx[mid], k, c)) lo = mid + 1;
                else hi = mid;
            }
            place += lo - b0;
        }
        rf_st<I64>(rank, s + place, c);
    }
    __threadfence_block();
    wg_barrier();
}

// Does rank r start a run of at least two ranks with equal images?  v: the image at rank r (set when the answer is yes).
// Called by every thread of a wave (the neighbours' images / tokens travel through lane shuffles).
template <bool I64, bool TOK>
__device__ __forceinline__ bool rf_run_start(const void *rank, const float *__restrict__ im, const uint16_t *tok, int64_t r, int64_t n, int lane,
                                             float &v)
{
    const bool valid = r < n;
    float vp = 0.0f, vn = 0.0f;
    v = 0.0f;
    if constexpr (TOK) {
        uint32_t t = 0x10000u;                                 // (no 16-bit token equals the stand-ins of ranks that do not exist)
        if (valid) t = tok[rf_col<I64>(rank, r, n)];
        uint32_t tp = __shfl_up(t, 1, 64), tn = __shfl_down(t, 1, 64);
        if (lane == 0) tp = valid && r > 0 ? tok[rf_col<I64>(rank, r - 1, n)] : 0x20000u;
        if (lane == 63) tn = r + 1 < n ? tok[rf_col<I64>(rank, r + 1, n)] : 0x20000u;
        if (!valid || (t != tp && t != tn)) return false;      // in no run: the common case, and no access to memory
        v = im[rf_col<I64>(rank, r, n)];
        if (r > 0) vp = im[rf_col<I64>(rank, r - 1, n)];
        if (r + 1 < n) vn = im[rf_col<I64>(rank, r + 1, n)];
    } else {
        if (valid) v = im[rf_col<I64>(rank, r, n)];
        vp = __shfl_up(v, 1, 64), vn = __shfl_down(v, 1, 64);
        if (lane == 0 && valid && r > 0) vp = im[rf_col<I64>(rank, r - 1, n)];
        if (lane == 63 && r + 1 < n) vn = im[rf_col<I64>(rank, r + 1, n)];
    }
    return valid && (r == 0 || !same_image(vp, v)) && r + 1 < n && same_image(v, vn);
}

// FALLBACK = false: the main launch (short runs in registers, runs up to RF_LDS from LDS, longer ones flag their row).
// FALLBACK = true: flagged rows only, runs longer than RF_LDS only, from this workgroup's slice of the workspace.
// TOK: the row's image tokens are staged in the dynamic LDS (n uint16) and filter the gathers.
template <bool I64, bool FALLBACK, bool TOK, int THREADS>
__global__ __launch_bounds__(THREADS) void rank_refine_f64_kernel(const double *__restrict__ out64, int64_t ld64, const float *__restrict__ img,
                                                                     int64_t ldi, int64_t q, int64_t n, void *rank_base, int64_t ldr,
                                                                     int32_t *__restrict__ row_flag, uint64_t *__restrict__ g_keys,
                                                                     int32_t *__restrict__ g_idx)
{
    __shared__ uint64_t s_keys[RF_LDS];
    __shared__ int32_t s_idx[RF_LDS];
    __shared__ uint64_t s_ballot[THREADS / WAVE];
    __shared__ int s_fail[THREADS / WAVE];
    __shared__ int s_medium, s_long;
    extern __shared__ __attribute__((aligned(16))) uint16_t s_tok[];
    static_assert(!(FALLBACK && TOK) && THREADS / WAVE <= RF_MAX_WAVES, "the fallback gathers; at most RF_MAX_WAVES waves");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int64_t row = blockIdx.x; row < q; row += gridDim.x) {
        if (FALLBACK && row_flag[row] == 0) continue;      // (uniform over the workgroup)
        void *rank = I64 ? (void *)((int64_t *)rank_base + row * ldr) : (void *)((int32_t *)rank_base + row * ldr);
        const float *im = img + row * ldi;
        const double *d64 = out64 + row * ld64;
        if (tid == 0) s_medium = 0, s_long = 0;
        if constexpr (TOK)
            for (int64_t c = tid; c < n; c += THREADS) s_tok[c] = image_token(im[c]);
        wg_barrier();

        // pass 0 (main launch): short runs; pass 1: the runs longer than RF_SHORT, one after the other by the whole workgroup
        for (int pass = FALLBACK ? 1 : 0; pass < 2; pass++) {
            if (pass == 1 && !FALLBACK) {
                wg_barrier();
                if (s_medium == 0) break;                  // (uniform: read behind the barrier)
            }
            for (int64_t base = 0; base < n; base += THREADS) {
                const int64_t r = base + tid;
                float v;
                const bool start = rf_run_start<I64, TOK>(rank, im, s_tok, r, n, lane, v);      // first rank of a run of >= 2
                int64_t len = 0;
                if (start) {                               // run length, as far as it matters: 2 .. RF_SHORT, or RF_SHORT + 1 for "longer"
                    len = 2;
                    while (len <= RF_SHORT && r + len < n && same_image(im[rf_col<I64>(rank, r + len, n)], v)) len++;
                }
                if (pass == 0) {
                    if (len > RF_SHORT) {
                        s_medium = 1;                      // (every writer stores the same value)
                    } else if (len >= 2) {
                        uint64_t k[RF_SHORT];
                        int64_t c[RF_SHORT];
#pragma unroll
                        for (int e = 0; e < RF_SHORT; e++) {
                            k[e] = ~0ull;
                            c[e] = INT64_MAX;              // padding sorts behind every real pair (a NaN key ties, the index decides)
                            if (e < len) {
                                c[e] = rf_col<I64>(rank, r + e, n);
                                k[e] = canon_key64(d64[c[e]]);
                            }
                        }
#pragma unroll
                        for (int round = 0; round < RF_SHORT; round++)
#pragma unroll
                            for (int e = round & 1; e + 1 < RF_SHORT; e += 2) {
                                const bool swap = k[e + 1] < k[e] || (k[e + 1] == k[e] && c[e + 1] < c[e]);
                                const uint64_t klo = swap ? k[e + 1] : k[e], khi = swap ? k[e] : k[e + 1];
                                const int64_t clo = swap ? c[e + 1] : c[e], chi = swap ? c[e] : c[e + 1];
                                k[e] = klo, k[e + 1] = khi, c[e] = clo, c[e + 1] = chi;
                            }
#pragma unroll
                        for (int e = 0; e < RF_SHORT; e++)
                            if (e < len) rf_st<I64>(rank, r + e, c[e]);
                    }
                    continue;
                }
                // ---- pass 1: every start of a run longer than RF_SHORT among these THREADS ranks, in rank order ----
                const uint64_t ballot = __ballot(len > RF_SHORT);
                if (lane == 0) s_ballot[wave] = ballot;
                wg_barrier();
                for (int w = 0; w < THREADS / WAVE; w++) {
                    uint64_t todo = s_ballot[w];
                    while (todo) {
                        const int bit = __builtin_ctzll(todo);
                        todo &= todo - 1;
                        const int64_t s = base + w * WAVE + bit;
                        // length of the run: the first rank behind s whose image differs, found THREADS ranks at a time
                        const float v0 = im[rf_col<I64>(rank, s, n)];
                        int64_t end = -1;
                        for (int64_t c0 = s + 1; end < 0; c0 += THREADS) {
                            const int64_t p = c0 + tid;
                            const bool in_run = p < n && same_image(im[rf_col<I64>(rank, p, n)], v0);
                            const uint64_t ok = __ballot(in_run);
                            if (lane == 0) s_fail[wave] = ok == ~0ull ? WAVE : __builtin_ctzll(~ok);
                            wg_barrier();
                            for (int ww = 0; ww < THREADS / WAVE && end < 0; ww++)
                                if (s_fail[ww] < WAVE) end = c0 + ww * WAVE + s_fail[ww];
                            wg_barrier();
                        }
                        const int64_t L = end - s;
                        if (!FALLBACK) {
                            if (L <= RF_LDS) rf_count_sort<I64>(rank, d64, n, s, L, s_keys, s_idx);
                            else if (tid == 0) s_long = 1;
                        } else if (L > RF_LDS) {
                            rf_chunk_sort<I64>(rank, d64, n, s, L, g_keys + (int64_t)blockIdx.x * n, g_idx + (int64_t)blockIdx.x * n, s_keys, s_idx);
                        }
                    }
                }
                wg_barrier();                              // s_ballot is rewritten by the next THREADS ranks
            }
        }
        if (!FALLBACK) {
            wg_barrier();
            if (tid == 0) row_flag[row] = s_long;
        }
        wg_barrier();                                      // (the next row rewrites the tokens and the flags)
    }
}

// workspace: [q] int32 row flags (padded to 16 bytes), then RF_FALLBACK_BLOCKS slices of n uint64 keys, then as many of n int32 indices
inline int64_t rf_flag_bytes(int64_t q) { return (q * 4 + 15) / 16 * 16; }

}  // namespace se

using namespace se;

extern "C" int64_t se_rank_refine_f64_workspace_bytes(int64_t q, int64_t n)
{
    if (q <= 0 || n <= 0) return 0;
    return rf_flag_bytes(q) + (int64_t)RF_FALLBACK_BLOCKS * n * 12;
}

extern "C" int se_rank_refine_f64(const double *out64, int64_t ld64, const float *img, int64_t ldi, int64_t q, int64_t n, void *rank,
                                  int idx64, int64_t ldr, void *workspace, int64_t workspace_bytes, se_stream_t stream)
{
    const char *who = "se_rank_refine_f64";
    if (q < 0 || n < 0) return fail(SE_ERR_INVALID, "%s: negative shape q=%lld n=%lld", who, (long long)q, (long long)n);
    if (idx64 == 2) return fail(SE_ERR_UNSUPPORTED, "%s: uint16 ranks are not served (idx64 = 0: int32, 1: int64)", who);
    if (idx64 != 0 && idx64 != 1) return fail(SE_ERR_INVALID, "%s: idx64 must be 0 (int32) or 1 (int64)", who);
    if (q == 0 || n == 0) return SE_OK;
    if (n > 0x7FFFFFFF) return fail(SE_ERR_UNSUPPORTED, "%s: rows of more than 2^31 - 1 columns", who);
    if (!out64 || !img || !rank) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if (ld64 < n || ldi < n || ldr < n) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    if (!workspace || (((uintptr_t)workspace) & 15)) return fail(SE_ERR_INVALID, "%s: the workspace must be 16-byte aligned", who);
    if (workspace_bytes < se_rank_refine_f64_workspace_bytes(q, n))
        return fail(SE_ERR_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
                    (long long)se_rank_refine_f64_workspace_bytes(q, n));
    hipStream_t s = (hipStream_t)stream;
    int32_t *flags = (int32_t *)workspace;
    uint64_t *g_keys = (uint64_t *)((char *)workspace + rf_flag_bytes(q));
    int32_t *g_idx = (int32_t *)(g_keys + (int64_t)RF_FALLBACK_BLOCKS * n);
    const dim3 grid((unsigned)(q < RF_MAX_BLOCKS ? q : RF_MAX_BLOCKS)), fgrid((unsigned)(q < RF_FALLBACK_BLOCKS ? q : RF_FALLBACK_BLOCKS));
    const size_t tok_bytes = (size_t)(n * 2 + 15) / 16 * 16;
    hipError_t err = hipSuccess;
    dispatch_bools(idx64 == 1, n <= RF_TOK_MAX_N, [&](auto i64, auto tok) {
        constexpr bool I64 = decltype(i64)::value, TOK = decltype(tok)::value;
        constexpr int THREADS = TOK ? RF_TOK_THREADS : RF_THREADS;
        auto kern = rank_refine_f64_kernel<I64, false, TOK, THREADS>;
        if (TOK) err = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tok_bytes);
        if (err != hipSuccess) return;
        hipLaunchKernelGGL(kern, grid, dim3(THREADS), TOK ? tok_bytes : 0, s, out64, ld64, img, ldi, q, n, rank, ldr, flags, g_keys, g_idx);
        hipLaunchKernelGGL((rank_refine_f64_kernel<I64, true, false, RF_THREADS>), fgrid, dim3(RF_THREADS), 0, s, out64, ld64, img, ldi, q, n, rank,
                           ldr, flags, g_keys, g_idx);
    });
    SE_HIP_CHECK(err);
    SE_LAUNCH_CHECK();
    return SE_OK;
}
