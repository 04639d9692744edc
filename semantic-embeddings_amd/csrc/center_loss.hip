// center_loss.hip -- gradient of the center loss (Wen et al.) with respect to the learned class centroids.
//
// Replaces what TF autodiff derives for the `cls_centroids` Embedding of learn_center_loss.py:17-41
// (center_loss_i = sum_d (embedding[i, d] - cls_centroids[y_i, d])^2 / 2):
//     d c[k, d] = - sum over {i : y_i = k} of fl(w_i * fl(x[i, d] - c[k, d]))
// accumulated from +0 in INCREASING i (TF's unsorted_segment_sum has no fixed order; this one does).  The forward pass and the
// input gradient are se_sqdist_loss_fwd / _bwd (include/sehip.h); only this reduction over the batch rows of each class is new.
//
// Layout: one wave owns one centroid row k and walks its class's batch rows in the fixed order of class_scan.h (the scan the table
// gradient of labelembed.hip calls; this kernel shares its constants and keeps the loop written out, see below): labels 64 at a time,
// a ballot, the set bits in ascending order.  A pass keeps 256 columns of the row in registers (4 per lane); wider rows take several
// passes, each re-scanning the labels.  Cost: C x B label reads (L2-resident) + B x D feature reads.
#include "class_scan.h"

namespace se {

using class_scan::WAVES, class_scan::COLS, class_scan::CHUNKS, class_scan::ROWS;

template <bool BF16>
__global__ __launch_bounds__(64 * WAVES) void center_loss_centroid_grad_kernel(
    const void *__restrict__ x, int64_t ldx, const int64_t *__restrict__ labels, const float *__restrict__ cent, int64_t ldc,
    const float *__restrict__ grad_loss_i, float grad_scale, int64_t B, int64_t D, int64_t C, float *__restrict__ dcent, int64_t lddc)
{
    const int lane = lane_id();
    const int64_t k = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);      // wave-uniform
    if (k >= C) return;
    const float *crow = cent + k * ldc;
    float *drow = dcent + k * lddc;
    for (int64_t d0 = 0; d0 < D; d0 += 64 * COLS) {
        float acc[COLS], c[COLS];
#pragma unroll
        for (int r = 0; r < COLS; r++) {
            const int64_t d = d0 + r * 64 + lane;
            acc[r] = 0.f;
            c[r] = d < D ? crow[d] : 0.f;
        }
        // The scan below is class_scan::scan's, written out: through the shared helper this kernel measured 0.25 us (2.4 %) above the
        // parent's range at B = 1024, C = 100 (profiles/loss_head_dedup.txt section 3); labelembed_table_grad_kernel uses the helper.
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
                const int64_t y = clamp_label(lab[j], C);      // the gather's clamp (se_sqdist_loss_fwd / _bwd)
                uint64_t hit = __ballot(i < B && y == k);
                while (hit) {                                   // matched rows in ascending order, ROWS of them loaded together
                    int64_t row[ROWS];
                    int n = 0;
#pragma unroll
                    for (int q = 0; q < ROWS; q++) {         // slots past the last match load the chunk's first row (< B) unused
                        row[q] = i0 + j * 64 + __builtin_ctzll(hit ? hit : 1ull);
                        n += hit ? 1 : 0;
                        hit &= hit - 1;
                    }
                    float w[ROWS], v[ROWS][COLS];
#pragma unroll
                    for (int q = 0; q < ROWS; q++) {
                        w[q] = grad_loss_i ? grad_loss_i[row[q]] : grad_scale;
#pragma unroll
                        for (int r = 0; r < COLS; r++) {
                            const int64_t d = d0 + r * 64 + lane;
                            v[q][r] = d < D ? ld_elem<BF16>(x, row[q] * ldx + d) : 0.f;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < ROWS; q++) {
                        if (q < n) {
#pragma unroll
                            for (int r = 0; r < COLS; r++) {
                                const float t = v[q][r] - c[r];          // -ffp-contract=off: three roundings, no fma
                                const float p = w[q] * t;
                                acc[r] = acc[r] - p;
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < COLS; r++) {
            const int64_t d = d0 + r * 64 + lane;
            if (d < D) drow[d] = acc[r];
        }
    }
}

}  // namespace se

using namespace se;

extern "C" int se_center_loss_centroid_grad(const void *x, int x_dtype, int64_t ldx, const int64_t *labels, const float *centroids,
                                            int64_t ldc, const float *grad_loss_i, float grad_scale, int64_t B, int64_t D, int64_t C,
                                            float *dcent, int64_t lddc, se_stream_t stream)
{
    if (B < 0 || D <= 0 || C <= 0)
        return fail(SE_ERR_INVALID, "se_center_loss_centroid_grad: bad shape B=%lld D=%lld C=%lld", (long long)B, (long long)D, (long long)C);
    if (!dcent || !centroids || (B > 0 && (!x || !labels))) return fail(SE_ERR_INVALID, "se_center_loss_centroid_grad: null pointer");
    if (ldx < D || ldc < D || lddc < D) return fail(SE_ERR_INVALID, "se_center_loss_centroid_grad: leading dimension < D");
    if (!is_float_dtype(x_dtype)) return fail(SE_ERR_INVALID, "se_center_loss_centroid_grad: bad dtype %d", x_dtype);
    const int64_t blocks = (C + WAVES - 1) / WAVES;
    if (blocks > 0x7FFFFFFF) return fail(SE_ERR_UNSUPPORTED, "se_center_loss_centroid_grad: C too large");
    hipStream_t s = (hipStream_t)stream;
    dispatch_bools(x_dtype == SE_DTYPE_BF16, [&](auto XB) {
        hipLaunchKernelGGL(center_loss_centroid_grad_kernel<XB()>, dim3((unsigned)blocks), dim3(64 * WAVES), 0, s, x, ldx, labels, centroids,
                           ldc, grad_loss_i, grad_scale, B, D, C, dcent, lddc);
    });
    SE_LAUNCH_CHECK();
    return SE_OK;
}
