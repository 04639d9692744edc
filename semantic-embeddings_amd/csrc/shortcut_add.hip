// shortcut_add.hip -- the pyramidal residual shortcut in one launch: out = s + ChannelPadding(AveragePooling2D(stride)(x)), and the
// gradient of x.
//
// Replaces layers.add([s, shortcut(x, n, stride)]) of models/cifar_pyramidnet.py:81-110 (and the same composition of
// models/cifar_resnet.py, whose padding is symmetric: pad_before > 0), which as avg_pool2d + pad + add writes a zero-padded copy of
// the shortcut as large as the block output only for the add to read it again.  Here s and x are read once and out is written once.
//
// Arithmetic (include/sehip.h states it; every operation a separately rounded float32 operation, bf16 widened first):
//     acc = x00;  acc = acc + x01;  acc = acc + x10;  acc = acc + x11          (stride 2; stride 1: acc = x)
//     out = round_to_dtype(s + acc / (float)(stride * stride))                  channels [pad_before, pad_before + Cin)
//     out = s                                                                   every other channel: the bits are copied
//     dx  = round_to_dtype(dout / (float)(stride * stride)), 0 on the trailing odd row / column
//
// Streaming kernels: nothing is shared between outputs, so no LDS, no barrier, no atomics, and the same bits whatever the launch
// geometry.  A thread takes one UNIT of V consecutive elements of the innermost axis -- channels in NHWC, image columns in NCHW (at
// stride 1 a channel plane of NCHW is contiguous, so a whole image is one row of C * H * W elements with the shortcut's segment in the
// middle, exactly the shape of one NHWC pixel) -- and consecutive threads take consecutive units: adjacent lanes touch adjacent memory
// in both layouts.  V is the largest power of two (16 bytes at most) that divides every extent and offset a unit could straddle and
// to which every pointer is aligned; V = 1 takes everything else element by element (PyramidNet widths 18, 21, 22 ... in NHWC), so
// there is no tail to treat apart.  int64 offsets; a grid-stride loop under a grid capped at SE_SHORTCUT_MAX_BLOCKS.
#include "se_common.h"

#pragma clang fp contract(off)

namespace se {

constexpr int SC_THREADS = 256;

template <class T, int N>
struct alignas(sizeof(T) * N) Vec {
    T v[N];
};

template <bool BF16>
using sc_elem_t = std::conditional_t<BF16, uint16_t, float>;

template <bool BF16>
__device__ __forceinline__ float sc_widen(sc_elem_t<BF16> e)
{
    if constexpr (BF16) return bf16_to_f32(e);
    else return e;
}

template <bool BF16>
__device__ __forceinline__ sc_elem_t<BF16> sc_round(float f)
{
    if constexpr (BF16) return f32_to_bf16(f);
    else return f;
}

// Geometry of one call, in elements.  "Row" form (NHWC at both strides, NCHW at stride 1): the output is `rows` rows of `L` elements,
// the shortcut adds to elements [off, off + n) of every row.  NCHW at stride 2 uses the image extents directly.
struct ScGeom {
    int64_t units;               // work items of V elements
    int64_t L, off, n;           // row form
    int64_t C, H, W, Cin, Hx, Wx, pad;
};

// ---- row form: TAPS = 1 (stride 1, either layout), TAPS = 4 (stride 2, NHWC: a row is one output pixel) ----
template <bool BF16, int V, int TAPS>
__global__ __launch_bounds__(SC_THREADS) void shortcut_rows_fwd_kernel(const void *s, const void *x, void *out, ScGeom g)
{
    using T = sc_elem_t<BF16>;
    using VT = Vec<T, V>;
    const int64_t step = (int64_t)gridDim.x * SC_THREADS;
    const int64_t lv = g.L / V;
    for (int64_t u = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; u < g.units; u += step) {
        const int64_t r = u / lv, j = (u - r * lv) * V;
        VT sv = *(const VT *)((const T *)s + r * g.L + j);
        if (j >= g.off && j < g.off + g.n) {             // V divides off and n: a unit lies wholly inside or outside
            int64_t xb;
            if constexpr (TAPS == 1) {
                xb = r * g.n + (j - g.off);
            } else {
                const int64_t t = r / g.W, w = r - t * g.W, b = t / g.H, h = t - b * g.H;
                xb = ((b * g.Hx + 2 * h) * g.Wx + 2 * w) * g.n + (j - g.off);
            }
            const T *xp = (const T *)x + xb;
            const VT x0 = *(const VT *)xp;
            if constexpr (TAPS == 1) {
#pragma unroll
                for (int k = 0; k < V; k++) sv.v[k] = sc_round<BF16>(sc_widen<BF16>(sv.v[k]) + sc_widen<BF16>(x0.v[k]));
            } else {
                const int64_t down = g.Wx * g.n;
                const VT x1 = *(const VT *)(xp + g.n), x2 = *(const VT *)(xp + down), x3 = *(const VT *)(xp + down + g.n);
#pragma unroll
                for (int k = 0; k < V; k++) {
                    float acc = sc_widen<BF16>(x0.v[k]);
                    acc = acc + sc_widen<BF16>(x1.v[k]);
                    acc = acc + sc_widen<BF16>(x2.v[k]);
                    acc = acc + sc_widen<BF16>(x3.v[k]);
                    const float pooled = acc / 4.0f;
                    sv.v[k] = sc_round<BF16>(sc_widen<BF16>(sv.v[k]) + pooled);
                }
            }
        }
        *(VT *)((T *)out + r * g.L + j) = sv;
    }
}

// one unit of dx per thread: `units` = (rows of dx) * n / V; a row of dx is an image (TAPS = 1, NCHW), or a pixel of x
template <bool BF16, int V, int TAPS>
__global__ __launch_bounds__(SC_THREADS) void shortcut_rows_bwd_kernel(const void *dout, void *dx, ScGeom g)
{
    using T = sc_elem_t<BF16>;
    using VT = Vec<T, V>;
    const int64_t step = (int64_t)gridDim.x * SC_THREADS;
    const int64_t nv = g.n / V;
    for (int64_t u = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; u < g.units; u += step) {
        const int64_t r = u / nv, i = (u - r * nv) * V;
        VT d;
        if constexpr (TAPS == 1) {
            d = *(const VT *)((const T *)dout + r * g.L + g.off + i);
        } else {
            const int64_t t = r / g.Wx, xx = r - t * g.Wx, b = t / g.Hx, y = t - b * g.Hx;
            if (y < 2 * g.H && xx < 2 * g.W) {
                const int64_t src = (b * g.H + (y >> 1)) * g.W + (xx >> 1);
                d = *(const VT *)((const T *)dout + src * g.L + g.off + i);
#pragma unroll
                for (int k = 0; k < V; k++) d.v[k] = sc_round<BF16>(sc_widen<BF16>(d.v[k]) / 4.0f);
            } else {                                     // trailing odd row / column of x: in no window
#pragma unroll
                for (int k = 0; k < V; k++) d.v[k] = sc_round<BF16>(0.0f);
            }
        }
        *(VT *)((T *)dx + r * g.n + i) = d;
    }
}

// ---- NCHW at stride 2: a unit is V consecutive output columns of one output row (b, c, h) ----
template <bool BF16, int V>
__global__ __launch_bounds__(SC_THREADS) void shortcut_nchw2_fwd_kernel(const void *s, const void *x, void *out, ScGeom g)
{
    using T = sc_elem_t<BF16>;
    using VT = Vec<T, V>;
    const int64_t step = (int64_t)gridDim.x * SC_THREADS;
    const int64_t wv = g.W / V;
    for (int64_t u = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; u < g.units; u += step) {
        const int64_t r = u / wv, w = (u - r * wv) * V;
        const int64_t t = r / g.H, h = r - t * g.H, b = t / g.C, c = t - b * g.C;
        VT sv = *(const VT *)((const T *)s + r * g.W + w);
        if (c >= g.pad && c < g.pad + g.Cin) {
            const T *top = (const T *)x + ((b * g.Cin + (c - g.pad)) * g.Hx + 2 * h) * g.Wx + 2 * w;
            const T *bot = top + g.Wx;
            const VT t0 = *(const VT *)top, t1 = *(const VT *)(top + V), b0 = *(const VT *)bot, b1 = *(const VT *)(bot + V);
            T tv[2 * V], bv[2 * V];
#pragma unroll
            for (int k = 0; k < V; k++) {
                tv[k] = t0.v[k];
                tv[V + k] = t1.v[k];
                bv[k] = b0.v[k];
                bv[V + k] = b1.v[k];
            }
#pragma unroll
            for (int k = 0; k < V; k++) {
                float acc = sc_widen<BF16>(tv[2 * k]);
                acc = acc + sc_widen<BF16>(tv[2 * k + 1]);
                acc = acc + sc_widen<BF16>(bv[2 * k]);
                acc = acc + sc_widen<BF16>(bv[2 * k + 1]);
                const float pooled = acc / 4.0f;
                sv.v[k] = sc_round<BF16>(sc_widen<BF16>(sv.v[k]) + pooled);
            }
        }
        *(VT *)((T *)out + r * g.W + w) = sv;
    }
}

// a unit is V consecutive columns of one row (b, ci, y) of dx; V >= 2 implies an even Wx, so only V = 1 meets the odd last column
template <bool BF16, int V>
__global__ __launch_bounds__(SC_THREADS) void shortcut_nchw2_bwd_kernel(const void *dout, void *dx, ScGeom g)
{
    using T = sc_elem_t<BF16>;
    constexpr int S = V >= 2 ? V / 2 : 1;              // dout elements behind one unit
    const int64_t step = (int64_t)gridDim.x * SC_THREADS;
    const int64_t wv = g.Wx / V;
    for (int64_t u = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; u < g.units; u += step) {
        const int64_t r = u / wv, xx = (u - r * wv) * V;
        const int64_t t = r / g.Hx, y = r - t * g.Hx, b = t / g.Cin, ci = t - b * g.Cin;
        Vec<T, V> d;
        if (y < 2 * g.H && xx < 2 * g.W) {
            const Vec<T, S> src = *(const Vec<T, S> *)((const T *)dout + ((b * g.C + g.pad + ci) * g.H + (y >> 1)) * g.W + (xx >> 1));
#pragma unroll
            for (int k = 0; k < V; k++) d.v[k] = sc_round<BF16>(sc_widen<BF16>(src.v[k / 2]) / 4.0f);
        } else {
#pragma unroll
            for (int k = 0; k < V; k++) d.v[k] = sc_round<BF16>(0.0f);
        }
        *(Vec<T, V> *)((T *)dx + r * g.Wx + xx) = d;
    }
}

// ---- host ----

// largest power of two <= vmax that divides every extent in `dims` and to whose byte size every pointer in `ptrs` is aligned
static int sc_vector_width(int vmax, int elem_bytes, std::initializer_list<int64_t> dims, std::initializer_list<const void *> ptrs)
{
    int v = vmax;
    for (; v > 1; v >>= 1) {
        bool ok = true;
        for (int64_t d : dims) ok = ok && d % v == 0;
        for (const void *p : ptrs) ok = ok && ((uintptr_t)p % (uintptr_t)(v * elem_bytes)) == 0;
        if (ok) break;
    }
    return v;
}

// a unit of V elements is one access of 16 bytes at most (float32: V <= 4; sc_vector_width never asks for more)
template <bool BF16, int V>
constexpr bool sc_fits = V * (int)sizeof(sc_elem_t<BF16>) <= 16;

// f(std::integral_constant<int, V>{}) for V = 1, 2, 4, 8
template <class F>
static void sc_dispatch_width(int v, F f)
{
    switch (v) {
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 1>{}); break;
    }
}

static dim3 sc_grid(int64_t units)
{
    int64_t blocks = (units + SC_THREADS - 1) / SC_THREADS;
    if (blocks > SE_SHORTCUT_MAX_BLOCKS) blocks = SE_SHORTCUT_MAX_BLOCKS;
    return dim3((unsigned)blocks);
}

// the checks both entry points share; SE_OK, or an error code with the text set
static int sc_check(const char *who, int dtype, int layout, int64_t B, int64_t C, int64_t H, int64_t W, int64_t Cin, int64_t Hx, int64_t Wx,
                    int stride, int64_t pad)
{
    if (!is_float_dtype(dtype)) return fail(SE_ERR_INVALID, "%s: bad dtype code %d", who, dtype);
    if (layout != SE_LAYOUT_NCHW && layout != SE_LAYOUT_NHWC) return fail(SE_ERR_INVALID, "%s: bad layout code %d", who, layout);
    if (B < 0 || C < 0 || H < 0 || W < 0 || Cin < 0 || Hx < 0 || Wx < 0 || pad < 0)
        return fail(SE_ERR_INVALID, "%s: negative extent", who);
    if (stride != 1 && stride != 2) return fail(SE_ERR_UNSUPPORTED, "%s: stride %d (1 and 2 are implemented)", who, stride);
    if (Cin + pad > C)
        return fail(SE_ERR_INVALID, "%s: %lld channels of x behind %lld padded ones do not fit the %lld of s", who, (long long)Cin,
                    (long long)pad, (long long)C);
    if (H != Hx / stride || W != Wx / stride)
        return fail(SE_ERR_INVALID, "%s: s is %lld x %lld but x, %lld x %lld, pools to %lld x %lld at stride %d", who, (long long)H,
                    (long long)W, (long long)Hx, (long long)Wx, (long long)(Hx / stride), (long long)(Wx / stride), stride);
    return SE_OK;
}

}  // namespace se

using namespace se;

extern "C" int se_shortcut_add_fwd(const void *s, const void *x, void *out, int dtype, int layout, int64_t B, int64_t C, int64_t H,
                                   int64_t W, int64_t Cin, int64_t Hx, int64_t Wx, int stride, int64_t pad_before, se_stream_t stream)
{
    const int rc = sc_check("se_shortcut_add_fwd", dtype, layout, B, C, H, W, Cin, Hx, Wx, stride, pad_before);
    if (rc != SE_OK) return rc;
    const int64_t total = B * C * H * W;
    if (total == 0) return SE_OK;
    if (!s || !out || (!x && Cin > 0)) return fail(SE_ERR_INVALID, "se_shortcut_add_fwd: null pointer");
    const bool bf16 = dtype == SE_DTYPE_BF16;
    const int eb = bf16 ? 2 : 4, vmax = 16 / eb;
    ScGeom g = {};
    g.C = C, g.H = H, g.W = W, g.Cin = Cin, g.Hx = Hx, g.Wx = Wx, g.pad = pad_before;
    hipStream_t st = (hipStream_t)stream;
    if (layout == SE_LAYOUT_NCHW && stride == 2) {
        const int v = Cin > 0 ? sc_vector_width(vmax, eb, {W, Wx}, {s, x, out}) : sc_vector_width(vmax, eb, {W}, {s, out});
        g.units = total / v;
        dispatch_bools(bf16, [&](auto BF) {
            sc_dispatch_width(v, [&](auto V) {
                if constexpr (sc_fits<BF(), V()>)
                    hipLaunchKernelGGL((shortcut_nchw2_fwd_kernel<BF(), V()>), sc_grid(g.units), dim3(SC_THREADS), 0, st, s, x, out, g);
            });
        });
    } else {
        const int64_t plane = layout == SE_LAYOUT_NCHW ? H * W : 1;       // NCHW, stride 1: an image is one row
        g.L = C * plane, g.off = pad_before * plane, g.n = Cin * plane;
        const int v = Cin > 0 ? sc_vector_width(vmax, eb, {g.L, g.off, g.n}, {s, x, out}) : sc_vector_width(vmax, eb, {g.L}, {s, out});
        g.units = total / v;
        dispatch_bools(bf16, stride == 2, [&](auto BF, auto POOL) {
            sc_dispatch_width(v, [&](auto V) {
                if constexpr (sc_fits<BF(), V()>)
                    hipLaunchKernelGGL((shortcut_rows_fwd_kernel<BF(), V(), POOL() ? 4 : 1>), sc_grid(g.units), dim3(SC_THREADS), 0, st, s, x,
                                       out, g);
            });
        });
    }
    SE_LAUNCH_CHECK();
    return SE_OK;
}

extern "C" int se_shortcut_add_bwd(const void *dout, void *dx, int dtype, int layout, int64_t B, int64_t C, int64_t H, int64_t W,
                                   int64_t Cin, int64_t Hx, int64_t Wx, int stride, int64_t pad_before, se_stream_t stream)
{
    const int rc = sc_check("se_shortcut_add_bwd", dtype, layout, B, C, H, W, Cin, Hx, Wx, stride, pad_before);
    if (rc != SE_OK) return rc;
    const int64_t total = B * Cin * Hx * Wx;                               // elements of dx
    if (total == 0) return SE_OK;
    if (!dx || (!dout && H * W > 0)) return fail(SE_ERR_INVALID, "se_shortcut_add_bwd: null pointer");
    const bool bf16 = dtype == SE_DTYPE_BF16;
    const int eb = bf16 ? 2 : 4, vmax = 16 / eb;
    ScGeom g = {};
    g.C = C, g.H = H, g.W = W, g.Cin = Cin, g.Hx = Hx, g.Wx = Wx, g.pad = pad_before;
    hipStream_t st = (hipStream_t)stream;
    if (layout == SE_LAYOUT_NCHW && stride == 2) {
        // a unit of V columns of dx reads V / 2 of dout: dout is aligned to half the unit's bytes at least
        int v = sc_vector_width(vmax, eb, {Wx}, {dx});
        while (v > 1 && ((uintptr_t)dout % (uintptr_t)(v / 2 * eb)) != 0) v >>= 1;
        g.units = total / v;
        dispatch_bools(bf16, [&](auto BF) {
            sc_dispatch_width(v, [&](auto V) {
                if constexpr (sc_fits<BF(), V()>)
                    hipLaunchKernelGGL((shortcut_nchw2_bwd_kernel<BF(), V()>), sc_grid(g.units), dim3(SC_THREADS), 0, st, dout, dx, g);
            });
        });
    } else {
        const int64_t plane = layout == SE_LAYOUT_NCHW ? H * W : 1;
        g.L = C * plane, g.off = pad_before * plane, g.n = Cin * plane;
        const int v = sc_vector_width(vmax, eb, {g.L, g.off, g.n}, {dout, dx});
        g.units = total / v;
        dispatch_bools(bf16, stride == 2, [&](auto BF, auto POOL) {
            sc_dispatch_width(v, [&](auto V) {
                if constexpr (sc_fits<BF(), V()>)
                    hipLaunchKernelGGL((shortcut_rows_bwd_kernel<BF(), V(), POOL() ? 4 : 1>), sc_grid(g.units), dim3(SC_THREADS), 0, st, dout,
                                       dx, g);
            });
        });
    }
    SE_LAUNCH_CHECK();
    return SE_OK;
}
