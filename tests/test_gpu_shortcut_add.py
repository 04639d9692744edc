"""GPU: se_shortcut_add_fwd / se_shortcut_add_bwd (the pyramidal residual shortcut, sehip.shortcut_add) bit for bit against a NumPy
float32 restatement of the arithmetic include/sehip.h fixes -- both dtypes, both layouts, forward and dx, every vector width the
host picks, more than one workgroup, more than one trip of the grid-stride loop -- and, as a cross-check of the mathematics, against
the same expression in float64 within the bound the operation count gives."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, Cin, C, Hx, Wx, stride, pad_before)
CASES = {
    "odd_dropped_row_col": (2, 5, 9, 5, 5, 2, 0),
    "non_square": (2, 5, 9, 3, 7, 1, 0),
    "symmetric_pad": (2, 5, 9, 3, 7, 1, 2),
    "symmetric_pad_s2": (2, 5, 9, 4, 6, 2, 2),
    "cin_eq_c": (2, 6, 6, 4, 6, 1, 0),
    "cin_eq_c_s2": (2, 6, 6, 4, 6, 2, 0),
    "one_pixel": (2, 5, 9, 1, 1, 1, 0),
    "one_pixel_s2": (2, 5, 9, 2, 2, 2, 0),
    "one_pixel_s2_odd": (2, 5, 9, 3, 3, 2, 0),
    "wide_channels": (1, 861, 864, 2, 2, 1, 0),          # channel extent beyond one workgroup's 256 threads, several workgroups
    "wide_channels_s2": (1, 861, 864, 4, 4, 2, 0),
    # every access width: extents, offsets and the padding are multiples of k = 2, 4, 8 (and of nothing larger)
    "width2": (2, 2, 6, 3, 4, 2, 2), "width4": (2, 4, 12, 3, 8, 2, 4), "width8": (2, 8, 24, 3, 16, 2, 8),
    "width2_s1": (2, 2, 6, 1, 1, 1, 2), "width4_s1": (2, 4, 12, 1, 1, 1, 4), "width8_s1": (2, 8, 24, 1, 1, 1, 8),
    "pyramid_block": (2, 72, 80, 8, 8, 2, 0),           # a PyramidNet bottleneck transition in small: widths 4 n
    "empty_batch": (0, 5, 9, 5, 5, 2, 0),
    "empty_image": (2, 5, 9, 1, 1, 2, 0),               # H = W = 0: nothing to add, dx is all zero
    # more units than the capped grid has threads: a second trip of the grid-stride loop (V = 1: odd plane, odd channel counts)
    "grid_stride": (1, 5, 7, 331, 331, 1, 1),
}
DTYPES = ["float32", "bfloat16"]
LAYOUTS = ["nchw", "nhwc"]


# ---- bfloat16 as NumPy sees it: uint16 bit patterns ----

def bf16_widen(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def bf16_round(f):
    """float32 -> bf16 bits, round to nearest even (finite values)."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def to_dtype_bits(f, dtype):
    """(the bits an array of float32 values has in ``dtype``, the float32 values those bits stand for)"""
    if dtype == "float32":
        f = np.ascontiguousarray(f, dtype=np.float32)
        return f.view(np.uint32), f
    bits = bf16_round(f)
    return bits, bf16_widen(bits)


# ---- the oracle: include/sehip.h's arithmetic in NumPy float32, on NCHW-logical arrays ----

def oracle_fwd(s, x, stride, pad):
    """float32 ``out`` before the rounding to the dtype."""
    B, C, H, W = s.shape
    Cin = x.shape[1]
    four = np.float32(stride * stride)
    if stride == 1:
        acc = x.copy()
    else:
        acc = x[:, :, 0:2 * H:2, 0:2 * W:2].copy()
        acc = acc + x[:, :, 0:2 * H:2, 1:2 * W:2]
        acc = acc + x[:, :, 1:2 * H:2, 0:2 * W:2]
        acc = acc + x[:, :, 1:2 * H:2, 1:2 * W:2]
    pooled = acc / four
    out = s.copy()
    out[:, pad:pad + Cin] = s[:, pad:pad + Cin] + pooled
    return out.astype(np.float32)


def oracle_bwd(g, x_shape, stride, pad):
    B, Cin, Hx, Wx = x_shape
    H, W = g.shape[2:]
    dx = np.zeros(x_shape, dtype=np.float32)
    q = g[:, pad:pad + Cin] / np.float32(stride * stride)
    for i in range(stride):
        for j in range(stride):
            dx[:, :, i:stride * H:stride, j:stride * W:stride] = q
    return dx


# ---- device plumbing ----

def to_device(bits, dtype, layout):
    """NCHW-logical bit patterns -> a device tensor of ``dtype`` in ``layout``."""
    if dtype == "float32":
        t = torch.from_numpy(bits.view(np.float32).copy())
    else:
        t = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
    t = t.cuda()
    return t.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else t.contiguous()


def bits_of(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.float32:
        return t.numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


_INPUTS = {}


def inputs(case, dtype, same_sign_windows=False):
    """Seeded (s, x, g) of a case as (bits, float32 values) pairs, computed once.  ``same_sign_windows``: every channel of x has one
    sign, so no pooling window cancels (the float64 cross-check's bound needs that, see there)."""
    key = (case, dtype, same_sign_windows)
    if key not in _INPUTS:
        B, Cin, C, Hx, Wx, stride, pad = CASES[case]
        rng = np.random.default_rng(sorted(CASES).index(case) * 7 + DTYPES.index(dtype))
        s = rng.standard_normal((B, C, Hx // stride, Wx // stride)).astype(np.float32)
        x = rng.standard_normal((B, Cin, Hx, Wx)).astype(np.float32)
        if same_sign_windows:
            x = np.abs(x) * rng.choice(np.float32([-1, 1]), size=(B, Cin, 1, 1))
        g = rng.standard_normal(s.shape).astype(np.float32)
        _INPUTS[key] = tuple(to_dtype_bits(a, dtype) for a in (s, x, g))
    return _INPUTS[key]


def run(case, dtype, layout, same_sign_windows=False):
    import sehip
    B, Cin, C, Hx, Wx, stride, pad = CASES[case]
    (sb, sv), (xb, xv), (gb, gv) = inputs(case, dtype, same_sign_windows)
    s, x, g = (to_device(b, dtype, layout) for b in (sb, xb, gb))
    s.requires_grad_(True)
    x.requires_grad_(True)
    out = sehip.shortcut_add(s, x, stride, pad)
    ds, dx = torch.autograd.grad(out, (s, x), g)
    return (s, x, g), (out, ds, dx), (sv, xv, gv)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_forward_and_dx_are_bit_exact(case, dtype, layout):
    B, Cin, C, Hx, Wx, stride, pad = CASES[case]
    (s, x, g), (out, ds, dx), (sv, xv, gv) = run(case, dtype, layout)
    assert out.shape == s.shape and out.dtype == s.dtype and dx.shape == x.shape and dx.dtype == x.dtype
    fmt = torch.channels_last if layout == "nhwc" else torch.contiguous_format
    assert out.is_contiguous(memory_format=fmt) and dx.is_contiguous(memory_format=fmt)
    want_out, _ = to_dtype_bits(oracle_fwd(sv, xv, stride, pad), dtype)
    want_dx, _ = to_dtype_bits(oracle_bwd(gv, xv.shape, stride, pad), dtype)
    assert np.array_equal(bits_of(out), want_out), (case, dtype, layout)
    assert np.array_equal(bits_of(dx), want_dx), (case, dtype, layout)
    assert np.array_equal(bits_of(ds), bits_of(g))                  # the gradient of s is the incoming gradient
    # the operands are only read
    assert np.array_equal(bits_of(s), inputs(case, dtype)[0][0]) and np.array_equal(bits_of(x), inputs(case, dtype)[1][0])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["odd_dropped_row_col", "symmetric_pad", "width4", "wide_channels_s2"])
def test_two_calls_give_identical_bits(case, dtype, layout):
    _, (out1, _, dx1), _ = run(case, dtype, layout)
    _, (out2, _, dx2), _ = run(case, dtype, layout)
    assert np.array_equal(bits_of(out1), bits_of(out2)) and np.array_equal(bits_of(dx1), bits_of(dx2))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stride", [1, 2])
def test_padded_channels_are_copied_not_added_to(stride, dtype, layout):
    """-0.0, both infinities and NaNs with payloads in s at a padded channel come back with the same bits: the kernel copies there,
    it does not add 0.0f (which would turn -0.0 into +0.0 and could quieten a NaN)."""
    import sehip
    B, Cin, C, Hx, Wx, pad = 2, 4, 10, 4, 4, 3
    rng = np.random.default_rng(5)
    sb, _ = to_dtype_bits(rng.standard_normal((B, C, Hx // stride, Wx // stride)), dtype)
    xb, xv = to_dtype_bits(rng.standard_normal((B, Cin, Hx, Wx)), dtype)
    sb = sb.copy()
    # -0.0, +inf, -inf, a quiet NaN with a payload, a negative one, a signalling NaN
    special = (np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345, 0x7F800001], dtype=np.uint32) if dtype == "float32"
               else np.array([0x8000, 0x7F80, 0xFF80, 0x7FC1, 0xFFC5, 0x7F81], dtype=np.uint16))
    padded = [c for c in range(C) if not pad <= c < pad + Cin]
    for k, bits in enumerate(special):
        sb[k % B, padded[k % len(padded)], (k // 2) % sb.shape[2], k % sb.shape[3]] = bits
    s, x = to_device(sb, dtype, layout), to_device(xb, dtype, layout)
    got = bits_of(sehip.shortcut_add(s, x, stride, pad))
    assert np.array_equal(got[:, padded], sb[:, padded])
    sv = sb.view(np.float32) if dtype == "float32" else bf16_widen(sb)
    want, _ = to_dtype_bits(oracle_fwd(sv, xv, stride, pad)[:, pad:pad + Cin], dtype)
    assert np.array_equal(got[:, pad:pad + Cin], want)


def roundings_bound(stride, pooled, s, dtype):
    """|computed - exact| <= (stride^2 + 1) 2^-24 (|pooled| + |s|) in float32: stride^2 - 1 additions inside the window, the division
    (exact for 1 and 4, counted all the same) and the final add, each one rounding of relative size 2^-24 of a value that, with
    windows of one sign, is at most |acc| = stride^2 |pooled| before the division and |s| + |pooled| after it.  bfloat16 adds the
    one rounding of the result to its 8-bit significand, 2^-8 (|pooled| + |s|), and nothing else (its inputs are exact in float32)."""
    e = (stride * stride + 1) * 2.0 ** -24 * (np.abs(pooled) + np.abs(s))
    return e + (2.0 ** -8 * (np.abs(pooled) + np.abs(s)) if dtype == "bfloat16" else 0.0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["odd_dropped_row_col", "symmetric_pad", "pyramid_block", "wide_channels_s2"])
def test_float64_cross_check_and_autograd_against_the_torch_composition(case, dtype, layout):
    """The reference's mathematics, s + ChannelPadding(AveragePooling2D(stride)(x)), as the torch composition in float64 on the
    device, with autograd for both gradients; the kernel stays within the operation-count bound of it.  Nothing is measured."""
    B, Cin, C, Hx, Wx, stride, pad = CASES[case]
    (s, x, g), (out, ds, dx), _ = run(case, dtype, layout, same_sign_windows=True)
    s64, x64 = s.detach().double().requires_grad_(True), x.detach().double().requires_grad_(True)
    pooled = F.avg_pool2d(x64, stride) if stride > 1 else x64
    padded = F.pad(pooled, (0, 0, 0, 0, pad, C - Cin - pad))
    ref = s64 + padded
    rds, rdx = torch.autograd.grad(ref, (s64, x64), g.double())
    n = lambda t: t.detach().double().cpu().numpy()
    bound = roundings_bound(stride, n(padded), n(s64), dtype)
    assert (np.abs(n(out) - n(ref)) <= bound).all()
    # dx = g / stride^2: one operation on one value (and the bf16 rounding); ds = g itself
    gq = np.abs(n(rdx))
    assert (np.abs(n(dx) - n(rdx)) <= roundings_bound(stride, gq, 0.0 * gq, dtype)).all()
    assert torch.equal(ds.double(), rds)


def test_argument_checks_run_before_any_launch():
    """Raw ctypes, NULL pointers: the verdict comes from the host-side checks, nothing is launched."""
    import sehip
    lib = sehip.lib()
    z = ctypes.c_void_p(0)
    F32, BF16, NCHW, NHWC = sehip.DTYPE_F32, sehip.DTYPE_BF16, sehip.LAYOUT_NCHW, sehip.LAYOUT_NHWC
    INVALID, UNSUPPORTED = -1, -3
    #                                      dtype layout B  C  H  W  Cin Hx Wx stride pad
    assert lib.se_shortcut_add_fwd(z, z, z, F32, NCHW, 2, 9, 2, 2, 5, 6, 6, 3, 0, z) == UNSUPPORTED
    assert b"stride" in lib.se_last_error()
    assert lib.se_shortcut_add_bwd(z, z, BF16, NHWC, 2, 9, 2, 2, 5, 6, 6, 3, 0, z) == UNSUPPORTED
    assert lib.se_shortcut_add_fwd(z, z, z, F32, NCHW, 2, 9, 3, 2, 5, 5, 5, 2, 0, z) == INVALID      # 5 x 5 pools to 2 x 2
    assert lib.se_shortcut_add_bwd(z, z, F32, NCHW, 2, 9, 2, 3, 5, 5, 5, 2, 0, z) == INVALID
    assert lib.se_shortcut_add_fwd(z, z, z, F32, NHWC, 2, 9, 5, 4, 5, 5, 5, 1, 0, z) == INVALID      # stride 1 keeps the size
    assert lib.se_shortcut_add_fwd(z, z, z, F32, NCHW, 2, 9, 2, 2, 5, 5, 5, 2, 5, z) == INVALID      # 5 + 5 > 9 channels
    assert b"channels" in lib.se_last_error()
    assert lib.se_shortcut_add_fwd(z, z, z, 7, NCHW, 2, 9, 2, 2, 5, 5, 5, 2, 0, z) == INVALID        # dtype
    assert lib.se_shortcut_add_fwd(z, z, z, F32, 2, 2, 9, 2, 2, 5, 5, 5, 2, 0, z) == INVALID          # layout
    assert lib.se_shortcut_add_fwd(z, z, z, F32, NCHW, -1, 9, 2, 2, 5, 5, 5, 2, 0, z) == INVALID
    assert lib.se_shortcut_add_fwd(z, z, z, F32, NCHW, 2, 9, 2, 2, 5, 5, 5, 2, 0, z) == INVALID       # NULL pointers with B > 0
    assert b"null pointer" in lib.se_last_error()
    assert lib.se_shortcut_add_bwd(z, z, F32, NCHW, 2, 9, 2, 2, 5, 5, 5, 2, 0, z) == INVALID
    assert lib.se_shortcut_add_fwd(z, z, z, F32, NCHW, 0, 9, 2, 2, 5, 5, 5, 2, 0, z) == 0             # B = 0 is accepted
    assert lib.se_shortcut_add_bwd(z, z, BF16, NHWC, 0, 9, 2, 2, 5, 5, 5, 2, 0, z) == 0


def test_binding_refuses_mixed_operands():
    import sehip
    s = torch.randn(2, 9, 3, 3, device="cuda")
    x = torch.randn(2, 5, 3, 3, device="cuda")
    with pytest.raises(sehip.SehipError, match="layout"):
        sehip.shortcut_add(s.contiguous(memory_format=torch.channels_last), x)
    with pytest.raises(sehip.SehipError, match="dtype"):
        sehip.shortcut_add(s, x.bfloat16())
    with pytest.raises(sehip.SehipError, match="layout"):
        sehip.shortcut_add(s[:, :, :, ::2], x[:, :, :, ::2])
    with pytest.raises(sehip.SehipError):
        sehip.shortcut_add(s.double(), x.double())
    with pytest.raises(sehip.SehipError, match="stride"):
        sehip.shortcut_add(s, torch.randn(2, 5, 9, 9, device="cuda"), stride=3)
    with pytest.raises(sehip.SehipError):
        sehip.shortcut_add(s.cpu(), x.cpu())


def test_capturable_in_a_hip_graph():
    """No allocation, no synchronisation, no atomics in either entry point: a captured forward + backward replays to the same bits."""
    import sehip
    case, dtype, layout = "pyramid_block", "float32", "nhwc"
    B, Cin, C, Hx, Wx, stride, pad = CASES[case]
    (sb, sv), (xb, xv), (gb, gv) = inputs(case, dtype)
    s, x, g = (to_device(b, dtype, layout) for b in (sb, xb, gb))
    fmt = torch.channels_last
    out, dx = torch.empty_like(s, memory_format=fmt), torch.empty_like(x, memory_format=fmt)
    lib_call = sehip.ops.call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    args = (sehip.DTYPE_F32, sehip.LAYOUT_NHWC, B, C, Hx // stride, Wx // stride, Cin, Hx, Wx, stride, pad)
    lib_call("se_shortcut_add_fwd", s, x, out, *args)          # code objects are loaded before the capture
    lib_call("se_shortcut_add_bwd", g, dx, *args)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        lib_call("se_shortcut_add_fwd", s, x, out, *args)
        lib_call("se_shortcut_add_bwd", g, dx, *args)
    out.zero_()
    dx.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(out), to_dtype_bits(oracle_fwd(sv, xv, stride, pad), dtype)[0])
    assert np.array_equal(bits_of(dx), to_dtype_bits(oracle_bwd(gv, xv.shape, stride, pad), dtype)[0])
