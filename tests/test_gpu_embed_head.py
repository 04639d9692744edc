"""se_embed_head_fwd (csrc/embed_head.hip) against the entry points it fuses, bit for bit.

The contract of include/sehip.h: mode 0 writes what se_cosine_loss_fwd writes and what se_nn_accuracy(dot_prod_sim = 1) computes
from that xhat; mode 1 what se_sqdist_loss_fwd writes and what se_nn_accuracy(dot_prod_sim = 0) computes from float32(x); the metric
arrives as the two counts, from which every k follows.  Every case here runs the siblings on the same inputs (same pitches, same
alignment) and compares int32 views.  Shapes are the small ones at which the kernel changes path: a partial 32-sample strip and several
strips, D on the scalar / odd-k / staged-chunk / 16-byte boundaries, class sets of one tile up to sliced ones, partial rounds of the
four waves, and the layouts that switch off the vector loads."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

POISON_F = -12345.5
POISON_I = -777
KS = (1, 2, 5)


def _call(*a):
    from sehip._lib import call
    return call(*a)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_f(a, b, nan_rows=None):
    """float tensors equal bit for bit; on rows flagged in nan_rows only NaN-ness is compared"""
    if nan_rows is None or not bool(nan_rows.any()):
        return torch.equal(_bits(a), _bits(b))
    keep = ~nan_rows
    return torch.equal(_bits(a[keep]), _bits(b[keep])) and torch.equal(torch.isnan(a[nan_rows]), torch.isnan(b[nan_rows]))


def _matrix(rows, cols, layout, dtype, gen, dev):
    """[rows, cols] view with the layout's pitch / alignment; padding holds NaN.  contig: pitch = cols; padded: pitch = cols + 8
    rounded to 8; off1: base one element past a 16-byte boundary, pitch cols + 1."""
    vals = torch.randn((rows, cols), generator=gen, dtype=torch.float32).to(dev).to(dtype)
    if layout == "contig":
        return vals.contiguous()
    if layout == "padded":
        ld = (cols // 8 + 2) * 8
        buf = torch.full((rows, ld), float("nan"), dtype=dtype, device=dev)
        buf[:, :cols] = vals
        return buf[:, :cols]
    assert layout == "off1"
    ld = cols + 1
    buf = torch.full((rows * ld + 8,), float("nan"), dtype=dtype, device=dev)
    view = buf[1:1 + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(vals)
    return view


def _out_f(rows, cols, pad, dev):
    buf = torch.full((rows, cols + pad), POISON_F, dtype=torch.float32, device=dev)
    return buf, buf[:, :cols]


class Result(object):
    pass


def run_head(mode, x, labels, emb, ldxhat_pad=0, lds_pad=0, skip=(), want_scores=True):
    """one se_embed_head_fwd through the C ABI on caller buffers; `skip`: optional outputs passed as NULL"""
    dev = x.device
    B, D = x.shape
    C = emb.shape[0]
    r = Result()
    r.xhat_buf, r.xhat = _out_f(B, D, ldxhat_pad, dev)
    r.scores_buf, r.scores = _out_f(B, C, lds_pad, dev)
    for name in ("inv_norm", "loss_i", "dist_i"):
        setattr(r, name, torch.full((B,), POISON_F, dtype=torch.float32, device=dev))
    r.loss_mean = torch.full((1,), POISON_F, dtype=torch.float32, device=dev)
    for name in ("n_better", "n_within", "best"):
        setattr(r, name, torch.full((B,), POISON_I, dtype=torch.int32, device=dev))
    need = _call("se_embed_head_workspace_bytes", mode, B, D, C)
    ws = torch.full((need // 8,), -1, dtype=torch.int64, device=dev) if need else None     # dirty: the call zeroes what it needs
    r.need = need

    def opt(name, t):
        return None if (name in skip or (name == "scores" and not want_scores)) else t

    dt = 0 if x.dtype == torch.float32 else 1
    _call("se_embed_head_fwd", mode, x, dt, x.stride(0) if B > 1 else max(x.stride(0), D), labels, emb, emb.stride(0) if C > 1 else max(emb.stride(0), D),
          B, D, C, opt("xhat", r.xhat), D + ldxhat_pad, opt("inv_norm", r.inv_norm), r.loss_i, opt("dist_i", r.dist_i), opt("loss_mean", r.loss_mean),
          r.n_better, r.n_within, opt("best", r.best), opt("scores", r.scores), C + lds_pad, ws, need)
    return r


def run_siblings(mode, x, labels, emb, ldxhat_pad=0, lds_pad=0, ks=KS):
    """the parent's sequence on the same inputs: the loss entry point, then one se_nn_accuracy per k"""
    dev = x.device
    B, D = x.shape
    C = emb.shape[0]
    r = Result()
    r.xhat_buf, r.xhat = _out_f(B, D, ldxhat_pad, dev)
    r.scores_buf, r.scores = _out_f(B, C, lds_pad, dev)
    for name in ("inv_norm", "loss_i", "dist_i"):
        setattr(r, name, torch.full((B,), POISON_F, dtype=torch.float32, device=dev))
    r.loss_mean = torch.full((1,), POISON_F, dtype=torch.float32, device=dev)
    r.best = torch.full((B,), POISON_I, dtype=torch.int32, device=dev)
    dt = 0 if x.dtype == torch.float32 else 1
    ldx = x.stride(0) if B > 1 else max(x.stride(0), D)
    lde = emb.stride(0) if C > 1 else max(emb.stride(0), D)
    if mode == 0:
        _call("se_cosine_loss_fwd", x, dt, ldx, labels, emb, lde, B, D, C, r.xhat, D + ldxhat_pad, r.inv_norm, r.loss_i, r.loss_mean)
        yp, ldp = r.xhat, D + ldxhat_pad
    else:
        _call("se_sqdist_loss_fwd", x, dt, ldx, labels, emb, lde, B, D, C, r.loss_i, r.dist_i, r.loss_mean)
        yp = x.float().contiguous()
        ldp = D
    need = _call("se_nn_accuracy_workspace_bytes", B, C)
    r.acc = {}
    for k in tuple(ks) + (C,):
        acc = torch.full((B,), POISON_F, dtype=torch.float32, device=dev)
        ws = torch.empty((need // 8,), dtype=torch.int64, device=dev) if need else None
        _call("se_nn_accuracy", yp, ldp, labels, emb, lde, B, D, C, 1 if mode == 0 else 0, k, acc, r.scores, C + lds_pad, r.best, ws, need)
        r.acc[k] = acc
    return r


def compare(mode, got, want, nan_rows=None, skip=(), scores=True):
    assert _same_f(got.loss_i, want.loss_i, nan_rows), "loss_i"
    if nan_rows is None or not bool(nan_rows.any()):
        if "loss_mean" not in skip:
            assert _same_f(got.loss_mean, want.loss_mean), "loss_mean"
    elif "loss_mean" not in skip:
        assert torch.equal(torch.isnan(got.loss_mean), torch.isnan(want.loss_mean))
    if mode == 0:
        if "xhat" not in skip:
            assert _same_f(got.xhat, want.xhat, nan_rows), "xhat"
            assert bool((got.xhat_buf[:, got.xhat.shape[1]:] == POISON_F).all()), "xhat pitch padding written"
        if "inv_norm" not in skip:
            assert _same_f(got.inv_norm, want.inv_norm, nan_rows), "inv_norm"
        assert bool((got.dist_i == POISON_F).all())
    else:
        if "dist_i" not in skip:
            assert _same_f(got.dist_i, want.dist_i, nan_rows), "dist_i"
        assert bool((got.xhat_buf == POISON_F).all()) and bool((got.inv_norm == POISON_F).all())
    if scores and "scores" not in skip:
        assert _same_f(got.scores, want.scores, nan_rows), "scores"
        assert bool((got.scores_buf[:, got.scores.shape[1]:] == POISON_F).all()), "scores pitch padding written"
    if "best" not in skip:
        assert torch.equal(got.best, want.best), "best"
    for k, acc in want.acc.items():
        derived = ((got.n_within >= 1) & (got.n_better < k)).float()
        assert torch.equal(derived, acc), "accuracy k=%d" % k
    for name in skip:
        t = getattr(got, name + "_buf", None)
        t = getattr(got, name) if t is None else t
        poison = POISON_I if t.dtype == torch.int32 else POISON_F
        assert bool((t == poison).all()), "%s was NULL but its buffer changed" % name


def make_inputs(B, D, C, dtype, x_layout="contig", e_layout="contig", seed=0):
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(1000 * seed + B * 7 + D * 3 + C)
    x = _matrix(B, D, x_layout, dtype, gen, dev)
    emb = _matrix(C, D, e_layout, torch.float32, gen, dev)
    emb.copy_(torch.nn.functional.normalize(emb.clone(), dim=1) if D > 1 else emb.clone())
    labels = torch.randint(0, C, (B,), generator=gen).to(dev)
    return x, labels, emb


# B in {1, 31, 32, 33, 67}, D in {1, 7, 64, 65, 100, 136}, C in {1, 31, 33, 100}: every value with both modes and both dtypes;
# C = 161 / 1000 at B = 64, D = 24 (class slices; the head cuts them into slices of four tiles, the sibling under tile32::tiles_per_block);
# B = 8192, D = 8, C = 161 (the sibling's slices of two tiles with an empty last one; the head: one slice, a second round of two waves);
# B = 2048, D = 8, C = 1000 (the head: four slices of two rounds each); D = 200 at C = 200 (two slices of 4 + 3 tiles, four k chunks)
SHAPES = [(1, 1, 1), (31, 7, 31), (32, 64, 33), (33, 65, 100), (67, 100, 100), (67, 136, 33), (33, 136, 1), (1, 100, 31),
          (64, 24, 161), (64, 24, 1000), (8192, 8, 161), (2048, 8, 1000), (40, 200, 200)]


def test_shape_table_covers_the_issue_values():
    assert {s[0] for s in SHAPES} >= {1, 31, 32, 33, 67, 64, 8192}
    assert {s[1] for s in SHAPES} >= {1, 7, 64, 65, 100, 136, 24, 8}
    assert {s[2] for s in SHAPES} >= {1, 31, 33, 100, 161, 1000}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1], ids=["cosine", "sqdist"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_output_matches_the_separate_entry_points(shape, mode, dtype):
    B, D, C = shape
    x, labels, emb = make_inputs(B, D, C, dtype)
    got = run_head(mode, x, labels, emb)
    want = run_siblings(mode, x, labels, emb)
    compare(mode, got, want)
    sliced = (C + 31) // 32 > 4 and (B + 31) // 32 < 256
    assert (got.need > 0) == sliced


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1], ids=["cosine", "sqdist"])
@pytest.mark.parametrize("layout", [("padded", "contig", 0, 0), ("contig", "padded", 0, 0), ("off1", "contig", 0, 0), ("contig", "off1", 0, 0),
                                    ("contig", "contig", 3, 0), ("contig", "contig", 0, 5), ("off1", "off1", 3, 5), ("padded", "padded", 4, 4)],
                         ids=lambda l: "-".join(map(str, l)))
def test_pitches_and_alignment(layout, mode, dtype):
    """ldx > D, lde > D, bases one element off a 16-byte boundary (element loads), ldxhat > D, lds > C; D = 136 is a multiple of 8 so
    that the aligned layouts take the 16-byte paths of both dtypes, 161 classes are sliced"""
    x_layout, e_layout, xpad, spad = layout
    for B, D, C in ((67, 136, 33), (40, 24, 161)):
        x, labels, emb = make_inputs(B, D, C, dtype, x_layout, e_layout, seed=1)
        got = run_head(mode, x, labels, emb, xpad, spad)
        want = run_siblings(mode, x, labels, emb, xpad, spad)
        compare(mode, got, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1], ids=["cosine", "sqdist"])
@pytest.mark.parametrize("C", [100, 161])
def test_special_rows(C, mode, dtype):
    B, D = 40, 24
    x, labels, emb = make_inputs(B, D, C, dtype, seed=2)
    emb = emb.to(torch.bfloat16).float()         # class rows a bf16 feature row can equal exactly
    x[0].zero_()                                 # all-zero features: the 1e-12 clamp, +-0 scores
    x[1].zero_(); x[1, 0] = -0.0
    emb[7] = emb[3]; labels[2] = 7               # two identical class rows, the label the higher one: n_within >= 2, best the lower
    x[2] = (emb[3] * 3).to(dtype)
    labels[3] = 3
    x[3] = (emb[3] * 3).to(dtype)
    x[4] = emb[11].to(dtype); labels[4] = 11     # a feature row equal to a class row
    x[5] = emb[12].to(dtype); labels[5] = 13     # ... of another class than the label
    labels[6] = -3; labels[8] = C + 5            # clamped like the siblings
    x[9, 5] = float("nan")
    x[10, :] = float("nan")
    x[11, 0] = float("inf")
    emb[20, :].zero_()                           # a zero class row: +-0 similarities
    nan_rows = torch.isnan(x.float()).any(dim=1) | torch.isinf(x.float()).any(dim=1)
    got = run_head(mode, x, labels, emb)
    want = run_siblings(mode, x, labels, emb)
    compare(mode, got, want, nan_rows=nan_rows)
    assert int(got.n_within[2]) >= 2 and int(got.best[2]) == 3 and int(got.best[3]) == 3
    assert int(got.n_within[4]) >= 1 and int(got.n_better[4]) == 0
    clamped = labels.clamp(0, C - 1)
    again = run_head(mode, x, clamped, emb)
    for name in ("loss_i", "n_better", "n_within", "best"):
        a, b = getattr(got, name), getattr(again, name)
        assert torch.equal(a[~nan_rows], b[~nan_rows]), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1], ids=["cosine", "sqdist"])
def test_each_optional_output_may_be_null(mode, dtype):
    for B, D, C in ((33, 24, 100), (40, 24, 161)):
        x, labels, emb = make_inputs(B, D, C, dtype, seed=3)
        want = run_siblings(mode, x, labels, emb)
        for name in ("xhat", "inv_norm", "dist_i", "loss_mean", "best", "scores"):
            got = run_head(mode, x, labels, emb, skip=(name,))
            compare(mode, got, want, skip=(name,))


def test_empty_batch_touches_nothing():
    x, labels, emb = make_inputs(4, 8, 5, torch.float32)
    bufs = [torch.full((4, 8), POISON_F, device="cuda") for _ in range(2)] + [torch.full((4,), POISON_F, device="cuda") for _ in range(4)]
    ints = [torch.full((4,), POISON_I, dtype=torch.int32, device="cuda") for _ in range(3)]
    for mode in (0, 1):
        rc = _call("se_embed_head_fwd", mode, x, 0, 8, labels, emb, 8, 0, 8, 5, bufs[0], 8, bufs[2], bufs[3], bufs[4], bufs[5],
                   ints[0], ints[1], ints[2], bufs[1], 8, None, 0)
        assert rc == 0
        assert _call("se_embed_head_fwd", mode, None, 0, 8, None, None, 8, 0, 8, 5, None, 8, None, None, None, None, None, None, None, None, 8, None, 0) == 0
    torch.cuda.synchronize()
    assert all(bool((b == POISON_F).all()) for b in bufs) and all(bool((i == POISON_I).all()) for i in ints)


def test_invalid_arguments_are_refused():
    import sehip
    lib = sehip.lib()
    B, D, C = 64, 24, 1000
    x, labels, emb = make_inputs(B, D, C, torch.float32)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    i = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    xhat, inv, loss, dist, mean, nb, nw, best, scores = f(B, D), f(B), f(B), f(B), f(1), i(B), i(B), i(B), f(B, C)
    need = lib.se_embed_head_workspace_bytes(0, B, D, C)
    assert need > 0 and lib.se_embed_head_workspace_bytes(0, B, D, 100) == 0 and lib.se_embed_head_workspace_bytes(1, 0, D, C) == 0
    ws = torch.zeros((need // 8 + 2,), dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    good = dict(mode=0, x=p(x), dt=0, ldx=D, labels=p(labels), emb=p(emb), lde=D, B=B, D=D, C=C, xhat=p(xhat), ldxhat=D, inv=p(inv), loss=p(loss),
                dist=p(dist), mean=p(mean), nb=p(nb), nw=p(nw), best=p(best), scores=p(scores), lds=C, ws=p(ws), wsb=need)
    order = list(good)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(**change):
        args = dict(good, **change)
        return lib.se_embed_head_fwd(*[args[k] for k in order], stream)

    assert run() == 0
    null = ctypes.c_void_p(0)
    bad = [dict(mode=2), dict(mode=-1), dict(dt=7), dict(x=null), dict(labels=null), dict(emb=null), dict(loss=null), dict(nb=null),
           dict(nw=null), dict(ldx=D - 1), dict(lde=D - 1), dict(ldxhat=D - 1), dict(lds=C - 1), dict(ws=null), dict(wsb=need - 8),
           dict(ws=ctypes.c_void_p(ws.data_ptr() + 4)), dict(D=0), dict(C=0), dict(B=-1)]
    for change in bad:
        assert run(**change) == sehip._lib.DEFINES["SE_ERR_INVALID"], change
        assert b"se_embed_head_fwd" in lib.se_last_error(), change
    assert run(mode=1, ldxhat=0, xhat=null, inv=null) == 0           # the other mode's outputs are ignored
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["cosine", "sqdist"])
@pytest.mark.parametrize("C", [100, 1000])
def test_graph_replay_equals_eager(C, mode, dtype):
    """one call captured as a single chain; inputs overwritten in place; C = 1000 covers the workspace re-initialisation on the stream"""
    import sehip
    B, D = 64, 24
    x, labels, emb = make_inputs(B, D, C, dtype, seed=4)
    kw = dict(mode=mode, want_xhat=True, want_inv_norm=True, want_dist=True, want_mean=True, want_scores=True, want_best=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sehip.embed_head_forward(x, labels, emb, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sehip.embed_head_forward(x, labels, emb, **kw)
    for seed in (5, 6):
        x2, labels2, _ = make_inputs(B, D, C, dtype, seed=seed)
        x.copy_(x2); labels.copy_(labels2)
        graph.replay()
        torch.cuda.synchronize()
        eager = sehip.embed_head_forward(x, labels, emb, **kw)
        for name, a, b in zip(out._fields, out, eager):
            assert (a is None) == (b is None), name
            if a is not None:
                assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_autograd_is_the_siblings_backward(dtype):
    import sehip
    x, labels, emb = make_inputs(67, 100, 100, dtype, seed=7)
    for mode, sibling in (("cosine", lambda a: sehip.cosine_embedding_loss(a, labels, emb, reduction="none")),
                          ("sqdist", lambda a: sehip.squared_distance_loss(a, labels, emb))):
        a = x.clone().requires_grad_(True)
        b = x.clone().requires_grad_(True)
        head = sehip.embedding_head(a, labels, emb, mode=mode, want_scores=True, want_best=True)
        head.loss_i.sum().backward()
        ref = sibling(b)
        ref.sum().backward()
        assert torch.equal(_bits(head.loss_i.detach()), _bits(ref.detach()))
        assert a.grad.dtype == b.grad.dtype and torch.equal(a.grad.float().view(torch.int32), b.grad.float().view(torch.int32))
        assert not head.n_better.requires_grad and not head.scores.requires_grad
        acc = sehip.nn_accuracy(head.xhat if mode == "cosine" else x.float(), labels, emb, dot_prod_sim=mode == "cosine", k=5)
        assert torch.equal(((head.n_within >= 1) & (head.n_better < 5)).float(), acc)
        assert (head.xhat is None) == (mode == "sqdist")
