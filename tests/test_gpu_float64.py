"""GPU: the opt-in float64 retrieval path -- se_pairwise_dist_f64 against the sequential float64 FMA chain bit for bit,
se_rank_refine_f64 against np.lexsort on crafted rows, pairwise_retrieval(precision='float64') against the chain (Gate 1) and
against NumPy's own float64 result (Gate 2), the case float32 ranks differently, and ``evaluate_retrieval.py --float64``.
The contract is DESIGN.md section 3.1; the restatement is tests/_f64_canon.py."""
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

import _f64_canon as fc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53


def _odd(n):
    return n + 1 + (n % 2)          # an odd leading dimension > n


def _dev_view(host, ld, dtype=None):
    """``host`` [r, c] on the device as a view of an [r, ld] buffer (ld > c: rows are not contiguous with each other)."""
    t = torch.from_numpy(np.ascontiguousarray(host))
    buf = torch.full((host.shape[0], ld), -7, dtype=t.dtype if dtype is None else dtype, device="cuda")
    buf[:, :host.shape[1]] = t.cuda()
    return buf[:, :host.shape[1]]


# ---------------------------------------------------------------- 1. the chain, bit for bit

def _special_features(rng, rows, d):
    x = rng.standard_normal((rows, d))
    x[0, 0] = -0.0
    if rows > 5:
        x[1, 0], x[2, d - 1], x[3, 0], x[4, d - 1], x[5, 0] = 0.0, -0.0, 5e-324 * 3, np.inf, np.nan      # +-0, a denormal, inf, NaN
    return x


@pytest.mark.parametrize("cosine", [True, False])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 7, 100, 130])
def test_pairwise_dist_f64_is_the_sequential_fma_chain(d, cosine):
    import sehip
    rng = np.random.default_rng(100 + d)
    for q, n in ((1, 1), (33, 33), (70, 70), (5, 19)):
        b = _special_features(rng, n, d)
        a = b if q == n else _special_features(rng, q, d)
        with np.errstate(all="ignore"):
            sqa, sqb = np.sum(a ** 2, axis=-1), np.sum(b ** 2, axis=-1)
        want = fc.chain_dist(a, b, cosine, sqa, sqb)
        ad = _dev_view(a, d + 3)
        bd = ad if q == n else _dev_view(b, d + 5)
        out = torch.full((q, _odd(n)), -7.0, dtype=torch.float64, device="cuda")
        img = torch.full((q, _odd(n) + 2), -7.0, dtype=torch.float32, device="cuda")
        got, gimg = sehip.pairwise_dist_f64(ad, None if q == n else bd, metric=sehip.METRIC_COSINE if cosine else sehip.METRIC_EUCLID,
                                            sqa=None if cosine else torch.from_numpy(sqa).cuda(),
                                            sqb=None if cosine else torch.from_numpy(sqb).cuda(), out=out[:, :n], img=img[:, :n])
        got, gimg = got.cpu().numpy(), gimg.cpu().numpy()
        assert fc.same_bits(got, want), (q, n, d, cosine)
        with np.errstate(all="ignore"):
            assert fc.same_bits(gimg, got.astype(np.float32)), (q, n, d, cosine)
        assert (out[:, n:] == -7.0).all() and (img[:, n:] == -7.0).all()          # nothing written past a row
        if q > 5:       # the special values did reach the result
            assert np.isnan(got[:, 5]).all() and not np.isnan(got[6:, 6:]).any()


def test_pairwise_dist_f64_without_image_and_argument_checks():
    import sehip
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((9, 6))).cuda()
    out, img = sehip.pairwise_dist_f64(x, img=None)
    assert img is None and fc.same_bits(out.cpu().numpy(), fc.chain_dist(x.cpu().numpy(), x.cpu().numpy(), True))
    with pytest.raises(sehip.SehipError, match="float64"):
        sehip.pairwise_dist_f64(x.float())
    with pytest.raises(sehip.SehipError, match="sqa"):
        sehip.pairwise_dist_f64(x, metric=sehip.METRIC_EUCLID)
    with pytest.raises(sehip.SehipError, match="SE_METRIC"):
        sehip.pairwise_dist_f64(x, metric=sehip.METRIC_DOT)
    rank16 = torch.zeros((9, 9), dtype=torch.int16, device="cuda")
    with pytest.raises(sehip.SehipError):
        sehip.rank_refine_f64_(out, out.float(), rank16)


# ---------------------------------------------------------------- 2. the repair

def _with_runs(base, runs, rng):
    """``base`` (ascending distinct float32-representable values) with, for every (first rank, length), that many values sharing the
    image of base[first] and differing in float64 -- in shuffled order, some of them tied exactly."""
    row = base.copy()
    for first, length in runs:
        steps = rng.permutation(length).astype(np.float64)
        if length >= 4:
            steps[:2] = steps[2]                                            # exact float64 ties inside the run
        row[first:first + length] = base[first] * (1.0 + steps * 2.0 ** -40)
        assert (row[first:first + length].astype(np.float32) == np.float32(base[first])).all()
    return row


def _repair_rows(n):
    rng = np.random.default_rng(n)
    base = np.sort(rng.standard_normal(4 * n).astype(np.float32))
    base = np.unique(base[base != 0])[:n].astype(np.float64)
    assert len(base) == n
    rows = [rng.permutation(base)]                                          # all-distinct images: nothing may change
    if n == 2:
        rows += [np.array([1.0 + 2.0 ** -40, 1.0]), np.array([0.0, -0.0]), np.array([np.nan, np.nan]), np.array([1.5, 1.5]),
                 np.array([np.nan, -1.0])]
    else:
        lengths = [L for L in (2, 3, 65) if 3 * L + 6 <= n]
        for L in lengths:                                                   # start, middle and end of the row
            rows.append(rng.permutation(_with_runs(base, [(0, L), (n // 2, L), (n - L, L)], rng)))
        mixed = _with_runs(base, [(3, 5)], rng)
        mixed[10:16] = [0.0, -0.0, -0.0, 0.0, -0.0, 0.0]                    # one run of zeros of both signs: index-ascending
        mixed[20:27] = np.nan                                               # NaNs last, index-ascending
        rows.append(rng.permutation(mixed))
    if n >= 3001:                                                           # a run beyond the LDS sort next to ones within it
        rows.append(rng.permutation(_with_runs(base, [(1, 2), (100, 65), (700, 1500), (2900, 8), (2990, 9)], rng)))
    rows.append(1.0 + np.arange(n)[::-1] * 2.0 ** -40)                      # ONE run, in descending index order
    return np.stack(rows)


@pytest.mark.parametrize("idx64", [False, True])
@pytest.mark.parametrize("n", [2, 64, 1000, 3001, 65536, 65537])
def test_rank_refine_f64_equals_lexsort(n, idx64):
    """65,536 columns: the longest row whose image tokens are staged in LDS; 65,537: the kernel that gathers every image."""
    import sehip
    d64 = _repair_rows(n)
    img = d64.astype(np.float32)
    first = fc.canon_rank(img.astype(np.float64))                            # what se_rank_rows returns for the image
    want = fc.canon_rank(d64)
    assert np.array_equal(first[0], want[0]) and np.array_equal(want[-1], np.arange(n)[::-1])
    assert not np.array_equal(first[1:], want[1:])
    dtype = np.int64 if idx64 else np.int32
    rank = _dev_view(first.astype(dtype), _odd(n) + 2)
    got = sehip.rank_refine_f64_(_dev_view(d64, _odd(n)), _dev_view(img, _odd(n) + 4), rank)
    assert got.data_ptr() == rank.data_ptr()
    got = got.cpu().numpy()
    for i in range(len(want)):
        assert np.array_equal(got[i], want[i]), (n, idx64, i)
    assert rank._base[:, n:].eq(-7).all()                                    # nothing written past a row


def test_rank_rows_f64_composes_ranking_and_repair():
    """The two kernels in sequence on a real image: se_rank_rows, then the repair."""
    import sehip
    d64 = _repair_rows(1000)
    got = sehip.rank_rows_f64(torch.from_numpy(d64).cuda(), torch.from_numpy(d64.astype(np.float32)).cuda()).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, fc.canon_rank(d64))


# ---------------------------------------------------------------- 3. / 4. end to end

N_E2E, D_E2E, SEED_E2E = 300, 100, 20261020
_e2e_cache = {}


def _e2e(normalize):
    """Features, the path's rankings [N, N] and NumPy's own float64 distances -- computed once per metric and not modified."""
    if normalize not in _e2e_cache:
        import evaluate_retrieval as er
        x = np.random.default_rng(SEED_E2E).standard_normal((N_E2E, D_E2E))
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)                   # the float64 path does not warn
            res = er.pairwise_retrieval(x.copy(), normalize=normalize, return_generator=False, precision='float64')
        ranks = np.array([res[i] for i in range(N_E2E)])
        _e2e_cache[normalize] = (x, ranks, fc.numpy_dist(x, normalize))
        for a in _e2e_cache[normalize]:
            a.setflags(write=False)
    return _e2e_cache[normalize]


@pytest.mark.parametrize("normalize", [True, False])
def test_pairwise_retrieval_float64_gate1_ranks_of_the_chain(normalize):
    """Gate 1: every sampled row is the stable argsort of the canonical chain's distances."""
    x, ranks, _ = _e2e(normalize)
    rows = np.random.default_rng(1).choice(N_E2E, 24, replace=False)
    if normalize:
        xn = x / np.linalg.norm(x, axis=-1, keepdims=True)
        want = fc.chain_dist(xn[rows], xn, True)
    else:
        sq = np.sum(x ** 2, axis=-1)
        want = fc.chain_dist(x[rows], x, False, sq[rows], sq)
    assert np.array_equal(ranks[rows], fc.canon_rank(want))


@pytest.mark.parametrize("normalize", [True, False])
def test_pairwise_retrieval_float64_gate2_ranks_of_numpy(normalize):
    """Gate 2: NumPy's float64 ranking, for every row, given that no row has a near-tie.  Two evaluations of a length-D dot product
    in any summation order differ by at most 2 gamma_D sum_k |x_ik x_jk| (each is within gamma_D of the exact value), which the
    distance doubles in the Euclidean form; that form adds three roundings (the sum of the norms, the subtraction on either side),
    each at most u times the largest magnitude involved, m = max(|s|, |distance|).  Two adjacent distances can each move by that
    much, so the gap must exceed twice the bound: 2 (4 gamma_D max_j sum_k |x_ik x_jk| + 3 u m) is asserted first, for every row."""
    x, ranks, dist = _e2e(normalize)
    xs = x / np.linalg.norm(x, axis=-1, keepdims=True) if normalize else x
    gamma = D_E2E * U / (1.0 - D_E2E * U)
    absdot = (np.abs(xs) @ np.abs(xs).T).max(axis=1)
    sq = np.sum(xs ** 2, axis=-1)
    mag = np.maximum(np.abs(dist).max(axis=1), 0.0 if normalize else sq + sq.max())
    bound = 2.0 * (4.0 * gamma * absdot + 3.0 * U * mag)
    gaps = np.diff(np.sort(dist, axis=1), axis=1).min(axis=1)
    assert (gaps > bound).all(), (gaps.min(), bound.max())
    assert gaps.min() > 1e4 * bound.max()                                    # (not a close call: ~1e-8 against ~1e-13)
    assert np.array_equal(ranks, np.argsort(dist, axis=1, kind='stable'))


# ---------------------------------------------------------------- 5. the point of it all

def test_float64_path_keeps_the_order_float32_loses():
    """Item 1 is item 2 with one coordinate moved by 2^-40: their float64 distances to query 0 differ (item 2 is nearer), their
    float32 features -- and distances -- are equal, so the float32 kernels return them by index."""
    import evaluate_retrieval as er
    x = np.array([[0.0, 0.0, 0.0], [1.0 + 2.0 ** -40, 0.5, 0.25], [1.0, 0.5, 0.25], [3.0, -1.0, 2.0], [-2.0, 0.5, 1.0]])
    want = np.argsort(fc.numpy_dist(x, False), axis=1, kind='stable')
    assert want[0].tolist()[:3] == [0, 2, 1]
    got64 = er.pairwise_retrieval(x.copy(), normalize=False, return_generator=False, precision='float64')
    assert [got64[i] for i in range(5)] == want.tolist()
    with pytest.warns(RuntimeWarning, match='float64 features'):
        got32 = er.pairwise_retrieval(x.copy(), normalize=False, return_generator=False)
    assert got32[0][:3] == [0, 1, 2]


# ---------------------------------------------------------------- 6. the command line

def _cli_problem(tmp_path):
    from datasets import get_data_generator
    g = np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))
    hpath = tmp_path / "cifar.parent-child.txt"
    with open(hpath, "w") as f:
        for p, c in g["edges"]:
            f.write("%d %d\n" % (p, c))
    ds = "synthetic:100x8x64x300"
    labels = list(get_data_generator(ds, None).labels_test)
    rng = np.random.default_rng(4)
    centers = rng.standard_normal((100, 24))
    feats = centers[labels] + 0.8 * rng.standard_normal((len(labels), 24))
    dump = tmp_path / "feat64.pickle"
    with open(dump, "wb") as f:
        pickle.dump({"feat": {i: feats[i].tolist() for i in range(len(labels))}}, f)      # lists: np.stack makes them float64
    return ds, str(hpath), str(dump), labels, feats


@pytest.mark.parametrize("norm", ["yes", "no"])
def test_evaluate_retrieval_cli_float64(tmp_path, capsys, norm):
    """``--float64`` on a 300-image float64 pickle: the table of the host mirror fed with NumPy's float64 rankings, to the tolerance
    of the float32 drop-in test, and no cast warning."""
    import evaluate_retrieval as er
    from class_hierarchy import ClassHierarchy
    ds, hpath, dump, labels, feats = _cli_problem(tmp_path)
    assert len(labels) == 300
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        perf = er.main(["--dataset", ds, "--data_root", str(tmp_path), "--hierarchy", hpath, "--feat", dump, "--label", "run", "--norm", norm,
                        "--plot_max", "0", "--float64"])
    assert not [w for w in seen if "float64" in str(w.message)]
    assert "AHP (WUP)" in capsys.readouterr().out
    rk = np.argsort(fc.numpy_dist(feats, norm == "yes"), axis=1, kind='stable')
    h = ClassHierarchy.from_file(hpath, id_type=int)
    want, _ = h.hierarchical_precision({i: rk[i].tolist() for i in range(len(labels))}, labels, [1, 10, 50, 100], compute_ahp=True,
                                       compute_ap=True, all_ids=list(range(len(labels))))
    for m, v in want.items():
        assert perf["run"][m] == pytest.approx(v, rel=1e-10, abs=1e-10), m


def test_recall_precision_device_float64(tmp_path):
    """plot_recall_precision.py --float64 goes through recall_precision_device(precision='float64'): the host statement of the
    reference's loop on NumPy's float64 rankings."""
    from recall_precision import recall_precision_device, recall_precision_host
    _, _, _, labels, feats = _cli_problem(tmp_path)
    levels, means, mAP, ap = recall_precision_device(feats, labels, normalize=True, precision='float64', tile_rows=128)
    rk = np.argsort(fc.numpy_dist(feats, True), axis=1, kind='stable')
    wl, wm, wmap, wap = recall_precision_host(rk, labels)
    assert np.allclose(levels, wl, rtol=0, atol=1e-12) and np.allclose(means, wm, rtol=1e-10, atol=1e-10)
    assert mAP == pytest.approx(wmap, rel=1e-10) and np.allclose(ap, wap, rtol=1e-10, atol=1e-10)
