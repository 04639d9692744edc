"""se_ndcg on the device against the NumPy restatement of its contract (tests/_ndcg_canon.py): every chunk form, class-table form,
place of the query's own entry and kind of cut-off list at the smallest shapes that reach them, through the C ABI with buffers the
test owns (rankings on their own pitch and base offset, ``out`` on a pitch of its own inside a sentinel-filled allocation); bit
equality where the contract promises it; the tie to se_hierarchical_precision; and the evaluation drivers end to end.

Bound: 1e-10 absolute, the bound this project holds hprec to.  The sums are non-negative, so float64 re-association costs about
list_len * 2^-53 relative: 5e-13 at the longest list here.  ``SE_NDCG_REPORT=<file>`` writes the worst deviation of every case."""
import os

import numpy as np
import pytest

import _ndcg_canon as canon
import _qg_standins as qg

pytestmark = pytest.mark.gpu

TOL = 1e-10
SENT = 0x7FF8DEADBEEF0001                              # a NaN no kernel computes
RECORDS = []


@pytest.fixture(scope="module")
def lib():
    import sehip
    from sehip import _lib
    sehip.lib()
    return _lib


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    path = os.environ.get("SE_NDCG_REPORT")
    if path and RECORDS:
        with open(path, "w") as f:
            f.write("se_ndcg vs tests/_ndcg_canon.py (float64), bound %g: worst absolute deviation per case\n\n" % TOL)
            f.write("\n".join(RECORDS) + "\n")
            f.write("\nworst of all: %.3e\n" % max(float(r.rsplit(" ", 1)[1]) for r in RECORDS))


def CH():
    import sehip
    return sehip.NDCG_CHUNK


def clsw_rule(L, q, gallery, C):
    """rank_stream.h's choose_class_table for shapes far below the LDS cap: 0 gathered, 1 bytes in LDS, 2 shorts in LDS."""
    if L * min(q, 4096) < 8 * gallery:
        return 0
    return 1 if C <= 256 else 2


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Case:
    """Random inputs of one call.  ``own``: per row the place of the query's own entry -- an int (clipped to the list), 'absent'
    (qidx = -1), 'missing' (a gallery item that is not in the list) -- or None for qidx == NULL."""

    def __init__(self, L, own, ks, want_full, gallery=64, C=10, ldr_pad=0, off=0, seed=0, poison=False, hot=False):
        rng = np.random.RandomState(1000 * seed + L % 977)
        self.L, self.ks, self.want_full, self.gallery, self.C, self.off = L, list(ks), want_full, gallery, C, off
        self.Q = Q = len(own) if own is not None else 6
        self.ldr = L + ldr_pad
        self.cls = rng.randint(0, C - 1, size=gallery).astype(np.int32)            # class C - 1 has no gallery item
        self.cls[: C - 1] = np.arange(C - 1)[:gallery]
        self.qcls = rng.randint(0, C, size=Q).astype(np.int32)
        self.qcls[0] = C - 1 if hot else self.qcls[0]                              # row 0: the class whose ideal is 0
        self.gain = [np.round(rng.rand(C, C), 3) for _ in range(2)]                # not symmetric; exact zeros among them
        for g in self.gain:
            g[rng.rand(C, C) < 0.2] = 0.0
            g[:, C - 1] = 1000.0                                                   # no gallery item has this class: see `poison`
        self.rank = rng.randint(0, gallery, size=(Q, L)).astype(np.int32)
        self.qidx = None
        if own is not None:
            self.qidx = np.zeros(Q, dtype=np.int32)
            for i, o in enumerate(own):
                self.qidx[i] = -1 if o == "absent" else rng.randint(gallery)
                if o == "absent":
                    continue
                row = self.rank[i]
                row[row == self.qidx[i]] = (self.qidx[i] + 1) % gallery
                if o != "missing":
                    row[min(int(o), L - 1)] = self.qidx[i]
        self.disc = canon.discounts(L + 3)
        nk = len(ks)
        reach = np.array([min(k, L) for k in ks] + [L])
        scale = np.concatenate(([0.0], np.cumsum(self.disc)))[reach]                # keeps the values of the order of 1
        self.ideal = (1.0 + rng.rand(C, 2, 2, nk + 1)) * scale
        if hot:
            self.ideal[C - 1] = 0.0
        self.read = L if want_full else min(L, max(ks) + 1)
        self.sent_rank = self.rank.copy()
        if poison:      # behind the part that is read: indices >= gallery, which land in a second half of `cls` that holds a class of gain 1000
            self.sent_rank[:, self.read:] += gallery
        self.want = canon.ndcg_rows(self.rank, L, self.cls, self.qcls, self.qidx, self.gain[0], self.gain[1], self.disc, self.ideal, ks, want_full)

    def device(self):
        import torch
        if not hasattr(self, "dev"):
            buf = torch.full((self.off + self.Q * self.ldr + 8,), 0x7FFFFFF0, dtype=torch.int32, device="cuda")     # pitch padding: far outside
            rows = buf[self.off: self.off + self.Q * self.ldr].view(self.Q, self.ldr)
            rows[:, :self.L] = up(self.sent_rank)
            assert buf.data_ptr() % 16 == 0
            cls2 = np.concatenate((self.cls, np.full(self.gallery, self.C - 1, dtype=np.int32)))
            gains = [g.copy() for g in self.gain]
            self.dev = dict(buf=buf, rows=rows, cls=up(cls2), qcls=up(self.qcls), qidx=None if self.qidx is None else up(self.qidx),
                            gain=[up(g) for g in gains], disc=up(self.disc), ideal=up(self.ideal),
                            ks=up(np.asarray(self.ks, dtype=np.int32)) if self.ks else None)
        return self.dev

    def run(self, lib, rows=None, ldo_pad=3):
        """One call on rows[0] .. rows[0] + rows[1] (default: all) -> [q, 2 nk + 2] with NaN where nothing may be written."""
        import torch
        d = self.device()
        t0, q = rows or (0, self.Q)
        nk = len(self.ks)
        ldo = 2 * nk + 2 + ldo_pad
        out = torch.full(((q + 1) * ldo,), SENT, dtype=torch.int64, device="cuda")
        lib.call("se_ndcg", d["rows"][t0:], self.ldr, q, self.L, d["cls"], self.gallery, d["qcls"][t0:], None if d["qidx"] is None else d["qidx"][t0:],
                 d["gain"][0], d["gain"][1], self.C, d["disc"], len(self.disc), d["ideal"], d["ks"], nk, int(self.want_full),
                 out.view(torch.float64), ldo)
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(q + 1, ldo)
        written = 2 * nk + (2 if self.want_full else 0)
        assert (got[:q, written:] == SENT).all() and (got[q] == SENT).all(), "a slot outside the contract was written"
        res = np.full((q, 2 * nk + 2), np.nan)
        res[:, :written] = got[:q, :written].view(np.float64)
        return res

    def check(self, lib, name, **kw):
        got = self.run(lib, **kw)
        assert np.array_equal(np.isnan(got), np.isnan(self.want)), name
        err = float(np.nanmax(np.abs(got - self.want))) if np.isfinite(self.want).any() else 0.0
        RECORDS.append("%-58s L=%-5d q=%-3d gallery=%-4d C=%-3d nk=%-3d full=%d clsw=%d  %.3e"
                       % (name, self.L, self.Q, self.gallery, self.C, len(self.ks), int(self.want_full), clsw_rule(self.L, self.Q, self.gallery, self.C), err))
        print(RECORDS[-1])
        assert err <= TOL, (name, err)
        return got


def pad4(L):
    """Pitch padding that keeps every row 16-byte aligned (the vector loads are taken)."""
    return (-L) % 4 + 4


def own_places(L):
    c = CH()
    return [0, 1000, c - 1, c, L - 1, "absent", "missing", 3]


IOTA = list(range(1, 11))


# ---------------------------------------------------------------------------------------------- chunk forms

@pytest.mark.parametrize("which", range(6))
def test_list_lengths_around_the_chunk(lib, which):
    """1, 7, CH - 1, CH, CH + 1, 2 CH + 3 entries; the own entry first, inside chunk 0, at CH - 1, at CH, last, absent, missing; the
    whole list and cut-offs 1..10 in order (one of which lies beyond the shortest lists); ldr > list_len."""
    c = CH()
    L = [1, 7, c - 1, c, c + 1, 2 * c + 3][which]
    Case(L, own_places(L), IOTA, True, ldr_pad=pad4(L), seed=1).check(lib, "lengths/iota/full")
    Case(L, own_places(L), [5, 1, 5, 300, 2, L + 10, c, c + 1], True, ldr_pad=pad4(L), seed=2).check(lib, "lengths/unsorted+duplicates+beyond/full")
    Case(L, None, IOTA, True, seed=3).check(lib, "lengths/qidx NULL")


def test_unaligned_rank_base_and_pitch(lib):
    """A base offset by one element and an odd pitch: the vector loads are refused (ranks_vec_ok), the values are the same."""
    L = 2 * CH() + 3
    assert L % 4 == 3
    a = Case(L, own_places(L), IOTA, True, ldr_pad=1, off=0, seed=4)
    b = Case(L, own_places(L), IOTA, True, ldr_pad=1, off=1, seed=4)
    c = Case(L, own_places(L), IOTA, True, ldr_pad=0, off=0, seed=4)
    ga, gb, gc = a.check(lib, "aligned"), b.check(lib, "base + 1 element"), c.check(lib, "odd pitch")
    assert np.array_equal(ga.view(np.int64), gb.view(np.int64)) and np.array_equal(ga.view(np.int64), gc.view(np.int64))


# ---------------------------------------------------------------------------------------------- class-table forms

FORMS = [  # name, L, Q (rows), gallery, C, the form choose_class_table must take
    ("bytes in LDS", 64, 16, 64, 10, 1),
    ("shorts in LDS", 64, 16, 64, 300, 2),
    ("gathered: little work", 64, 4, 64, 10, 0),
    ("gathered: long list, one query", 2 * 2048 + 3, 1, 600, 10, 0),
    ("bytes in LDS, long", 2 * 2048 + 3, 8, 600, 256, 1),
    ("shorts in LDS, long", 2 * 2048 + 3, 8, 600, 257, 2),
]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_class_table_forms(lib, form):
    name, L, Q, gallery, C, clsw = form
    assert clsw_rule(L, Q, gallery, C) == clsw and CH() == 2048
    own = (own_places(L) * 2)[:Q]
    Case(L, own, [3, 1, 40, 2], True, gallery=gallery, C=C, seed=5).check(lib, "form/" + name)
    Case(L, own, [3, 1, 40, 2], False, gallery=gallery, C=C, seed=6, poison=True).check(lib, "form/" + name + "/head only")


# ---------------------------------------------------------------------------------------------- cut-offs

def test_cutoff_lists(lib):
    c = CH()
    L = c + 1
    rng = np.random.RandomState(3)
    Case(L, own_places(L), rng.randint(1, L + 6, size=512).tolist(), True, seed=7).check(lib, "ks/512 random")
    Case(L, own_places(L), list(range(1, 513)), True, seed=8).check(lib, "ks/1..512 in order")
    Case(L, own_places(L), [], True, seed=9).check(lib, "ks/none, whole list only")
    Case(L, own_places(L), [1], False, seed=10, poison=True).check(lib, "ks/[1], head only")
    Case(L, own_places(L), [2 * c, 7], False, seed=11).check(lib, "ks/beyond the list, head only")


def test_head_only_reads_the_head(lib):
    """want_full = 0: only max(ks) + 1 entries of a row are read.  Everything behind them is an index >= gallery whose class, were it
    looked up, carries a gain of 1000 (gathered form) or lies outside the class table (LDS forms): the values come out right."""
    for L, ks in ((2 * CH() + 3, [10, 3, 250]), (300, IOTA), (CH() + 1, [CH() - 1])):
        for gallery, C, rows in ((64, 10, 8), (600, 10, 1)):
            own = own_places(L)[:rows]
            Case(L, own, ks, False, gallery=gallery, C=C, seed=12, poison=True, ldr_pad=3).check(lib, "head only/poisoned tail")


def test_ideal_of_zero_gives_zero(lib):
    case = Case(100, [0, 5, "absent", "missing"], [1, 5, 200], True, seed=13, hot=True)
    got = case.check(lib, "ideal 0")
    assert (got[0] == 0.0).all() and (got[1:] != 0.0).any()


# ---------------------------------------------------------------------------------------------- row independence

def test_rows_do_not_depend_on_their_call(lib):
    """The same rows in one call, twice; split into two calls (1 + 7 rows: the single row falls under the gathered form); in reversed
    row order: the same bits."""
    L = 2 * CH() + 3
    case = Case(L, own_places(L), [5, 1, 5, 300, 2, L + 10], True, gallery=600, seed=14, ldr_pad=pad4(L))
    assert clsw_rule(L, 8, 600, 10) == 1 and clsw_rule(L, 7, 600, 10) == 1 and clsw_rule(L, 1, 600, 10) == 0
    whole = case.check(lib, "independence/one call")
    again = case.run(lib)
    parts = np.concatenate([case.run(lib, rows=(0, 1)), case.run(lib, rows=(1, 7))])
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)  # noqa: E731
    assert np.array_equal(bits(whole), bits(again)) and np.array_equal(bits(whole), bits(parts))
    rev = Case(L, own_places(L), [5, 1, 5, 300, 2, L + 10], True, gallery=600, seed=14, ldr_pad=pad4(L))
    for name in ("rank", "sent_rank", "qcls", "qidx", "want"):
        setattr(rev, name, getattr(rev, name)[::-1].copy())
    assert np.array_equal(bits(rev.check(lib, "independence/reversed rows")), bits(whole[::-1]))


# ---------------------------------------------------------------------------------------------- the tie to se_hierarchical_precision

def _clustered():
    g = np.load(os.path.join(qg.GOLDEN, "retrieval_cluster_cos.npz"))
    feats = np.ascontiguousarray(g["features"], dtype=np.float32)
    leaves = sorted(set(qg.load_fixture()["gallery_labels"].tolist()))
    return feats, [leaves[(7 * i) % len(leaves)] for i in range(len(feats))]


def test_unit_discounts_equal_hierarchical_precision():
    """disc = 1 and the matching ideal: NDCG@k is the P@k of the reference-pinned kernel, on canonical rankings of clustered features
    with the CIFAR taxonomy's tables, for the rows whose query stands first in its own ranking."""
    import torch
    import sehip
    from class_hierarchy import _best_curves
    from evaluate_retrieval import ranking_tiles
    feats, labels = _clustered()
    n = len(feats)
    h = qg.cifar_hierarchy()
    classes = sorted(set(labels))
    cls = np.asarray([classes.index(c) for c in labels], dtype=np.int32)
    wup, lcs = h.similarity_tables_device(classes)
    rank = torch.cat([t.clone() for _, t in ranking_tiles(torch.from_numpy(feats).cuda(), True)])[:, :n].contiguous()
    counts = np.bincount(cls, minlength=len(classes))
    ks = torch.tensor([1, 2, 5, 10, 50, 100], dtype=torch.int32, device="cuda")
    cls_d, qidx = up(cls), torch.arange(n, dtype=torch.int32, device="cuda")
    best = [_best_curves(t, counts, n, rank.device) for t in (wup, lcs)]
    prec = sehip.hierarchical_precision(rank, cls_d, cls_d, qidx, wup, lcs, best[0], best[1], ks)
    ones = torch.ones(n, dtype=torch.float64, device="cuda")
    ideal = torch.stack([sehip.ndcg_ideal(t, counts, ones, ks.tolist(), full=False) for t in (wup, lcs)], dim=2).contiguous()
    got = sehip.ndcg(rank, cls_d, cls_d, qidx, wup, lcs, ones, ideal, ks)
    first = (rank[:, 0] == qidx).cpu().numpy()
    assert first.sum() >= n // 2
    err = (got[:, :12] - prec[:, :12]).abs().cpu().numpy()[first].max()
    RECORDS.append("%-58s n=%d rows=%d  %.3e" % ("disc = 1 against se_hierarchical_precision's P@k", n, int(first.sum()), err))
    assert err <= TOL, err


# ---------------------------------------------------------------------------------------------- end to end

def _close(per_query, want_q, ids):
    worst = 0.0
    for m, vals in want_q.items():
        worst = max(worst, float(np.abs(np.array([per_query[m][i] for i in ids]) - np.array([vals[i] for i in ids])).max()))
    return worst


def test_all_pairs_end_to_end():
    """hierarchical_precision_device(..., ndcg=[1, 10, 0]) against the host ClassHierarchy.ndcg over pairwise_retrieval's rankings;
    the existing columns are what they are without the argument; per_query='table' carries the columns into a bootstrap."""
    import bootstrap
    from evaluate_retrieval import pairwise_retrieval
    feats, labels = _clustered()
    feats, labels = feats[:300], labels[:300]
    h, ks = qg.cifar_hierarchy(), [1, 10, 50]
    base_m, base_q = h.hierarchical_precision_device(feats.copy(), labels, ks, compute_ahp=True, compute_ap=True, normalize=True)
    means, per_query = h.hierarchical_precision_device(feats.copy(), labels, ks, compute_ahp=True, compute_ap=True, normalize=True, ndcg=[1, 10, 0])
    assert list(means)[:len(base_m)] == list(base_m) and all(means[m] == base_m[m] and per_query[m] == base_q[m] for m in base_m)
    retrieved = pairwise_retrieval(feats.copy(), normalize=True, return_generator=False)
    want_m, want_q = h.ndcg(retrieved, labels, [1, 10, 0])
    assert list(means)[len(base_m):] == list(want_m)
    err = _close(per_query, want_q, range(len(feats)))
    RECORDS.append("%-58s n=%d  %.3e" % ("end to end/all pairs, full rankings", len(feats), err))
    assert err <= TOL and all(abs(means[m] - want_m[m]) <= TOL for m in want_m)
    # cut-offs alone: the fused top-L path
    m2, q2 = h.hierarchical_precision_device(feats.copy(), labels, ks, compute_ahp=50, normalize=True, ndcg=[10, 1])
    err = _close(q2, {m: want_q[m] for m in want_q if "@" in m}, range(len(feats)))
    RECORDS.append("%-58s n=%d  %.3e" % ("end to end/all pairs, top-L lists", len(feats), err))
    assert err <= TOL
    # the table form, resampled
    mt, table = h.hierarchical_precision_device(feats.copy(), labels, ks, compute_ahp=True, compute_ap=True, normalize=True, ndcg=[1, 5, 10, 0],
                                                per_query="table")      # 9 + 8 = 17 columns
    cols = [table.columns[m] for m in want_m]
    iv = bootstrap.confidence_intervals(table.values[:, cols].contiguous(), reps=200, level=0.95, seed=1)
    assert np.abs(iv.mean - np.array([means[m] for m in want_m])).max() <= 1e-12
    assert (iv.lo <= iv.mean).all() and (iv.mean <= iv.hi).all() and (iv.hi - iv.lo > 0).any()
    # 17 columns are more than one launch resamples: groups of columns, the same queries drawn in each (what --bootstrap does with --ndcg)
    import sehip
    assert table.values.shape[1] > sehip.BOOTSTRAP_COLS_MAX
    wide = bootstrap.replicate_means(table.values, 50, seed=1)
    assert wide.shape == (50, table.values.shape[1]) and np.array_equal(wide[:, cols], iv.rep_means[:50])


def test_gallery_end_to_end():
    """Held-out queries against a gallery: cut-offs from the top-L lists, everything from the ranked gallery."""
    from test_ndcg_host import _host_rankings
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    h, ks = qg.cifar_hierarchy(), [1, 10]
    retrieved = _host_rankings(g, True)
    want_m, want_q = h.ndcg(retrieved, labels, [1, 10, 0], gallery_ids=kw["gallery_ids"])
    m1, q1 = h.hierarchical_precision_device(queries, labels, ks, compute_ahp=10, normalize=True, ndcg=[1, 10], **kw)
    e1 = _close(q1, {m: want_q[m] for m in want_q if "@" in m}, kw["ids"])
    queries, labels, kw = qg.fixture_arguments(g)
    m2, q2 = h.hierarchical_precision_device(queries, labels, ks, compute_ahp=True, compute_ap=True, normalize=True, rank_gallery=True,
                                             ndcg=[1, 10, 0], **kw)
    e2 = _close(q2, want_q, kw["ids"])
    RECORDS.append("%-58s %.3e" % ("end to end/gallery, top-L lists", e1))
    RECORDS.append("%-58s %.3e" % ("end to end/gallery, rank_gallery", e2))
    assert e1 <= TOL and e2 <= TOL
    with pytest.raises(ValueError, match="--rank_gallery"):
        h.hierarchical_precision_device(queries, labels, ks, compute_ahp=10, normalize=True, ndcg=[0], **kw)


def test_given_rankings_end_to_end():
    """Partial lists completed in all_ids order on the device, then scored: the host statement's values."""
    import test_ranked_host as R
    g, labels, as_dict, as_arrays, all_ids = R.partial_fixture()
    h = R.hierarchy()
    means, per_query = h.hierarchical_precision_ranked(as_arrays, labels, [1, 5], compute_ahp=True, compute_ap=True, all_ids=all_ids, ndcg=[1, 5, 0])
    want_m, want_q = h.ndcg(as_dict, labels, [1, 5, 0], all_ids=all_ids)
    err = _close(per_query, want_q, list(as_dict))
    RECORDS.append("%-58s %.3e" % ("end to end/given partial rankings + all_ids", err))
    assert err <= TOL and all(abs(means[m] - want_m[m]) <= TOL for m in want_m)
