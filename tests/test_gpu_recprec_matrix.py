"""The recall-precision kernels on the device, through every path tests/test_recprec_matrix_host.py holds its case tables to.

Every call goes through the C ABI (``sehip._lib.call``) on buffers the test owns: rankings and slabs on their own pitch and, where the
case says so, on a base 4 or 8 bytes behind 16-byte alignment, ranking padding of indices far outside the gallery, slab padding of NaN,
every output inside a sentinel-filled allocation with a guard behind it.  Every call is made twice (identical bytes), every slot the
contract does not name keeps its sentinel, and everything but AP is held to the host reference bit for bit: positions, counts,
``prec_sum``, ``first_miss``, ``bin_sum``, ``bin_count`` -- the contract fixes the order of the float64 sums, and max is exact.
AP: |ap - exact| <= (R + 2) 2^-53 exact against the Fraction value (R correctly rounded quotients, R - 1 additions of non-negative
terms in any order, one division; R = 0 gives exactly 0.0) -- far below the smallest term 1 / L, so a dropped or doubled term fails it.

``SE_RECPREC_MATRIX_REPORT=<file>`` writes the per-case AP deviations in units of the bound and the bit checks that ran
(profiles/recprec_matrix_gpu.txt): the lines above the file's "recorded by hand" marker.  The marker and what follows it -- the
mutation runs, made off-tree, and the wall times -- are kept as the file has them.
"""
import fractions
import os

import numpy as np
import pytest

import test_recprec_matrix_host as H

pytestmark = pytest.mark.gpu

SENT32 = 0x5EADBEE5                                    # no position, count or sum of these cases
SENT64 = 0x7FF8DEADBEEF0001                            # a NaN no kernel computes
GUARD = 64
PAD_RANK = {H.INT32: 0x7FFFFFF0, H.UINT16: -1}         # pitch padding of the rankings: far outside any gallery (0xFFFF as int16)
U = fractions.Fraction(1, 2 ** 53)
RECORDS = []
REPORT_BY_HAND = "---- recorded by hand"                # the report's lines above this marker are rewritten, the marker and the rest are kept


@pytest.fixture(scope="module")
def lib():
    import sehip
    from sehip import _lib
    sehip.lib()
    return _lib


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    path = os.environ.get("SE_RECPREC_MATRIX_REPORT")
    if path and RECORDS:
        kept = ""                                      # what the file holds from REPORT_BY_HAND on was written by hand and stays
        if os.path.exists(path):
            with open(path) as f:
                old = f.read()
            if REPORT_BY_HAND in old:
                kept = "\n" + old[old.index(REPORT_BY_HAND):]
        with open(path, "w") as f:
            f.write("se_relevant_positions(_r16), se_recall_precision_reduce, se_count_preceding, se_count_to_positions vs the host references of\n"
                    "tests/test_recprec_matrix_host.py.  bits: compared bit for bit with the reference; repeat: the same call twice, identical bytes;\n"
                    "guard: sentinel slots behind (and between) the outputs checked; AP: largest |ap - exact| in units of its bound (R + 2) 2^-53 exact\n\n")
            f.write("\n".join(RECORDS) + "\n" + kept)


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(n, dtype, fill=None):
    """-> (allocation of n + GUARD elements, the same memory as `dtype`): sentinel everywhere, or `fill` [n] in front of the guard."""
    import torch
    sent = SENT32 if dtype in (torch.int32, torch.float32) else SENT64
    raw = torch.full((n + GUARD,), sent, dtype=torch.int32 if sent == SENT32 else torch.int64, device="cuda")
    if fill is not None and n:
        raw[:n] = up(fill).view(raw.dtype)
    return raw, raw.view(dtype)


def guard_ok(raw, n):
    return bool((raw[n:] == (SENT32 if raw.element_size() == 4 else SENT64)).all())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.itemsize == 8 else np.int32)


def pitched(rows, ld, off_bytes, pad, dtype):
    """[n, ld] device view `off_bytes` into a 16-byte aligned buffer filled with `pad`; columns 0 .. rows.shape[1] hold `rows`."""
    import torch
    n, w = rows.shape
    esize = torch.empty((), dtype=dtype).element_size()
    off = off_bytes // esize
    assert off * esize == off_bytes and ld >= w
    buf = torch.full((off + n * ld + 8,), pad, dtype=dtype, device="cuda")
    view = buf[off:off + n * ld].view(n, ld)
    view[:, :w] = up(rows)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() - buf.data_ptr() == off_bytes
    return buf, view


# ------------------------------------------------------------------ positions

@pytest.mark.parametrize("name", [c["name"] for c in H.POS_CASES])
def test_positions(lib, name):
    import torch
    c, d = H.POS_BY_NAME[name], H.pos_data(name)
    if c["Q"] > H.RESIDENT_MAX:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert H.persistent_grids(c["Q"], cus)[-1] < c["Q"]                 # workgroups take several rows
        if c["kind"] == "mixed":                                            # ... of differing chunk counts, at this device's row stride
            H.assert_par_carries(name, cus)
    cls, qcls, hit_off = up(d["cls"]), up(d["qcls"]), up(d["hit_off"])
    qidx = None if d["qidx"] is None else up(d["qidx"])
    total = int(d["hit_off"][-1])
    for rt in c["rt"]:
        rk = d["rk"].astype(np.int32) if rt == H.INT32 else d["rk"].astype(np.uint16).view(np.int16)
        buf, rows = pitched(rk, c["ldr"], c["off_bytes"], PAD_RANK[rt], torch.int32 if rt == H.INT32 else torch.int16)
        assert H.rank_vec_ok(c["ldr"], rt, c["off_bytes"]) == (rows.data_ptr() % min(16, 4 * H.ESIZE[rt]) == 0 and (c["ldr"] * H.ESIZE[rt]) % min(16, 4 * H.ESIZE[rt]) == 0)
        outs = []
        for _ in range(2):
            raw, out = guarded(total, torch.int32)
            lib.call("se_relevant_positions_r16" if rt == H.UINT16 else "se_relevant_positions", rows, c["ldr"], c["Q"], c["L"], cls, c["G"],
                     qcls, qidx, c["num_classes"], hit_off, out)
            torch.cuda.synchronize()
            assert guard_ok(raw, total), ("written behind the last query's R positions", name, rt)
            outs.append(raw.cpu().numpy()[:total])
        assert np.array_equal(outs[0], outs[1]), ("two identical calls differ", name, rt)
        bad = np.flatnonzero(outs[0] != d["want"])
        assert bad.size == 0, (name, rt, [(int(np.searchsorted(d["hit_off"], b, side="right")) - 1, int(b), int(outs[0][b]), int(d["want"][b])) for b in bad[:5]])
    RECORDS.append("positions %-20s CLSW %d  Q %4d  L %4d  %s  bits %d positions x %d types, repeat %d, guard %d"
                   % (name, H.pos_case_clsw(c), c["Q"], c["L"], "  ".join("%s vec_ok %d" % (rt, H.pos_case_vec_ok(c, rt)) for rt in c["rt"]),
                      total, len(c["rt"]), len(c["rt"]), 2 * len(c["rt"])))


# ------------------------------------------------------------------ reduce

class Reduce:
    """The accumulators of one problem on the device, each inside its guarded allocation, pre-filled with reduce_prior."""

    def __init__(self, name, bins, lib):
        import torch
        self.c, self.d, self.bins, self.lib = H.REDUCE_BY_NAME[name], H.reduce_data(name), bins, lib
        self.C, self.n, self.Q = len(self.c["R"]), int(self.d["class_off"][-1]), len(self.d["qcls"])
        ps, fm, bs, bc = H.reduce_prior(name, bins)
        self.class_off = up(self.d["class_off"])
        self.ap_raw, self.ap = guarded(self.Q, torch.float64)
        self.ps_raw, self.ps = guarded(self.n, torch.float64, ps)
        self.fm_raw, self.fm = guarded(self.C, torch.int64, fm)
        nb = self.C * (bins + 1) if bins else 0
        self.bs_raw, self.bs = guarded(nb, torch.float64, bs.ravel() if bins else None)
        self.bc_raw, self.bc = guarded(nb, torch.int64, bc.ravel() if bins else None)
        self.nb = nb

    def run(self, rows):
        """The whole problem in tiles of `rows` queries (0: one tile) -> host copies (ap, prec_sum, first_miss, bin_sum, bin_count)."""
        import torch
        for q0, hit_pos, hit_off, order, class_start in H.reduce_tiles(self.c["name"], rows):
            q = len(order)
            hp_raw, hp = guarded(len(hit_pos), torch.int32, hit_pos)
            self.lib.call("se_recall_precision_reduce", hp, up(hit_off), q, up(order), up(class_start), self.C, self.class_off, self.n,
                          self.bins, self.ap[q0:], self.ps, self.fm, self.bs if self.bins else None, self.bc if self.bins else None)
        torch.cuda.synchronize()
        for raw, n, what in ((self.ap_raw, self.Q, "ap"), (self.ps_raw, self.n, "prec_sum"), (self.fm_raw, self.C, "first_miss"),
                             (self.bs_raw, self.nb, "bin_sum"), (self.bc_raw, self.nb, "bin_count")):
            assert guard_ok(raw, n), ("written behind " + what, self.c["name"], self.bins, rows)
        return tuple(r.cpu().numpy()[:n] for r, n in ((self.ap_raw, self.Q), (self.ps_raw, self.n), (self.fm_raw, self.C),
                                                     (self.bs_raw, self.nb), (self.bc_raw, self.nb)))


@pytest.mark.parametrize("name", [c["name"] for c in H.REDUCE_CASES])
def test_reduce(lib, name):
    c, d = H.REDUCE_BY_NAME[name], H.reduce_data(name)
    for bins in c["B"]:
        exact, ps, fm, bs, bc = H.reduce_expected(name, bins)
        want = (None, ps, fm, bs.ravel() if bins else np.zeros(0), bc.ravel() if bins else np.zeros(0, dtype=np.int64))
        first, n_bits, worst = None, 0, fractions.Fraction(0)
        for rows in c["tilings"] + c["tilings"][:1]:                      # the first tiling twice: identical bytes
            got = Reduce(name, bins, lib).run(rows)
            tag = (name, bins, rows)
            for k, what in ((1, "prec_sum"), (2, "first_miss"), (3, "bin_sum"), (4, "bin_count")):
                bad = np.flatnonzero(got[k] != bits(want[k]).astype(np.int64))
                assert bad.size == 0, (what, tag, bad[:5].tolist(), got[k][bad[:5]].view(np.float64 if k in (1, 3) else np.int64).tolist(),
                                       np.asarray(want[k])[bad[:5]].tolist())
                n_bits += got[k].size
            ap = got[0].view(np.float64)
            for i, (a, e) in enumerate(zip(ap.tolist(), exact)):
                R = len(d["pos"][i])
                if R == 0:
                    assert got[0][i] == 0, ("AP of a query without relevant items is +0.0", tag, i, a)
                    continue
                dev, bound = abs(fractions.Fraction(a) - e), (R + 2) * U * e
                assert dev <= bound, ("AP", tag, i, R, a, float(e), float(dev / bound))
                worst = max(worst, dev / bound)
            if first is None:
                first = got
            else:
                assert all(np.array_equal(x, y) for x, y in zip(first, got)), ("the tiling (or a repeated call) changed a bit", tag)
        line = "reduce    %-12s C %2d  Q %5d  max R %7d  bins %7d  tilings %s + repeat  AP worst %.3f of bound  bits %d values, guard 5 buffers" \
            % (name, len(c["R"]), len(d["qcls"]), max(c["R"]), bins, "/".join(str(r or "all") for r in c["tilings"]), float(worst), n_bits)
        print(line)
        RECORDS.append(line)


# ------------------------------------------------------------------ counting

def count_call(lib, pd, ldp, off_bytes, col_offset, d, max_rel, cnt, qidx="given"):
    import torch
    buf, rows = pitched(pd, ldp, off_bytes, float("nan"), torch.float32)
    lib.call("se_count_preceding", rows, ldp, pd.shape[0], pd.shape[1], col_offset, d["dev"][0], d["dev"][1], d["dev"][2],
             d["dev"][3] if qidx == "given" else None, max_rel, cnt)
    torch.cuda.synchronize()


def on_device(d):
    d = dict(d)
    d["dev"] = (up(d["hit_off"]), up(d["rel_d"]), up(d["rel_i"]), up(d["qidx"]))
    return d


@pytest.mark.parametrize("n_cols", H.COUNT_COLS)
def test_count_one_call(lib, n_cols):
    import torch
    d = on_device(H.count_case(n_cols))
    total = int(d["hit_off"][-1])
    outs = []
    for _ in range(2):
        raw, cnt = guarded(total, torch.int32, d["prior"])
        count_call(lib, d["pd"], (n_cols + 3) // 4 * 4, 0, 0, d, max(H.COUNT_R), cnt)
        assert guard_ok(raw, total)
        outs.append(raw.cpu().numpy()[:total])
    assert np.array_equal(outs[0], outs[1])
    bad = np.flatnonzero(outs[0] != d["want"])
    assert bad.size == 0, (n_cols, bad[:5].tolist(), outs[0][bad[:5]].tolist(), d["want"][bad[:5]].tolist())
    RECORDS.append("count     n_cols %5d  chunks %d  cut vector step in chunks %s  bits %d counts on a non-zero prior, repeat 1, guard 2"
                   % (n_cols, H.count_geometry(len(H.COUNT_R), n_cols, max(H.COUNT_R))[1], H.cut_vector_steps(n_cols, H.RC_CHUNK), total))


def test_count_slabs_at_odd_columns(lib):
    """The 32,773-column gallery as four slabs cut at odd columns, each on its own pitch and base, counted in two orders."""
    import torch
    d = on_device(H.count_case(H.COUNT_N))
    total = int(d["hit_off"][-1])
    slabs = list(zip(zip(H.COUNT_SLABS, H.COUNT_SLABS[1:]), H.SLAB_LAYOUTS))
    for order in (slabs, slabs[::-1]):
        raw, cnt = guarded(total, torch.int32, d["prior"])
        for (a, b), (pad, off) in order:
            count_call(lib, d["pd"][:, a:b], (b - a + 3) // 4 * 4 + pad, off, a, d, 0, cnt)
        assert guard_ok(raw, total)
        got = raw.cpu().numpy()[:total]
        bad = np.flatnonzero(got != d["want"])
        assert bad.size == 0, (bad[:5].tolist(), got[bad[:5]].tolist(), d["want"][bad[:5]].tolist())
    RECORDS.append("count     slabs %s of 32773 columns, forwards and backwards  bits %d counts x 2, guard 2" % (list(H.COUNT_SLABS), total))


@pytest.mark.parametrize("R", H.KEY_RS)
def test_count_key_lists(lib, R):
    import torch
    d = on_device(H.key_case(R))
    total = int(d["hit_off"][-1])
    for max_rel in H.key_max_rels(R):
        outs = []
        for _ in range(2):
            raw, cnt = guarded(total, torch.int32, d["prior"])
            count_call(lib, d["pd"], H.KEY_COLS + 1, 0, 0, d, max_rel, cnt)
            assert guard_ok(raw, total)
            outs.append(raw.cpu().numpy()[:total])
        assert np.array_equal(outs[0], outs[1])
        bad = np.flatnonzero(outs[0] != d["want"])
        assert bad.size == 0, (R, max_rel, bad[:5].tolist(), outs[0][bad[:5]].tolist(), d["want"][bad[:5]].tolist())
    RECORDS.append("count     keys %4d  max_rel %s -> LDS keys %s  bits %d counts x 4, repeat 4, guard 8"
                   % (R, list(H.key_max_rels(R)), [H.count_geometry(3, H.KEY_COLS, m)[2] for m in H.key_max_rels(R)], total))


@pytest.mark.parametrize("big", [False, True])
def test_scan(lib, big):
    import torch
    d = H.scan_case(big)
    q, total = len(d["hit_off"]) - 1, int(d["hit_off"][-1])
    hit_off = up(d["hit_off"])
    outs = []
    for in_place in (False, True, False):
        craw, cnt = guarded(total, torch.int32, d["cnt"])
        raw, out = (craw, cnt) if in_place else guarded(total, torch.int32)
        lib.call("se_count_to_positions", cnt, hit_off, q, out)
        torch.cuda.synchronize()
        assert guard_ok(raw, total) and guard_ok(craw, total)
        assert in_place or np.array_equal(craw.cpu().numpy()[:total], d["cnt"]), "the out-of-place scan changed its input"
        outs.append(raw.cpu().numpy()[:total])
        assert np.array_equal(outs[-1], d["want"]), (big, in_place, np.flatnonzero(outs[-1] != d["want"])[:5].tolist())
    assert np.array_equal(outs[0], outs[2])
    RECORDS.append("scan      Q %5d  R %s  bits %d positions out of place, in place, repeat 1, guard 5"
                   % (q, sorted(set(np.diff(d["hit_off"]).tolist())), total))
