"""The hierarchical-precision kernels on the device, through every path tests/test_hprec_matrix_host.py holds its case table to.

Every case calls the C ABI directly (``sehip._lib.call``) with buffers the test owns: rankings on their own pitch and base offset
inside a buffer whose padding holds indices outside the gallery, ``out`` on a pitch of its own inside a sentinel-filled allocation
with a guard row behind the last query, curves built by ``se_hprec_reciprocal_curves`` for the case's ``rcp_len`` (which may exceed
the lists).  Per call: every produced column within 1e-10 of ``_hprec_standin`` (the project's bound for this kernel, hprec.hip:28-29),
every other slot still the sentinel; and bit equality wherever the code gives no reason for a difference -- a repeated call, the
class-ordered against the static visit, a tile of five rows alone (gathered classes, singles) against the same rows inside the full
call (class table, pairs), uint16 against int32 ranks on every row whose chunks take the same forms in both types.

``SE_HPREC_MATRIX_REPORT=<file>`` writes the table of deviations and of the bit checks that ran (profiles/hprec_matrix_gpu.txt).
"""
import os

import numpy as np
import pytest

import test_hprec_matrix_host as H

pytestmark = pytest.mark.gpu

TOL = 1e-10                                            # hprec.hip:28-29; every hprec test of this suite uses it
SENT = 0x7FF8DEADBEEF0001                              # a NaN no kernel computes
PAD_RANK = {H.INT32: 0x7FFFFFF0, H.UINT16: -1}         # pitch padding of the rankings: far outside any gallery (0xFFFF as int16)
TILE = 5                                               # rows of the tile call: fewer than 8 queries are gathered and drawn one by one
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
    path = os.environ.get("SE_HPREC_MATRIX_REPORT")
    if path and RECORDS:
        with open(path, "w") as f:
            f.write("se_hierarchical_precision(_r16) vs _hprec_standin (float64), bound %g; bit checks: repeat = the same call twice, "
                    "order = class-ordered vs static visit,\ntile = %d rows alone vs inside the full call, rt = uint16 vs int32 ranks "
                    "(bits on every row whose chunks take the same forms in both types, else the bound only)\n\n" % (TOL, TILE))
            f.write("\n".join(RECORDS) + "\n")


def sentinel(n):
    import torch
    return torch.full((n,), SENT, dtype=torch.int64, device="cuda")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


class Device:
    """One case on the device: everything but the rankings' element type."""

    def __init__(self, c, lib):
        import torch
        d = H.case_data(c["name"])
        self.c, self.d, self.lib = c, d, lib
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.cls, self.qcls = up(d["cls"]), up(d["qcls"])
        self.qidx = None if d["qidx"] is None else up(d["qidx"])
        self.tab_w, self.tab_l = up(d["tab_w"]), up(d["tab_l"])
        self.ks = up(d["ks"]) if len(d["ks"]) else None
        best_w, best_l = up(d["best_w"]), up(d["best_l"])
        ldb, rcp_len = best_w.stride(0), c["rcp_len"]
        assert ldb >= rcp_len and best_l.stride(0) == ldb
        lp = int(lib.call("se_hprec_curve_len", rcp_len))
        assert lp == H.curve_len(rcp_len)
        self.rcp = torch.empty((c["C"] * 2 * lp * 2,), dtype=torch.float64, device="cuda")
        lib.call("se_hprec_reciprocal_curves", best_w, best_l, ldb, c["C"], rcp_len, self.rcp)
        self.ranks = {}

    def rank_rows(self, rt):
        """[Q, ldr] view `off` elements into a 16-byte aligned buffer; columns L .. ldr hold indices outside the gallery."""
        import torch
        if rt not in self.ranks:
            c = self.c
            dt = torch.int32 if rt == H.INT32 else torch.int16
            buf = torch.full((c["off"] + c["Q"] * c["ldr"],), PAD_RANK[rt], dtype=dt, device="cuda")
            rows = buf[c["off"]:].view(c["Q"], c["ldr"])
            rk = self.d["rk"] if rt == H.INT32 else self.d["rk"].astype(np.uint16).view(np.int16)
            rows[:, :c["L"]] = torch.from_numpy(np.ascontiguousarray(rk)).cuda()
            assert buf.data_ptr() % 16 == 0 and (rows.data_ptr() - buf.data_ptr()) == c["off"] * H.ESIZE[rt]
            self.ranks[rt] = (buf, rows)
        return self.ranks[rt][1]

    def run(self, rt, ordered, ahp_len, want_ap, rows=None):
        """One call on queries rows[0] .. rows[0] + rows[1] (default: all).  Checks every slot the call must leave alone; -> [q, 2 nk + 3]."""
        import torch
        c, lib = self.c, self.lib
        t0, q = rows or (0, c["Q"])
        nk = len(c["ks"])
        ldo = 2 * nk + 3 + c["ldo_pad"]
        out = sentinel((q + 1) * ldo)
        ws = None
        if ordered:
            nbytes = int(lib.call("se_hprec_order_workspace_bytes", q))
            assert nbytes == 4 * (H.HP_WS_HEAD + 4 * q)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
            assert ws.data_ptr() % 16 == 0
        rk = self.rank_rows(rt)
        lib.call("se_hierarchical_precision_r16" if rt == H.UINT16 else "se_hierarchical_precision",
                 rk[t0:], c["ldr"], q, c["L"], self.cls, c["gallery"], self.qcls[t0:], None if self.qidx is None else self.qidx[t0:],
                 self.tab_w, self.tab_l, c["C"], self.rcp, c["rcp_len"], self.ks, nk, ahp_len, want_ap, out.view(torch.float64), ldo, ws)
        torch.cuda.synchronize()
        raw = out.cpu().numpy().reshape(q + 1, ldo)
        tag = (c["name"], rt, ordered, ahp_len, want_ap, rows)
        assert (raw[q] == SENT).all(), ("guard row written", tag)
        assert (raw[:q, 2 * nk + 3:] == SENT).all(), ("ldo padding written", tag)
        assert (raw[:q, :2 * nk] != SENT).all(), ("a cut-off column was left out", tag)
        assert ((raw[:q, 2 * nk:2 * nk + 2] == SENT) == (ahp_len < 0)).all(), ("AHP columns", tag)
        assert ((raw[:q, 2 * nk + 2] == SENT) == (not want_ap)).all(), ("AP column", tag)
        return raw[:q, :2 * nk + 3].view(np.float64)


def produced(nk, ahp_len, want_ap):
    return list(range(2 * nk)) + ([2 * nk, 2 * nk + 1] if ahp_len >= 0 else []) + ([2 * nk + 2] if want_ap else [])


@pytest.mark.parametrize("name", [c["name"] for c in H.CASES])
def test_case_vs_oracle(lib, name):
    c = H.CASE_BY_NAME[name]
    dev = Device(c, lib)
    nk = len(c["ks"])
    w = H.case_clsw(c)
    first = c["class_order"] != "off"
    t0 = max(0, c["Q"] // 2 - 2)
    tile = (t0, TILE) if c["Q"] > TILE else None
    if tile and w != 0:
        assert H.clsw(c["L"], TILE, c["gallery"], c["C"], nk)[0] == 0          # the tile gathers what the full call reads from its table
    got, worst, checks = {}, {}, {"repeat": 0, "order": 0, "tile": 0}
    for rt in c["rt"]:
        worst[rt] = 0.0
        for ahp_len, want_ap in c["calls"]:
            a = dev.run(rt, first, ahp_len, want_ap)
            cols = produced(nk, ahp_len, want_ap)
            want = H.case_oracle(name, ahp_len, want_ap)
            err = np.abs(a[:, cols] - want[:, cols])
            worst[rt] = max(worst[rt], float(np.nanmax(err))) if err.size else worst[rt]
            print("%s %s ahp_len=%d ap=%d: largest deviation %.3e" % (name, rt, ahp_len, want_ap, float(np.nanmax(err)) if err.size else 0.0))
            assert (err <= TOL).all(), (name, rt, ahp_len, want_ap, float(np.nanmax(err)), np.argwhere(~(err <= TOL))[:5].tolist())
            got[(rt, ahp_len, want_ap)] = a
            tag = (name, rt, ahp_len, want_ap)
            assert np.array_equal(bits(dev.run(rt, first, ahp_len, want_ap)), bits(a)), ("two identical calls differ", tag)
            checks["repeat"] += 1
            if c["class_order"] == "both":
                # the chunk forms depend on the list, the cut-offs and the query's position only: not on NQ or the visit
                assert np.array_equal(bits(dev.run(rt, not first, ahp_len, want_ap)), bits(a)), ("class-ordered vs static visit", tag)
                checks["order"] += 1
            if tile:
                alone = dev.run(rt, first, ahp_len, want_ap, rows=tile)
                assert np.array_equal(bits(alone), bits(a[t0:t0 + TILE])), ("tile alone vs inside the full call", tag)
                checks["tile"] += 1
    rt_check = "-"
    if set(c["rt"]) == set(H.BOTH):
        # uint16 and int32 ranks give the same bits where both take the same loads.  Where vec_ok differs (L = 6148 on its own pitch,
        # a base 8 bytes into the buffer) one type runs FAST chunks and the other TAIL / general ones: the sums are associated
        # differently, and only the bound above holds.  That is the design, not a defect to "fix" here.
        # So: every row whose chunks take the same forms in both types (all rows where vec_ok agrees; elsewhere the absent queries,
        # the calls without AHP, the one-chunk lists) is held to the bits, the others to the bound.
        same = H.case_vec_ok(c, H.INT32) == H.case_vec_ok(c, H.UINT16)
        f32, f16 = H.case_forms(c, H.INT32), H.case_forms(c, H.UINT16)
        n_bits = n_bound = 0
        for call in c["calls"]:
            rows = np.array([f32[(u, call)] == f16[(u, call)] for u in range(c["Q"])])
            assert rows.all() or not same
            a16, a32 = got[(H.UINT16,) + call], got[(H.INT32,) + call]
            assert np.array_equal(bits(a16[rows]), bits(a32[rows])), ("uint16 vs int32", name, call, np.flatnonzero((bits(a16) != bits(a32)).any(axis=1) & rows)[:5].tolist())
            n_bits, n_bound = n_bits + int(rows.sum()), n_bound + int((~rows).sum())
        rt_check = "bits %d rows" % n_bits + (", bound %d rows" % n_bound if n_bound else "")
    line = "%-16s CLSW %d  Q %4d  L %4d  calls %2d  " % (name, w, c["Q"], c["L"], len(c["calls"]))
    line += "  ".join("%s vec_ok %d max|dev| %.3e" % (rt, H.case_vec_ok(c, rt), worst[rt]) for rt in c["rt"])
    line += "  repeat %d order %d tile %d rt %s" % (checks["repeat"], checks["order"], checks["tile"], rt_check)
    RECORDS.append(line)
    print(line)


@pytest.mark.parametrize("C,n", H.RCP_CASES)
def test_reciprocal_curves_bitwise(lib, C, n):
    """se_hprec_reciprocal_curves alone: 1 / (best - 1) and 1 / best at hp_slot(i), bit for bit (float64 division is IEEE on both
    sides; best[0] = 1 gives +inf on both), +0 in the slots behind the curve, nothing outside the table; NaN in the pitch padding of
    the inputs."""
    import torch
    rng = np.random.default_rng(n)
    ldb = n + 3
    best = []
    for _ in range(2):
        b = np.full((C, ldb), np.nan)
        b[:, :n] = 1.0 + np.concatenate([np.zeros((C, 1)), np.cumsum(rng.random((C, n - 1)) * 0.8 + 0.1, axis=1)], axis=1)
        best.append(b)
    lp = int(lib.call("se_hprec_curve_len", n))
    assert lp == H.curve_len(n)
    total = C * 2 * lp * 2
    out = sentinel(total + 64)
    bw, bl = (torch.from_numpy(b).cuda() for b in best)
    lib.call("se_hprec_reciprocal_curves", bw, bl, ldb, C, n, out.view(torch.float64))
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[total:] == SENT).all()
    got = raw[:total].view(np.float64).reshape(C, 2, lp, 2)
    want = np.zeros((C, 2, lp, 2))
    slot = H.hp_slot(np.arange(n))
    assert len(set(slot.tolist())) == n and slot.max() < lp
    with np.errstate(divide="ignore"):
        for t, b in enumerate(best):
            want[:, 0, slot, t] = 1.0 / (b[:, :n] - 1.0)
            want[:, 1, slot, t] = 1.0 / b[:, :n]
    assert np.isposinf(want[:, 0, 0, :]).all() and np.isfinite(want[:, 1]).all()
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5].tolist()


def test_refusals_before_any_launch(lib):
    """Arguments se_hierarchical_precision must refuse, with the code it promises, leaving `out` alone."""
    import torch
    from sehip import SehipError
    L = G = Q = 8
    C, nk = 3, 2
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32, device="cuda")  # noqa: E731
    rk = torch.arange(L, dtype=torch.int32, device="cuda").repeat(Q, 1)
    cls, qcls = torch.zeros(G, dtype=torch.int32, device="cuda"), torch.zeros(Q, dtype=torch.int32, device="cuda")
    tab = torch.ones((C, C), dtype=torch.float64, device="cuda")
    best = torch.arange(1, L + 1, dtype=torch.float64, device="cuda").repeat(C, 1)
    rcp = torch.empty((C * 2 * H.curve_len(L) * 2,), dtype=torch.float64, device="cuda")
    lib.call("se_hprec_reciprocal_curves", best, best, L, C, L, rcp)
    ks = i32(1, 2)
    out = sentinel((Q + 1) * (2 * 513 + 3))
    o = out.view(torch.float64)
    ws = torch.empty((4 * (H.HP_WS_HEAD + 4 * Q) + 16,), dtype=torch.uint8, device="cuda")
    name = "se_hierarchical_precision"

    def args(**kw):
        a = dict(rank=rk, ldr=L, q=Q, L=L, cls=cls, gallery=G, qcls=qcls, qidx=None, wup=tab, lcs=tab, C=C, rcp=rcp, rcp_len=L, ks=ks, nk=nk,
                 ahp_len=0, want_ap=1, out=o, ldo=2 * nk + 3, ws=None)
        a.update(kw)
        return tuple(a.values())

    def refused(code, fn=name, **kw):
        with pytest.raises(SehipError, match=r"\(code %d\)" % code):
            lib.call(fn, *args(**kw))
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), kw

    invalid, unsupported = lib.DEFINES["SE_ERR_INVALID"], lib.DEFINES["SE_ERR_UNSUPPORTED"]
    refused(invalid, rcp_len=L - 1)
    refused(invalid, ks=torch.arange(1, 514, dtype=torch.int32, device="cuda"), nk=513, ldo=2 * 513 + 3)
    refused(invalid, ldo=2 * nk + 2)
    assert ws.data_ptr() % 16 == 0
    refused(invalid, ws=ws[4:])
    refused(invalid, fn="se_hierarchical_precision_r16", rank=rk.to(torch.int16), gallery=65537,
            cls=torch.zeros(65537, dtype=torch.int32, device="cuda"))
    # 10,300 classes: 164,800 bytes of similarity rows, over the 160 KB of LDS.  Refused before anything reads a table, so the tables
    # of this call are the small ones (and no workspace: not even the order kernel would run)
    assert H.clsw(L, Q, G, 10300, nk) is None
    refused(unsupported, C=10300)
    # and the call the refusals were variations of is accepted
    lib.call(name, *args(ws=ws))
    torch.cuda.synchronize()
    assert not bool((out[:Q * (2 * nk + 3)] == SENT).any()) and bool((out[Q * (2 * nk + 3):] == SENT).all())
