"""The fused distance + top-k family (csrc/topk.hip, csrc/prefilter.hip, the two fused epilogues of csrc/pdist_mfma.hip) through every
kernel instantiation and data-dependent path its host code can choose, at the smallest shapes that reach them.

``se_topk_rows`` takes the exact radix select, or -- from 8,192 columns -- the sample select, which sorts 512 x {1, 2, 4, 8, 16}
candidates per row (chosen by the row's candidate count) and hands rows outside [k, 8,192] candidates to the radix select.
``se_retrieve_topk`` takes the distance slab (small galleries), the fp32 fused passes (``pdist_kernel<METRIC, MULTI_KB, SYM, VEC, EPI>``:
8 ``EPI_GROUPMIN`` and 16 ``EPI_FILTER`` instantiations, ``topk_lists_kernel`` with the same five sort widths) or the pre-filter
(``pf_tile_kernel`` x 4, ``pf_big_kernel`` x 2, six ``pf_refine_kernel<METRIC, VEC, LONGROWS>`` builds sorting 64 x {1 .. 16} exact
distances, candidate sub-lists with a shared spill region), and behind both fused forms ``topk_fallback_kernel`` in a staged and an
unstaged form.

The first part of this file restates those choices in Python, each next to the name of the C++ function it mirrors.  The CPU tests
hold the case tables to every instantiation, sort width, count edge, ``last_steps`` value and product threshold: a row that leaves a
table, or drifts to another path, fails there and not silently on the device.  A case's claimed candidate count, refinement count
``m`` and spill count are DERIVED on the host from the case's own data (``sample_outcome``, ``cluster_outcome``), never stated.

Deterministic counts: the gallery of a counting case holds clusters of exact copies of orthonormal centres, the other rows are
orthogonal to every centre, every query sits next to one centre, and ``SE_TOPK_J=1`` makes the threshold the smallest sampled
distance.  A query's candidates are then exactly the copies of its centre (the copies tie; the index breaks the tie), so candidate
count = m = the cluster's size, and the sub-list of every candidate follows from the restated geometry.  A two-level cluster puts
copies of a companion of the centre under the sample and the centre's own copies behind the last sampled row: the threshold admits
both, the k-th distance only the latter (candidate count > m: lists of more than 1,024 entries that are accepted).

Each GPU case calls the C ABI with buffers the test owns: operands inside NaN-filled buffers (layouts of tests/test_gpu_pdist.py),
outputs and the workspace inside sentinel-filled allocations, the workspace exactly ``se_retrieve_topk_workspace_bytes`` long -- which
must be the restated size.  ``out_d`` / ``out_i`` must equal ``canon_topk_rows(canon_pdist(...))`` on every row; on the pre-filter
path the counters of ``se_phase_timing_read`` must equal the derived ones.  Switches of the tuning library run in child processes, one
per group of cases, one after another.

Recorded while restating (nothing here is changed or removed by this file):
  * ``SE_TOPK_FUSED=1`` takes the fused passes from 256 gallery rows (``fused_plan_compute``: n >= 256 and S = n / 2 rounded down
    to 128 >= 128), so the fused cases start at n = 256; smaller galleries take the slab whatever the switch says.
  * ``topk_lists_kernel`` sorts more than 4,096 entries only for a list capacity above 4,096, and the capacity is at most 8,192: the
    8,192 / 8,193 edge needs a gallery of more than 8,192 rows (the only fused cases above 1,000 rows besides the refinement edges).
  * In the product library n = 16,384 with k = 513 does NOT take the fp32 fused passes: ``fused_plan_compute`` finds k / n too large for
    its 2,048-row sample (j > G / 2) and the call takes the slab.  ``PRODUCT_THRESHOLDS`` pins what the plan really decides.
  * ``pf_refine_kernel<*, false, true>`` does not exist: LONGROWS implies 16-byte rows.
"""
import collections
import functools
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

TESTS_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_DIR = os.path.dirname(TESTS_DIR)
PKG_DIR = os.path.join(ROOT_DIR, "semantic-embeddings_amd")
if __name__ == "__main__":
    sys.path[:0] = [PKG_DIR, ROOT_DIR, TESTS_DIR]

from oracle import retrieval_oracle as ro  # noqa: E402
import test_gpu_pdist as PD  # noqa: E402         (place, layout_pitch, layout_aligned and the four layouts)
import test_gpu_rank_matrix as RM  # noqa: E402   (canon_key)
import test_gpu_topk as TK  # noqa: E402          (want_topk, PROBE)

F32 = np.float32
COS, EUC = ro.METRIC_COSINE, ro.METRIC_EUCLID
CONTIG, PADDED, COL1, ROWS = PD.CONTIG, PD.PADDED, PD.COL1, PD.ROWS

# ------------------------------------------------------------------ constants of topk.hip / prefilter.hip / pdist_mfma.hip

TK_THREADS, TK_SAMPLES, TK_CAP, TOPK_MAX = 512, 2048, 8192, 2048
FUSED_GROUP, FB_GRID, FUSED_P_FAIL = 16, 256, 1e-6
RF_MAX, PF_K_MAX, RF_STAGE_M, RF_STAGE_D = 1024, 512, 384, 256
PD_TILE, PD_MAX_LD = 128, 1 << 23
PF_BM, PF_BK, PB_BM, PF_WGS_PER_CU = 128, 128, 256, 2
CUS = 256                                             # num_cus() of the MI355X
SORT_WIDTHS = (1, 2, 4, 8, 16)
SLAB, FP32, PREF = "slab", "fp32", "prefilter"


def align256(v):
    return (v + 255) // 256 * 256


def env_int(env, name):
    """atoi of a tuning switch, None when it is not set."""
    return int(env[name]) if name in env else None


# ------------------------------------------------------------------ se_topk_rows, restated

def pivot_rank(n, k):
    """se_topk_rows: -> (sample select taken, pivot rank r)."""
    m = float(k) * TK_SAMPLES / float(n)
    rr = (2.0 + math.sqrt(4.0 + m)) * (2.0 + math.sqrt(4.0 + m)) + 4.0
    r = int(math.ceil(rr))
    upper = (rr + 4.0 * math.sqrt(rr) + 8.0) / TK_SAMPLES * float(n)
    return (n >= 4 * TK_SAMPLES and r < TK_SAMPLES and upper <= float(TK_CAP)), r


def sample_positions(n):
    """topk_sample_kernel: column of sample tid * 4 + r, (tid * 4 + r) * N / 2048 in integer arithmetic."""
    return (np.arange(TK_SAMPLES, dtype=np.int64) * n) // TK_SAMPLES


def sort_width(total, unit):
    """with_width behind sort_candidates<TK_THREADS> (unit 512) and sort_candidates<WAVE> (unit 64): values per thread / lane."""
    return next(w for w in SORT_WIDTHS if total <= w * unit or w == 16)


def sample_outcome(row, k):
    """topk_sample_kernel on one row -> (candidate count, sort width | "redo"); (None, "radix") when se_topk_rows skips the kernel."""
    n = len(row)
    sample, r = pivot_rank(n, k)
    if not sample:
        return None, "radix"
    keys = RM.canon_key(row)
    pivot = np.sort(keys[sample_positions(n)])[r]
    total = int((keys <= pivot).sum())
    if total < k or total > TK_CAP:
        return total, "redo"
    return total, sort_width(total, TK_THREADS)


# ------------------------------------------------------------------ retrieve_topk_plan and what it calls, restated

Plan = collections.namedtuple("Plan", "S step G j cap")
Geom = collections.namedtuple("Geom", "big gi gj parts tpp")
Layout = collections.namedtuple("Layout", "qt parts cap nsub spill geom kp total")
Retrieve = collections.namedtuple("Retrieve", "path plan layout need")


def binom_sf(G, p, j):
    """binom_sf: P(Binomial(G, p) >= j)."""
    if j <= 0:
        return 1.0
    if j > G:
        return 0.0
    if p <= 0.0:
        return 0.0
    if p >= 1.0:
        return 1.0
    lp, lq = math.log(p), math.log1p(-p)
    s = 0.0
    for x in range(j, G + 1):
        s += math.exp(math.lgamma(G + 1.0) - math.lgamma(x + 1.0) - math.lgamma(G - x + 1.0) + x * lp + (G - x) * lq)
    return s if s < 1.0 else 1.0


@functools.lru_cache(maxsize=None)
def _fused_plan(n, ldg, k, force, env_j, env_cap):
    if force == 0:
        return None
    if n < (256 if force == 1 else 16384):
        return None
    S = 4096 if n >= 65536 else 2048
    if S > n // 2:
        S = n // 2 // 128 * 128
    if S < 128:
        return None
    step = n // S
    if step * ldg >= PD_MAX_LD:
        step = (PD_MAX_LD - 1) // ldg
    if step < 1:
        return None
    G = S // FUSED_GROUP
    if G > 256:
        return None
    q0 = float(k) / float(n)
    pi0 = 1.0 - math.pow(1.0 - q0, float(FUSED_GROUP))
    j = 1
    while j <= G and binom_sf(G, pi0, j) > FUSED_P_FAIL:
        j += 1
    forced = force == 1
    if j > G // 2:
        if not forced:
            return None
        if j > G:
            j = G
    q1 = q0
    for _ in range(400):
        if not q1 < 1.0:
            break
        pi1 = 1.0 - math.pow(1.0 - q1, float(FUSED_GROUP))
        if 1.0 - binom_sf(G, pi1, j) <= FUSED_P_FAIL:
            break
        q1 *= 1.05
    if q1 > 0.25 and not forced:
        return None
    if q1 > 1.0:
        q1 = 1.0
    capd = q1 * float(n) + 6.0 * math.sqrt(q1 * float(n)) + 64.0
    if capd < 2.0 * k:
        capd = 2.0 * k
    if capd > float(n):
        capd = float(n)
    cap = int((capd + 255.0) / 256.0) * 256
    if forced and cap > TK_CAP:
        cap = TK_CAP
    if env_j is not None:
        j = env_j
    if env_cap is not None:
        cap = env_cap
    if cap > TK_CAP or j < 1 or j > G:
        return None
    return Plan(S, step, G, j, cap)


def fused_plan_compute(n, ldg, k, env):
    """fused_plan_compute (SE_TOPK_FUSED, SE_TOPK_J, SE_TOPK_CAP of the tuning library): the plan, or None for the slab."""
    force = env_int(env, "SE_TOPK_FUSED")
    return _fused_plan(n, ldg, k, -1 if force is None else force, env_int(env, "SE_TOPK_J"), env_int(env, "SE_TOPK_CAP"))


def pf_padded_dim(d):
    """pf_padded_dim."""
    return (d + PF_BK - 1) // PF_BK * PF_BK


def last_steps(d):
    """pf_pass: k = 16 MFMA steps of the last chunk that hold data."""
    in_last = d - (pf_padded_dim(d) // PF_BK - 1) * PF_BK
    return PF_BK // 16 if (in_last <= 0 or in_last >= PF_BK) else (in_last + 15) // 16


def pf_geometry(n_a, n_q, want_parts, kp, env):
    """pf_geometry (SE_PF_BIG of the tuning library)."""
    big = 1 if (kp >= 256 and n_a >= 4096 and n_q >= 256) else 0
    if "SE_PF_BIG" in env:
        big = 1 if (kp > 0 and int(env["SE_PF_BIG"]) != 0) else 0
    bm = PB_BM if big else PF_BM
    tiles_m, tiles_n = (n_a + bm - 1) // bm, (n_q + bm - 1) // bm
    pf_grid = max(CUS * PF_WGS_PER_CU // 8 * 8, 8)
    per_xcd = (CUS // 8 * 8 if big else pf_grid) // 8
    gi = 8
    while gi > 1 and (gi > tiles_n or per_xcd % gi):
        gi >>= 1
    gj = max(1, min(per_xcd // gi, tiles_m))
    nsq = (tiles_n + gi - 1) // gi
    parts = want_parts if want_parts > 0 else (4 * 8 + nsq - 1) // nsq
    max_parts = tiles_m // gj if tiles_m // gj > 0 else 1
    parts = min(parts, max_parts)
    if parts * gj > 256:
        parts = 256 // gj if 256 // gj > 0 else 1
    parts = max(parts, 1)
    tpp = (tiles_m + parts - 1) // parts
    parts = (tiles_m + tpp - 1) // tpp
    return Geom(big, gi, gj, parts, tpp)


def sub_list_of_row(row, g):
    """pf_tile_kernel / pf_big_kernel: the sub-list (gallery range p, tile sequence j) -> p * gj + j that gallery row `row` is appended to."""
    t = row // (PB_BM if g.big else PF_BM)
    p = t // g.tpp
    return p * g.gj + (t - p * g.tpp) % g.gj


def fused_layout(q, n, d, plan, pf, env):
    """fused_layout (SE_TOPK_CAP, SE_TOPK_SPILL of the tuning library)."""
    cap, parts, nsub, spill, geom, kp = plan.cap, 1, 0, 0, None, 0
    if pf:
        geom = pf_geometry(n, q, 0, pf_padded_dim(d), env)
        nsub = geom.parts * geom.gj
        total_cap = align256(plan.cap * 3 // 2)
        cap = (total_cap // nsub + 32 + 15) // 16 * 16
        if "SE_TOPK_CAP" in env:
            cap = int(env["SE_TOPK_CAP"]) // nsub if int(env["SE_TOPK_CAP"]) // nsub > 0 else 1
        spill = nsub
        if "SE_TOPK_SPILL" in env:
            spill = int(env["SE_TOPK_SPILL"])
        parts = nsub + spill
        per_row = parts * (cap * 8 + 4) + plan.G * 4 + 16
    else:
        per_row = cap * 8 + plan.G * 4 + 16
    qt = (4 << 30) // per_row // 128 * 128
    qt = min(max(qt, 128), q)
    off_cnt = align256(qt * 4)
    off_gm = off_cnt + align256(qt * parts * 4 + 16 + qt * 4)
    off_lists = off_gm + align256(qt * plan.G * 4)
    off_spill = off_lists + align256(qt * (nsub if pf else parts) * cap * 8)
    off_scratch = off_spill + align256(qt * (spill if pf else 0) * cap * 8)
    total = off_scratch + align256(FB_GRID * n * 4)
    if pf:
        kp = pf_padded_dim(d)
        total += align256(qt * 4) + 256 + 2 * align256(n * 4) + 2 * align256(qt * 4) + align256(n * kp * 2) + align256(qt * kp * 2)
    return Layout(qt, parts, cap, nsub, spill, geom, kp, total)


def topk_qtile(q, n):
    """topk_qtile."""
    rows = (2 << 30) // (n * 4) // 128 * 128
    return min(max(rows, 128), q)


def retrieve_topk_plan(q, n, d, ldg, k, env=None):
    """retrieve_topk_plan + prefilter_wanted (SE_TOPK_PREFILTER): path, plan, layout and se_retrieve_topk_workspace_bytes."""
    env = env or {}
    plan = fused_plan_compute(n, ldg, k, env)
    if plan is None:
        return Retrieve(SLAB, None, None, topk_qtile(q, n) * ((n + 3) // 4 * 4) * 4)
    pf = k <= PF_K_MAX and (int(env["SE_TOPK_PREFILTER"]) != 0 if "SE_TOPK_PREFILTER" in env else True)
    L = fused_layout(q, n, d, plan, pf, env)
    return Retrieve(PREF if pf else FP32, plan, L, L.total)


def kblock_starts_on_4(kb):
    beg, ok = 0, True
    for length in (kb or [0]):
        ok = ok and beg % 4 == 0
        beg += length
    return ok


def fused_tuples(metric, kb, layout, d, q, n, allpairs, step, env):
    """launch_fused2 for both passes of a case whose operands share `layout`: -> ((METRIC, MULTI_KB, VEC) of the EPI_GROUPMIN launch,
    (METRIC, MULTI_KB, SYM, VEC) of the EPI_FILTER launch).  allpairs: SYM_T (the same tensor, and for the Euclidean metric the same
    norms, on both sides), COPY_T (a second copy of the gallery), ASYM_T."""
    multi = kb is not None and len(kb) > 1
    ld, aligned = PD.layout_pitch(layout, d), PD.layout_aligned(layout)
    vec_filter = ld % 4 == 0 and aligned and kblock_starts_on_4(kb)
    vec_sample = (step * ld) % 4 == 0 and ld % 4 == 0 and aligned and kblock_starts_on_4(kb)
    sym = allpairs == SYM_T and q == n and n > PD_TILE and "SE_TOPK_NOSYM" not in env
    return (metric, multi, vec_sample), (metric, multi, sym, vec_filter)


def refine_tuple(metric, layout, d):
    """retrieve_topk_prefilter: (METRIC, VEC, LONGROWS) of pf_refine_kernel."""
    vec = PD.layout_pitch(layout, d) % 4 == 0 and PD.layout_aligned(layout)
    return metric, vec, vec and d >= RF_STAGE_D


def fallback_staged(kb, layout, d):
    """topk_fallback_kernel: 16-byte rows and every K-block but the last a multiple of 4."""
    return PD.layout_pitch(layout, d) % 4 == 0 and PD.layout_aligned(layout) and all(b % 4 == 0 for b in (kb or [d])[:-1])


def rows_staged(metric, layout, d, kb, m):
    """pf_refine_kernel: the LDS row gather, given the refinement count m."""
    _, vec, longrows = refine_tuple(metric, layout, d)
    return longrows and vec and m <= RF_STAGE_M and d >= RF_STAGE_D and all(b % 4 == 0 for b in (kb or [d])[:-1])


# ------------------------------------------------------------------ case tables

SYM_T, COPY_T, ASYM_T = "sym", "copy", "asym"
# mode: FP32 / PREF (tuning library, SE_TOPK_FUSED=1; FP32 adds SE_TOPK_PREFILTER=0), SLAB (product library).  q: queries (all-pairs: n).
# clusters: None (random rows, no count claimed) or the cluster sizes (two queries per cluster; counts derived by cluster_outcome);
# align: every cluster starts on a multiple of it.  env: further switches.
Case = collections.namedtuple("Case", "mode metric pairs q n d k kb layout clusters align env")
KB = {7: (3, 4), 64: (32, 32), 100: (64, 36), 129: (64, 65), 555: (278, 277), 1000: (448, 276, 276)}      # later blocks on / off multiples of 4
QPC = 2                                               # queries per cluster
GAP = 0.05                                            # > 4.1 eps of the pre-filter on unit rows of up to 1,024 columns (eps < 0.01)


def case_id(c):
    return "%s-m%d-%s-%dx%dx%d-k%d-%s-%s-%s-%s" % (c.mode, c.metric, c.pairs, c.q, c.n, c.d, c.k, "kb%d" % len(c.kb) if c.kb else "kb1", c.layout,
                                                   "c" + ".".join(str(s).replace(", ", "+").strip("()") for s in c.clusters) if c.clusters else "rnd",
                                                   "_".join("%s%s" % (k[3:], v) for k, v in sorted(c.env)) or "noenv")


def E(**kw):
    return tuple(sorted(("SE_" + k, str(v)) for k, v in kw.items()))


def case_env(c):
    env = {"SE_TOPK_FUSED": "1"} if c.mode in (FP32, PREF) else {}
    if c.mode == FP32:
        env["SE_TOPK_PREFILTER"] = "0"
    if c.clusters:
        env["SE_TOPK_J"] = "1"
    env.update(dict(c.env))
    return env


def _fp32_tuple_cases():
    """The 16 EPI_FILTER tuples (hence the 8 EPI_GROUPMIN ones), each at two tile remainders, ragged in both directions; and k = 513,
    the first k past the pre-filter (PF_K_MAX) where the switch-free plan of such a gallery would be the slab."""
    cases = []
    ns = ((257, 450), (300, 641), (383, 700), (514, 259))            # n % 128: (1, 66), (44, 1), (127, 60), (2, 3)
    ks = (1, 10, 25, 40, 100, 251, 7, 64)
    for t, (metric, multi, sym, vec) in enumerate(itertools.product((COS, EUC), (False, True), (False, True), (False, True))):
        for rep in range(2):
            n, k = ns[t % 4][rep], ks[(t + 3 * rep) % len(ks)]
            if multi:
                d = (64, 100, 1000, 100)[(t + rep) % 4] if vec else (7, 129, 555, 64)[(t // 2 + rep) % 4]
                layout = (CONTIG, PADDED, ROWS)[(t + rep) % 3] if vec else (COL1 if d == 64 else (CONTIG, ROWS)[rep])
            else:
                d = (64, 100, 7, 1)[(t // 2 + rep) % 4] if vec else (1, 7, 129, 555)[(t // 2 + rep) % 4]
                layout = (PADDED if (d % 4 or rep) else CONTIG) if vec else (CONTIG, COL1)[rep]
            pairs = SYM_T if sym else (COPY_T, ASYM_T)[rep]
            q = n if pairs != ASYM_T else (130, 77, 200, 129)[t % 4]
            cases.append(Case(FP32, metric, pairs, q, n, d, min(k, n), KB[d] if multi else None, layout, None, 1, ()))
    # the symmetric walk switched off on an all-pairs call: the same bits
    cases.append(Case(FP32, EUC, SYM_T, 300, 300, 100, 25, None, CONTIG, None, 1, E(TOPK_NOSYM=1)))
    cases.append(Case(FP32, COS, ASYM_T, 77, 700, 64, PF_K_MAX + 1, None, CONTIG, None, 1, ()))
    return cases


def _fp32_list_cases():
    """topk_lists_kernel: every sort width, k - 1 / k, and cap / cap + 1 at 1,024 / 4,096 / 8,192."""
    return [
        Case(FP32, COS, ASYM_T, 16, 7800, 64, 251, None, CONTIG, (250, 251, 512, 513, 1024, 1025, 2048, 2049), 12, E(TOPK_CAP=8192)),
        Case(FP32, EUC, ASYM_T, 16, 7800, 64, 251, None, COL1, (250, 251, 512, 513, 1024, 1025, 2048, 2049), 12, E(TOPK_CAP=1024)),
        Case(FP32, EUC, ASYM_T, 4, 8800, 64, 64, KB[64], CONTIG, (4096, 4097), 12, E(TOPK_CAP=8192)),
        Case(FP32, COS, ASYM_T, 4, 8800, 64, 64, None, CONTIG, (4096, 4097), 12, E(TOPK_CAP=4096)),
        Case(FP32, COS, ASYM_T, 2, 8704, 64, 100, None, PADDED, (8192,), 12, E(TOPK_CAP=8192)),
        Case(FP32, EUC, ASYM_T, 2, 8704, 64, 100, None, CONTIG, (8193,), 12, E(TOPK_CAP=8192)),
    ]


M_EDGES = (63, 64, 65, 128, 129, 256, 257, 384, 385, 512, 513, 1024, 1025)       # k - 1 / k at k = 64, every sort_candidates<WAVE> width, RF_STAGE_M, RF_MAX
TWO_LEVEL = ((100, 924), (100, 925), (384, 700), (385, 700))
SPILL_N, SPILL_D = 600, 64                                                        # 5 gallery tiles = 5 sub-lists, one cluster per tile


def _pref_cluster_cases():
    """The six pf_refine_kernel tuples over the m edges (total = m: the staged-list edge 1,024 / 1,025 too), and the spill edges."""
    me = lambda metric, d, kb, layout: Case(PREF, metric, ASYM_T, QPC * len(M_EDGES), 5100, d, 64, kb, layout, M_EDGES, 12, E(TOPK_CAP=8192))  # noqa: E731
    cases = [me(COS, 64, None, CONTIG), me(EUC, 64, None, COL1), me(COS, 65, None, COL1), me(EUC, 100, None, ROWS),
             me(COS, 256, None, CONTIG), me(EUC, 260, None, PADDED), me(COS, 1000, KB[1000], CONTIG), me(EUC, 1000, KB[1000], ROWS),
             me(EUC, 556, (278, 278), CONTIG), me(COS, 556, (278, 278), CONTIG)]
    # two-level clusters: lists of 1,024 (staged in LDS) / 1,025 (walked in place) entries of which 100 are refined, and 1,084 / 1,085
    # entries with m on both sides of RF_STAGE_M
    two = lambda metric, d, kb, layout: Case(PREF, metric, ASYM_T, QPC * len(TWO_LEVEL), 5100, d, 64, kb, layout, TWO_LEVEL, 12, E(TOPK_CAP=8192))  # noqa: E731
    cases += [two(COS, 64, None, CONTIG), two(EUC, 64, None, COL1), two(COS, 256, None, CONTIG), two(EUC, 1000, KB[1000], ROWS)]
    sp = lambda metric, clusters, layout, **env: Case(PREF, metric, ASYM_T, QPC * len(clusters), SPILL_N, SPILL_D, 8, None, layout, clusters, 128, E(**env))  # noqa: E731
    cases += [
        # sub-list capacity 80 / 5 = 16, spill region 2 x 16: sub-list full, one more, spill region full, one more
        sp(COS, (16, 17, 48, 49), CONTIG, TOPK_CAP=80, TOPK_SPILL=2),
        sp(EUC, (16, 17, 48, 49), COL1, TOPK_CAP=80, TOPK_SPILL=2),
        # every query beyond the spill region: all redone, same bits
        sp(COS, (49, 50, 128), PADDED, TOPK_CAP=80, TOPK_SPILL=2),
        # no spill region at all
        sp(EUC, (16, 17), CONTIG, TOPK_CAP=80, TOPK_SPILL=0),
        # the spill region of the product's size (as many slots as sub-lists): 16 + 5 x 16
        sp(COS, (96, 97), CONTIG, TOPK_CAP=80),
        # the 256 x 256 filter kernel: 3 tiles = 3 sub-lists of 96 / 3 = 32, spill 1 x 32
        sp(EUC, (32, 33, 64, 65), CONTIG, TOPK_CAP=96, TOPK_SPILL=1, PF_BIG=1),
        sp(COS, (32, 33, 64, 65), COL1, TOPK_CAP=96, TOPK_SPILL=1, PF_BIG=1),
    ]
    return cases


PF_DEPTHS_ONE = (1, 17, 33, 64, 65, 96, 100, 128)                 # last_steps 1 .. 8 with one chunk (128: the full last chunk)
PF_DEPTHS_MANY = (129, 145, 161, 192, 193, 224, 228, 256, 555)    # the same with two chunks; 555: five chunks


def _pref_random_cases():
    """Every last_steps value with one and with several chunks, both tile kernels and the 256 x 256 kernel at one-tile and several-tile
    galleries, all-pairs calls (one image serves both sides), K-blocks, every layout."""
    cases = []
    layouts = (CONTIG, PADDED, COL1, ROWS)
    for i, d in enumerate(PF_DEPTHS_ONE + PF_DEPTHS_MANY):
        metric = (COS, EUC)[i % 2]
        n = (300, 385, 513, 700, 259)[i % 5]
        pairs = (ASYM_T, ASYM_T, SYM_T, ASYM_T, COPY_T)[i % 5]
        q = n if pairs != ASYM_T else (130, 77, 200)[i % 3]
        kb = KB.get(d) if i % 2 else None
        cases.append(Case(PREF, metric, pairs, q, n, d, min((1, 10, 25, 100)[i % 4], n), kb, layouts[i % 4], None, 1, ()))
    cases.append(Case(PREF, EUC, ASYM_T, 77, 700, 64, PF_K_MAX, None, CONTIG, None, 1, ()))                        # the last k of the pre-filter
    for metric in (COS, EUC):
        cases.append(Case(PREF, metric, ASYM_T, 130, 256, 100, 10, None, CONTIG, None, 1, E(PF_BIG=1)))             # one tile of 256 rows
        cases.append(Case(PREF, metric, SYM_T, 700, 700, 129, 25, KB[129], COL1, None, 1, E(PF_BIG=1)))             # three tiles, ragged
        cases.append(Case(PREF, 1 - metric, ASYM_T, 300, 641, 1000, 40, KB[1000], PADDED, None, 1, E(PF_BIG=1)))
    return cases


def _slab_cases():
    """The slab path of the product library: n % 4 in {1, 2, 3} (slab pitch (n + 3) / 4 * 4), every layout, both metrics, K-blocks."""
    return [
        Case(SLAB, COS, ASYM_T, 130, 129, 100, 25, None, CONTIG, None, 1, ()),
        Case(SLAB, EUC, ASYM_T, 77, 130, 7, 10, KB[7], COL1, None, 1, ()),
        Case(SLAB, COS, COPY_T, 131, 131, 555, 131, KB[555], PADDED, None, 1, ()),
        Case(SLAB, EUC, SYM_T, 257, 257, 64, 40, None, ROWS, None, 1, ()),
        Case(SLAB, COS, SYM_T, 258, 258, 129, 1, KB[129], COL1, None, 1, ()),
        Case(SLAB, EUC, ASYM_T, 200, 699, 1000, 251, KB[1000], PADDED, None, 1, ()),
    ]


FP32_CASES = _fp32_tuple_cases() + _fp32_list_cases()
PREF_CASES = _pref_cluster_cases() + _pref_random_cases()
SLAB_CASES = _slab_cases()
ALL_CASES = FP32_CASES + PREF_CASES + SLAB_CASES

# product thresholds: (n, k) -> the path retrieve_topk_plan takes in the product library (no switches); 48 queries, D = 64
# (16,384 rows resolve k up to 355: k = 512 and 513 both take the slab there; the pre-filter / fp32 edge PF_K_MAX itself is pinned by the
# k = 512 and k = 513 cases of the tuning-library tables, and by the plan of a 50,000-row gallery below)
PRODUCT_THRESHOLDS = (((16383, 64), SLAB), ((16384, 64), PREF), ((16384, 355), PREF), ((16384, 356), SLAB), ((16384, 512), SLAB), ((16384, 513), SLAB))
PRODUCT_FP32 = ((50000, 512), (50000, 513))           # PREF / FP32: restated only (tests/test_gpu_topk.py runs that size)


# ------------------------------------------------------------------ case data and what the host derives from it

def normalize(x):
    return ro.canon_normalize_rows(np.ascontiguousarray(x, dtype=F32))


def cluster_sizes(c):
    """-> [(copies of the centre outside the sample, copies of what the sample sees)]: a plain cluster of T copies is (0, T) -- its
    first row is sampled; a two-level cluster (TA, TB) has TB copies of a COMPANION of the centre under the sample and TA copies of the
    centre itself behind the last sampled row, so tau admits TA + TB candidates and the k-th distance only TA of them."""
    return [s if isinstance(s, tuple) else (0, s) for s in c.clusters]


def cluster_starts(c):
    """-> [(first row of the TA block or None, first row of the TB block)] of every cluster."""
    plan = case_plan(c).plan
    starts, pos, tail = [], 0, plan.S * plan.step
    for ta, tb in cluster_sizes(c):
        pos = (pos + c.align - 1) // c.align * c.align
        tail = (tail + c.align - 1) // c.align * c.align
        starts.append((tail if ta else None, pos))
        pos += tb
        tail += ta
    two = any(ta for ta, _ in cluster_sizes(c))
    assert all(b < plan.S * plan.step for _, b in starts) and pos <= (plan.S * plan.step if two else c.n) and tail <= c.n, case_id(c)
    return starts


@functools.lru_cache(maxsize=2)
def case_data(c):
    """-> (queries [q, d], gallery [n, d]) float32, unit rows.  Random cases: gaussian rows, the queries a permuted subset (or all) of
    the gallery.  Cluster cases: orthonormal centres (and companions: centre + 0.7 x a direction of its own), clusters of exact copies,
    every other row orthogonal to all of them, QPC queries next to every centre."""
    rng = np.random.default_rng((c.metric * 7919 + c.n * 31 + c.d * 131 + c.k * 17 + c.q) % (1 << 31))
    if not c.clusters:
        g = rng.standard_normal((c.n, c.d)).astype(F32)
        if c.d > 1 or c.metric == COS:
            g = normalize(g)
        g[c.n // 2] = g[1]                                              # one exact duplicate: a tie broken by index
        qs = g if c.pairs != ASYM_T else np.ascontiguousarray(g[rng.permutation(max(c.n, c.q))[:c.q] % c.n])
        assert qs.shape == (c.q, c.d) and g.shape == (c.n, c.d)
        return qs, g
    nc = len(c.clusters)
    basis, _ = np.linalg.qr(rng.standard_normal((c.d, c.d)))
    centres, extra, rest = normalize(basis[:, :nc].T), basis[:, nc:2 * nc].T, basis[:, 2 * nc:].T
    g = normalize(rng.standard_normal((c.n, rest.shape[0])) @ rest)
    for (tail, start), (ta, tb), ctr, ex in zip(cluster_starts(c), cluster_sizes(c), centres, extra):
        g[start:start + tb] = normalize((ctr + 0.7 * ex)[None, :])[0] if ta else ctr
        if ta:
            g[tail:tail + ta] = ctr
    qs = np.concatenate([normalize(ctr[None, :] + 0.1 * rng.standard_normal((QPC, c.d)) / math.sqrt(c.d)) for ctr in centres])
    assert qs.shape == (c.q, c.d) and g.shape == (c.n, c.d)
    return qs, g


@functools.lru_cache(maxsize=2)
def case_oracle(c):
    qs, g = case_data(c)
    pd = ro.canon_pdist(qs, g, c.metric, kblocks=c.kb)
    return pd, ro.canon_topk_rows(pd, c.k)


def case_plan(c):
    return retrieve_topk_plan(c.q, c.n, c.d, PD.layout_pitch(c.layout, c.d), c.k, case_env(c))


Outcome = collections.namedtuple("Outcome", "total m spilled redone")


def cluster_outcome(c):
    """Per query of a cluster case, from the case's own distances and the restated plan and geometry: candidate count, refinement
    count m, entries sent to the spill region, and whether the query is handed to the exact fallback.  tau is the smallest sampled
    distance (SE_TOPK_J=1); nothing may lie within GAP above tau or above the k-th distance, so the half-precision pass sees the same
    sets.  fp32 path: m and spilled are 0."""
    pd, _ = case_oracle(c)
    r = case_plan(c)
    env = case_env(c)
    assert env.get("SE_TOPK_J") == "1" and r.plan.j == 1
    sampled = np.arange(r.plan.S, dtype=np.int64) * r.plan.step
    out = []
    for row in pd:
        tau = row[sampled].min()
        cand = np.nonzero(row <= tau)[0]
        assert not ((row > tau) & (row <= tau + GAP)).any()
        total = len(cand)
        if r.path == FP32:
            out.append(Outcome(total, 0, 0, total < c.k or total > r.plan.cap))
            continue
        L = r.layout
        per_sub = np.bincount([sub_list_of_row(int(i), L.geom) for i in cand], minlength=L.nsub)
        spilled = int(np.maximum(per_sub - L.cap, 0).sum())
        overflow = spilled > L.spill * L.cap
        m = 0
        if total >= c.k:
            kth = np.partition(row, c.k - 1)[c.k - 1]
            m = int((row <= kth).sum())
            assert not ((row > kth) & (row <= kth + GAP)).any()
        out.append(Outcome(total, m, spilled, overflow or total < c.k or m > RF_MAX))
    return out


def expected_counters(c):
    """What se_phase_timing_read reports behind a pre-filter call: every query, the redone ones, and m / the candidate count summed over
    the accepted ones.  Random cases claim the query count only."""
    if not c.clusters:
        return {"queries": c.q}
    oc = cluster_outcome(c)
    return {"queries": c.q, "redone": sum(o.redone for o in oc), "recomputed": sum(o.m for o in oc if not o.redone),
            "candidates": sum(o.total for o in oc if not o.redone)}


# ------------------------------------------------------------------ se_topk_rows cases

# (name, n, k, input pitch - n (NaN padding), col_offset, rows of the call (0: the block once), candidate counts of the constructed rows)
RowsCase = collections.namedtuple("RowsCase", "name n k pad col_offset q edges")
ROWS_CASES = [
    RowsCase("radix-8191", 8191, 251, 5, 0, 0, ()),
    RowsCase("radix-k-is-n", 2048, 2048, 0, 7, 0, ()),
    RowsCase("radix-k-is-n-ragged", 333, 333, 3, 0, 0, ()),
    RowsCase("sample-k1", 8192, 1, 0, 0, 0, (22, 512, 513)),                          # (a count is at least the pivot's rank + 1 = 22)
    RowsCase("sample-k251", 8192, 251, 4, 1000, 0, (250, 251, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192)),
    RowsCase("sample-k2048", 8192, 2048, 0, 0, 0, (2047, 2048, 2049, 4096, 4097, 8192)),
    RowsCase("sample-cap", 8704, 251, 7, 123456, 0, (8192, 8193, 8704)),
    RowsCase("persistent", 8192, 251, 4, 0, 2100, (250, 251, 513, 1025, 2049, 4097)),
]
ROWS_GRIDS = (1024, 2048)                              # topk_sample_kernel / topk_rows_kernel


def edge_row(rng, n, k, total):
    """A row with exactly `total` keys <= the pivot: r distinct small values and the pivot value at sample positions, total - r - 1
    further values not above the pivot elsewhere (at a sample position: the pivot value itself, which leaves the pivot's rank alone),
    larger values everywhere else.  The values repeat: ties are broken by index."""
    sample, r = pivot_rank(n, k)
    assert sample and total >= r + 1
    pos = sample_positions(n)
    row = (10.0 + rng.integers(0, 50, size=n)).astype(F32)
    chosen = rng.permutation(TK_SAMPLES)
    row[pos[chosen[:r]]] = (-(1.0 + np.arange(r)) / 1024.0).astype(F32)
    pivot = F32(1.0)
    row[pos[chosen[r]]] = pivot
    free = np.setdiff1d(np.arange(n), pos)
    free = free[rng.permutation(len(free))]
    extra = total - r - 1
    low = free[:min(extra, len(free))]
    row[low] = rng.choice(np.array([1.0, 0.5, 0.5, 0.0, -0.0, -3.0], dtype=F32), size=len(low))
    if extra > len(free):
        row[pos[chosen[r + 1:r + 1 + extra - len(free)]]] = pivot
    return row


def special_rows(rng, n):
    """Signed zeros, infinities, NaN (sorted last), one value everywhere, and gaussian rows."""
    rows = [rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)]
    v = rng.standard_normal(n).astype(F32)
    v[::3] = rng.choice(np.array([0.0, -0.0], dtype=F32), size=len(v[::3]))
    v[5::97] = np.inf
    v[7::89] = -np.inf
    rows.append(v)
    w = rng.standard_normal(n).astype(F32)
    w[::2] = np.nan
    rows.append(w)
    rows.append(np.full(n, 2.5, dtype=F32))
    rows.append(np.full(n, np.nan, dtype=F32))
    return rows


@functools.lru_cache(maxsize=2)
def rows_block(rc):
    rng = np.random.default_rng(rc.n * 7 + rc.k)
    rows = special_rows(rng, rc.n)
    for t in rc.edges:                                 # constructed rows between ordinary ones: the repair pass redoes some and skips others
        rows.insert(len(rows) // 2, edge_row(rng, rc.n, rc.k, t))
    if rc.q:
        while any(math.gcd(len(rows), g) != 1 for g in ROWS_GRIDS):
            rows.append(rng.standard_normal(rc.n).astype(F32))
    return np.stack(rows)


# ------------------------------------------------------------------ CPU: the restatements and the tables

def test_topk_rows_restatement_and_edges():
    assert pivot_rank(8191, 251) == (False, 108) and pivot_rank(8192, 251) == (True, 108)
    assert pivot_rank(8192, 1) == (True, 21) and pivot_rank(8192, 2048)[0] and pivot_rank(50000, 251)[0]
    assert not pivot_rank(2048, 2048)[0] and not pivot_rank(1000000, 2048)[0]                # upper bound above TK_CAP
    assert sample_positions(8192)[[0, 1, 2047]].tolist() == [0, 4, 8188] and sample_positions(8704)[[1, 4, 2047]].tolist() == [4, 17, 8699]
    assert len(set(sample_positions(8704).tolist())) == TK_SAMPLES
    assert [sort_width(t, 512) for t in (1, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    seen, edges = set(), set()
    for rc in ROWS_CASES:
        block = rows_block(rc)
        sample, r = pivot_rank(rc.n, rc.k)
        assert sample == (not rc.name.startswith("radix")), rc.name
        outcomes = [sample_outcome(row, rc.k) for row in block]
        # every constructed row has exactly the claimed candidate count, and the width / redo verdict that count selects
        got = [o for o in outcomes if o[0] in rc.edges]
        for t in rc.edges:
            want = "redo" if (t < rc.k or t > TK_CAP) else sort_width(t, TK_THREADS)
            assert (t, want) in got, (rc.name, t, outcomes)
            edges.add((rc.k, t))
        seen |= {o[1] for o in outcomes}
        if any(t < rc.k or t > TK_CAP for t in rc.edges):      # redone and kept rows next to each other, in both orders
            redo = [o[1] == "redo" for o in outcomes]
            assert any(a and not b for a, b in zip(redo, redo[1:])) and any(b and not a for a, b in zip(redo, redo[1:])), rc.name
        if rc.q:
            assert rc.q > max(ROWS_GRIDS) and all(math.gcd(len(block), g) == 1 for g in ROWS_GRIDS)
    assert seen == {1, 2, 4, 8, 16, "redo", "radix"}
    # both sides of every count edge: k - 1 / k, 512 x {1, 2, 4, 8} (+ 1), TK_CAP (+ 1)
    for k in (251, 2048):
        assert {(k, k - 1), (k, k)} <= edges
    for t in (512, 1024, 2048, 4096):
        assert {(251, t), (251, t + 1)} <= edges, t
    assert {(251, 8192), (251, 8193)} <= edges
    assert {rc.n for rc in ROWS_CASES} >= {8191, 8192} and {rc.k for rc in ROWS_CASES} >= {1, 251, 2048}
    assert any(rc.k == rc.n for rc in ROWS_CASES) and any(rc.pad and rc.col_offset for rc in ROWS_CASES)


def test_plan_restatement_thresholds_and_switches():
    # the product library: slab below 16,384 rows, pre-filter up to k = 512, fp32 fused passes above (where the sample resolves k / n)
    for (n, k), path in PRODUCT_THRESHOLDS:
        assert retrieve_topk_plan(48, n, 64, 64, k).path == path, (n, k)
    assert [retrieve_topk_plan(48, n, 64, 64, k).path for n, k in PRODUCT_FP32] == [PREF, FP32]
    assert retrieve_topk_plan(150, 50000, 100, 100, 1000).path == FP32 and retrieve_topk_plan(384, 20000, 100, 100, 251).path == PREF
    paths = {(n, k): p for (n, k), p in PRODUCT_THRESHOLDS}
    assert paths[(16383, 64)] != paths[(16384, 64)] and paths[(16384, 355)] != paths[(16384, 356)]
    assert {(c.mode, c.k) for c in ALL_CASES if c.k in (PF_K_MAX, PF_K_MAX + 1) and not c.clusters} == {(PREF, PF_K_MAX), (FP32, PF_K_MAX + 1)}
    # plans of full-size calls the library is known to make (50,000 x 100, k = 251: 2,048 samples, 128 group minima)
    p = retrieve_topk_plan(50000, 50000, 100, 100, 251)
    assert (p.plan.S, p.plan.step, p.plan.G) == (2048, 24, 128) and 1 < p.plan.j <= 64 and p.plan.cap % 256 == 0 and p.layout.geom.big == 0
    assert retrieve_topk_plan(50000, 50000, 1000, 1000, 251).layout.geom.big == 1
    # the tuning switches
    f1 = {"SE_TOPK_FUSED": "1"}
    assert retrieve_topk_plan(10, 255, 64, 64, 5, f1).path == SLAB and retrieve_topk_plan(10, 256, 64, 64, 5, f1).path == PREF
    assert retrieve_topk_plan(10, 256, 64, 64, 5, dict(f1, SE_TOPK_PREFILTER="0")).path == FP32
    assert retrieve_topk_plan(10, 300, 64, 64, 5, {"SE_TOPK_FUSED": "0"}).path == SLAB
    assert retrieve_topk_plan(10, 700, 64, 64, 600, f1).path == FP32                          # k above PF_K_MAX
    assert retrieve_topk_plan(10, 700, 64, 64, 5, dict(f1, SE_TOPK_CAP="8193")).path == SLAB     # a capacity above TK_CAP: no plan
    p = retrieve_topk_plan(10, 700, 64, 64, 5, dict(f1, SE_TOPK_J="1", SE_TOPK_CAP="80", SE_TOPK_SPILL="2"))
    assert (p.plan.S, p.plan.step, p.plan.G, p.plan.j) == (256, 2, 16, 1)
    assert (p.layout.geom, p.layout.nsub, p.layout.cap, p.layout.spill, p.layout.parts) == (Geom(0, 1, 6, 1, 6), 6, 13, 2, 8)
    assert retrieve_topk_plan(10, 700, 64, 64, 5, dict(f1, SE_PF_BIG="1")).layout.geom == Geom(1, 1, 3, 1, 3)
    # last_steps and the padded depth
    assert [last_steps(d) for d in (1, 16, 17, 32, 33, 64, 65, 96, 100, 112, 113, 127, 128, 129, 256, 257, 555, 1000)] == \
        [1, 1, 2, 2, 3, 4, 5, 6, 7, 7, 8, 8, 8, 1, 8, 1, 3, 7]
    assert [pf_padded_dim(d) for d in (1, 128, 129, 1000)] == [128, 128, 256, 1024]
    # slab workspace: rows on a 16-byte pitch
    assert [retrieve_topk_plan(10, n, 7, 7, 3).need for n in (129, 130, 131, 132)] == [10 * 132 * 4] * 4


def census(cases):
    gm, flt, refine, fallback, pf_kernels = (collections.defaultdict(set) for _ in range(5))
    for c in cases:
        r = case_plan(c)
        assert r.path == c.mode, (case_id(c), r.path)
        env = case_env(c)
        if c.mode == FP32:
            a, b = fused_tuples(c.metric, c.kb, c.layout, c.d, c.q, c.n, c.pairs, r.plan.step, env)
            gm[a].add(c.n % PD_TILE)
            flt[b].add((c.n % PD_TILE, c.q % PD_TILE))
        if c.mode == PREF:
            refine[refine_tuple(c.metric, c.layout, c.d)].add(c.d)
            pf_kernels[(c.metric, "groupmin")].add(c.n)
            pf_kernels[(c.metric, "big" if r.layout.geom.big else "filter")].add((c.n + (PB_BM if r.layout.geom.big else PF_BM) - 1) // (PB_BM if r.layout.geom.big else PF_BM))
        if c.mode in (FP32, PREF):
            fallback[(c.metric, fallback_staged(c.kb, c.layout, c.d))].add(bool(c.clusters) and any(o.redone for o in cluster_outcome(c)))
    return gm, flt, refine, fallback, pf_kernels


def test_case_tables_reach_every_instantiation():
    assert len({case_id(c) for c in ALL_CASES}) == len(ALL_CASES)
    # a row that leaves a table changes a count
    assert (len(FP32_CASES), len(PREF_CASES), len(SLAB_CASES), len(ROWS_CASES), len(PRODUCT_THRESHOLDS)) == (40, 45, 6, 8, 6)
    for c in ALL_CASES:
        assert c.n <= 16384 and c.k <= min(c.n, TOPK_MAX) and (c.q == c.n) == (c.pairs != ASYM_T), case_id(c)
        assert c.kb is None or (sum(c.kb) == c.d and len(c.kb) > 1), case_id(c)
        assert c.n <= 1000 or c.clusters, case_id(c)                              # only the count edges need more than 1,000 rows
        if c.mode in (FP32, PREF):
            assert c.n >= 256 and (c.pairs != SYM_T or c.n > PD_TILE), case_id(c)
    gm, flt, refine, fallback, pf_kernels = census(ALL_CASES)
    # the 8 EPI_GROUPMIN and the 16 EPI_FILTER instantiations of pdist_kernel, each at two tile remainders
    assert set(gm) == set(itertools.product((COS, EUC), (False, True), (False, True))), sorted(gm)
    assert set(flt) == set(itertools.product((COS, EUC), (False, True), (False, True), (False, True))), sorted(flt)
    assert all(len(v) >= 2 for v in gm.values()) and all(len({r[0] for r in v}) >= 2 for v in flt.values()), (gm, flt)
    assert all(any(r[0] for r in v) for v in flt.values())                       # ragged last tiles everywhere
    # SYM with a K-block list, and SYM without 16-byte loads
    assert all(flt[(m, True, True, v)] for m in (COS, EUC) for v in (False, True)) and all(flt[(m, mu, True, False)] for m in (COS, EUC) for mu in (False, True))
    # K-block lists whose later blocks start on and off multiples of 4
    assert {kblock_starts_on_4(c.kb) for c in FP32_CASES if c.kb} == {True, False}
    assert sum("SE_TOPK_NOSYM" in dict(c.env) for c in FP32_CASES) == 1
    # pf_tile_kernel<METRIC, GROUPMIN | FILTER> and pf_big_kernel<METRIC>, the latter at one-tile and several-tile galleries
    assert set(pf_kernels) == set(itertools.product((COS, EUC), ("groupmin", "filter", "big")))
    assert all(1 in pf_kernels[(m, "big")] and max(pf_kernels[(m, "big")]) >= 3 for m in (COS, EUC))
    # the six legal pf_refine_kernel tuples; LONGROWS at D = 256, 260, 1000 and with a K-block that is no multiple of 4
    assert set(refine) == {(m, v, l) for m in (COS, EUC) for v, l in ((False, False), (True, False), (True, True))}
    assert set().union(*(refine[(m, True, True)] for m in (COS, EUC))) >= {256, 260, 1000, 556}
    for m in (COS, EUC):
        direct = [c for c in PREF_CASES if c.clusters and c.metric == m and refine_tuple(m, c.layout, c.d)[2] and not rows_staged(m, c.layout, c.d, c.kb, 64)]
        assert direct and all(any(b % 4 for b in c.kb[:-1]) for c in direct), m
    # topk_fallback_kernel<METRIC>, staged and unstaged, each with queries that are certainly redone (the count cases)
    assert set(fallback) == set(itertools.product((COS, EUC), (False, True))) and all(True in v for v in fallback.values()), fallback
    # all-pairs pre-filter call at a small ragged n; every layout on every path
    assert any(c.mode == PREF and c.pairs == SYM_T and c.n % PF_BM for c in PREF_CASES)
    for cases in (FP32_CASES, PREF_CASES, SLAB_CASES):
        assert {c.layout for c in cases} == {CONTIG, PADDED, COL1, ROWS}, cases[0].mode
    # the slab: n % 4 in {1, 2, 3}, both metrics, K-blocks
    assert {c.n % 4 for c in SLAB_CASES} >= {1, 2, 3} and {c.metric for c in SLAB_CASES} == {COS, EUC} and any(c.kb for c in SLAB_CASES)
    print("\ncases: fp32 fused %d, pre-filter %d, slab %d, se_topk_rows %d" % (len(FP32_CASES), len(PREF_CASES), len(SLAB_CASES), len(ROWS_CASES)))
    print("EPI_GROUPMIN tuples x cases: " + " ".join("%d%d%d:%d" % (t + (sum(fused_tuples(c.metric, c.kb, c.layout, c.d, c.q, c.n, c.pairs, case_plan(c).plan.step, case_env(c))[0] == t for c in FP32_CASES),)) for t in sorted(gm)))
    print("EPI_FILTER tuples x cases: " + " ".join("%d%d%d%d:%d" % (t + (sum(fused_tuples(c.metric, c.kb, c.layout, c.d, c.q, c.n, c.pairs, case_plan(c).plan.step, case_env(c))[1] == t for c in FP32_CASES),)) for t in sorted(flt)))
    print("pf_refine_kernel tuples x cases: " + " ".join("%d%d%d:%d" % (t + (sum(refine_tuple(c.metric, c.layout, c.d) == t for c in PREF_CASES),)) for t in sorted(refine)))


def test_case_tables_reach_every_last_steps_value():
    one = {last_steps(c.d) for c in PREF_CASES if not c.clusters and pf_padded_dim(c.d) == PF_BK}
    many = {last_steps(c.d) for c in PREF_CASES if not c.clusters and pf_padded_dim(c.d) > PF_BK}
    assert one == set(range(1, 9)) and many == set(range(1, 9)), (one, many)
    depths = {c.d for c in PREF_CASES}
    assert {128, 256} <= depths and any(17 <= d % 128 <= 32 for d in depths)          # full last chunks; D in 17 .. 32 mod 128
    assert set(ERROR_BOUND_DEPTHS) == {1, 16, 17, 32, 33, 64, 65, 96, 112, 113, 127, 128, 129, 256, 257}


def test_cluster_cases_claim_derived_counts_on_every_edge():
    """The counts of every counting case, derived from its own distances: sort widths and count edges of topk_lists_kernel and
    pf_refine_kernel, the staged-list and row-gather edges, the spill edges."""
    lists_w, lists_edges, refine_w, m_seen, staged_rows, spill_seen = set(), set(), collections.defaultdict(set), collections.defaultdict(set), set(), set()
    lists_staged = set()
    lines = []
    for c in ALL_CASES:
        if not c.clusters:
            continue
        oc = cluster_outcome(c)
        r = case_plan(c)
        # every query of a cluster has exactly the cluster's size as its candidate count
        assert [o.total for o in oc] == [ta + tb for ta, tb in cluster_sizes(c) for _ in range(QPC)], case_id(c)
        if c.mode == FP32:
            assert r.plan.cap == int(dict(c.env)["SE_TOPK_CAP"])
            for o in oc:
                lists_edges.add((o.total, "redo" if o.redone else sort_width(o.total, TK_THREADS), r.plan.cap))
                if not o.redone:
                    lists_w.add(sort_width(o.total, TK_THREADS))
        else:
            t = refine_tuple(c.metric, c.layout, c.d)
            for o, (ta, tb) in zip(oc, [s for s in cluster_sizes(c) for _ in range(QPC)]):
                assert o.m == (0 if o.total < c.k else (ta or tb)), case_id(c)
                lists_staged.add((t[1:], o.total <= RF_MAX, o.m, o.redone))
                if not o.redone:
                    refine_w[t].add(sort_width(o.m, 64))
                    staged_rows.add((t, rows_staged(c.metric, c.layout, c.d, c.kb, o.m), o.m))
                m_seen[t].add((o.m or o.total, o.redone))
                spill_seen.add((r.layout.cap, r.layout.spill, r.layout.geom.big, o.total, o.spilled, o.redone))
        lines.append("%s: %s" % (case_id(c), " ".join("%d%s" % (o.total, "R" if o.redone else "") for o in oc[::QPC])))
    # topk_lists_kernel: five widths; k - 1 / k; 512 x {1, 2, 4, 8} and one more; cap / cap + 1 at three capacities
    assert lists_w == set(SORT_WIDTHS)
    have = {(t, w) for t, w, _ in lists_edges}
    assert {(250, "redo"), (251, 1), (512, 1), (513, 2), (1024, 2), (1025, 4), (2048, 4), (2049, 8), (4096, 8), (4097, 16), (8192, 16), (8193, "redo")} <= have, sorted(have)
    assert {(1024, 2, 1024), (1025, "redo", 1024), (4096, 8, 4096), (4097, "redo", 4096), (8192, 16, 8192), (8193, "redo", 8192)} <= lists_edges
    # pf_refine_kernel: every tuple sees every width and both sides of k - 1 / k, 64 x {1 .. 8}, RF_STAGE_M, RF_MAX (= the staged-list edge)
    for t in {(m, v, l) for m in (COS, EUC) for v, l in ((False, False), (True, False), (True, True))}:
        assert refine_w[t] == set(SORT_WIDTHS), t
        assert {(63, True), (64, False), (65, False), (128, False), (129, False), (256, False), (257, False), (384, False), (385, False),
                (512, False), (513, False), (1024, False), (1025, True)} <= m_seen[t], (t, sorted(m_seen[t]))
    for m in (COS, EUC):                               # the LDS row gather on both sides of RF_STAGE_M, and never without LONGROWS
        assert {((m, True, True), True, 384), ((m, True, True), False, 385)} <= staged_rows
    assert not any(s for t, s, _ in staged_rows if not t[2])
    # candidate lists staged in LDS (up to RF_MAX entries) and walked in place (one more), both ACCEPTED, per (VEC, LONGROWS); with
    # the row gather on both sides of RF_STAGE_M behind a list that is walked in place
    for vl in ((False, False), (True, False), (True, True)):
        assert {(vl, True, 100, False), (vl, False, 100, False), (vl, False, 384, False), (vl, False, 385, False)} <= lists_staged, (vl, sorted(lists_staged))
    # spill: sub-list exactly full (nothing spilled), one more, spill region exactly full, one more (redone), no spill region
    assert {(16, 2, 0, 16, 0, False), (16, 2, 0, 17, 1, False), (16, 2, 0, 48, 32, False), (16, 2, 0, 49, 33, True), (16, 2, 0, 128, 112, True),
            (16, 0, 0, 16, 0, False), (16, 0, 0, 17, 1, True), (16, 5, 0, 96, 80, False), (16, 5, 0, 97, 81, True),
            (32, 1, 1, 32, 0, False), (32, 1, 1, 33, 1, False), (32, 1, 1, 64, 32, False), (32, 1, 1, 65, 33, True)} <= spill_seen, sorted(spill_seen)
    assert any(all(o.redone for o in cluster_outcome(c)) for c in PREF_CASES if c.clusters)     # every query redone
    print("\ncandidate counts per cluster (R: handed to the exact fallback):\n  " + "\n  ".join(lines))


def test_oracle_cost_of_the_largest_cases():
    """The sizes the tables may use: the oracle's work per case stays small (q x n x d multiply-adds, sort of q x n keys)."""
    for c in ALL_CASES:
        assert c.q * c.n * c.d <= 5e8 and c.q * c.n <= 1.3e6, case_id(c)
        qs, g = case_data(c)
        assert qs.shape == (c.q, c.d) and g.shape == (c.n, c.d) and np.isfinite(qs).all() and np.isfinite(g).all(), case_id(c)
    for rc in ROWS_CASES:
        assert rows_block(rc).shape[0] * rc.n <= 3e5, rc.name


# ------------------------------------------------------------------ GPU: one se_retrieve_topk call through the C ABI

GUARD = 4096
WS_FILL, OUT_FILL = 0xA5, 0x7FC0DEAD


def guarded(nbytes):
    """-> (buffer, view of nbytes 256-byte aligned bytes inside it); everything else holds WS_FILL."""
    import torch
    buf = torch.full((nbytes + 2 * GUARD + 256,), WS_FILL, dtype=torch.uint8, device="cuda")
    start = GUARD + (-(buf.data_ptr() + GUARD)) % 256
    return buf, buf[start:start + nbytes], start


def guard_intact(buf, start, nbytes):
    return bool((buf[:start] == WS_FILL).all()) and bool((buf[start + nbytes:] == WS_FILL).all())


def run_retrieve(c, sehip, want_path=None):
    """One se_retrieve_topk call of a case in test-owned buffers; every assertion of a GPU case.  -> (phases, counters)."""
    import torch
    from sehip import _lib
    qs, g = case_data(c)
    _, (wd, wi) = case_oracle(c)
    assert qs.shape == (c.q, c.d) and g.shape == (c.n, c.d) and wi.shape == (c.q, c.k)
    r = case_plan(c)
    G = PD.place(g, c.layout)
    Q = G if c.pairs == SYM_T else PD.place(qs, c.layout)
    ldg = G.stride(0)
    assert ldg == PD.layout_pitch(c.layout, c.d) and (G.data_ptr() % 16 == 0) == PD.layout_aligned(c.layout)
    sqg = sehip.row_sqnorm(G) if c.metric == EUC else None
    sqq = sqg if c.pairs == SYM_T else (sehip.row_sqnorm(Q) if c.metric == EUC else None)
    need = int(_lib.call("se_retrieve_topk_workspace_bytes", c.q, c.n, c.d, ldg, c.k))
    assert need == r.need, "workspace: library %d bytes, restated %d" % (need, r.need)
    ws_buf, ws, ws_start = guarded(need)
    od_buf = torch.full(((c.q + 2) * c.k,), OUT_FILL, dtype=torch.int32, device="cuda")
    oi_buf = torch.full(((c.q + 2) * c.k,), OUT_FILL, dtype=torch.int32, device="cuda")
    od = od_buf[c.k:(c.q + 1) * c.k].view(torch.float32)
    oi = oi_buf[c.k:(c.q + 1) * c.k]
    kb = (__import__("ctypes").c_int32 * len(c.kb))(*c.kb) if c.kb else None
    sehip.phase_timing(True)
    try:
        _lib.call("se_retrieve_topk", Q, Q.stride(0), G, ldg, sqq, sqg, c.q, c.n, c.d, c.metric, kb, len(c.kb) if c.kb else 0, 0, c.k,
                  od, oi, ws, need)
        torch.cuda.synchronize()
        phases, counters = sehip.phase_timing_read()
    finally:
        sehip.phase_timing(False)
    got_i, got_d = oi.view(c.q, c.k).cpu().numpy(), od.view(c.q, c.k).cpu().numpy()
    bad = np.nonzero((got_i != wi).any(axis=1) | (got_d != wd).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d rows differ from canon.c, first %d" % (case_id(c), len(bad), bad[0])
    assert np.array_equal(got_i, wi) and np.array_equal(got_d, wd)
    # nothing written outside [q, k] of either output, nor outside the workspace
    for buf in (od_buf, oi_buf):
        assert bool((buf[:c.k] == OUT_FILL).all()) and bool((buf[(c.q + 1) * c.k:] == OUT_FILL).all()), case_id(c)
    assert guard_intact(ws_buf, ws_start, need), "%s: bytes written outside the workspace" % case_id(c)
    # the path that ran: only the pre-filter marks phases and reports counters
    path = want_path or c.mode
    if path == PREF:
        assert {"convert", "sample", "threshold", "filter", "refine", "fallback"} <= set(phases), phases
        want = expected_counters(c)
        assert counters is not None and {k: counters[k] for k in want} == want, (case_id(c), counters, want)
    else:
        assert not phases and counters is None, (case_id(c), phases, counters)
    return phases, counters


@pytest.fixture(scope="module")
def sehip():
    import sehip as m
    m.lib()
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("c", SLAB_CASES, ids=[case_id(c) for c in SLAB_CASES])
def test_slab_cases_vs_oracle(sehip, c):
    run_retrieve(c, sehip)


@pytest.mark.gpu
@pytest.mark.parametrize("nk,path", PRODUCT_THRESHOLDS, ids=lambda v: str(v).replace(" ", ""))
def test_product_thresholds_take_the_predicted_path(sehip, nk, path):
    """The product library, no switches, on both sides of each threshold: the phases name the path, the workspace is the restated one."""
    n, k = nk
    c = Case(path, (COS, EUC)[k % 2], ASYM_T, 48, n, 64, k, None, CONTIG, None, 1, ())
    assert case_plan(c).path == path
    run_retrieve(c, sehip, path)


def _child(group, env, timeout):
    e = dict(os.environ, SEHIP_LIB=os.path.join(PKG_DIR, "sehip", "libsehip_tuning.so"), **env)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), group], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=timeout)
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-6000:]
    print("\n" + "\n".join(ln for ln in out.stdout.splitlines() if ln.startswith("CASE")))
    return out.stdout


@pytest.mark.gpu
def test_fp32_fused_cases_in_one_child():
    """SE_TOPK_FUSED=1, SE_TOPK_PREFILTER=0: the 24 pdist_kernel tuples and topk_lists_kernel's widths and edges."""
    out = _child("fp32", {}, 240)
    for c in FP32_CASES:
        assert "CASE %s ok" % case_id(c) in out, case_id(c)


@pytest.mark.gpu
def test_prefilter_cases_in_one_child():
    """SE_TOPK_FUSED=1: tile kernels, refinement tuples, m / list / spill edges -- outputs, guards and counters."""
    out = _child("prefilter", {}, 240)
    for c in PREF_CASES:
        assert "CASE %s ok" % case_id(c) in out, case_id(c)


# ------------------------------------------------------------------ the pre-filter's error bound, depth by depth

ERROR_BOUND_DEPTHS = (1, 16, 17, 32, 33, 64, 65, 96, 112, 113, 127, 128, 129, 256, 257)
ERROR_BOUND_BODY = TK.PROBE + (
    "rng = np.random.default_rng(12)\n"
    "for d in %r:\n"
    "    n, q = 260, 130\n"
    "    base = rng.standard_normal((n, d)).astype(np.float32)\n"
    "    cancel = np.concatenate([base[:, :d // 2], -base[:, :d - d // 2] * (1 + 1e-3 * rng.standard_normal((n, d - d // 2)))], axis=1).astype(np.float32)\n"
    "    worst_bound = worst_a1 = 0.0\n"
    "    for name, g in (('gauss', base), ('cancel', cancel)):\n"
    "        for metric in (0, 1):\n"
    "            gg = ro.canon_normalize_rows(g) if metric == 0 else np.ascontiguousarray(g)\n"
    "            qs = np.ascontiguousarray(gg[rng.permutation(n)[:q]])\n"
    "            dt, eps = probe(qs, gg, metric)\n"
    "            exact = ro.canon_pdist(qs, gg, metric)\n"
    "            err = np.abs(dt.T.astype(np.float64) - exact.astype(np.float64))\n"
    "            assert np.isfinite(eps).all() and (eps > 0).all(), (d, name, metric)\n"
    "            ratio = float((err / eps[:, None].astype(np.float64)).max())\n"
    "            worst_bound = max(worst_bound, ratio)\n"
    "            assert ratio <= 1.0, (d, name, metric, ratio)\n"                      # the design's condition: |d~ - d| <= eps(query), every pair
    "            if metric == 0:\n"
    "                a, b = image(qs), image(gg)\n"
    "                v64 = a @ b.T; s64 = np.abs(a) @ np.abs(b).T\n"
    "                kp = (d + 127) // 128 * 128\n"
    "                a1 = float((np.abs(-dt.T.astype(np.float64) - v64) / ((kp / 16) * 2.0 ** -20 * s64 + 1e-300)).max())\n"
    "                worst_a1 = max(worst_a1, a1)\n"
    "                assert a1 <= 1.0, (d, name, a1)\n"                                    # assumption A1's allowance itself
    "    print('BOUND d=%%d last_steps=%%d: worst |d~ - d| / eps = %%.4f; worst accumulation error / A1 allowance = %%.5f' %% (d, T2.last_steps(d), worst_bound, worst_a1))\n"
) % (ERROR_BOUND_DEPTHS,)


@pytest.mark.gpu
def test_prefilter_error_bound_by_depth():
    """|d~ - d| <= eps(query) for every pair at every last_steps value and on both sides of every 16-column step and chunk edge,
    gaussian and cancellation-heavy operands, both metrics; and the matrix core's accumulation error within what A1 allows."""
    out = TK.run_with_tuning_lib("import test_gpu_topk_matrix as T2\n" + ERROR_BOUND_BODY, timeout=240)
    lines = [ln for ln in out.splitlines() if ln.startswith("BOUND")]
    print("\n" + "\n".join(lines))
    assert len(lines) == len(ERROR_BOUND_DEPTHS)


# ------------------------------------------------------------------ GPU: se_topk_rows

@pytest.mark.gpu
@pytest.mark.parametrize("rc", ROWS_CASES, ids=[rc.name for rc in ROWS_CASES])
def test_topk_rows_cases_vs_oracle(sehip, rc):
    """se_topk_rows of the product library: radix and sample select, every sort width and count edge (the constructed rows), NaN in
    the pitch padding, col_offset, more rows than either persistent grid (laid out and compared on the device)."""
    import torch
    from sehip import _lib
    block = rows_block(rc)
    rows = block.shape[0]
    q = rc.q or rows
    src = torch.arange(q, device="cuda") % rows
    ldp = rc.n + rc.pad
    pd_buf = torch.full((q + 2, ldp), float("nan"), dtype=torch.float32, device="cuda")
    pd_buf[1:q + 1, :rc.n] = torch.from_numpy(block).cuda()[src]
    pd = pd_buf[1:q + 1, :rc.n]
    od_buf = torch.full(((q + 2) * rc.k,), OUT_FILL, dtype=torch.int32, device="cuda")
    oi_buf = torch.full(((q + 2) * rc.k,), OUT_FILL, dtype=torch.int32, device="cuda")
    od, oi = od_buf[rc.k:(q + 1) * rc.k].view(torch.float32), oi_buf[rc.k:(q + 1) * rc.k]
    _lib.call("se_topk_rows", pd, ldp, q, rc.n, rc.col_offset, rc.k, od, oi)
    torch.cuda.synchronize()
    wd, wi = ro.canon_topk_rows(block, rc.k, col_offset=rc.col_offset)
    wd_t, wi_t = torch.from_numpy(wd).cuda()[src], torch.from_numpy(wi).cuda()[src]
    got_d, got_i = od.view(q, rc.k), oi.view(q, rc.k)
    ok = (got_i == wi_t).all(dim=1) & ((got_d == wd_t) | (got_d.isnan() & wd_t.isnan())).all(dim=1)
    assert bool(ok.all()), "%s: row %d (block row %d) differs from canon.c" % (rc.name, int(torch.nonzero(~ok)[0]), int(torch.nonzero(~ok)[0]) % rows)
    if not rc.q:                                        # the small calls also through the host comparator
        assert np.array_equal(got_i.cpu().numpy(), wi) and np.array_equal(got_d.cpu().numpy(), wd, equal_nan=True)
    for buf in (od_buf, oi_buf):
        assert bool((buf[:rc.k] == OUT_FILL).all()) and bool((buf[(q + 1) * rc.k:] == OUT_FILL).all()), rc.name


# ------------------------------------------------------------------ children

def _child_main(group):
    import sehip
    sehip.lib()
    cases = {"fp32": FP32_CASES, "prefilter": PREF_CASES}[group]
    switches = set()
    for c in cases:
        env = case_env(c)
        for name in switches - set(env):
            del os.environ[name]
        os.environ.update(env)
        switches = set(env)
        _, counters = run_retrieve(c, sehip)
        print("CASE %s ok %s" % (case_id(c), counters or ""), flush=True)
    print("CHILD-OK")


if __name__ == "__main__":
    _child_main(sys.argv[1])
