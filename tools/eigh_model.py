"""NumPy model of se_eigh_f64 (csrc/eigh.hip): two-sided block Jacobi with the round-robin ordering of sehip.eigh_schedule.

The model makes the kernel's decisions in the kernel's order -- blocks of EB = 32 columns, the matrix padded with exact zeros to an
even number of blocks, one sweep = nb - 1 rounds of nb / 2 disjoint block pairs, every pair's 64 x 64 sub-block diagonalised by
cyclic Jacobi in the same round-robin order over its 64 indices with the same skip rule, the accumulated rotation J applied as
A <- J^T A J, V <- V J, the off-norm summed directly, the same stopping rule -- with NumPy's products in the place of the MFMA
tiles.  It exists to fix the tolerance of tests/test_gpu_eigh.py without looking at the device: for every test matrix it prints

    eigenvalues     max |sort(w) - lam_ref|        / (n eps s)
    residual        max |A V - V diag(w)|          / (n eps s)
    orthogonality   max |V^T V - I|                / (n eps)

with lam_ref = np.linalg.eigh(A)[0], s = max |lam_ref|, eps = 2^-52.  The test's constant c is 4 x the worst of these ratios
(the margin covers the MFMA summation order and extra sweeps).

    python tools/eigh_model.py            # every matrix of the GPU test, the ratios and the constant
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "semantic-embeddings_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

EB = 32                     # block width (EIGH_B)
P = 2 * EB                  # pair width
MAX_INNER = 12              # inner sweeps of one pair at most (EIGH_MAX_INNER)
SKIP_REL = 2.0 ** -54       # a rotation is skipped when |a_pq| <= SKIP_REL sqrt(|a_pp a_qq|) ...
SKIP_ABS = 2.0 ** -54       # ... or <= SKIP_ABS |A|_F / n, or a_pq == 0
EPS = 2.0 ** -52


def schedule(nb):
    from sehip.ops import eigh_schedule
    return eigh_schedule(nb)


def _needs(s, p, q, delta):
    apq = s[p, q]
    return (apq != 0.0) & (np.abs(apq) > np.maximum(SKIP_REL * np.sqrt(np.abs(s[p, p] * s[q, q])), delta))


def pair_jacobi(s, delta):
    """Cyclic Jacobi on the P x P block ``s`` (in place); returns (J, rotated)."""
    m = s.shape[0]
    j = np.eye(m)
    rounds = [(np.array([min(a, b) for a, b in r]), np.array([max(a, b) for a, b in r])) for r in schedule(m)]
    iu = np.triu_indices(m, 1)
    rotated = False
    for _ in range(MAX_INNER):
        if not _needs(s, iu[0], iu[1], delta).any():
            break
        rotated = True
        for p, q in rounds:
            app, aqq, apq = s[p, p], s[q, q], s[p, q]
            go = _needs(s, p, q, delta)
            with np.errstate(all="ignore"):
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(1.0 + theta * theta))
            c = 1.0 / np.sqrt(1.0 + t * t)
            sn = t * c
            c, sn = np.where(go, c, 1.0), np.where(go, sn, 0.0)
            for mat in (s, j):                                  # columns: (p, q) <- (c p - s q, s p + c q)
                cp, cq = mat[:, p].copy(), mat[:, q].copy()
                mat[:, p], mat[:, q] = c * cp - sn * cq, sn * cp + c * cq
            rp, rq = s[p, :].copy(), s[q, :].copy()             # rows of s alike
            s[p, :], s[q, :] = c[:, None] * rp - sn[:, None] * rq, sn[:, None] * rp + c[:, None] * rq
            s[p[go], q[go]] = 0.0
            s[q[go], p[go]] = 0.0
    return j, rotated


def eigh_model(a, max_sweeps=30):
    """(w ascending, v, sweeps used or -1 not converged / -2 non-finite) of the symmetric matrix ``a``."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    nb = 2 * max((n + P - 1) // P, 1)
    npad = nb * EB
    ap = np.zeros((npad, npad))
    ap[:n, :n] = a
    v = np.eye(npad)
    fro2 = float((ap * ap).sum())
    if not np.isfinite(fro2):
        return np.full(n, np.nan), np.full((n, n), np.nan), -2

    def off2():
        sq = ap * ap
        np.fill_diagonal(sq, 0.0)
        return float(sq.sum())
    tol2 = (n * 2.0 ** -106) * fro2                             # off <= sqrt(n) 2^-53 |A|_F
    delta = SKIP_ABS * np.sqrt(fro2) / max(n, 1)
    info = -1
    for sweep in range(max_sweeps + 1):
        if off2() <= tol2:
            info = sweep
            break
        if sweep == max_sweeps:
            break
        for rnd in schedule(nb):
            for bp, bq in rnd:
                bp, bq = min(bp, bq), max(bp, bq)
                idx = np.r_[bp * EB:(bp + 1) * EB, bq * EB:(bq + 1) * EB]
                s = ap[np.ix_(idx, idx)].copy()
                j, rotated = pair_jacobi(s, delta)
                if not rotated:
                    continue
                ap[:, idx] = ap[:, idx] @ j
                ap[idx, :] = j.T @ ap[idx, :]
                ap[np.ix_(idx, idx)] = s
                v[:, idx] = v[:, idx] @ j
    lam = np.diag(ap)[:n]
    order = np.argsort(lam, kind="stable")
    return lam[order], v[:n, :n][:, order], info


def test_matrices():
    """{name: matrix} -- the matrices of tests/test_gpu_eigh.py."""
    from test_gpu_eigh import matrices
    return matrices()


def ratios(a, w, v):
    n = a.shape[0]
    lam = np.linalg.eigh(a)[0]
    s = max(float(np.abs(lam).max()), np.finfo(np.float64).tiny)
    ne = n * EPS
    return (np.abs(np.sort(w) - lam).max() / (ne * s), np.abs(a @ v - v * w[None, :]).max() / (ne * s),
            np.abs(v.T @ v - np.eye(n)).max() / ne)


if __name__ == "__main__":
    worst = 0.0
    for name, a in test_matrices().items():
        w, v, info = eigh_model(a)
        r = ratios(a, w, v)
        worst = max(worst, *r)
        print("%-28s n=%4d sweeps=%2d  eigenvalues %7.3f  residual %7.3f  orthogonality %7.3f   (x n eps)" % ((name, a.shape[0], info) + r))
    print("worst ratio %.3f -> c = 4 x worst = %.1f" % (worst, 4 * worst))
