"""Float64 NumPy restatement of the hierarchy-aware classifier losses (se_hxe_fwd / _bwd, se_soft_xent_fwd / _bwd) that does NOT use
the range encoding of ClassHierarchy.hxe_encoding: the probability of a node is the sum of the softmax over its explicit descendant
set, the loss is the weighted sum of -log conditionals along the label's path, the gradient is the closed form.  Also the
ingredients of the derived error bounds of tests/test_gpu_hxe.py, and seeded random trees.

For the instantiation matrix (tests/test_hxe_matrix_host.py, tests/test_gpu_hxe_matrix.py): caterpillar trees whose paths hold every
level count up to the limit, ``range_model`` -- a float64 restatement of the arithmetic include/sehip.h states ON the range encoding,
which can be given one defect at a time -- and the same for the soft labels."""
import numpy as np

U = 2.0 ** -24      # unit round-off of float32


def random_tree(C, seed, internal=None):
    """(ClassHierarchy, classes): a seeded random tree with C leaves (ids 0 .. C - 1) under ``internal`` inner nodes (ids from
    10 ** 6; node 10 ** 6 is the root).  Chains and inner nodes without a class below them occur."""
    from class_hierarchy import ClassHierarchy
    rng = np.random.default_rng(seed)
    internal = max(1, int(internal if internal is not None else max(2, C // 3)))
    base = 10 ** 6
    parents, children = {}, {}
    for i in range(1, internal):
        p = base + int(rng.integers(i // 2, i))                # depth grows like log(i) / log(4 / 3): about 20 at i = 340
        parents[base + i] = [p]
        children.setdefault(p, []).append(base + i)
    for c in range(C):
        p = base + int(rng.integers(0, internal))
        parents[c] = [p]
        children.setdefault(p, []).append(c)
    return ClassHierarchy(parents, children), list(range(C))


def caterpillar_tree(n, extra=0):
    """(ClassHierarchy, classes): a spine of n - 1 inner nodes (ids from 10 ** 6, the first is the root), leaf i under spine node i,
    the last spine node with two leaves, and ``extra`` more leaves directly under the root.  No inner node has one child, so no
    level is dropped: leaf i has i + 1 kept levels (the last two leaves n - 1), the extra leaves 1."""
    from class_hierarchy import ClassHierarchy
    base = 10 ** 6
    parents, children = {}, {}

    def edge(p, c):
        parents[c] = [p]
        children.setdefault(p, []).append(c)
    for i in range(1, n - 1):
        edge(base + i - 1, base + i)
    for i in range(n - 1):
        edge(base + i, i)
    edge(base + n - 2, n - 1)
    for i in range(extra):
        edge(base, n + i)
    return ClassHierarchy(parents, children), list(range(n + extra))


def one_class_tree():
    """(ClassHierarchy, classes): one class under one node -- the only edge adds no class, so the path has no level (h = 0)."""
    from class_hierarchy import ClassHierarchy
    return ClassHierarchy({0: [10]}, {10: [0]}), [0]


class Canon(object):
    """The class tree of ``classes`` in ``hierarchy`` by explicit sets."""

    def __init__(self, hierarchy, classes):
        self.h, self.classes = hierarchy, list(classes)
        self.anc = [set(hierarchy.all_hypernym_depths(c)) for c in self.classes]
        closure = set().union(*self.anc)
        self.roots = [n for n in closure if not hierarchy.parents.get(n)]
        self.forest = len(self.roots) > 1
        self._mask = {}

    def mask(self, node):
        """bool [C]: the classes below ``node`` (None: the virtual top of a forest, every class)."""
        if node not in self._mask:
            self._mask[node] = np.ones(len(self.classes), dtype=bool) if node is None else np.asarray([node in a for a in self.anc])
        return self._mask[node]

    def path(self, c):
        """[a_0 = c, a_1, ..., top] and the number of edges from the top to each of them."""
        nodes = [c]
        while self.h.parents.get(nodes[-1]):
            ps = self.h.parents[nodes[-1]]
            assert len(set(ps)) == 1, "not a tree at %r" % (nodes[-1],)
            nodes.append(ps[0])
        if self.forest:
            nodes.append(None)
        return nodes, [len(nodes) - 1 - i for i in range(len(nodes))]

    def edges(self, c, alpha=0.1, weights=None, float32_weights=True):
        """[(lambda_l, mask of a_l, mask of a_{l+1}, dropped)]: dropped = both cover the same classes (the term is exactly 0)."""
        nodes, depth = self.path(c)
        out = []
        for l in range(len(nodes) - 1):
            lam = float(weights(nodes[l])) if weights is not None else float(np.exp(-alpha * depth[l]))
            if float32_weights:
                lam = float(np.float32(lam))
            lo, hi = self.mask(nodes[l]), self.mask(nodes[l + 1])
            out.append((lam, lo, hi, bool((lo == hi).all())))
        return out

    def hxe(self, z, y, alpha=0.1, weights=None):
        """z [B, C] float64 (the rounded inputs), y [B] -> dict of float64 ``loss`` [B], ``dz`` [B, C] (for w_i = 1), and for the
        bounds: ``scale`` [B] = sum_l lambda_l (|L_l| + |L_{l+1}| + 1) over the kept levels, ``absgrad`` [B, C] = the closed form
        with every term taken positive (lambda_0 included for the label), ``x`` = z - M, ``levels`` [B] kept levels."""
        z = np.asarray(z, dtype=np.float64)
        B, C = z.shape
        loss, dz, scale, absgrad, levels = np.zeros(B), np.zeros((B, C)), np.zeros(B), np.zeros((B, C)), np.zeros(B, dtype=int)
        M = z.max(axis=1, keepdims=True)
        x = z - M
        e = np.exp(x)
        for i in range(B):
            c = int(y[i])
            for lam, lo, hi, dropped in self.edges(self.classes[c], alpha, weights):
                if dropped:
                    continue
                levels[i] += 1
                single = lo.sum() == 1
                S_lo, S_hi = e[i, lo].sum(), e[i, hi].sum()
                L_lo = x[i, c] if single else np.log(S_lo)          # the label's own level: exact
                L_hi = np.log(S_hi)
                loss[i] += lam * (L_hi - L_lo)
                scale[i] += lam * (abs(L_lo) + abs(L_hi) + 1.0)
                up = lam * e[i] * hi / S_hi
                down = lam * lo.astype(np.float64) if single else lam * e[i] * lo / S_lo
                dz[i] += up - down
                absgrad[i] += up + down
        return {"loss": loss, "dz": dz, "scale": scale, "absgrad": absgrad, "x": x, "levels": levels}


def soft(z, y, table):
    """Cross-entropy of softmax(z) against table[y]: float64 loss [B], dz [B, C] (w_i = 1), and for the bounds ``scale`` [B] =
    sum_c Q_c (|M - z_c| + |log S| + 1) and ``absgrad`` = sum(Q) p + Q."""
    z, Q = np.asarray(z, dtype=np.float64), np.asarray(table, dtype=np.float64)[np.asarray(y)]
    M = z.max(axis=1, keepdims=True)
    lS = np.log(np.exp(z - M).sum(axis=1, keepdims=True))
    with np.errstate(invalid="ignore"):
        t = np.where(Q != 0, Q * ((M - z) + lS), 0.0)
    p = np.exp(z - M - lS)
    sq = Q.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):                       # a zero target adds nothing to the scale either, whatever its logit
        scale = np.where(Q != 0, Q * (np.abs(M - z) + np.abs(lS) + 1.0), 0.0).sum(axis=1)
    return {"loss": t.sum(axis=1), "dz": sq * p - Q, "scale": scale, "absgrad": sq * p + Q, "x": z - M}


def log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    M = z.max(axis=1, keepdims=True)
    return z - M - np.log(np.exp(z - M).sum(axis=1, keepdims=True))


def sum_depth(C):
    """Additions on the longest path of the kernels' fixed-order sum over a row of C classes: every thread adds its values in
    order (at most ceil(C / G) + 8 of them: G = 64 threads up to C = 1024, 256 above; 8 for a last, partly filled 16-byte unit), then
    6 butterfly steps across the wave and 2 across the four waves."""
    G = 64 if C <= 1024 else 256
    return -(-C // G) + 8 + 6 + 2


def loss_k(C):
    """k of the loss bound  k * 2^-24 * sum_l lambda_l (|L_l| + |L_{l+1}| + 1)  (tests/test_gpu_hxe.py derives it)."""
    return 13.0 + 2.0 * (np.log(C) + 4.0 + sum_depth(C))


def grad_factor(C, x):
    """Per element: the relative error bound of e_c * H, in units of 2^-24 (tests/test_gpu_hxe.py derives it)."""
    return 2.0 * np.abs(x) + 2.0 * np.log(C) + sum_depth(C) + 20.0


def soft_bounds(C, ref, w=1.0):
    """(loss bound [B], dz bound [B, C]) of the soft-label kernels against ``soft`` (tests/test_gpu_hxe.py derives them)."""
    D = sum_depth(C)
    with np.errstate(invalid="ignore"):
        lb = (D + np.log(C) + 10.0) * U * ref["scale"]
        gb = np.where(ref["absgrad"] == 0, 0.0, U * abs(w) * (2.0 * np.abs(ref["x"]) + 7.0 * np.log(C) + 2.0 * D + 12.0) * ref["absgrad"])
    return lb, gb


MAX_LEVELS, AUX = 32, 34                   # SE_HXE_MAX_LEVELS; floats of aux per row: M, H_0 .. H_32
DEFECTS = ("chunk", "hi", "lev", "lambda_h", "h0_slot", "tail", "label_term")


def range_model(enc, z, y, defect=None, E=1, sentinel=np.nan):
    """The arithmetic of include/sehip.h ON the range encoding ``enc`` (hxe_encoding's dict), in float64: dict of ``loss`` [B],
    ``dz`` [B, C] (w_i = 1) and ``aux`` [B, 34] (M, H_0 .. H_h, then ``sentinel``).  Labels are clamped as the kernels clamp them.

    ``defect``: one way a kernel could be wrong -- "chunk": the levels from 24 on skipped in the sums and in the backward's count;
    "hi": ``<=`` for ``<`` at a range's hi; "lev": lev(c) one too large in the backward; "lambda_h": 0.5 where lambda_h = 0 is read;
    "h0_slot": the label's H_0 read from aux slot 2 (H_1 -- the same value unless h = 0, where the slot is unused); "tail": the
    classes of a part-filled last unit of ``E`` dropped from the sums and never stored (``sentinel`` stays); "label_term":
    lambda_0 e_y / S_1 in the place of the constant lambda_0."""
    assert defect is None or defect in DEFECTS
    z = np.asarray(z, dtype=np.float64)
    B, C = z.shape
    pos, off = np.asarray(enc["pos"], dtype=np.int64), np.asarray(enc["path_off"], dtype=np.int64)
    loss, dz, aux = np.zeros(B), np.zeros((B, C)), np.full((B, AUX), sentinel, dtype=np.float64)
    live = np.ones(C, dtype=bool)
    if defect == "tail" and E > 1:
        live[C // E * E:] = False
    for i in range(B):
        c = min(max(int(y[i]), 0), C - 1)
        a, b = int(off[c]), int(off[c + 1])
        h = b - a
        lo, hi, lam = enc["lvl_lo"][a:b].astype(np.int64), enc["lvl_hi"][a:b].astype(np.int64), enc["lvl_w"][a:b].astype(np.float64)
        seen = min(h, 24) if defect == "chunk" else h
        M = z[i].max()
        x = z[i] - M
        e = np.exp(x)
        inside = [(pos >= lo[l]) & ((pos <= hi[l]) if defect == "hi" else (pos < hi[l])) for l in range(h)]
        S = np.asarray([e[inside[l] & live].sum() if l < seen else 0.0 for l in range(h)])
        L = [x[c]]
        with np.errstate(divide="ignore"):
            for l in range(h):
                L.append(max(np.log(S[l]), x[c]))
        for l in range(h):
            if L[l + 1] != L[l]:
                loss[i] += lam[l] * (L[l + 1] - L[l])
        nxt = np.append(lam[1:], 0.5 if defect == "lambda_h" else 0.0) if h else lam
        g = np.asarray([(lam[l] - nxt[l]) / S[l] if S[l] != 0 else 0.0 for l in range(h)])
        H = np.zeros(MAX_LEVELS + 3)                               # H[k] = H_k; 0 past h, as the lanes past h hold
        for k in range(h, 0, -1):
            H[k] = H[k + 1] + g[k - 1]
        H[0] = H[1]
        aux[i, 0] = M
        aux[i, 1:2 + h] = H[:1 + h]
        out = np.zeros(C, dtype=np.int64)
        for l in range(seen):
            out += ~inside[l]
        d = e * H[np.minimum(1 + out + (1 if defect == "lev" else 0), MAX_LEVELS + 2)]
        H0 = aux[i, 2] if defect == "h0_slot" else H[0]
        lam0 = lam[0] if h else 0.0
        d[c] = e[c] * H0 - (lam0 * e[c] / S[0] if defect == "label_term" and h and S[0] != 0 else lam0)
        d[~live] = sentinel
        dz[i] = d
    return {"loss": loss, "dz": dz, "aux": aux}


def soft_model(z, y, rows, defect=None):
    """The soft-label arithmetic of include/sehip.h in float64 on ``rows`` [B, C] (the table rows of the labels): ``loss``, ``dz``.
    ``defect`` "zero_inf": a class with target 0 contributes 0 * ((M - z_c) + log S) -- NaN where z_c = -inf."""
    z, Q = np.asarray(z, dtype=np.float64), np.asarray(rows, dtype=np.float64)
    M = z.max(axis=1, keepdims=True)
    lS = np.log(np.exp(z - M).sum(axis=1, keepdims=True))
    with np.errstate(invalid="ignore"):
        t = Q * (M - z) if defect == "zero_inf" else np.where(Q != 0, Q * (M - z), 0.0)
    sq = Q.sum(axis=1, keepdims=True)
    return {"loss": t.sum(axis=1) + sq[:, 0] * lS[:, 0], "dz": sq * np.exp(-((M - z) + lS)) - Q}


def synthetic_rows(C, B, seed):
    """float32 [B, C] soft-label rows: non-negative, not normalised, about a quarter of the entries exactly 0."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.0, 2.0 / C, size=(B, C)).astype(np.float32)
    q[rng.random((B, C)) < 0.25] = 0.0
    return q
