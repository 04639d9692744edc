"""Float64 NumPy restatement of the hierarchy-aware classifier losses (se_hxe_fwd / _bwd, se_soft_xent_fwd / _bwd) that does NOT use
the range encoding of ClassHierarchy.hxe_encoding: the probability of a node is the sum of the softmax over its explicit descendant
set, the loss is the weighted sum of -log conditionals along the label's path, the gradient is the closed form.  Also the
ingredients of the derived error bounds of tests/test_gpu_hxe.py, and seeded random trees."""
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
    return {"loss": t.sum(axis=1), "dz": sq * p - Q, "scale": (Q * (np.abs(M - z) + np.abs(lS) + 1.0)).sum(axis=1),
            "absgrad": sq * p + Q, "x": z - M}


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
