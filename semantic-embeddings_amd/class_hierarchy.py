"""Class taxonomy + hierarchical retrieval metrics: the consumer of the rankings produced by
``evaluate_retrieval.pairwise_retrieval``.

Same public surface as the reference's ``class_hierarchy.ClassHierarchy``
(reference: class_hierarchy.py:7-367 -- ``from_file``/``save``, ``lcs``, ``wup_similarity``,
``lcs_height``, ``depth``, ``heights``/``max_height``, ``hierarchical_precision`` ...), but built
differently: node properties are computed once by memoised graph walks, and
``hierarchical_precision`` works on NumPy look-up tables (class x class similarity matrices gathered
along the ranking + prefix sums) instead of per-element Python dictionary look-ups.  The metric
definitions (Deng et al., CVPR 2011 hierarchical precision; area under the HP@k curve; average
precision) and every corner of the reference's bookkeeping are kept, so the numbers agree with the
reference to float64 round-off (tests/test_class_hierarchy.py checks against values produced by the
imported reference).
"""
import os
import types
import warnings

import numpy as np

_trapz = getattr(np, "trapezoid", None) or np.trapz

HXE_MAX_LEVELS = 32     # levels of one class's path in ClassHierarchy.hxe_encoding (SE_HXE_MAX_LEVELS of include/sehip.h)


class _VirtualTop(object):
    """The node ``hxe_encoding`` puts above the roots of a forest."""

    def __repr__(self):
        return '<virtual top>'


_VIRTUAL_TOP = _VirtualTop()


class ClassHierarchy(object):
    """A DAG of classes given as parent->children / child->parents adjacency dictionaries."""

    def __init__(self, parents, children):
        self.parents = parents
        self.children = children
        self.nodes = set(parents) | set(children)
        self._depth = {False: {}, True: {}}
        self._anc_depth = {False: {}, True: {}}
        self._anc_dist = {}
        self._lcs_cache = {}
        self._wup_cache = {}
        self._luts = {}
        self.heights = {}
        for node in self.nodes:
            self._height(node)
        self.max_height = max(self.heights.values())

    # ------------------------------------------------------------------ construction / IO

    @classmethod
    def from_file(cls, rel_file, is_a_relations=False, id_type=str):
        """Reads "<parent> <child>" lines ("<child> <parent>" with ``is_a_relations``)."""
        parents, children = {}, {}
        with open(rel_file) as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                first, second = (id_type(tok) for tok in line.split(maxsplit=1))
                parent, child = (second, first) if is_a_relations else (first, second)
                parents.setdefault(child, []).append(parent)
                children.setdefault(parent, []).append(child)
        return cls(parents, children)

    def save(self, filename, is_a_relations=False):
        """Writes the edges back in the format ``from_file`` reads."""
        with open(filename, 'w') as f:
            if is_a_relations:
                f.writelines('{} {}\n'.format(c, p) for c, ps in self.parents.items() for p in ps)
            else:
                f.writelines('{} {}\n'.format(p, c) for p, cs in self.children.items() for c in cs)

    # ------------------------------------------------------------------ node properties

    def _height(self, node):
        """Longest downward path to a leaf (leaves: 0)."""
        h = self.heights.get(node)
        if h is None:
            kids = self.children.get(node, ())
            h = 1 + max((self._height(k) for k in kids), default=-1) if node in self.children else 0
            self.heights[node] = h
        return h

    def is_tree(self):
        return all(len(ps) <= 1 for ps in self.parents.values())

    def depth(self, id, use_min_depth=False):
        """Roots have depth 1; otherwise 1 + max (or min) over the parents' depths."""
        memo = self._depth[use_min_depth]
        if id not in memo:
            ps = self.parents.get(id) or []
            if not ps:
                memo[id] = 1
            else:
                pick = min if use_min_depth else max
                memo[id] = 1 + pick(self.depth(p, use_min_depth) for p in ps)
        return memo[id]

    def all_hypernym_depths(self, id, use_min_depth=False):
        """{ancestor (incl. id): depth of that ancestor}."""
        memo = self._anc_depth[use_min_depth]
        if id not in memo:
            out = {}
            for p in self.parents.get(id) or []:
                out.update(self.all_hypernym_depths(p, use_min_depth))
            out[id] = self.depth(id, use_min_depth)
            memo[id] = out
        return memo[id]

    def all_hypernym_distances(self, id):
        """{ancestor (incl. id): fewest upward edges from id}."""
        if id not in self._anc_dist:
            out = {id: 0}
            for p in self.parents.get(id, ()):
                for anc, dist in self.all_hypernym_distances(p).items():
                    if dist + 1 < out.get(anc, float('inf')):
                        out[anc] = dist + 1
            self._anc_dist[id] = out
        return self._anc_dist[id]

    def root_paths(self, id):
        """Every path from a direct parent of ``id`` up to a root."""
        paths = []
        for p in self.parents.get(id, ()):
            above = self.root_paths(p)
            paths.extend([[p] + tail for tail in above] if above else [[p]])
        return paths

    # ------------------------------------------------------------------ pairwise class relations

    def lcs(self, a, b, use_min_depth=False):
        """Deepest common ancestor (``None`` if there is none).  Among equally deep candidates --
        only possible in non-tree hierarchies, where the reference's pick is arbitrary -- the one
        with the smallest height, then the smallest repr, is chosen deterministically."""
        key = (a, b)
        if key not in self._lcs_cache:
            da = self.all_hypernym_depths(a, use_min_depth)
            common = da.keys() & self.all_hypernym_depths(b, use_min_depth).keys()
            best = None
            if common:
                top = max(da[h] for h in common)
                best = min((h for h in common if da[h] == top), key=lambda h: (self.heights[h], repr(h)))
            self._lcs_cache[(a, b)] = self._lcs_cache[(b, a)] = best
        return self._lcs_cache[key]

    def shortest_path_length(self, a, b):
        da, db = self.all_hypernym_distances(a), self.all_hypernym_distances(b)
        return min((da[h] + db[h] for h in da.keys() & db.keys()), default=None)

    def wup_similarity(self, a, b):
        """Wu-Palmer: 2 depth(lcs) / (depth_via_lcs(a) + depth_via_lcs(b))."""
        key = (a, b)
        if key not in self._wup_cache:
            anc = self.lcs(a, b)
            ds = self.depth(anc)
            d1 = ds + self.shortest_path_length(a, anc)
            d2 = ds + self.shortest_path_length(b, anc)
            self._wup_cache[(a, b)] = self._wup_cache[(b, a)] = (2.0 * ds) / (d1 + d2)
        return self._wup_cache[key]

    def lcs_height(self, a, b):
        """height(lcs(a, b)) / height of the hierarchy (a dissimilarity in [0, 1])."""
        return self.heights[self.lcs(a, b)] / self.max_height

    def similarity_tables(self, classes):
        """(WUP, 1 - LCS height) as float64 [C, C] matrices over ``classes`` (cached)."""
        key = tuple(classes)
        if key not in self._luts:
            c = len(key)
            wup = np.empty((c, c))
            lcs = np.empty((c, c))
            for i, a in enumerate(key):
                for j in range(i, c):
                    b = key[j]
                    wup[i, j] = wup[j, i] = self.wup_similarity(a, b)
                    lcs[i, j] = lcs[j, i] = 1.0 - np.array(self.heights[self.lcs(a, b)]) / self.max_height
            self._luts[key] = (wup, lcs)
        return self._luts[key]

    def pair_table_encoding(self, classes):
        """What ``se_class_pair_tables`` reads, built in time linear in the size of the hierarchy (no pairwise loop).

        Every node of the ancestor closure of ``classes`` gets a preference rank: depth descending, height ascending, repr
        ascending -- the order in which ``lcs`` picks among common ancestors -- so that ``lcs(a, b)`` is the common ancestor of
        smallest rank.  Per class (CSR): the ranks of its ancestors (itself included), ascending, and ``shortest_path_length``
        to each (in a DAG the path may pass through a higher common ancestor, so it is not always the upward distance).
        Returns a dict of int32 arrays ``off`` [C + 1], ``rank`` / ``spl`` [nnz], ``depth`` / ``height`` [R] (per rank), the
        ``nodes`` in rank order, ``max_anc`` (longest list) and ``max_height``."""
        key = tuple(classes)
        anc = [self.all_hypernym_depths(c) for c in key]
        nodes = sorted(set().union(*anc), key=lambda h: (-self.depth(h), self.heights[h], repr(h)))
        pos = {h: r for r, h in enumerate(nodes)}
        off = np.zeros(len(key) + 1, dtype=np.int32)
        ranks, spls = [], []
        for i, (c, a) in enumerate(zip(key, anc)):
            rs = sorted(pos[h] for h in a)
            ranks.extend(rs)
            spls.extend(self.shortest_path_length(c, nodes[r]) for r in rs)
            off[i + 1] = len(ranks)
        return {'off': off, 'rank': np.asarray(ranks, dtype=np.int32), 'spl': np.asarray(spls, dtype=np.int32),
                'depth': np.asarray([self.depth(h) for h in nodes], dtype=np.int32),
                'height': np.asarray([self.heights[h] for h in nodes], dtype=np.int32), 'nodes': nodes,
                'max_anc': int(np.diff(off).max()) if len(key) else 1, 'max_height': self.max_height}

    def similarity_tables_device(self, classes, diag_one=False, distance=False, want_wup=True, want_lcs=True, device=None):
        """``similarity_tables(classes)`` as float64 [C, C] device tensors, bitwise (``se_class_pair_tables``): (wup, lcs), an
        unrequested table is None.  ``diag_one``: lcs diagonal 1 (compute_class_embedding.py's convention) instead of
        1 - height(c) / H; ``distance``: the lcs table holds the LCS height h / H instead of 1 - h / H.  Raises KeyError naming
        the first pair of classes without a common ancestor."""
        import torch
        import sehip
        key = tuple(classes)
        enc = self.pair_table_encoding(key)
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        ints = {k: torch.from_numpy(enc[k]).to(dev) for k in ('off', 'rank', 'spl', 'depth', 'height')}
        wup, lcs, missing = sehip.class_pair_tables(ints['off'], ints['rank'], ints['spl'], ints['depth'], ints['height'],
                                                    enc['max_anc'], enc['max_height'], diag_one=diag_one, distance=distance,
                                                    want_wup=want_wup, want_lcs=want_lcs)
        miss = int(missing.item())
        if miss >= 0:
            raise KeyError('classes {!r} and {!r} have no common ancestor'.format(key[miss // len(key)], key[miss % len(key)]))
        return wup, lcs

    # ------------------------------------------------------------------ hierarchy-aware classifier losses

    def _class_tree(self, classes):
        """The sub-hierarchy spanned by ``classes`` (their ancestor closure) as a tree whose leaves are the classes:
        ``(top, parent, kids, d, rng)`` -- the top node (``_VIRTUAL_TOP`` above several roots), node -> parent, node -> children in
        sorted order, node -> number of edges from the top, node -> ``(lo, hi)`` range of leaf positions in depth-first order.
        ``ValueError`` naming the node: an unknown or repeated class, a node with several parents, a class above another class."""
        key = list(classes)
        cls_set = set()
        for c in key:
            if c not in self.nodes:
                raise ValueError('class {!r} is unknown to the hierarchy'.format(c))
            if c in cls_set:
                raise ValueError('class {!r} is listed twice'.format(c))
            cls_set.add(c)
        parent, kids = {}, {}
        for c in key:
            node = c
            while node not in parent:
                ps = self.parents.get(node) or []
                if len(set(ps)) > 1:
                    raise ValueError('the hierarchy spanned by the classes is not a tree: node {!r} has {} parents'.format(node, len(set(ps))))
                parent[node] = ps[0] if ps else None
                if not ps:
                    break
                kids.setdefault(ps[0], set()).add(node)
                node = ps[0]
                if node in cls_set:
                    raise ValueError('class {!r} is an ancestor of class {!r}'.format(node, c))
        for c in key:       # (a class reached from below after its own walk)
            if c in kids:
                raise ValueError('class {!r} is an ancestor of another class'.format(c))
        roots = [n for n, p in parent.items() if p is None]
        if len(roots) > 1:
            top = _VIRTUAL_TOP
            kids[top] = set(roots)
            for r in roots:
                parent[r] = top
            parent[top] = None
        else:
            top = roots[0]

        def ordered(nodes):
            try:
                return sorted(nodes)
            except TypeError:
                return sorted(nodes, key=repr)
        kids = {n: ordered(k) for n, k in kids.items()}
        d, rng, nleaf = {top: 0}, {}, 0
        stack = [(top, 0)]
        while stack:        # depth-first, children in sorted order; a node's range closes when its last child's has
            node, i = stack.pop()
            ch = kids.get(node, ())
            if i == 0 and not ch:
                rng[node] = (nleaf, nleaf + 1)
                nleaf += 1
            elif i < len(ch):
                stack.append((node, i + 1))
                d[ch[i]] = d[node] + 1
                stack.append((ch[i], 0))
            else:
                rng[node] = (rng[ch[0]][0], rng[ch[-1]][1])
        return top, parent, kids, d, rng

    def hxe_encoding(self, classes, alpha=0.1, weights=None):
        """What ``se_hxe_fwd`` / ``se_hxe_bwd`` read (``sehip.hierarchical_cross_entropy``): the class tree as position ranges.

        The classes are the leaves of the sub-hierarchy they span.  In a depth-first order of that tree (children visited in sorted
        order, so the encoding is reproducible) the classes below any node are one range of positions.  Returns a dict of
        ``pos`` int32 [C] (position of class ``c``: a permutation of 0 .. C - 1), ``path_off`` int32 [C + 1], ``lvl_lo`` / ``lvl_hi``
        int32 [nnz], ``lvl_w`` float32 [nnz] and ``max_levels`` (the longest path).  Entries ``path_off[y] .. path_off[y + 1]`` are
        the levels ``l = 0 .. h_y - 1`` of class ``y`` walking up, ``a_0 = y, a_1, ..., a_h = top``: entry ``l`` stands for the edge
        ``a_l -> a_{l+1}`` and holds the range ``[lo, hi)`` of the PARENT ``a_{l+1}`` and the weight ``lambda_l``; the last range is
        ``[0, C)``.  An edge whose parent covers the same classes as its child is dropped (its conditional probability is 1, its
        term 0), so the ranges of a path grow strictly; more than 32 remaining levels raise ``ValueError``.

        OUR weight rule: ``lambda_l = exp(-alpha * d(a_l))`` with ``d(v)`` the number of edges from the top to ``v`` in the hierarchy
        as given (before edges are dropped): the edge below the top weighs ``exp(-alpha)``, deeper edges less, and nothing is
        normalised.  Several roots get a virtual top at ``d = 0`` (the roots then have ``d = 1``).  ``weights``, a callable
        ``node -> float`` evaluated at ``a_l``, replaces the rule -- to restate another convention; published implementations differ
        (on normalisation among other things) and no bit parity with any of them is claimed.

        ``ValueError`` naming the node: the spanned sub-hierarchy is not a tree (DAG hierarchies are refused, not mis-scored), a
        class is an ancestor of another class, a class is unknown to the hierarchy."""
        key = list(classes)
        tree = self._class_tree(key)
        d, rng = tree[3], tree[4]
        pos = np.asarray([rng[c][0] for c in key], dtype=np.int32)
        path_off = np.zeros(len(key) + 1, dtype=np.int32)
        lo, hi, w = [], [], []
        for i, edges in enumerate(self._kept_edges(key, tree)):
            for node, up in edges:
                lo.append(rng[up][0])
                hi.append(rng[up][1])
                w.append(float(weights(node)) if weights is not None else float(np.exp(-float(alpha) * d[node])))
            path_off[i + 1] = len(lo)
        return {'pos': pos, 'path_off': path_off, 'lvl_lo': np.asarray(lo, dtype=np.int32), 'lvl_hi': np.asarray(hi, dtype=np.int32),
                'lvl_w': np.asarray(w, dtype=np.float32), 'max_levels': int(np.diff(path_off).max()) if len(key) else 0}

    @staticmethod
    def _kept_edges(key, tree):
        """Per class of ``key``, walking up the ``tree`` of ``_class_tree``: the edges ``(node, parent)`` whose parent covers more
        classes than the node -- the levels of the range encodings.  More than ``HXE_MAX_LEVELS`` of them raise ``ValueError``."""
        top, parent, rng = tree[0], tree[1], tree[4]
        for c in key:
            edges, node = [], c
            while node != top:
                up = parent[node]
                if rng[up] != rng[node]:
                    edges.append((node, up))
                node = up
            if len(edges) > HXE_MAX_LEVELS:
                raise ValueError('class {!r} has {} levels above it, more than the {} a path may have'.format(c, len(edges), HXE_MAX_LEVELS))
            yield edges

    def tree_risk_encoding(self, classes):
        """What ``se_tree_risk_topk`` reads (``sehip.tree_risk_topk``, ``mistakes.crm_classification``): the position ranges of
        ``hxe_encoding`` with the HEIGHT of every range's node in place of the weights.

        Returns a dict of ``pos``, ``path_off``, ``lvl_lo``, ``lvl_hi`` (as ``hxe_encoding`` builds them), ``lvl_h`` int32 [nnz],
        ``own_h`` int32 [C], ``max_levels`` and ``max_height``.  ``lvl_h[e]`` is ``heights`` of the DEEPEST node that covers the range
        of entry ``e``: walking up from class ``k``, that node is ``lcs(k, j)`` for every class ``j`` the range adds, because ``lcs``
        prefers depth (nodes above it with the same range are never a lowest common subsumer).  ``own_h[k]`` is the height of class
        ``k`` itself, ``heights[lcs(k, k)]``.

        ``ValueError``: whatever ``hxe_encoding`` refuses (a DAG, a class above a class, an unknown class), and a forest -- classes
        under different roots have no common subsumer, so their risk has no value."""
        key = list(classes)
        tree = self._class_tree(key)
        if tree[0] is _VIRTUAL_TOP:
            raise ValueError('the classes span a forest ({} roots): classes under different roots have no common subsumer'
                             .format(len(tree[2][_VIRTUAL_TOP])))
        rng = tree[4]
        path_off = np.zeros(len(key) + 1, dtype=np.int32)
        lo, hi, h = [], [], []
        for i, edges in enumerate(self._kept_edges(key, tree)):
            for _, up in edges:
                lo.append(rng[up][0])
                hi.append(rng[up][1])
                h.append(self.heights[up])
            path_off[i + 1] = len(lo)
        return {'pos': np.asarray([rng[c][0] for c in key], dtype=np.int32), 'path_off': path_off,
                'lvl_lo': np.asarray(lo, dtype=np.int32), 'lvl_hi': np.asarray(hi, dtype=np.int32), 'lvl_h': np.asarray(h, dtype=np.int32),
                'own_h': np.asarray([self.heights[c] for c in key], dtype=np.int32),
                'max_levels': int(np.diff(path_off).max()) if len(key) else 0, 'max_height': int(self.max_height)}

    def height_table(self, classes, device=None, tables=None):
        """int32 [C, C] device tensor of ``heights[lcs(a, b)]`` in levels -- the metric gathers of ``mistakes.mistake_metrics`` and
        the dense path of ``mistakes.crm_classification``.  From ``similarity_tables_device(distance=True, want_wup=False)``, which
        holds ``h / max_height`` in float64, as ``rint(table * max_height)``; nothing may move by more than 1e-9.  Works on a DAG.
        ``tables`` (tests): a stand-in for ``similarity_tables_device``."""
        import torch
        make = tables if tables is not None else self.similarity_tables_device
        _, lcs = make(classes, distance=True, want_wup=False, device=device)
        scaled = lcs * float(self.max_height)
        table = torch.round(scaled)
        assert float((scaled - table).abs().max()) <= 1e-9, 'an LCS height is no whole number of levels'
        return table.to(torch.int32)

    def soft_label_table(self, classes, beta):
        """float32 [C, C] targets of ``sehip.soft_label_cross_entropy``: row ``y`` is ``softmax_c(-beta * d(y, c))`` with
        ``d(y, c) = lcs_height(y, c)`` = height of the lowest common subsumer / height of the hierarchy, 1 minus the LCS_HEIGHT
        similarity of the retrieval metrics.  Computed in float64 and rounded once.  (Where the classes span a tree the heights
        are read off the tree's position ranges, C path walks instead of C * C ``lcs`` calls; the values are the same.)"""
        key = list(classes)
        C = len(key)
        h = np.empty((C, C), dtype=np.float64)
        try:
            top, parent, _, _, rng = self._class_tree(key)
        except ValueError:
            top = None
        if top is not None and top is not _VIRTUAL_TOP:
            pos = np.asarray([rng[c][0] for c in key])
            for i, c in enumerate(key):
                path, node = [], c
                while node is not None:
                    path.append(node)
                    node = parent[node]
                row = np.empty(C, dtype=np.float64)
                for node in reversed(path):     # from the top down: the deepest node above both classes writes last
                    row[rng[node][0]:rng[node][1]] = self.heights[node]
                h[i] = row[pos]
        else:
            for i, a in enumerate(key):
                for j in range(i, C):
                    h[i, j] = h[j, i] = self.heights[self.lcs(a, key[j])]
        logit = -float(beta) * (h / self.max_height)
        e = np.exp(logit - logit.max(axis=1, keepdims=True))
        return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)

    # ------------------------------------------------------------------ retrieval metrics

    def hierarchical_precision(self, retrieved, labels, ks=[1, 10, 50, 100], compute_ahp=False, compute_ap=False,
                               ignore_qids=True, all_ids=None):
        """Hierarchical precision@k, area under that curve (AHP / AHP@K) and AP per query + means.

        Arguments and return value as in the reference (class_hierarchy.py:211-316):
        ``retrieved`` maps query id -> ranked id list (dict or generator of pairs), ``labels`` maps
        image id -> class label; returns ``(means, per_query)`` with metric names ``"P@K (WUP)"``,
        ``"P@K (LCS_HEIGHT)"``, ``"AHP[@K] (...)"`` and ``"AP"``.

        Bookkeeping kept from the reference: the best-possible cumulative similarity of a query
        class is taken from the FIRST query of that class (full list, query included); removing the
        query shifts that curve left at the query's rank and subtracts its self-similarity of 1;
        ids missing from a ranking are appended in ``all_ids`` order."""
        ks = [ks] if isinstance(ks, int) else list(ks)
        kmax = max(ks)
        ahp_clip = None if isinstance(compute_ahp, bool) else int(compute_ahp)
        if ahp_clip is not None:
            kmax = max(kmax, ahp_clip)
        full_lists = compute_ahp is True

        prec = {n: {} for n in _metric_columns(ks, compute_ahp, compute_ap)}
        ahp_names = [n for n in prec if n.startswith('AHP')]

        # label -> row/column index of the similarity tables
        get_label = labels.__getitem__
        label_of = {}
        best_cum = {}
        class_list, class_pos = [], {}

        def cls_index(lbl):
            if lbl not in class_pos:
                class_pos[lbl] = len(class_list)
                class_list.append(lbl)
            return class_pos[lbl]

        lut_cache = {'n': -1, 'wup': None, 'lcs': None}

        def tables():
            if lut_cache['n'] != len(class_list):
                lut_cache['wup'], lut_cache['lcs'] = self.similarity_tables(class_list)
                lut_cache['n'] = len(class_list)
            return lut_cache['wup'], lut_cache['lcs']

        items = retrieved if isinstance(retrieved, types.GeneratorType) else retrieved.items()
        for qid, ret in items:
            lbl = get_label(qid)
            if all_ids and (len(ret) < len(all_ids)):
                seen = set(ret)
                ret = list(ret) + [i for i in all_ids if i not in seen]
            need_full = full_lists or (lbl not in best_cum)
            head = ret if need_full else ret[:kmax + 1]
            cols = np.fromiter((cls_index(label_of.setdefault(r, get_label(r)) if r in label_of else
                                          label_of.setdefault(r, get_label(r))) for r in head), dtype=np.int64, count=len(head))
            qi = cls_index(lbl)
            wup_t, lcs_t = tables()
            wup = wup_t[qi, cols]
            lcs = lcs_t[qi, cols]
            if lbl not in best_cum:
                best_cum[lbl] = (np.cumsum(np.sort(wup)[::-1]), np.cumsum(np.sort(lcs)[::-1]))
            cum_best_wup, cum_best_lcs = best_cum[lbl]

            q_pos = None
            if ignore_qids:
                try:
                    q_pos = ret.index(qid)
                except ValueError:
                    q_pos = None
                if q_pos is not None and q_pos < len(wup):
                    wup = np.delete(wup, q_pos)
                    lcs = np.delete(lcs, q_pos)
                    cum_best_wup = np.concatenate((cum_best_wup[:q_pos], cum_best_wup[q_pos + 1:] - 1.0))
                    cum_best_lcs = np.concatenate((cum_best_lcs[:q_pos], cum_best_lcs[q_pos + 1:] - 1.0))

            cw, cl = np.cumsum(wup), np.cumsum(lcs)
            for k in ks:
                kk = min(k, len(cw))
                prec['P@{} (WUP)'.format(k)][qid] = (cw[kk - 1] if kk else 0.0) / cum_best_wup[k - 1]
                prec['P@{} (LCS_HEIGHT)'.format(k)][qid] = (cl[kk - 1] if kk else 0.0) / cum_best_lcs[k - 1]
            if compute_ahp:
                if ahp_clip is None:
                    prec[ahp_names[0]][qid] = _trapz(cw / cum_best_wup, dx=1. / len(wup))
                    prec[ahp_names[1]][qid] = _trapz(cl / cum_best_lcs, dx=1. / len(lcs))
                else:
                    prec[ahp_names[0]][qid] = _trapz(cw[:ahp_clip] / cum_best_wup[:ahp_clip], dx=1. / ahp_clip)
                    prec[ahp_names[1]][qid] = _trapz(cl[:ahp_clip] / cum_best_lcs[:ahp_clip], dx=1. / ahp_clip)
            if compute_ap:
                rel = np.fromiter((label_of.setdefault(r, get_label(r)) == lbl for r in ret), dtype=bool, count=len(ret))
                if ignore_qids and q_pos is not None:
                    rel = np.delete(rel, q_pos)
                prec['AP'][qid] = _average_precision(rel)

        return {metric: sum(values.values()) / len(values) for metric, values in prec.items()}, prec

    def ndcg(self, retrieved, labels, ks=[1, 10, 0], ignore_qids=True, all_ids=None, gallery_ids=None, disc=None):
        """Normalised discounted cumulative gain per query + means, with the class similarities as gains: the plain host statement
        of what ``se_ndcg`` computes (``hierarchical_precision_device(..., ndcg=ks)``), for small inputs and as the tests' reference.

        ``retrieved``, ``labels``, ``ignore_qids``, ``all_ids`` as in ``hierarchical_precision``; ``ks``: cut-offs, 0 = the whole list.
        Returns ``(means, per_query)`` with the metrics ``"NDCG@K (WUP)"``, ``"NDCG@K (LCS_HEIGHT)"`` and, for 0, ``"NDCG (WUP)"`` /
        ``"NDCG (LCS_HEIGHT)"``.

        Per query: the ranked list (completed in ``all_ids`` order when it is shorter), the query's own id dropped where it occurs
        (``ignore_qids``); ``DCG@k = sum_{p = 1 .. min(k, len)} sim(query class, class of item p) * disc[p - 1]`` with
        ``disc[p - 1] = 1 / log2(p + 1)`` unless ``disc`` is given.  The ideal DCG takes the same sum over the GALLERY's
        similarities to the query's class in descending order -- the gallery is ``gallery_ids``, else ``all_ids``, else the ids of the
        first list -- without the query's own item when the query is a gallery item (and ``ignore_qids``), whether or not that item
        occurs in the list.  NDCG = DCG / ideal, 0 where the ideal is 0."""
        nd = _ndcg_request(ks)
        if nd is None:
            raise ValueError('no NDCG cut-off given')
        cuts, whole = nd
        columns = _metric_columns([], False, False, nd)
        items = list(retrieved) if isinstance(retrieved, types.GeneratorType) else list(retrieved.items())
        prec = {n: {} for n in columns}
        if not items:
            return {n: float('nan') for n in columns}, prec
        g_ids = list(gallery_ids if gallery_ids is not None else (all_ids if all_ids else items[0][1]))
        g_set = set(g_ids)
        class_list = sorted(set(labels[i] for i in g_ids) | set(labels[q] for q, _ in items), key=repr)
        class_pos = {c: i for i, c in enumerate(class_list)}
        tables = self.similarity_tables(class_list)
        g_cls = np.asarray([class_pos[labels[i]] for i in g_ids], dtype=np.int64)
        n_max = max(len(g_ids), max(len(r) for _, r in items))
        w = 1 / np.log2(np.arange(2, n_max + 2)) if disc is None else np.asarray(disc, dtype=np.float64)
        for qid, ret in items:
            ret = list(ret)
            if all_ids and len(ret) < len(all_ids):
                seen = set(ret)
                ret = ret + [i for i in all_ids if i not in seen]
            if ignore_qids and qid in ret:
                del ret[ret.index(qid)]
            qc = class_pos[labels[qid]]
            cols = np.asarray([class_pos[labels[r]] for r in ret], dtype=np.int64)
            pool = g_cls
            if ignore_qids and qid in g_set:
                pool = np.delete(g_cls, g_ids.index(qid))
            for tname, table in zip(('WUP', 'LCS_HEIGHT'), tables):
                gains = table[qc, cols]
                best = np.sort(table[qc, pool])[::-1]
                for k in cuts + ([0] if whole else []):
                    kk, kb = (min(k, len(gains)), min(k, len(best))) if k else (len(gains), len(best))
                    dcg, idcg = float(np.dot(gains[:kk], w[:kk])), float(np.dot(best[:kb], w[:kb]))
                    prec[('NDCG@{} ({})'.format(k, tname)) if k else 'NDCG ({})'.format(tname)][qid] = dcg / idcg if idcg > 0 else 0.0
        return {metric: sum(values.values()) / len(values) for metric, values in prec.items()}, prec

    def hierarchical_precision_device(self, features, labels, ks=[1, 10, 50, 100], compute_ahp=False, compute_ap=False,
                                      normalize=False, ids=None, tile_rows=None, distributed=False, group=None, kblocks=None,
                                      gather_per_query=True, kernels=None, per_query=True, head_via_topk=True,
                                      gallery=None, gallery_labels=None, gallery_ids=None, tile_cols=None, rank_gallery=False,
                                      precision=None, ndcg=None):
        """``hierarchical_precision(pairwise_retrieval(features, normalize), labels, ...)`` (ignore_qids = True, every
        image is query and gallery item) without leaving the GPU: the rankings stay device tensors
        (``evaluate_retrieval.ranking_tiles``) and the per-query gather + prefix sums run in
        ``se_hierarchical_precision`` instead of the reference's Python loop (class_hierarchy.py:257-314, ~0.6 h at
        N = 50k) -- and the 330 s ``.tolist()`` hand-off of evaluate_retrieval.py:69-73 disappears.

        ``features``: float32 ``[N, D]`` array or (device) tensor (a device copy is normalised when ``normalize``);
        ``labels``: class label of image ``ids[i]`` (``ids`` defaults to ``range(N)``), as a sequence or a mapping.
        Returns ``(means, per_query)`` exactly like ``hierarchical_precision``; ``per_query=False`` returns ``(means, None)`` with
        the means taken on the device (the CLI only prints means: at N = 50k and 250 cut-offs the per-query dictionaries are
        25 million Python floats, seconds of host time after milliseconds of kernels).  ``per_query='table'`` returns the means of
        ``per_query=False`` and, in the place of the dictionaries, a ``bootstrap.MetricTable``: the float64 device tensor
        ``[queries, columns]`` itself, the ``{metric name: column}`` map and the query ids in row order (what ``--bootstrap`` resamples).

        ``distributed`` (one process per GPU, ``torch.distributed`` initialised): every rank holds all features.
        * metrics that need full rankings (AP, un-clipped AHP): the QUERIES are sharded -- rank r ranks rows
          ``shard_bounds(N, G)[r]`` against the replicated gallery, no data-path collective; the per-query metric rows
          are all-gathered (``gather_per_query``) or only their sums all-reduced;
        * otherwise (P@k and AHP@clip only) the GALLERY is sharded: per-shard fused distance + top-L with
          L = max(ks, clip) + 1, RCCL all-gather of the ``(distance, global index)`` lists, canonical k-way merge
          (``sharded_retrieval.sharded_topk``), then each rank scores its share of the queries.
        With one process the same fused top-L path serves P@k / AHP@clip-only requests (``head_via_topk``; the full-ranking
        path otherwise).  ``kblocks`` (None | 'openblas' | list: the BLAS K-block list for D > 448) reaches BOTH paths -- the
        top-L kernels restart their FMA chain per block exactly like the full-ranking ones, so one process and G processes
        return the same near-tie orders.
        ``kernels`` (tests): CPU stand-ins ``{'ranking_tiles', 'hierarchical_precision', 'local_topk', 'merge', 'device'}``.

        ``gallery`` (features like ``features``; ``gallery_labels`` defaults to ``labels``, ``gallery_ids`` like ``ids``): the rows of
        ``features`` are QUERIES against this gallery -- the reference's ``hierarchical_precision(retrieved, labels, ...)`` for any
        ``query id -> ranked gallery ids`` mapping.  A query whose id is a gallery id is dropped from its own ranking
        (``ignore_qids``), the others keep every item; best-possible curves come from the gallery's class counts.  P@k / AHP@K take
        the (sharded-gallery) fused top-L path, AP the counting path of ``recall_precision_device(..., gallery=...)``: no ranking of
        the gallery is made.  Un-clipped AHP needs the whole list and raises ``ValueError`` here (CLI: pass ``--clip_ahp`` or
        ``--rank_gallery``).

        ``rank_gallery`` (opt-in, with ``gallery``; CLI: ``--rank_gallery``): every query's row is ranked against the WHOLE gallery --
        ``ranking_tiles(..., gallery=...)``: ``se_pairwise_dist`` + ``se_rank_rows`` on a tile of query rows -- and every requested
        metric of a query is read from that one ranking by ``se_hierarchical_precision``: P@k, AHP over the whole list
        (``compute_ahp=True``: ``np.trapz(cumsum(sim) / cum_best, dx=1 / len)``, where ``len`` is the gallery without the query's own
        item if it has one) or AHP@K, and AP (no counting pass).  8 bytes per (query, gallery item) pass through device memory, tile
        by tile: before the first launch the tile is sized from the free device memory, after the two ``[C, G]`` float64 best curves,
        their reciprocal table and the operands; a problem that cannot fit raises a ``ValueError`` naming the estimate (``tile_rows``
        overrides the size, not the check).  Several ranks: the QUERIES are sharded, the gallery is replicated (a whole ranking needs
        the whole gallery), rows gathered or sums reduced as above.  No queries at all: the means are NaN, the dictionaries empty.
        ``kernels`` (tests): ``{'normalize_rows_', 'row_sqnorm', 'pairwise_dist', 'rank_rows', 'hierarchical_precision', 'device'}``, the
        names the counting path looks up.

        ``precision='float64'`` (opt-in; CLI: ``--float64``): float64 ``features`` are ranked in float64, as the reference ranks them --
        ``ranking_tiles(..., precision='float64')`` -- and every metric is read from those full rankings (the fused top-L path is a
        float32 path and is not taken).  The metric kernels read ranks only and are the same.  All-pairs in one process only: a
        ``gallery``, ``kblocks`` or several ranks raise ``ValueError``, as float32 features do.

        ``ndcg`` (opt-in; CLI: ``--ndcg K [K ...]``): a list of cut-offs, 0 = the whole list.  Appends the columns ``NDCG@K (WUP)``,
        ``NDCG@K (LCS_HEIGHT)`` and, for 0, ``NDCG (WUP)`` / ``NDCG (LCS_HEIGHT)`` behind the others -- normalised discounted cumulative
        gain with the class similarities as gains and ``1 / log2(position + 1)`` as weights (``se_ndcg``; the host statement is
        ``ClassHierarchy.ndcg``) -- read from the same rank tile as the other metrics, directly after them.  Whole-list NDCG needs
        whole rankings: it takes the full-ranking path as AP does, and with a ``gallery`` and no ``rank_gallery`` it raises
        ``ValueError`` like un-clipped AHP; cut-offs K > 0 are served from the top-L lists, L = max(ks, clip, ndcg) + 1.  Without
        ``ndcg`` every output is what it was.  ``kernels`` (tests): ``'ndcg'``."""
        import torch
        import torch.distributed as dist
        from evaluate_retrieval import RANKING_KERNELS, _resolve_kblocks, is_float64, resolve_kernels, to_device_f64
        from recall_precision import gallery_problem, recall_precision_device, to_device_f32
        from sharded_retrieval import shard_bounds, sharded_topk
        if rank_gallery and gallery is None:
            raise ValueError('rank_gallery=True needs a gallery: without one every image is ranked against all the others already')
        if gallery is not None and not rank_gallery and compute_ahp is True:
            raise ValueError('un-clipped AHP needs the whole ranking of the gallery, which a separate gallery does not get by default: '
                             'pass compute_ahp=K (--clip_ahp K on the command line), or opt into that ranking with rank_gallery=True '
                             '(--rank_gallery)')
        nd = _ndcg_request(ndcg)
        if nd is not None and nd[1] and gallery is not None and not rank_gallery:
            raise ValueError('whole-list NDCG (cut-off 0) needs the whole ranking of the gallery, which a separate gallery does not get by '
                             'default: ask for cut-offs K > 0 only, or opt into that ranking with rank_gallery=True (--rank_gallery)')
        f64 = is_float64(precision)
        if f64 and (gallery is not None or kblocks is not None):
            raise ValueError("precision='float64' ranks all pairs of one float64 feature matrix with ONE FMA chain per distance: a "
                             "separate gallery (rank_gallery included) stays float32, kblocks does not apply")
        # ---- the problem, the device and this rank's queries ----
        given = dict(kernels or {})
        native_metrics = 'hierarchical_precision' not in given
        kernels = resolve_kernels(given, ('hierarchical_precision', 'ranking_tiles', 'device') + (('ndcg',) if nd else ()))
        ks = [ks] if isinstance(ks, int) else list(ks)
        ahp_clip = None if isinstance(compute_ahp, bool) else int(compute_ahp)
        ahp_len = -1 if not compute_ahp else (0 if ahp_clip is None else ahp_clip)
        ncol = 2 * len(ks) + 3 + (2 * len(nd[0]) + 2 if nd else 0)
        p = gallery_problem(features, labels, ids, gallery, gallery_labels, gallery_ids)
        nq, ng, C, dev = int(p.qf.shape[0]), int(p.gf.shape[0]), len(p.class_list), kernels['device']
        if rank_gallery and ng == 0:
            raise ValueError('the gallery is empty')
        if rank_gallery and nq == 0:     # nothing to average
            names = list(_metric_columns(ks, compute_ahp, compute_ap, nd))
            return {m: float('nan') for m in names}, _empty_per_query(names, per_query, dev)
        world = dist.get_world_size(group) if (distributed and dist.is_initialized()) else 1
        rank = dist.get_rank(group) if world > 1 else 0
        if f64 and world > 1:
            raise ValueError("precision='float64' runs in one process: the sharded multi-GPU evaluation stays float32")
        q0, q1 = shard_bounds(nq, world)[rank] if world > 1 else (0, nq)
        # top-L lists are enough when no metric reads past the head of a ranking; a separate gallery is ranked in full on request only
        head_only = (not compute_ap) and (not compute_ahp or ahp_clip is not None) and not (nd and nd[1])
        use_top_lists = (not rank_gallery) if gallery is not None else (head_only and (world > 1 or head_via_topk) and not f64)
        if rank_gallery:    # before anything is launched
            tile_rows = _ranked_gallery_tile_rows(dev, q1 - q0, ng, C, 4 * int(p.qf.shape[1]) * (nq + ng), ncol, tile_rows,
                                                  native_metrics, 'rank_rows' not in given)

        # ---- class tables and best-possible curves ----
        # with the native kernels the class tables are built on the device as well (se_class_pair_tables: the same bits as
        # similarity_tables, whose double loop costs ~18 us per pair on the host); CPU stand-ins keep the host tables
        if (not given) and dev.type == 'cuda':
            wup_t, lcs_t = self.similarity_tables_device(p.class_list, device=dev)
        else:
            wup_t, lcs_t = self.similarity_tables(p.class_list)
        # best-possible cumulative similarity per query class: descending-sorted similarities of the whole gallery.  The C x N float64
        # curves are built ON THE DEVICE (round 6: 180 host cumsums of 50,000 entries + 80 MB of host-to-device copies were 25 of the 56 ms
        # of a 50,000-item evaluation): per class the C similarity values in descending order, each repeated by its class count,
        # then one float64 prefix sum per row.
        counts = np.bincount(p.gcls, minlength=C)
        best = [_best_curves(t, counts, ng, dev) for t in (wup_t, lcs_t)]
        L = min(ng, max(ks + [ahp_clip or 0] + (nd[0] if nd else [])) + 1)
        if use_top_lists:
            best = [b[:, :L + 1].contiguous() for b in best]
            topk_kblocks = _resolve_kblocks(kblocks, int(p.qf.shape[1]))     # (here: its D > 448 warning names the caller)
        tables = [_on_device(t, dev) for t in (wup_t, lcs_t)] + best

        def reciprocal_curves():    # the best curves pre-divided for se_hierarchical_precision (the CPU stand-ins of the tests divide themselves)
            if not native_metrics:
                return {}
            import sehip
            return {'curves': sehip.hprec_reciprocal_curves(*best)}

        # ---- operands: ONE device copy of the features when every image is query and gallery item ----
        fq = to_device_f64(p.qf, dev) if f64 else to_device_f32(p.qf, dev)
        fg = fq if p.gf is p.qf else to_device_f32(p.gf, dev)
        gcls_d = torch.from_numpy(p.gcls).to(dev)
        if gallery is None:
            qcls_d, qidx_d = gcls_d, torch.arange(nq, dtype=torch.int32, device=dev)
        else:
            qcls_d, qidx_d = torch.from_numpy(p.qcls).to(dev), torch.from_numpy(p.qidx).to(dev)
        ks_d = torch.tensor(ks, dtype=torch.int32, device=dev)
        score_ndcg = _ndcg_scorer(nd, kernels, tables[0], tables[1], counts, ng, dev)

        def score(ranks, r0, want_ap, extra):       # metric rows of queries r0 .. r0 + len(ranks)
            r1 = r0 + ranks.shape[0]
            qc, qi = qcls_d[r0:r1].contiguous(), qidx_d[r0:r1].contiguous()
            rows = kernels['hierarchical_precision'](ranks, gcls_d, qc, qi, *tables, ks_d, ahp_len=ahp_len, want_ap=want_ap, **extra)
            return rows if score_ndcg is None else torch.cat([rows, score_ndcg(ranks, gcls_d, qc, qi)], dim=1)   # the same tile, directly after

        def top_lists():
            """Fused distance + top-L (the Q x N matrix is never written) over this rank's shard of the gallery, lists merged across the
            ranks; then the metric rows of this rank's queries."""
            g0, g1 = shard_bounds(ng, world)[rank]
            metric = None
            if 'local_topk' not in given:
                import sehip
                if normalize:
                    sehip.normalize_rows_(fq)
                    if fg is not fq:
                        sehip.normalize_rows_(fg)
                metric = sehip.METRIC_COSINE if normalize else sehip.METRIC_EUCLID
            _, top_i = sharded_topk(fq, fg[g0:g1], L, g0, metric=metric, group=group, local_topk=given.get('local_topk'),
                                    merge=given.get('merge'), kblocks=topk_kblocks)
            return [score(top_i[q0:q1].contiguous(), q0, False, reciprocal_curves())] if q1 > q0 else []

        def ranked_tiles():
            """Full rankings of this rank's queries, tile by tile; each tile is consumed before the next one overwrites it."""
            extra = reciprocal_curves()     # once per gallery, shared by every tile
            if f64:
                tiles_kw = {'precision': 'float64'}
            elif gallery is not None:
                tiles_kw = {'gallery': fg, 'kernels': {k: given[k] for k in RANKING_KERNELS if k in given}}
            # (16-bit ranks between the two kernels -- ranking_tiles(idx16=True), se_hierarchical_precision_r16 -- give the same results
            # from half the bytes, but measured at 50k x 50k the ranking gains 0.24 ms and the metric kernel, which is not bound by its
            # rank stream, loses 0.41 ms to the unpacking: int32 stays the default; SE_EVAL_IDX16=1 switches)
            elif native_metrics and 'ranking_tiles' not in given and ng <= 53248 and os.environ.get('SE_EVAL_IDX16') and not nd:    # (se_ndcg: int32 ranks)
                tiles_kw = {'idx16': True}
            else:
                tiles_kw = {}
            return [score(tile, r0, compute_ap, extra)
                    for r0, tile in kernels['ranking_tiles'](fq, normalize, tile_rows=tile_rows, queries=(q0, q1), kblocks=kblocks, **tiles_kw)]

        outs = top_lists() if use_top_lists else ranked_tiles()
        res_d = outs[0] if len(outs) == 1 else (torch.cat(outs) if outs else torch.zeros((0, ncol), dtype=torch.float64, device=dev))
        columns = _metric_columns(ks, compute_ahp, compute_ap, nd)      # (host work from here on runs under the kernels launched above)
        if use_top_lists and compute_ap:    # a separate gallery: counted, not ranked; every rank gets every query's AP
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)      # queries without a relevant item: AP 0, as in the reference
                aps = recall_precision_device(features, labels, normalize=normalize, ids=ids, kblocks=kblocks, tile_rows=tile_rows,
                                              tile_cols=tile_cols, kernels=given, gallery=gallery, gallery_labels=gallery_labels, gallery_ids=gallery_ids,
                                              distributed=distributed, group=group)[3]
            res_d[:, columns['AP']] = torch.from_numpy(aps[q0:q1]).to(dev)
        return _metric_rows_to_results(res_d, columns, nq, p.q_ids, q0, q1, world, group, gather_per_query, per_query)

    def hierarchical_precision_ranked(self, retrieved, labels, ks=[1, 10, 50, 100], compute_ahp=False, compute_ap=False,
                                      ignore_qids=True, all_ids=None, per_query=True, tile_rows=None, kernels=None, ndcg=None):
        """``hierarchical_precision(retrieved, labels, ks, compute_ahp, compute_ap, ignore_qids, all_ids)`` (class_hierarchy.py:211-316)
        for GIVEN rankings -- from another system, an approximate index, re-ranked or truncated lists -- scored on the device instead
        of in the reference's per-query Python loop.

        ``retrieved``: the reference's dict ``query id -> ranked id list`` or generator of such pairs, or, where Python lists are
        impossible, the array form ``(query_ids [Q], ranking [Q, L][, lengths [Q]])`` with ``ranking`` a 2-d integer array or (device)
        tensor of ids (``recall_precision.ranked_problem``).  ``labels`` maps id -> class label.  The gallery is ``all_ids`` when that
        is given: ids missing from a list are appended in its order (class_hierarchy.py:262-264), on the device
        (``se_complete_rankings``).  Without ``all_ids`` the gallery is the id set of the first list and every list must be a
        permutation of it.  Returns ``(means, per_query)`` as the reference does; ``per_query=False`` returns ``(means, None)``,
        ``per_query='table'`` ``(means, bootstrap.MetricTable)`` as ``hierarchical_precision_device`` does.

        Best-possible curves: the reference takes a class's curve from the first query of that class -- the sorted similarities of
        that query's (completed) list.  Every completed list holds the whole gallery, so that curve is the one
        ``hierarchical_precision_device`` builds from the gallery's class counts (``_best_curves``), whichever query comes first:
        the class tables (device tables included), ``_best_curves``, ``hprec_reciprocal_curves``, the scoring call and
        ``_metric_rows_to_results`` are reused as they are.  That equivalence is what fails for partial lists WITHOUT ``all_ids``,
        where the reference's curve depends on which ids the first query of a class happens to list: those are refused.

        Tiles of query rows: index lists up, ``complete_rankings``, ``hierarchical_precision``; a tile is consumed before the next is
        made, and its size comes from the free device memory (``recall_precision.ranked_tile_rows``; ``tile_rows`` overrides the
        size, not the check).
        Head-only shortcut: when no metric reads past the head of a ranking (no AP; AHP clipped or off) and every list holds at
        least ``min(N, max(ks, clip) + 1)`` entries, nothing is completed -- the heads are scored with that list length, exactly as
        the top-L path of ``hierarchical_precision_device`` scores its lists, so top-250 lists against 1.28 M gallery items never
        become a Q x N matrix.  (Duplicates inside a head are then not looked for.)

        ``ValueError``: an id that is not in the gallery (named, with its query); a list that names an id twice (its query named);
        partial lists without ``all_ids`` (use the host ``hierarchical_precision``); ``max(ks)`` or the AHP clip beyond what a
        ranking holds (the gallery, less the query's own item when queries are gallery items and ``ignore_qids``); an empty
        gallery.  No queries: NaN means and empty dictionaries, as ``hierarchical_precision_device`` returns.  One process, one GPU.
        ``kernels`` (tests): CPU stand-ins ``{'complete_rankings', 'hierarchical_precision', 'ndcg', 'device'}``.

        ``ndcg``: as in ``hierarchical_precision_device`` -- cut-offs, 0 = the whole list; columns appended behind the others.  Cut-offs
        K > 0 count like ``ks`` towards the heads and their bounds; 0 needs completed lists and disables the head-only shortcut."""
        import torch
        from evaluate_retrieval import resolve_kernels
        from recall_precision import _raise_on_bad_rows, ranked_problem, ranked_tile_rows
        given = dict(kernels or {})
        native_metrics = 'hierarchical_precision' not in given
        nd = _ndcg_request(ndcg)
        kernels = resolve_kernels(given, ('complete_rankings', 'hierarchical_precision', 'device') + (('ndcg',) if nd else ()))
        ks = [ks] if isinstance(ks, int) else list(ks)
        ahp_clip = None if isinstance(compute_ahp, bool) else int(compute_ahp)
        ahp_len = -1 if not compute_ahp else (0 if ahp_clip is None else ahp_clip)
        ncol = 2 * len(ks) + 3 + (2 * len(nd[0]) + 2 if nd else 0)
        columns = _metric_columns(ks, compute_ahp, compute_ap, nd)
        p = ranked_problem(retrieved, labels, ignore_qids, all_ids)
        nq, ng, C, dev = len(p.q_ids), len(p.g_ids), len(p.class_list), kernels['device']
        if nq == 0:         # nothing to average
            return {m: float('nan') for m in columns}, _empty_per_query(columns, per_query, dev)
        if ng == 0:
            raise ValueError('the gallery is empty')
        kmax = max(ks + [ahp_clip or 0] + (nd[0] if nd else []))
        scored = ng - 1 if (p.qidx is not None and (p.qidx >= 0).any()) else ng      # entries of the shortest scored ranking
        if kmax > scored or min(ks) < 1 or (ahp_clip is not None and ahp_clip < 1):
            raise ValueError('cut-offs {} and AHP clip {} must lie in [1, {}]: a ranking of the {} gallery items{} holds no more'
                             .format(ks, ahp_clip, scored, ng, ', the query\'s own item dropped,' if scored < ng else ''))
        # top-L heads are enough when no metric reads past the head of a ranking and every list has one
        L = min(ng, kmax + 1)
        head_only = (not compute_ap) and (not compute_ahp or ahp_clip is not None) and not (nd and nd[1]) and int(p.lengths.min()) >= L

        # ---- class tables and best-possible curves, as hierarchical_precision_device builds them ----
        if (not given) and dev.type == 'cuda':
            wup_t, lcs_t = self.similarity_tables_device(p.class_list, device=dev)
        else:
            wup_t, lcs_t = self.similarity_tables(p.class_list)
        counts = np.bincount(p.gcls, minlength=C)
        if not head_only:       # before anything is launched
            curve_len = 0
            if native_metrics:
                import sehip
                curve_len = int(sehip._lib.call('se_hprec_curve_len', ng))
            tile_rows = ranked_tile_rows(dev, nq, ng, p.list_len, 2 * 8 * C * ng + 32 * C * curve_len, 8 * ncol, tile_rows,
                                         'hierarchical precision')
        else:
            tile_rows = max(1, min(nq, int(tile_rows or max(128, (1 << 28) // max(p.list_len, 1)))))
        best = [_best_curves(t, counts, ng, dev) for t in (wup_t, lcs_t)]
        if head_only:
            best = [b[:, :L + 1].contiguous() for b in best]
        tables = [_on_device(t, dev) for t in (wup_t, lcs_t)] + best
        extra = {}
        if native_metrics:      # the best curves pre-divided for se_hierarchical_precision: once per gallery, shared by every tile
            import sehip
            extra = {'curves': sehip.hprec_reciprocal_curves(*best)}
        gcls_d, qcls_d = torch.from_numpy(p.gcls).to(dev), torch.from_numpy(p.qcls).to(dev)
        qidx_d = None if p.qidx is None else torch.from_numpy(p.qidx).to(dev)
        ks_d = torch.tensor(ks, dtype=torch.int32, device=dev)
        score_ndcg = _ndcg_scorer(nd, kernels, tables[0], tables[1], counts, ng, dev)

        def score(ranks, r0, want_ap):       # metric rows of queries r0 .. r0 + len(ranks)
            r1 = r0 + ranks.shape[0]
            qc, qi = qcls_d[r0:r1].contiguous(), None if qidx_d is None else qidx_d[r0:r1].contiguous()
            rows = kernels['hierarchical_precision'](ranks, gcls_d, qc, qi, *tables, ks_d, ahp_len=ahp_len, want_ap=want_ap, **extra)
            return rows if score_ndcg is None else torch.cat([rows, score_ndcg(ranks, gcls_d, qc, qi)], dim=1)   # the same tile, directly after

        outs = []
        for r0 in range(0, nq, tile_rows):      # each tile is consumed before the next one is made
            r1 = min(nq, r0 + tile_rows)
            lists_d, len_d = p.index_tile(r0, r1, dev)
            if head_only:
                outs.append(score(lists_d[:, :L].contiguous(), r0, False))
            else:
                rank, status = kernels['complete_rankings'](lists_d, ng, lengths=len_d)
                _raise_on_bad_rows(status, p, r0)
                outs.append(score(rank, r0, compute_ap))
        res_d = outs[0] if len(outs) == 1 else torch.cat(outs)
        return _metric_rows_to_results(res_d, columns, nq, p.q_ids, 0, nq, 1, None, True, per_query)


def _metric_columns(ks, compute_ahp, compute_ap, ndcg=None):
    """Metric name -> column of se_hierarchical_precision's ``[Q, 2 len(ks) + 3]`` output, in the order of the result dictionaries:
    ``P@k (WUP)`` and ``P@k (LCS_HEIGHT)`` per cut-off, ``AHP[@K] (WUP)`` / ``(LCS_HEIGHT)`` (``compute_ahp``: True or K), ``AP``.
    ``ndcg`` (``_ndcg_request``'s pair, or None): se_ndcg's ``[Q, 2 len(cuts) + 2]`` columns stand behind those -- ``NDCG@K (WUP)``
    and ``NDCG@K (LCS_HEIGHT)`` per cut-off, then ``NDCG (WUP)`` / ``NDCG (LCS_HEIGHT)`` when the whole list was asked for."""
    nk = len(ks)
    col = {}
    for t, k in enumerate(ks):
        col['P@{} (WUP)'.format(k)] = t
        col['P@{} (LCS_HEIGHT)'.format(k)] = nk + t
    if compute_ahp:
        sfx = '' if isinstance(compute_ahp, bool) else '@{}'.format(int(compute_ahp))
        col['AHP{} (WUP)'.format(sfx)] = 2 * nk
        col['AHP{} (LCS_HEIGHT)'.format(sfx)] = 2 * nk + 1
    if compute_ap:
        col['AP'] = 2 * nk + 2
    if ndcg:
        cuts, whole = ndcg
        for t, k in enumerate(cuts):
            col['NDCG@{} (WUP)'.format(k)] = 2 * nk + 3 + t
            col['NDCG@{} (LCS_HEIGHT)'.format(k)] = 2 * nk + 3 + len(cuts) + t
        if whole:
            col['NDCG (WUP)'] = 2 * nk + 3 + 2 * len(cuts)
            col['NDCG (LCS_HEIGHT)'] = 2 * nk + 3 + 2 * len(cuts) + 1
    return col


def _ndcg_request(ndcg):
    """The ``ndcg`` argument of the evaluations -- None, an int or a list of cut-offs, 0 = the whole list -- as ``(cut-offs > 0 in
    the order given, each once; whether the whole list is asked for)``, or None when nothing is."""
    if ndcg is None or ndcg is False:
        return None
    asked = [ndcg] if isinstance(ndcg, (int, np.integer)) else list(ndcg)
    if not asked:
        return None
    if any(int(k) != k or k < 0 for k in asked):
        raise ValueError('NDCG cut-offs must be integers >= 0 (0: the whole list), got {}'.format(asked))
    cuts = []
    for k in asked:
        if k > 0 and int(k) not in cuts:
            cuts.append(int(k))
    return cuts, any(k == 0 for k in asked)


def _ndcg_scorer(nd, kernels, wup_d, lcs_d, counts, ng, dev):
    """``score(ranks, gcls, qcls, qidx) -> [rows, 2 len(cuts) + 2]`` float64 rows of ``kernels['ndcg']`` (``sehip.ndcg``) for one
    gallery, or None when no NDCG is asked for (``nd``: ``_ndcg_request``).  Built once per evaluation: the discounts
    ``1 / log2(p + 1)`` of every gallery position and the ideal DCG of every query class from the gallery's class counts
    (``sehip.ndcg_ideal``: member and non-member queries, both tables, every cut-off and the whole list)."""
    if not nd:
        return None
    import torch
    import sehip
    cuts, whole = nd
    disc = sehip.ndcg_discounts(ng, dev)
    ideal = torch.stack([sehip.ndcg_ideal(t, counts, disc, cuts, full=whole) for t in (wup_d, lcs_d)], dim=2).contiguous()
    cuts_d = torch.tensor(cuts, dtype=torch.int32, device=dev)

    def score(ranks, gcls_d, qcls_d, qidx_d):
        return kernels['ndcg'](ranks, gcls_d, qcls_d, qidx_d, wup_d, lcs_d, disc, ideal, cuts_d, want_full=whole)
    return score


def _ranked_gallery_tile_rows(dev, nq, ng, C, feature_bytes, ncol, tile_rows, native_metrics, native_ranking):
    """Query rows per tile of ``hierarchical_precision_device(..., rank_gallery=True)`` for this rank's ``nq`` queries, from what the
    evaluation will hold on the device, known before anything is launched: the two [C, G] float64 best curves, their reciprocal table
    (per class two rows of se_hprec_curve_len(G) double2), the operands (``feature_bytes``), and per tile row its distances, its ranks
    (rows of 16-byte pitch) and its metrics, plus the ranking's workspace.  ``tile_rows`` overrides the size, not the check: a
    problem that cannot fit the free device memory raises ``ValueError``."""
    if native_metrics or native_ranking:
        import sehip
    row_bytes = 8 * ((ng + 3) // 4 * 4) + 8 * ncol

    def tile_bytes(rows):
        return rows * row_bytes + (int(sehip.rank_rows_workspace_bytes(rows, ng)) if native_ranking else 0)

    fixed = 2 * 8 * C * ng + 32 * C * (int(sehip._lib.call('se_hprec_curve_len', ng)) if native_metrics else 0) + feature_bytes
    free = _free_device_bytes(dev)
    budget = None if free is None else free - free // 10        # a tenth stays free: allocator granularity, the other kernels' scratch
    rows = max(1, nq)
    if tile_rows is not None:
        rows = max(1, min(rows, int(tile_rows)))
    elif budget is not None:
        rows = max(1, min(rows, (budget - fixed) // row_bytes))
        while rows > 1 and fixed + tile_bytes(rows) > budget:
            rows = rows * 3 // 4
        if 128 < rows < nq:
            rows = rows // 128 * 128
    estimate = fixed + tile_bytes(rows)
    if budget is not None and estimate > budget:
        raise ValueError('ranking {} queries against a gallery of {} items in {} classes needs an estimated {:,} bytes of device memory '
                         '({:,} for the best-possible curves, their reciprocal table and the features, {:,} for a tile of {} query row{}), '
                         '{:,} are free: use the counting path (rank_gallery=False with compute_ahp=K), fewer classes or a smaller gallery'
                         .format(nq, ng, C, estimate, fixed, estimate - fixed, rows, '' if rows == 1 else 's', free))
    return rows


def _wants_table(per_query):
    """``per_query='table'``: the per-query values as ``bootstrap.MetricTable`` -- the float64 device tensor [queries, columns], the
    ``{metric name: column}`` map and the query ids in row order -- instead of dictionaries (minutes of host time at 50,000 queries x
    500 columns)."""
    return isinstance(per_query, str) and per_query == 'table'


def _empty_per_query(names, per_query, dev):
    """The second return value when there is no query at all."""
    if not per_query:
        return None
    if _wants_table(per_query):
        import torch
        from bootstrap import MetricTable
        names = list(names)
        return MetricTable(torch.zeros((0, len(names)), dtype=torch.float64, device=dev), {m: c for c, m in enumerate(names)}, [])
    return {m: {} for m in names}


def _metric_rows_to_results(res_d, columns, n, ids, q0, q1, world, group, gather_per_query, per_query):
    """``(means, per_query)`` from this rank's rows ``q0 .. q1`` of se_hierarchical_precision's output (all-gathered, or only their
    sums all-reduced, under several ranks); ``columns``: ``_metric_columns``.  ``per_query='table'``: ``_wants_table``."""
    import torch
    import torch.distributed as dist
    from sharded_retrieval import shard_bounds
    ncol, dev = res_d.shape[1], res_d.device
    sums = None
    if world > 1:
        if gather_per_query and per_query:    # ragged all-gather: pad every shard to the largest one
            rows_max = max(e - s for s, e in shard_bounds(n, world))
            padded = torch.zeros((rows_max, ncol), dtype=torch.float64, device=dev)
            padded[:res_d.shape[0]] = res_d
            gathered = torch.empty((world * rows_max, ncol), dtype=torch.float64, device=dev)
            dist.all_gather_into_tensor(gathered, padded, group=group)
            res_d = torch.cat([gathered[r * rows_max:r * rows_max + (e - s)] for r, (s, e) in enumerate(shard_bounds(n, world))])
            q0, q1 = 0, n
        else:                   # the means only: one all-reduce of ncol sums
            sums = res_d.sum(dim=0)
            dist.all_reduce(sums, group=group)
    if not per_query or _wants_table(per_query):
        if sums is None:        # every row is here (one process, or gathered): the column means
            sums = res_d.sum(dim=0)
        sums = sums.cpu().numpy()
        means = {name: float(sums[c]) / n for name, c in columns.items()}
        if per_query:           # 'table': the rows stay on the device (the means are those of per_query=False, bit for bit)
            from bootstrap import MetricTable
            return means, MetricTable(res_d, dict(columns), list(ids[q0:q1]))
        return means, None
    res = res_d.cpu().numpy()
    prec = {name: dict(zip(ids[q0:q1], res[:, c].tolist())) for name, c in columns.items()}
    if sums is not None:
        sums = sums.cpu().numpy()
        return {name: float(sums[c]) / n for name, c in columns.items()}, prec
    return {metric: sum(values.values()) / len(values) for metric, values in prec.items()}, prec


def _best_curves(table, counts, n, dev):
    """[C, n] float64 device curves: per query class the C similarity values in descending order, each repeated by the gallery's count
    of its class (``counts``, n items in all), then one prefix sum per row."""
    import torch
    C = len(counts)
    if torch.is_tensor(table):      # device table: the descending values are the same whatever order ties take
        vals, order = torch.sort(table, dim=1, descending=True)
        reps = torch.from_numpy(counts.astype(np.int64)).to(dev)[order]
        flat = torch.repeat_interleave(vals.reshape(-1), reps.reshape(-1), output_size=C * n)
        return flat.view(C, n).cumsum(dim=1)
    table = np.asarray(table, dtype=np.float64)
    order = np.argsort(-table, axis=1, kind='stable')
    vals = torch.from_numpy(np.take_along_axis(table, order, axis=1)).to(dev)
    reps = torch.from_numpy(counts[order].astype(np.int64)).to(dev)
    flat = torch.repeat_interleave(vals.reshape(-1), reps.reshape(-1), output_size=C * n)
    return flat.view(C, n).cumsum(dim=1)


def _free_device_bytes(dev):
    """Bytes of device memory an allocation on ``dev`` can still get -- free on the device, or held unused by torch's caching
    allocator; None where there is nothing to size against (the CPU stand-ins of the tests)."""
    import torch
    dev = torch.device(dev)
    if dev.type != 'cuda':
        return None
    return int(torch.cuda.mem_get_info(dev)[0]) + int(torch.cuda.memory_reserved(dev)) - int(torch.cuda.memory_allocated(dev))


def _on_device(table, dev):
    import torch
    return table if torch.is_tensor(table) else torch.from_numpy(np.ascontiguousarray(table)).to(dev)


def _average_precision(relevant):
    """AP of a ranking with distinct scores: mean over the relevant items of precision at their
    rank (== sklearn.metrics.average_precision_score for tie-free scores; 0 if nothing is relevant)."""
    hits = np.flatnonzero(relevant)
    if hits.size == 0:
        return 0.0
    return float(np.mean(np.arange(1, hits.size + 1) / (hits + 1.0)))
