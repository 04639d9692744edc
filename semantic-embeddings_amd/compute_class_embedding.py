"""Semantic class embeddings from a class hierarchy (step 1 of the method) on the MI355X kernels of classemb.hip.

Drop-in for the reference's ``compute_class_embedding.py``: the same command line, class order, printed lines and pickle
``{'ind2label', 'label2ind', 'embedding'}`` (float64), and the same importable functions:

* the class distances ``lcs_height(a, b)`` of every pair (compute_class_embedding.py:212-216, a Python double loop) come from
  ``se_class_pair_tables`` (``ClassHierarchy.similarity_tables_device`` with the reference's zero-distance diagonal);
* ``unitsphere_embedding`` (:14-40): row c of the reference solves ``E[:c, :c] x = S[c, :c]`` and sets ``E[c, c] =
  sqrt(1 - |x|^2)`` -- which is the lower Cholesky factor of S with its diagonal read as 1 -- so it is one ``se_cholesky_f64``
  (O(n^3 / 3) on the matrix cores instead of n solves of growing size, O(n^4)).  A failed pivot leaves that row's diagonal and
  every later row NaN, as the reference's sqrt of a negative does, and warns;
* ``euclidean_embedding`` (:76-130, "spheres"): class 0 at the origin, class c >= 1 at row c - 1 of the Cholesky factor of the
  Gram matrix ``G_ij = (d_0i^2 + d_0j^2 - d_ij^2) / 2`` of the classes 1 .. n - 1 -- the reference's successive hypersphere
  intersections solve exactly these triangular systems.  A failed pivot raises the reference's RuntimeError for that class;
* ``sim_approx`` / ``mds`` (:44-72, :134-160): their ``np.linalg.eigh`` is ``se_eigh_f64`` (``sim_approx_factor`` /
  ``mds_factor``: two-sided block Jacobi in float64 on the matrix cores; the double-centring of mds is formed on the device from
  the row, column and grand means instead of two n^3 products).  The reference's rules act on the device eigenvalues unchanged:
  a negative eigenvalue is the RuntimeError of sim_approx, mds keeps ``lam > eps``, the largest eigenvalue comes last in
  approx_sim and first in mds.  The importable ``sim_approx`` / ``mds`` are the host NumPy forms; ``main`` takes them when no
  GPU is present and above ``EIGH_DEVICE_MAX_CLASSES`` classes.  The host's LAPACK is measured faster at every size; the
  constant caps what the device path may cost (see its comment).

The deviation report ("Maximum/Average deviation from target ...") is formed on the device in float64 (an n^3 product at
n = 8,142 would take minutes of host BLAS).  Results are tolerance-equal to the reference (the factorisation sums in another
order; eigenvectors up to sign and to the basis of a cluster of equal eigenvalues); the tables are bit-identical.
"""
import argparse
import pickle
import sys
import time
import warnings
from collections import OrderedDict

import numpy as np

from class_hierarchy import ClassHierarchy

METHODS = ['unitsphere', 'approx_sim', 'spheres', 'mds']

# main() takes the device eigensolver up to this many classes and the host's np.linalg.eigh above it.  This is a cap on what the
# device path may cost, not a crossover: the block Jacobi solver loses to the host's LAPACK at every measured size
# (profiles/classemb_eigh_bench.txt: 14 ms against 0.5 ms at n = 100, 46 ms against 1.6 ms at 200, 0.14 s against 0.014 s at 512,
# 0.72 s against 0.04 s at 1,000, 12.7 s against 4.2 s at 8,142).  Up to 512 classes the loss is at most 0.12 s of a command that
# takes seconds, and the step stays on the device with the tables and the deviation report; above it the host is taken.
EIGH_DEVICE_MAX_CLASSES = 512


def _square(a, what):
    a = np.asarray(a) if not hasattr(a, 'is_cuda') else a
    if (a.ndim != 2) or (a.shape[0] != a.shape[1]):
        raise ValueError('Given {} has invalid shape. Expected: (n, n). Got: {}'.format(what, tuple(a.shape)))
    if a.shape[0] == 0:
        raise ValueError('Empty {} given.'.format(what))
    return a


def _to_device(a):
    """float64 device copy (contiguous rows) of an array or tensor."""
    import torch
    if torch.is_tensor(a):
        return a.detach().to(device=torch.device('cuda', torch.cuda.current_device()), dtype=torch.float64).contiguous().clone()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _host(a):
    """NumPy form of an array or tensor."""
    return a.detach().cpu().numpy() if hasattr(a, 'is_cuda') else a


def unitsphere_factor(class_sim):
    """Device form of ``unitsphere_embedding``: (embedding float64 [n, n] device tensor, failed row or -1)."""
    import sehip
    e = _to_device(class_sim)
    e.fill_diagonal_(1.0)          # the reference places every class on the unit sphere whatever the diagonal says
    _, info = sehip.cholesky_lower_(e)
    return e, int(info.item())


def unitsphere_embedding(class_sim):
    """Embedding of n classes on the unit sphere of R^n whose dot products are ``class_sim`` (n x n): the rows of its lower
    Cholesky factor.  A class that cannot be placed (its pivot is <= 0) gets NaN on its diagonal and NaN rows follow it,
    with a RuntimeWarning naming it."""
    _square(class_sim, 'class_sim')
    e, fail = unitsphere_factor(class_sim)
    if fail >= 0:
        warnings.warn('class #{} cannot be placed on the unit sphere (the similarities are not positive definite); its '
                      'diagonal and every later row are NaN'.format(fail + 1), RuntimeWarning, stacklevel=2)
    return e.cpu().numpy()


def spheres_factor(class_dist):
    """Device form of ``euclidean_embedding``: (embedding float64 [n, n - 1] device tensor, failed class index or -1)."""
    import sehip
    import torch
    d = _to_device(class_dist)
    n = d.shape[0]
    emb = torch.zeros((n, max(n - 1, 0)), dtype=torch.float64, device=d.device)
    if n < 2:
        return emb, -1
    sq = d * d
    g = (sq[0, 1:, None] + sq[None, 0, 1:] - sq[1:, 1:]) * 0.5
    g = g.contiguous()
    _, info = sehip.cholesky_lower_(g)
    emb[1:] = g
    fail = int(info.item())
    return emb, (fail + 1 if fail >= 0 else -1)


def euclidean_embedding(class_dist, solver='general'):
    """Embedding of n classes in R^(n - 1) whose Euclidean distances are ``class_dist`` (a metric): class 0 at the origin,
    the others at the rows of the Cholesky factor of their Gram matrix around it.  ``solver`` is accepted for compatibility
    ('general' / 'triangular'; one factorisation serves both).  RuntimeError if a class cannot be placed."""
    _square(class_dist, 'class_dist')
    if solver not in ('general', 'triangular'):
        raise ValueError('Unknown solver: {}'.format(solver))
    emb, fail = spheres_factor(class_dist)
    if fail >= 0:
        row = emb[fail, :fail - 1]
        d_sq = float((row * row).sum())
        r0 = float(np.asarray(class_dist, dtype=np.float64)[0, fail]) if not hasattr(class_dist, 'is_cuda') else float(class_dist[0, fail])
        raise RuntimeError('Failed to place class #{}: There is no common intersection of all spheres (offset: {}).'.format(
            fail + 1, np.sqrt(d_sq) - abs(r0)))
    return emb.cpu().numpy()


def _device_eigh(matrix, what):
    """(ascending eigenvalues, eigenvector columns) of a symmetric device matrix by ``se_eigh_f64``; an input the solver cannot
    decompose raises."""
    import sehip
    lam, vec, info = sehip.eigh(matrix, overwrite_a=True)
    if info == sehip.EIGH_NONFINITE:
        raise RuntimeError('Given {} holds NaN or infinite values.'.format(what))
    if info < 0:
        raise RuntimeError('The eigendecomposition of {} did not converge.'.format(what))
    return lam, vec


def sim_approx_factor(class_sim, num_dim=None):
    """Device form of ``sim_approx``: the embedding as a float64 [n, min(n, num_dim)] device tensor.  RuntimeError if an
    eigenvalue of ``class_sim`` is negative, like the reference."""
    lam, vec = _device_eigh(_to_device(class_sim), 'class_sim')
    if bool((lam < 0).any()):
        raise RuntimeError('Given class_sim is not positive semi-definite.')
    emb = vec * lam.sqrt()[None, :]
    if num_dim is not None and num_dim < emb.shape[1]:
        emb = emb[:, emb.shape[1] - num_dim:]
    return emb.contiguous()


def mds_factor(class_dist, num_dim=None):
    """Device form of ``mds``: the embedding as a float64 device tensor [n, number of eigenvalues kept].  The double-centred
    matrix -(D^2 - row means - column means + grand mean) / 2 is formed element-wise; like ``np.linalg.eigh`` only its lower
    triangle counts."""
    import torch
    sq = _to_device(class_dist)
    sq.mul_(sq)
    b = (sq - sq.mean(dim=1, keepdim=True) - sq.mean(dim=0, keepdim=True) + sq.mean()).mul_(-0.5)
    b = b.tril() + b.tril(-1).T
    lam, vec = _device_eigh(b.contiguous(), 'class_dist')
    keep = lam > np.finfo(np.float64).eps
    lam, vec = lam[keep], vec[:, keep]
    if num_dim is not None:
        top = torch.argsort(lam, stable=True).flip(0)[:num_dim]
        lam, vec = lam[top], vec[:, top]
    return (vec * lam.sqrt()[None, :]).contiguous()


def sim_approx(class_sim, num_dim=None):
    """Embedding whose dot products best approximate ``class_sim`` in at most ``num_dim`` dimensions (all n by default): the
    eigenvectors of the similarity matrix scaled by the roots of their eigenvalues, largest last.  Host NumPy ``eigh``."""
    class_sim = _square(class_sim, 'class_sim')
    if hasattr(class_sim, 'is_cuda'):
        class_sim = class_sim.detach().cpu().numpy()
    lam, vec = np.linalg.eigh(class_sim)
    if (lam < 0).any():
        raise RuntimeError('Given class_sim is not positive semi-definite.')
    emb = vec * np.sqrt(lam)[None, :]
    if num_dim is not None and num_dim < emb.shape[1]:
        emb = emb[:, emb.shape[1] - num_dim:]
    return emb


def mds(class_dist, num_dim=None):
    """Classical multidimensional scaling of the distance matrix ``class_dist``: the eigenvectors of the double-centred squared
    distances with an eigenvalue above machine epsilon, scaled by its root; the ``num_dim`` largest when given.  Host NumPy."""
    if hasattr(class_dist, 'is_cuda'):
        class_dist = class_dist.detach().cpu().numpy()
    n = class_dist.shape[0]
    centre = np.eye(n, dtype=class_dist.dtype) - np.ones(class_dist.shape, dtype=class_dist.dtype) / n
    b = np.dot(centre, np.dot(class_dist ** 2, centre)) / -2
    lam, vec = np.linalg.eigh(b)
    keep = lam > np.finfo(class_dist.dtype).eps
    lam, vec = lam[keep], vec[:, keep]
    if num_dim is not None:
        top = np.argsort(lam)[::-1][:num_dim]
        lam, vec = lam[top], vec[:, top]
    return vec * np.sqrt(lam[None, :])


def deviation(embedding, target, distances):
    """(max, mean) of |E E^T - target| (``distances`` False) or |pdist(E) - target| in float64: on the device, or in NumPy when
    there is none (the host path of approx_sim / mds)."""
    import torch
    if not torch.cuda.is_available():
        e, t = np.asarray(embedding, dtype=np.float64), np.asarray(target, dtype=np.float64)
        err_max, err_sum = 0.0, 0.0
        for r0 in range(0, e.shape[0], 256):                # 256 rows at a time: never more than a [256, n] block
            est = e[r0:r0 + 256] @ e.T
            if distances:
                sq = (e * e).sum(-1)
                est = np.sqrt(np.maximum(sq[r0:r0 + 256, None] + sq[None, :] - 2.0 * est, 0.0))
            err = np.abs(est - t[r0:r0 + 256])
            err_max, err_sum = max(err_max, float(err.max())), err_sum + float(err.sum())
        return err_max, err_sum / t.size
    e, t = _to_device(embedding), _to_device(target)
    if distances:
        est = torch.cdist(e, e, compute_mode='donot_use_mm_for_euclid_dist')     # direct differences, like scipy's pdist
    else:
        est = e @ e.T
    err = (est - t).abs_()
    return float(err.max()), float(err.mean())


def class_order(hierarchy, class_list=None, str_ids=False):
    """The target classes in the reference's order: the first word of every non-empty line of ``class_list`` (first occurrence
    wins), else the leaves of the hierarchy, sorted unless the ids are strings."""
    id_type = str if str_ids else int
    if class_list is not None:
        with open(class_list) as f:
            return list(OrderedDict((id_type(line.strip().split()[0]), None) for line in f if line.strip() != '').keys())
    labels = [c for c in hierarchy.nodes if (c not in hierarchy.children) or (len(hierarchy.children[c]) == 0)]
    if not str_ids:
        labels.sort()
    return labels


def build_parser():
    """Same flags, choices and defaults as the reference CLI (compute_class_embedding.py:166-179)."""
    p = argparse.ArgumentParser(description='Computes semantic class embeddings based on a given hierarchy.',
                                formatter_class=argparse.RawTextHelpFormatter)
    p.add_argument('--hierarchy', type=str, required=True, help='File of parent-child (or, with --is_a, is-a) relations, one per line.')
    p.add_argument('--is_a', action='store_true', default=False, help='--hierarchy holds is-a relations ("child parent") instead of parent-child ones.')
    p.add_argument('--str_ids', action='store_true', default=False, help='Treat class ids as strings (default: integers).')
    p.add_argument('--class_list', type=str, default=None,
                   help='File whose lines start with the ids of the classes to embed. Default: every leaf of the hierarchy.')
    p.add_argument('--out', type=str, required=True, help='Output pickle with the items "embedding", "ind2label" and "label2ind".')
    p.add_argument('--method', type=str, default='unitsphere', choices=METHODS,
                   help='''Embedding algorithm:
    - "unitsphere": n-dimensional unit-norm embeddings whose dot products are the semantic similarities.
    - "approx_sim": embeddings of any dimensionality whose dot products approximate the semantic similarities.
    - "spheres": (n-1)-dimensional embeddings whose Euclidean distances are the semantic dissimilarities (hypersphere intersections).
    - "mds": embeddings of any dimensionality whose Euclidean distances approximate the semantic dissimilarities (classical MDS).
Default: "unitsphere"''')
    p.add_argument('--num_dim', type=int, default=None, help='Embedding dimensions of the "mds" and "approx_sim" methods.')
    p.add_argument('--norm', action='store_true', default=False, help='L2-normalise the embeddings (most useful with approx_sim).')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    on_device = torch.cuda.is_available()
    if not on_device and args.method not in ('approx_sim', 'mds'):
        import sehip
        raise sehip.SehipError('compute_class_embedding.py runs on a ROCm GPU; there is no CPU fallback')
    id_type = str if args.str_ids else int
    hierarchy = ClassHierarchy.from_file(args.hierarchy, is_a_relations=args.is_a, id_type=id_type)
    unique_labels = class_order(hierarchy, args.class_list, args.str_ids)
    linear_labels = {lbl: i for i, lbl in enumerate(unique_labels)}

    # target distances lcs_height(a, b) of every pair, zero on the diagonal
    if on_device:
        _, sem_class_dist = hierarchy.similarity_tables_device(unique_labels, diag_one=True, distance=True, want_wup=False)
    else:       # the eigendecomposition methods without a GPU: the host tables (1 - lcs_height off the diagonal)
        sem_class_dist = 1. - hierarchy.similarity_tables(unique_labels)[1]
        np.fill_diagonal(sem_class_dist, 0.)

    device_eigh = on_device and len(unique_labels) <= EIGH_DEVICE_MAX_CLASSES
    start_time = time.time()
    if args.method == 'spheres':
        embedding = euclidean_embedding(sem_class_dist)
    elif args.method == 'mds':
        num_dim = args.num_dim if args.num_dim else len(unique_labels) - 1
        embedding = mds_factor(sem_class_dist, num_dim).cpu().numpy() if device_eigh else mds(_host(sem_class_dist), num_dim)
    elif args.method == 'unitsphere':
        embedding = unitsphere_embedding(1. - sem_class_dist)
    elif device_eigh:
        embedding = sim_approx_factor(1. - sem_class_dist, args.num_dim).cpu().numpy()
    else:
        embedding = sim_approx(_host(1. - sem_class_dist), args.num_dim)
    stop_time = time.time()
    print('Computed {}-dimensional semantic embeddings for {} classes using the "{}" method in {} seconds.'.format(
        embedding.shape[1], embedding.shape[0], args.method, stop_time - start_time))
    if args.method in ('unitsphere', 'approx_sim'):
        err_max, err_mean = deviation(embedding, 1. - sem_class_dist, distances=False)
        print('Maximum deviation from target similarities: {}'.format(err_max))
        print('Average deviation from target similarities: {}'.format(err_mean))
    else:
        err_max, err_mean = deviation(embedding, sem_class_dist, distances=True)
        print('Maximum deviation from target distances: {}'.format(err_max))
        print('Average deviation from target distances: {}'.format(err_mean))

    if args.norm:
        embedding /= np.linalg.norm(embedding, axis=-1, keepdims=True)

    with open(args.out, 'wb') as dump_file:
        pickle.dump({'ind2label': unique_labels, 'label2ind': linear_labels, 'embedding': embedding}, dump_file)
    return embedding


if __name__ == '__main__':
    main(sys.argv[1:])
