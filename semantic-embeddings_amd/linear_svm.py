"""Linear SVM classification on the MI355X: a drop-in for the ``LinearSVC`` of the reference's evaluate_classification_accuracy.py.

The reference fits scikit-learn's ``LinearSVC(C)`` with its defaults (``penalty='l2'``, ``loss='squared_hinge'``,
``multi_class='ovr'``, ``fit_intercept=True``, ``intercept_scaling=1``).  liblinear appends a constant-1 feature, so the bias is
regularised; for every class column ``c`` of ``classes_`` (``y_ic = +1`` if ``y_i == classes_[c]``, ``-1`` otherwise) it minimises

    f_c(w, b) = 1/2 (|w|^2 + b^2) + C sum_i max(0, 1 - y_ic (w . x_i + b))^2 .

``f_c`` is strictly convex, so every solver converges to the same optimum; that optimum is the target here, not liblinear's
trajectory.  ``LinearSVC.fit`` runs liblinear's primal trust-region Newton method (Lin, Weng & Keerthi 2008) for all classes at
once: every class keeps its own iterate, trust radius and conjugate-gradient state, and every O(N) step is one of the two fp32
MFMA contractions of ``csrc/svm.hip`` (margins with a fused epilogue, and ``Z^T [X | 1]``).  The host reads one small array of
per-class scalars per CG step and decides, in float64, what the next vector updates are.

Differences from scikit-learn, on purpose:

* the data and the model are float32 (scikit-learn converts to float64); sums over samples are combined in float64;
* near the optimum the float32 objective cannot resolve a step's decrease any more: when the predicted decrease falls below that
  resolution, a step is accepted when it lowers the gradient norm (liblinear would compare the objective values);
* converged classes leave the working set (and a set of fewer than 3 classes is padded with finished ones, which are not
  changed); ``n_iter_`` is the largest number of outer iterations of any class;
* binary problems raise ``ValueError`` (the reference's ``decision_function(X).argsort(-1)[:, ::-1]`` cannot take them).

``objective_host`` / ``gradient_host`` / ``hessian_vector_host`` are the NumPy float64 statement of the same problem, and
``fit_host`` runs the same solver on them (tests and ``tools/make_svm_golden.py``).
"""
import sys
import warnings

import numpy as np

ETA0, ETA1, ETA2 = 1e-4, 0.25, 0.75
SIGMA1, SIGMA2, SIGMA3 = 0.25, 0.5, 4.0
MIN_COLUMNS = 3                 # the kernels take at least 3 class columns


class ConvergenceWarning(UserWarning):
    pass


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 host statement.  Wb [C, D + 1]: row c = (w_c, b_c); Y [N, C] of +-1; X [N, D].
# ---------------------------------------------------------------------------------------------------------------------------------

def signs(y_idx, n_classes):
    """[N, C] float64 of +1 (class index == column) / -1."""
    y_idx = np.asarray(y_idx)
    return np.where(y_idx[:, None] == np.arange(n_classes)[None, :], 1.0, -1.0)


def _aug(X):
    X = np.asarray(X, dtype=np.float64)
    return np.hstack([X, np.ones((X.shape[0], 1))])


def objective_host(X, Y, Wb, C):
    """f_c of every class column, float64 [C]."""
    Wb = np.asarray(Wb, dtype=np.float64)
    T = np.maximum(0.0, 1.0 - Y * (_aug(X) @ Wb.T))
    return 0.5 * np.sum(Wb * Wb, axis=1) + C * np.sum(T * T, axis=0)


def gradient_host(X, Y, Wb, C):
    """grad f_c, float64 [C, D + 1] (bias component last)."""
    Xa, Wb = _aug(X), np.asarray(Wb, dtype=np.float64)
    T = np.maximum(0.0, 1.0 - Y * (Xa @ Wb.T))
    return Wb + (-2.0 * C * Y * T).T @ Xa


def hessian_vector_host(X, Y, Wb, V, C):
    """Generalised Hessian of f_c at Wb times V: V + 2C X_I^T X_I V (I: the samples with 1 - y m > 0), float64 [C, D + 1]."""
    Xa, Wb, V = _aug(X), np.asarray(Wb, dtype=np.float64), np.asarray(V, dtype=np.float64)
    A = (1.0 - Y * (Xa @ Wb.T)) > 0.0
    return V + (np.where(A, 2.0 * C * (Xa @ V.T), 0.0)).T @ Xa


class _HostOps:
    """The solver's primitives in NumPy float64 (rows = the working set's class columns)."""
    f_rtol = 1e-14

    def __init__(self, X, y_idx, C, n_classes):
        self.Xa, self.y, self.C = _aug(X), np.asarray(y_idx), float(C)
        self.width = self.Xa.shape[1]
        self.cols = np.arange(n_classes)

    def set_columns(self, cols):
        self.cols = np.asarray(cols)
        self.Y = np.where(self.y[:, None] == self.cols[None, :], 1.0, -1.0)

    def zeros(self, rows):
        return np.zeros((rows, self.width))

    def fg(self, W):
        T = 1.0 - self.Y * (self.Xa @ W.T)
        self.A = T > 0.0
        Tp = np.where(self.A, T, 0.0)
        f = 0.5 * np.sum(W * W, axis=1) + self.C * np.sum(Tp * Tp, axis=0)
        G = W + (-2.0 * self.C * self.Y * Tp).T @ self.Xa
        return f, G, np.sum(G * G, axis=1)

    def hv(self, V):
        return V + np.where(self.A, 2.0 * self.C * (self.Xa @ V.T), 0.0).T @ self.Xa

    def gram(self, vecs):
        return np.stack([np.sum(vecs[a] * vecs[b], axis=1) for a in range(len(vecs)) for b in range(a, len(vecs))], axis=1)

    def axpby(self, alpha, x, beta, y):
        return alpha[:, None] * x + beta[:, None] * y

    def take(self, v, idx):
        return v[idx]

    def put(self, full, idx, part):
        full[idx] = part

    def to_host(self, v):
        return np.asarray(v[:, :self.width], dtype=np.float64)


class _DeviceOps:
    """The solver's primitives on the sehip SVM kernels.  Vectors are float32 [rows, ldv] device tensors (ldv = D + 1 rounded up
    to 4; the padding columns stay zero)."""
    f_rtol = 1e-6       # resolution of the float32 objective (relative)

    def __init__(self, X, y_idx, C, n_classes):
        import torch
        import sehip
        self.torch, self.sehip = torch, sehip
        self.X, self.C = X, float(C)
        self.dev = X.device
        self.N, self.D = X.shape
        self.width = self.D + 1
        self.ldv = (self.width + 3) // 4 * 4
        self.labels = torch.from_numpy(np.ascontiguousarray(y_idx, dtype=np.int32)).to(self.dev)
        self.Z = torch.empty((self.N, max(n_classes, MIN_COLUMNS)), dtype=torch.float32, device=self.dev)
        self.mask = torch.empty((self.N, (max(n_classes, MIN_COLUMNS) + 31) // 32), dtype=torch.int32, device=self.dev)
        self.nblk = sehip.ops.svm_loss_blocks(self.N)
        self.loss = torch.empty((max(n_classes, MIN_COLUMNS), self.nblk), dtype=torch.float32, device=self.dev)
        self.ws = None

    def set_columns(self, cols):
        self.cols = self.torch.from_numpy(np.ascontiguousarray(cols, dtype=np.int32)).to(self.dev)

    def zeros(self, rows):
        return self.torch.zeros((rows, self.ldv), dtype=self.torch.float32, device=self.dev)

    def _workspace(self, rows):
        need = self.sehip.svm_reduce_workspace_bytes(self.N, self.D, rows)
        if self.ws is None or self.ws.numel() < need:
            self.ws = None
            self.ws = self.torch.empty((need,), dtype=self.torch.uint8, device=self.dev)
        return self.ws

    def fg(self, W):
        sh, rows = self.sehip, W.shape[0]
        z = self.Z[:, :rows]
        sh.svm_margin(sh.SVM_GRAD, self.X, W, d=self.D, labels=self.labels, col_class=self.cols, cpen=self.C, mask=self.mask,
                      out=z, loss_part=self.loss[:rows])
        lsum = sh.svm_rowsum(self.loss[:rows], length=self.nblk)
        G = sh.svm_reduce(z, self.X, d=self.D, plus=W, out=self.zeros(rows), workspace=self._workspace(rows))
        gr = sh.svm_gram([W, G], length=self.width)
        host = self.torch.cat([lsum[:, None], gr], dim=1).cpu().numpy()        # the one read of an evaluation
        f = 0.5 * host[:, 1] + self.C * host[:, 0]
        return f, G, host[:, 3]

    def hv(self, V):
        sh, rows = self.sehip, V.shape[0]
        z = self.Z[:, :rows]
        sh.svm_margin(sh.SVM_HV, self.X, V, d=self.D, cpen=self.C, mask=self.mask, out=z)
        return sh.svm_reduce(z, self.X, d=self.D, plus=V, out=self.zeros(rows), workspace=self._workspace(rows))

    def gram(self, vecs):
        return self.sehip.svm_gram(vecs, length=self.width).cpu().numpy()

    def axpby(self, alpha, x, beta, y):
        ab = self.torch.from_numpy(np.stack([alpha, beta]).astype(np.float64)).pin_memory().to(self.dev, non_blocking=True)
        return self.sehip.svm_axpby(ab[0], x, ab[1], y, out=self.zeros(x.shape[0]), length=self.width)

    def take(self, v, idx):
        return v[self.torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(self.dev)]

    def put(self, full, idx, part):
        full[self.torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(self.dev)] = part

    def to_host(self, v):
        return v[:, :self.width].cpu().numpy()


def _tron(ops, n_classes, tol, max_iter, verbose=0):
    """Batched trust-region Newton over every class column.  Returns (W [n_classes, D + 1] in the ops' layout, n_iter [n_classes],
    converged [n_classes])."""
    W_full = ops.zeros(n_classes)
    ws = np.arange(n_classes)                       # class columns of the working set's rows
    ops.set_columns(ws)
    W = ops.zeros(n_classes)
    f, G, gg = ops.fg(W)
    gnorm0 = np.sqrt(gg)                            # per class column (the working set is all columns here)
    gnorm = gnorm0.copy()
    delta = gnorm.copy()
    first = np.ones(n_classes, bool)
    n_iter = np.zeros(n_classes, np.int64)
    done = gnorm <= tol * gnorm0
    frozen = np.zeros(n_classes, bool)
    converged = np.zeros(n_classes, bool)
    converged[done] = True
    while True:
        live = ~done & ~frozen
        if not live.any():
            break
        if live.sum() < len(ws):                    # compact: finished rows go home, the rest move up
            gone = np.nonzero(~live)[0]
            ops.put(W_full, ws[gone], ops.take(W, gone))
            keep = list(np.nonzero(live)[0])
            for i in gone:                           # pad to MIN_COLUMNS rows with finished ones (left unchanged)
                if len(keep) >= min(MIN_COLUMNS, n_classes):
                    break
                keep.append(i)
            keep = np.array(sorted(keep))
            W = ops.take(W, keep)
            ws, gnorm0, delta, first = ws[keep], gnorm0[keep], delta[keep], first[keep]
            frozen, done, live = ~live[keep], np.zeros(len(keep), bool), live[keep]
            ops.set_columns(ws)
            f, G, gg = ops.fg(W)
            gnorm = np.sqrt(gg)
        rows = len(ws)
        one, zero = np.ones(rows), np.zeros(rows)
        lv = live.astype(np.float64)

        # ---- truncated CG on the trust region (liblinear's trcg), every live row at once ----
        s = ops.zeros(rows)
        r = ops.axpby(-one, G, zero, G)
        d = ops.axpby(-one, G, zero, G)
        cgtol = 0.1 * gnorm
        cg = live.copy()
        cg_iters = np.zeros(rows, np.int64)
        max_cg = 4 * ops.width + 20
        while cg.any():
            Hd = ops.hv(d)
            q = ops.gram([s, d, r, Hd])                # ss sd sr sH dd dr dH rr rH HH: the one read of a CG step
            ss, sd, dd, dH, rr, rH, HH = q[:, 0], q[:, 1], q[:, 4], q[:, 6], q[:, 7], q[:, 8], q[:, 9]
            with np.errstate(divide="ignore", invalid="ignore"):
                alpha = np.where(cg, rr / dH, 0.0)
                dsq = delta * delta
                bnd = cg & (ss + 2.0 * alpha * sd + alpha * alpha * dd > dsq)
                rad = np.sqrt(np.maximum(sd * sd + dd * (dsq - ss), 0.0))
                ab = np.where(sd >= 0, (dsq - ss) / (sd + rad), (rad - sd) / dd)
                a = np.where(bnd, ab, alpha)
                a = np.where(cg & np.isfinite(a), a, 0.0)
                rnew = rr - 2.0 * a * rH + a * a * HH
                beta = np.where(rr > 0, rnew / rr, 0.0)
            cg_iters += cg
            cont = cg & ~bnd & (np.sqrt(np.maximum(rnew, 0.0)) > cgtol) & (cg_iters < max_cg)
            s = ops.axpby(one, s, a, d)
            r = ops.axpby(one, r, -a, Hd)
            d = ops.axpby(cont.astype(np.float64), r, np.where(cont, beta, 1.0), d)
            cg = cont

        # ---- trust-region step ----
        q = ops.gram([G, s, r])                         # gg gs gr ss sr rr
        gs, ss, sr = q[:, 1], q[:, 3], q[:, 4]
        prered = -0.5 * (gs - sr)
        snorm = np.sqrt(ss)
        Wn = ops.axpby(one, W, lv, s)
        fn, Gn, ggn = ops.fg(Wn)
        actred = f - fn
        delta = np.where(first & live, np.minimum(delta, snorm), delta)
        with np.errstate(divide="ignore", invalid="ignore"):
            den = fn - f - gs
            alpha = np.where(den <= 0, SIGMA3, np.maximum(SIGMA1, -0.5 * (gs / den)))
        noisy = np.abs(prered) <= ops.f_rtol * np.abs(f)
        accept = live & np.where(noisy, ggn < gg, actred > ETA0 * prered)
        nd = np.where(actred < ETA0 * prered, np.minimum(np.maximum(alpha, SIGMA1) * snorm, SIGMA2 * delta),
             np.where(actred < ETA1 * prered, np.maximum(SIGMA1 * delta, np.minimum(alpha * snorm, SIGMA2 * delta)),
             np.where(actred < ETA2 * prered, np.maximum(SIGMA1 * delta, np.minimum(alpha * snorm, SIGMA3 * delta)),
                      np.maximum(delta, np.minimum(alpha * snorm, SIGMA3 * delta)))))
        nd = np.where(noisy, np.where(accept, delta, SIGMA2 * np.minimum(delta, snorm)), nd)
        delta = np.where(live, nd, delta)
        first &= ~live
        n_iter[ws[live]] += 1
        if np.array_equal(accept, live):            # every live row moves: the trial's evaluation is the new one
            W, f, G, gg = Wn, np.where(live, fn, f), Gn, np.where(live, ggn, gg)
        else:
            acc = accept.astype(np.float64)
            W = ops.axpby(acc, Wn, 1.0 - acc, W)
            f, G, gg = ops.fg(W)
        gnorm = np.sqrt(gg)
        conv = live & accept & (gnorm <= tol * gnorm0)
        converged[ws[conv]] = True
        stuck = live & ~conv & ((np.abs(prered) <= 1e-15 * np.abs(f)) | (n_iter[ws] >= max_iter))
        if verbose:
            sys.stderr.write("tron: %d live classes, CG steps %d (max), |g| / |g0| max %.3e, accepted %d\n" % (
                live.sum(), cg_iters.max(), float(np.max(np.where(live, gnorm / np.maximum(gnorm0, 1e-300), 0.0))), accept.sum()))
        done = done | conv | stuck
    ops.put(W_full, ws, W)
    return W_full, n_iter, converged


def fit_host(X, y_idx, n_classes, C=1.0, tol=1e-4, max_iter=1000):
    """The solver of ``LinearSVC.fit`` on the float64 host statement: (Wb [C, D + 1], n_iter [C], converged [C])."""
    ops = _HostOps(X, y_idx, C, n_classes)
    W, n_iter, conv = _tron(ops, n_classes, tol, max_iter)
    return W, n_iter, conv


class LinearSVC:
    """scikit-learn's ``LinearSVC`` (defaults: squared hinge, L2 penalty, one-vs-rest, fit_intercept with intercept_scaling 1) fitted
    on the device.  ``X`` may be a NumPy array or a device tensor; it is used in float32 (scikit-learn uses float64).
    ``coef_`` [C, D] and ``intercept_`` [C] are float32; ``classes_`` is ``np.unique(y)``."""

    def __init__(self, C=1.0, tol=1e-4, max_iter=1000, verbose=0, penalty='l2', loss='squared_hinge', dual='auto',
                 multi_class='ovr', fit_intercept=True, intercept_scaling=1, class_weight=None, random_state=None):
        if penalty != 'l2' or loss != 'squared_hinge' or multi_class != 'ovr' or not fit_intercept or intercept_scaling != 1 \
                or class_weight is not None:
            raise NotImplementedError("only LinearSVC's defaults (penalty='l2', loss='squared_hinge', multi_class='ovr', "
                                      "fit_intercept=True, intercept_scaling=1, class_weight=None) are implemented")
        if not C > 0:
            raise ValueError("C must be positive")
        self.C, self.tol, self.max_iter, self.verbose = float(C), float(tol), int(max_iter), verbose
        self.dual, self.random_state = dual, random_state      # accepted for signature compatibility; the optimum is unique

    @staticmethod
    def _device_rows(X):
        import torch
        import sehip
        sehip._lib.require_gpu()
        dev = torch.device('cuda', torch.cuda.current_device())
        if torch.is_tensor(X):
            X = X.detach().to(device=dev, dtype=torch.float32)
            if X.dim() != 2 or X.stride(1) != 1:
                X = X.contiguous()
            return X
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2:
            raise ValueError("X must be 2-d")
        return torch.from_numpy(X).to(dev)

    def fit(self, X, y, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError("sample weights are not implemented")
        y = y.detach().cpu().numpy() if hasattr(y, 'detach') else np.asarray(y)
        self.classes_ = np.unique(y)
        if len(self.classes_) < 3:
            raise ValueError("LinearSVC on the device needs at least 3 classes, got %d (the reference ranks the columns of a "
                             "2-d decision_function, which a binary problem does not have)" % len(self.classes_))
        Xd = self._device_rows(X)
        if Xd.shape[0] != len(y):
            raise ValueError("X has %d rows, y %d labels" % (Xd.shape[0], len(y)))
        y_idx = np.searchsorted(self.classes_, y)
        ops = _DeviceOps(Xd, y_idx, self.C, len(self.classes_))
        W, n_iter, conv = _tron(ops, len(self.classes_), self.tol, self.max_iter, self.verbose)
        if not conv.all():
            warnings.warn("Liblinear-style solver did not converge for %d of %d classes within max_iter=%d; increase the number "
                          "of iterations." % (int((~conv).sum()), len(conv), self.max_iter), ConvergenceWarning)
        self._W, self._d = W, Xd.shape[1]
        host = ops.to_host(W)
        self.coef_ = np.ascontiguousarray(host[:, :-1])
        self.intercept_ = np.ascontiguousarray(host[:, -1])
        self.n_iter_ = int(n_iter.max()) if len(n_iter) else 0
        return self

    def decision_function(self, X, return_device=False):
        """Scores ``X coef_^T + intercept_`` [N, C] (float32, one MFMA pass)."""
        import sehip
        Xd = self._device_rows(X)
        if Xd.shape[1] != self._d:
            raise ValueError("X has %d features, the model %d" % (Xd.shape[1], self._d))
        S = sehip.svm_margin(sehip.SVM_SCORE, Xd, self._W, d=self._d)
        return S if return_device else S.cpu().numpy()

    def predict(self, X):
        return self.classes_[np.argmax(self.decision_function(X), axis=1)]
