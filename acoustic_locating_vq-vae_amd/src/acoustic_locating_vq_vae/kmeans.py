"""k-means on the device: ``KMeans``, with sklearn.cluster.KMeans(algorithm="lloyd") semantics (csrc/kmeans.hip).

The use it was written for is the codebook initialisation of the quantiser (``ConvolutionalVQVAE.init_codebook``,
``Trainer.init_codebook``); it is also a general tool for analysing latents and codes, next to ``TSNE``.

The contract, as sklearn 1.7 states it for dense input without sample weights:

1. X (N, D) float GPU tensor (fp32 on the device; there is no CPU fallback: a CPU tensor raises).  N < n_clusters raises
   ValueError.  X is centred by its column means for the run (sklearn's accuracy step) and the centres shifted back.
2. ``tol`` becomes ``mean(var(X, axis=0)) * tol``.
3. ``init="k-means++"``: greedy k-means++ with ``n_local_trials = 2 + int(log(K))``: the first centre is a uniformly drawn
   row; ``closest_dist_sq`` (fp64) and ``current_pot`` = its sum; per round, T uniforms x ``current_pot`` are searched in
   the inclusive cumsum of ``closest_dist_sq`` (first entry >= the value, clipped to N - 1), each candidate's potential is
   sum(min(closest_dist_sq, d(candidate, .))), and the candidate of least potential (lowest on ties) becomes the next
   centre.  ``init`` as an array / tensor of shape (K, D) is used as given.  ``init="random"`` is not implemented.
4. Lloyd, per iteration i: (1) assign every row to its nearest centre (the quantiser's argmin, lowest index on ties);
   (2) update: each centre = the mean of its rows; (3) relocate empty clusters (sklearn's _relocate_empty_clusters_dense:
   the rows farthest from the OLD centre of their label move to the empty clusters, their values leave their old
   cluster's sum; nothing moves when every distance is 0); (4) stop on strict convergence (labels unchanged since the
   previous iteration), else when ``center_shift_tot = sum |c_new - c_old|^2 <= tol``.  Without strict convergence one
   more assignment makes the labels match the final centres.  ``n_iter_ = i + 1``.  ``inertia_`` = sum |x - c_label|^2.
5. ``n_init="auto"``: 1 run (for k-means++ and for an explicit init).  With ``n_init > 1`` the run of least inertia is
   kept, the first one on ties (an explicit init runs once, with a RuntimeWarning, as sklearn does).
6. ``predict(X)``: the nearest of ``cluster_centers_``.

At most one host read per Lloyd iteration (the convergence verdict), plus one per run (the inertia) and one per fit (the
tolerance).  Every sum runs in one fixed order: two fits of the same input are bitwise identical.

Deliberate differences from sklearn:

* k-means++ draws come from a ``torch.Generator`` seeded by ``random_state`` (a fresh seed when None), so the stream
  differs from numpy's: the same seed gives other centres than sklearn.  ``_kmeans_plusplus`` takes injected draws.
* The assignment's distance is the quantiser's ``fl32(fl32(|x|^2 + |c|^2) - 2 x.c)``, not sklearn's ``|c|^2 - 2 x.c``:
  labels agree except at near-ties.
* Centres are summed in fp64 (sklearn: in the input's dtype), k-means++ distances are fp64 sums of fp64 differences, and
  its cumsum is blocked (64-row block sums, then a scan inside the block).
* Empty-cluster relocation has a defined order: rows by distance descending, ties to the lower row index, paired with the
  empty clusters in ascending order (sklearn takes the farthest rows from ``argpartition``, in no defined order), so
  parity with sklearn is exact only when one cluster is empty per iteration.
* ``n_init > 1`` compares inertias only (sklearn also keeps the first run when a better one is the same clustering).
"""
import math
import warnings

import numpy as np
import torch

from . import _native as N

_MAX_K = 16384
_MAX_D = 512


def _as_rows(X, name="X"):
    if not isinstance(X, torch.Tensor):
        raise TypeError("%s must be a torch tensor on the GPU (got %s)" % (name, type(X).__name__))
    if not X.is_cuda:
        raise RuntimeError("%s must live on the GPU (got %s); k-means has no CPU fallback" % (name, X.device))
    if X.dim() != 2:
        raise ValueError("%s must be (N, D) (got %s)" % (name, tuple(X.shape)))
    if not X.is_floating_point():
        raise TypeError("%s must be a float tensor (got %s)" % (name, X.dtype))
    return X.detach().to(torch.float32).contiguous()


def _kmeans_plusplus(X, K, first, uniforms):
    """Greedy k-means++ of the rows of X (N, D) fp32 with injected draws: ``first`` the first centre's row, ``uniforms``
    (K-1, T) in [0, 1).  -> (centres (K, D) fp32, indices (K,) int64), on X's device."""
    X = _as_rows(X)
    u = None
    if K > 1:
        u = torch.as_tensor(np.asarray(uniforms) if not isinstance(uniforms, torch.Tensor) else uniforms)
        u = u.to(device=X.device, dtype=torch.float64).contiguous()
    return N.kmeans_plusplus(X, int(K), int(first), u)


class KMeans:
    """sklearn.cluster.KMeans(algorithm="lloyd") on the device; the contract and its deliberate differences: the module
    docstring."""

    def __init__(self, n_clusters=8, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, random_state=None,
                 algorithm="lloyd"):
        if not isinstance(n_clusters, (int, np.integer)) or isinstance(n_clusters, bool) or n_clusters < 1:
            raise ValueError("n_clusters must be an integer >= 1 (got %r)" % (n_clusters,))
        if n_clusters > _MAX_K:
            raise ValueError("n_clusters=%d > %d is not supported" % (n_clusters, _MAX_K))
        if isinstance(init, str):
            if init == "random":
                raise NotImplementedError("init='random' is not implemented (use 'k-means++' or an array)")
            if init != "k-means++":
                raise ValueError("init must be 'k-means++' or an array of shape (n_clusters, n_features) (got %r)" % init)
        elif not isinstance(init, (torch.Tensor, np.ndarray)):
            raise TypeError("init must be 'k-means++' or an array / tensor (got %s)" % type(init).__name__)
        if n_init != "auto" and (not isinstance(n_init, (int, np.integer)) or isinstance(n_init, bool) or n_init < 1):
            raise ValueError("n_init must be 'auto' or an integer >= 1 (got %r)" % (n_init,))
        if not isinstance(max_iter, (int, np.integer)) or isinstance(max_iter, bool) or max_iter < 1:
            raise ValueError("max_iter must be an integer >= 1 (got %r)" % (max_iter,))
        if not (isinstance(tol, (int, float, np.floating)) and not isinstance(tol, bool) and tol >= 0):
            raise ValueError("tol must be a number >= 0 (got %r)" % (tol,))
        if algorithm != "lloyd":
            raise NotImplementedError("algorithm=%r is not implemented (only 'lloyd')" % (algorithm,))
        self.n_clusters, self.init, self.n_init, self.max_iter = int(n_clusters), init, n_init, int(max_iter)
        self.tol, self.random_state, self.algorithm = float(tol), random_state, algorithm

    # -------------------------------------------------------------------------------------------------------------
    def _generator(self):
        g = torch.Generator()
        if self.random_state is None:
            g.seed()
        else:
            g.manual_seed(int(self.random_state))
        return g

    def _check_input(self, X):
        X = _as_rows(X)
        n, d = X.shape
        if n < self.n_clusters:
            raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n, self.n_clusters))
        if d > _MAX_D:
            raise ValueError("n_features=%d > %d is not supported" % (d, _MAX_D))
        return X

    def _init_array(self, X):
        init = self.init
        init = init.detach() if isinstance(init, torch.Tensor) else torch.as_tensor(np.asarray(init))
        init = init.to(device=X.device, dtype=torch.float32).contiguous()
        if tuple(init.shape) != (self.n_clusters, X.shape[1]):
            raise ValueError("init should be of shape (%d, %d) (got %s)" % (self.n_clusters, X.shape[1], tuple(init.shape)))
        return init

    def _lloyd(self, Xc, centers, tol):
        """One run from ``centers`` (centred space) -> (labels, inertia (1,) fp64 device, centres, n_iter)."""
        K, D = centers.shape
        dev = Xc.device
        spare = torch.empty_like(centers)
        stats = torch.empty((1,), device=dev, dtype=torch.float64)
        flags = torch.empty((4,), device=dev, dtype=torch.int32)
        flags_host = torch.empty((4,), dtype=torch.int32, pin_memory=True)
        ws = None
        labels_old = None
        strict = False
        for i in range(self.max_iter):
            labels = N.vq_argmin(Xc, centers)
            ws = N.kmeans_update(Xc, labels, labels_old, centers, spare, None, stats, flags, tol, ws)
            centers, spare = spare, centers
            flags_host.copy_(flags)            # the iteration's one host read: the verdict
            verdict = int(flags_host[0])
            if verdict == 1:
                strict = True
                break
            if verdict == 2:
                break
            labels_old = labels
        if not strict:
            labels = N.vq_argmin(Xc, centers)
        return labels, N.kmeans_inertia(Xc, labels, centers), centers, i + 1

    def fit(self, X, y=None):
        X = self._check_input(X)
        K = self.n_clusters
        mean, var_mean = N.kmeans_col_stats(X)
        tol = float(var_mean.item()) * self.tol if self.tol != 0 else 0.0
        Xc = N.kmeans_add_rows(X, mean, -1.0)
        explicit = not isinstance(self.init, str)
        n_init = 1 if self.n_init == "auto" else int(self.n_init)
        if explicit and n_init != 1:
            warnings.warn("Explicit initial center position passed: performing only one init in KMeans instead of "
                          "n_init=%d." % n_init, RuntimeWarning, stacklevel=2)
            n_init = 1
        g = None if explicit else self._generator()
        T = 2 + int(math.log(K))
        best = None
        for _ in range(n_init):
            if explicit:
                init = N.kmeans_add_rows(self._init_array(X), mean, -1.0)
            else:
                first = int(torch.randint(X.shape[0], (1,), generator=g))
                u = torch.rand((K - 1, T), generator=g, dtype=torch.float64)
                init, _ = _kmeans_plusplus(Xc, K, first, u)
            labels, inertia, centers, n_iter = self._lloyd(Xc, init, tol)
            inertia = float(inertia.item())
            if best is None or inertia < best[1]:
                best = (labels, inertia, centers, n_iter)
        labels, inertia, centers, n_iter = best
        self.cluster_centers_ = N.kmeans_add_rows(centers, mean, 1.0)
        self.labels_ = labels
        self.inertia_ = inertia
        self.n_iter_ = n_iter
        self.n_features_in_ = X.shape[1]
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def predict(self, X):
        if not hasattr(self, "cluster_centers_"):
            raise RuntimeError("this KMeans instance is not fitted yet: call fit first")
        X = _as_rows(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError("X has %d features, but KMeans is expecting %d" % (X.shape[1], self.n_features_in_))
        return N.vq_argmin(X, self.cluster_centers_)
