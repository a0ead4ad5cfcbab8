"""Float64 numpy restatement of k-means as acoustic_locating_vq_vae/kmeans.py states it (sklearn.cluster.KMeans(
algorithm="lloyd") semantics), written from the description, for the tests of csrc/kmeans.hip: Lloyd's iteration with the
empty-cluster relocation in its defined order, and greedy k-means++ with injected draws."""
import numpy as np


def tolerance(X, tol):
    """sklearn's _tolerance: mean(var(X, axis=0)) * tol."""
    if tol == 0:
        return 0.0
    return float(np.mean(np.var(np.asarray(X, np.float64), axis=0)) * tol)


def assign(X, C):
    """Labels (lowest index on ties) and the squared distances to the nearest centre."""
    xx = (X * X).sum(1)
    cc = (C * C).sum(1)
    d = np.maximum(xx[:, None] + cc[None, :] - 2.0 * X @ C.T, 0.0)
    lab = np.argmin(d, axis=1)
    return lab, d[np.arange(X.shape[0]), lab]


def relocate(X, centers_old, sums, counts, labels):
    """sklearn's _relocate_empty_clusters_dense on (sums, counts), in place, with the package's order: rows by distance to
    the OLD centre of their label descending (ties to the lower row), paired with the empty clusters ascending.  Returns the
    number relocated."""
    empty = np.flatnonzero(counts == 0)
    if empty.size == 0:
        return 0
    dist = ((X - centers_old[labels]) ** 2).sum(1)
    if dist.max() == 0:
        return 0
    order = np.lexsort((np.arange(X.shape[0]), -dist))[:empty.size]
    for e, f in zip(empty, order):
        o = labels[f]
        sums[o] -= X[f]
        sums[e] = X[f]
        counts[e] = 1
        counts[o] -= 1
    return int(empty.size)


def update(X, labels, centers_old, K):
    """One M-step: (centres, center_shift_tot, relocated)."""
    D = X.shape[1]
    sums = np.zeros((K, D))
    np.add.at(sums, labels, X)
    counts = np.bincount(labels, minlength=K).astype(np.int64)
    moved = relocate(X, centers_old, sums, counts, labels)
    centers = sums.copy()
    nz = counts > 0
    centers[nz] = sums[nz] * (1.0 / counts[nz])[:, None]
    shift = np.sqrt(((centers - centers_old) ** 2).sum(1))
    return centers, float((shift ** 2).sum()), moved


def lloyd(X, centers_init, max_iter=300, tol=0.0, trace=None):
    """sklearn's _kmeans_single_lloyd on (already centred) X with an absolute tol.  -> (labels, inertia, centres, n_iter).
    ``trace``: a list that receives the number of clusters relocated in each iteration."""
    X = np.asarray(X, np.float64)
    C = np.asarray(centers_init, np.float64).copy()
    K = C.shape[0]
    labels_old = np.full(X.shape[0], -1)
    strict = False
    for i in range(max_iter):
        labels, _ = assign(X, C)
        C_new, shift_tot, moved = update(X, labels, C, K)
        if trace is not None:
            trace.append(moved)
        C = C_new
        if np.array_equal(labels, labels_old):
            strict = True
            break
        if shift_tot <= tol:
            break
        labels_old = labels
    if not strict:
        labels, _ = assign(X, C)
    inertia = float(((X - C[labels]) ** 2).sum())
    return labels, inertia, C, i + 1


def kmeans_plusplus(X, K, first, uniforms):
    """Greedy k-means++ (sklearn's _kmeans_plusplus) with injected draws: first index, uniforms (K-1, T).  -> indices."""
    X = np.asarray(X, np.float64)
    N = X.shape[0]
    idx = [int(first)]
    closest = ((X - X[first]) ** 2).sum(1)
    pot = closest.sum()
    for c in range(1, K):
        r = np.asarray(uniforms[c - 1]) * pot
        cand = np.minimum(np.searchsorted(np.cumsum(closest), r), N - 1)
        d = ((X[None, :, :] - X[cand][:, None, :]) ** 2).sum(-1)
        d = np.minimum(closest[None, :], d)
        pots = d.sum(1)
        b = int(np.argmin(pots))
        pot = pots[b]
        closest = d[b]
        idx.append(int(cand[b]))
    return np.array(idx)


def fit(X, init, max_iter=300, tol=1e-4, trace=None):
    """KMeans(init=<array>, n_init=1).fit(X): centre X by its column mean, run Lloyd, shift the centres back.
    -> (labels, inertia, centres, n_iter)."""
    X = np.asarray(X, np.float64)
    mean = X.mean(0)
    labels, inertia, C, n_iter = lloyd(X - mean, np.asarray(init, np.float64) - mean, max_iter, tolerance(X, tol), trace)
    return labels, inertia, C + mean, n_iter


def planted(seed, N, D, K, spread=4.0, noise=1.0, far=None):
    """The golden cases' data, regenerated from the frozen legacy RandomState stream: K planted centres, N float32 rows
    around them, and an init of K distinct rows (row ``far`` of it moved far away from every row, so that its cluster
    starts empty)."""
    rs = np.random.RandomState(seed)
    centres = rs.randn(K, D) * spread
    lab = rs.randint(K, size=N)
    X = (centres[lab] + rs.randn(N, D) * noise).astype(np.float32)
    init = X[rs.permutation(N)[:K]].copy()
    if far is not None:
        init[far] = (X.mean(0) + 100.0 * spread).astype(np.float32)
    return X, init


def checksum(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
