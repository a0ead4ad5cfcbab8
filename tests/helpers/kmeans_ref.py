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
    the OLD centre of their label descending (ties to the lower row), paired with the empty clusters ascending.
    -> (number relocated, the (row, empty cluster) pairs in order).  The number is that of the pairs really made, which is
    what the contract's "clusters relocated" means: with fewer rows than empty clusters the pairing stops when the rows run
    out, and the clusters left over stay empty."""
    empty = np.flatnonzero(counts == 0)
    if empty.size == 0:
        return 0, []
    dist = ((X - centers_old[labels]) ** 2).sum(1)
    if dist.max() == 0:
        return 0, []
    order = np.lexsort((np.arange(X.shape[0]), -dist))[:empty.size]
    pairs = []
    for e, f in zip(empty, order):
        o = labels[f]
        sums[o] -= X[f]
        sums[e] = X[f]
        counts[e] = 1
        counts[o] -= 1
        pairs.append((int(f), int(e)))
    return len(pairs), pairs


def update(X, labels, centers_old, K, full=False):
    """One M-step: (centres, center_shift_tot, relocated); with ``full`` also (counts after relocation, number of empty
    clusters before it, the relocation's (row, empty cluster) pairs)."""
    D = X.shape[1]
    sums = np.zeros((K, D))
    np.add.at(sums, labels, X)
    counts = np.bincount(labels, minlength=K).astype(np.int64)
    n_empty = int((counts == 0).sum())
    moved, pairs = relocate(X, centers_old, sums, counts, labels)
    centers = sums.copy()
    nz = counts > 0
    centers[nz] = sums[nz] * (1.0 / counts[nz])[:, None]
    shift = np.sqrt(((centers - centers_old) ** 2).sum(1))
    if full:
        return centers, float((shift ** 2).sum()), moved, counts, n_empty, pairs
    return centers, float((shift ** 2).sum()), moved


def shift_of_rounded(centers, centers_old):
    """center_shift_tot as the device states it: the centres rounded to fp32 first, then sum_k sqrt(|c32 - c_old|^2)^2 in
    float64.  (``update`` returns the shift of the unrounded centres, which differs by about 1e-7 relative.)  The squares of
    one cluster are added in finalize_kernel's order (128 partial sums over d = t, t + 128, ..; two 64-wide butterflies;
    their sum), so that what is left to differ is the order of the K terms and the last bit of each."""
    c32 = np.asarray(centers, np.float64).astype(np.float32).astype(np.float64)
    sq = (c32 - np.asarray(centers_old, np.float64)) ** 2
    K, D = sq.shape
    pad = np.zeros((K, -(-D // 128) * 128))
    pad[:, :D] = sq
    pad = pad.reshape(K, -1, 128)
    acc = np.zeros((K, 128))
    for q in range(pad.shape[1]):
        acc = acc + pad[:, q, :]
    w = acc.reshape(K, 2, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w[:, :, :o] + w[:, :, o:2 * o]
    shift = np.sqrt(w[:, 0, 0] + w[:, 1, 0])
    return float((shift ** 2).sum())


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
    """Greedy k-means++ (sklearn's _kmeans_plusplus) with injected draws: first index, uniforms (K-1, T).  -> indices.
    The candidates' distances are taken one candidate at a time (no (T, N, D) temporary)."""
    X = np.asarray(X, np.float64)
    N = X.shape[0]
    idx = [int(first)]
    closest = ((X - X[first]) ** 2).sum(1)
    pot = closest.sum()
    for c in range(1, K):
        r = np.asarray(uniforms[c - 1]) * pot
        cand = np.minimum(np.searchsorted(np.cumsum(closest), r), N - 1)
        d = np.empty((cand.shape[0], N))
        for t, j in enumerate(cand):
            d[t] = np.minimum(closest, ((X - X[j]) ** 2).sum(1))
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


# ------------------------------------------------------------------------------------- inputs for the kernel-edge tests
def lattice(seed, N, D, K, lo=-16, hi=16):
    """Rows (N, D) and old centres (K, D), fp32, drawn from the integers in [lo, hi].  Every fp64 sum the kernels take of
    such data (cluster sums, squared distances, block sums, potentials) is an integer below 2^53, exact in any order."""
    rs = np.random.RandomState(seed)
    X = rs.randint(lo, hi + 1, size=(N, D)).astype(np.float32)
    C = rs.randint(lo, hi + 1, size=(K, D)).astype(np.float32)
    return X, C


def labels_uniform(seed, N, K):
    return np.random.RandomState(seed).randint(K, size=N).astype(np.int64)


def labels_sorted(seed, N, K):
    return np.sort(labels_uniform(seed, N, K))


def labels_blocks(N, K, block=1024):
    """One label per block of ``block`` rows (block b -> label b mod K)."""
    return ((np.arange(N) // block) % K).astype(np.int64)


def labels_one(N, k):
    """Every row in cluster k."""
    return np.full(N, k, np.int64)


def empty_clusters(K, n_empty):
    """``n_empty`` clusters of [0, K): runs at the front, in the middle and at the end of the range (1: cluster 0; 2: the
    first and the last)."""
    assert 0 <= n_empty < K
    front, end, mid = (n_empty + 2) // 3, (n_empty + 1) // 3, n_empty // 3
    m0 = front + (K - front - end - mid) // 2
    e = np.concatenate([np.arange(front), np.arange(m0, m0 + mid), np.arange(K - end, K)]).astype(np.int64)
    assert np.unique(e).size == n_empty
    return e


def labels_with_empty(seed, N, K, empty):
    """Uniform labels over the clusters not in ``empty``, each of which gets at least one row (N >= K - len(empty))."""
    rs = np.random.RandomState(seed)
    keep = np.setdiff1d(np.arange(K), np.asarray(empty, np.int64))
    assert N >= keep.size > 0
    lab = keep[rs.randint(keep.size, size=N)]
    lab[rs.permutation(N)[:keep.size]] = keep
    return lab.astype(np.int64)


def top_gaps(dist, n):
    """The relative gaps (d_i - d_{i+1}) / d_i between the n + 1 largest distances, in descending order (fewer when there
    are fewer rows).  A relocation of n clusters has an order the reference alone decides when every gap is either 0
    between bit-identical rows of one label (the tie goes to the lower row on both sides) or far above the rounding of an
    fp64 sum of D terms (1e-9 is asked)."""
    d = np.sort(np.asarray(dist, np.float64))[::-1][:n + 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(d[:-1] > 0, (d[:-1] - d[1:]) / d[:-1], 0.0)


def relocation_order_is_decided(X, labels, centers_old, n, gap=1e-9):
    """top_gaps' precondition for the n farthest rows: each gap >= ``gap``, or exactly 0 between identical rows of one
    label."""
    X = np.asarray(X, np.float64)
    dist = ((X - np.asarray(centers_old, np.float64)[labels]) ** 2).sum(1)
    order = np.lexsort((np.arange(X.shape[0]), -dist))[:n + 1]
    for a, b, g in zip(order[:-1], order[1:], top_gaps(dist, n)):
        same = labels[a] == labels[b] and np.array_equal(X[a], X[b])
        if not (g >= gap or (g == 0 and same)):
            return False
    return True


def add_rows_both(x, v, alpha):
    """fp32 x + alpha * v[None, :] as a device may round it: (product rounded to fp32, then the sum rounded; the fused
    multiply-add, rounded once).  alpha is taken as the fp32 value the entry point receives."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    p = np.float64(np.float32(alpha)) * np.asarray(v, np.float32).astype(np.float64)[None, :]   # exact: 24 x 24 bits
    plain = (x64 + p.astype(np.float32).astype(np.float64)).astype(np.float32)                 # exact fp64 sum of two fp32
    s = x64 + p
    bb = s - x64
    err = (x64 - (s - bb)) + (p - bb)                 # TwoSum: x64 + p = s + err exactly
    fused = s.astype(np.float32)
    # s is the fp64 nearest the true sum, so the fp32 rounding of the two differs only when s sits on an fp32 midpoint
    f64 = fused.astype(np.float64)
    up = np.nextafter(fused, np.float32(np.inf))
    dn = np.nextafter(fused, np.float32(-np.inf))
    fused = np.where((s == 0.5 * (f64 + up.astype(np.float64))) & (err > 0), up, fused)
    fused = np.where((s == 0.5 * (f64 + dn.astype(np.float64))) & (err < 0), dn, fused)
    return plain, fused.astype(np.float32)


def ulp_distance(a, b):
    """Elementwise distance of two fp32 arrays in units in the last place (the number of fp32 values between them)."""
    def key(t):
        i = np.ascontiguousarray(t, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
