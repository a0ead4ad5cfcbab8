"""The grid of the kernel-edge tests of csrc/kmeans.hip, shared by tests/test_kmeans_edges_gpu.py (which runs it on the
device) and tests/test_kmeans_cpu.py (which checks its preconditions on the host).  Hand-picked pairs of the extremes of
N in {1, 63, 64, 65, 1023, 1024, 1025, 5000, 130000}, K in {1, 2, 1000, 1024, 1025, 4096, 16384} and
D in {1, 3, 63, 64, 65, 127, 128, 129, 200, 511, 512}; every case is generated from its seed (kmeans_ref.lattice / planted).

The labels are an input of every case: they are drawn, never computed, so no fp32 argmin decides anything here."""
import numpy as np

import kmeans_ref as R

FAR = 40.0   # a lattice value outside [-16, 16]: such a row is farther from any old centre than every ordinary row

# (name, N, D, K, label maker, argument of the maker)
#   uniform / sorted: drawn labels (clusters that get no row are empty: about K e^(-N/K) of them)
#   blocks: one label per 1024-row block        one: every row in cluster <arg>
#   empty: <arg> chosen clusters (front, middle, end of the range) empty, every other one populated
#   dup / two / alone / still: <arg> chosen clusters empty and, in this order: the two farthest rows bit-identical and of one
#   label; two distinct far rows of one label; a far row that is the only row of its cluster; every row equal to its old
#   centre (nothing may move)
UPDATE_LATTICE = [
    ("n1", 1, 1, 1, "uniform", None),
    ("n63", 63, 3, 2, "uniform", None),
    ("n64_sorted", 64, 63, 2, "sorted", None),
    ("n65_one", 65, 65, 2, "one", 1),                    # cluster 0 empty
    ("n1023_k1000", 1023, 127, 1000, "uniform", None),   # hundreds of empty clusters, distance ties
    ("n1024_k1024_sorted", 1024, 128, 1024, "sorted", None),
    ("n1025_k1025", 1025, 129, 1025, "uniform", None),   # perk = 2; several hundred relocations
    ("n5000_d512", 5000, 512, 7, "uniform", None),
    ("n5000_k4096", 5000, 511, 4096, "uniform", None),   # perk = 4
    ("n5000_blocks", 5000, 64, 1000, "blocks", None),    # 995 empty; each 1024-row block shares one label
    ("n130000_blocks", 130000, 1, 2, "blocks", None),
    ("n130000_one", 130000, 65, 2, "one", 1),            # a cluster of 1016 segments; cluster 0 empty
    ("n130000_k4096_e7", 130000, 64, 4096, "empty", 7),
    ("n130000_k16384_e2", 130000, 3, 16384, "empty", 2),  # K * NB = 2 080 768 label counts
    ("n5000_k16384_all_but_one", 5000, 128, 16384, "one", 8191),  # K - 1 empty, the rows run out after 5000
    ("n5000_k1025_all_but_one", 5000, 129, 1025, "one", 512),     # K - 1 empty, 1024 relocations
    ("dup_e2", 1025, 3, 8, "dup", 2),
    ("dup_e7", 5000, 200, 1024, "dup", 7),
    ("two_e2", 1025, 63, 8, "two", 2),
    ("two_e7", 1024, 5, 16, "two", 7),
    ("alone_e1", 65, 3, 4, "alone", 1),
    ("alone_e2", 1023, 64, 1000, "alone", 2),
    ("still_e2", 1025, 129, 8, "still", 2),
    ("still_e7", 5000, 3, 1025, "still", 7),
]

# Gaussian rows (kmeans_ref.planted; the old centres are its init rows), same makers
UPDATE_GAUSS = [
    ("g65", 65, 511, 2, "uniform", None),
    ("g5000", 5000, 200, 7, "uniform", None),
    ("g1025_k1025", 1025, 129, 1025, "uniform", None),   # hundreds of relocations: needs the top_gaps precondition
    ("g130000_dup_e2", 130000, 64, 4096, "dup", 2),
    ("g5000_e7", 5000, 127, 1000, "empty", 7),
]

# (N, D, K): kmeans_inertia (labels uniform), kmeans_col_stats and kmeans_add_rows (N, D)
ROW_SHAPES = [(1, 1, 1), (63, 127, 2), (65, 3, 2), (1023, 129, 1025), (1024, 64, 1024), (5000, 512, 7),
              (130000, 64, 4096), (130000, 1, 16384)]

# (name, N, D, K, T, first, duplicate rows)
PLUSPLUS = [
    ("k1", 63, 1, 1, 1, 62, False),
    ("n63_all", 63, 127, 63, 2, 0, False),                # K = N
    ("n64_dups", 64, 129, 8, 2, 63, True),
    ("n65_d1_zero_potential", 65, 1, 65, 16, 0, False),   # at most 33 distinct rows: the potential reaches 0 before K
    ("n65_all", 65, 128, 65, 2, 64, False),
    ("n4097_t16", 4097, 512, 5, 16, 0, False),
    ("n4097_t1", 4097, 300, 3, 1, 4096, False),
    ("n4097_hit_block_end", 4097, 64, 2, 1, 5, False),    # the draw times the potential EQUALS the cumsum at the end of a
    ("n4097_hit_mid_block", 4097, 63, 2, 1, 4000, False), # 64-row block / at a row inside one: ">=" decides, not ">"
]

# vq_ema_stats (N, D, K, maker); vq_ema_update (K, D)
EMA_STATS = [(1, 1, 1, "uniform"), (5000, 129, 1023, "uniform"), (5000, 512, 1025, "sorted"), (130000, 1, 16384, "uniform"),
             (1023, 129, 16384, "uniform"), (130000, 64, 1025, "blocks")]
EMA_UPDATE = [(1, 1), (1, 512), (1023, 129), (1025, 512), (16384, 1), (16384, 129)]


def case_seed(name):
    return 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100000


def make_labels(seed, N, K, maker, arg):
    """-> (labels, the clusters left empty on purpose or None)."""
    if maker == "uniform":
        return R.labels_uniform(seed, N, K), None
    if maker == "sorted":
        return R.labels_sorted(seed, N, K), None
    if maker == "blocks":
        return R.labels_blocks(N, K), None
    if maker == "one":
        return R.labels_one(N, arg), np.setdiff1d(np.arange(K), [arg])
    empty = R.empty_clusters(K, arg)
    return R.labels_with_empty(seed, N, K, empty), empty


def plant_far_rows(X, C, labels, maker):
    """The special relocation cases, in place on X / labels (see UPDATE_LATTICE)."""
    N, D = X.shape
    if maker == "still":
        X[:] = C[labels]
        return
    sign = np.where(np.arange(D) % 2 == 0, 1.0, -1.0).astype(np.float32)
    a, b = N // 3, N - 2                       # b in the last (ragged) label block when N > 1024
    if maker == "dup":
        labels[b] = labels[a]
        X[a] = FAR * sign
        X[b] = X[a]
    elif maker == "two":
        labels[b] = labels[a]
        X[a] = FAR * sign
        X[b] = X[a]
        X[b, 0] -= 1.0
    elif maker == "alone":
        k = labels[a]
        others = np.flatnonzero((labels == k) & (np.arange(N) != a))
        spare = labels[(a + 1) % N] if labels[(a + 1) % N] != k else labels[np.flatnonzero(labels != k)[0]]
        labels[others] = spare
        X[a] = FAR * sign


def update_case(case, gauss=False):
    """-> (X (N, D) fp32, old centres (K, D) fp32, labels (N,) int64, n_empty: the number of clusters without a row)."""
    name, N, D, K, maker, arg = case
    seed = case_seed(name)
    if gauss:
        X, C = R.planted(seed, N, D, K)
    else:
        X, C = R.lattice(seed, N, D, K)
    base = {"dup": "empty", "two": "empty", "alone": "empty", "still": "empty"}.get(maker, maker)
    labels, _ = make_labels(seed + 1, N, K, base, arg)
    if base != maker:
        if gauss and maker == "dup":
            a, b = N // 3, N - 2
            labels[b] = labels[a]
            X[a] = C[labels[a]] + np.float32(100.0)
            X[b] = X[a]
        else:
            plant_far_rows(X, C, labels, maker)
    n_empty = int(K - np.unique(labels).size)
    return X, C, labels, n_empty


def plusplus_case(case):
    """-> (X, uniforms (K - 1, T) fp64 or None).  The draws hold 0.0 (first round) and 1 - 2^-53 (last round)."""
    name, N, D, K, T, first, dups = case
    seed = case_seed(name)
    X, _ = R.lattice(seed, N, D, 1)
    if dups:
        X[10:20] = X[first]
        X[40] = X[41]
    if K == 1:
        return X, None
    u = np.random.RandomState(seed + 2).uniform(size=(K - 1, T))
    u[0, 0] = 0.0
    u[-1, -1] = 1.0 - 2.0 ** -53
    if "_hit_" in name:
        u[0, 0] = exact_hit_draw(X, first, 63 if name.endswith("block_end") else 31)
    return X, u


def exact_hit_draw(X, first, lane):
    """A draw u with fl64(u * pot) == cumsum[j] exactly, for a row j = lane (mod 64) of non-zero distance to row ``first``
    past the first few blocks: the search must return j itself (the first entry >= the value)."""
    X64 = X.astype(np.float64)
    d = ((X64 - X64[first]) ** 2).sum(1)
    cs = np.cumsum(d)
    pot = cs[-1]
    for j in range(5 * 64 + lane, X.shape[0] - 64, 64):
        u = cs[j] / pot
        if d[j] > 0 and u * pot == cs[j]:
            return u
    raise AssertionError("no exact hit")
