"""k-means without a GPU: the float64 restatement (tests/helpers/kmeans_ref.py) pinned against scikit-learn itself on the
golden cases and on random ones, the golden data's checksums, the KMeans constructor's and input refusals, and the argument
errors of every alvq_kmeans_* entry point, which must fail before anything is launched; and the preconditions of the
kernel-edge grid (tests/helpers/kmeans_edge_cases.py, run on the device by tests/test_kmeans_edges_gpu.py): lattice sums and
distances exact in float64, the label makers, the relocation pairs and their count, the top_gaps precondition of the
Gaussian relocation cases, and the two roundings of add_rows."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import kmeans_ref as R  # noqa: E402
from acoustic_locating_vq_vae import kmeans as KM  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "g9_kmeans.npz")
LLOYD = ["l64k16", "l128k16", "l64k256", "l128k256", "empty"]
PLUSPLUS = ["pp32k64", "pp128k256"]


@pytest.fixture(scope="module")
def native():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native
    return _native


def lloyd_case(g, name):
    N, D, K, far = (int(v) for v in g[name + "_shape"])
    X, init = R.planted(int(g[name + "_seed"]), N, D, K, far=None if far < 0 else far)
    assert R.checksum(X) == str(g[name + "_sha"])
    return X, init


def test_golden_data_regenerates_and_restatement_matches_sklearn_outputs():
    g = np.load(GOLD)
    for name in LLOYD:
        X, init = lloyd_case(g, name)
        trace = []
        lab, inertia, C, n_iter = R.fit(X, init, trace=trace)
        assert np.array_equal(lab, g[name + "_labels"]), name
        assert n_iter == int(g[name + "_n_iter"]), name
        assert abs(inertia - float(g[name + "_inertia"])) <= 1e-9 * inertia, name
        assert np.linalg.norm(C - g[name + "_centers"]) <= 1e-6 * np.linalg.norm(C), name
        if name == "empty":
            assert trace[0] == 1 and max(trace) == 1
    for name in PLUSPLUS:
        N, D, K = (int(v) for v in g[name + "_shape"])
        X, _ = R.planted(int(g[name + "_seed"]), N, D, 3 * K, spread=2.0)
        assert R.checksum(X) == str(g[name + "_sha"])
        idx = R.kmeans_plusplus(X, K, int(g[name + "_first"]), g[name + "_uniforms"])
        assert np.array_equal(idx, g[name + "_indices"]), name
        assert g[name + "_uniforms"].shape == (K - 1, 2 + int(np.log(K)))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_against_sklearn_random_cases(seed):
    sk = pytest.importorskip("sklearn.cluster")
    rs = np.random.RandomState(100 + seed)
    N, D, K = 600 + 100 * seed, 8 * seed, 5 + 3 * seed
    X, init = R.planted(100 + seed, N, D, K)
    km = sk.KMeans(n_clusters=K, init=init.astype(np.float64), n_init=1, algorithm="lloyd").fit(X.astype(np.float64))
    lab, inertia, C, n_iter = R.fit(X, init)
    assert np.array_equal(lab, km.labels_) and n_iter == km.n_iter_
    assert abs(inertia - km.inertia_) <= 1e-9 * inertia
    np.testing.assert_allclose(C, km.cluster_centers_, rtol=0, atol=1e-9 * np.abs(C).max())
    # k-means++ with sklearn's own draws replayed
    Xp = rs.randn(400, 6)
    T = 2 + int(np.log(K))
    r2 = np.random.RandomState(seed)
    first = r2.choice(400, p=np.ones(400) / 400)
    u = np.stack([r2.uniform(size=T) for _ in range(K - 1)])
    _, want = sk.kmeans_plusplus(Xp, K, random_state=seed)
    assert np.array_equal(R.kmeans_plusplus(Xp, K, first, u), want)


def test_restatement_relocates_exactly_one_empty_cluster_like_sklearn():
    sk = pytest.importorskip("sklearn.cluster")
    X, init = R.planted(7, 500, 4, 6, far=2)
    trace = []
    lab, inertia, C, n_iter = R.fit(X, init, trace=trace)
    km = sk.KMeans(n_clusters=6, init=init.astype(np.float64), n_init=1, algorithm="lloyd").fit(X.astype(np.float64))
    assert trace[0] == 1
    assert np.array_equal(lab, km.labels_) and n_iter == km.n_iter_


def test_constructor_refusals():
    for kw in ({"n_clusters": 0}, {"n_clusters": 2.5}, {"n_clusters": 20000}, {"init": "bogus"}, {"n_init": 0},
               {"n_init": "many"}, {"max_iter": 0}, {"tol": -1.0}):
        with pytest.raises(ValueError):
            KM.KMeans(**kw)
    with pytest.raises(NotImplementedError):
        KM.KMeans(init="random")
    with pytest.raises(NotImplementedError):
        KM.KMeans(algorithm="elkan")
    with pytest.raises(TypeError):
        KM.KMeans(init=[[0.0]])


def test_input_refusals_without_a_gpu():
    km = KM.KMeans(n_clusters=3)
    with pytest.raises(RuntimeError, match="GPU"):
        km.fit(torch.zeros(10, 4))                 # no CPU fallback
    with pytest.raises(TypeError):
        km.fit(np.zeros((10, 4), np.float32))
    with pytest.raises(RuntimeError, match="not fitted"):
        KM.KMeans().predict(torch.zeros(3, 2))


def test_kmeans_entry_points_reject_bad_arguments_before_any_launch(native):
    lib = native.lib()
    names = [n for n in native.EXPORTS if n.startswith("alvq_kmeans_")]
    assert len(names) == 9
    for name in names:
        res, args = native._SIGNATURES[name]
        if res is not native._i32:
            continue
        vals = [0.0 if a in (ctypes.c_float, ctypes.c_double) else (0 if a in (ctypes.c_int, ctypes.c_int64) else None)
                for a in args]
        rc = getattr(lib, name)(*vals)
        assert rc < 0 and lib.alvq_last_error().startswith(name.encode()), name
    # zero sizes with non-null pointers
    p = ctypes.c_void_p(16)
    assert lib.alvq_kmeans_update_f32(p, p, None, p, ctypes.c_void_p(32), None, p, p, p, 0, 4, 4, 0.0, None) == -1
    assert lib.alvq_kmeans_update_f32(p, p, None, p, p, None, p, p, p, 8, 4, 4, 0.0, None) == -1   # centres aliased
    assert lib.alvq_kmeans_inertia_f32(p, p, p, p, p, 8, 0, 4, None) == -1
    assert lib.alvq_kmeans_col_stats_f32(p, p, p, p, 8, 0, None) == -1
    assert lib.alvq_kmeans_add_rows_f32(p, p, p, 0, 4, 1.0, None) == -1
    assert lib.alvq_kmeans_plusplus_f32(p, p, p, p, p, 8, 9, 4, 3, 0, None) == -1        # K > N
    assert lib.alvq_kmeans_plusplus_f32(p, p, p, p, p, 8, 4, 4, 17, 0, None) == -2       # T > 16
    assert lib.alvq_kmeans_plusplus_f32(p, p, p, p, p, 8, 4, 4, 3, 8, None) == -1        # first out of range
    assert lib.alvq_kmeans_update_f32(p, p, None, p, ctypes.c_void_p(32), None, p, p, p, 8, 20000, 4, 0.0, None) == -2
    assert lib.alvq_kmeans_update_workspace_bytes(8, 4, 513) == -1
    assert lib.alvq_kmeans_plusplus_workspace_bytes(8, 0) == -1
    assert lib.alvq_kmeans_inertia_workspace_bytes(10) == 80


# ------------------------------------------------------------------ preconditions of tests/test_kmeans_edges_gpu.py
import kmeans_edge_cases as E  # noqa: E402


def _int_sums(Xi, labels, K):
    s = np.zeros((K, Xi.shape[1]), np.int64)
    np.add.at(s, labels, Xi)
    return s


@pytest.mark.parametrize("case", E.UPDATE_LATTICE, ids=[c[0] for c in E.UPDATE_LATTICE])
def test_lattice_update_cases_are_exact_in_float64(case):
    """Cluster sums and row distances of the restatement equal int64 arithmetic, and the clusters the maker promises to
    leave empty are exactly the empty ones."""
    name, N, D, K, maker, arg = case
    X, C, labels, n_empty = E.update_case(case)
    assert X.dtype == np.float32 and C.dtype == np.float32 and labels.dtype == np.int64
    assert X.shape == (N, D) and C.shape == (K, D) and labels.shape == (N,)
    assert labels.min() >= 0 and labels.max() < K
    Xi, Ci = X.astype(np.int64), C.astype(np.int64)
    assert np.array_equal(Xi.astype(np.float32), X) and np.array_equal(Ci.astype(np.float32), C)
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    sums = np.zeros((K, D))
    np.add.at(sums, labels, X64)
    assert np.array_equal(sums, _int_sums(Xi, labels, K).astype(np.float64))
    dist_i = ((Xi - Ci[labels]) ** 2).sum(1)
    assert np.array_equal(((X64 - C64[labels]) ** 2).sum(1), dist_i.astype(np.float64))
    assert int(dist_i.sum()) < 2 ** 53 and np.abs(Xi).sum() < 2 ** 53
    counts = np.bincount(labels, minlength=K)
    assert n_empty == int((counts == 0).sum())
    if maker in ("empty", "dup", "two", "still", "alone"):
        assert n_empty == arg, name
    if maker == "empty":
        want = E.R.empty_clusters(K, arg)
        assert np.array_equal(np.flatnonzero(counts == 0), want)
    if maker == "one":
        assert n_empty == K - 1 and counts[arg] == N
    # what the special cases are there for
    centres, shift, moved, cnt, ne, pairs = R.update(X64, labels, C64, K, full=True)
    assert cnt.sum() == N and moved == min(ne, N) * (0 if maker == "still" else 1)
    rows = [p[0] for p in pairs]
    a, b = N // 3, N - 2
    if maker == "dup":
        assert rows[:2] == [a, b] and np.array_equal(X[a], X[b]) and dist_i[a] == dist_i[b]
    if maker == "two":
        assert rows[:2] == [a, b] and labels[a] == labels[b] and dist_i[a] > dist_i[b]
    if maker == "alone":
        assert rows[0] == a and counts[labels[a]] == 1 and cnt[labels[a]] == 0
        assert not centres[labels[a]].any()
    if maker == "still":
        assert dist_i.max() == 0 and pairs == [] and ne == arg
    if name in ("n1023_k1000", "n1025_k1025"):
        d = np.sort(dist_i)[::-1][:moved + 1]
        assert moved > 300 and (d[:-1] == d[1:]).any()       # relocations through exact distance ties


def test_lattice_row_and_plusplus_cases_are_exact_in_float64():
    for N, D, K in E.ROW_SHAPES:
        X, C = R.lattice(N + D + K, N, D, K)
        lab = R.labels_uniform(N + D, N, K)
        Xi, Ci = X.astype(np.int64), C.astype(np.int64)
        d = ((X.astype(np.float64) - C.astype(np.float64)[lab]) ** 2).sum(1)
        assert float(d.sum()) == float(((Xi - Ci[lab]) ** 2).sum())
        assert np.array_equal(X.astype(np.float64).sum(0), Xi.sum(0).astype(np.float64))
    for case in E.PLUSPLUS:
        name, N, D, K, T, first, dups = case
        X, u = E.plusplus_case(case)
        Xi = X.astype(np.int64)
        assert (u is None) == (K == 1) and (u is None or u.shape == (K - 1, T))
        if u is not None:
            assert u.max() < 1.0
            if "_hit_" in name:                                   # the draw lands exactly on a cumsum entry
                d = ((X.astype(np.float64) - X.astype(np.float64)[first]) ** 2).sum(1)
                j = int(np.searchsorted(np.cumsum(d), u[0, 0] * d.sum()))
                assert np.cumsum(d)[j] == u[0, 0] * d.sum() and d[j] > 0 and j % 64 == (63 if "block_end" in name else 31)
                assert j > 320 and R.kmeans_plusplus(X, K, first, u)[1] == j
            else:
                assert u[0, 0] == 0.0 and u[-1, -1] == 1.0 - 2.0 ** -53
        for j in (first, 0, N - 1):
            d = ((X.astype(np.float64) - X.astype(np.float64)[j]) ** 2).sum(1)
            di = ((Xi - Xi[j]) ** 2).sum(1)
            assert np.array_equal(d, di.astype(np.float64)) and float(np.cumsum(d)[-1]) == float(di.sum())
        idx = R.kmeans_plusplus(X, K, first, u)
        assert idx.shape == (K,) and idx[0] == first
        if name == "n65_d1_zero_potential":
            seen = np.unique(X[idx[:40]]).size
            assert seen == np.unique(X).size and (idx[40:] == 0).all()   # potential 0: every draw finds row 0
        if name in ("n63_all", "n65_all"):
            assert np.unique(idx).size == N
        if name == "n4097_t16":
            d = ((X.astype(np.float64) - X.astype(np.float64)[first]) ** 2).sum(1)     # a candidate in the ragged block
            assert np.searchsorted(np.cumsum(d), (1.0 - 2.0 ** -53) * d.sum()) == N - 1


def test_label_makers():
    for K, n in [(2, 1), (8, 2), (8, 7), (16, 7), (1025, 7), (1025, 1024), (16384, 2), (4096, 7), (5, 0)]:
        e = R.empty_clusters(K, n)
        assert e.size == n and np.unique(e).size == n and (n == 0 or (e[0] == 0 and e.min() >= 0 and e.max() < K))
        if n >= 2:
            assert e[-1] == K - 1
        if 3 <= n < K - 1:
            assert ((e > 0) & (e < K - 1) & (np.abs(e - K // 2) <= n)).any()
        for N in (K - n, K + 3, 3 * K + 1):
            lab = R.labels_with_empty(K + N, N, K, e)
            assert np.array_equal(np.flatnonzero(np.bincount(lab, minlength=K) == 0), e)
    lab = R.labels_sorted(3, 5000, 7)
    assert (np.diff(lab) >= 0).all() and np.array_equal(np.sort(R.labels_uniform(3, 5000, 7)), lab)
    lab = R.labels_blocks(5000, 3)
    assert all(np.unique(lab[i:i + 1024]).size == 1 for i in range(0, 5000, 1024)) and list(lab[::1024]) == [0, 1, 2, 0, 1]
    assert (R.labels_one(9, 4) == 4).all()


def test_relocate_pairs_order_and_count():
    X = np.array([[0.0], [5.0], [5.0], [1.0], [-5.0]])
    C = np.zeros((5, 1))
    lab = np.zeros(5, np.int64)
    c, shift, moved, cnt, ne, pairs = R.update(X, lab, C, 5, full=True)
    assert ne == 4 and moved == 4 and pairs == [(1, 1), (2, 2), (4, 3), (3, 4)]       # ties to the lower row
    assert list(cnt) == [1, 1, 1, 1, 1] and list(c[:, 0]) == [0.0, 5.0, 5.0, -5.0, 1.0]
    # fewer rows than empty clusters: the pairing stops when the rows run out
    c, shift, moved, cnt, ne, pairs = R.update(X[:3], lab[:3], np.zeros((7, 1)), 7, full=True)
    assert ne == 6 and moved == 3 and [p[1] for p in pairs] == [1, 2, 3] and [p[0] for p in pairs] == [1, 2, 0]
    assert list(cnt) == [0, 1, 1, 1, 0, 0, 0] and not c[0].any()
    assert R.update(X, lab, C, 5)[2] == 4                       # the three-value form the other tests use
    # shift of the fp32-rounded centres: about 1e-7 from the unrounded one, not equal
    Xg, Cg = R.planted(5, 300, 7, 3)
    labg = R.labels_uniform(5, 300, 3)
    cg, sh, _ = R.update(Xg.astype(np.float64), labg, Cg.astype(np.float64), 3)
    sr = R.shift_of_rounded(cg, Cg)
    assert sr != sh and abs(sr - sh) <= 1e-6 * sh


def test_top_gaps_and_the_gaussian_relocation_cases():
    g = R.top_gaps(np.array([1.0, 4.0, 4.0, 2.0, 0.5]), 3)
    assert np.array_equal(g, [0.0, 0.5, 0.5])
    assert R.top_gaps(np.array([3.0]), 2).size == 0
    relocating = 0
    for case in E.UPDATE_GAUSS:
        X, C, labels, n_empty = E.update_case(case, gauss=True)
        assert int((np.bincount(labels, minlength=case[3]) == 0).sum()) == n_empty
        if n_empty:
            relocating += 1
            assert R.relocation_order_is_decided(X, labels, C, n_empty), case[0]
        if case[4] == "dup":
            a, b = case[1] // 3, case[1] - 2
            pairs = R.update(X.astype(np.float64), labels, C.astype(np.float64), case[3], full=True)[5]
            assert [p[0] for p in pairs] == [a, b]
    assert relocating >= 3
    # a near tie between different rows is refused
    X = np.array([[1.0], [1.0 + 1e-12], [0.0]])
    assert not R.relocation_order_is_decided(X, np.zeros(3, np.int64), np.zeros((1, 1)), 1)
    assert R.relocation_order_is_decided(X[[0, 0, 2]], np.zeros(3, np.int64), np.zeros((1, 1)), 1)


def test_add_rows_both_against_exact_rationals():
    from fractions import Fraction
    rs = np.random.RandomState(0)
    x = rs.randn(6, 5).astype(np.float32)
    v = rs.randn(5).astype(np.float32)
    alpha = np.float32(-0.7)
    # fl64(x + alpha v) on an fp32 midpoint with the true sum below it: the fused result must round down, not to even
    x[0, 0] = np.float32(1.0 + 2.0 ** -23)
    v[0] = np.float32(2.0 ** -12 * (1.0 - 2.0 ** -23))
    plain, fused = R.add_rows_both(x, v, np.float32(2.0 ** -12 * (1.0 + 2.0 ** -23)))
    assert fused[0, 0] == np.float32(1.0 + 2.0 ** -23) and plain[0, 0] == np.float32(1.0 + 2.0 ** -22)
    plain, fused = R.add_rows_both(x, v, alpha)

    def fl32(q):                                            # nearest fp32 of a rational (ties to even)
        f = np.float32(float(q))                            # double rounding is checked away below
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        best = min(cands, key=lambda c: (abs(Fraction(float(c)) - q), int(np.float32(c).view(np.int32)) & 1))
        return np.float32(best)

    for i in range(6):
        for j in range(5):
            p = Fraction(float(alpha)) * Fraction(float(v[j]))
            assert fused[i, j] == fl32(Fraction(float(x[i, j])) + p)
            assert plain[i, j] == fl32(Fraction(float(x[i, j])) + Fraction(float(fl32(p))))
    assert R.ulp_distance(np.float32([1.0, -0.0, -1.0]), np.float32([1.0 + 2.0 ** -23, 0.0, -1.0 - 2.0 ** -22])).tolist() == [1, 0, 2]


def test_vq_ema_update_rounded_is_the_float64_update_rounded():
    import vq_ema_ref as V
    rs = np.random.RandomState(1)
    K, D = 37, 5
    cs, W = rs.rand(K).astype(np.float32) + 0.5, rs.randn(K, D).astype(np.float32)
    c, s = rs.randint(0, 4, K).astype(np.float32), rs.randn(K, D).astype(np.float32)
    a, b, e = V.update_rounded(cs, W, c, s, 0.99, 1e-5)
    a64, b64, e64 = V.update(cs, W, c, s, 0.99, 1e-5)
    assert a.dtype == b.dtype == e.dtype == np.float32
    assert np.array_equal(a, a64.astype(np.float32)) and np.array_equal(b, b64.astype(np.float32))
    assert R.ulp_distance(e, e64.astype(np.float32)).max() <= 2
