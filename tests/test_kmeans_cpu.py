"""k-means without a GPU: the float64 restatement (tests/helpers/kmeans_ref.py) pinned against scikit-learn itself on the
golden cases and on random ones, the golden data's checksums, the KMeans constructor's and input refusals, and the argument
errors of every alvq_kmeans_* entry point, which must fail before anything is launched."""
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
