"""Regenerate tests/golden/g9_kmeans.npz with scikit-learn (1.7.2 at the time of writing):

    python tests/golden/make_kmeans_goldens.py

The data are not stored: each case keeps its seed and shape, X is regenerated from the frozen legacy np.random.RandomState
stream (tests/helpers/kmeans_ref.py: planted) and checked against the stored sha256.  Stored per case: sklearn's labels_,
cluster_centers_, inertia_ and n_iter_ for KMeans(init=<array>, n_init=1, algorithm="lloyd").  A Lloyd case is accepted only
when sklearn's float32 and float64 runs give the same labels and n_iter_ (no near-ties) and the float64 restatement agrees.
The k-means++ replay stores the first index and the uniforms drawn from RandomState(seed) exactly as _kmeans_plusplus draws
them, and sklearn's chosen indices."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import kmeans_ref as R  # noqa: E402

# (name, seed, N, D, K, far): far = index of an init centre placed away from all rows (an empty cluster in iteration 1)
LLOYD = [("l64k16", 11, 3000, 64, 16, None), ("l128k16", 12, 4000, 128, 16, None),
         ("l64k256", 13, 4000, 64, 256, None), ("l128k256", 14, 5000, 128, 256, None), ("empty", 15, 2000, 32, 12, 5)]
PLUSPLUS = [("pp32k64", 21, 2000, 32, 64), ("pp128k256", 22, 4000, 128, 256)]


def main():
    import sklearn
    from sklearn.cluster import KMeans, kmeans_plusplus
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, seed, N, D, K, far in LLOYD:
        X, init = R.planted(seed, N, D, K, far=far)
        runs = {}
        for dt in (np.float32, np.float64):
            km = KMeans(n_clusters=K, init=init.astype(dt), n_init=1, max_iter=300, tol=1e-4, algorithm="lloyd").fit(X.astype(dt))
            runs[dt] = km
        a, b = runs[np.float32], runs[np.float64]
        trace = []
        lab, inertia, C, n_iter = R.fit(X, init, trace=trace)
        ok = np.array_equal(a.labels_, b.labels_) and a.n_iter_ == b.n_iter_ and np.array_equal(lab, b.labels_) and n_iter == b.n_iter_
        if far is not None:
            ok = ok and max(trace) == 1
        assert ok, (name, a.n_iter_, b.n_iter_, n_iter, trace)
        print(name, "n_iter", b.n_iter_, "inertia", b.inertia_, "relocated per iteration", trace)
        for k, v in (("seed", seed), ("shape", (N, D, K, -1 if far is None else far)), ("sha", R.checksum(X)),
                     ("labels", b.labels_.astype(np.int16)), ("centers", b.cluster_centers_.astype(np.float32)),
                     ("inertia", b.inertia_), ("n_iter", b.n_iter_)):
            out["%s_%s" % (name, k)] = np.array(v)
    for name, seed, N, D, K in PLUSPLUS:
        X, _ = R.planted(seed, N, D, 3 * K, spread=2.0)
        T = 2 + int(np.log(K))
        rs = np.random.RandomState(seed)
        first = rs.choice(N, p=np.ones(N) / N)
        uniforms = np.stack([rs.uniform(size=T) for _ in range(K - 1)])
        idx32 = kmeans_plusplus(X, K, random_state=seed)[1]
        idx64 = kmeans_plusplus(X.astype(np.float64), K, random_state=seed)[1]
        mine = R.kmeans_plusplus(X, K, first, uniforms)
        assert idx32[0] == first and np.array_equal(idx32, idx64) and np.array_equal(mine, idx64), name
        print(name, "T", T, "first", first)
        for k, v in (("seed", seed), ("shape", (N, D, K)), ("sha", R.checksum(X)), ("first", first),
                     ("uniforms", uniforms), ("indices", idx64.astype(np.int32))):
            out["%s_%s" % (name, k)] = np.array(v)
    path = os.path.join(HERE, "g9_kmeans.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
