"""k-means on the device (csrc/kmeans.hip, acoustic_locating_vq_vae.kmeans) against scikit-learn's recorded outputs
(tests/golden/g9_kmeans.npz; sklearn itself is not needed here): Lloyd from a given init (labels identical, centres and
inertia to 1e-5, n_iter_ equal), the case with an empty cluster, the k-means++ replay with sklearn's draws, bitwise
repeatability, n_init, and the codebook-init shape N = 256 000, D = 128, K = 1024."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import kmeans_ref as R  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import kmeans as KM  # noqa: E402

DEV = "cuda"
GOLD = os.path.join(ROOT, "tests", "golden", "g9_kmeans.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def lloyd_case(g, name):
    N_, D, K, far = (int(v) for v in g[name + "_shape"])
    X, init = R.planted(int(g[name + "_seed"]), N_, D, K, far=None if far < 0 else far)
    assert R.checksum(X) == str(g[name + "_sha"])
    return X, init


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("name", ["l64k16", "l128k16", "l64k256", "l128k256", "empty"])
def test_lloyd_matches_sklearn(g, name):
    X, init = lloyd_case(g, name)
    km = KM.KMeans(n_clusters=init.shape[0], init=init).fit(torch.from_numpy(X).to(DEV))
    assert np.array_equal(km.labels_.cpu().numpy(), g[name + "_labels"])
    assert km.n_iter_ == int(g[name + "_n_iter"])
    assert rel_l2(km.cluster_centers_.cpu().numpy(), g[name + "_centers"]) <= 1e-5
    assert abs(km.inertia_ - float(g[name + "_inertia"])) <= 1e-5 * float(g[name + "_inertia"])
    assert km.cluster_centers_.dtype == torch.float32 and km.labels_.dtype == torch.int64
    assert np.array_equal(km.predict(torch.from_numpy(X).to(DEV)).cpu().numpy(), g[name + "_labels"])


def test_update_relocates_the_empty_cluster(g):
    """One update on the empty case's first labels: the far centre gets no row, the farthest row moves to it."""
    X, init = lloyd_case(g, "empty")
    Xc = X.astype(np.float64) - X.astype(np.float64).mean(0)
    x = torch.from_numpy(Xc.astype(np.float32)).to(DEV)
    c = torch.from_numpy((init.astype(np.float64) - X.astype(np.float64).mean(0)).astype(np.float32)).to(DEV)
    labels = N.vq_argmin(x, c)
    K = c.shape[0]
    new = torch.empty_like(c)
    counts = torch.empty(K, device=DEV, dtype=torch.int32)
    stats = torch.empty(1, device=DEV, dtype=torch.float64)
    flags = torch.empty(4, device=DEV, dtype=torch.int32)
    N.kmeans_update(x, labels, None, c, new, counts, stats, flags, 0.0)
    f = flags.cpu().numpy()
    assert f[1] == 1 and f[2] == 1 and f[3] == 1 and f[0] == 0
    want, shift_tot, moved = R.update(x.cpu().numpy().astype(np.float64), labels.cpu().numpy(), c.cpu().numpy().astype(np.float64), K)
    assert moved == 1
    assert rel_l2(new.cpu().numpy(), want) <= 1e-6
    assert counts.cpu().numpy().min() >= 1 and counts.cpu().numpy().sum() == X.shape[0]
    assert abs(float(stats[0]) - shift_tot) <= 1e-6 * shift_tot


@pytest.mark.parametrize("name", ["pp32k64", "pp128k256"])
def test_kmeans_plusplus_replays_sklearn(g, name):
    N_, D, K = (int(v) for v in g[name + "_shape"])
    X, _ = R.planted(int(g[name + "_seed"]), N_, D, 3 * K, spread=2.0)
    x = torch.from_numpy(X).to(DEV)
    centers, idx = KM._kmeans_plusplus(x, K, int(g[name + "_first"]), g[name + "_uniforms"])
    assert np.array_equal(idx.cpu().numpy(), g[name + "_indices"])
    assert torch.equal(centers, x[idx])


def test_two_fits_are_bitwise_identical():
    X, _ = R.planted(31, 20000, 64, 64)
    x = torch.from_numpy(X).to(DEV)
    a = KM.KMeans(n_clusters=64, random_state=5).fit(x)
    b = KM.KMeans(n_clusters=64, random_state=5).fit(x)
    assert torch.equal(a.cluster_centers_, b.cluster_centers_) and torch.equal(a.labels_, b.labels_)
    assert a.inertia_ == b.inertia_ and a.n_iter_ == b.n_iter_


def test_n_init_keeps_the_least_inertia():
    X, _ = R.planted(32, 6000, 16, 40, spread=1.0)
    x = torch.from_numpy(X).to(DEV)
    best = KM.KMeans(n_clusters=40, n_init=3, random_state=9).fit(x)
    # the same three runs one by one: the generator's stream continues from run to run
    g = torch.Generator().manual_seed(9)
    single = KM.KMeans(n_clusters=40, random_state=9)
    mean, var_mean = N.kmeans_col_stats(x)
    xc = N.kmeans_add_rows(x, mean, -1.0)
    inertias = []
    for _ in range(3):
        first = int(torch.randint(x.shape[0], (1,), generator=g))
        u = torch.rand((39, 2 + int(np.log(40))), generator=g, dtype=torch.float64)
        init, _ = KM._kmeans_plusplus(xc, 40, first, u)
        inertias.append(float(single._lloyd(xc, init, float(var_mean.item()) * 1e-4)[1].item()))
    assert best.inertia_ == min(inertias)
    assert len(set(inertias)) > 1 or best.inertia_ == inertias[0]


def test_codebook_init_shape_every_cluster_nonempty():
    torch.manual_seed(0)
    x = torch.randn(256000, 128, device=DEV) * torch.linspace(0.5, 2.0, 128, device=DEV)
    km = KM.KMeans(n_clusters=1024, random_state=0, max_iter=20).fit(x)
    counts = torch.bincount(km.labels_, minlength=1024)
    assert int(counts.min()) > 0 and int(counts.sum()) == 256000
    assert 1 <= km.n_iter_ <= 20 and np.isfinite(km.inertia_)


def test_refusals_on_the_device():
    x = torch.randn(5, 4, device=DEV)
    with pytest.raises(ValueError, match="n_samples=5"):
        KM.KMeans(n_clusters=6).fit(x)
    with pytest.raises(ValueError, match="init should be of shape"):
        KM.KMeans(n_clusters=2, init=np.zeros((3, 4), np.float32)).fit(x)
    with pytest.warns(RuntimeWarning, match="Explicit initial center"):
        KM.KMeans(n_clusters=2, init=x[:2].cpu().numpy(), n_init=3).fit(x)
