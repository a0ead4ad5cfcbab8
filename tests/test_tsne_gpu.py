"""Exact t-SNE on the device (csrc/tsne.hip, acoustic_locating_vq_vae.tsne) against the float64 restatement of
tests/helpers/tsne_ref.py, element by element: code distances exactly, the perplexity search's beta bitwise, the joint P to
4 fp32 ulps, the descent to 1e-9 of max|Y|; the schedule and stop rules through the public TSNE; full runs on planted clusters;
a matrix with more than 2^31 elements; and the error paths.  Parity with sklearn itself is unpinned (it is absent)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import tsne_ref as R  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import tsne as T  # noqa: E402

DEV = "cuda"


def planted(n_per, L, K, noise, seed, n_clusters=3):
    """n_clusters centres of L random codes; each point copies its centre and re-draws a `noise` share of its codes."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, K, (n_clusters, L))
    codes, labels = [], []
    for c in range(n_clusters):
        x = np.repeat(centres[c][None], n_per, 0)
        flip = rng.random(x.shape) < noise
        x[flip] = rng.integers(0, K, int(flip.sum()))
        codes.append(x)
        labels += [c] * n_per
    return np.concatenate(codes).astype(np.int64), np.array(labels)


def sqdist_nan_filled(codes32):
    n, L = codes32.shape
    d2 = torch.full((n, n), float("nan"), device=DEV)
    N._check(N.lib().alvq_tsne_code_sqdist_f32(codes32.data_ptr(), d2.data_ptr(), n, L, N._stream()), "sqdist")
    return d2


def affinities_nan_filled(d2):
    """Device affinities with beta / S / workspace pre-filled with NaN: an unwritten element fails."""
    P = d2.clone()
    n = P.shape[0]
    beta = torch.full((n,), float("nan"), device=DEV, dtype=torch.float64)
    S = torch.full((n,), float("nan"), device=DEV, dtype=torch.float64)
    ws = torch.full((N.lib().alvq_tsne_affinities_workspace_bytes(n) // 8,), float("nan"), device=DEV, dtype=torch.float64)
    N._check(N.lib().alvq_tsne_affinities_f32(P.data_ptr(), beta.data_ptr(), S.data_ptr(), ws.data_ptr(), n, float(PERP[0]),
                                              N._stream()), "affinities")
    return P, beta, S


PERP = [30.0]


def ulp_close(a, b, ulps=4, floor=1e-12):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulps * sp) | (np.abs(a - b) <= floor)


def check_affinities(d2_np, perplexity):
    PERP[0] = perplexity
    P, beta, S = affinities_nan_filled(torch.from_numpy(d2_np).to(DEV))
    P_np, beta_np, S_np = P.cpu().numpy(), beta.cpu().numpy(), S.cpu().numpy()
    Pw, bw, Sw, Hw, flagged = R.affinities(d2_np, perplexity)
    n = d2_np.shape[0]
    assert np.isfinite(P_np).all() and np.isfinite(beta_np).all() and np.isfinite(S_np).all()
    ok = ~flagged
    assert np.array_equal(beta_np[ok], bw[ok]), np.nonzero(beta_np[ok] != bw[ok])
    assert np.all(np.abs(S_np[ok] - Sw[ok]) <= 1e-12 * np.abs(Sw[ok]))
    for i in np.nonzero(flagged)[0]:                  # a decision within 1e-12 of its threshold: the entropy target only
        d = d2_np[i].astype(np.float64)
        m = np.arange(n) != i
        p = np.exp(-d[m] * beta_np[i])
        assert abs(np.log(p.sum()) + beta_np[i] * (d[m] * p).sum() / p.sum() - np.log(perplexity)) <= 1e-5
    keep = np.ix_(ok, ok)
    close = ulp_close(P_np[keep], Pw[keep])
    assert close.all(), (np.argwhere(~close)[:5], P_np[keep][~close][:5], Pw[keep][~close][:5])
    assert torch.equal(P, P.T)                                                         # exactly symmetric
    assert np.all(np.diag(P_np) == 0)
    assert abs(P_np.astype(np.float64).sum() - 1.0) <= 1e-6
    return P, flagged


# ------------------------------------------------------------------------------------------------------------- distances
@pytest.mark.parametrize("n", [2, 63, 64, 65, 1000])
@pytest.mark.parametrize("L", [1, 7, 201])
def test_code_distances_exact(n, L):
    rng = np.random.default_rng(n * 1000 + L)
    codes = rng.integers(0, 3 if L < 10 else 8, (n, L))
    got = sqdist_nan_filled(torch.from_numpy(codes.astype(np.int32)).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(got, R.code_sqdist(codes))


def test_code_distances_from_int64_and_onehot():
    codes, _ = planted(40, 201, 1024, 0.1, 1)
    want = R.code_sqdist(codes)
    c = torch.from_numpy(codes).to(DEV)
    np.testing.assert_array_equal(T.code_sq_distances(c).cpu().numpy(), want)                      # int64
    np.testing.assert_array_equal(T.code_sq_distances(c.int()).cpu().numpy(), want)                # int32
    oh = torch.nn.functional.one_hot(c, 1024).float()
    np.testing.assert_array_equal(T.code_sq_distances(oh).cpu().numpy(), want)                     # (N, L, K)
    np.testing.assert_array_equal(T.code_sq_distances(oh.view(120, -1), n_codes=1024).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------------ affinities
@pytest.mark.parametrize("perplexity", [5.0, 30.0, 100.0])
def test_affinities_match_restatement(perplexity):
    codes, _ = planted(100, 201, 1024, 0.3, 2)
    d2 = R.code_sqdist(codes)
    check_affinities(d2, perplexity)


def test_affinities_duplicate_rows():
    codes, _ = planted(50, 30, 16, 0.4, 3)
    codes[7] = codes[8]
    codes[60] = codes[61] = codes[62]
    d2 = R.code_sqdist(codes)
    assert d2[7, 8] == 0 and d2[60, 62] == 0
    check_affinities(d2, 10.0)


def test_affinities_underflowing_rows():
    n = 8
    i = np.arange(n)
    d2 = (800.0 + 6.0 * np.abs(i[:, None] - i[None, :]) + 1.3 * i[None, :]).astype(np.float32)    # exp(-d) == 0 at beta = 1
    np.fill_diagonal(d2, 0.0)
    check_affinities(d2, 2.0)


def test_affinities_repeatable():
    codes, _ = planted(70, 50, 32, 0.3, 4)
    d2 = torch.from_numpy(R.code_sqdist(codes)).to(DEV)
    PERP[0] = 20.0
    a, b = affinities_nan_filled(d2)[0], affinities_nan_filled(d2)[0]
    assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------------- descent
@pytest.fixture(scope="module")
def small_p():
    codes, labels = planted(40, 201, 1024, 0.2, 5)
    d2 = torch.from_numpy(R.code_sqdist(codes)).to(DEV)
    P = d2.clone()
    N.tsne_affinities(P, 15.0)
    Y0 = np.random.default_rng(6).standard_normal((120, 2)) * 1e-2
    return P, P.cpu().numpy(), Y0


def run_device(P, Y0, n, e, m, lr, update=None, gains=None):
    Y = torch.from_numpy(np.array(Y0)).to(DEV)
    u = torch.zeros_like(Y) if update is None else torch.from_numpy(np.array(update)).to(DEV)
    g = torch.ones_like(Y) if gains is None else torch.from_numpy(np.array(gains)).to(DEV)
    grad = torch.full_like(Y, float("nan"))
    stats = torch.full((2,), float("nan"), device=DEV, dtype=torch.float64)
    N.tsne_descend(P, Y, u, g, grad, stats, n, e, m, lr)
    return Y.cpu().numpy(), u.cpu().numpy(), g.cpu().numpy(), grad.cpu().numpy(), stats.cpu().numpy()


def test_first_gradient_matches_restatement(small_p):
    P, P_np, Y0 = small_p
    Y, u, g, grad, stats = run_device(P, Y0, 1, 12.0, 0.5, 50.0)
    Yw, uw, gw, gradw, klw, gnw = R.descend(P_np, Y0, 1, 12.0, 0.5, 50.0)
    assert np.abs(grad - gradw).max() <= 1e-9 * np.abs(gradw).max()
    assert np.array_equal(g, gw)
    assert abs(stats[0] - klw) <= 1e-9 * abs(klw) and abs(stats[1] - gnw) <= 1e-9 * gnw
    assert np.abs(Y - Yw).max() <= 1e-9 * np.abs(Yw).max()


# lr 5: at N = 120 the sklearn default (50) makes the exaggerated phase chaotic -- the restatement itself moves by 30 % after
# 49 iterations from a 1e-14 change of its init -- while at 5 that change stays below 2e-12
@pytest.mark.parametrize("n_iter", [49, 50])
def test_fifty_iterations_match_restatement(small_p, n_iter):
    P, P_np, Y0 = small_p
    Y, u, g, grad, stats = run_device(P, Y0, n_iter, 12.0, 0.5, 5.0)
    Yw, uw, gw, gradw, klw, gnw = R.descend(P_np, Y0, n_iter, 12.0, 0.5, 5.0)
    scale = np.abs(Yw).max()
    assert np.abs(Y - Yw).max() <= 1e-9 * scale
    assert np.abs(u - uw).max() <= 1e-9 * scale
    assert np.abs(g - gw).max() <= 1e-9
    assert abs(stats[0] - klw) <= 1e-9 * abs(klw)
    # continuing from the state is the same as one longer call: the phase state lives in the caller's buffers
    Y2, *_ = run_device(P, Y, 10, 1.0, 0.8, 5.0, u, g)
    Yw2, *_ = R.descend(P_np, Yw, 10, 1.0, 0.8, 5.0, uw, gw)
    assert np.abs(Y2 - Yw2).max() <= 1e-9 * np.abs(Yw2).max()


def test_phase_switch_resets_update_and_gains(small_p, monkeypatch):
    """Every device call of a fit is recorded with the state it starts from: phase 1 is iterations 0..249 at e = 12,
    momentum 0.5; phase 2 starts at 250 from update = 0 and gains = 1, at e = 1, momentum 0.8."""
    calls = []
    real = N.tsne_descend

    def spy(P, Y, update, gains, grad, stats, n_iter, e, m, lr, workspace=None):
        calls.append((n_iter, e, m, lr, bool((update == 0).all()), bool((gains == 1).all())))
        return real(P, Y, update, gains, grad, stats, n_iter, e, m, lr, workspace)

    monkeypatch.setattr(T.N_, "tsne_descend", spy)
    t = T.TSNE(perplexity=15.0, max_iter=300, random_state=0, min_grad_norm=0.0)
    t.fit_transform(sqd(small_p))
    first = [k for k, c in enumerate(calls) if c[1] == 1.0][0]
    assert sum(c[0] for c in calls[:first]) == 250 and sum(c[0] for c in calls[first:]) == 50
    assert all(c[1:4] == (12.0, 0.5, 50.0) for c in calls[:first]) and all(c[1:4] == (1.0, 0.8, 50.0) for c in calls[first:])
    assert calls[0][4:] == (True, True) and calls[first][4:] == (True, True)           # reset at each phase's start
    assert calls[1][4:] == (False, False)                                              # and carried within a phase
    assert t.n_iter_ == 299 and [i for i, _, _ in t._trace] == [49, 99, 149, 199, 249, 299]


def sqd(small_p):
    return torch.from_numpy(planted(40, 201, 1024, 0.2, 5)[0]).to(DEV)


def test_min_grad_norm_stops_each_phase_at_its_first_check(small_p):
    t = T.TSNE(perplexity=15.0, min_grad_norm=1e3, random_state=0)
    t.fit_transform(sqd(small_p))
    assert t.n_iter_ == 99
    assert [i for i, _, _ in t._trace] == [49, 99]
    assert np.isfinite(t.kl_divergence_)


@pytest.mark.parametrize("niwp", [50, 100])
def test_no_progress_stops_where_the_restatement_rule_does(small_p, niwp):
    t = T.TSNE(perplexity=15.0, n_iter_without_progress=niwp, max_iter=2000, random_state=1)
    t.fit_transform(sqd(small_p))
    kls = {i: kl for i, kl, _ in t._trace}
    gns = {i: gn for i, _, gn in t._trace}
    want = R.schedule(lambda ph, i, c: (kls[i] if c else None, gns.get(i, 1.0)), 2000, niwp, 1e-7)
    assert (t.kl_divergence_, t.n_iter_) == want


# ------------------------------------------------------------------------------------------------------------- full runs
@pytest.fixture(scope="module")
def clusters():
    codes, labels = planted(100, 201, 1024, 0.1, 7)
    return torch.from_numpy(codes).to(DEV), labels


def test_planted_clusters_separate(clusters):
    codes, labels = clusters
    t = T.TSNE(perplexity=30.0, random_state=0)
    Y = t.fit_transform(codes)
    assert Y.shape == (300, 2) and Y.dtype == torch.float64 and Y.is_cuda
    assert t.learning_rate_ == 50.0
    Yn = Y.cpu().numpy()
    d = ((Yn[:, None] - Yn[None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, 1)[:, :5]
    pure = (labels[nn] == labels[:, None]).all(1)
    assert pure.mean() >= 0.99, pure.mean()
    kl249 = [kl for i, kl, _ in t._trace if i == 249][0]
    assert t.kl_divergence_ < kl249
    Y2 = T.TSNE(perplexity=30.0, random_state=0).fit_transform(codes)
    assert torch.equal(Y, Y2)                                                   # bitwise repeatable


def test_every_input_form_gives_the_same_embedding(clusters):
    codes, _ = clusters
    kw = dict(perplexity=30.0, random_state=3, max_iter=300)
    ref = T.TSNE(**kw).fit_transform(codes)
    oh = torch.nn.functional.one_hot(codes, 1024).float()
    d2 = T.code_sq_distances(codes)
    for X, extra in ((codes.int(), {}), (oh, {}), (oh.view(300, -1), {"n_codes": 1024}), (d2, {"metric": "precomputed"})):
        assert torch.equal(T.TSNE(**kw, **extra).fit_transform(X), ref)
    assert torch.equal(d2, T.code_sq_distances(codes))                         # the precomputed input is left as given


# ----------------------------------------------------------------------------------------------------------------- scale
def z_torch(Y):
    Yt = torch.from_numpy(Y).to(DEV)
    z = torch.zeros((), device=DEV, dtype=torch.float64)
    for a in range(0, Yt.shape[0], 4096):
        d = ((Yt[a:a + 4096, None, :] - Yt[None, :, :]) ** 2).sum(-1)
        num = 1.0 / (1.0 + d)
        idx = torch.arange(a, min(a + 4096, Yt.shape[0]), device=DEV)
        num[idx - a, idx] = 0.0
        z += num.sum()
    return float(z)


def test_past_two_to_the_31_elements():
    n, L, K, perp = 46400, 16, 4, 30.0
    assert n * n > 2 ** 31
    rng = np.random.default_rng(8)
    codes = rng.integers(0, K, (n, L))
    rows = np.array([0, 1, 46281, 46282, 46283, n - 1])          # 46281 straddles element 2^31
    d2 = T.code_sq_distances(torch.from_numpy(codes).to(DEV))
    d2_rows = R.code_sqdist(codes, rows)
    np.testing.assert_array_equal(d2[torch.from_numpy(rows).to(DEV)].cpu().numpy(), d2_rows)
    P = d2
    beta, S = N.tsne_affinities(P, perp)
    b_np, S_np = beta.cpu().numpy(), S.cpu().numpy()
    Pc, bw, Sw, Hw, flagged = R.search_rows(d2_rows, rows, perp)
    ok = ~flagged
    assert np.array_equal(b_np[rows][ok], bw[ok]) and np.all(np.abs(S_np[rows][ok] - Sw[ok]) <= 1e-12 * Sw[ok])
    # P row i = max((Pc_ij + Pc_ji) / total, eps), Pc_ji from the device's beta_j and S_j (checked above on samples)
    P_rows = P[torch.from_numpy(rows).to(DEV)].cpu().numpy()
    for a, i in enumerate(rows):
        if flagged[a]:
            continue
        d = d2_rows[a].astype(np.float64)
        pji = (np.exp(-d * b_np) / S_np).astype(np.float32)
        x = (Pc[a] + pji).astype(np.float64)
        x[i] = 0.0
        total = x.max() / P_rows[a][np.argmax(x)]
        assert abs(total / (2.0 * n) - 1.0) <= 1e-3                              # the conditional rows each sum to 1
        want = np.maximum(x / total, R.EPS)
        want[i] = 0.0
        assert np.all(np.abs(P_rows[a] - want) <= 1e-5 * want + 1e-12), i
    s = sum(float(P[k:k + 2048].sum(dtype=torch.float64)) for k in range(0, n, 2048))
    assert abs(s - 1.0) <= 1e-6
    # three descent iterations, each checked on the sampled rows from the state before it
    Y = torch.from_numpy(np.random.default_rng(9).standard_normal((n, 2)) * 1e-4).to(DEV)
    u, g = torch.zeros_like(Y), torch.ones_like(Y)
    grad, stats = torch.empty_like(Y), torch.empty((2,), device=DEV, dtype=torch.float64)
    for _ in range(3):
        Yp, up, gp = Y.cpu().numpy(), u.cpu().numpy(), g.cpu().numpy()
        N.tsne_descend(P, Y, u, g, grad, stats, 1, 12.0, 0.5, n / 48.0)
        gr = R.grad_rows(P_rows, Yp, rows, 12.0, Z=z_torch(Yp))
        Yw, uw, gw, _ = R.apply_step(Yp[rows], up[rows], gp[rows], gr, 0.5, n / 48.0)
        Yn = Y.cpu().numpy()
        assert np.abs(Yn[rows] - Yw).max() <= 1e-9 * np.abs(Yn).max()
        assert np.array_equal(g.cpu().numpy()[rows], gw)
    assert np.isfinite(stats.cpu().numpy()).all()
    del P, d2


# -------------------------------------------------------------------------------------------------------------- end to end
def test_latent_codes_of_a_vqvae_embed():
    from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE
    torch.manual_seed(0)
    model = ConvolutionalVQVAE(20, 32, 8, 1, 16, 0.25, 1024).cuda().eval()
    B = 24
    x = torch.randn(B, 20, 40, device=DEV)
    with torch.no_grad():
        idx = model.get_latent_indices(x)[3]
    codes = idx.view(B, -1)
    Y = T.TSNE(perplexity=5.0, max_iter=250, random_state=0).fit_transform(codes)
    assert Y.shape == (B, 2) and torch.isfinite(Y).all()


# -------------------------------------------------------------------------------------------------------------- errors
def test_error_paths():
    codes = torch.randint(0, 8, (20, 5), device=DEV)
    with pytest.raises(RuntimeError, match="GPU"):
        T.TSNE(perplexity=5.0).fit_transform(codes.cpu())
    bad = torch.nn.functional.one_hot(codes, 8).float()
    bad[3, 2, 5] = 0.5
    with pytest.raises(ValueError, match="precomputed"):
        T.TSNE(perplexity=5.0).fit_transform(bad)
    with pytest.raises(ValueError, match="perplexity"):
        T.TSNE(perplexity=20.0).fit_transform(codes)
    with pytest.raises(ValueError, match="init"):
        T.TSNE(perplexity=5.0, init=np.zeros((19, 2))).fit_transform(codes)
    d2 = T.code_sq_distances(codes)
    d2[1, 2] = -1.0
    with pytest.raises(ValueError, match="non-negative"):
        T.TSNE(perplexity=5.0, metric="precomputed").fit_transform(d2)
    with pytest.raises(ValueError, match="square"):
        T.TSNE(perplexity=5.0, metric="precomputed").fit_transform(d2[:, :7])
    with pytest.raises(ValueError):
        T.code_sq_distances(torch.full((4, 3), -2, device=DEV, dtype=torch.int64))
