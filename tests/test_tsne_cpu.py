"""Exact t-SNE without a GPU: the float64 restatement (tests/helpers/tsne_ref.py) against finite differences, the perplexity
target and the one-hot definition of the code distance; the package's check-by-check schedule (tsne._schedule) against the
restatement's per-iteration loop on hand-built KL and gradient-norm sequences; the argument errors of every alvq_tsne_* entry
point, which must fail before anything is launched; and the TSNE constructor's refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import tsne_ref as R  # noqa: E402
from acoustic_locating_vq_vae import tsne as T  # noqa: E402


@pytest.fixture(scope="module")
def native():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native
    return _native


def random_p(n, seed):
    rng = np.random.default_rng(seed)
    d2 = rng.uniform(0.5, 6.0, (n, n)).astype(np.float32)
    d2 = ((d2 + d2.T) / 2).astype(np.float32)
    np.fill_diagonal(d2, 0.0)
    P, *_ = R.affinities(d2, 3.0)
    return P


def test_gradient_matches_finite_differences_of_kl():
    # with e = 1 the t-SNE gradient is the exact gradient of KL(P || Q); an exaggerated one is not (t-SNE's convention)
    exaggeration = 1.0
    n = 9
    P = random_p(n, 1)
    Y = np.random.default_rng(2).standard_normal((n, 2))
    _, g = R.kl_grad(P, Y, exaggeration)
    h = 1e-6
    fd = np.zeros_like(Y)
    for i in range(n):
        for c in range(2):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[i, c] += h
            Ym[i, c] -= h
            fd[i, c] = (R.kl_grad(P, Yp, exaggeration)[0] - R.kl_grad(P, Ym, exaggeration)[0]) / (2 * h)
    assert np.abs(fd - g).max() <= 1e-6 * np.abs(g).max()


def test_row_subset_gradient_matches_full():
    n = 40
    P = random_p(n, 3)
    Y = np.random.default_rng(4).standard_normal((n, 2))
    _, g = R.kl_grad(P, Y, 12.0)
    rows = np.array([0, 7, 39])
    assert np.abs(R.grad_rows(P[rows], Y, rows, 12.0) - g[rows]).max() <= 1e-12 * np.abs(g).max()


@pytest.mark.parametrize("perplexity", [5.0, 30.0])
def test_converged_rows_hit_the_entropy_target(perplexity):
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 16, (120, 11))
    d2 = R.code_sqdist(codes)
    Pc, beta, S, H, flagged = R.conditional_p(d2, perplexity)
    ok = np.abs(H - np.log(perplexity)) <= 1e-5
    # a row whose k nearest are tied has entropy > log k at any beta: the target is out of reach when k > perplexity, and
    # only such rows (k >= perplexity: at k == perplexity it is reached only in the limit) end unconverged, as in sklearn
    off = d2 + np.where(np.eye(120, dtype=bool), np.inf, 0)
    ties = (off == off.min(1, keepdims=True)).sum(1)
    assert np.all(ties[~ok] >= perplexity) and np.all(ok[ties < perplexity])
    assert ok.mean() > 0.5
    # the entropy of the stored conditional distribution of a converged row is the target too
    p = Pc[ok].astype(np.float64) / Pc[ok].astype(np.float64).sum(1, keepdims=True)
    ent = -(p * np.log(np.where(p > 0, p, 1.0))).sum(1)
    assert np.abs(ent - np.log(perplexity)).max() <= 1e-4


def test_underflowing_row_takes_the_1e_minus_8_path():
    n = 8
    i = np.arange(n)
    d2 = (800.0 + 6.0 * np.abs(i[:, None] - i[None, :]) + 1.3 * i[None, :]).astype(np.float32)   # exp(-d) == 0 at beta = 1
    np.fill_diagonal(d2, 0.0)
    Pc, beta, S, H, _ = R.conditional_p(d2, 2.0)
    assert np.all(np.exp(-d2[~np.eye(n, dtype=bool)].astype(np.float64)) == 0.0)            # S = 0 at the first step
    assert np.all(beta < 1.0) and np.all(np.isfinite(Pc))
    assert np.abs(H - np.log(2.0)).max() <= 1e-5
    assert np.allclose(Pc.sum(1), 1.0, atol=1e-6)


def test_code_distances_equal_onehot_squared_distances():
    rng = np.random.default_rng(6)
    codes = rng.integers(0, 12, (30, 7))
    codes[3] = codes[4]                                                   # a duplicate row: distance 0
    d2 = R.code_sqdist(codes)
    assert d2.dtype == np.float32
    np.testing.assert_array_equal(d2, R.onehot_sqdist(codes, 12).astype(np.float32))
    assert d2[3, 4] == 0 and np.all(np.diag(d2) == 0)
    np.testing.assert_array_equal(R.code_sqdist(codes, rows=[5, 29]), d2[[5, 29]])


def test_joint_p_is_symmetric_normalised_and_clamped():
    P = random_p(25, 7)
    assert np.array_equal(P, P.T)
    assert abs(P.astype(np.float64).sum() - 1.0) < 1e-6
    off = ~np.eye(25, dtype=bool)
    assert P[off].min() >= np.float32(R.EPS) and np.all(np.diag(P) == 0)


# ------------------------------------------------------------------------------------------------------------------ schedule
def run_both(kl_of, gn_of, max_iter, niwp=300, mgn=1e-7, ee=12.0):
    """The package's schedule with a fake device (step(n) advances n iterations) against the restatement's loop."""
    calls, pos = [], {"i": -1}

    def run_phase(e, m):
        calls.append(("phase", e, m, pos["i"] + 1))

        def step(n):
            pos["i"] += n
            calls.append(("step", n))
            return kl_of(pos["i"]), gn_of(pos["i"])
        return step

    kl, it, trace = T._schedule(run_phase, max_iter, ee, niwp, mgn)
    want = R.schedule(lambda ph, i, c: (kl_of(i) if c else None, gn_of(i)), max_iter, niwp, mgn)
    return (kl, it), want, calls, trace


def test_schedule_runs_both_phases_with_resets():
    (kl, it), want, calls, trace = run_both(lambda i: 10.0 - 1e-3 * i, lambda i: 1.0, 1000)
    assert (kl, it) == want == (10.0 - 1e-3 * 999, 999)
    phases = [c for c in calls if c[0] == "phase"]
    assert phases == [("phase", 12.0, 0.5, 0), ("phase", 1.0, 0.8, 250)]
    # the host reads once per check (49, 99, ..., 249, 299, ..., 999): 5 + 15 reads, one per 50-iteration chunk
    assert [t[0] for t in trace] == list(range(49, 1000, 50))
    assert all(c[1] == 50 for c in calls if c[0] == "step")


def test_schedule_last_chunk_ends_at_max_iter():
    (kl, it), want, calls, trace = run_both(lambda i: 5.0 - 1e-3 * i, lambda i: 1.0, 321)
    assert (kl, it) == want == (5.0 - 1e-3 * 320, 320)
    assert trace[-1][0] == 320 and [c[1] for c in calls if c[0] == "step"][-1] == 21


def test_min_grad_norm_stops_each_phase_at_its_first_check():
    (kl, it), want, calls, _ = run_both(lambda i: 1.0, lambda i: 0.5, 1000, mgn=1e3)
    assert (kl, it) == want and it == 99
    assert [c for c in calls if c[0] == "phase"][1][3] == 50                # phase 2 starts right after i = 49


@pytest.mark.parametrize("niwp", [49, 50, 120, 300])
def test_no_progress_stops_where_the_restatement_does(niwp):
    def kl_of(i):  # improves until 399, then flat
        return 3.0 - 1e-3 * min(i, 399)
    (kl, it), want, _, _ = run_both(kl_of, lambda i: 1.0, 1000, niwp=niwp)
    assert (kl, it) == want
    assert it < 999


def test_no_progress_in_the_exploration_phase_uses_250():
    def kl_of(i):  # flat from the start: the exploration phase never stops on progress (250 > its length)
        return 2.0
    (kl, it), want, _, _ = run_both(kl_of, lambda i: 1.0, 1000, niwp=100)
    assert (kl, it) == want == (2.0, 449)            # phase 2: best at 299; 399 - 299 = 100 is not > 100, 449 - 299 is


def test_max_iter_250_leaves_phase_one_values():
    (kl, it), want, calls, _ = run_both(lambda i: 1.0 / (i + 1), lambda i: 1.0, 250)
    assert (kl, it) == want == (1.0 / 250, 249)
    assert sum(c[1] for c in calls if c[0] == "step") == 250


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_tsne_abi_argument_errors_do_not_launch(native):
    lib = native.lib()
    p = 16  # any non-null value: no launch may happen before the checks fail
    assert lib.alvq_tsne_code_sqdist_f32(None, p, 10, 3, None) == -1 and b"null" in lib.alvq_last_error()
    assert lib.alvq_tsne_code_sqdist_f32(p, None, 10, 3, None) == -1
    for n, l in ((1, 3), (65537, 3), (10, 0), (10, 4097), (0, 1), (-5, 2)):
        assert lib.alvq_tsne_code_sqdist_f32(p, p, n, l, None) == -1, (n, l)
    assert b"alvq_tsne_code_sqdist_f32" in lib.alvq_last_error()

    assert lib.alvq_tsne_affinities_workspace_bytes(10) == 11 * 8
    assert lib.alvq_tsne_affinities_workspace_bytes(65536) == 65537 * 8
    for n in (1, 0, 65537):
        assert lib.alvq_tsne_affinities_workspace_bytes(n) == -1
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.alvq_tsne_affinities_f32(*args, 10, 3.0, None) == -1
    for n, perp in ((1, 0.5), (65537, 30.0), (10, 0.0), (10, -1.0), (10, 10.0), (10, 12.0), (10, float("nan"))):
        assert lib.alvq_tsne_affinities_f32(p, p, p, p, n, perp, None) == -1, (n, perp)
    assert b"perplexity" in lib.alvq_last_error()

    assert lib.alvq_tsne_descend_workspace_bytes(10) == 51 * 8
    for n in (1, 65537):
        assert lib.alvq_tsne_descend_workspace_bytes(n) == -1
    ok = [p] * 7
    for k in range(7):
        args = list(ok)
        args[k] = None
        assert lib.alvq_tsne_descend_f64(*args, 10, 1, 12.0, 0.5, 200.0, None) == -1, k
    for n, it, e, m, lr in ((1, 1, 12.0, 0.5, 200.0), (65537, 1, 1.0, 0.5, 1.0), (10, 0, 12.0, 0.5, 200.0),
                            (10, 1, 0.0, 0.5, 200.0), (10, 1, 1.0, 1.0, 200.0), (10, 1, 1.0, -0.1, 200.0),
                            (10, 1, 1.0, 0.8, 0.0)):
        assert lib.alvq_tsne_descend_f64(*ok, n, it, e, m, lr, None) == -1, (n, it, e, m, lr)


# ----------------------------------------------------------------------------------------------------------- constructor
@pytest.mark.parametrize("kwargs, exc", [
    ({"n_components": 3}, NotImplementedError),
    ({"method": "barnes_hut"}, NotImplementedError),
    ({"method": "fast"}, ValueError),
    ({"max_iter": 100}, ValueError),
    ({"n_iter": 249}, ValueError),
    ({"init": "pca"}, NotImplementedError),
    ({"init": "spectral"}, ValueError),
    ({"metric": "cosine"}, ValueError),
    ({"perplexity": 0.0}, ValueError),
    ({"learning_rate": -1.0}, ValueError),
])
def test_constructor_refusals(kwargs, exc):
    with pytest.raises(exc):
        T.TSNE(**kwargs)


def test_constructor_defaults():
    t = T.TSNE()
    assert (t.perplexity, t.early_exaggeration, t.learning_rate, t.max_iter) == (30.0, 12.0, "auto", 1000)
    assert (t.n_iter_without_progress, t.min_grad_norm, t.metric, t.init) == (300, 1e-7, "euclidean", "random")
    assert T.TSNE(n_iter=400).max_iter == 400


def test_cpu_input_is_refused():
    import torch
    with pytest.raises(RuntimeError, match="GPU"):
        T.TSNE(perplexity=2.0).fit_transform(torch.zeros((5, 3), dtype=torch.int64))
