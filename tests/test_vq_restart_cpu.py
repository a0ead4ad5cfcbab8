"""Dead-code restarts of VectorQuantizerEMA without a GPU: the numpy restatement (tests/helpers/vq_restart_ref.py), the planted
collapse on the restatement alone, the keyword contract (errors before the library is touched, nothing new when the feature
is off, private generator, distinct positions) and the C ABI's argument checks."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import vq_ema_ref as E_  # noqa: E402
import vq_restart_ref as R  # noqa: E402
from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE  # noqa: E402
from acoustic_locating_vq_vae.vq_vae.vector_quantizer import VectorQuantizerEMA  # noqa: E402

CFG = (20, 48, 8, 2, 24, 0.25, 64)


def _state(K=12, D=3, seed=0):
    g = np.random.default_rng(seed)
    return g.uniform(2.0, 5.0, size=K), g.normal(size=(K, D)), g.normal(size=(K, D)), g.normal(size=(4, D))


def test_no_dead_code_gives_the_input_back():
    cs, W, E, cand = _state()
    for fn, dt in ((R.restart, np.float64), (R.restart32, np.float32)):
        cs2, W2, E2, n, dead = fn(cs, W, E, cand, 1.0)
        assert (n, dead) == (0, 0)
        assert np.array_equal(cs2, cs.astype(dt)) and np.array_equal(W2, W.astype(dt)) and np.array_equal(E2, E.astype(dt))
        assert cs2.dtype == dt


def test_threshold_zero_is_the_identity():
    cs, W, E, cand = _state()
    cs[3] = 0.0                                           # an unused code: 0 < 0 is false
    cs2, W2, E2, n, dead = R.restart(cs, W, E, cand, 0.0)
    assert (n, dead) == (0, 0) and np.array_equal(cs2, cs) and np.array_equal(W2, W) and np.array_equal(E2, E)


def test_ascending_order_and_the_cap():
    cs, W, E, cand = _state()
    for k in (9, 2, 7, 5, 11, 0):
        cs[k] = 0.25
    cs2, W2, E2, n, dead = R.restart(cs, W, E, cand, 1.0)   # six dead, four candidates: the lowest four, in order
    assert (n, dead) == (4, 6)
    for j, k in enumerate((0, 2, 5, 7)):
        assert np.array_equal(E2[k], cand[j]) and np.array_equal(W2[k], cand[j]) and cs2[k] == 1.0
    for k in (9, 11):                                        # past the cap: they wait
        assert cs2[k] == 0.25 and np.array_equal(E2[k], E[k]) and np.array_equal(W2[k], W[k])
    alive = [k for k in range(12) if k not in (0, 2, 5, 7)]
    assert np.array_equal(cs2[alive], cs[alive]) and np.array_equal(E2[alive], E[alive]) and np.array_equal(W2[alive], W[alive])
    # fewer dead than candidates: exactly the dead ones move
    cs3, _, E3, n3, dead3 = R.restart(cs2, W2, E2, cand, 1.0)
    assert (n3, dead3) == (2, 2) and np.array_equal(E3[9], cand[0]) and np.array_equal(E3[11], cand[1])
    assert np.array_equal(E3[[0, 2, 5, 7]], cand)


def test_a_restarted_code_sits_on_its_candidate():
    cs, W, E, cand = _state(seed=3)
    cs[[1, 4]] = 1e-3
    for thr in (1.0, 0.7, 1.9):                              # (the other codes are alive above 2)
        cs2, W2, E2, n, _ = R.restart32(cs, W, E, cand, thr)
        assert n == 2 and cs2[1] == np.float32(thr) and cs2[4] == np.float32(thr)
        assert np.array_equal(E2[[1, 4]], cand[:2].astype(np.float32))
        assert np.array_equal(W2[[1, 4]], cand[:2].astype(np.float32) * np.float32(thr))
        np.testing.assert_allclose(W2[[1, 4]] / cs2[[1, 4], None], cand[:2], rtol=3e-7)
        assert W2.dtype == np.float32


def test_step_is_the_update_then_the_restart():
    g = np.random.default_rng(5)
    K, D = 8, 4
    rows = g.normal(size=(40, D))
    idx = np.arange(40) % 3                                # 14, 13, 13 rows; codes 3..7 win nothing
    cs0, W0 = np.zeros(K), g.normal(size=(K, D))
    cs, W, E, n, dead = R.step(cs0, W0, rows, idx, 0.9, 1e-5, rows[[7, 3]], 1.0)
    ucs, uW, uE = E_.step(cs0, W0, rows, idx, 0.9, 1e-5)
    assert (n, dead) == (2, 5) and np.array_equal(E[3], rows[7]) and np.array_equal(E[4], rows[3])
    assert np.array_equal(E[:3], uE[:3]) and np.array_equal(cs[5:], ucs[5:]) and np.array_equal(W[5:], uW[5:])
    c, s = E_.stats(rows, idx, K)
    cs32, W32, E32, n32, dead32 = R.step32(cs0, W0, c, s, 0.9, 1e-5, rows[[7, 3]], 1.0)
    assert (n32, dead32) == (2, 5) and E32.dtype == np.float32 and np.array_equal(E32[3], rows[7].astype(np.float32))


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_planted_collapse_on_the_restatement(seed):
    """48 planted clusters, 64 codes from a unit normal, cluster sizes from zero: without restarts about half of the codebook
    is in use after 40 steps, with them nearly all of it, at a fraction of the quantisation error."""
    used_off, mse_off, _ = R.planted(seed, False)
    used_on, mse_on, total = R.planted(seed, True)
    print("seed %d: used %d -> %d, mse %.3f -> %.3f, %d restarts" % (seed, used_off, used_on, mse_off, mse_on, total))
    assert used_off <= 40
    assert used_on >= 56
    assert mse_on * 3 <= mse_off
    assert total > 0


# ------------------------------------------------------------------------------------------------- keyword contract
@pytest.fixture
def no_launch(monkeypatch):
    """Any call that gets as far as the library fails the test."""
    from acoustic_locating_vq_vae import _native

    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(_native, "lib", boom)


def test_keyword_errors_come_before_the_library(no_launch):
    with pytest.raises(ValueError, match="dead_code_threshold"):
        VectorQuantizerEMA(16, 4, 0.25, 0.99, dead_code_threshold=-1.0)
    with pytest.raises(ValueError, match="dead_code_threshold"):
        VectorQuantizerEMA(16, 4, 0.25, 0.99, dead_code_threshold=float("nan"))
    for r in (0, 17, -3):
        with pytest.raises(ValueError, match="restart_candidates"):
            VectorQuantizerEMA(16, 4, 0.25, 0.99, dead_code_threshold=1.0, restart_candidates=r)
        with pytest.raises(ValueError, match="restart_candidates"):
            ConvolutionalVQVAE(*CFG, decay=0.99, dead_code_threshold=1.0, restart_candidates=r + 48 if r > 0 else r)
    with pytest.raises(ValueError, match="dead_code_threshold"):
        ConvolutionalVQVAE(*CFG, decay=0.99, dead_code_threshold=-0.5)
    with pytest.raises(ValueError, match="decay"):
        ConvolutionalVQVAE(*CFG, dead_code_threshold=1.0)                       # decay == 0: no usage state to test
    with pytest.raises(ValueError, match="decay"):
        ConvolutionalVQVAE(*CFG, decay=0.0, dead_code_threshold=0.5, restart_candidates=8)
    VectorQuantizerEMA(16, 4, 0.25, 0.99)                                      # the default R = 64 > K is no error when off
    vq = VectorQuantizerEMA(16, 4, 0.25, 0.99, dead_code_threshold=2.0, restart_candidates=16, restart_seed=5)
    assert (vq._dead_code_threshold, vq._restart_candidates, vq._restart_seed) == (2.0, 16, 5)
    m = ConvolutionalVQVAE(*CFG, decay=0.9, dead_code_threshold=1.5, restart_candidates=8, restart_seed=2)
    assert (m._vq._dead_code_threshold, m._vq._restart_candidates, m._vq._restart_seed) == (1.5, 8, 2)
    assert m._vq.restarts_enabled() and not ConvolutionalVQVAE(*CFG, decay=0.9)._vq.restarts_enabled()


def test_restarts_leave_keys_draws_and_pickles_alone(no_launch):
    torch.manual_seed(7)
    a = ConvolutionalVQVAE(*CFG, decay=0.99)
    after_a = torch.rand(4)
    torch.manual_seed(7)
    b = ConvolutionalVQVAE(*CFG, decay=0.99, dead_code_threshold=1.0, restart_candidates=8, restart_seed=3)
    assert torch.equal(after_a, torch.rand(4))                                 # the global generator: the same draws
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not hasattr(a._vq, "_restart_gen") and not hasattr(a._vq, "_restart_rows")
    assert a._vq.restarted_codes() == (0, 0)                                   # off: no device read either
    assert b._vq._restart_rows.dtype == torch.int64 and b._vq._restart_rows.shape == (8,)
    r = pickle.loads(pickle.dumps(b))
    assert r._vq.restarts_enabled() and torch.equal(r._vq._restart_gen.get_state(), b._vq._restart_gen.get_state())
    assert list(r.state_dict()) == list(sb)


def test_positions_are_distinct_private_and_reproducible(no_launch):
    vq = VectorQuantizerEMA(64, 4, 0.25, 0.9, dead_code_threshold=1.0, restart_candidates=32, restart_seed=11)
    torch.manual_seed(1)
    before = torch.rand(3)
    torch.manual_seed(1)
    seen = []
    for rows in (32, 33, 100, 5000, 1 << 20):
        vq.draw_restart_rows(rows)
        got = vq._restart_rows.tolist()
        assert len(set(got)) == 32 and min(got) >= 0 and max(got) < rows
        seen.append(got)
    assert torch.equal(before, torch.rand(3))                                  # never the global generator
    assert sorted(seen[0]) == list(range(32))                                  # rows == R: every row once
    again = VectorQuantizerEMA(64, 4, 0.25, 0.9, dead_code_threshold=1.0, restart_candidates=32, restart_seed=11)
    for rows, want in zip((32, 33, 100, 5000, 1 << 20), seen):
        again.draw_restart_rows(rows)
        assert again._restart_rows.tolist() == want
    other = VectorQuantizerEMA(64, 4, 0.25, 0.9, dead_code_threshold=1.0, restart_candidates=32, restart_seed=12)
    other.draw_restart_rows(5000)
    assert other._restart_rows.tolist() != seen[3]
    vq.draw_restart_rows(5000, 3)                                              # a rank's share: the first n entries
    assert len(set(vq._restart_rows[:3].tolist())) == 3
    with pytest.raises(ValueError, match="rows"):
        vq.draw_restart_rows(31)
    # uniform: over many draws of 2 from 8 every position comes up about equally often
    small = VectorQuantizerEMA(8, 4, 0.25, 0.9, dead_code_threshold=1.0, restart_candidates=2)
    hits = np.zeros(8)
    for _ in range(4000):
        small.draw_restart_rows(8)
        hits[small._restart_rows.tolist()] += 1
    assert hits.min() > 850 and hits.max() < 1150, hits                      # mean 1000, sd 27


def test_restart_abi_argument_checks():
    """The two entry points refuse bad arguments before any launch (no GPU here: a launch would fail differently)."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native
    lib = _native.lib()
    fake = 256                                                                 # never dereferenced: the checks come first
    ok = (fake, fake, fake, fake, 100, 16, 8)
    for first, stride in ((0, 0), (2, 2), (-1, 1)):
        rc = lib.alvq_vq_restart_gather_f32(*ok, first, stride, None)
        assert rc < 0 and b"stride" in lib.alvq_last_error()
    assert lib.alvq_vq_restart_gather_f32(fake, fake, fake, fake, 100, 513, 8, 0, 1, None) < 0 and b"512" in lib.alvq_last_error()
    assert lib.alvq_vq_restart_gather_f32(fake, fake, fake, None, 100, 16, 8, 0, 1, None) < 0 and b"null" in lib.alvq_last_error()
    assert lib.alvq_vq_restart_gather_f32(fake, fake, fake, fake, 0, 16, 8, 0, 1, None) < 0
    dead = lib.alvq_vq_restart_dead_f32
    assert dead(fake, fake, fake, fake, None, fake, 16385, 4, 8, 1.0, None) < 0 and b"16384" in lib.alvq_last_error()
    assert dead(fake, fake, fake, fake, None, fake, 64, 513, 8, 1.0, None) < 0 and b"512" in lib.alvq_last_error()
    for r in (0, 65):
        assert dead(fake, fake, fake, fake, None, fake, 64, 4, r, 1.0, None) < 0 and b"R=" in lib.alvq_last_error()
    assert dead(fake, fake, fake, fake, None, fake, 64, 4, 8, -1.0, None) < 0 and b"threshold" in lib.alvq_last_error()
    assert dead(fake, fake, fake, fake, None, fake, 64, 4, 8, float("nan"), None) < 0
    assert dead(fake, fake, fake, fake, None, None, 64, 4, 8, 1.0, None) < 0 and b"null" in lib.alvq_last_error()
    assert {"alvq_vq_restart_gather_f32", "alvq_vq_restart_dead_f32"} <= set(_native.EXPORTS)
