"""WPE dereverberation, the parts that need no GPU: the numpy restatement (tests/helpers/wpe_ref.py) is pinned -- float64
against np.longdouble, on inputs it must dereverberate, and on the bins it must refuse -- so that the yardstick of
tests/test_wpe_gpu.py is itself a WPE; and the host-side argument rules of acoustic_locating_vq_vae.dereverberation.

Float64 against longdouble: max |Y - Y_ld| <= 8 M u cond_2(R) max |x| with u = 1.1e-16, the forward bound c n u kappa of a
Cholesky solve.  Dereverberation: sum |Y - S|^2 / sum |X - S|^2, the share of the reverberation's energy that is left, on the
inputs of ``ar_bin`` (a clean excitation through a stable delayed autoregression, the model WPE inverts)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import wpe_ref as R  # noqa: E402
from acoustic_locating_vq_vae import dereverberation as DV  # noqa: E402

U = 1.1e-16
# (B, D, F, T, taps, delay, psd_context, loading): the parity shapes of tests/test_wpe_gpu.py
PARITY = [(2, 1, 9, 64, 1, 1, 0, 1e-10), (2, 1, 9, 96, 5, 3, 0, 1e-10), (1, 1, 5, 200, 10, 3, 0, 1e-10),
          (1, 1, 3, 500, 10, 3, 1, 1e-10), (2, 2, 5, 200, 8, 2, 0, 1e-10), (1, 4, 3, 300, 16, 3, 0, 1e-10),
          (1, 3, 4, 257, 7, 3, 2, 1e-10), (1, 1, 3, 12, 10, 3, 0, 1e-3), (1, 2, 3, 40, 32, 1, 0, 1e-3),
          (1, 4, 2, 2000, 16, 3, 0, 1e-10), (2, 1, 201, 500, 10, 3, 0, 1e-10)]
LONGDOUBLE_BINS = 4          # bins per shape taken through the (slow) longdouble restatement


@pytest.mark.parametrize("B,D,F,T,taps,delay,ctx,loading", PARITY)
def test_float64_restatement_against_longdouble(B, D, F, T, taps, delay, ctx, loading):
    c = R.case(B, D, F, T, taps, delay, ctx, loading)
    assert not c.status.any() and c.cond.max() <= R.COND_CAP
    worst = 0.0
    for n in range(min(LONGDOUBLE_BINS, B * F)):
        b, f = divmod(n, F)
        y_ld, st, _ = R.wpe_bin(c.X[b, :, f], taps, delay, 3, ctx, 1e-10, loading, dtype=np.longdouble)
        err = float(np.abs(c.Y[b, :, f] - y_ld).max())
        bound = 8 * D * taps * U * c.cond[b, f] * np.abs(c.X[b, :, f]).max()
        worst = max(worst, err / bound)
        assert st == 0 and err <= bound, (b, f, err, bound)
    print("%s: largest |Y - Y_ld| / bound %.3g, cond up to %.3g" % ((B, D, F, T, taps, delay, ctx), worst, c.cond.max()))


@pytest.mark.parametrize("T,D,taps,delay,ctx,limit", [(500, 1, 10, 3, 1, 0.1), (257, 3, 7, 3, 2, 0.5)])
def test_restatement_dereverberates(T, D, taps, delay, ctx, limit):
    for s in range(4):
        S, X = R.ar_bin(T, D, min(taps, 6), delay, R.bin_seed(s, T, D))
        Y, st, cond = R.wpe_bin(X, taps, delay, 3, ctx)
        left = float(np.sum(np.abs(Y - S) ** 2) / np.sum(np.abs(X - S) ** 2))
        print("T %d D %d seed %d: reverberant energy left %.4f, cond %.3g" % (T, D, R.bin_seed(s, T, D), left, cond))
        assert st == 0 and left <= limit


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_restatement_refuses_bad_bins(dtype):
    _, X = R.ar_bin(40, 2, 3, 1, 5)
    Y, st, _ = R.wpe_bin(np.zeros((2, 40), complex), 3, 1, dtype=dtype)
    assert st == R.BAD_POWER == 1 and not Y.any()
    bad = X.copy()
    bad[1, 7] = np.nan
    Y, st, _ = R.wpe_bin(bad, 3, 1, dtype=dtype)
    assert st == R.BAD_POWER and np.array_equal(Y.astype(complex), bad, equal_nan=True)
    for T in (2, 3):                                   # T <= delay: no frame has a past, R = 0
        Y, st, _ = R.wpe_bin(X[:, :T], 4, 3, dtype=dtype)
        assert st == R.BAD_PIVOT == 2 and np.array_equal(Y.astype(complex), X[:, :T])
    Y, st, _ = R.wpe_bin(X[:, :4], 4, 3, loading=1e-3, dtype=dtype)       # one frame with a past is enough once R is loaded
    assert st == 0


def test_stacked_past_layout():
    X = np.arange(1, 11).reshape(2, 5) * (1 + 1j)
    Xt = R.stack_past(X, 2, 1)                          # entry k D + d at t: x_d[t - 1 - k]
    assert Xt.shape == (4, 5)
    assert np.array_equal(Xt[0], [0, X[0, 0], X[0, 1], X[0, 2], X[0, 3]])
    assert np.array_equal(Xt[1], [0, X[1, 0], X[1, 1], X[1, 2], X[1, 3]])
    assert np.array_equal(Xt[2], [0, 0, X[0, 0], X[0, 1], X[0, 2]])
    assert np.array_equal(Xt[3], [0, 0, X[1, 0], X[1, 1], X[1, 2]])


SPEC = torch.zeros(2, 1, 5, 20, dtype=torch.complex128)


@pytest.mark.parametrize("spec,kwargs", [
    (SPEC.real, {}),                                            # not complex
    (SPEC.to(torch.complex32), {}),
    (SPEC[0, 0, 0], {}),                                        # one dimension
    (SPEC[None], {}),                                           # five
    ("spec", {}),
    (torch.zeros(1, 9, 5, 20, dtype=torch.complex64), {"taps": 1}),     # nine microphones
    (torch.zeros(1, 8, 5, 20, dtype=torch.complex64), {"taps": 9}),     # D taps = 72
    (torch.zeros(1, 0, 5, 20, dtype=torch.complex64), {}),
    (torch.zeros(0, 5, 20, dtype=torch.complex64), {}),
    (torch.zeros(5, 0, dtype=torch.complex64), {}),             # no frames
    (torch.zeros(0, 20, dtype=torch.complex64), {}),            # no bins
    (SPEC, {"taps": 0}), (SPEC, {"taps": 65}), (SPEC, {"taps": 2.0}), (SPEC, {"taps": True}),
    (SPEC, {"delay": -1}), (SPEC, {"delay": 65}), (SPEC, {"delay": 1.5}),
    (SPEC, {"iterations": 0}), (SPEC, {"iterations": 17}),
    (SPEC, {"psd_context": -1}), (SPEC, {"psd_context": 65}),
    (SPEC, {"eps": -1e-3}), (SPEC, {"eps": float("nan")}), (SPEC, {"eps": float("inf")}), (SPEC, {"eps": "small"}),
    (SPEC, {"loading": -1.0}), (SPEC, {"loading": float("inf")}), (SPEC, {"loading": None}),
])
def test_wpe_argument_rules(spec, kwargs):
    with pytest.raises(ValueError, match="^wpe: "):
        DV.wpe(spec, **kwargs)


def test_wpe_too_many_frames():
    with pytest.raises(ValueError, match="T <= 65535"):
        DV.wpe(torch.zeros(1, 65536, dtype=torch.complex64))


def test_cpu_tensors_are_refused_last():
    for spec in (SPEC, SPEC[:, 0], SPEC[0, 0], SPEC.to(torch.complex64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            DV.wpe(spec)
    with pytest.raises(ValueError, match="^wpe: taps"):          # the ranges come first
        DV.wpe(SPEC, taps=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DV.dereverberate(torch.zeros(2, 4000))


@pytest.mark.parametrize("wave", [torch.zeros(2, 3, 400), torch.zeros(400, dtype=torch.float16), torch.zeros(400, dtype=torch.int32),
                                  np.zeros(400)])
def test_dereverberate_argument_rules(wave):
    with pytest.raises(ValueError, match="^dereverberate: "):
        DV.dereverberate(wave)
