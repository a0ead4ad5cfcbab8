"""Speech measures, the parts that need no GPU: the host-side filter design and band edges of acoustic_locating_vq_vae.
speech_metrics, the float64 restatement (tests/helpers/speech_metrics_ref.py) on inputs whose answer is known, and the
host-side argument rules."""
import os
import sys

import numpy as np
import pytest
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import speech_metrics_ref as R  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as M  # noqa: E402

BAND_LO = [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
BAND_HI = BAND_LO[1:] + [219]


@pytest.mark.parametrize("up,down", [(5, 8), (3, 2), (160, 441)])
def test_filter_design_is_scipys(up, down):
    h, u, d = M.resample_filter(up, down)
    R_ = max(u, d)
    assert (u, d) == (up, down) and h.dtype == np.float64 and h.shape == (20 * R_ + 1,)
    want = scipy.signal.firwin(20 * R_ + 1, 1.0 / R_, window=("kaiser", 5.0)) * up
    err = np.abs(h - want).max()
    print("%d/%d: max |h - firwin| = %.3g" % (up, down, err))
    assert err <= 1e-15
    assert np.array_equal(h, R.resample_filter(up, down)[0])


def test_filter_ratio_is_reduced_by_the_gcd():
    h, u, d = M.resample_filter(10000, 16000)
    assert (u, d) == (5, 8) and np.array_equal(h, M.resample_filter(5, 8)[0])


def test_band_edges():
    assert M.stoi_band_edges() == (BAND_LO, BAND_HI)
    assert R.band_edges() == (BAND_LO, BAND_HI)


def test_restatement_of_identical_signals_is_one():
    x = np.random.default_rng(0).standard_normal(5248)
    r = R.stoi(x, x)
    assert r.status == 0 and r.kept_frames == r.nf == 40 and abs(r.value - 1.0) <= 1e-12


def test_restatement_falls_as_noise_is_added():
    g = np.random.default_rng(1)
    x, noise = g.standard_normal(5248), g.standard_normal(5248)
    values = [R.stoi(x, x + noise * 10.0 ** (-snr / 20.0)).value for snr in (10.0, 0.0, -10.0)]
    print("stoi at +10, 0, -10 dB SNR:", values)
    assert 1.0 > values[0] > values[1] > values[2] > 0.0


def test_restatement_status_rows():
    g = np.random.default_rng(2)
    x = g.standard_normal(5248)
    r = R.stoi(x[:255], x[:255])
    assert np.isnan(r.value) and r.kept_frames == 0 and r.nf == 0 and r.status == R.BAD_ENERGY
    assert R.stoi(np.zeros(5248), x).status == R.BAD_ENERGY
    bad = x.copy()
    bad[100] = np.inf
    assert R.stoi(bad, x).status == R.BAD_ENERGY
    r = R.stoi(x[:3967], x[:3967])
    assert r.status == R.FEW_FRAMES and r.kept_frames == 29 and np.isnan(r.value)


def test_restatement_of_si_sdr_and_lsd():
    g = np.random.default_rng(3)
    s, noise = g.standard_normal(4000), g.standard_normal(4000)
    # orthogonalised noise at a tenth of the energy: 10 dB, whatever the estimate's gain and offset
    s0 = s - s.mean()
    noise = noise - noise.mean()
    noise -= s0 * (noise @ s0) / (s0 @ s0)
    noise *= np.sqrt((s0 @ s0) / (noise @ noise) / 10.0)
    assert abs(R.si_sdr(s, 0.3 * (s + noise) + 2.0) - 10.0) <= 1e-9
    assert R.si_sdr(s, -4.0 * s) == np.inf and np.isnan(R.si_sdr(np.full(10, 3.0), s[:10]))
    p = g.random((65, 7)) + 0.1
    assert abs(R.log_spectral_distance(p, 100.0 * p, eps=0.0) - 20.0) <= 1e-12
    assert R.log_spectral_distance(p, p) == 0.0
    q = p.copy()
    q[3, 2] = -1e-3
    assert np.isnan(R.log_spectral_distance(p, q)) and np.isnan(R.log_spectral_distance(q, p))


def test_host_side_rejections():
    x = torch.zeros(2, 4000, dtype=torch.float64)
    for call in (M.stoi, M.si_sdr):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(x, x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(x[0].float(), x[0].float())
        for a, b in ((x, x[:, :3999]), (x, x[0]), (x, x.float()), (x.half(), x.half()), (x[None], x[None]),
                     (x.numpy(), x.numpy()), (x[:, :1], x[:, :1]), (x[:0], x[:0])):
            with pytest.raises(ValueError):
                call(a, b)
    for fs in (16000.0, "16000", None, 0, -8000, True):
        with pytest.raises(ValueError, match="fs"):
            M.stoi(x, x, fs=fs)
    with pytest.raises(ValueError, match="512"):
        M.stoi(x, x, fs=10007)                       # 10000 / 10007 does not reduce
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.stoi(x, x, fs=10000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.resample_poly(x, 5, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.resample_poly(x[0, :1], 5, 8)              # a single sample is a signal to the resampler
    for up, down in ((513, 1), (1, 1026 // 2 + 1), (0, 3), (3, -1), (2.0, 3), (True, 3)):
        with pytest.raises(ValueError):
            M.resample_poly(x, up, down)
    with pytest.raises(ValueError):
        M.resample_poly(torch.zeros(2, 3, 4), 5, 8)
    p = torch.zeros(2, 65, 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.log_spectral_distance(p, p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.log_spectral_distance(p[0].double(), p[0].double())
    for a, b in ((p, p[:, :, :8]), (p, p.double()), (p[0, 0], p[0, 0]), (p.half(), p.half()), (p[:, :0], p[:, :0])):
        with pytest.raises(ValueError):
            M.log_spectral_distance(a, b)
    for eps in (-1e-10, float("nan"), "0", None):
        with pytest.raises(ValueError, match="eps"):
            M.log_spectral_distance(p, p, eps=eps)


def test_entry_points_check_their_arguments_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native as N
    lib = N.lib()
    p = 4096            # never dereferenced: every call below is rejected first

    def rejected(name, good, bads):
        fn = getattr(lib, name)
        for pos, bad in bads:
            args = list(good)
            args[pos] = bad
            assert fn(*args, None) == -1, (name, pos, bad)
            assert lib.alvq_last_error().startswith(name.encode()), (name, pos, bad, lib.alvq_last_error())

    for sfx in ("f32", "f64"):
        rejected("alvq_resample_poly_" + sfx, [p, p, p, 1, 100, 5, 8, 80],
                 [(0, None), (1, None), (2, None), (3, 0), (3, 65536), (4, 0), (4, (1 << 24) + 1), (5, 0), (5, 513), (6, 0),
                  (6, 513), (7, -1), (7, 5121)])
        rejected("alvq_si_sdr_" + sfx, [p, p, p, 1, 100], [(0, None), (1, None), (2, None), (3, 0), (4, 1), (4, (1 << 24) + 1)])
        rejected("alvq_lsd_" + sfx, [p, p, p, 1, 65, 9, 1e-10],
                 [(0, None), (1, None), (2, None), (3, 0), (4, 0), (5, 0), (4, 1 << 30), (6, -1.0), (6, float("nan"))])
    import ctypes
    lo, hi = (ctypes.c_int * 15)(*BAND_LO), (ctypes.c_int * 15)(*BAND_HI)
    lo_p, hi_p = ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(hi, ctypes.c_void_p)
    backwards = ctypes.cast((ctypes.c_int * 15)(*BAND_HI), ctypes.c_void_p)
    negative = ctypes.cast((ctypes.c_int * 15)(*([-1] + BAND_LO[1:])), ctypes.c_void_p)
    low = ctypes.cast((ctypes.c_int * 15)(*([0] + BAND_LO[1:])), ctypes.c_void_p)
    high = ctypes.cast((ctypes.c_int * 15)(*(BAND_HI[:-1] + [257])), ctypes.c_void_p)
    past = ctypes.cast((ctypes.c_int * 15)(*(BAND_HI[:-1] + [258])), ctypes.c_void_p)
    rejected("alvq_stoi_f64", [p, p, lo_p, hi_p, p, p, p, p, 1, 4000],
             [(i, None) for i in range(8)] + [(8, 0), (8, 65536), (9, 1), (9, (1 << 24) + 1), (2, backwards), (2, negative), (3, past)])
    # bands that span more than the 256 bins one workgroup transforms
    assert lib.alvq_stoi_f64(p, p, low, high, p, p, p, p, 1, 4000, None) == -1 and b"span" in lib.alvq_last_error()
    assert lib.alvq_stoi_workspace_bytes(2, 3968) == 2 * 30 * (8 + 240 + 4) + 256
    assert lib.alvq_stoi_workspace_bytes(1, 255) == 256
    assert lib.alvq_stoi_workspace_bytes(0, 4000) == lib.alvq_stoi_workspace_bytes(1, 1) == -1
    assert lib.alvq_stoi_workspace_bytes(1, (1 << 24) + 1) == -1
