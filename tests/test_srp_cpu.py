"""GCC-PHAT / SRP-PHAT localisation, the parts that need no GPU: the numpy restatement (tests/helpers/srp_ref.py) is pinned --
float64 against np.longdouble to the bounds tests/test_srp_gpu.py holds the device to, on inputs whose source it must find, on
the items it must flag, and through an image-source room -- so that the yardstick of the GPU test is itself a locator; and
the host-side argument rules of acoustic_locating_vq_vae.localization.

The bounds, with u = 1.1e-16 (derived in srp_ref): cross-spectra (T + 8) u; map (P F_band + T + 16 Theta + 32 + K) u, K = 8 for the
kernel's rotation recurrence, with
Theta = 2 pi f_hi (fs / n_fft) max tau, the phase of the longest path at the top bin; GCC (F_band + T + 8 pi L + 32) u."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import dsp_ref  # noqa: E402
import rir_ref  # noqa: E402
import srp_ref as R  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import localization as LOC  # noqa: E402

GCC_LAGS = 8
IDS = ["-".join(str(v) for v in s) for s in R.PARITY]


# ------------------------------------------------------------------------------------------ the restatement against longdouble
@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
def test_float64_restatement_against_longdouble(shape):
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c, ref = R.parity_case(shape), R.reference(shape)
    psi_ld, st_ld = R.cross_spectra(c.X, f_lo, f_hi, dtype=np.longdouble)
    S_ld, best_ld, status_ld = R.srp_phat(psi_ld, c.mics, c.cand, R.FS, n_fft, R.C, f_lo, f_hi, dtype=np.longdouble)
    theta = R.theta_max(f_hi, R.FS, n_fft, c.mics, c.cand)
    e_psi, b_psi = float(np.abs(ref.psi - psi_ld).max()), R.psi_bound(T)
    e_map, b_map = float(np.abs(ref.map - S_ld).max()), R.map_bound(D, T, f_lo, f_hi, theta)
    L = min(GCC_LAGS, n_fft // 2)
    e_gcc = float(np.abs(R.gcc_phat(ref.psi, n_fft, L, f_lo, f_hi) - R.gcc_phat(psi_ld, n_fft, L, f_lo, f_hi, np.longdouble)).max())
    b_gcc = R.gcc_bound(T, f_lo, f_hi, L)
    print("%s: measured / bound: psi %.3g, map %.3g (bound %.3g, Theta %.4g), gcc %.3g"
          % (shape, e_psi / b_psi, e_map / b_map, b_map, theta, e_gcc / b_gcc))
    assert not ref.status.any() and not status_ld.any() and not st_ld.any()
    assert e_psi <= b_psi and e_map <= b_map and e_gcc <= b_gcc
    assert np.array_equal(best_ld, ref.best)


@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
@pytest.mark.parametrize("single", [False, True], ids=["complex128", "complex64"])
def test_restatement_finds_the_true_candidate(shape, single):
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c, ref = R.parity_case(shape), R.reference(shape, single)
    bound = R.map_bound(D, T, f_lo, f_hi, R.theta_max(f_hi, R.FS, n_fft, c.mics, c.cand))
    print("%s: arg-max %s, true %s, gap to the runner-up %s, 1e3 x bound %.3g" % (shape, ref.best, c.true, ref.gap, 1e3 * bound))
    assert np.array_equal(ref.best, c.true)
    assert (ref.gap > 1e3 * bound).all()
    assert np.abs(ref.map).max() <= 1 + bound


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_gcc_peak_lag_is_arrival_at_i_minus_arrival_at_j(dtype):
    """A noiseless two-microphone case: the peak lag of the restatement's GCC is (r_i - r_j) fs / c, rounded."""
    n_fft, F, T = 400, 201, 6
    g = np.random.default_rng(11)
    mics = np.array([[2.5, 1.5, 1.5], [2.5, 1.8, 1.5]])
    for src in ([3.5, 3.0, 1.5], [1.0, 0.5, 2.0]):                  # 11.33 and -8.29 samples
        r = np.linalg.norm(np.array(src) - mics, axis=1)
        S = g.standard_normal((F, T)) + 1j * g.standard_normal((F, T))
        omega = 2 * np.pi * np.arange(F) * R.FS / n_fft
        X = np.stack([S * np.exp(-1j * omega * rd / R.C)[:, None] / rd for rd in r])[None]
        psi, st = R.cross_spectra(X, 1, 199, dtype)
        corr = R.gcc_phat(psi, n_fft, 20, 1, 199, dtype)
        want = (r[0] - r[1]) * R.FS / R.C
        assert st[0] == 0 and abs(want) > 3
        assert int(np.argmax(corr[0, 0])) - 20 == int(np.round(want))


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_restatement_flags_bad_items(dtype):
    shape = R.PARITY[1]
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c = R.parity_case(shape)
    X = np.concatenate([c.X, c.X[:1], c.X[:1]])
    X[0, :, f_lo:f_hi + 1] = 0                        # silent inside the band
    X[1, 1, f_lo + 3, 2] = complex(1.0, np.nan)       # one NaN inside the band
    X[2, 0, f_hi + 1, 0] = np.nan                     # a NaN outside the band does not flag
    mics = np.broadcast_to(c.mics, (4, D, 3)).copy()
    mics[3, 1, 2] = np.nan
    psi, st = R.cross_spectra(X, f_lo, f_hi, dtype)
    assert list(st) == [2, 1, 0, 0]
    S, best, status = R.srp_phat(psi, mics, c.cand, R.FS, n_fft, R.C, f_lo, f_hi, dtype, spectrum_status=st)
    assert list(status) == [2, 1, 0, 4] and list(best[[0, 1, 3]]) == [-1, -1, -1] and best[2] == c.true[0]
    assert not S[0].any() and np.isnan(S[1]).all() and np.isnan(S[3]).all() and np.isfinite(S[2]).all()
    assert list(R.srp_phat(psi, mics, c.cand, R.FS, n_fft, R.C, f_lo, f_hi, dtype)[2]) == [2, 1, 0, 4]     # status from psi alone
    cand = c.cand.copy()
    cand[5, 0] = np.inf
    assert list(R.srp_phat(psi, c.mics, cand, R.FS, n_fft, R.C, f_lo, f_hi, dtype)[2]) == [6, 5, 4, 4]


def test_pairs_and_weights():
    assert R.pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert list(R.weights(400, 0, 3)) == [1, 2, 2, 2] and list(R.weights(400, 198, 200)) == [2, 2, 1]
    assert list(R.weights(401, 199, 200)) == [2, 2]                          # odd n_fft: no Nyquist bin
    u = R.unit(np.array([0j, 3 + 4j, 1e-320 + 0j, 1e300 + 1e300j]))
    assert u[0] == 0 and abs(u[1] - (0.6 + 0.8j)) < 1e-15 and u[2] == 1 and abs(abs(u[3]) - 1) < 1e-15


# ------------------------------------------------------------------------------------------------------------------ the room
ROOM_ANGLES = (5, 23, 40, 61)


def room_setup():
    """DATASET_CONFIG's room: four microphones on a tetrahedron of radius 0.05 m around the receiver, one second of noise under
    the envelope of the WPE room test, 72 ring candidates."""
    cfg = FE.DATASET_CONFIG
    fs, n = cfg["fs"], 16000
    g = np.random.default_rng(3)
    t = np.arange(n) / fs
    envelope = (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + 0.3)) * (0.6 + 0.4 * np.sin(2 * np.pi * 1.3 * t))
    wave = (g.standard_normal(n) * envelope).astype(np.float32)
    rcv = np.array(cfg["receiver_position"], dtype=np.float64)
    mics = rcv + 0.05 / np.sqrt(3.0) * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)
    room = np.array(cfg["room_dimensions"], dtype=np.float64)
    cand = np.minimum(R.ring(72, rcv, cfg["R"], cfg["Z_LOC_SOURCE"]), room)
    return cfg, wave, rcv, mics, room, cand


@pytest.mark.parametrize("k", ROOM_ANGLES)
def test_restatement_locates_a_source_in_the_room(k):
    """rir_ref.rir -> dsp_ref.fir_same -> dsp_ref.stft -> the restatement, band (8, 187): the arg-max lies within one ring
    candidate of the source's (circular distance)."""
    cfg, wave, rcv, mics, room, cand = room_setup()
    beta = rir_ref.sabine_beta(room, FE.SOUND_SPEED, cfg["reverberation_time"])
    h = np.stack([rir_ref.rir(FE.SOUND_SPEED, cfg["fs"], m, cand[k], room, beta, cfg["n_sample"]) for m in mics])
    echoed = dsp_ref.fir_same(np.broadcast_to(wave.astype(np.float64), (4, wave.size)), h)[0]
    X = dsp_ref.stft(echoed, 400, 160)[0].astype(np.complex128)[None]
    psi, st = R.cross_spectra(X, 8, 187)
    S, best, status = R.srp_phat(psi, mics, cand, cfg["fs"], 400, FE.SOUND_SPEED, 8, 187, spectrum_status=st)
    dist = min((int(best[0]) - k) % 72, (k - int(best[0])) % 72)
    print("source on candidate %d: arg-max %d, peak %.4f" % (k, best[0], S[0].max()))
    assert status[0] == 0 and dist <= 1


# -------------------------------------------------------------------------------------------------------------- host checks
SPEC = torch.zeros(2, 4, 201, 6, dtype=torch.complex128)
MICS = torch.zeros(4, 3, dtype=torch.float64)
CAND = torch.zeros(9, 3, dtype=torch.float64)


@pytest.mark.parametrize("spec,kwargs", [
    (SPEC.real, {}), (SPEC.to(torch.complex32), {}), (SPEC[0, 0], {}), (SPEC[None], {}), ("spec", {}),
    (torch.zeros(1, 9, 201, 6, dtype=torch.complex64), {}),             # nine microphones
    (torch.zeros(1, 1, 201, 6, dtype=torch.complex64), {}),             # one
    (torch.zeros(0, 4, 201, 6, dtype=torch.complex64), {}),
    (torch.zeros(4, 201, 0, dtype=torch.complex64), {}),                # no frames
    (torch.zeros(4, 0, 6, dtype=torch.complex64), {}),                  # no bins
    (torch.zeros(4, 2, 6, dtype=torch.complex64), {}),                  # the default band is empty
    (SPEC, {"band": (5, 4)}), (SPEC, {"band": (-1, 4)}), (SPEC, {"band": (0, 201)}), (SPEC, {"band": (1.0, 4)}),
    (SPEC, {"band": 7}), (SPEC, {"band": (1, 2, 3)}), (SPEC, {"band": (True, 4)}),
])
def test_cross_spectra_argument_rules(spec, kwargs):
    with pytest.raises(ValueError, match="^cross_spectra: "):
        LOC.cross_spectra(spec, **kwargs)


def test_cross_spectra_too_many_frames():
    with pytest.raises(ValueError, match="T <= 65535"):
        LOC.cross_spectra(torch.zeros(2, 3, 65536, dtype=torch.complex64))


@pytest.mark.parametrize("kwargs", [{"max_lag": -1}, {"max_lag": 201}, {"max_lag": 2.0}, {"max_lag": True}, {"max_lag": 4, "n_fft": 512},
                                    {"max_lag": 4, "n_fft": 400.0}, {"max_lag": 4, "band": (3, 2)}])
def test_gcc_phat_argument_rules(kwargs):
    with pytest.raises(ValueError, match="^gcc_phat: "):
        LOC.gcc_phat(SPEC, **kwargs)


@pytest.mark.parametrize("kwargs", [{"fs": 0}, {"fs": float("nan")}, {"fs": "16k"}, {"fs": -16000.0}])
def test_tdoa_argument_rules(kwargs):
    with pytest.raises(ValueError, match="^tdoa: "):
        LOC.tdoa(SPEC, 4, **kwargs)
    with pytest.raises(ValueError, match="^gcc_phat: max_lag"):
        LOC.tdoa(SPEC, 500)


@pytest.mark.parametrize("mics,cand,kwargs", [
    (MICS[:3], CAND, {}),                                               # three positions for four microphones
    (MICS.float(), CAND, {}), (MICS, CAND.float(), {}),
    (MICS[:, :2], CAND, {}), (MICS, CAND[:, :2], {}),
    (MICS[None].expand(3, 4, 3), CAND, {}), (MICS, CAND[None].expand(3, 9, 3), {}),      # three items for two
    (MICS, CAND[:0], {}), (MICS.numpy(), CAND, {}), (MICS, [[0.0, 0.0, 0.0]], {}),
    (MICS, CAND, {"fs": 0.0}), (MICS, CAND, {"fs": float("inf")}), (MICS, CAND, {"c": -340.0}), (MICS, CAND, {"c": None}),
    (MICS, CAND, {"n_fft": 402}), (MICS, CAND, {"band": (0, 300)}),
])
def test_srp_phat_argument_rules(mics, cand, kwargs):
    with pytest.raises(ValueError, match="^srp_phat: "):
        LOC.srp_phat(SPEC, mics, cand, **kwargs)


def test_cpu_tensors_are_refused_last():
    for spec in (SPEC, SPEC[0], SPEC.to(torch.complex64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            LOC.cross_spectra(spec)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            LOC.gcc_phat(spec, 4)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            LOC.tdoa(spec, 4)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            LOC.srp_phat(spec, MICS, CAND)
    with pytest.raises(ValueError, match="^srp_phat: band"):            # the ranges come first
        LOC.srp_phat(SPEC, MICS, CAND, band=(9, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LOC.locate_on_ring(SPEC, MICS, [2.5, 1.5, 1.5], [4, 5, 3], 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LOC.ring_candidates(72, [2.5, 1.5, 1.5], [4, 5, 3], 1, 1, device="cpu")
    with pytest.raises(ValueError, match="^ring_candidates: n_angles"):
        LOC.ring_candidates(0, [2.5, 1.5, 1.5], [4, 5, 3], 1, 1)
    with pytest.raises(ValueError, match="^locate_on_ring: "):
        LOC.locate_on_ring(np.zeros((4, 201, 6), complex), MICS, [2.5, 1.5, 1.5], [4, 5, 3], 1, 1)


def test_array_front_end_argument_rules():
    src = torch.zeros(2, 3, dtype=torch.float64)
    for bad_src, bad_mics in ((src.float(), MICS), (src[0], MICS), (src, MICS.float()), (src, MICS[:, :2]),
                              (src, MICS[None].expand(3, 4, 3)), (src, MICS[:0])):
        with pytest.raises(ValueError, match="^array_impulse_responses: "):
            FE.array_impulse_responses(bad_src, bad_mics, [4, 5, 3], reverberation_time=0.4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FE.array_impulse_responses(src, MICS, [4, 5, 3], reverberation_time=0.4)
    wave, h = torch.zeros(2, 800), torch.zeros(2, 4, 64, dtype=torch.float64)
    for bad_wave, bad_h in ((wave.double(), h), (wave[0], h), (wave, h.float()), (wave, h[0]), (wave, h[:1])):
        with pytest.raises(ValueError, match="^array_spectrograms: "):
            FE.array_spectrograms(bad_wave, bad_h)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FE.array_spectrograms(wave, h)
