"""CPU checks of the front-end test references and of the front-end C entry points' argument checks (no GPU).

tests/helpers/dsp_ref.py restates the STFT, inverse STFT, FIR and spectrogram arithmetic of csrc/stft.hip and csrc/istft.hip
directly; here it is pinned to independent implementations (torch.stft / torch.istft through oracle/stft_oracle.py and
tests/helpers/griffin_lim_ref.py, scipy.signal.convolve, oracle/front_end_oracle.py) on the grids tests/test_dsp_edges_gpu.py
holds the kernels to.  The argument tests pass a non-null fake pointer: every call must fail its host checks before any launch.
"""
import os
import sys

import numpy as np
import pytest
import scipy.signal as ss
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import dsp_ref as R  # noqa: E402
import griffin_lim_ref as GL  # noqa: E402
from oracle import front_end_oracle, stft_oracle  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 0x1000           # a non-null pointer: every call below must fail its host checks before touching it
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def native():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native
    return _native


# ------------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("n_fft,hop,lengths", R.stft_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_stft_matches_torch_stft(n_fft, hop, lengths):
    for S in lengths:
        x = R.stft_signal(2, S, S).astype(np.float64)
        frames = R.check_frames(1 + S // hop, S)
        X, l1, l1x = R.stft(x, n_fft, hop, frames)
        want = stft_oracle.stft_complex(torch.from_numpy(x), n_fft, hop).numpy()[..., frames]
        assert X.shape == want.shape
        # torch.stft's own rounding is not confined to the frame: hold it to the frame's l1 plus the item's loudest frame
        l1 = l1.astype(np.float64)
        scale = l1 + l1.max(axis=-1, keepdims=True)
        assert (np.abs(X.astype(np.complex128) - want) <= 8 * EPS * scale[:, None, :]).all(), S
        assert (l1 <= l1x).all()


@pytest.mark.parametrize("n_fft,hop,S", [(4, 1, 3), (6, 7, 5), (62, 3, 40), (400, 160, 1601), (2048, 2055, 1025),
                                         (1024, 1, 600)])
def test_impulse_closed_form_matches_stft(n_fft, hop, S):
    for p in R.impulse_positions(S, n_fft):
        x = np.zeros(S)
        x[p] = 1.0
        X, l1, l1x = R.stft(x, n_fft, hop)
        Y, m1, m1x = R.stft_of_impulse(p, S, n_fft, hop)
        assert np.abs(X - Y).max() <= 1e-17 and np.abs(l1 - m1).max() <= 1e-17 and np.abs(l1x - m1x).max() <= 1e-17, p
        assert (Y[0].imag == 0).all() and (np.abs(Y[-1].imag) <= 1e-18).all()
    with pytest.raises(ValueError):
        R.stft_of_impulse(S, S, n_fft, hop)


@pytest.mark.parametrize("n_fft", R.ISTFT_NFFT)
def test_istft_matches_torch_istft(n_fft):
    checked = 0
    for hop in R.istft_hops(n_fft):
        for T in R.ISTFT_T:
            for length in R.istft_lengths(n_fft, hop, T):
                if not R.istft_env_ok(n_fft, hop, T, length, 1e-6):
                    continue
                rng = np.random.default_rng(n_fft + hop + T + length)
                spec = rng.standard_normal((2, n_fft // 2 + 1, T)) + 1j * rng.standard_normal((2, n_fft // 2 + 1, T))
                y, A, _, _, env = R.istft(spec, n_fft, hop, length)
                want = GL.istft(torch.from_numpy(spec), n_fft, hop, length).numpy()
                assert y.shape == want.shape == (2, length)
                assert (np.abs(y.astype(np.float64) - want) <= 1e-12 * (A.astype(np.float64) + 1e-300)).all(), (hop, T, length)
                checked += 1
    assert checked > 0


def test_istft_ignores_dc_and_nyquist_imaginary_parts():
    rng = np.random.default_rng(4)
    spec = rng.standard_normal((1, 33, 5)) + 1j * rng.standard_normal((1, 33, 5))
    s2 = spec.copy()
    s2[:, 0] = s2[:, 0].real + 5j
    s2[:, -1] = s2[:, -1].real - 2j
    assert np.array_equal(R.istft(spec, 64, 16, 80)[0], R.istft(s2, 64, 16, 80)[0])


@pytest.mark.parametrize("S,Nh", R.FIR_CASES)
def test_fir_same_matches_scipy_direct(S, Nh):
    rng = np.random.default_rng(S + 7 * Nh)
    wave = rng.standard_normal((2, S)).astype(np.float32)
    h = rng.standard_normal((2, Nh))
    out, mag = R.fir_same(wave, h)
    for b in range(2):
        want = ss.convolve(wave[b].astype(np.float64), h[b], mode="same", method="direct")
        assert (np.abs(out[b].astype(np.float64) - want) <= (Nh + 1) * EPS * mag[b].astype(np.float64)).all()
    shared, _ = R.fir_same(wave, h[0])
    assert np.array_equal(shared[0], R.fir_same(wave[:1], h[:1])[0][0])


@pytest.mark.parametrize("F,T", R.RIR_CASES)
def test_spec_rir_wiener_matches_front_end_oracle(F, T):
    """The oracle follows the dataset generator on one item (max |r| over that item): on a batch the helper must equal it
    item by item, and the items' scales must not mix."""
    rng = np.random.default_rng(F + T)
    B = 3
    Sc = (rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T))).astype(np.complex64)
    Sc *= np.array([1.0, 1e-6, 1e6], dtype=np.float32)[:, None, None]
    Ec = rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T))
    speech, echoed, rir, wiener, wscale = (a.astype(np.float64) for a in R.spec_rir_wiener(Sc, Ec))
    assert np.allclose(rir.max(axis=(1, 2)), 1.0, rtol=1e-15)
    assert (np.abs(wiener) <= wscale * (1 + 1e-12)).all()
    for b in range(B):
        s_t, e_t = torch.from_numpy(Sc[b]), torch.from_numpy(Ec[b])
        # oracle's arithmetic, on given spectra (convert_speech_to_specs's lines :41-49)
        rir_spec = s_t.to(torch.complex128) / (e_t + 1e-8)
        rir_spec = rir_spec / rir_spec.abs().max()
        w = torch.sum(e_t * torch.conj(s_t), dim=1) / (torch.sum(s_t * torch.conj(s_t), dim=1) + 1e-8)
        assert np.allclose(speech[b], s_t.abs().pow(2).numpy(), rtol=1e-6, atol=0)
        assert np.allclose(echoed[b], e_t.abs().pow(2).numpy(), rtol=1e-14, atol=0)
        assert np.abs(rir[b] - rir_spec.abs().pow(2).numpy()).max() <= 1e-14
        assert (np.abs(wiener[b] - w.abs().pow(2).numpy()) <= 1e-6 * wscale[b]).all()


def test_spec_rir_wiener_matches_front_end_oracle_on_waveforms():
    """End to end through the oracle's own STFT on one waveform pair (F = 201)."""
    rng = np.random.default_rng(9)
    wave = torch.from_numpy(rng.standard_normal((1, 3200)).astype(np.float32))
    h = rng.standard_normal(64) * np.exp(-np.arange(64) / 8.0)
    want = front_end_oracle.convert_speech_to_specs(wave, h)
    sspec = stft_oracle.stft_complex(wave).numpy()
    echoed_wave, _ = R.fir_same(wave.numpy(), h)
    espec = stft_oracle.stft_complex(torch.from_numpy(echoed_wave.astype(np.float64))).numpy()
    speech, echoed, rir, wiener, _ = R.spec_rir_wiener(sspec, espec)
    for got, w in zip((speech, rir, echoed, wiener), want):
        w = w.numpy()
        assert np.abs(got[0].astype(np.float64) - w).max() <= 1e-6 * np.abs(w).max()


# --------------------------------------------------------------------------------------------------- argument checks
def _stft(lib, name, wave=FAKE, out=FAKE, B=1, S=1600, n_fft=400, hop=160):
    return getattr(lib, name)(wave, out, B, S, n_fft, hop, None)


@pytest.mark.parametrize("name", ["alvq_stft_power_f32", "alvq_stft_complex_f32", "alvq_stft_power_f64", "alvq_stft_complex_f64"])
def test_stft_argument_errors_do_not_launch(native, name):
    lib = native.lib()
    limit = 2048 if name.endswith("f32") else 1024
    cases = [
        (dict(wave=None), EINVAL, b"null"),
        (dict(out=None), EINVAL, b"null"),
        (dict(n_fft=401), EINVAL, b"bad dims"),
        (dict(n_fft=3), EINVAL, b"bad dims"),
        (dict(n_fft=2), EINVAL, b"bad dims"),
        (dict(n_fft=0), EINVAL, b"bad dims"),
        (dict(B=0), EINVAL, b"bad dims"),
        (dict(B=-1), EINVAL, b"bad dims"),
        (dict(hop=0), EINVAL, b"bad dims"),
        (dict(hop=-160), EINVAL, b"bad dims"),
        (dict(S=200), EINVAL, b"reflect"),                            # S = n_fft/2
        (dict(S=0), EINVAL, b"reflect"),
        (dict(S=-5), EINVAL, b"reflect"),
        (dict(n_fft=limit + 2, S=4 * limit), EUNSUPPORTED, b"too large"),
        (dict(n_fft=2 * limit, S=4 * limit), EUNSUPPORTED, b"too large"),
    ]
    for kw, code, msg in cases:
        assert _stft(lib, name, **kw) == code, kw
        assert msg in lib.alvq_last_error(), (kw, lib.alvq_last_error())


def _fir(lib, wave=FAKE, h=FAKE, out=FAKE, B=2, S=1000, Nh=64, stride=0):
    return lib.alvq_fir_same_f64(wave, h, out, B, S, Nh, stride, None)


def test_fir_same_argument_errors_do_not_launch(native):
    lib = native.lib()
    cases = [
        (dict(wave=None), b"null"), (dict(h=None), b"null"), (dict(out=None), b"null"),
        (dict(Nh=1001), b"bad dims"),                                  # Nh > S
        (dict(Nh=0), b"bad dims"), (dict(Nh=-3), b"bad dims"),
        (dict(B=0), b"bad dims"), (dict(B=-2), b"bad dims"),
        (dict(S=0, Nh=1), b"bad dims"), (dict(S=-1, Nh=1), b"bad dims"),
        (dict(stride=63), b"h_batch_stride"), (dict(stride=1), b"h_batch_stride"), (dict(stride=-1), b"h_batch_stride"),
    ]
    for kw, msg in cases:
        assert _fir(lib, **kw) == EINVAL, kw
        assert msg in lib.alvq_last_error(), (kw, lib.alvq_last_error())


def test_spec_rir_wiener_argument_errors_do_not_launch(native):
    lib = native.lib()
    for i in range(7):
        ptrs = [FAKE] * 7
        ptrs[i] = None
        assert lib.alvq_spec_rir_wiener_f64(*ptrs, 1, 201, 11, None) == EINVAL, i
        assert b"null" in lib.alvq_last_error()
    for B, F, T in [(0, 201, 11), (-1, 201, 11), (1, 0, 11), (1, -201, 11), (1, 201, 0), (1, 201, -11)]:
        assert lib.alvq_spec_rir_wiener_f64(*([FAKE] * 7), B, F, T, None) == EINVAL, (B, F, T)
        assert b"bad dims" in lib.alvq_last_error()
