"""Inverse STFT and Griffin-Lim on the device (csrc/istft.hip, front_end.istft / griffin_lim / waveform_from_reconstruction).

Parity is unpinned, as for the forward STFT: torchaudio and librosa are absent, so the reference is the float64 restatement on
torch.stft / torch.istft in tests/helpers/griffin_lim_ref.py (pinned itself by tests/test_griffin_lim_cpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from oracle import stft_oracle  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import griffin_lim_ref as GL  # noqa: E402


def rel_max(a, b):
    a, b = a.detach().cpu().to(torch.float64), b.detach().cpu().to(torch.float64)
    return float((a - b).abs().max() / b.abs().max())


def rel_l2(a, b):
    a, b = a.detach().cpu().to(torch.float64), b.detach().cpu().to(torch.float64)
    return float((a - b).norm() / b.norm())


def chirp(S, seed):
    """A chirp plus white noise (the test_front_end_gpu.py waveform)."""
    t = torch.arange(S, dtype=torch.float64) / 16000.0
    g = torch.Generator().manual_seed(seed)
    return torch.sin(2 * np.pi * (200.0 + 900.0 * t) * t) * (0.3 + 0.7 * torch.rand(1, generator=g, dtype=torch.float64)) + \
        0.05 * torch.randn(S, generator=g, dtype=torch.float64)


def batch(B, S, dtype, seed=0):
    return torch.stack([chirp(S, seed + b) for b in range(B)]).to(dtype)


def rand_phases(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, dtype=dtype, generator=g)


TOL_RT = {torch.float64: 1e-12, torch.float32: 1e-5}


# ------------------------------------------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("B,S,length", [(1, 16000, None), (3, 16000, None), (1, 80000, None), (3, 80000, None), (2, 16037, 16037)])
def test_round_trip(dtype, B, S, length):
    x = batch(B, S, dtype, seed=S + B)
    spec = N.stft_complex(x.cuda())
    y = FE.istft(spec, length=length)
    n = length or 160 * (spec.shape[2] - 1)
    assert y.shape == (B, n) and y.dtype == dtype
    assert rel_max(y, x[:, :n]) <= TOL_RT[dtype]


def test_round_trip_librosa_framing():
    """n_fft 2048, hop 512: librosa's default framing, which the reference's sout_test.py uses.  float32 only: 2048 is the f32
    limit of both transforms (the f64 one is 1024, as for alvq_stft_complex_f64)."""
    x = batch(2, 22050, torch.float32, seed=3)
    spec = N.stft_complex(x.cuda(), 2048, 512)
    y = FE.istft(spec, n_fft=2048, hop=512, length=22050)
    assert rel_max(y, x) <= TOL_RT[torch.float32]
    with pytest.raises(RuntimeError, match="too large"):
        FE.istft(spec.to(torch.complex128), n_fft=2048, hop=512)


# ------------------------------------------------------------------------------------------------- 2. arbitrary spectra
@pytest.mark.parametrize("dtype,tol", [(torch.complex128, 1e-12), (torch.complex64, 2e-5)])
@pytest.mark.parametrize("n_fft,hop,T,length", [(400, 160, 37, None), (400, 100, 20, 2500), (64, 16, 9, 100)])
def test_istft_matches_restatement_on_arbitrary_spectra(dtype, tol, n_fft, hop, T, length):
    """Not consistent STFTs, with non-zero imaginary parts at DC and Nyquist (which the inverse ignores, as irfft)."""
    g = torch.Generator().manual_seed(n_fft + T)
    spec = torch.randn((2, n_fft // 2 + 1, T), dtype=torch.complex128, generator=g)
    assert float(spec[:, 0].imag.abs().min()) > 0 and float(spec[:, -1].imag.abs().max()) > 0.1
    got = FE.istft(spec.to(dtype).cuda(), n_fft=n_fft, hop=hop, length=length)
    want = GL.istft(spec, n_fft, hop, length)
    assert got.shape == want.shape
    if length is not None and length > hop * (T - 1):                    # zero-padded past the overlap-added signal
        assert float(got[:, hop * (T - 1) + n_fft // 2:].abs().max()) == 0.0
    assert rel_max(got, want) <= tol


# ------------------------------------------------------------------------------------------------- 3./4. Griffin-Lim
def _gl_problem(dtype, B=2, S=16000, seed=11):
    x = batch(B, S, torch.float64, seed=seed)
    mag = stft_oracle.stft_complex(x).abs()
    init = rand_phases(mag.shape, torch.complex128, seed)
    return mag, init


@pytest.mark.parametrize("n_iter", [0, 1, 4, 32])
@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_griffin_lim_f64_matches_restatement(n_iter, momentum):
    mag, init = _gl_problem(torch.float64)
    got = FE.griffin_lim(mag.cuda(), power=1.0, n_iter=n_iter, momentum=momentum, init=init.cuda())
    want = GL.griffin_lim(mag, init, n_iter, momentum)
    assert got.shape == want.shape == (2, 16000)
    assert rel_l2(got, want) <= 1e-9, rel_l2(got, want)


def test_griffin_lim_f32_against_f64_restatement():
    mag, init = _gl_problem(torch.float32)
    got = FE.griffin_lim(mag.float().cuda(), power=1.0, n_iter=4, momentum=0.99, init=init.to(torch.complex64).cuda())
    want = GL.griffin_lim(mag, init, 4, 0.99)
    assert got.dtype == torch.float32 and rel_l2(got, want) <= 1e-4, rel_l2(got, want)


def test_griffin_lim_f32_converges_like_f64():
    mag, init = _gl_problem(torch.float32)
    got = FE.griffin_lim(mag.float().cuda(), power=1.0, n_iter=32, momentum=0.99, init=init.to(torch.complex64).cuda())
    sc = GL.spectral_convergence(got.cpu(), mag)
    sc_ref = GL.spectral_convergence(GL.griffin_lim(mag, init, 32, 0.99), mag)
    sc0 = GL.spectral_convergence(GL.griffin_lim(mag, init, 0, 0.99), mag)
    # measured on an MI355X: f32 0.071245, f64 restatement 0.071245, n_iter = 0: 0.759989
    print("spectral convergence: f32 %.6f, f64 restatement %.6f, n_iter=0 %.6f" % (sc, sc_ref, sc0))
    assert sc <= 1.05 * sc_ref and sc < sc0


def test_griffin_lim_power_input_and_default_init():
    """power=2 (what the dataset stores) is the magnitude squared; the default init is torch.rand of the complex dtype."""
    mag, init = _gl_problem(torch.float32)
    mag = mag.float().cuda()
    a = FE.griffin_lim(mag, power=1.0, n_iter=2, init=init.to(torch.complex64).cuda())
    b = FE.griffin_lim(mag * mag, n_iter=2, init=init.to(torch.complex64).cuda())
    assert rel_l2(b, a) < 1e-5
    g1, g2 = torch.Generator(device="cuda").manual_seed(5), torch.Generator(device="cuda").manual_seed(5)
    c = FE.griffin_lim(mag, power=1.0, n_iter=2, generator=g1)
    ref_init = torch.rand(mag.shape, dtype=torch.complex64, device="cuda", generator=g2)
    d = FE.griffin_lim(mag, power=1.0, n_iter=2, init=ref_init)
    assert torch.equal(c, d) and torch.isfinite(c).all()


# ------------------------------------------------------------------------------------------------- 5. determinism, capture
def test_deterministic_and_graph_capturable():
    mag, init = _gl_problem(torch.float32, B=3)
    mag, init = (mag * mag).float().cuda(), init.to(torch.complex64).cuda()
    e1 = FE.griffin_lim(mag, n_iter=8, init=init)
    e2 = FE.griffin_lim(mag, n_iter=8, init=init)
    assert torch.equal(e1, e2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = FE.griffin_lim(mag, n_iter=8, init=init)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, e1)


# ------------------------------------------------------------------------------------------------- 6. model output -> waveform
def test_waveform_from_reconstruction_undoes_the_standardisation():
    x = batch(2, 16000, torch.float32, seed=21).cuda()
    raw = N.stft_power(x)
    init = rand_phases(raw.shape, torch.complex64, 21).cuda()
    # One iteration: the standardised spectrogram is rounded to float32, and un-standardising it leaves ~eps * mean of absolute
    # error on every bin, which the square root turns into a relative 7e-7 (L2) of the magnitude.  The first inverse carries
    # that through (a float64 restatement of this same round trip on the host: 9.6e-7 of the waveform at n_iter 0 and 1); the
    # momentum-0.99 iteration then amplifies any input perturbation (same restatement: 1.3e-5 at n_iter 4, 8.1e-5 measured
    # here on an MI355X), so n_iter 4 would test Griffin-Lim's conditioning, not this helper.
    want = FE.griffin_lim(raw, n_iter=1, init=init)
    got = FE.waveform_from_reconstruction(N.standardise(raw, take_abs=True), raw, n_iter=1, init=init)
    assert rel_l2(got, want) <= 1e-5, rel_l2(got, want)
    # a decoder output longer than the input is cropped to raw's frames
    longer = torch.cat([N.standardise(raw, take_abs=True), torch.zeros_like(raw[:, :, :3])], dim=2)
    assert torch.equal(FE.waveform_from_reconstruction(longer, raw, n_iter=1, init=init), got)


def test_waveform_from_model_output():
    from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE
    torch.manual_seed(0)
    model = ConvolutionalVQVAE(201, 32, 8, 1, 16, 0.25, 32).cuda().eval()
    raw = N.stft_power(batch(2, 8000, torch.float32, seed=31).cuda())
    with torch.no_grad():
        recon = model(N.standardise(raw, take_abs=True))[1]
    wave = FE.waveform_from_reconstruction(recon, raw, n_iter=4)
    assert wave.shape == (2, 160 * (raw.shape[2] - 1)) and torch.isfinite(wave).all()


# ------------------------------------------------------------------------------------------------- 7. errors
def test_errors():
    with pytest.raises(RuntimeError, match="GPU"):
        FE.griffin_lim(torch.ones(1, 201, 11))
    with pytest.raises(RuntimeError, match="GPU"):
        FE.istft(torch.ones(1, 201, 11, dtype=torch.complex64))
    with pytest.raises(ValueError, match="frequency bins"):
        FE.griffin_lim(torch.ones(1, 201, 11, device="cuda"), n_fft=512)
    with pytest.raises(RuntimeError, match="frequency bins"):
        FE.istft(torch.ones(1, 201, 11, dtype=torch.complex64, device="cuda"), n_fft=512)
    with pytest.raises(ValueError, match="momentum"):
        FE.griffin_lim(torch.ones(1, 201, 11, device="cuda"), momentum=1.0)
    with pytest.raises(RuntimeError, match="NOLA"):
        FE.istft(torch.ones(1, 201, 11, dtype=torch.complex64, device="cuda"), hop=500)
