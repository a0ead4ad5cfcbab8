"""CPU restatement of the inverse STFT and Griffin-Lim on torch.stft / torch.istft (test infrastructure, not product code).

PARITY UNPINNED, as for the forward STFT (oracle/stft_oracle.py): torchaudio and librosa are absent and the reference holds no
fixture, so this restates torchaudio's published semantics:
  InverseSpectrogram(n_fft, hop, center=True, pad=0, normalized=True)(spec)
      = torch.istft(spec * sqrt(sum w^2), n_fft, hop, window=w, center=True, normalized=False, onesided=True, length=length)
  functional.griffinlim(specgram, w, n_fft, hop, n_fft, power, n_iter, momentum, length, rand_init) on specgram * sqrt(sum w^2),
with w the periodic Hann window, so that a spectrogram normalised as oracle/stft_oracle.py::stft_complex gives a waveform at
the original scale.
"""
import torch


def _window(n_fft, dtype):
    return torch.hann_window(n_fft, periodic=True, dtype=dtype)


def istft(spec, n_fft=400, hop=160, length=None):
    """spec (..., n_fft/2+1, T) complex, normalised as stft_oracle.stft_complex -> (..., length) waveform."""
    real = torch.float64 if spec.dtype == torch.complex128 else torch.float32
    w = _window(n_fft, real)
    return torch.istft(spec * w.pow(2).sum().sqrt(), n_fft, hop_length=hop, win_length=n_fft, window=w, center=True,
                       normalized=False, onesided=True, length=length)


def griffin_lim(mag, angles, n_iter, momentum, n_fft=400, hop=160, length=None):
    """torchaudio.functional.griffinlim's loop on the magnitude mag (normalised as stft_complex) from the complex start
    phases angles (used as given)."""
    w = _window(n_fft, mag.dtype)
    spec = mag * w.pow(2).sum().sqrt()
    T = mag.shape[-1]
    length = hop * (T - 1) if length is None else length
    tprev = torch.zeros((), dtype=angles.dtype)
    for _ in range(n_iter):
        inverse = torch.istft(spec * angles, n_fft, hop_length=hop, win_length=n_fft, window=w, length=length)
        rebuilt = torch.stft(inverse, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect",
                             normalized=False, onesided=True, return_complex=True)
        a = rebuilt - tprev * (momentum / (1 + momentum))
        angles = a / (a.abs() + 1e-16)
        tprev = rebuilt
    return torch.istft(spec * angles, n_fft, hop_length=hop, win_length=n_fft, window=w, length=length)


def spectral_convergence(wave, mag, n_fft=400, hop=160):
    """|| |STFT(wave)| - mag || / || mag ||, the STFT normalised as stft_complex (the usual Griffin-Lim figure of merit)."""
    from oracle import stft_oracle
    got = stft_oracle.stft_complex(wave.to(torch.float64), n_fft, hop).abs()
    mag = mag.to(torch.float64)
    return float((got - mag).norm() / mag.norm())
