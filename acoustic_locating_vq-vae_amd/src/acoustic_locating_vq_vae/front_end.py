"""Waveform front end on the device.

The reference prepares its training samples offline (scripts/genereate_dataset.py:35-49): a torchaudio complex
spectrogram of the clean speech, the same of the speech convolved with a room impulse response, and from the two the
"RIR spectrogram", the Wiener estimate and three power spectrograms.  These functions do that arithmetic with the
HIP kernels of csrc/stft.hip, so the train loops can start from waveforms instead of from a pre-generated dataset:

    speech_spec, rir_spec, echoed_spec, wiener_est = specs_from_waveform(wave, h_rir)      # the sample 6-tuple's tensors
    x = speech_input_from_waveform(wave)                                                   # straight into Trainer.step

The way back, to listen to a spectrogram or to what a model makes of it (torchaudio InverseSpectrogram and
functional.griffinlim in the reference's notebooks; HIP kernels of csrc/istft.hip):

    wave = istft(spec, length=S)                                    # exact inverse of N.stft_complex (keeps the phase)
    wave = griffin_lim(power)                                       # power (or magnitude, power=1) -> waveform, 32 iterations
    wave = waveform_from_reconstruction(model(x)[1], raw_power)    # a speech model's standardised output -> waveform

The room impulse response itself comes from the ``rir_generator`` C++ package in the reference
(genereate_dataset.py:21-29), which is out of scope; any (Nh,) or (B, Nh) float64 response can be passed in.
"""
import torch

from . import _native as N
from .data_preprocessing import SPEC_FRAMES

N_FFT, HOP = 400, 160        # genereate_dataset.py:73-74 at fs = 16 kHz


def specs_from_waveform(wave, h_rir, n_fft=N_FFT, hop=HOP):
    """wave (B,S) float32 on the GPU, h_rir (Nh,) or (B,Nh) float64 ->
    (speech_spec (B,F,T) fp32, rir_spec fp64, echoed_spec fp64, wiener_est (B,F) fp64), all powers, with the
    reference's precisions: the clean branch is complex64, everything touched by the convolution is float64."""
    wave = wave.contiguous()
    echoed_wave = N.fir_same(wave, h_rir.contiguous())                      # :38  ss.convolve(..., mode='same')
    speech = N.stft_complex(wave, n_fft, hop)                               # :37
    echoed = N.stft_complex(echoed_wave, n_fft, hop)                        # :39
    speech_pow, echoed_pow, rir_pow, wiener = N.spec_rir_wiener(speech, echoed)   # :41-49
    return speech_pow, rir_pow, echoed_pow, wiener


def speech_input_from_waveform(wave, n_fft=N_FFT, hop=HOP, frames=SPEC_FRAMES):
    """wave (B,S) float32 -> the raw batch a speech train step takes: power spectrogram cropped to ``frames`` frames
    (the collate's crop, data_preprocessing.py:67-69); ``Trainer.step`` standardises it on the device."""
    power = N.stft_power(wave.contiguous(), n_fft, hop)
    if power.shape[2] < frames:
        raise ValueError("waveform gives %d frames, the collate needs %d" % (power.shape[2], frames))
    return power[:, :, :frames].contiguous()


def istft(spec, n_fft=N_FFT, hop=HOP, length=None):
    """The inverse of ``N.stft_complex``: spec (B, n_fft/2+1, T) complex64 / complex128 on the GPU -> (B, length) waveforms
    (torchaudio InverseSpectrogram(n_fft, hop, center=True, pad=0, normalized=True)).  length defaults to hop*(T-1); a longer
    one is zero-padded, as torch.istft does."""
    return N.istft(spec, n_fft, hop, length)


def griffin_lim(spec, power=2.0, n_iter=32, momentum=0.99, length=None, init=None, generator=None, n_fft=N_FFT, hop=HOP):
    """Waveforms (B, length) from a power spectrogram (power=2, what the dataset stores) or a magnitude (power=1), (B, F, T)
    float32 / float64 on the GPU and normalised as ``N.stft_complex``, by torchaudio.functional.griffinlim's iteration.
    init: complex start phases (B, F, T); by default torchaudio's rand_init, ``torch.rand`` of the complex dtype on the device
    (from ``generator`` if one is given).  length defaults to hop*(T-1)."""
    if spec.dim() != 3 or spec.dtype not in (torch.float32, torch.float64):
        raise ValueError("griffin_lim: expected a float32 / float64 (B, F, T) spectrogram, got %s %s" % (spec.dtype, tuple(spec.shape)))
    B, F, T = spec.shape
    if F != n_fft // 2 + 1:
        raise ValueError("griffin_lim: %d frequency bins, n_fft=%d has %d" % (F, n_fft, n_fft // 2 + 1))
    if not 0.0 <= momentum < 1.0:
        raise ValueError("griffin_lim: momentum must be in [0, 1), got %r" % (momentum,))
    if n_iter < 0:
        raise ValueError("griffin_lim: n_iter must be >= 0, got %r" % (n_iter,))
    if power <= 0:
        raise ValueError("griffin_lim: power must be > 0, got %r" % (power,))
    if not spec.is_cuda:
        raise RuntimeError("griffin_lim: spec must live on the GPU (got %s); the HIP path has no CPU fallback" % spec.device)
    cdtype = torch.complex128 if spec.dtype == torch.float64 else torch.complex64
    length = hop * (T - 1) if length is None else int(length)
    mag = (spec if power == 1.0 else spec.pow(1.0 / power)).contiguous()
    if init is None:
        init = torch.rand(spec.shape, dtype=cdtype, device=spec.device, generator=generator)
    elif init.shape != spec.shape or init.dtype != cdtype:
        raise ValueError("griffin_lim: init must be %s of shape %s" % (cdtype, tuple(spec.shape)))
    return N.griffin_lim(mag, init.contiguous(), n_iter, momentum, n_fft, hop, length)


def waveform_from_reconstruction(recon, raw_power, **gl_kwargs):
    """What a speech model sounds like: its standardised output recon (B, F, T') -> (B, length) waveforms.

    The speech loop trains on x = (|raw| - mean) / (std + 1e-8) over the frequency axis of each frame (train_speech.py; the
    Trainer's ``N.standardise(raw, take_abs=True)``, unbiased std).  This undoes that with raw_power's own per-frame statistics,
    crops a longer decoder output to raw_power's T frames (as train_speech.py / train_echoed_speech.py do), clamps the power
    at 0 and runs ``griffin_lim`` on it (gl_kwargs: its keyword arguments)."""
    raw = raw_power.abs()
    T = raw.shape[2]
    if recon.dim() != 3 or recon.shape[:2] != raw.shape[:2] or recon.shape[2] < T:
        raise ValueError("waveform_from_reconstruction: recon %s does not cover raw_power %s" % (tuple(recon.shape), tuple(raw.shape)))
    mean = raw.mean(dim=1, keepdim=True)
    std = raw.std(dim=1, keepdim=True)
    power = (recon.detach()[:, :, :T].to(raw.dtype) * (std + 1e-8) + mean).clamp_min(0.0)
    return griffin_lim(power.contiguous(), power=2.0, **gl_kwargs)
