"""The baseline a dereverberating model is measured against, on the device (csrc/wpe.hip): weighted prediction error (WPE,
Nakatani, Yoshioka, Kinoshita, Miyoshi and Juang 2010), the standard blind dereverberator, on complex spectrograms.  It keeps
the phase, so ``istft``, ``si_sdr`` and ``stoi`` apply to its output directly.  Float64 arithmetic, fixed-order sums, one
launch, no host sync.

    from acoustic_locating_vq_vae.dereverberation import dereverberate, wpe
    from acoustic_locating_vq_vae.front_end import waveform_from_reconstruction
    from acoustic_locating_vq_vae.speech_metrics import stoi, si_sdr
    stoi(clean_wave, echoed_wave).value                  # (B,) what the room did to the speech (fs = 16000) ...
    stoi(clean_wave, dereverberate(echoed_wave)).value   # ... what WPE recovers from the echoed waveform alone ...
    stoi(clean_wave, waveform_from_reconstruction(recon, raw_power, length=clean_wave.shape[1])).value   # ... and the model
    si_sdr(clean_wave, dereverberate(echoed_wave))       # (B,) dB; WPE keeps the phase, so SI-SDR applies too
    wpe(N.stft_complex(echoed_wave)).spec                # the dereverberated (B, F, T) spectrogram itself

STOI and SI-SDR compare sample against sample, so the pair must be lined up: the dataset's 'same' convolution leaves the echoed
signal (Nh - 1) // 2 samples ahead of the clean one, and WPE does not move it.

Definitions (in full: include/alvq.h).  Every (item, frequency bin) is a problem of its own over the T frames of its D
microphones.  The stacked past x~_t has M = D taps entries, entry k D + d = x_d[t - delay - k] (0 before the first frame).
Starting from y = x, ``iterations`` times: p_t = the mean of |y_d[u]|^2 over the microphones and the frames u within
psd_context of t that exist; lambda_t = max(p_t, eps max_t p_t); R = sum_t x~_t x~_t^H / lambda_t and
P = sum_t x~_t x_t^H / lambda_t; R gets loading tr(R) / M on its diagonal; G = R^-1 P by Cholesky; y_t = x_t - G^H x~_t.
The delay keeps the filter from predicting the speech itself (its correlation reaches over a frame or two), so what it
predicts, and removes, is the late reverberation.  ``status`` (int32 per item and bin) is 0, or 1 = a non-finite value or no
power at all in the bin, or 2 = a Cholesky pivot <= 0 or not finite (always where T <= delay); such a bin comes back unchanged.
Nothing here reads it: the caller does, when it can sync.
"""
import collections

import torch

from . import _native as N
from . import _rules as rules
from ._rules import MAX_FRAMES, MAX_MICROPHONES  # noqa: F401 -- public here
from .front_end import HOP, N_FFT

WPE = collections.namedtuple("WPE", "spec status")

MAX_FILTER = 64          # D taps
MAX_DELAY = 64
MAX_ITERATIONS = 16
MAX_PSD_CONTEXT = 64


def wpe(spec, taps=10, delay=3, iterations=3, psd_context=0, eps=1e-10, loading=1e-10):
    """WPE dereverberation of a complex spectrogram: spec (F, T), (B, F, T) (what ``N.stft_complex`` returns: one microphone)
    or (B, D, F, T), complex64 or complex128 on the GPU -> ``WPE(spec, status)``: the dereverberated spectrogram of the same
    shape and dtype and the int32 status of every bin, (F,), (B, F) or (B, F).  D <= 8, D taps <= 64, T <= 65535."""
    if not isinstance(spec, torch.Tensor) or spec.dim() not in (2, 3, 4):
        raise ValueError("wpe: spec must be an (F, T), (B, F, T) or (B, D, F, T) tensor")
    if spec.dtype not in (torch.complex64, torch.complex128):
        raise ValueError("wpe: spec must be complex64 or complex128, got %s" % spec.dtype)
    rules.int_in("wpe", "taps", taps, 1, MAX_FILTER)
    rules.int_in("wpe", "delay", delay, 0, MAX_DELAY)
    rules.int_in("wpe", "iterations", iterations, 1, MAX_ITERATIONS)
    rules.int_in("wpe", "psd_context", psd_context, 0, MAX_PSD_CONTEXT)
    rules.nonneg("wpe", "eps", eps)
    rules.nonneg("wpe", "loading", loading)
    x = {2: spec[None, None], 3: spec[:, None], 4: spec}[spec.dim()]
    rules.frames("wpe", x.shape, spec.shape)
    D = x.shape[1]
    if D < 1 or D > MAX_MICROPHONES or D * taps > MAX_FILTER:
        raise ValueError("wpe: need 1 <= D <= 8 microphones and D taps <= 64, got D = %d, taps = %d" % (D, taps))
    rules.on_gpu("wpe", x, "spec")
    out, status = N.wpe(x, taps, delay, iterations, psd_context, float(eps), float(loading))
    if spec.dim() == 2:
        return WPE(out[0, 0], status[0])
    return WPE(out[:, 0] if spec.dim() == 3 else out, status)


def dereverberate(wave, n_fft=N_FFT, hop=HOP, **wpe_kwargs):
    """Waveforms with the late reverberation taken off: wave (B, S) or (S,), float32 or float64 on the GPU -> the same shape
    and dtype, ``istft(wpe(N.stft_complex(wave)).spec, length=S)`` with ``wpe``'s keywords."""
    if not isinstance(wave, torch.Tensor) or wave.dim() not in (1, 2):
        raise ValueError("dereverberate: wave must be an (S,) or (B, S) tensor")
    if wave.dtype not in (torch.float32, torch.float64):
        raise ValueError("dereverberate: wave must be float32 or float64, got %s" % wave.dtype)
    rules.on_gpu("dereverberate", wave, "wave")
    rows = (wave[None] if wave.dim() == 1 else wave).contiguous()
    out = N.istft(wpe(N.stft_complex(rows, n_fft, hop), **wpe_kwargs).spec, n_fft, hop, rows.shape[1])
    return out[0] if wave.dim() == 1 else out
