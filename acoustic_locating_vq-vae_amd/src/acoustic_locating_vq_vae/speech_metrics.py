"""What a listener gets from a waveform or a spectrogram, measured on the device (csrc/speech_metrics.hip): short-time
objective intelligibility (STOI), scale-invariant SDR, the log-spectral distance of power spectrograms, and the rational
resampler STOI needs to get to 10 kHz.  Float64 arithmetic, fixed-order sums, no host sync.

    from acoustic_locating_vq_vae.front_end import waveform_from_reconstruction
    from acoustic_locating_vq_vae.speech_metrics import stoi, si_sdr, log_spectral_distance, resample_poly
    recon_wave = waveform_from_reconstruction(recon, raw_power, length=clean_wave.shape[1])   # Griffin-Lim: arbitrary phase
    stoi(clean_wave, recon_wave).value           # (B,) how intelligible the recovered speech is ...
    stoi(clean_wave, echoed_wave).value          # ... next to the echoed input the model started from (fs = 16000)
    si_sdr(clean_wave, echoed_wave)              # (B,) dB; for pairs that keep their phase
    log_spectral_distance(clean_power, recon_power)   # (B,) dB, straight on (B, F, T) power spectrograms
    wave_16k = resample_poly(wave_44k, 160, 441)      # scipy.signal.resample_poly's defaults, along the last axis

Definitions (in full: include/alvq.h).  ``resample_poly`` reduces up / down by their gcd and filters with
h[k] = sinc((k - half) / R) / R * kaiser(beta = 5)[k], R = max(up, down), half = 10 R, normalised to sum 1 and multiplied by up:
y[m] = sum_j x[j] h[m down - j up + half], ceil(n up / down) samples.  The filter is designed on the host with numpy and kept
on the device per (up, down): the first call with a ratio copies it there, so warm a ratio up before capturing a graph.

``stoi`` is the measure of Taal, Hendriks, Heusdens and Jensen (2011) at 10 kHz: frames of 256 samples at hop 128 under a Hann
window, frames of the clean signal more than 40 dB below its loudest dropped from both signals, 15 one-third-octave band
envelopes from 150 Hz out of a 512-point DFT, and the mean over bands and 30-frame segments of the correlation between the
clean envelope and the degraded one, scaled to the clean energy and clipped at -15 dB signal-to-distortion.  Other rates go
through ``resample_poly(., 10000, fs)`` first; pystoi and the MATLAB original resample with another filter, so at fs != 10000
values differ from theirs at about the third decimal (unmeasured here: neither is available).  ``status`` (int32 per row) is
0, or 1 = fewer than 256 samples at 10 kHz or a clean row of zero or non-finite energy (value NaN, kept_frames 0), or 2 =
fewer than 30 frames kept (value NaN).  Nothing here reads it: the caller does, when it can sync.  STOI compares frame
against frame, so the pair must be lined up: the dataset's 'same' convolution leaves the echoed signal (Nh - 1) // 2 samples
ahead of the clean one.
"""
import collections
import functools
import math

import numpy as np
import torch

from . import _native as N

STOI = collections.namedtuple("STOI", "value kept_frames status")

STOI_FS = 10000
STOI_NFFT = 512
STOI_BANDS = 15
STOI_MIN_FREQ = 150.0
MAX_RATE = 512


def resample_filter(up, down):
    """(h, up, down): the (2 half + 1) float64 taps of ``resample_poly`` as a numpy array, and up / down reduced by their
    gcd.  R = max(up, down) above 512 raises ValueError."""
    for name, v in (("up", up), ("down", down)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("resample_poly: %s must be a positive integer, got %r" % (name, v))
    g = math.gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    R = max(up, down)
    if R > MAX_RATE:
        raise ValueError("resample_poly: max(up, down) = %d after reduction, need <= %d" % (R, MAX_RATE))
    half = 10 * R
    k = np.arange(2 * half + 1, dtype=np.float64)
    h = np.sinc((k - half) / R) / R * np.kaiser(2 * half + 1, 5.0)
    return h / np.sum(h) * up, up, down


def stoi_band_edges():
    """(lo, hi): band j of STOI sums the 512-point DFT bins lo[j] <= k < hi[j] at 10 kHz, the bins nearest (the first on a
    tie) to 150 * 2^((2 j - 1) / 6) and 150 * 2^((2 j + 1) / 6) Hz."""
    f = np.arange(STOI_NFFT // 2 + 1, dtype=np.float64) * STOI_FS / STOI_NFFT
    centre = STOI_MIN_FREQ * 2.0 ** (np.arange(STOI_BANDS) / 3.0)
    lo = [int(np.argmin(np.abs(f - c * 2.0 ** (-1.0 / 6.0)))) for c in centre]
    hi = [int(np.argmin(np.abs(f - c * 2.0 ** (1.0 / 6.0)))) for c in centre]
    return lo, hi


@functools.lru_cache(maxsize=None)
def _device_filter(up, down, device):
    return torch.from_numpy(resample_filter(up, down)[0]).to(device)


def _rows(x, who, name, min_n=2):
    """x as a contiguous (B, n) tensor, and whether it came as (n,).  The device is checked by the caller, last."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("%s: %s must be an (n,) or (B, n) tensor" % (who, name))
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: %s must be float32 or float64, got %s" % (who, name, x.dtype))
    single = x.dim() == 1
    rows = x.unsqueeze(0) if single else x
    if rows.shape[0] < 1 or rows.shape[0] > 65535 or rows.shape[1] < min_n or rows.shape[1] > 1 << 24:
        raise ValueError("%s: need 1 <= B <= 65535 and %d <= n <= 2^24, got shape %s" % (who, min_n, tuple(x.shape)))
    return rows.contiguous(), single


def _pair(a, b, who, names, dims=(1, 2)):
    """Two tensors of one shape and dtype."""
    for t, name in zip((a, b), names):
        if not isinstance(t, torch.Tensor) or t.dim() not in dims:
            raise ValueError("%s: %s must be a tensor of %s dimensions" % (who, name, " or ".join(str(d) for d in dims)))
    if a.shape != b.shape:
        raise ValueError("%s: %s %s and %s %s differ in shape" % (who, names[0], tuple(a.shape), names[1], tuple(b.shape)))
    if a.dtype != b.dtype:
        raise ValueError("%s: %s is %s and %s is %s" % (who, names[0], a.dtype, names[1], b.dtype))


def _on_gpu(who, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("%s: the tensors must live on the GPU (got %s); the HIP path has no CPU fallback" % (who, t.device))


def resample_poly(x, up, down):
    """``scipy.signal.resample_poly(x, up, down)`` with its defaults along the last axis: x (B, n) or (n,), float32 or float64
    on the GPU -> float64 with ceil(n up / down) samples a row.  max(up, down) <= 512 after reduction by their gcd."""
    _, up, down = resample_filter(up, down)
    rows, single = _rows(x, "resample_poly", "x", min_n=1)
    _on_gpu("resample_poly", rows)
    y = N.resample_poly(rows, _device_filter(up, down, rows.device), up, down)
    return y[0] if single else y


def stoi(clean, degraded, fs=16000):
    """Short-time objective intelligibility of degraded against clean: (B, n) or (n,), float32 or float64 on the GPU, sampled
    at fs (a positive integer) -> ``STOI(value, kept_frames, status)`` of (B,) device tensors (0-d for (n,) input): float64,
    int32, int32.  1 for identical signals, falling with noise and reverberation."""
    if isinstance(fs, bool) or not isinstance(fs, (int, np.integer)) or fs < 1:
        raise ValueError("stoi: fs must be a positive integer, got %r" % (fs,))
    _pair(clean, degraded, "stoi", ("clean", "degraded"))
    if fs != STOI_FS:
        resample_filter(STOI_FS, fs)
    x, single = _rows(clean, "stoi", "clean")
    y, _ = _rows(degraded, "stoi", "degraded")
    _on_gpu("stoi", x, y)
    if fs != STOI_FS:
        x, y = resample_poly(x, STOI_FS, int(fs)), resample_poly(y, STOI_FS, int(fs))
    out = N.stoi(x.double(), y.double(), *stoi_band_edges())
    return STOI(*(t[0] for t in out)) if single else STOI(*out)


def si_sdr(reference, estimate):
    """Scale-invariant signal-to-distortion ratio of estimate against reference: (B, n) or (n,), float32 or float64 on the GPU
    -> (B,) float64 dB (0-d for (n,) input).  +inf for an exact multiple of the reference, NaN for a reference of zero or
    non-finite energy."""
    _pair(reference, estimate, "si_sdr", ("reference", "estimate"))
    s, single = _rows(reference, "si_sdr", "reference")
    e, _ = _rows(estimate, "si_sdr", "estimate")
    _on_gpu("si_sdr", s, e)
    out = N.si_sdr(s, e)
    return out[0] if single else out


def log_spectral_distance(p, q, eps=1e-10):
    """Log-spectral distance of power spectrograms p, q: (B, F, T) or (F, T), float32 or float64 on the GPU -> (B,) float64 dB
    (0-d for (F, T) input), the mean over the frames of sqrt(mean_f (10 log10((p + eps) / (q + eps)))^2).  A spectrogram pair
    with a negative or non-finite entry gives NaN."""
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (math.isfinite(eps) and eps >= 0):
        raise ValueError("log_spectral_distance: eps must be a finite number >= 0, got %r" % (eps,))
    _pair(p, q, "log_spectral_distance", ("p", "q"), dims=(2, 3))
    if p.dtype not in (torch.float32, torch.float64):
        raise ValueError("log_spectral_distance: p and q must be float32 or float64, got %s" % p.dtype)
    single = p.dim() == 2
    ps, qs = (p.unsqueeze(0), q.unsqueeze(0)) if single else (p, q)
    B, F, T = ps.shape
    if B < 1 or B > 65535 or F < 1 or T < 1 or F * T > 1 << 30:
        raise ValueError("log_spectral_distance: need 1 <= B <= 65535, F, T >= 1 and F T <= 2^30, got shape %s" % (tuple(p.shape),))
    _on_gpu("log_spectral_distance", ps, qs)
    out = N.lsd(ps.contiguous(), qs.contiguous(), float(eps))
    return out[0] if single else out
