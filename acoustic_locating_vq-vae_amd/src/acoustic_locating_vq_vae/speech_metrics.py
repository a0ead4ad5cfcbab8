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

Separated sources come back in an order nobody chose (``separation.auxiva``, ``ilrma``, ``cacgmm``); the scores that say which
output is which talker, and what is left in it, are here too (csrc/separation_metrics.hip), with the same guarantees and
graph-capturable:

    from acoustic_locating_vq_vae.speech_metrics import pairwise_si_sdr, assign, pit_si_sdr, si_bss_eval, si_sdr_improvement
    pairwise_si_sdr(clean, waves)                # (B, K, J) dB: every estimate against every reference, si_sdr's bits
    pit = pit_si_sdr(clean, waves)               # PIT(value (B, K), perm (B, K), status (B,)): the permutation-invariant SI-SDR
    separation.reorder(sep.spec, pit.perm)       # the separated spectrograms in the talkers' order
    si_bss_eval(clean, waves)                    # SIBSS(sdr, sir, sar, perm, status): crosstalk (sir) or artefacts (sar)?
    si_sdr_improvement(clean, waves, mixture)    # (B, K) dB gained over the mixture
    assign(table, maximize=False)                # ASSIGN(perm, total, status) of any (B, K, J) cost table, K <= J <= 8

``pairwise_si_sdr``'s entry [b, i, j] is ``si_sdr(references[b, i], estimates[b, j])`` bit for bit.  ``assign`` searches all
injections pi of the K rows into the J columns in lexicographic order of (pi(0), ..., pi(K-1)); the score of pi is
table[0, pi(0)] + table[1, pi(1)] + ..., k rising; a NaN score is skipped, ties go to the first injection; status 1 where
every score is NaN (perm the identity, total NaN).  ``si_bss_eval`` is the scale-invariant split of Le Roux, Wisdom, Erdogan and
Hershey ("SDR -- half-baked or well done?", 2019): with s_p the item's centred references, e the centred estimate
perm[b, i] selects, G = [<s_p, s_q>] and g = [<s_p, e>]: target = (g[i] / G[i, i]) s_i, proj = sum_p c_p s_p with G c = g
(Gaussian elimination, partial pivoting), interf = proj - target, artif = e - proj; sdr = |target|^2 / |target - e|^2, sir =
|target|^2 / |interf|^2, sar = |proj|^2 / |artif|^2 in dB, the energies summed sample by sample, +inf where a denominator is
0.  Its status per item: 0; 1 = a reference of zero or non-finite centred energy or a non-finite sample in a selected estimate
(sir, sar NaN); 2 = a pivot that is 0 or not finite, as two identical references give (sir, sar NaN); 3 = a perm row that is
not an injection into 0..J-1 (all NaN; found on the device).  In full: include/alvq.h.
"""
import collections
import functools
import math

import numpy as np
import torch

from . import _native as N
from . import _rules as rules

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
    rows, single = rules.rows("resample_poly", "x", x, 1, rules.MAX_BATCH)
    _on_gpu("resample_poly", rows)
    return rules.unbatch(N.resample_poly(rows, _device_filter(up, down, rows.device), up, down), not single)


def stoi(clean, degraded, fs=16000):
    """Short-time objective intelligibility of degraded against clean: (B, n) or (n,), float32 or float64 on the GPU, sampled
    at fs (a positive integer) -> ``STOI(value, kept_frames, status)`` of (B,) device tensors (0-d for (n,) input): float64,
    int32, int32.  1 for identical signals, falling with noise and reverberation."""
    if isinstance(fs, bool) or not isinstance(fs, (int, np.integer)) or fs < 1:
        raise ValueError("stoi: fs must be a positive integer, got %r" % (fs,))
    _pair(clean, degraded, "stoi", ("clean", "degraded"))
    if fs != STOI_FS:
        resample_filter(STOI_FS, fs)
    x, single = rules.rows("stoi", "clean", clean, max_b=rules.MAX_BATCH)
    y, _ = rules.rows("stoi", "degraded", degraded, max_b=rules.MAX_BATCH)
    _on_gpu("stoi", x, y)
    if fs != STOI_FS:
        x, y = resample_poly(x, STOI_FS, int(fs)), resample_poly(y, STOI_FS, int(fs))
    return rules.unbatch(STOI(*N.stoi(x.double(), y.double(), *stoi_band_edges())), not single)


def si_sdr(reference, estimate):
    """Scale-invariant signal-to-distortion ratio of estimate against reference: (B, n) or (n,), float32 or float64 on the GPU
    -> (B,) float64 dB (0-d for (n,) input).  +inf for an exact multiple of the reference, NaN for a reference of zero or
    non-finite energy."""
    _pair(reference, estimate, "si_sdr", ("reference", "estimate"))
    s, single = rules.rows("si_sdr", "reference", reference, max_b=rules.MAX_BATCH)
    e, _ = rules.rows("si_sdr", "estimate", estimate, max_b=rules.MAX_BATCH)
    _on_gpu("si_sdr", s, e)
    return rules.unbatch(N.si_sdr(s, e), not single)


def log_spectral_distance(p, q, eps=1e-10):
    """Log-spectral distance of power spectrograms p, q: (B, F, T) or (F, T), float32 or float64 on the GPU -> (B,) float64 dB
    (0-d for (F, T) input), the mean over the frames of sqrt(mean_f (10 log10((p + eps) / (q + eps)))^2).  A spectrogram pair
    with a negative or non-finite entry gives NaN."""
    rules.nonneg("log_spectral_distance", "eps", eps)
    _pair(p, q, "log_spectral_distance", ("p", "q"), dims=(2, 3))
    if p.dtype not in (torch.float32, torch.float64):
        raise ValueError("log_spectral_distance: p and q must be float32 or float64, got %s" % p.dtype)
    single = p.dim() == 2
    ps, qs = (p.unsqueeze(0), q.unsqueeze(0)) if single else (p, q)
    B, F, T = ps.shape
    if B < 1 or B > 65535 or F < 1 or T < 1 or F * T > 1 << 30:
        raise ValueError("log_spectral_distance: need 1 <= B <= 65535, F, T >= 1 and F T <= 2^30, got shape %s" % (tuple(p.shape),))
    _on_gpu("log_spectral_distance", ps, qs)
    return rules.unbatch(N.lsd(ps.contiguous(), qs.contiguous(), float(eps)), not single)


# ------------------------------------------------------------------------------------------------------ separation scores
ASSIGN = collections.namedtuple("ASSIGN", "perm total status")
PIT = collections.namedtuple("PIT", "value perm status")
SIBSS = collections.namedtuple("SIBSS", "sdr sir sar perm status")

MAX_SOURCES = 8


def _sources(references, estimates, who, square=False):
    """references as contiguous (B, K, n) and estimates as (B, J, n), and whether they came without B.  square: K <= J is
    required (every reference takes an estimate of its own).  The device is checked by the caller, last."""
    for t, name in ((references, "references"), (estimates, "estimates")):
        if not isinstance(t, torch.Tensor) or t.dim() not in (2, 3):
            raise ValueError("%s: %s must be a (sources, n) or (B, sources, n) tensor" % (who, name))
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError("%s: %s must be float32 or float64, got %s" % (who, name, t.dtype))
    if references.dim() != estimates.dim() or references.dtype != estimates.dtype:
        raise ValueError("%s: references %s %s and estimates %s %s differ in rank or dtype"
                         % (who, references.dtype, tuple(references.shape), estimates.dtype, tuple(estimates.shape)))
    single = references.dim() == 2
    s, e = (references[None], estimates[None]) if single else (references, estimates)
    (B, K, n), J = s.shape, e.shape[1]
    if e.shape[0] != B or e.shape[2] != n:
        raise ValueError("%s: references %s and estimates %s differ in B or n" % (who, tuple(references.shape), tuple(estimates.shape)))
    if B < 1 or B > 65535 or K < 1 or K > MAX_SOURCES or J < 1 or J > MAX_SOURCES or n < 2 or n > 1 << 24:
        raise ValueError("%s: need 1 <= B <= 65535, 1 <= K, J <= 8 and 2 <= n <= 2^24, got references %s and estimates %s"
                         % (who, tuple(references.shape), tuple(estimates.shape)))
    if square and K > J:
        raise ValueError("%s: %d references need at least as many estimates, got %d" % (who, K, J))
    return s.contiguous(), e.contiguous(), single


def pairwise_si_sdr(references, estimates):
    """The SI-SDR of every estimate against every reference: (B, K, n) and (B, J, n), or (K, n) and (J, n), float32 or float64
    on the GPU, 1 <= K, J <= 8 -> (B, K, J) float64 dB ((K, J) without B).  Entry [b, i, j] has the bits of
    ``si_sdr(references[b, i], estimates[b, j])``; the reference row is streamed once per pass for all J estimates."""
    s, e, single = _sources(references, estimates, "pairwise_si_sdr")
    _on_gpu("pairwise_si_sdr", s, e)
    return rules.unbatch(N.pairwise_si_sdr(s, e), not single)


def assign(table, maximize=True):
    """The assignment of J columns to K <= J rows with the largest (``maximize=False``: smallest) sum of entries: table
    (B, K, J) or (K, J), float64 on the GPU, J <= 8 -> ``ASSIGN(perm (B, K) int32, total (B,) float64, status (B,) int32)``,
    without B for a (K, J) table.  Exhaustive and exact: the rule is the module's docstring."""
    who = "assign"
    if not isinstance(table, torch.Tensor) or table.dim() not in (2, 3):
        raise ValueError("%s: table must be a (K, J) or (B, K, J) tensor" % who)
    if table.dtype != torch.float64:
        raise ValueError("%s: table must be float64, got %s" % (who, table.dtype))
    if not isinstance(maximize, bool):
        raise ValueError("%s: maximize must be True or False, got %r" % (who, maximize))
    single = table.dim() == 2
    t = table[None] if single else table
    B, K, J = t.shape
    if B < 1 or B > 65535 or K < 1 or K > J or J > MAX_SOURCES:
        raise ValueError("%s: need 1 <= B <= 65535 and 1 <= K <= J <= 8, got shape %s" % (who, tuple(table.shape)))
    _on_gpu(who, t)
    return rules.unbatch(ASSIGN(*N.assign(t.contiguous(), maximize)), not single)


def _pit(s, e):
    table = N.pairwise_si_sdr(s, e)
    perm, _, status = N.assign(table, True)
    return table, PIT(torch.gather(table, 2, perm.long()[:, :, None])[:, :, 0], perm, status)


def pit_si_sdr(references, estimates):
    """The permutation-invariant SI-SDR: ``assign(pairwise_si_sdr(references, estimates))`` -> ``PIT(value (B, K) float64 dB,
    perm (B, K) int32, status (B,) int32)``, value[b, k] = table[b, k, perm[b, k]] gathered on the device; K <= J, so K talkers
    can be scored against, say, ``cacgmm``'s K + 1 classes.  Without B for (K, n) input."""
    s, e, single = _sources(references, estimates, "pit_si_sdr", square=True)
    _on_gpu("pit_si_sdr", s, e)
    return rules.unbatch(_pit(s, e)[1], not single)


def si_bss_eval(references, estimates, perm=None):
    """Scale-invariant SDR, SIR and SAR of estimates[b, perm[b, i]] against references[b, i] among the item's K references:
    shapes as ``pit_si_sdr``; perm None (``pit_si_sdr``'s) or int32 (B, K) on the GPU ((K,) without B) ->
    ``SIBSS(sdr, sir, sar (B, K) float64 dB, perm (B, K) int32, status (B,) int32)``.  sdr[b, i] has the bits of
    ``pairwise_si_sdr``'s [b, i, perm[b, i]]; a low sir says crosstalk was left, a low sar says the target was distorted.  The
    definitions and the status values are the module's docstring."""
    who = "si_bss_eval"
    s, e, single = _sources(references, estimates, who, square=True)
    if perm is not None:
        want = tuple(s.shape[1:2]) if single else tuple(s.shape[:2])
        if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int32 or tuple(perm.shape) != want:
            raise ValueError("%s: perm must be None or an int32 %s tensor for references %s" % (who, want, tuple(references.shape)))
    _on_gpu(who, s, e)
    if perm is None:
        p = _pit(s, e)[1].perm
    else:
        _on_gpu(who, perm)
        p = (perm[None] if single else perm).contiguous()
    sdr, sir, sar, status = N.si_bss_eval(s, e, p)
    return rules.unbatch(SIBSS(sdr, sir, sar, p, status), not single)


def si_sdr_improvement(references, estimates, mixture):
    """What a separator gained: ``pit_si_sdr(references, estimates).value[b, k]`` minus the SI-SDR of the mixture against
    references[b, k] (``pairwise_si_sdr`` with the mixture as the one estimate).  mixture: (B, n), or (n,) for (K, n) sources,
    of the sources' dtype -> (B, K) float64 dB."""
    who = "si_sdr_improvement"
    s, e, single = _sources(references, estimates, who, square=True)
    if not isinstance(mixture, torch.Tensor) or mixture.dtype != s.dtype \
            or tuple(mixture.shape) != ((s.shape[2],) if single else (s.shape[0], s.shape[2])):
        raise ValueError("%s: mixture must be a %s %s tensor for references %s"
                         % (who, s.dtype, (s.shape[2],) if single else (s.shape[0], s.shape[2]), tuple(references.shape)))
    _on_gpu(who, s, e, mixture)
    m = (mixture[None] if single else mixture)[:, None].contiguous()
    return rules.unbatch(_pit(s, e)[1].value - N.pairwise_si_sdr(s, m)[:, :, 0], not single)
