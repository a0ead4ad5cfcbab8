"""Float64 numpy restatement of the speech measures of acoustic_locating_vq_vae.speech_metrics (STOI of Taal, Hendriks,
Heusdens and Jensen 2011, SI-SDR, log-spectral distance) -- TEST INFRASTRUCTURE ONLY.  The kernels are
csrc/speech_metrics.hip; the definitions are the comments on alvq_stoi_f64, alvq_si_sdr_* and alvq_lsd_* in include/alvq.h.

Loops over frames and segments, one definition a line, no cleverness.  ``resample_poly`` restates the polyphase formula with
a loop over output samples; the tests compare the device against scipy.signal.resample_poly itself.
"""
import collections
import math

import numpy as np

FS = 10000
N_FRAME, HOP, NFFT = 256, 128, 512
NUM_BANDS, MIN_FREQ = 15, 150.0
SEG = 30
BETA_DB = -15.0
DYN_RANGE_DB = 40.0
EPS = 2.0 ** -52
BAD_ENERGY, FEW_FRAMES = 1, 2

Stoi = collections.namedtuple("Stoi", "value kept_frames status nf margin")


def window():
    """The 258-point symmetric Hann window without its zero end points."""
    i = np.arange(N_FRAME, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 1.0) / (N_FRAME + 1.0))


def band_edges():
    """(lo, hi): band j sums the DFT bins lo[j] <= k < hi[j], the bins nearest (first on a tie) to the one-third-octave edges."""
    f = np.arange(NFFT // 2 + 1, dtype=np.float64) * FS / NFFT
    lo, hi = [], []
    for j in range(NUM_BANDS):
        lo.append(int(np.argmin((f - MIN_FREQ * 2.0 ** ((2 * j - 1) / 6.0)) ** 2)))
        hi.append(int(np.argmin((f - MIN_FREQ * 2.0 ** ((2 * j + 1) / 6.0)) ** 2)))
    return lo, hi


def frames(x):
    """The frames that lie wholly inside x, (nf, 256)."""
    nf = (len(x) - N_FRAME) // HOP + 1 if len(x) >= N_FRAME else 0
    return np.stack([x[HOP * t:HOP * t + N_FRAME] for t in range(nf)]) if nf else np.zeros((0, N_FRAME))


def stoi(clean, degraded):
    """STOI of one pair of rows at 10 kHz -> Stoi(value, kept_frames, status, nf, margin); margin is the smallest distance in
    dB of a frame's level to the silent-frame threshold (inf where there is none)."""
    x, y = np.asarray(clean, dtype=np.float64), np.asarray(degraded, dtype=np.float64)
    assert x.shape == y.shape and x.ndim == 1
    W = window()
    fx, fy = frames(x) * W, frames(y) * W
    nf = fx.shape[0]
    bad = Stoi(np.nan, 0, BAD_ENERGY, nf, np.inf)
    if nf == 0:
        return bad
    energy = np.array([np.sum(fx[t] * fx[t]) for t in range(nf)])
    if not (np.all(np.isfinite(energy)) and energy.max() > 0.0):
        return bad
    e = 20.0 * np.log10(np.sqrt(energy) + EPS)
    threshold = e.max() - DYN_RANGE_DB
    keep = [t for t in range(nf) if e[t] > threshold]
    margin = float(np.min(np.abs(e - threshold)))
    M = len(keep)
    if M < SEG:
        return Stoi(np.nan, M, FEW_FRAMES, nf, margin)
    # both signals rebuilt from the kept frames by overlap-add
    xr, yr = np.zeros(HOP * (M - 1) + N_FRAME), np.zeros(HOP * (M - 1) + N_FRAME)
    for m, t in enumerate(keep):
        xr[HOP * m:HOP * m + N_FRAME] += fx[t]
        yr[HOP * m:HOP * m + N_FRAME] += fy[t]
    # one-third-octave band envelopes
    lo, hi = band_edges()
    X, Y = np.zeros((NUM_BANDS, M)), np.zeros((NUM_BANDS, M))
    for m in range(M):
        sx = np.abs(np.fft.rfft(xr[HOP * m:HOP * m + N_FRAME] * W, NFFT)) ** 2
        sy = np.abs(np.fft.rfft(yr[HOP * m:HOP * m + N_FRAME] * W, NFFT)) ** 2
        for j in range(NUM_BANDS):
            X[j, m] = np.sqrt(np.sum(sx[lo[j]:hi[j]]))
            Y[j, m] = np.sqrt(np.sum(sy[lo[j]:hi[j]]))
    # clipped, normalised correlation of every 30-frame segment of every band
    clip = 1.0 + 10.0 ** (-BETA_DB / 20.0)
    total = 0.0
    for s in range(SEG, M + 1):
        for j in range(NUM_BANDS):
            xs, ys = X[j, s - SEG:s], Y[j, s - SEG:s]
            alpha = np.sqrt(np.sum(xs * xs)) / (np.sqrt(np.sum(ys * ys)) + EPS)
            yc = np.minimum(alpha * ys, clip * xs)
            xs = xs - np.mean(xs)
            yc = yc - np.mean(yc)
            xs = xs / (np.sqrt(np.sum(xs * xs)) + EPS)
            yc = yc / (np.sqrt(np.sum(yc * yc)) + EPS)
            total += np.sum(xs * yc)
    return Stoi(total / (NUM_BANDS * (M - SEG + 1)), M, 0, nf, margin)


def si_sdr(reference, estimate):
    """Scale-invariant signal-to-distortion ratio in dB; +inf for an exact multiple of the reference, NaN for a reference of
    zero or non-finite energy."""
    s, e = np.asarray(reference, dtype=np.float64), np.asarray(estimate, dtype=np.float64)
    s, e = s - np.mean(s), e - np.mean(e)
    ss = np.sum(s * s)
    if not (np.isfinite(ss) and ss > 0.0):
        return np.nan
    alpha = np.sum(e * s) / ss
    target = alpha * s
    num, den = np.sum(target * target), np.sum((target - e) ** 2)
    if np.isnan(num) or np.isnan(den):
        return np.nan
    if den == 0.0:
        return np.inf
    return 10.0 * np.log10(num / den)


def log_spectral_distance(p, q, eps=1e-10):
    """Mean over the frames t of sqrt(mean_f (10 log10((p + eps) / (q + eps)))^2) for power spectrograms (F, T), in dB; NaN
    for negative or non-finite input."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    if not (np.all(np.isfinite(p)) and np.all(np.isfinite(q)) and p.min() >= 0.0 and q.min() >= 0.0):
        return np.nan
    F, T = p.shape
    total = 0.0
    for t in range(T):
        d = 10.0 * np.log10((p[:, t] + eps) / (q[:, t] + eps))
        total += np.sqrt(np.sum(d * d) / F)
    return total / T


def resample_filter(up, down):
    """(h, up, down, half) of scipy.signal.resample_poly's default filter after reducing up / down by their gcd."""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    R = max(up, down)
    half = 10 * R
    k = np.arange(2 * half + 1, dtype=np.float64)
    h = np.sinc((k - half) / R) / R * np.kaiser(2 * half + 1, 5.0)
    return h / np.sum(h) * up, up, down, half


def resample_poly(x, up, down):
    """y[m] = sum_j x[j] h[m down - j up + half] over the j with both indices in range, j ascending; ceil(n up / down) samples."""
    x = np.asarray(x, dtype=np.float64)
    h, up, down, half = resample_filter(up, down)
    n = len(x)
    y = np.zeros(-(-n * up // down))
    for m in range(len(y)):
        j0 = max(0, -((half - m * down) // up))
        j1 = min(n - 1, (m * down + half) // up)
        acc = 0.0
        for j in range(j0, j1 + 1):
            acc += x[j] * h[m * down - j * up + half]
        y[m] = acc
    return y
