"""The baseline a learned locator is measured against, on the device (csrc/srp_phat.hip): the textbook way from a microphone
array's spectrograms to a source position -- PHAT-weighted cross-spectra of the microphone pairs, generalised
cross-correlation (GCC-PHAT, Knapp and Carter 1976) with its time differences of arrival, and the steered response power map
(SRP-PHAT, DiBiase 2000) over candidate positions with its arg-max.  Float64 arithmetic, fixed-order sums, no host sync.

    from acoustic_locating_vq_vae import front_end as FE, localization as LOC
    h = FE.array_impulse_responses(src, mics, room, reverberation_time=0.4, nsample=6400)     # (B, D, nsample)
    spec = FE.array_spectrograms(wave, h)                                                     # (B, D, F, T) complex128
    ring = LOC.locate_on_ring(spec, mics, receiver, room, R=1, z=1)   # theta (B,): the label ``LocationModule`` regresses
    LOC.srp_phat(spec, mics, grid).best                                # (B,) the arg-max over any (G, 3) grid of positions
    LOC.tdoa(spec, max_lag=8)                                          # (B, P) seconds, pair (i, j): arrival at i minus at j
    LOC.music(spec, mics, grid, n_sources=2).null                      # (B, G) the MUSIC null spectrum: sources are its minima

Definitions (in full: include/alvq.h).  The pairs p = (i, j), i < j, run in lexicographic order, P = D (D - 1) / 2.  With
u(z) = z / |z| (0 for z = 0) taken per microphone, psi[p, f] = mean_t u(X_i[f, t]) conj(u(X_j[f, t])) inside the band and 0
outside it.  w_f = 1 at DC and at Nyquist, 2 elsewhere, W1 its sum over the band.  GCC: r[p, l] = (1 / W1) sum_f w_f
Re(psi[p, f] e^{+j 2 pi f l / n_fft}), whose peak lag is (arrival at i) - (arrival at j) in samples.  SRP: with
tau_d(q) = |q - m_d| / c, S[g] = (1 / (P W1)) sum_p sum_f w_f Re(psi[p, f] e^{+j 2 pi f (fs / n_fft) (tau_i(q_g) - tau_j(q_g))}),
which is 1 for perfectly coherent arrivals from q_g.  ``status`` (int32 per item) is a set of bits: 1 = a non-finite
spectrogram value inside the band, 4 = a non-finite microphone or candidate coordinate (either: the map row is NaN), 2 = the
item is silent inside the band (the row is 0); ``best`` is -1 with any of them.  Nothing here reads it: the caller does, when
it can sync.  The band is given in bins, (f_lo, f_hi) inclusive; None means (1, F - 2): everything but DC and Nyquist.
"""
import collections
import math

import numpy as np
import torch

from . import _native as N
from . import front_end as FE
from .front_end import N_FFT, SOUND_SPEED

GCC = collections.namedtuple("GCC", "corr lags")
SRP = collections.namedtuple("SRP", "map best status")
Ring = collections.namedtuple("Ring", "theta source map status")
Music = collections.namedtuple("Music", "null best status values")

MAX_MICROPHONES = 8
MAX_FRAMES = 65535


def _int_in(who, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or v > hi:
        raise ValueError("%s: %s must be an integer in [%d, %d], got %r" % (who, name, lo, hi, v))


def _positive(who, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v > 0):
        raise ValueError("%s: %s must be a finite number > 0, got %r" % (who, name, v))


def _spec4(who, spec, n_fft=None):
    """spec as (B, D, F, T), checked; whether it came with a batch dimension."""
    if not isinstance(spec, torch.Tensor) or spec.dim() not in (3, 4):
        raise ValueError("%s: spec must be a (D, F, T) or (B, D, F, T) tensor" % who)
    if spec.dtype not in (torch.complex64, torch.complex128):
        raise ValueError("%s: spec must be complex64 or complex128, got %s" % (who, spec.dtype))
    x = spec[None] if spec.dim() == 3 else spec
    B, D, F, T = x.shape
    if B < 1 or B > 65535 or F < 1 or B * F > 2 ** 31 - 1 or T < 1 or T > MAX_FRAMES:
        raise ValueError("%s: need 1 <= B <= 65535, F >= 1, B F <= 2^31 - 1 and 1 <= T <= 65535, got shape %s" % (who, tuple(spec.shape)))
    if D < 2 or D > MAX_MICROPHONES:
        raise ValueError("%s: need 2 <= D <= 8 microphones, got D = %d" % (who, D))
    if n_fft is not None:
        _int_in(who, "n_fft", n_fft, 2, 2 ** 24)
        if F != n_fft // 2 + 1:
            raise ValueError("%s: %d frequency bins, n_fft=%d has %d" % (who, F, n_fft, n_fft // 2 + 1))
    return x, spec.dim() == 4


def _band(who, band, F):
    if band is None:
        band = (1, F - 2)
        if F < 3:
            raise ValueError("%s: the default band (1, F - 2) is empty for F = %d; give band" % (who, F))
    if not isinstance(band, (tuple, list)) or len(band) != 2:
        raise ValueError("%s: band must be (f_lo, f_hi) in bins, got %r" % (who, band))
    lo, hi = band
    _int_in(who, "band[0]", lo, 0, F - 1)
    _int_in(who, "band[1]", hi, lo, F - 1)
    return int(lo), int(hi)


def _on_gpu(who, t, name="spec"):
    if not t.is_cuda:
        raise RuntimeError("%s: %s must live on the GPU (got %s); the HIP path has no CPU fallback" % (who, name, t.device))


def _geometry(who, name, t, B, rows=None):
    """A float64 (n, 3) or (B, n, 3) tensor of positions."""
    if not isinstance(t, torch.Tensor) or t.dim() not in (2, 3) or t.shape[-1] != 3 or t.dtype != torch.float64:
        raise ValueError("%s: %s must be a float64 (n, 3) or (B, n, 3) tensor" % (who, name))
    if t.dim() == 3 and t.shape[0] != B:
        raise ValueError("%s: %s holds %d items, spec %d" % (who, name, t.shape[0], B))
    if t.shape[-2] < 1 or (rows is not None and t.shape[-2] != rows):
        raise ValueError("%s: %s must hold %s positions, got %d" % (who, name, rows if rows is not None else ">= 1", t.shape[-2]))


def cross_spectra(spec, band=None):
    """PHAT-weighted cross-spectra: spec (D, F, T) or (B, D, F, T), complex64 or complex128 on the GPU -> (P, F) or (B, P, F)
    complex128, 0 outside the band."""
    x, batched = _spec4("cross_spectra", spec)
    lo, hi = _band("cross_spectra", band, x.shape[2])
    _on_gpu("cross_spectra", x)
    psi, _ = N.phat_cross_spectra(x, lo, hi)
    return psi if batched else psi[0]


def gcc_phat(spec, max_lag, band=None, n_fft=N_FFT):
    """GCC-PHAT of every microphone pair at the integer lags -max_lag .. max_lag: ``GCC(corr, lags)`` with corr
    (B, P, 2 max_lag + 1) float64 (no B for a (D, F, T) spec) and lags (2 max_lag + 1,) int64, both on the GPU."""
    x, batched = _spec4("gcc_phat", spec, n_fft)
    _int_in("gcc_phat", "max_lag", max_lag, 0, n_fft // 2)
    lo, hi = _band("gcc_phat", band, x.shape[2])
    _on_gpu("gcc_phat", x)
    psi, _ = N.phat_cross_spectra(x, lo, hi)
    corr = N.gcc_phat(psi, n_fft, max_lag, lo, hi)
    lags = torch.arange(-int(max_lag), int(max_lag) + 1, device=x.device)
    return GCC(corr if batched else corr[0], lags)


def tdoa(spec, max_lag, fs=16000, band=None, n_fft=N_FFT):
    """Time differences of arrival, (B, P) float64 seconds (no B for a (D, F, T) spec): for the pair (i, j) the arrival at i
    minus the arrival at j.  The arg-max lag of ``gcc_phat`` (the lowest on ties) plus the vertex of the parabola through the
    peak and its neighbours, delta = 0.5 (r[-1] - r[+1]) / (r[-1] - 2 r[0] + r[+1]), where the peak is interior and that
    denominator is < 0; delta = 0 otherwise."""
    _positive("tdoa", "fs", fs)
    corr, lags = gcc_phat(spec, max_lag, band, n_fft)
    n = corr.shape[-1]
    # the lowest index of the maximum (torch.argmax does not promise which of several it returns); 0 for a row with a NaN
    index = torch.arange(n, device=corr.device)
    peak = torch.where(corr == corr.amax(dim=-1, keepdim=True), index, n).amin(dim=-1).clamp_max(n - 1)
    peak = torch.where(torch.isnan(corr).any(dim=-1), torch.zeros_like(peak), peak)
    delta = torch.zeros_like(corr[..., 0])
    if n >= 3:
        mid = peak.clamp(1, n - 2)
        left, centre, right = (corr.gather(-1, (mid + o).unsqueeze(-1)).squeeze(-1) for o in (-1, 0, 1))
        den = left - 2.0 * centre + right
        ok = (peak == mid) & (den < 0)
        delta = torch.where(ok, 0.5 * (left - right) / torch.where(ok, den, torch.ones_like(den)), delta)
    return (lags[peak].to(torch.float64) + delta) / float(fs)


def srp_phat(spec, mics, candidates, fs=16000, n_fft=N_FFT, c=SOUND_SPEED, band=None):
    """The SRP-PHAT map: spec (D, F, T) or (B, D, F, T) complex64 / complex128, microphones mics (D, 3) or (B, D, 3) and
    candidates (G, 3) or (B, G, 3), float64, all on the GPU -> ``SRP(map, best, status)``: map (B, G) float64, best (B,) int32
    (the arg-max, the lowest index on ties; -1 with a status), status (B,) int32 -- (G,) and two scalars for a (D, F, T) spec."""
    x, batched = _spec4("srp_phat", spec, n_fft)
    B, D = x.shape[0], x.shape[1]
    _positive("srp_phat", "fs", fs)
    _positive("srp_phat", "c", c)
    lo, hi = _band("srp_phat", band, x.shape[2])
    _geometry("srp_phat", "mics", mics, B, D)
    _geometry("srp_phat", "candidates", candidates, B)
    if B * candidates.shape[-2] > 2 ** 31 - 1:
        raise ValueError("srp_phat: need B G <= 2^31 - 1, got B = %d, G = %d" % (B, candidates.shape[-2]))
    _on_gpu("srp_phat", x)
    _on_gpu("srp_phat", mics, "mics")
    _on_gpu("srp_phat", candidates, "candidates")
    psi, _ = N.phat_cross_spectra(x, lo, hi)
    out, best, status = N.srp_phat(psi, mics, candidates, fs, n_fft, c, lo, hi)
    return SRP(out, best, status) if batched else SRP(out[0], best[0], status[0])


def _music_rules(who, B, D, F, mics, candidates, n_sources, fs, n_fft, c, band):
    """The rules ``music`` and ``music_from_covariance`` share, ValueErrors only -> the band in bins."""
    _int_in(who, "n_sources", n_sources, 1, D - 1)
    _positive(who, "fs", fs)
    _positive(who, "c", c)
    lo, hi = _band(who, band, F)
    _geometry(who, "mics", mics, B, D)
    _geometry(who, "candidates", candidates, B)
    if B * candidates.shape[-2] > 2 ** 31 - 1:
        raise ValueError("%s: need B G <= 2^31 - 1, got B = %d, G = %d" % (who, B, candidates.shape[-2]))
    return lo, hi


def _music(cov, cov_status, mics, candidates, n_sources, fs, n_fft, c, lo, hi):
    """Checked arguments, cov (B, F, D, D) -> a batched Music."""
    B, F, D, _ = cov.shape
    values, vectors, eig_status = N.eigh(cov.reshape(B * F, D, D))
    values, vectors, eig_status = values.view(B, F, D), vectors.view(B, F, D, D), eig_status.view(B, F)
    null, best, status = N.music(vectors, values, mics, candidates, n_sources, fs, n_fft, c, lo, hi)
    bins = eig_status if cov_status is None else (eig_status | cov_status)
    flagged = (bins[:, lo:hi + 1] != 0).any(dim=1)
    status = status | flagged.to(torch.int32)
    null = torch.where(flagged[:, None], torch.full_like(null, float("nan")), null)
    best = torch.where(flagged, torch.full_like(best, -1), best)
    return Music(null, best, status, values)


def music(spec, mics, candidates, n_sources=1, fs=16000, n_fft=N_FFT, c=SOUND_SPEED, band=None):
    """MUSIC (Schmidt 1986), the subspace locator: spec (D, F, T) or (B, D, F, T) complex64 / complex128, mics (D, 3) or
    (B, D, 3) and candidates (G, 3) or (B, G, 3), float64, all on the GPU; 1 <= n_sources <= D - 1 is the dimension K of the
    signal subspace -> ``Music(null, best, status, values)``.  The spatial covariance of every bin (no mask), its
    eigendecomposition (``subspace.eigh``), then with e_k the eigenvectors of the K largest eigenvalues and a_d =
    e^{-j 2 pi f (fs / n_fft) tau_d(q)} (``beamforming.steering_vectors``' sign), null[g] = the mean over the band's counted
    bins of 1 - (1 / D) sum_k |e_k^H a(q_g)|^2: 0 where the steering vector lies in the signal subspace, so sources are its
    minima.  A bin whose eigenvalues are all 0 is not counted.  null (B, G) float64; best (B,) int32 the arg-min (the lowest
    index on ties); status (B,) int32 bits: 1 = a non-finite value, or a covariance / eigensolver status, inside the band (the
    row is NaN), 4 = a non-finite coordinate (NaN), 2 = no counted bin (the row is 1); best is -1 with any; values
    (B, F, D) float64, the eigenvalues ascending: their profile tells how many sources there are -- (G,), two scalars and
    (F, D) for a (D, F, T) spec."""
    who = "music"
    x, batched = _spec4(who, spec, n_fft)
    B, D, F = x.shape[0], x.shape[1], x.shape[2]
    lo, hi = _music_rules(who, B, D, F, mics, candidates, n_sources, fs, n_fft, c, band)
    _on_gpu(who, x)
    _on_gpu(who, mics, "mics")
    _on_gpu(who, candidates, "candidates")
    cov, cov_status = N.spatial_covariance(x, None)
    out = _music(cov, cov_status, mics, candidates, n_sources, fs, n_fft, c, lo, hi)
    return out if batched else Music(out.null[0], out.best[0], out.status[0], out.values[0])


def music_from_covariance(cov, mics, candidates, n_sources=1, fs=16000, n_fft=N_FFT, c=SOUND_SPEED, band=None):
    """``music`` on spatial covariances the caller has formed -- ``beamforming.spatial_covariance(spec, mask).cov`` with the
    mask of a model, say: cov (F, D, D) or (B, F, D, D) complex128 on the GPU, Hermitian (the lower triangle is read),
    F = n_fft / 2 + 1, 2 <= D <= 8.  The covariances' own status is the caller's."""
    who = "music_from_covariance"
    if not isinstance(cov, torch.Tensor) or cov.dim() not in (3, 4) or cov.dtype != torch.complex128:
        raise ValueError("%s: cov must be a complex128 (F, D, D) or (B, F, D, D) tensor" % who)
    batched = cov.dim() == 4
    y = cov if batched else cov[None]
    B, F, D = y.shape[0], y.shape[1], y.shape[2]
    if y.shape[3] != D or D < 2 or D > MAX_MICROPHONES:
        raise ValueError("%s: need square covariances of 2 <= D <= 8 microphones, got shape %s" % (who, tuple(cov.shape)))
    if B < 1 or B > 65535 or F < 1 or B * F > 2 ** 31 - 1:
        raise ValueError("%s: need 1 <= B <= 65535, F >= 1 and B F <= 2^31 - 1, got shape %s" % (who, tuple(cov.shape)))
    _int_in(who, "n_fft", n_fft, 2, 2 ** 24)
    if F != n_fft // 2 + 1:
        raise ValueError("%s: %d frequency bins, n_fft=%d has %d" % (who, F, n_fft, n_fft // 2 + 1))
    lo, hi = _music_rules(who, B, D, F, mics, candidates, n_sources, fs, n_fft, c, band)
    _on_gpu(who, y, "cov")
    _on_gpu(who, mics, "mics")
    _on_gpu(who, candidates, "candidates")
    out = _music(y, None, mics, candidates, n_sources, fs, n_fft, c, lo, hi)
    return out if batched else Music(out.null[0], out.best[0], out.status[0], out.values[0])


def ring_candidates(n_angles, receiver, room, R, z, device="cuda"):
    """The positions the dataset generator can produce, as candidates: ``(theta_grid (n,), points (n, 3))`` float64 on the GPU
    with theta_k = -pi + 2 pi k / n and points = min(receiver + (R cos theta, R sin theta, z), room)
    (``front_end.source_positions``, its clip to the room included)."""
    _int_in("ring_candidates", "n_angles", n_angles, 1, 2 ** 31 - 1)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("ring_candidates: device must be a GPU (got %s); the HIP path has no CPU fallback" % device)
    theta = -math.pi + (2.0 * math.pi / n_angles) * torch.arange(n_angles, dtype=torch.float64, device=device)
    points = FE._ring_sources(theta, FE._positions(receiver, "receiver", device), FE._positions(room, "room", device), R, z)
    return theta, points


def locate_on_ring(spec, mics, receiver, room, R, z, n_angles=360, method="srp", n_sources=1, **srp_kwargs):
    """The classical estimate of the label ``LocationModule`` is trained on: SRP-PHAT over ``ring_candidates`` ->
    ``Ring(theta (B,), source (B, 3), map (B, n_angles), status (B,))``, theta and source those of the arg-max (of candidate
    0 where status is not 0: read status).  method "music" runs ``music(spec, mics, points, n_sources, ...)`` in its place:
    map is then the null spectrum and the pick its arg-min."""
    if not isinstance(spec, torch.Tensor):
        raise ValueError("locate_on_ring: spec must be a (D, F, T) or (B, D, F, T) tensor")
    if method not in ("srp", "music"):
        raise ValueError("locate_on_ring: method must be 'srp' or 'music', got %r" % (method,))
    if method == "srp" and n_sources != 1:
        raise ValueError("locate_on_ring: n_sources goes with method 'music', got %r" % (n_sources,))
    _on_gpu("locate_on_ring", spec)
    theta, points = ring_candidates(n_angles, receiver, room, R, z, spec.device)
    if method == "music":
        found = music(spec, mics, points, n_sources, **srp_kwargs)
        pick = found.best.clamp_min(0).to(torch.int64)
        return Ring(theta[pick], points[pick], found.null, found.status)
    srp = srp_phat(spec, mics, points, **srp_kwargs)
    pick = srp.best.clamp_min(0).to(torch.int64)
    return Ring(theta[pick], points[pick], srp.map, srp.status)
