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

import torch

from . import _native as N
from . import _rules as rules
from . import front_end as FE
from ._rules import MAX_FRAMES, MAX_MICROPHONES  # noqa: F401 -- public here
from .front_end import N_FFT, SOUND_SPEED

GCC = collections.namedtuple("GCC", "corr lags")
SRP = collections.namedtuple("SRP", "map best status")
Ring = collections.namedtuple("Ring", "theta source map status")
Music = collections.namedtuple("Music", "null best status values")


def _band(who, band, F):
    if band is None:
        band = (1, F - 2)
        if F < 3:
            raise ValueError("%s: the default band (1, F - 2) is empty for F = %d; give band" % (who, F))
    if not isinstance(band, (tuple, list)) or len(band) != 2:
        raise ValueError("%s: band must be (f_lo, f_hi) in bins, got %r" % (who, band))
    lo, hi = band
    rules.int_in(who, "band[0]", lo, 0, F - 1)
    rules.int_in(who, "band[1]", hi, lo, F - 1)
    return int(lo), int(hi)


def cross_spectra(spec, band=None):
    """PHAT-weighted cross-spectra: spec (D, F, T) or (B, D, F, T), complex64 or complex128 on the GPU -> (P, F) or (B, P, F)
    complex128, 0 outside the band."""
    x, batched = rules.spec4("cross_spectra", spec, 2)
    lo, hi = _band("cross_spectra", band, x.shape[2])
    rules.on_gpu("cross_spectra", x, "spec")
    return rules.unbatch(N.phat_cross_spectra(x, lo, hi)[0], batched)


def gcc_phat(spec, max_lag, band=None, n_fft=N_FFT):
    """GCC-PHAT of every microphone pair at the integer lags -max_lag .. max_lag: ``GCC(corr, lags)`` with corr
    (B, P, 2 max_lag + 1) float64 (no B for a (D, F, T) spec) and lags (2 max_lag + 1,) int64, both on the GPU."""
    x, batched = rules.spec4("gcc_phat", spec, 2, n_fft)
    rules.int_in("gcc_phat", "max_lag", max_lag, 0, n_fft // 2)
    lo, hi = _band("gcc_phat", band, x.shape[2])
    rules.on_gpu("gcc_phat", x, "spec")
    psi, _ = N.phat_cross_spectra(x, lo, hi)
    corr = N.gcc_phat(psi, n_fft, max_lag, lo, hi)
    lags = torch.arange(-int(max_lag), int(max_lag) + 1, device=x.device)
    return GCC(rules.unbatch(corr, batched), lags)


def tdoa(spec, max_lag, fs=16000, band=None, n_fft=N_FFT):
    """Time differences of arrival, (B, P) float64 seconds (no B for a (D, F, T) spec): for the pair (i, j) the arrival at i
    minus the arrival at j.  The arg-max lag of ``gcc_phat`` (the lowest on ties) plus the vertex of the parabola through the
    peak and its neighbours, delta = 0.5 (r[-1] - r[+1]) / (r[-1] - 2 r[0] + r[+1]), where the peak is interior and that
    denominator is < 0; delta = 0 otherwise."""
    rules.positive("tdoa", "fs", fs)
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
    x, batched = rules.spec4("srp_phat", spec, 2, n_fft)
    lo, hi = _map_rules("srp_phat", x.shape[0], x.shape[1], x.shape[2], mics, candidates, fs, c, band)
    rules.all_on_gpu("srp_phat", spec=x, mics=mics, candidates=candidates)
    psi, _ = N.phat_cross_spectra(x, lo, hi)
    return rules.unbatch(SRP(*N.srp_phat(psi, mics, candidates, fs, n_fft, c, lo, hi)), batched)


def _map_rules(who, B, D, F, mics, candidates, fs, c, band):
    """The rules of a map over candidates for D microphones and F bins, ValueErrors only -> the band in bins."""
    rules.positive(who, "fs", fs)
    rules.positive(who, "c", c)
    lo, hi = _band(who, band, F)
    rules.positions(who, "mics", mics, B, D)
    rules.positions(who, "candidates", candidates, B)
    if B * candidates.shape[-2] > 2 ** 31 - 1:
        raise ValueError("%s: need B G <= 2^31 - 1, got B = %d, G = %d" % (who, B, candidates.shape[-2]))
    return lo, hi


def _music_rules(who, B, D, F, mics, candidates, n_sources, fs, c, band):
    """The rules ``music`` and ``music_from_covariance`` share, ValueErrors only -> the band in bins."""
    rules.int_in(who, "n_sources", n_sources, 1, D - 1)
    return _map_rules(who, B, D, F, mics, candidates, fs, c, band)


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
    x, batched = rules.spec4(who, spec, 2, n_fft)
    B, D, F = x.shape[0], x.shape[1], x.shape[2]
    lo, hi = _music_rules(who, B, D, F, mics, candidates, n_sources, fs, c, band)
    rules.all_on_gpu(who, spec=x, mics=mics, candidates=candidates)
    cov, cov_status = N.spatial_covariance(x, None)
    return rules.unbatch(_music(cov, cov_status, mics, candidates, n_sources, fs, n_fft, c, lo, hi), batched)


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
    rules.bins(who, "shape %s" % (tuple(cov.shape),), B, F)
    rules.n_fft_bins(who, n_fft, F)
    lo, hi = _music_rules(who, B, D, F, mics, candidates, n_sources, fs, c, band)
    rules.all_on_gpu(who, cov=y, mics=mics, candidates=candidates)
    return rules.unbatch(_music(y, None, mics, candidates, n_sources, fs, n_fft, c, lo, hi), batched)


def ring_candidates(n_angles, receiver, room, R, z, device="cuda"):
    """The positions the dataset generator can produce, as candidates: ``(theta_grid (n,), points (n, 3))`` float64 on the GPU
    with theta_k = -pi + 2 pi k / n and points = min(receiver + (R cos theta, R sin theta, z), room)
    (``front_end.source_positions``, its clip to the room included)."""
    rules.int_in("ring_candidates", "n_angles", n_angles, 1, 2 ** 31 - 1)
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
    rules.on_gpu("locate_on_ring", spec, "spec")
    theta, points = ring_candidates(n_angles, receiver, room, R, z, spec.device)
    if method == "music":
        found = music(spec, mics, points, n_sources, **srp_kwargs)
        pick = found.best.clamp_min(0).to(torch.int64)
        return Ring(theta[pick], points[pick], found.null, found.status)
    srp = srp_phat(spec, mics, points, **srp_kwargs)
    pick = srp.best.clamp_min(0).to(torch.int64)
    return Ring(theta[pick], points[pick], srp.map, srp.status)
