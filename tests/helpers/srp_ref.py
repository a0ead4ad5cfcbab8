"""PHAT cross-spectra, GCC-PHAT and the SRP-PHAT map restated in numpy, straight from the definitions on
alvq_phat_cross_spectra_* / alvq_gcc_phat_f64 / alvq_srp_phat_f64 in include/alvq.h: in float64, or in np.longdouble (the
yardstick's yardstick).  Every pair and every bin is written out as the header has it -- one complex exponential per (pair,
bin, candidate) on the difference of the two delays -- with none of the kernel's regrouping.  Also the generator of the tests'
inputs (``case``) and the error bounds the CPU and the GPU tests share."""
import collections
import functools

import numpy as np

LD = np.longdouble
FS, C = 16000.0, 340.0
CENTRE = np.array([2.5, 1.5, 1.5])
U = 1.1e-16
BAD_SPECTRUM, SILENT, BAD_GEOMETRY = 1, 2, 4

Case = collections.namedtuple("Case", "X mics cand true")
Reference = collections.namedtuple("Reference", "psi map best status gap")


def _types(dtype):
    return (np.float64, np.complex128) if dtype == np.float64 else (LD, np.clongdouble)


def _pi(dtype):
    return np.pi if dtype == np.float64 else np.arccos(LD(-1))


def pairs(D):
    """(i, j), i < j, in lexicographic order."""
    return [(i, j) for i in range(D) for j in range(i + 1, D)]


def weights(n_fft, f_lo, f_hi, dtype=np.float64):
    """w_f over the band: 1 at DC and (n_fft even) at n_fft / 2, 2 elsewhere."""
    f = np.arange(f_lo, f_hi + 1)
    return np.where((f == 0) | (2 * f == n_fft), 1, 2).astype(dtype)


def unit(X, dtype=np.float64):
    """z / hypot(re z, im z) per component, 0 for z = 0."""
    real, cplx = _types(dtype)
    re, im = np.asarray(X.real).astype(real), np.asarray(X.imag).astype(real)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        h = np.hypot(re, im)
        zero = h == 0
        safe = np.where(zero, real(1), h)
        out = np.zeros(re.shape, cplx)
        out.real = np.where(zero, real(0), re / safe)
        out.imag = np.where(zero, real(0), im / safe)
    return out


def cross_spectra(X, f_lo, f_hi, dtype=np.float64):
    """X (B, D, F, T) complex -> (psi (B, P, F) complex of ``dtype``'s precision, 0 outside the band; status (B,) int32 with the
    bits 1 (a non-finite value of X inside the band) and 2 (every psi of the item 0))."""
    real, cplx = _types(dtype)
    B, D, F, T = X.shape
    pr = pairs(D)
    psi = np.zeros((B, len(pr), F), cplx)
    band = slice(f_lo, f_hi + 1)
    u = unit(X[:, :, band], dtype)
    with np.errstate(invalid="ignore"):
        for p, (i, j) in enumerate(pr):
            psi[:, p, band] = np.sum(u[:, i] * np.conj(u[:, j]), axis=-1) / real(T)
    status = np.zeros(B, np.int32)
    for b in range(B):
        xb = X[b, :, band]
        if not (np.isfinite(xb.real).all() and np.isfinite(xb.imag).all()):
            status[b] |= BAD_SPECTRUM
        elif not psi[b].any():
            status[b] |= SILENT
    return psi, status


def gcc_phat(psi, n_fft, L, f_lo, f_hi, dtype=np.float64):
    """psi (B, P, F) -> r (B, P, 2 L + 1) of ``dtype``: (1 / W1) sum_f w_f Re(psi e^{+j 2 pi f l / n_fft})."""
    real, cplx = _types(dtype)
    w = weights(n_fft, f_lo, f_hi, real)
    f = np.arange(f_lo, f_hi + 1).astype(real)
    lags = np.arange(-L, L + 1).astype(real)
    rot = np.exp(1j * (2 * _pi(dtype) * f[:, None] * lags[None, :] / real(n_fft)).astype(real)).astype(cplx)      # (Fb, lags)
    with np.errstate(invalid="ignore"):
        terms = (psi[:, :, f_lo:f_hi + 1, None].astype(cplx) * rot).real * w[:, None]
        return np.sum(terms, axis=2) / np.sum(w)


def delays(mics, cand, c=C, dtype=np.float64):
    """tau (B or 1, G, D) = |q_g - m_d| / c from mics (D, 3) or (B, D, 3) and cand (G, 3) or (B, G, 3)."""
    real, _ = _types(dtype)
    m = np.asarray(mics).astype(real)
    q = np.asarray(cand).astype(real)
    m = m[None] if m.ndim == 2 else m
    q = q[None] if q.ndim == 2 else q
    d = q[:, :, None, :] - m[:, None, :, :]
    return np.sqrt(np.sum(d * d, axis=-1)) / real(c)


def srp_phat(psi, mics, cand, fs, n_fft, c, f_lo, f_hi, dtype=np.float64, spectrum_status=None):
    """psi (B, P, F) -> (map (B, G) of ``dtype``, best (B,) int32, status (B,) int32), as the header defines them.
    spectrum_status: the status of ``cross_spectra`` (otherwise bit 1 is taken from a non-finite psi inside the band)."""
    real, cplx = _types(dtype)
    B, P, F = psi.shape
    D = next(d for d in range(2, 9) if d * (d - 1) // 2 == P)
    w = weights(n_fft, f_lo, f_hi, real)
    W1 = np.sum(w)
    f = np.arange(f_lo, f_hi + 1).astype(real)
    tau = delays(mics, cand, c, dtype)
    tau = np.broadcast_to(tau, (B,) + tau.shape[1:])
    G = tau.shape[1]
    S = np.zeros((B, G), real)
    two_pi = 2 * _pi(dtype)
    with np.errstate(invalid="ignore"):
        for p, (i, j) in enumerate(pairs(D)):
            dt = tau[:, :, i] - tau[:, :, j]                                                        # (B, G)
            phase = two_pi * f[None, None, :] * (real(fs) / real(n_fft)) * dt[:, :, None]          # (B, G, Fb)
            rot = np.exp(1j * phase.astype(real)).astype(cplx)
            S += np.sum((psi[:, p, None, f_lo:f_hi + 1].astype(cplx) * rot).real * w, axis=-1)
        S = S / (real(P) * W1)
    status = np.zeros(B, np.int32)
    best = np.zeros(B, np.int32)
    mb = np.broadcast_to(np.asarray(mics, float) if np.ndim(mics) == 3 else np.asarray(mics, float)[None], (B, D, 3))
    qb = np.broadcast_to(np.asarray(cand, float) if np.ndim(cand) == 3 else np.asarray(cand, float)[None], (B, G, 3))
    for b in range(B):
        band = psi[b, :, f_lo:f_hi + 1]
        if spectrum_status is not None:
            status[b] = spectrum_status[b]
        elif not (np.isfinite(band.real).all() and np.isfinite(band.imag).all()):
            status[b] |= BAD_SPECTRUM
        elif not band.any():
            status[b] |= SILENT
        if not (np.isfinite(mb[b]).all() and np.isfinite(qb[b]).all()):
            status[b] |= BAD_GEOMETRY
        if status[b] & (BAD_SPECTRUM | BAD_GEOMETRY):
            S[b] = np.nan
        elif status[b] & SILENT:
            S[b] = 0
        best[b] = -1 if status[b] else int(np.argmax(S[b]))           # np.argmax: the first of several maxima
    return S, best, status


# ------------------------------------------------------------------------------------------------------------------ bounds
def theta_max(f_hi, fs, n_fft, mics, cand, c=C):
    """Theta = 2 pi f_hi (fs / n_fft) max tau: the phase of the longest path at the top bin.  It enters the map's bound because
    a delay is rounded relative to itself, not relative to the difference of two delays."""
    return float(2 * np.pi * f_hi * (fs / n_fft) * delays(mics, cand, c).max())


def psi_bound(T):
    """|psi - psi_ref| <= (T + 8) u: products of unit phasors averaged over T."""
    return (T + 8) * U


ANCHOR = 8          # K: csrc/steered_map.h (kSteerAnchor) re-anchors the maps' rotation recurrence along f every 8 bins


def map_bound(D, T, f_lo, f_hi, theta):
    """|S - S_ref| <= (P F_band + T + 16 Theta + 32 + K) u: the summation of P F_band weighted terms of size at most
    w_f / (P W1), the psi error, the phase error, slack, and K for the kernel's rotation recurrence (at most 3 u a step on a
    phasor, K - 1 steps, two phasors a pair term: 42 u, within K + 32)."""
    P = D * (D - 1) // 2
    return (P * (f_hi - f_lo + 1) + T + 16 * theta + 32 + ANCHOR) * U


def gcc_bound(T, f_lo, f_hi, L):
    """|r - r_ref| <= (F_band + T + 8 pi L + 32) u."""
    return (f_hi - f_lo + 1 + T + 8 * np.pi * L + 32) * U


# ------------------------------------------------------------------------------------------------------------------- inputs
# (B, D, T, G, f_lo, f_hi, n_fft): the parity shapes of tests/test_srp_gpu.py, pinned by tests/test_srp_cpu.py
PARITY = [(2, 2, 1, 8, 1, 200, 400),          # one frame, one pair, Nyquist inside the band
          (2, 3, 5, 37, 8, 100, 400),         # odd G
          (1, 4, 16, 72, 8, 187, 400),
          (2, 8, 7, 360, 8, 187, 400),        # P = 28, more candidates than one tile
          (1, 8, 130, 64, 0, 200, 400),       # T no multiple of 64, the DC and Nyquist weights
          (3, 4, 3, 1, 8, 100, 400),          # G = 1
          (1, 8, 1500, 16, 8, 40, 400),       # rows that cannot sit in LDS whole
          (2, 4, 9, 24, 1, 31, 64)]           # n_fft = 64, F = 33


def ring(G, centre=CENTRE, R=1.0, z=1.0):
    """G candidates on the ring of radius R at height z above centre, theta_k = -pi + 2 pi k / G."""
    theta = -np.pi + 2 * np.pi * np.arange(G) / G
    return centre + np.stack((R * np.cos(theta), R * np.sin(theta), np.full(G, z)), axis=1)


@functools.lru_cache(maxsize=None)
def case(B, D, T, G, seed, n_fft=400, snr=0.1, aperture=0.05):
    """``Case(X, mics, cand, true)``: microphones mics (D, 3) = centre + aperture U(-1, 1)^3 around [2.5, 1.5, 1.5], G ring
    candidates cand (G, 3) of radius 1 at height +1, a true candidate index per item, and X (B, D, F, T) complex128 with
    X_d[f, t] = S[f, t] e^{-j omega_f r_d / c} / r_d plus complex Gaussian noise of scale snr (S complex Gaussian, r_d the
    distance from the true candidate to microphone d, omega_f = 2 pi f fs / n_fft).  The arrays are shared: read-only."""
    g = np.random.default_rng(seed)
    F = n_fft // 2 + 1
    mics = CENTRE + aperture * g.uniform(-1, 1, (D, 3))
    cand = ring(G)
    true = g.integers(0, G, B)
    omega = 2 * np.pi * np.arange(F) * FS / n_fft
    X = np.zeros((B, D, F, T), complex)
    for b in range(B):
        S = g.standard_normal((F, T)) + 1j * g.standard_normal((F, T))
        r = np.linalg.norm(cand[true[b]] - mics, axis=1)
        for d in range(D):
            noise = g.standard_normal((F, T)) + 1j * g.standard_normal((F, T))
            X[b, d] = S * np.exp(-1j * omega * r[d] / C)[:, None] / r[d] + snr * noise
    for a in (X, mics, cand, true):
        a.setflags(write=False)
    return Case(X, mics, cand, true)


def parity_case(shape):
    B, D, T, G, f_lo, f_hi, n_fft = shape
    return case(B, D, T, G, B + D + T + G, n_fft)


@functools.lru_cache(maxsize=None)
def reference(shape, single=False):
    """The float64 restatement of a parity shape, computed once: ``Reference(psi, map, best, status, gap)``; gap (B,) is the
    map's largest value less its runner-up (inf for G = 1).  single: of the input rounded to complex64 and promoted again."""
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c = parity_case(shape)
    X = c.X.astype(np.complex64).astype(np.complex128) if single else c.X
    psi, st = cross_spectra(X, f_lo, f_hi)
    S, best, status = srp_phat(psi, c.mics, c.cand, FS, n_fft, C, f_lo, f_hi, spectrum_status=st)
    top = np.sort(S, axis=1)[:, ::-1]
    gap = top[:, 0] - top[:, 1] if G > 1 else np.full(B, np.inf)
    for a in (psi, S, best, status, gap):
        a.setflags(write=False)
    return Reference(psi, S, best, status, gap)
