"""Float64 numpy restatement of the image-source room impulse response (Allen & Berkley 1979, as Habets' RIR generator states
it; what ``rir_generator.generate`` computes for an omnidirectional receiver) -- TEST INFRASTRUCTURE ONLY.

Every tap is evaluated directly (one cos and one sin per tap), vectorised over the images; the kernel (csrc/rir.hip) computes
the same sum with per-image rotations instead.  rir_generator itself is absent here, so parity with it is unpinned: the pins are
the closed-form direct path, reciprocity, scipy's lfilter and this restatement.
"""
import numpy as np


def sabine_beta(L, c, reverberation_time):
    """The six reflection coefficients from Sabine's formula, +sqrt(1 - alpha) (rir_generator's keyword reverberation_time)."""
    L = np.asarray(L, dtype=np.float64)
    V = np.prod(L)
    S = 2.0 * (L[0] * L[2] + L[1] * L[2] + L[0] * L[1])
    alpha = 24.0 * V * np.log(10.0) / (c * S * reverberation_time)
    if alpha > 1:
        raise ValueError("reflection coefficients cannot be computed for this room and reverberation time")
    return np.full(6, np.sqrt(1.0 - alpha))


def window_length(fs):
    return 2 * int(np.floor(0.004 * fs + 0.5))


def images(c, fs, r, s, L, beta, nsample, order=-1, dim=3):
    """(d in samples, gain) of every image whose floor(d) < nsample, in enumeration order (m_x, q, m_y, j, m_z, k)."""
    beta = np.array(beta, dtype=np.float64)
    if dim == 2:
        beta[4] = beta[5] = 0.0
    cTs = c / fs
    s = np.asarray(s, dtype=np.float64) / cTs
    r = np.asarray(r, dtype=np.float64) / cTs
    Ls = np.asarray(L, dtype=np.float64) / cTs
    n = [int(np.ceil(nsample / (2.0 * Ls[a]))) for a in range(3)]
    m = [np.arange(-n[a], n[a] + 1) for a in range(3)]
    mx, q, my, j, mz, k = [g.ravel() for g in np.meshgrid(m[0], [0, 1], m[1], [0, 1], m[2], [0, 1], indexing="ij")]
    keep = np.ones(mx.shape, dtype=bool) if order == -1 else \
        (np.abs(2 * mx - q) + np.abs(2 * my - j) + np.abs(2 * mz - k) <= order)
    mx, q, my, j, mz, k = (v[keep] for v in (mx, q, my, j, mz, k))
    x = (1 - 2 * q) * s[0] - r[0] + 2 * mx * Ls[0]
    y = (1 - 2 * j) * s[1] - r[1] + 2 * my * Ls[1]
    z = (1 - 2 * k) * s[2] - r[2] + 2 * mz * Ls[2]
    d = np.sqrt(x * x + y * y + z * z)
    refl = (np.power(beta[0], np.abs(mx - q)) * np.power(beta[1], np.abs(mx)) * np.power(beta[2], np.abs(my - j)) *
            np.power(beta[3], np.abs(my)) * np.power(beta[4], np.abs(mz - k)) * np.power(beta[5], np.abs(mz)))
    inside = np.floor(d) < nsample
    d, refl = d[inside], refl[inside]
    return d, refl / (4.0 * np.pi * d * cTs)


def highpass(h, fs):
    """The generator's 100 Hz high-pass, as its recurrence: y0 = B1 y1 + B2 y2 + x;  h = y0 + A1 y1 + R1 y2."""
    W = 2.0 * np.pi * 100.0 / fs
    R1 = np.exp(-W)
    B1, B2, A1 = 2.0 * R1 * np.cos(W), -R1 * R1, -(1.0 + R1)
    out = np.empty_like(h)
    y1 = y2 = 0.0
    for i, x in enumerate(h):
        y0 = B1 * y1 + B2 * y2 + x
        out[i] = y0 + A1 * y1 + R1 * y2
        y2, y1 = y1, y0
    return out


def highpass_coefficients(fs):
    """(b, a) of the same filter for scipy.signal.lfilter."""
    W = 2.0 * np.pi * 100.0 / fs
    R1 = np.exp(-W)
    B1, B2, A1 = 2.0 * R1 * np.cos(W), -R1 * R1, -(1.0 + R1)
    return np.array([1.0, A1, R1]), np.array([1.0, -B1, -B2])


def rir(c, fs, r, s, L, beta, nsample, order=-1, dim=3, hp_filter=True, chunk=1 << 14):
    """One response (nsample,) float64: every tap of every image evaluated directly."""
    d, gain = images(c, fs, r, s, L, beta, nsample, order, dim)
    Tw = window_length(fs)
    h = np.zeros(nsample)
    taps = np.arange(Tw)
    for i in range(0, d.size, chunk):
        dd, gg = d[i:i + chunk, None], gain[i:i + chunk, None]
        t = np.floor(dd).astype(np.int64) - Tw // 2 + 1 + taps
        u = t - dd
        v = gg * 0.5 * (1.0 + np.cos(2.0 * np.pi * u / Tw)) * np.sinc(u)
        ok = (t >= 0) & (t < nsample)
        h += np.bincount(t[ok], weights=v[ok], minlength=nsample)
    return highpass(h, fs) if hp_filter else h


def direct_path(c, fs, r, s, nsample):
    """Closed form of the beta = 0, unfiltered response: only the direct path, w(t-d) sinc(pi (t-d)) / (4 pi |s-r|)."""
    dist = float(np.linalg.norm(np.asarray(s, dtype=np.float64) - np.asarray(r, dtype=np.float64)))
    d = dist * fs / c
    Tw = window_length(fs)
    t = np.arange(nsample)
    u = t - d
    h = 0.5 * (1.0 + np.cos(2.0 * np.pi * u / Tw)) * np.sinc(u) / (4.0 * np.pi * dist)
    h[np.abs(t - (np.floor(d) + 0.5)) > Tw / 2] = 0.0          # only the Tw taps floor(d) - Tw/2 + 1 ... floor(d) + Tw/2
    return h


# ------------------------------------------------------------------------------------------------------- longdouble twins
def ld_pi():
    """pi in np.longdouble (np.pi is a float64)."""
    return 4 * np.arctan(np.longdouble(1))


def highpass_ld(h, fs):
    """``highpass`` with its coefficients and its recurrence in np.longdouble; the input is taken as it is."""
    LD = np.longdouble
    W = 2 * ld_pi() * 100 / LD(fs)
    R1 = np.exp(-W)
    B1, B2, A1 = 2 * R1 * np.cos(W), -R1 * R1, -(1 + R1)
    out = np.empty(len(h), dtype=LD)
    y1 = y2 = LD(0)
    for i, x in enumerate(np.asarray(h).astype(LD)):
        y0 = B1 * y1 + B2 * y2 + x
        out[i] = y0 + A1 * y1 + R1 * y2
        y2, y1 = y1, y0
    return out


def rir_ld(c, fs, r, s, L, beta, nsample, order=-1, dim=3, hp_filter=True, chunk=1 << 12):
    """``rir`` with every tap and every sum in np.longdouble, (nsample,): ``images``' own float64 (d, gain) in their order are
    the twin's exact input (frac = d - floor(d) is exact), so the distance between the two is the rounding of ``rir``'s
    per-tap arithmetic and of its sums.  sin(pi u) of the tap u = m - frac is taken as -(-1)^m sin(pi frac) with the
    longdouble pi (np.sinc's pi is a float64), and sin(pi frac) from the smaller of frac and 1 - frac."""
    LD = np.longdouble
    d, gain = images(c, fs, r, s, L, beta, nsample, order, dim)
    fd = np.floor(d).astype(np.int64)
    frac, gain = (d - fd).astype(LD), gain.astype(LD)
    Tw = window_length(fs)
    pi = ld_pi()
    h = np.zeros(nsample, dtype=LD)
    m = np.arange(Tw) - Tw // 2 + 1
    sign = np.where(m % 2 == 0, -1, 1).astype(LD)             # sin(pi (m - frac)) = -(-1)^m sin(pi frac)
    for i in range(0, fd.size, chunk):
        ff, gg = frac[i:i + chunk, None], gain[i:i + chunk, None]
        t = fd[i:i + chunk, None] + m
        u = m.astype(LD) - ff
        zero = u == 0
        sf = np.sin(pi * np.where(ff > 0.5, 1 - ff, ff))      # sin(pi frac) = sin(pi (1 - frac)): no digits lost next to 1
        sinc = np.where(zero, LD(1), sign * sf / (pi * np.where(zero, LD(1), u)))
        v = gg * (LD(0.5) * (1 + np.cos(2 * pi * u / Tw))) * sinc
        ok = (t >= 0) & (t < nsample)
        np.add.at(h, t[ok], v[ok])
    return highpass_ld(h, fs) if hp_filter else h
