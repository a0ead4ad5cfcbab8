"""Float64 numpy restatement of the room-acoustic parameters of an impulse response (Schroeder's backward integration with
least-squares line fits, ISO 3382) -- TEST INFRASTRUCTURE ONLY.  The kernels are csrc/room_acoustics.hip; the definitions
are the comment on alvq_room_acoustics_* in include/alvq.h.

The tail energies are one reversed cumsum of the squares (sequential, so monotone), the onset is argmax |h| (first index; a
NaN counts as the largest value, numpy's rule), and each decay time is a centred least-squares fit.
"""
import collections

import numpy as np

RANGES = {"t30": (-5.0, -35.0), "t20": (-5.0, -25.0), "edt": (0.0, -10.0)}   # (hi, lo) dB
COLUMNS = ("t30", "t20", "edt", "c50", "c80", "d50", "drr")
BAD_ENERGY, SHORT_RANGE, NO_LATE_ENERGY = 1, 2, 4

Result = collections.namedtuple("Result", COLUMNS + ("onset", "status", "margin"))


def sample_counts(fs):
    """(k50, k80, kdirect): 50, 80 and 2.5 ms in samples, floor(ms * 1e-3 * fs + 0.5)."""
    return tuple(int(np.floor(ms * 1e-3 * fs + 0.5)) for ms in (50.0, 80.0, 2.5))


def tail_energy(h):
    """T[t] = sum_{s >= t} h[s]^2 for t in [0, n], with T[n] = 0."""
    h = np.asarray(h, dtype=np.float64)
    return np.concatenate((np.cumsum((h * h)[::-1])[::-1], [0.0]))


def edc_db(h):
    """10 log10(T(t) / T(0)): -inf where T(t) = 0, the whole row NaN when T(0) is 0 or not finite."""
    T = tail_energy(h)[:-1]
    if not (np.isfinite(T[0]) and T[0] > 0.0):
        return np.full(T.shape, np.nan)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(T / T[0])


def _decay_time(L, fs, hi, lo):
    """(-60 / slope of the least-squares line of L against k / fs over {k : lo <= L[k] <= hi}, margin in dB); NaN when the
    set holds fewer than two samples.  The margin is the smallest distance between a threshold and the L values on either
    side of each end of the set; hi = 0 is skipped (L[0] = 0 meets it exactly)."""
    member = (L >= lo) & (L <= hi)
    idx = np.nonzero(member)[0]
    margin = np.inf
    if idx.size:
        first, last = idx[0], idx[-1]
        finite = lambda v: abs(v) if np.isfinite(v) else np.inf   # noqa: E731
        if hi != 0.0:
            margin = min(margin, finite(L[first] - hi))
            if first > 0:
                margin = min(margin, finite(L[first - 1] - hi))
        margin = min(margin, finite(L[last] - lo))
        if last + 1 < L.size:
            margin = min(margin, finite(L[last + 1] - lo))
    else:                                    # an empty set: every L is on the far side of a threshold
        with np.errstate(invalid="ignore"):
            d = np.minimum(np.abs(L - lo), np.abs(L - hi) if hi != 0.0 else np.inf)
        d = d[np.isfinite(d)]
        margin = float(d.min()) if d.size else np.inf
    if idx.size < 2:
        return np.nan, margin
    x = idx.astype(np.float64) / fs
    y = L[idx]
    xc, yc = x - x.mean(), y - y.mean()
    return -60.0 / (np.dot(xc, yc) / np.dot(xc, xc)), margin


def parameters(h, fs=16000.0):
    """One response h (n,) -> Result(t30, t20, edt, c50, c80, d50, drr, onset, status, margin); margin is a dict by decay
    range."""
    h = np.asarray(h, dtype=np.float64)
    n = h.shape[0]
    k50, k80, kd = sample_counts(fs)
    a = np.abs(h)
    n0 = int(np.argmax(a))                   # first index of the maximum; the first NaN if there is one
    T = tail_energy(h)
    nan = {c: np.nan for c in COLUMNS}
    if not (np.isfinite(T[0]) and T[0] > 0.0):
        return Result(onset=n0, status=BAD_ENERGY, margin={k: np.inf for k in RANGES}, **nan)
    status = 0
    with np.errstate(divide="ignore"):
        L = 10.0 * np.log10(T[n0:n] / T[n0])
    out, margins = {}, {}
    for name, (hi, lo) in RANGES.items():
        out[name], margins[name] = _decay_time(L, fs, hi, lo)
        if np.isnan(out[name]):
            status |= SHORT_RANGE

    def clip(t):
        return min(max(t, 0), n)

    def ratio_db(early, late):
        nonlocal status
        if late == 0.0:
            status |= NO_LATE_ENERGY
            return np.inf
        return 10.0 * np.log10(early / late)

    for name, k in (("c50", k50), ("c80", k80)):
        out[name] = ratio_db(T[n0] - T[clip(n0 + k)], T[clip(n0 + k)])
    out["d50"] = (T[n0] - T[clip(n0 + k50)]) / T[n0]
    out["drr"] = ratio_db(T[clip(n0 - kd)] - T[clip(n0 + kd + 1)], T[clip(n0 + kd + 1)])
    return Result(onset=n0, status=status, margin=margins, **out)


def analytic_decay(T60, fs=16000.0, n=4096, seed=0):
    """h[t] = +-exp(-a t) with a = 3 ln10 / (T60 fs) (60 dB of energy decay in T60 seconds) and seeded random signs; the
    energy decay is exactly exponential, so t30 = t20 = edt = T60 up to the truncation at n."""
    a = 3.0 * np.log(10.0) / (T60 * fs)
    sign = np.where(np.random.default_rng(seed).random(n) < 0.5, -1.0, 1.0)
    return sign * np.exp(-a * np.arange(n, dtype=np.float64))


def analytic_c50(T60, fs=16000.0, n=4096):
    """The closed form of c50 for analytic_decay: squares are a geometric series of ratio r = exp(-2a), onset at 0."""
    a = 3.0 * np.log(10.0) / (T60 * fs)
    k50 = sample_counts(fs)[0]
    r = np.exp(-2.0 * a)
    return 10.0 * np.log10((1.0 - r ** k50) / (r ** k50 - r ** n))
