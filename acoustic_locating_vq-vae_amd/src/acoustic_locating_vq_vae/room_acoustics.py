"""What reverberation an impulse response has, measured on the device (csrc/room_acoustics.hip): Schroeder's backward
integration and least-squares line fits to the decay curve (ISO 3382), float64, one launch, no host sync.

    from acoustic_locating_vq_vae.room_acoustics import room_acoustic_parameters, reverberation_time, energy_decay_curve
    h = scene_impulse_responses(scenes.source, scenes.receiver, scenes.room, scenes.reverberation_time, nsample=6400)
    p = room_acoustic_parameters(h)              # RoomAcoustics of (B,) device tensors
    p.t30, p.edt, p.c50, p.drr                   # what the rooms do, next to scenes.reverberation_time, what was asked for

Definitions (in full: include/alvq.h): the onset n0 is the first index of max |h|; with E(a, b) the energy of the samples
a <= t < b, the decay level is L(t) = 10 log10(E(t, n) / E(n0, n)); t30, t20 and edt are -60 / slope of the least-squares
line of L against time over -5..-35, -5..-25 and 0..-10 dB; c50 / c80 are the early-to-late energy ratios at 50 / 80 ms after
the onset in dB, d50 the early share of the energy, drr the energy within 2.5 ms of the onset over what follows, in dB.
There is no octave-band filtering and no noise-floor compensation: a response that ends in a noise floor wants truncating
first.  ``status`` (int32 per row) is 0, or bit 1 = zero or non-finite energy (every value NaN), bit 2 = a decay range with
fewer than two samples (that value NaN), bit 4 = no late energy (that ratio +inf).  Nothing here reads it: the caller does,
when it can sync.
"""
import collections
import math

from . import _native as N
from . import _rules as rules

RoomAcoustics = collections.namedtuple("RoomAcoustics", "t30 t20 edt c50 c80 d50 drr onset status")


def sample_counts(fs):
    """(k50, k80, kdirect): 50, 80 and 2.5 ms in samples at rate fs, floor(ms * 1e-3 * fs + 0.5)."""
    return tuple(int(math.floor(ms * 1e-3 * fs + 0.5)) for ms in (50.0, 80.0, 2.5))


def _rows(h, who):
    """h as a contiguous (B, n) tensor on the GPU, and whether it came with a batch dimension."""
    rows, single = rules.rows(who, "h", h)
    rules.on_gpu(who, h, "h")
    return rows, not single


def _rate(fs, who):
    if isinstance(fs, bool) or not isinstance(fs, (int, float)) or not (math.isfinite(fs) and fs > 0):
        raise ValueError("%s: fs must be a positive number, got %r" % (who, fs))
    return float(fs)


def energy_decay_curve(h):
    """Schroeder's energy decay curve 10 log10(sum_{s >= t} h[s]^2 / sum_s h[s]^2) in dB: h (B, n) or (n,), float32 or
    float64 on the GPU -> float64 of the same shape.  -inf where nothing follows; a row of zero or non-finite energy is NaN."""
    rows, batched = _rows(h, "energy_decay_curve")
    return rules.unbatch(N.edc(rows), batched)


def room_acoustic_parameters(h, fs=16000):
    """h (B, n) or (n,), float32 or float64 on the GPU (``rir_generate``'s (nsample, M) layout through ``.t()``) ->
    ``RoomAcoustics(t30, t20, edt, c50, c80, d50, drr, onset, status)`` of (B,) device tensors (0-d for an (n,) input): float64
    but onset and status, int32.  Times in s, ratios in dB.  The arithmetic is float64 for either input type."""
    fs = _rate(fs, "room_acoustic_parameters")
    rows, batched = _rows(h, "room_acoustic_parameters")
    out, onset, status = N.room_acoustics(rows, fs, *sample_counts(fs))
    return rules.unbatch(RoomAcoustics(*out.unbind(1), onset, status), batched)


def reverberation_time(h, fs=16000, method="t30"):
    """One decay time of ``room_acoustic_parameters``: method "t30", "t20" or "edt"."""
    if method not in ("t30", "t20", "edt"):
        raise ValueError("reverberation_time: method must be 't30', 't20' or 'edt', got %r" % (method,))
    return getattr(room_acoustic_parameters(h, fs), method)
