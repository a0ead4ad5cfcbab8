"""The argument rules the signal and array modules share: plain functions that raise, each with one wording.  A rule lives
here when two call sites raise the same exception with the same text at the same place among their other checks; a module
whose wording differs keeps its own (DESIGN.md lists them).  ``who`` is the public function the message names.  Nothing here
imports the package.
"""
import math

import numpy as np
import torch

MAX_MICROPHONES = 8
MAX_FRAMES = 65535               # T: a grid dimension of the array kernels
MAX_BATCH = 65535                # B: likewise
MAX_BINS = 2 ** 31 - 1           # B F: the kernels index (item, bin) in an int


def int_in(who, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or v > hi:
        raise ValueError("%s: %s must be an integer in [%d, %d], got %r" % (who, name, lo, hi, v))


def positive(who, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v > 0):
        raise ValueError("%s: %s must be a finite number > 0, got %r" % (who, name, v))


def nonneg(who, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v >= 0):
        raise ValueError("%s: %s must be a finite number >= 0, got %r" % (who, name, v))


def on_gpu(who, t, name):
    if not t.is_cuda:
        raise RuntimeError("%s: %s must live on the GPU (got %s); the HIP path has no CPU fallback" % (who, name, t.device))


def all_on_gpu(who, **tensors):
    """``on_gpu`` of every named tensor in the order given; an argument that is None is not there."""
    for name, t in tensors.items():
        if t is not None:
            on_gpu(who, t, name)


def bins(who, what, B, F):
    if B < 1 or B > MAX_BATCH or F < 1 or B * F > MAX_BINS:
        raise ValueError("%s: need 1 <= B <= 65535, F >= 1 and B F <= 2^31 - 1, got %s" % (who, what))


def frames(who, dims, shape):
    """The kernels' limits on B, F and T of dims = (B, D, F, T); ``shape`` is what the caller was given."""
    B, _, F, T = dims
    if B < 1 or B > MAX_BATCH or F < 1 or B * F > MAX_BINS or T < 1 or T > MAX_FRAMES:
        raise ValueError("%s: need 1 <= B <= 65535, F >= 1, B F <= 2^31 - 1 and 1 <= T <= 65535, got shape %s" % (who, tuple(shape)))


def microphones(who, D, min_d=1):
    if D < min_d or D > MAX_MICROPHONES:
        raise ValueError("%s: need %d <= D <= 8 microphones, got D = %d" % (who, min_d, D))


def n_fft_bins(who, n_fft, F):
    int_in(who, "n_fft", n_fft, 2, 2 ** 24)
    if F != n_fft // 2 + 1:
        raise ValueError("%s: %d frequency bins, n_fft=%d has %d" % (who, F, n_fft, n_fft // 2 + 1))


def spec4(who, spec, min_d=1, n_fft=None):
    """spec, complex (D, F, T) or (B, D, F, T) with min_d <= D <= 8, as (B, D, F, T); whether it came with a batch dimension.
    With n_fft: F must be n_fft / 2 + 1."""
    if not isinstance(spec, torch.Tensor) or spec.dim() not in (3, 4):
        raise ValueError("%s: spec must be a (D, F, T) or (B, D, F, T) tensor" % who)
    if spec.dtype not in (torch.complex64, torch.complex128):
        raise ValueError("%s: spec must be complex64 or complex128, got %s" % (who, spec.dtype))
    x = spec[None] if spec.dim() == 3 else spec
    frames(who, x.shape, spec.shape)
    microphones(who, x.shape[1], min_d)
    if n_fft is not None:
        n_fft_bins(who, n_fft, x.shape[2])
    return x, spec.dim() == 4


def waves3(who, waves):
    if not isinstance(waves, torch.Tensor) or waves.dim() != 3:
        raise ValueError("%s: waves must be a (B, D, S) tensor" % who)
    if waves.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: waves must be float32 or float64, got %s" % (who, waves.dtype))


def stft_dims(who, waves, n_fft, hop):
    """(B, D, F, T) of the spectrograms of waves (B, D, S), within the kernels' limits."""
    B, D, S = waves.shape
    if B < 1 or B > MAX_BATCH or D < 1 or D > MAX_MICROPHONES or S < 1:
        raise ValueError("%s: need 1 <= B <= 65535, 1 <= D <= 8 and S >= 1, got shape %s" % (who, tuple(waves.shape)))
    int_in(who, "n_fft", n_fft, 2, 2 ** 24)
    int_in(who, "hop", hop, 1, n_fft)
    F, T = n_fft // 2 + 1, 1 + S // hop
    if T > MAX_FRAMES or B * F > MAX_BINS:
        raise ValueError("%s: need B F <= 2^31 - 1 and T = 1 + S / hop <= 65535, got F = %d, T = %d" % (who, F, T))
    return B, D, F, T


def rows(who, name, x, min_n=2, max_b=None):
    """x, float32 or float64 (n,) or (B, n), as a contiguous (B, n) tensor; whether it came as (n,).  max_b: the cap on B,
    where the kernel has one.  The device is the caller's to check."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("%s: %s must be an (n,) or (B, n) tensor" % (who, name))
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: %s must be float32 or float64, got %s" % (who, name, x.dtype))
    single = x.dim() == 1
    r = x.unsqueeze(0) if single else x
    if r.shape[0] < 1 or (max_b is not None and r.shape[0] > max_b) or r.shape[1] < min_n or r.shape[1] > 1 << 24:
        raise ValueError("%s: need %s and %d <= n <= 2^24, got shape %s"
                         % (who, "B >= 1" if max_b is None else "1 <= B <= %d" % max_b, min_n, tuple(x.shape)))
    return r.contiguous(), single


def positions(who, name, t, B, count=None):
    """t: float64 positions (n, 3) for every item, or (B, n, 3); n >= 1, or ``count`` where it is given."""
    if not isinstance(t, torch.Tensor) or t.dim() not in (2, 3) or t.shape[-1] != 3 or t.dtype != torch.float64:
        raise ValueError("%s: %s must be a float64 (n, 3) or (B, n, 3) tensor" % (who, name))
    if t.dim() == 3 and t.shape[0] != B:
        raise ValueError("%s: %s holds %d items, spec %d" % (who, name, t.shape[0], B))
    if t.shape[-2] < 1 or (count is not None and t.shape[-2] != count):
        raise ValueError("%s: %s must hold %s positions, got %d" % (who, name, count if count is not None else ">= 1", t.shape[-2]))


def unbatch(out, batched):
    """What a function returns: ``out`` for a batched call; for one without a batch dimension item 0 of the tensor, or of
    every field of the named tuple."""
    if batched:
        return out
    return out[0] if isinstance(out, torch.Tensor) else type(out)(*(t[0] for t in out))
