"""Plain high-precision restatements of the waveform front-end kernels (csrc/stft.hip, csrc/istft.hip): test infrastructure.

Every function here spells its operation out element by element in numpy -- explicit reflect indices, an explicit periodic
Hann window, a direct DFT whose twiddle angles are reduced exactly as 2 pi ((k n) mod N) / N -- and accumulates in
``np.longdouble`` (80-bit extended on x86), so its own rounding is far below the float64 bounds the GPU tests hold the kernels
to.  None of it calls torch.stft / torch.istft / scipy: tests/test_dsp_ref_cpu.py checks it against those independently.

Alongside each result the helpers return the scale the per-element error bounds are measured against (the sum of the absolute
values of the terms that make up that element), so a bound follows every element, however quiet, instead of the loudest
element of the batch.
"""
import functools

import numpy as np

LD = np.longdouble
PI = np.arccos(LD(-1))


def hann(n_fft):
    """Periodic Hann window w[n] = 0.5 - 0.5 cos(2 pi n / N), in extended precision."""
    n = np.arange(n_fft)
    return LD(0.5) - LD(0.5) * np.cos(2 * PI * n.astype(LD) / n_fft)


@functools.lru_cache(maxsize=16)
def _table(n_fft):
    """cos and sin of 2 pi m / N, m = 0 .. N-1 (read-only)."""
    ang = 2 * PI * np.arange(n_fft).astype(LD) / n_fft
    c, s = np.cos(ang), np.sin(ang)
    c.flags.writeable = s.flags.writeable = False
    return c, s


def _twiddle(k, n, n_fft):
    """cos and sin of 2 pi ((k n) mod N) / N for integer arrays k, n (outer product)."""
    c, s = _table(n_fft)
    m = np.multiply.outer(np.asarray(k), np.asarray(n)) % n_fft
    return c[m], s[m]


def reflect_index(t, n, S, n_fft, hop):
    """Sample index read by frame t at window position n: i = t*hop + n - N/2, mirrored as -i below 0 and 2(S-1)-i above S-1."""
    i = np.add.outer(np.asarray(t) * hop, np.asarray(n)) - n_fft // 2
    i = np.where(i < 0, -i, i)
    return np.where(i > S - 1, 2 * (S - 1) - i, i)


def n_frames(S, hop):
    return 1 + S // hop


def stft(x, n_fft, hop, frames=None):
    """Normalised one-sided STFT of x (..., S): center=True, reflect padding, periodic Hann, divided by sqrt(sum w^2).

    Returns (X, l1, l1x):
      X    (..., n_fft/2+1, len(frames)) complex (extended-precision real and imaginary parts, as complex256);
      l1   (..., len(frames)) = sum_n |x_i w_n| / sqrt(sum w^2), the scale of a frame's accumulated products;
      l1x  (..., len(frames)) = sum_n |x_i| / sqrt(sum w^2), the scale of an absolute error in the window values themselves.
    ``frames``: the frame indices to compute (default: all 1 + S // hop)."""
    x = np.asarray(x).astype(LD)
    S = x.shape[-1]
    if n_fft % 2 or S <= n_fft // 2:
        raise ValueError("stft: need even n_fft and S > n_fft/2 (n_fft=%d S=%d)" % (n_fft, S))
    t = np.arange(n_frames(S, hop)) if frames is None else np.asarray(frames)
    n = np.arange(n_fft)
    w = hann(n_fft)
    norm = np.sqrt(np.sum(w * w))
    fr = x[..., reflect_index(t, n, S, n_fft, hop)]                       # (..., T, N)
    fw = fr * w
    c, s = _twiddle(np.arange(n_fft // 2 + 1), n, n_fft)                   # (F, N)
    re = np.matmul(fw, c.T) / norm                                         # (..., T, F)
    im = -np.matmul(fw, s.T) / norm
    X = np.swapaxes(re + 1j * im, -1, -2)
    return X, np.sum(np.abs(fw), axis=-1) / norm, np.sum(np.abs(fr), axis=-1) / norm


def stft_of_impulse(p, S, n_fft, hop):
    """Closed form of ``stft`` for the unit impulse at sample p (0 <= p < S): (X, l1, l1x) as ``stft`` returns them, all frames.

    Frame t reads sample p at every window position n whose reflect-padded index lands on p: directly (t*hop + n - N/2 = p),
    through the left mirror (= -p, p > 0) and through the right one (= 2(S-1) - p, p < S-1).  Each such n contributes
    w[n] e^{-2 pi i k n / N} / sqrt(sum w^2)."""
    if not 0 <= p < S:
        raise ValueError("impulse position %d outside [0, %d)" % (p, S))
    T, F = n_frames(S, hop), n_fft // 2 + 1
    w = hann(n_fft)
    norm = np.sqrt(np.sum(w * w))
    images = [p] + ([-p] if p > 0 else []) + ([2 * (S - 1) - p] if p < S - 1 else [])
    X = np.zeros((F, T), dtype=np.clongdouble)
    l1 = np.zeros(T, dtype=LD)
    l1x = np.zeros(T, dtype=LD)
    k = np.arange(F)
    for t in range(T):
        for raw in images:
            n = raw - t * hop + n_fft // 2
            if 0 <= n < n_fft:
                c, s = _twiddle(k, np.array([n]), n_fft)
                X[:, t] += w[n] * (c[:, 0] - 1j * s[:, 0]) / norm
                l1[t] += w[n] / norm
                l1x[t] += 1 / norm
    return X, l1, l1x


def istft(spec, n_fft, hop, length=None):
    """Inverse of ``stft`` (torchaudio InverseSpectrogram, normalized=True): spec (..., n_fft/2+1, T) complex -> (..., length).

    Explicit irfft that ignores the imaginary parts at DC and Nyquist, multiplied by sqrt(sum w^2) (the input is normalised),
    windowed, overlap-added and divided by the overlap-added w^2 envelope; the first n_fft/2 samples are dropped (center=True)
    and output past the overlap-added signal is 0.  length defaults to hop*(T-1).

    Returns (y, terms, raw, wsum, env):
      terms (..., length) = sum over the frames covering the sample of w[n] * scale * sum_k |term_k| / env, the scale of the
            accumulated products (scale = sqrt(sum w^2) / N, term_k the k-th real term of the inverse DFT of sample n);
      raw   (..., length) = the same without the window factor: the scale of an absolute error in the window values;
      wsum  (length,) = sum over covering frames of w[n] / env (the envelope's sensitivity to its window values);
      env   (length,) = the overlap-added w^2 (0 past the signal)."""
    spec = np.asarray(spec)
    F, T = spec.shape[-2], spec.shape[-1]
    if F != n_fft // 2 + 1:
        raise ValueError("istft: %d bins for n_fft=%d" % (F, n_fft))
    length = hop * (T - 1) if length is None else length
    re, im = spec.real.astype(LD), spec.imag.astype(LD)
    n = np.arange(n_fft)
    w = hann(n_fft)
    scale = np.sqrt(np.sum(w * w)) / n_fft
    c, s = _twiddle(np.arange(1, F - 1), n, n_fft)                        # (F-2, N)
    sgn = np.where(n % 2 == 1, LD(-1), LD(1))
    # (..., T, N): the irfft of every frame, and the sum of |terms| that makes it up
    mid = 2 * (np.matmul(np.swapaxes(re[..., 1:F - 1, :], -1, -2), c) - np.matmul(np.swapaxes(im[..., 1:F - 1, :], -1, -2), s))
    x = re[..., 0, :, None] + sgn * re[..., F - 1, :, None] + mid
    mag = (np.abs(re[..., 0, :, None]) + np.abs(re[..., F - 1, :, None])
           + 2 * (np.matmul(np.swapaxes(np.abs(re[..., 1:F - 1, :]), -1, -2), np.abs(c))
                  + np.matmul(np.swapaxes(np.abs(im[..., 1:F - 1, :]), -1, -2), np.abs(s))))
    total = n_fft + hop * (T - 1)
    lead = spec.shape[:-2]
    acc = np.zeros(lead + (total,), dtype=LD)
    accm = np.zeros(lead + (total,), dtype=LD)
    accr = np.zeros(lead + (total,), dtype=LD)
    env = np.zeros(total, dtype=LD)
    wsum = np.zeros(total, dtype=LD)
    for t in range(T):
        sl = slice(t * hop, t * hop + n_fft)
        acc[..., sl] += x[..., t, :] * w * scale
        accm[..., sl] += mag[..., t, :] * w * scale
        accr[..., sl] += mag[..., t, :] * scale
        env[sl] += w * w
        wsum[sl] += w
    p = np.arange(n_fft // 2, n_fft // 2 + length)
    inside = p < total
    pc = np.where(inside, p, 0)
    e = np.where(inside, env[pc], LD(1))
    y = np.where(inside, acc[..., pc] / e, LD(0))
    terms = np.where(inside, accm[..., pc] / e, LD(0))
    raw = np.where(inside, accr[..., pc] / e, LD(0))
    return y, terms, raw, np.where(inside, wsum[pc] / e, LD(0)), np.where(inside, env[pc], LD(0))


def fir_same(wave, h):
    """scipy.signal.convolve(wave, h, mode="same") as the direct sum out[i] = sum_j h[j] * wave[i + (Nh-1)//2 - j] (zero outside
    [0, S)).  wave (..., S); h (Nh,) or (..., Nh) matching wave's leading dims.  Returns (out, mag) with
    mag[i] = sum_j |h[j] * wave[i + (Nh-1)//2 - j]|."""
    wave = np.asarray(wave).astype(LD)
    h = np.asarray(h).astype(LD)
    S, Nh = wave.shape[-1], h.shape[-1]
    off = (Nh - 1) // 2
    pad = np.zeros(wave.shape[:-1] + (S + 2 * Nh,), dtype=LD)
    pad[..., Nh:Nh + S] = wave                                           # pad[..., Nh + m] = wave[..., m]
    out = np.zeros(wave.shape, dtype=LD)
    mag = np.zeros(wave.shape, dtype=LD)
    for j in range(Nh):
        seg = pad[..., Nh + off - j:Nh + off - j + S]
        hj = h[..., j:j + 1]
        out += hj * seg
        mag += np.abs(hj * seg)
    return out, mag


def spec_rir_wiener(S, E):
    """The dataset generator's spectrogram arithmetic (the comment above spec_stats_kernel in csrc/stft.hip) on S (B, F, T)
    complex64 and E (B, F, T) complex128, with max |r| taken per batch item:
      r = S / (E + 1e-8);  rir = |r / max_item |r||^2;  wiener[b, f] = |sum_t E conj(S) / (sum_t |S|^2 + 1e-8)|^2;
      speech = |S|^2;  echoed = |E|^2.
    Returns (speech, echoed, rir, wiener, wiener_scale) in extended precision, where
    wiener_scale[b, f] = (sum_t |E||S| / (sum_t |S|^2 + 1e-8))^2 is a scale of wiener that does not shrink when the
    numerator cancels."""
    S = np.asarray(S).astype(np.clongdouble)
    E = np.asarray(E).astype(np.clongdouble)
    speech = S.real ** 2 + S.imag ** 2
    echoed = E.real ** 2 + E.imag ** 2
    d = E + LD(1e-8)
    r = S / d
    ra = np.abs(r)
    g = ra.reshape(ra.shape[0], -1).max(axis=1)[:, None, None]
    rir = (ra / g) ** 2
    den = np.sum(speech, axis=-1) + LD(1e-8)
    num = np.sum(E * np.conj(S), axis=-1)
    wiener = np.abs(num / den) ** 2
    wscale = (np.sum(np.abs(E) * np.abs(S), axis=-1) / den) ** 2
    return speech, echoed, rir, wiener, wscale


# ------------------------------------------------------------------------------------------------------------ case grids
# Shared by tests/test_dsp_edges_gpu.py (kernel vs helper) and tests/test_dsp_ref_cpu.py (helper vs torch / scipy), so the
# helpers are cross-checked on exactly the shapes the kernels are held to.

STFT_NFFT = (4, 6, 62, 256, 400, 510, 512, 1024, 2048)       # 2048: float32 only (the float64 limit is 1024)
STFT_F64_MAX = 1024


def stft_hops(n_fft):
    return sorted({1, 3, n_fft // 2, n_fft - 1, n_fft, n_fft + 7})


def stft_lengths(n_fft, hop, seed):
    """Signal lengths for one (n_fft, hop): the smallest legal S = n_fft/2+1 (frames reflect at both ends), S = hop-1 (T = 1)
    when legal, a multiple of hop, and two lengths with T = 1 + S // hop in the residues mod 8 picked by ``seed`` (the kernels
    tile 8 frames per workgroup; the caller cycles seed over the hops of one n_fft so every residue occurs)."""
    rng = np.random.default_rng(seed)
    smin = n_fft // 2 + 1
    out = [smin]
    if hop - 1 >= smin:
        out.append(hop - 1)
    out.append(hop * max(1, -(-smin // hop)))
    tmin = n_frames(smin, hop)
    for r in (2 * seed % 8, (2 * seed + 1) % 8):
        T = tmin + (r - tmin) % 8
        S = hop * (T - 1) + int(rng.integers(0, hop))
        while S < smin:
            T += 8
            S = hop * (T - 1) + int(rng.integers(0, hop))
        out.append(S)
    return sorted(set(out))


def stft_cases():
    """[(n_fft, hop, [S, ...])]: every n_fft with every hop of ``stft_hops``."""
    return [(n, h, stft_lengths(n, h, j)) for n in STFT_NFFT for j, h in enumerate(stft_hops(n))]


def check_frames(T, seed, keep=24):
    """The frames a reference is computed on: all of them up to ``keep``, else the first and last 8 (whole 8-frame tiles at
    both ends, the reflected frames among them) and 8 seeded ones in between."""
    if T <= keep:
        return np.arange(T)
    rng = np.random.default_rng(seed)
    mid = rng.choice(np.arange(8, T - 8), size=keep - 16, replace=False)
    return np.sort(np.concatenate([np.arange(8), mid, np.arange(T - 8, T)]))


def stft_signal(B, S, seed):
    """(B, S) float32 test signals: item 0 white noise, item 1 a tone over the middle half on a 1e-6 noise floor (the first
    and last frames see only the floor), item 2 white noise at 1e3."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, S))
    i = np.arange(S)
    if B > 1:
        tone = np.sin(2 * np.pi * 0.0123 * i + 0.3) * ((i >= S // 4) & (i < 3 * S // 4))
        x[1] = tone + 1e-6 * x[1]
    if B > 2:
        x[2] *= 1e3
    return x.astype(np.float32)


def impulse_positions(S, n_fft):
    return sorted({0, 1, n_fft // 2 - 1, n_fft // 2, S - 1 - n_fft // 2, S - 2, S - 1} & set(range(S)))


FIR_CASES = [(S, Nh) for S in (1, 2, 1023, 1024, 1025, 4097) for Nh in sorted({1, 2, 255, 256, 257, 511, 512, 513, S}) if Nh <= S]

RIR_CASES = [(F, T) for F in (1, 3, 201, 513) for T in (1, 255, 256, 257, 700)]

ISTFT_NFFT = (4, 64, 512, 1024, 2048)                        # 2048: float32 only
ISTFT_T = (1, 2, 7, 8, 9, 17)


def istft_hops(n_fft):
    """Hops that satisfy NOLA (hop < n_fft): 1, a hop that does not divide n_fft, and n_fft/4 (or 1 at n_fft = 4)."""
    return sorted({1, max(1, n_fft // 4), n_fft // 2 - 1 if n_fft > 4 else 3})


def istft_lengths(n_fft, hop, T):
    """Output lengths shorter than, equal to and longer than hop*(T-1) (>= 1): base + 3 stays inside the overlap-added
    signal, base + n_fft/2 + 3 runs 3 samples past it (those are 0)."""
    base = hop * (T - 1)
    return sorted({max(1, base - 3), base, base + 3, base + n_fft // 2 + 3} - {0})


def istft_env_ok(n_fft, hop, T, length, floor=1e-6):
    """True when the overlap-added w^2 is >= floor over the output samples the overlap-added signal covers (below that the
    inversion itself is ill-conditioned, and the host NOLA check rejects what falls under 1e-11)."""
    w = hann(n_fft).astype(np.float64)
    total = n_fft + hop * (T - 1)
    env = np.zeros(total)
    for t in range(T):
        env[t * hop:t * hop + n_fft] += w * w
    p = np.arange(n_fft // 2, min(n_fft // 2 + length, total))
    return bool(p.size == 0 or env[p].min() >= floor)
