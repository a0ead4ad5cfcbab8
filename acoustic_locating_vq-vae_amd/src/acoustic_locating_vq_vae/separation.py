"""The baseline a learned separator or mask estimator is measured against, on the device (csrc/iva.hip): AuxIVA, auxiliary-function
independent vector analysis with iterative projection (Ono, WASPAA 2011).  ``localization.music`` says there are two talkers and
where; this gives the two talkers.  It is blind (no geometry, no masks), has no frequency permutation problem (the source model
ties all bins of a source together), starts from W = I and is deterministic.  Its output keeps its phase, so ``front_end.istft``,
``speech_metrics.si_sdr`` and ``stoi`` apply directly, and its ratio masks are what ``beamforming.mvdr`` and ``gev`` take.
Float64 arithmetic, fixed-order sums, no host sync.

    from acoustic_locating_vq_vae import front_end as FE, beamforming as BF, separation as SEP
    spec = FE.array_spectrograms(wave, h)                         # (B, D, F, T): D microphones, here K = D sources
    sep = SEP.auxiva(spec, iterations=20)                         # IVA(spec (B, D, F, T), w (B, F, D, D), status (B, F))
    FE.istft(sep.spec[:, k], length=S)                            # source k as microphone ref heard it
    m = SEP.masks(sep.spec)                                       # (B, K, F, T) float64, summing to 1 over k
    BF.mvdr(spec, noise_mask=1 - m[:, k], speech_mask=m[:, k])    # ... or BF.gev: the mask-driven beamformers' baseline
    SEP.auxiva(spec, 10, w0=sep.w)                                # ten more iterations: w is the only state
    SEP.separate_waves(waves)                                     # (B, D, S) waveforms in, (B, D, S) out

Definitions (in full: include/alvq.h).  The input is X[b, d, f, t], 1 <= D <= 8, 1 <= T <= 65535, B <= 65535, B F <= 2^31 - 1.
The state is W[b, f], a D x D complex128 demixing matrix per bin; row k extracts source k: y_k[t] = sum_d W[k, d] x_d[t], d
rising, the sum starting from the first product.  Start: W = I, or ``w0``.  Before the first iteration a bin that holds a
non-finite value or nothing but zeros gets status 1: it keeps W = I and Y = X bit for bit and contributes nothing to p.
One iteration: (1) p[b, k, t] = sum_f |y_k[f, t]|^2 over the item's bins whose status is not 1, f rising; r = sqrt(p).
(2) phi[k, t] = 1 / max(r, eps max_t r) ("laplace") or F / max(p, eps max_t p) ("gauss", time-varying Gaussian); phi = 1 for a
source whose max_t is 0 or not finite.  (3) For each bin of status 0, for k = 0 .. D - 1 in this order, row k replaced before row
k + 1 is computed: V_k = (1 / T) sum_t phi[k, t] x_t x_t^H, exactly Hermitian; solve (W V_k) w = e_k by Gaussian elimination with
partial pivoting (the pivot of the largest |z|^2, ties to the lowest row); w <- w / sqrt(Re(w^H V_k w)); W[k, :] <- conj(w).  A
pivot that is 0 or not finite, or a Re(w^H V_k w) that is <= 0 or not finite, gives the bin status 2: it goes back to W = I, is
not updated again and goes on contributing y = x to p.  After ``iterations`` iterations the sources are projected back onto
microphone ``ref`` (the minimal distortion principle): A = W^-1 by the same elimination (a singular W: status 2, W = I, Y = X) and
Y[b, k, f, t] = A[ref, k] y_k[f, t], the image of source k at microphone ref, in the input's dtype.  Ratio masks:
M[b, k, f, t] = |Y_k|^2 / sum_j |Y_j|^2 in float64, j rising; 1 / K where the sum is 0 and 0 where it is not finite.
Nothing here reads a status: the caller does, when it can sync.

AuxIVA is a determined method: exactly D sources for D microphones and no class for diffuse noise.  For one or two talkers on a
larger array the classical mask estimator is cACGMM spatial clustering (csrc/cacgmm.hip), K classes on D microphones:

    init = SEP.time_masks(B, K, F, T, generator=g)                # (B, K, F, T) float64, constant over frequency
    r = SEP.cacgmm(spec, init, iterations=20)                     # CACGMM(masks, prior, cov, quadratic, status)
    BF.gev(spec, 1 - r.masks[:, k], r.masks[:, k])                # class k against the rest
    SEP.cacgmm(spec, r.masks, 10, quadratic0=r.quadratic)         # ten more iterations, bit for bit

Its definitions are ``cacgmm``'s docstring and, in full, include/alvq.h.
"""
import collections

import torch

from . import _native as N
from .beamforming import MAX_FRAMES, MAX_MICROPHONES, _spec4
from .dereverberation import _nonneg
from .front_end import HOP, N_FFT
from .localization import _int_in, _on_gpu

IVA = collections.namedtuple("IVA", "spec w status")
CACGMM = collections.namedtuple("CACGMM", "masks prior cov quadratic status")

MAX_ITERATIONS = 256
MODELS = {"laplace": N.IVA_LAPLACE, "gauss": N.IVA_GAUSS}
MAX_CLASSES = 8


def _iva_rules(who, D, iterations, model, ref, eps):
    """The rules of the keywords for D microphones; ValueErrors only."""
    _int_in(who, "iterations", iterations, 0, MAX_ITERATIONS)
    if not isinstance(model, str) or model not in MODELS:
        raise ValueError("%s: model must be one of 'laplace', 'gauss', got %r" % (who, model))
    _int_in(who, "ref", ref, 0, D - 1)
    _nonneg(who, "eps", eps)


def auxiva(spec, iterations=20, model="laplace", ref=0, eps=1e-10, w0=None):
    """AuxIVA of an array's spectrograms: spec (D, F, T) or (B, D, F, T), complex64 or complex128 on the GPU, and w0 None or a
    complex128 (F, D, D) / (B, F, D, D) start -> ``IVA(spec, w, status)``: the D separated spectrograms as microphone ``ref``
    heard them, of spec's shape and dtype, the demixing matrices w (B, F, D, D) complex128 and status (B, F) int32 (no B for a
    (D, F, T) spec).  ``auxiva(X, a + b).w`` equals ``auxiva(X, b, w0=auxiva(X, a).w).w`` bit for bit."""
    who = "auxiva"
    x, batched = _spec4(who, spec)
    B, D, F, T = x.shape
    _iva_rules(who, D, iterations, model, ref, eps)
    if w0 is not None:
        want = (B, F, D, D) if batched else (F, D, D)
        if not isinstance(w0, torch.Tensor) or w0.dtype != torch.complex128 or tuple(w0.shape) != want:
            raise ValueError("%s: w0 must be a complex128 %s tensor for spec %s" % (who, want, tuple(spec.shape)))
        w0 = w0 if batched else w0[None]
    _on_gpu(who, x, "spec")
    if w0 is not None:
        _on_gpu(who, w0, "w0")
    out = IVA(*N.auxiva(x, int(iterations), MODELS[model], int(ref), float(eps), w0))
    return out if batched else IVA(*(t[0] for t in out))


def masks(sep_spec):
    """Ratio masks of separated spectrograms: sep_spec (K, F, T) or (B, K, F, T), complex64 or complex128 on the GPU, K <= 8 ->
    float64 of the same shape, M[:, k] = |Y_k|^2 / sum_j |Y_j|^2.  ``M[:, k]`` and ``1 - M[:, k]`` are the speech and noise
    masks of ``beamforming.mvdr`` and ``gev`` for source k."""
    who = "masks"
    y, batched = _spec4(who, sep_spec)
    _on_gpu(who, y, "sep_spec")
    m = N.separation_masks(y)
    return m if batched else m[0]


def separate_waves(waves, iterations=20, model="laplace", ref=0, n_fft=N_FFT, hop=HOP):
    """Waveforms in, waveforms out: waves (B, D, S), float32 or float64 on the GPU -> (B, D, S) of the same dtype, row k
    ``front_end.istft`` of source k of ``auxiva`` on spec = ``N.stft_complex`` of the B D rows, which has F = n_fft / 2 + 1 bins
    and T = 1 + S / hop frames, as ``beamforming.beamform_waves`` goes."""
    who = "separate_waves"
    if not isinstance(waves, torch.Tensor) or waves.dim() != 3:
        raise ValueError("%s: waves must be a (B, D, S) tensor" % who)
    if waves.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: waves must be float32 or float64, got %s" % (who, waves.dtype))
    B, D, S = waves.shape
    if B < 1 or B > 65535 or D < 1 or D > MAX_MICROPHONES or S < 1:
        raise ValueError("%s: need 1 <= B <= 65535, 1 <= D <= 8 and S >= 1, got shape %s" % (who, tuple(waves.shape)))
    _int_in(who, "n_fft", n_fft, 2, 2 ** 24)
    _int_in(who, "hop", hop, 1, n_fft)
    F, T = n_fft // 2 + 1, 1 + S // hop
    if T > MAX_FRAMES or B * F > 2 ** 31 - 1:
        raise ValueError("%s: need B F <= 2^31 - 1 and T = 1 + S / hop <= 65535, got F = %d, T = %d" % (who, F, T))
    _iva_rules(who, D, iterations, model, ref, 0.0)
    _on_gpu(who, waves, "waves")
    spec = N.stft_complex(waves.reshape(B * D, S).contiguous(), n_fft, hop).view(B, D, F, T)
    sep = auxiva(spec, iterations, model, ref)
    return N.istft(sep.spec.reshape(B * D, F, T), n_fft, hop, S).view(B, D, S)


def _class_array(who, name, a, B, F, T, batched, K=None):
    """a as float64 (B, K, F, T) for a spectrogram of (B, D, F, T): (K, F, T) without the batch, and F may be 1 (every bin the
    same), which is expanded here."""
    lead = (B,) if batched else ()
    if not isinstance(a, torch.Tensor) or a.dtype != torch.float64 or a.dim() != len(lead) + 3:
        raise ValueError("%s: %s must be a float64 %s tensor" % (who, name, lead + ("K", F, T)))
    a = a if batched else a[None]
    if a.shape[0] != B or a.shape[2] not in (1, F) or a.shape[3] != T or (K is not None and a.shape[1] != K):
        raise ValueError("%s: %s must be %s (or with 1 in place of F), got %s"
                         % (who, name, lead + ("K" if K is None else K, F, T), tuple(a.shape[0 if batched else 1:])))
    if a.shape[1] < 1 or a.shape[1] > MAX_CLASSES:
        raise ValueError("%s: need 1 <= K <= 8 classes, got K = %d" % (who, a.shape[1]))
    return a.expand(B, a.shape[1], F, T)


def cacgmm(spec, init, iterations=20, quadratic0=None, floor=1e-10):
    """cACGMM spatial clustering (Ito, Araki, Nakatani, EUSIPCO 2016; csrc/cacgmm.hip): the masks of K classes -- talkers and
    diffuse noise alike -- on D microphones, K and D independent, which is what ``auxiva`` cannot give.  spec (D, F, T) or
    (B, D, F, T), complex64 or complex128 on the GPU, 2 <= D <= 8; init (B, K, F, T) float64 (``time_masks``), 1 <= K <= 8, or
    (B, K, 1, T), expanded over the bins here; quadratic0 None or like init -> ``CACGMM(masks (B, K, F, T) float64 summing to 1
    over k, prior (B, K, T), cov (B, F, K, D, D) complex128, the normalised class matrices, quadratic (B, K, F, T), status
    (B, F) int32)``, without B for a (D, F, T) spec.  ``masks[:, k]`` and ``1 - masks[:, k]`` are the speech and noise masks of
    ``beamforming.mvdr`` and ``gev``.  ``cacgmm(X, init, a + b)`` equals ``cacgmm(X, r.masks, b, quadratic0=r.quadratic)`` with
    ``r = cacgmm(X, init, a)`` bit for bit.

    Definitions (in full: include/alvq.h).  z[f, t] = x / |x|; gamma = init as it is, q = quadratic0 or 1.  A bin with a
    non-finite value, a negative or non-finite init or a quadratic0 that is not > 0 gets status 1, emits masks = 1 / K, cov = I,
    quadratic = 1 and stays out of the priors; a frame of zeros is silent: weight 0 in the M-step, gamma = prior and q = 1 after
    the E-step.  One iteration: (1) prior[b, k, t] = the mean of gamma over the item's bins of status 0, f rising.  (2) per bin
    and class B_k = D sum_t (gamma / q) z z^H / sum_t gamma (I for a class without weight), eigendecomposed; lambda_i <-
    max(lambda_i, floor lambda_max), then scaled to sum to D; a failure gives status 2.  (3) per frame
    q_k = sum_i |v_i^H z|^2 / lambda_i, l_k = log prior - log det B_k - D log q_k, gamma = softmax_k l_k.  There is no frequency
    permutation alignment: the priors shared over frequency stand in for it, which is why the init should be constant over
    frequency.  Nothing here reads a status: the caller does, when it can sync."""
    who = "cacgmm"
    x, batched = _spec4(who, spec)
    B, D, F, T = x.shape
    if D < 2:
        raise ValueError("%s: need 2 <= D <= 8 microphones, got D = %d" % (who, D))
    g0 = _class_array(who, "init", init, B, F, T, batched)
    q0 = None if quadratic0 is None else _class_array(who, "quadratic0", quadratic0, B, F, T, batched, g0.shape[1])
    _int_in(who, "iterations", iterations, 1, MAX_ITERATIONS)
    _nonneg(who, "floor", floor)
    if floor > 1:
        raise ValueError("%s: floor must be in [0, 1], got %r" % (who, floor))
    _on_gpu(who, x, "spec")
    _on_gpu(who, g0, "init")
    if q0 is not None:
        _on_gpu(who, q0, "quadratic0")
    out = CACGMM(*N.cacgmm(x, g0, int(iterations), float(floor), q0))
    return out if batched else CACGMM(*(t[0] for t in out))


def time_masks(B, K, F, T, generator=None, device="cuda"):
    """An init for ``cacgmm`` that is constant over frequency: uniform(0, 1) + 1e-3 per (b, k, t) from ``generator``, normalised
    over k and repeated over f -> (B, K, F, T) float64 on ``device``.  With an independent init per bin the classes of different
    bins come out in different orders, and the masks near chance across bins."""
    who = "time_masks"
    for name, v, hi in (("B", B, 65535), ("K", K, MAX_CLASSES), ("F", F, 2 ** 31 - 1), ("T", T, MAX_FRAMES)):
        _int_in(who, name, v, 1, hi)
    m = torch.rand((B, K, 1, T), dtype=torch.float64, generator=generator, device=device) + 1e-3
    return (m / m.sum(dim=1, keepdim=True)).expand(B, K, F, T).contiguous()
