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

AuxIVA's source model is one activity per frame, shared by all bins; it says nothing about which frequencies a source occupies.
ILRMA (independent low-rank matrix analysis; Kitamura et al., IEEE/ACM TASLP 2016; csrc/ilrma.hip) keeps AuxIVA's demixing update
and gives every source a rank-``bases`` non-negative model of its variance over (f, t), fitted by multiplicative updates:

    b0, a0 = SEP.nmf_init(B, D, F, T, bases=2, generator=g)       # (B, D, F, L) and (B, D, L, T) float64, uniform(0, 1) + 1e-3
    r = SEP.ilrma(spec, b0, a0, iterations=30)                    # ILRMA(spec, w, basis, activations, status)
    SEP.ilrma(spec, r.basis, r.activations, 10, w0=r.w)           # ten more iterations, bit for bit
    SEP.ilrma(spec, b0, a0, 30, w0=SEP.auxiva(spec, 10).w)        # started from AuxIVA, which has ordered the bins' sources
    SEP.masks(r.spec)                                             # as for auxiva
    SEP.separate_waves(waves, method="ilrma", bases=2, generator=g)

A random start at few bins can lock the sources of different bins in different orders -- this is known of ILRMA -- which is what
``w0`` is for.  Its definitions are ``ilrma``'s docstring and, in full, include/alvq.h.

All three return their sources in an order nobody chose.  ``speech_metrics`` scores the outputs against the clean talkers on
the device (csrc/separation_metrics.hip) and says which is which; ``reorder`` applies that:

    from acoustic_locating_vq_vae import speech_metrics as SM
    waves = FE.istft(sep.spec.reshape(B * D, F, T), length=S).view(B, D, S)
    pit = SM.pit_si_sdr(clean, waves)                             # PIT(value (B, K) dB, perm (B, K), status (B,))
    SEP.reorder(sep.spec, SM.pit_si_sdr(clean, waves).perm)       # (B, K, F, T): output perm[b, k] is talker k
    SM.si_bss_eval(clean, waves)                                  # sir: crosstalk left (demixing); sar: artefacts (masking)

That is ONE order per item.  A separation that is right inside every bin but orders its sources differently from bin to bin --
what any estimator that works per bin gives, a learned one included -- is repaired by ``align_permutations``
(csrc/permutation_align.hip): Sawada's correlation of the classes' time profiles against per-source centroids.  ``permute_bins``
applies its result to (B, K, F, T) arrays, ``permute_rows`` to the small per-bin ones (w, cov):

    r = SEP.cacgmm(spec, init_drawn_per_bin, 10)
    a = SEP.align_permutations(r.masks)                           # ALIGN(perm (B, F, K), score (B, F), changed (B,), status (B, F))
    SEP.cacgmm(spec, SEP.permute_bins(r.masks, a.perm), 10, quadratic0=SEP.permute_bins(r.quadratic, a.perm))

    a = SEP.align_permutations(SEP.masks(r.spec))                 # r: an auxiva / ilrma result whose bins disagree
    SEP.permute_bins(r.spec, a.perm)                              # then istft, pit_si_sdr
    SEP.auxiva(spec, 10, w0=SEP.permute_rows(r.w, a.perm))        # ... or go on from the aligned demixing matrices

Its definitions are ``align_permutations``' docstring and, in full, include/alvq.h.
"""
import collections

import torch

from . import _native as N
from . import _rules as rules
from ._rules import MAX_FRAMES, MAX_MICROPHONES
from .front_end import HOP, N_FFT

IVA = collections.namedtuple("IVA", "spec w status")
ILRMA = collections.namedtuple("ILRMA", "spec w basis activations status")
CACGMM = collections.namedtuple("CACGMM", "masks prior cov quadratic status")
ALIGN = collections.namedtuple("ALIGN", "perm score changed status")

MAX_ITERATIONS = 256
MODELS = {"laplace": N.IVA_LAPLACE, "gauss": N.IVA_GAUSS}
METHODS = ("auxiva", "ilrma")
MAX_CLASSES = 8
MAX_BASES = 16


def _iva_rules(who, D, iterations, model, ref, eps):
    """The rules of the keywords for D microphones; ValueErrors only."""
    rules.int_in(who, "iterations", iterations, 0, MAX_ITERATIONS)
    if not isinstance(model, str) or model not in MODELS:
        raise ValueError("%s: model must be one of 'laplace', 'gauss', got %r" % (who, model))
    rules.int_in(who, "ref", ref, 0, D - 1)
    rules.nonneg(who, "eps", eps)


def _start_w(who, w0, spec, dims, batched):
    """w0 as (B, F, D, D), or None: a complex128 tensor of the rank that mirrors spec's."""
    if w0 is None:
        return None
    B, D, F, _ = dims
    want = (B, F, D, D) if batched else (F, D, D)
    if not isinstance(w0, torch.Tensor) or w0.dtype != torch.complex128 or tuple(w0.shape) != want:
        raise ValueError("%s: w0 must be a complex128 %s tensor for spec %s" % (who, want, tuple(spec.shape)))
    return w0 if batched else w0[None]


def auxiva(spec, iterations=20, model="laplace", ref=0, eps=1e-10, w0=None):
    """AuxIVA of an array's spectrograms: spec (D, F, T) or (B, D, F, T), complex64 or complex128 on the GPU, and w0 None or a
    complex128 (F, D, D) / (B, F, D, D) start -> ``IVA(spec, w, status)``: the D separated spectrograms as microphone ``ref``
    heard them, of spec's shape and dtype, the demixing matrices w (B, F, D, D) complex128 and status (B, F) int32 (no B for a
    (D, F, T) spec).  ``auxiva(X, a + b).w`` equals ``auxiva(X, b, w0=auxiva(X, a).w).w`` bit for bit."""
    who = "auxiva"
    x, batched = rules.spec4(who, spec)
    B, D, F, T = x.shape
    _iva_rules(who, D, iterations, model, ref, eps)
    w0 = _start_w(who, w0, spec, x.shape, batched)
    rules.all_on_gpu(who, spec=x, w0=w0)
    return rules.unbatch(IVA(*N.auxiva(x, int(iterations), MODELS[model], int(ref), float(eps), w0)), batched)


def _ilrma_rules(who, D, iterations, ref, floor):
    """The rules of ILRMA's keywords for D microphones; ValueErrors only."""
    rules.int_in(who, "iterations", iterations, 0, MAX_ITERATIONS)
    rules.int_in(who, "ref", ref, 0, D - 1)
    rules.positive(who, "floor", floor)


def ilrma(spec, basis0, activations0, iterations=20, ref=0, floor=1e-10, w0=None):
    """ILRMA of an array's spectrograms: spec (D, F, T) or (B, D, F, T), complex64 or complex128 on the GPU; basis0 (B, D, F, L)
    and activations0 (B, D, L, T) float64 (``nmf_init``), 1 <= L <= 16, without B for a (D, F, T) spec; w0 as for ``auxiva`` ->
    ``ILRMA(spec, w, basis, activations, status)``: the D separated spectrograms as microphone ``ref`` heard them, the demixing
    matrices w (B, F, D, D) complex128, the fitted factors and status (B, F) int32, the ranks mirroring spec's.
    ``ilrma(X, b0, a0, m + n)`` equals ``ilrma(X, r.basis, r.activations, n, w0=r.w)`` with ``r = ilrma(X, b0, a0, m)`` bit for
    bit.

    Definitions (in full: include/alvq.h).  The variance of source k is r_k[f, t] = sum_l basis[k, f, l] activations[k, l, t].
    A bin gets status 1 as in ``auxiva``, and also where its basis0 rows hold a value that is not finite or not > 0; every bin
    of an item whose activations0 hold such a value gets it.  Such a bin keeps W = I and Y = X, its basis rows come back as
    given, and it stays out of every sum over f.  One iteration: (1) P[k, f, t] = |y_k[f, t]|^2 and lam[k], its mean over the
    bins whose status is not 1 (1 where that is not > 0 and finite); (2) W[f][k, :] /= sqrt(lam[k]), P /= lam[k], basis[k] =
    max(basis[k] / lam[k], floor), which leaves the cost unchanged and puts the floor on a known scale; (3) with R = max(sum_l
    basis activations, floor): basis <- max(basis sqrt(sum_t P R^-2 activations / sum_t activations / R), floor); (4) with R
    recomputed: activations <- max(activations sqrt(sum_f P R^-2 basis / sum_f basis / R), floor); a ratio that is not finite
    leaves the entry as it was, and max(., floor) sends a value that is not finite to floor; (5) with R recomputed, step (3)
    of ``auxiva`` in every bin of status 0 with phi[k, t] replaced by 1 / R[k, f, t].  Then ``auxiva``'s projection onto
    microphone ``ref``.  Nothing here reads a status: the caller does, when it can sync."""
    who = "ilrma"
    x, batched = rules.spec4(who, spec)
    B, D, F, T = x.shape
    lead = (B,) if batched else ()
    if not isinstance(basis0, torch.Tensor) or basis0.dtype != torch.float64 or basis0.dim() != len(lead) + 3 \
            or tuple(basis0.shape[:-1]) != lead + (D, F):
        raise ValueError("%s: basis0 must be a float64 %s tensor for spec %s" % (who, lead + (D, F, "L"), tuple(spec.shape)))
    L = basis0.shape[-1]
    if L < 1 or L > MAX_BASES:
        raise ValueError("%s: need 1 <= L <= 16 bases, got L = %d" % (who, L))
    if not isinstance(activations0, torch.Tensor) or activations0.dtype != torch.float64 or tuple(activations0.shape) != lead + (D, L, T):
        raise ValueError("%s: activations0 must be a float64 %s tensor for basis0 %s" % (who, lead + (D, L, T), tuple(basis0.shape)))
    _ilrma_rules(who, D, iterations, ref, floor)
    w0 = _start_w(who, w0, spec, x.shape, batched)
    b0, a0 = (basis0, activations0) if batched else (basis0[None], activations0[None])
    rules.all_on_gpu(who, spec=x, basis0=b0, activations0=a0, w0=w0)
    return rules.unbatch(ILRMA(*N.ilrma(x, b0, a0, int(iterations), int(ref), float(floor), w0)), batched)


def nmf_init(B, D, F, T, bases=2, generator=None, device="cuda"):
    """A start for ``ilrma``, the companion of ``time_masks``: (basis0 (B, D, F, bases), activations0 (B, D, bases, T)) float64
    on ``device``, uniform(0, 1) + 1e-3 from ``generator``, the basis drawn first."""
    who = "nmf_init"
    for name, v, hi in (("B", B, rules.MAX_BATCH), ("D", D, MAX_MICROPHONES), ("F", F, rules.MAX_BINS), ("T", T, MAX_FRAMES),
                        ("bases", bases, MAX_BASES)):
        rules.int_in(who, name, v, 1, hi)
    basis0 = torch.rand((B, D, F, bases), dtype=torch.float64, generator=generator, device=device) + 1e-3
    activations0 = torch.rand((B, D, bases, T), dtype=torch.float64, generator=generator, device=device) + 1e-3
    return basis0, activations0


def masks(sep_spec):
    """Ratio masks of separated spectrograms: sep_spec (K, F, T) or (B, K, F, T), complex64 or complex128 on the GPU, K <= 8 ->
    float64 of the same shape, M[:, k] = |Y_k|^2 / sum_j |Y_j|^2.  ``M[:, k]`` and ``1 - M[:, k]`` are the speech and noise
    masks of ``beamforming.mvdr`` and ``gev`` for source k."""
    who = "masks"
    y, batched = rules.spec4(who, sep_spec)
    rules.on_gpu(who, y, "sep_spec")
    return rules.unbatch(N.separation_masks(y), batched)


def reorder(x, perm):
    """The sources of x in the order perm gives: x (B, J, ...) with perm (B, K), or x (J, ...) with perm (K,), on the GPU --
    spectrograms, waveforms or masks, any dtype; perm int32 or int64 as ``speech_metrics.pit_si_sdr`` and ``assign`` return
    it -> (B, K, ...), out[b, k] = x[b, perm[b, k]], by torch indexing on the device.  The entries of perm must lie in
    0..J-1 (``assign``'s always do); they are not read here."""
    who = "reorder"
    if not isinstance(perm, torch.Tensor) or perm.dtype not in (torch.int32, torch.int64) or perm.dim() not in (1, 2):
        raise ValueError("%s: perm must be an int32 or int64 (K,) or (B, K) tensor" % who)
    batched = perm.dim() == 2
    if not isinstance(x, torch.Tensor) or x.dim() < perm.dim():
        raise ValueError("%s: x must be a tensor of at least %d dimensions for a perm of %d" % (who, perm.dim(), perm.dim()))
    if perm.shape[-1] < 1 or x.shape[perm.dim() - 1] < 1 or (batched and (x.shape[0] != perm.shape[0] or x.shape[0] < 1)):
        raise ValueError("%s: x %s and perm %s do not go together" % (who, tuple(x.shape), tuple(perm.shape)))
    rules.all_on_gpu(who, x=x, perm=perm)
    index = perm.long()
    if not batched:
        return x[index]
    return x[torch.arange(x.shape[0], device=x.device)[:, None], index]


def separate_waves(waves, iterations=20, model="laplace", ref=0, n_fft=N_FFT, hop=HOP, method="auxiva", bases=2, generator=None):
    """Waveforms in, waveforms out: waves (B, D, S), float32 or float64 on the GPU -> (B, D, S) of the same dtype, row k
    ``front_end.istft`` of source k of ``auxiva`` on spec = ``N.stft_complex`` of the B D rows, which has F = n_fft / 2 + 1 bins
    and T = 1 + S / hop frames, as ``beamforming.beamform_waves`` goes.  method "ilrma": ``ilrma`` in its place, started from
    ``nmf_init(B, D, F, T, bases, generator)``; ``model`` is AuxIVA's and must then be left at its default."""
    who = "separate_waves"
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError("%s: method must be one of 'auxiva', 'ilrma', got %r" % (who, method))
    if method == "ilrma" and model != "laplace":
        raise ValueError("%s: model belongs to method 'auxiva'; with method 'ilrma' leave it at its default, got %r" % (who, model))
    rules.waves3(who, waves)
    B, D, F, T = rules.stft_dims(who, waves, n_fft, hop)
    S = waves.shape[2]
    _iva_rules(who, D, iterations, model, ref, 0.0)
    rules.int_in(who, "bases", bases, 1, MAX_BASES)
    if generator is not None and not isinstance(generator, torch.Generator):
        raise ValueError("%s: generator must be a torch.Generator or None, got %r" % (who, generator))
    rules.on_gpu(who, waves, "waves")
    spec = N.stft_complex(waves.reshape(B * D, S).contiguous(), n_fft, hop).view(B, D, F, T)
    if method == "ilrma":
        sep = ilrma(spec, *nmf_init(B, D, F, T, bases, generator, waves.device), iterations=iterations, ref=ref)
    else:
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
    permutation alignment inside: the priors shared over frequency stand in for it, which is why the init should be constant
    over frequency; masks whose classes have come out in a different order in every bin are repaired by
    ``align_permutations``.  Nothing here reads a status: the caller does, when it can sync."""
    who = "cacgmm"
    x, batched = rules.spec4(who, spec)
    B, D, F, T = x.shape
    rules.microphones(who, D, 2)
    g0 = _class_array(who, "init", init, B, F, T, batched)
    q0 = None if quadratic0 is None else _class_array(who, "quadratic0", quadratic0, B, F, T, batched, g0.shape[1])
    rules.int_in(who, "iterations", iterations, 1, MAX_ITERATIONS)
    rules.nonneg(who, "floor", floor)
    if floor > 1:
        raise ValueError("%s: floor must be in [0, 1], got %r" % (who, floor))
    rules.all_on_gpu(who, spec=x, init=g0, quadratic0=q0)
    return rules.unbatch(CACGMM(*N.cacgmm(x, g0, int(iterations), float(floor), q0)), batched)


def time_masks(B, K, F, T, generator=None, device="cuda"):
    """An init for ``cacgmm`` that is constant over frequency: uniform(0, 1) + 1e-3 per (b, k, t) from ``generator``, normalised
    over k and repeated over f -> (B, K, F, T) float64 on ``device``.  With an independent init per bin the classes of different
    bins come out in different orders, and the masks near chance across bins."""
    who = "time_masks"
    for name, v, hi in (("B", B, rules.MAX_BATCH), ("K", K, MAX_CLASSES), ("F", F, rules.MAX_BINS), ("T", T, MAX_FRAMES)):
        rules.int_in(who, name, v, 1, hi)
    m = torch.rand((B, K, 1, T), dtype=torch.float64, generator=generator, device=device) + 1e-3
    return (m / m.sum(dim=1, keepdim=True)).expand(B, K, F, T).contiguous()


def _bin_perm(who, name, perm, B, K, F, batched):
    """perm as int32 (B, F, K) for an array of (B, K, F, ...): (F, K) without the batch."""
    want = (B, F, K) if batched else (F, K)
    if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int32 or tuple(perm.shape) != want:
        raise ValueError("%s: %s must be an int32 %s tensor" % (who, name, want))
    return perm if batched else perm[None]


def _class_rows(who, x, dtypes, what):
    """x as (B, K, F, T), checked against the kernels' limits; whether it came with a batch dimension."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4) or x.dtype not in dtypes:
        raise ValueError("%s: %s must be a (K, F, T) or (B, K, F, T) tensor of %s" % (who, what, " or ".join(str(d) for d in dtypes)))
    y = x if x.dim() == 4 else x[None]
    B, K, F, T = y.shape
    if B < 1 or B > rules.MAX_BATCH or K < 1 or K > MAX_CLASSES or F < 1 or B * F > rules.MAX_BINS or T < 1 or T > MAX_FRAMES:
        raise ValueError("%s: need 1 <= B <= 65535, 1 <= K <= 8, F >= 1, B F <= 2^31 - 1 and 1 <= T <= 65535, got shape %s"
                         % (who, tuple(x.shape)))
    return y, x.dim() == 4


def align_permutations(profile, iterations=10, perm0=None):
    """Frequency permutation alignment (Sawada, Araki, Makino, IEEE TASLP 2011, the global stage; csrc/permutation_align.hip):
    profile (K, F, T) or (B, K, F, T) float64 on the GPU, the time profile of class j of bin f -- ``cacgmm``'s masks, ``masks`` of
    a separation, powers, log-powers: any finite reals, 1 <= K <= 8, 2 <= T <= 65535 -- and perm0 None (the identity) or an
    int32 (F, K) / (B, F, K) start -> ``ALIGN(perm (B, F, K) int32, score (B, F) float64, changed (B,) int32, status (B, F)
    int32)``, without B for a (K, F, T) profile (changed is then a scalar tensor).  perm[b, f, k] is the class of bin f that is
    source k: ``permute_bins(x, perm)`` and ``permute_rows(a, perm)`` apply it.  changed counts the bins that the LAST iteration
    moved: 0 at a fixed point.  ``align_permutations(P, a + b)`` equals ``align_permutations(P, b, perm0 = align_permutations(P,
    a).perm)`` bit for bit.

    Definitions (in full: include/alvq.h).  A bin with a non-finite value, or whose perm0 row is not a permutation of 0..K-1,
    gets status 1, perm = the identity and score = NaN, and stays out of every centroid.  Every row (b, j, f) is centred and
    scaled to unit length over t, u = (P - m) / |P - m|, a constant row to 0.  One iteration (Jacobi: all bins are scored
    against the same centroids): (1) c[b, k, t] = sum_f u[perm[b, f, k], f, t], f rising, scaled to unit length over t;
    (2) per bin table[k, j] = sum_t c[k, t] u[j, f, t], and the new perm[b, f, :] is the permutation of the largest total by
    ``speech_metrics.assign``'s exhaustive rule, score its total.  Nothing here reads a status: the caller does, when it can
    sync."""
    who = "align_permutations"
    p, batched = _class_rows(who, profile, (torch.float64,), "profile")
    B, K, F, T = p.shape
    if T < 2:
        raise ValueError("%s: need T >= 2 frames, got T = %d" % (who, T))
    rules.int_in(who, "iterations", iterations, 1, MAX_ITERATIONS)
    p0 = None if perm0 is None else _bin_perm(who, "perm0", perm0, B, K, F, batched)
    rules.all_on_gpu(who, profile=p, perm0=p0)
    return rules.unbatch(ALIGN(*N.align_permutations(p, int(iterations), p0)), batched)


def permute_bins(x, perm):
    """The classes of every bin of x in the order perm gives (csrc/permutation_align.hip): x (K, F, T) or (B, K, F, T), float32,
    float64, complex64 or complex128 on the GPU -- masks, quadratic, separated spectrograms -- and perm int32 (F, K) / (B, F, K)
    as ``align_permutations`` returns it -> a new tensor of x's shape and dtype, out[b, k, f, t] = x[b, perm[b, f, k], f, t].  A
    bin of perm with an entry outside 0..K-1 passes through unpermuted."""
    who = "permute_bins"
    y, batched = _class_rows(who, x, (torch.float32, torch.float64, torch.complex64, torch.complex128), "x")
    B, K, F, _ = y.shape
    p = _bin_perm(who, "perm", perm, B, K, F, batched)
    rules.all_on_gpu(who, x=y, perm=p)
    return rules.unbatch(N.permute_bins(y, p), batched)


def permute_rows(a, perm):
    """The rows of the small per-bin arrays in the order perm gives: a (F, K, ...) or (B, F, K, ...) of any dtype on the GPU --
    ``auxiva``'s and ``ilrma``'s w, whose row k extracts source k, ``cacgmm``'s cov -- and perm int32 (F, K) / (B, F, K) ->
    out[b, f, k] = a[b, f, perm[b, f, k]], by torch indexing on the device (these arrays are small).  The entries of perm must
    lie in 0..K-1 (``align_permutations``' always do); they are not read here.  ILRMA's basis and activations cannot be permuted
    per bin, because an activation is shared by all bins of a source: after aligning an ILRMA result go on with
    ``auxiva(spec, n, w0=permute_rows(r.w, perm))``, or restart ``ilrma`` from ``nmf_init`` with that w0."""
    who = "permute_rows"
    if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int32 or perm.dim() not in (2, 3):
        raise ValueError("%s: perm must be an int32 (F, K) or (B, F, K) tensor" % who)
    if not isinstance(a, torch.Tensor) or a.dim() < perm.dim() or tuple(a.shape[:perm.dim()]) != tuple(perm.shape) or perm.numel() < 1:
        raise ValueError("%s: a must be a tensor of shape %s + (...) for this perm" % (who, tuple(perm.shape)))
    rules.all_on_gpu(who, a=a, perm=perm)
    index = perm.long().reshape(tuple(perm.shape) + (1,) * (a.dim() - perm.dim())).expand(a.shape)
    return torch.gather(a, perm.dim() - 1, index)
