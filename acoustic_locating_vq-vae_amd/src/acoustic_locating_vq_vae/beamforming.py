"""The baseline a multi-channel enhancer is measured against, on the device (csrc/beamform.hip): the textbook ways from a
microphone array's D spectrograms to one -- delay-and-sum, which steers at a position; MVDR (Capon 1969), which also takes a
noise covariance (MPDR where that is the observed mixture's); and the MVDR from two mask-weighted covariances (Souden, Benesty
and Affes 2010), which needs no geometry and is where a learned model plugs in: its time-frequency masks say which frames count
as speech and which as noise.  Float64 arithmetic, fixed-order sums, no host sync.

    from acoustic_locating_vq_vae import front_end as FE, localization as LOC, beamforming as BF
    h = FE.array_impulse_responses(src, mics, room, reverberation_time=0.4, nsample=6400)     # (B, D, nsample)
    spec = FE.array_spectrograms(wave, h)                                                     # (B, D, F, T) complex128
    BF.delay_and_sum(spec, mics, src).spec                        # (B, F, T): listen in the direction of src
    BF.mvdr(spec, mics, src).spec                                 # MPDR: the mixture's own covariance
    BF.mvdr(spec, mics, src, noise_mask=m_noise).spec             # MVDR: the covariance of the frames a mask calls noise
    BF.mvdr(spec, noise_mask=m_noise, speech_mask=m_speech).spec  # Souden: two masks (B, F, T), no geometry
    BF.gev(spec, m_noise, m_speech).spec                          # GEV / max-SNR: the same two masks, an eigenvector
    BF.gev_weights(cov_n, cov_s).rtf                              # ... and the steering vector (RTF) the masks imply
    beam, srp = BF.locate_and_beamform(spec, mics, grid)          # SRP-PHAT's arg-max over a (G, 3) grid, then MPDR at it
    FE.istft(beam.spec, length=S)                                 # (B, S): speech_metrics.stoi and si_sdr apply directly

Definitions (in full: include/alvq.h).  Every (item, frequency bin) is a problem of its own.  With weights m_t >= 0 (1 without
a mask), Phi[i][j] = sum_t m_t x_i[t] conj(x_j[t]) / sum_t m_t.  With tau_d = |q - m_d| / c, the steering vector towards q is
a_d[f] = e^{-j 2 pi f (fs / n_fft) (tau_d - tau_ref)}: the sign of ``localization.srp_phat``, so its arg-max steers correctly.
Phi' = Phi_n + loading tr(Phi_n) / D I.  Delay-and-sum: w = a / D.  MVDR: z = Phi'^-1 a by Cholesky, w = z / Re(a^H z).
Souden: G = Phi'^-1 Phi_s, w = G[:, ref] / Re tr G.  The output is y[t] = sum_d conj(w_d) x_d[t].  ``status`` (int32 per item
and bin) is 0, or 1 = a non-finite spectrogram value, a negative or non-finite mask value or a mask that sums to 0 (the
covariance is then all zeros), or 2 = a Cholesky pivot or the denominator <= 0 or not finite; a bin with 2 (every bin with 1
ends there) gets w = e_ref: the reference microphone passes through.  ``steering_vectors``' status is per item: bit 4 = a
non-finite coordinate, the row is NaN.  Nothing here reads a status: the caller does, when it can sync.
"""
import collections

import torch

from . import _native as N
from . import _rules as rules
from . import localization as LOC
from ._rules import MAX_FRAMES, MAX_MICROPHONES  # noqa: F401 -- public here
from .front_end import HOP, N_FFT, SOUND_SPEED

Cov = collections.namedtuple("Cov", "cov status")
Weights = collections.namedtuple("Weights", "w status")
Beam = collections.namedtuple("Beam", "spec weights status")
Gev = collections.namedtuple("Gev", "w rtf gain status")

METHODS = {"das": N.BEAMFORM_DAS, "mvdr": N.BEAMFORM_MVDR, "souden": N.BEAMFORM_SOUDEN}


def _mask3(who, name, mask, dims, batched):
    """mask as float64 (B, F, T) for a spectrogram of dims = (B, D, F, T)."""
    B, _, F, T = dims
    want = (B, F, T) if batched else (F, T)
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.float64 or tuple(mask.shape) != want:
        raise ValueError("%s: %s must be a float64 %s tensor for spec %s" % (who, name, want, tuple(dims) if batched else tuple(dims[1:])))
    return mask if batched else mask[None]


def _cplx(who, name, t, dims):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.complex128 or t.dim() not in dims:
        raise ValueError("%s: %s must be a complex128 tensor of %s dimensions" % (who, name, " or ".join(str(d) for d in dims)))


def steering_vectors(mics, source, F, fs=16000, n_fft=N_FFT, c=SOUND_SPEED, ref=0):
    """Steering vectors towards a position: microphones mics (D, 3) or (B, D, 3) and source (3,) or (B, 3), float64 on the GPU
    -> ``(A, status)``: A (B, D, F) complex128 with A[:, ref] = 1 and status (B,) int32 -- (D, F) and a scalar where neither
    argument has a batch dimension.  F need not be n_fft / 2 + 1: bin f stands for the frequency f fs / n_fft."""
    who = "steering_vectors"
    if not isinstance(mics, torch.Tensor) or mics.dim() not in (2, 3) or mics.shape[-1] != 3 or mics.dtype != torch.float64:
        raise ValueError("%s: mics must be a float64 (D, 3) or (B, D, 3) tensor" % who)
    if not isinstance(source, torch.Tensor) or source.dim() not in (1, 2) or source.shape[-1] != 3 or source.dtype != torch.float64:
        raise ValueError("%s: source must be a float64 (3,) or (B, 3) tensor" % who)
    batched = mics.dim() == 3 or source.dim() == 2
    B = source.shape[0] if source.dim() == 2 else (mics.shape[0] if mics.dim() == 3 else 1)
    if mics.dim() == 3 and mics.shape[0] != B:
        raise ValueError("%s: mics holds %d items, source %d" % (who, mics.shape[0], B))
    D = mics.shape[-2]
    rules.microphones(who, D)
    rules.int_in(who, "F", F, 1, 2 ** 24)
    rules.bins(who, "B = %d, F = %d" % (B, F), B, F)
    rules.positive(who, "fs", fs)
    rules.int_in(who, "n_fft", n_fft, 2, 2 ** 24)
    rules.positive(who, "c", c)
    rules.int_in(who, "ref", ref, 0, D - 1)
    rules.all_on_gpu(who, mics=mics, source=source)
    src = source.expand(B, 3) if source.dim() == 1 else source
    A, status = N.steering_vectors(mics, src, F, fs, n_fft, c, ref)
    return (A, status) if batched else (A[0], status[0])


def spatial_covariance(spec, mask=None):
    """Spatial covariances: spec (D, F, T) or (B, D, F, T), complex64 or complex128, and mask None or float64 (F, T) / (B, F, T)
    weights >= 0, on the GPU -> ``Cov(cov, status)``: cov (B, F, D, D) complex128, exactly Hermitian, and status (B, F) int32
    (no B for a (D, F, T) spec)."""
    who = "spatial_covariance"
    x, batched = rules.spec4(who, spec)
    if mask is not None:
        mask = _mask3(who, "mask", mask, x.shape, batched)
    rules.all_on_gpu(who, spec=x, mask=mask)
    return rules.unbatch(Cov(*N.spatial_covariance(x, mask)), batched)


def weights(method, noise_cov=None, steering=None, speech_cov=None, ref=0, loading=1e-6):
    """Beamformer weights: method "das" (steering), "mvdr" (noise_cov, steering) or "souden" (noise_cov, speech_cov);
    covariances (F, D, D) or (B, F, D, D) and steering (D, F) or (B, D, F), complex128 on the GPU -> ``Weights(w, status)``:
    w (B, F, D) complex128 and status (B, F) int32 (no B where the arguments have none).  An argument the method does not
    read must be None."""
    who = "weights"
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError("%s: method must be one of 'das', 'mvdr', 'souden', got %r" % (who, method))
    need = {"das": (False, True, False), "mvdr": (True, True, False), "souden": (True, False, True)}[method]
    given = (("noise_cov", noise_cov, (3, 4)), ("steering", steering, (2, 3)), ("speech_cov", speech_cov, (3, 4)))
    for wanted, (name, t, dims) in zip(need, given):
        if wanted and t is None:
            raise ValueError("%s: method %r needs %s" % (who, method, name))
        if not wanted and t is not None:
            raise ValueError("%s: method %r does not read %s" % (who, method, name))
        if wanted:
            _cplx(who, name, t, dims)
    used = [(name, t, dims) for wanted, (name, t, dims) in zip(need, given) if wanted]
    batched = used[0][1].dim() == used[0][2][1]
    for name, t, dims in used:
        if (t.dim() == dims[1]) != batched:
            raise ValueError("%s: %s and %s must both have a batch dimension or neither" % (who, used[0][0], name))
    noise_cov, steering, speech_cov = (None if t is None else (t if batched else t[None]) for t in (noise_cov, steering, speech_cov))
    if steering is not None:
        B, D, F = steering.shape
    else:
        B, F, D = noise_cov.shape[:3]
    for name, t in (("noise_cov", noise_cov), ("speech_cov", speech_cov)):
        if t is not None and tuple(t.shape) != (B, F, D, D):
            raise ValueError("%s: %s must be %s, got %s" % (who, name, (B, F, D, D) if batched else (F, D, D),
                                                           tuple(t.shape) if batched else tuple(t.shape[1:])))
    rules.microphones(who, D)
    rules.bins(who, "B = %d, F = %d" % (B, F), B, F)
    rules.int_in(who, "ref", ref, 0, D - 1)
    rules.nonneg(who, "loading", loading)
    rules.all_on_gpu(who, noise_cov=noise_cov, steering=steering, speech_cov=speech_cov)
    out = Weights(*N.beamform_weights(METHODS[method], B, D, F, noise_cov, speech_cov, steering, ref, float(loading)))
    return rules.unbatch(out, batched)


def apply(spec, w):
    """y = w^H x: spec (D, F, T) or (B, D, F, T), complex64 or complex128, and w (F, D) or (B, F, D) complex128 on the GPU ->
    (F, T) or (B, F, T) of spec's dtype."""
    who = "apply"
    x, batched = rules.spec4(who, spec)
    B, D, F, T = x.shape
    want = (B, F, D) if batched else (F, D)
    if not isinstance(w, torch.Tensor) or w.dtype != torch.complex128 or tuple(w.shape) != want:
        raise ValueError("%s: w must be a complex128 %s tensor for spec %s" % (who, want, tuple(spec.shape)))
    rules.all_on_gpu(who, spec=x, w=w)
    return rules.unbatch(N.beamform_apply(x, w if batched else w[None]), batched)


def _geometry_rules(who, dims, batched, mics, source, fs, n_fft, c, ref):
    """The rules of mics, source and the steering keywords for a spectrogram of dims = (B, D, F, T); ValueErrors only."""
    B, D = dims[0], dims[1]
    if not isinstance(mics, torch.Tensor) or mics.dtype != torch.float64 or tuple(mics.shape) not in ((D, 3), (B, D, 3)) \
            or (mics.dim() == 3 and not batched):
        raise ValueError("%s: mics must be a float64 (%d, 3)%s tensor" % (who, D, " or (%d, %d, 3)" % (B, D) if batched else ""))
    if not isinstance(source, torch.Tensor) or source.dtype != torch.float64 \
            or tuple(source.shape) not in (((3,), (B, 3)) if batched else ((3,),)):
        raise ValueError("%s: source must be a float64 (3,)%s tensor" % (who, " or (%d, 3)" % B if batched else ""))
    rules.positive(who, "fs", fs)
    rules.int_in(who, "n_fft", n_fft, 2, 2 ** 24)
    rules.positive(who, "c", c)
    rules.int_in(who, "ref", ref, 0, D - 1)


def _mvdr_rules(who, dims, batched, mics, source, noise_mask, speech_mask, ref, loading, fs, n_fft, c):
    """``mvdr``'s rules for a spectrogram of dims = (B, D, F, T), ValueErrors only -> (whether geometry is given, the masks as
    (B, F, T) or None)."""
    if (mics is None) != (source is None):
        raise ValueError("%s: mics and source come together" % who)
    geometry = mics is not None
    if geometry and speech_mask is not None:
        raise ValueError("%s: speech_mask goes with noise_mask and no geometry (Souden); with mics and source give noise_mask or no mask" % who)
    if not geometry and (noise_mask is None or speech_mask is None):
        raise ValueError("%s: without mics and source both noise_mask and speech_mask are needed (Souden)" % who)
    if noise_mask is not None:
        noise_mask = _mask3(who, "noise_mask", noise_mask, dims, batched)
    if speech_mask is not None:
        speech_mask = _mask3(who, "speech_mask", speech_mask, dims, batched)
    rules.int_in(who, "ref", ref, 0, dims[1] - 1)
    rules.nonneg(who, "loading", loading)
    if geometry:
        _geometry_rules(who, dims, batched, mics, source, fs, n_fft, c, ref)
    return geometry, noise_mask, speech_mask


def _steer(x, mics, source, fs, n_fft, c, ref):
    """Checked arguments -> the steering vectors (B, D, F) for the (B, D, F, T) spectrogram x."""
    return N.steering_vectors(mics, source.expand(x.shape[0], 3), x.shape[2], fs, n_fft, c, ref)[0]


def _das(x, mics, source, fs, n_fft, c, ref):
    """``delay_and_sum`` of checked arguments, x (B, D, F, T) -> a batched Beam."""
    w = weights("das", steering=_steer(x, mics, source, fs, n_fft, c, ref))
    return Beam(apply(x, w.w), w.w, w.status)


def _mvdr(x, geometry, mics, source, noise_mask, speech_mask, ref, loading, fs, n_fft, c):
    """``mvdr`` of checked arguments, x (B, D, F, T) and masks (B, F, T) -> a batched Beam."""
    noise = spatial_covariance(x, noise_mask)
    status = noise.status
    if geometry:
        w = weights("mvdr", noise.cov, _steer(x, mics, source, fs, n_fft, c, ref), ref=ref, loading=loading)
    else:
        speech = spatial_covariance(x, speech_mask)
        status = status | speech.status
        w = weights("souden", noise.cov, speech_cov=speech.cov, ref=ref, loading=loading)
    return Beam(apply(x, w.w), w.w, status | w.status)


def delay_and_sum(spec, mics, source, fs=16000, n_fft=N_FFT, c=SOUND_SPEED, ref=0):
    """Delay-and-sum towards source: spec (D, F, T) or (B, D, F, T), mics (D, 3) or (B, D, 3), source (3,) or (B, 3) ->
    ``Beam(spec, weights, status)``: ``apply(spec, weights("das", steering=A).w)`` with A = ``steering_vectors(mics, source,
    F, ...)``; status (B, F) is 0.  A non-finite coordinate gives a NaN item: ``steering_vectors`` tells."""
    who = "delay_and_sum"
    x, batched = rules.spec4(who, spec)
    _geometry_rules(who, x.shape, batched, mics, source, fs, n_fft, c, ref)
    rules.all_on_gpu(who, spec=x, mics=mics, source=source)
    return rules.unbatch(_das(x, mics, source, fs, n_fft, c, ref), batched)


def mvdr(spec, mics=None, source=None, noise_mask=None, speech_mask=None, ref=0, loading=1e-6, fs=16000, n_fft=N_FFT,
         c=SOUND_SPEED):
    """The MVDR beamformer in its three forms -> ``Beam(spec, weights, status)``, spec (B, F, T) in the input's dtype, weights
    (B, F, D) complex128, status (B, F) int32 = the covariances' status OR the weights' (no B for a (D, F, T) spec):
      mics and source, no mask       MPDR: ``weights("mvdr", spatial_covariance(spec).cov, A)``
      mics, source and noise_mask    MVDR: ``weights("mvdr", spatial_covariance(spec, noise_mask).cov, A)``
      noise_mask and speech_mask     Souden: ``weights("souden", spatial_covariance(spec, noise_mask).cov,
                                     speech_cov=spatial_covariance(spec, speech_mask).cov)``, no geometry
    with A = ``steering_vectors(mics, source, F, fs, n_fft, c, ref)``.  Any other combination is a ValueError.  A non-finite
    coordinate makes the item's A NaN, so the denominator of every one of its bins is NaN: status 2 and the reference
    microphone in all of them (``steering_vectors`` names the cause, its bit 4; it is not repeated here)."""
    who = "mvdr"
    x, batched = rules.spec4(who, spec)
    geometry, noise_mask, speech_mask = _mvdr_rules(who, x.shape, batched, mics, source, noise_mask, speech_mask, ref, loading, fs,
                                                    n_fft, c)
    rules.all_on_gpu(who, spec=x, mics=mics, source=source, noise_mask=noise_mask, speech_mask=speech_mask)
    return rules.unbatch(_mvdr(x, geometry, mics, source, noise_mask, speech_mask, ref, loading, fs, n_fft, c), batched)


def gev_weights(noise_cov, speech_cov, ref=0, loading=1e-6):
    """The GEV (max-SNR) beamformer of two covariances (Warsitz and Haeb-Umbach 2007) and the steering vector they imply
    (covariance whitening, Markovich-Golan and Gannot 2015): noise_cov, speech_cov (F, D, D) or (B, F, D, D) complex128 on the
    GPU -> ``Gev(w, rtf, gain, status)``.  With Phi' = noise_cov + loading tr(noise_cov) / D I = L L^H and (lambda_max, u) the
    top eigenpair of L^-1 speech_cov L^-H (``subspace.eigh``'s solver, inside the kernel): v = L^-H u maximises
    v^H speech_cov v / v^H Phi' v, a = Phi' v is the steering vector up to scale, rtf = a / a_ref the relative transfer
    function and w = v conj(a_ref) the weights normalised to w^H rtf = 1 (the MVDR towards rtf where speech_cov has rank
    1); gain = lambda_max.  w, rtf (B, F, D) complex128, gain (B, F) float64, status (B, F) int32: 0, or 2 = a pivot or
    lambda_max <= 0 or not finite, a_ref = 0 or the eigensolver did not converge; such a bin gets w = rtf = e_ref and gain
    0."""
    who = "gev_weights"
    _cplx(who, "noise_cov", noise_cov, (3, 4))
    _cplx(who, "speech_cov", speech_cov, (3, 4))
    if noise_cov.dim() != speech_cov.dim():
        raise ValueError("%s: noise_cov and speech_cov must both have a batch dimension or neither" % who)
    batched = noise_cov.dim() == 4
    pn, ps = (noise_cov, speech_cov) if batched else (noise_cov[None], speech_cov[None])
    B, F, D = pn.shape[:3]
    for name, t in (("noise_cov", pn), ("speech_cov", ps)):
        if tuple(t.shape) != (B, F, D, D):
            raise ValueError("%s: %s must be %s, got %s" % (who, name, (B, F, D, D) if batched else (F, D, D),
                                                           tuple(t.shape) if batched else tuple(t.shape[1:])))
    rules.microphones(who, D)
    rules.bins(who, "B = %d, F = %d" % (B, F), B, F)
    rules.int_in(who, "ref", ref, 0, D - 1)
    rules.nonneg(who, "loading", loading)
    rules.all_on_gpu(who, noise_cov=pn, speech_cov=ps)
    return rules.unbatch(Gev(*N.beamform_gev(pn, ps, ref, float(loading))), batched)


def gev(spec, noise_mask, speech_mask, ref=0, loading=1e-6):
    """The GEV beamformer from two masks: ``apply(spec, gev_weights(spatial_covariance(spec, noise_mask).cov,
    spatial_covariance(spec, speech_mask).cov, ref, loading).w)`` -> ``Beam(spec, weights, status)`` as ``mvdr`` returns it,
    status the covariances' OR the weights'."""
    who = "gev"
    x, batched = rules.spec4(who, spec)
    if noise_mask is None or speech_mask is None:
        raise ValueError("%s: both noise_mask and speech_mask are needed" % who)
    noise_mask = _mask3(who, "noise_mask", noise_mask, x.shape, batched)
    speech_mask = _mask3(who, "speech_mask", speech_mask, x.shape, batched)
    rules.int_in(who, "ref", ref, 0, x.shape[1] - 1)
    rules.nonneg(who, "loading", loading)
    rules.all_on_gpu(who, spec=x, noise_mask=noise_mask, speech_mask=speech_mask)
    noise, speech = spatial_covariance(x, noise_mask), spatial_covariance(x, speech_mask)
    w = gev_weights(noise.cov, speech.cov, ref=ref, loading=loading)
    return rules.unbatch(Beam(apply(x, w.w), w.w, noise.status | speech.status | w.status), batched)


def locate_and_beamform(spec, mics, candidates, ref=0, loading=1e-6, fs=16000, n_fft=N_FFT, c=SOUND_SPEED, band=None):
    """Find the source, then listen there: ``localization.srp_phat(spec, mics, candidates, fs, n_fft, c, band)`` and MPDR
    (``mvdr(spec, mics, source)``) steered at its arg-max candidate -- at candidate 0 where ``best`` is -1: read the status ->
    ``(Beam, SRP)``."""
    srp = LOC.srp_phat(spec, mics, candidates, fs=fs, n_fft=n_fft, c=c, band=band)
    pick = srp.best.clamp_min(0).to(torch.int64)
    if candidates.dim() == 3:
        source = candidates.gather(1, pick.view(-1, 1, 1).expand(-1, 1, 3))[:, 0]
    else:
        source = candidates[pick]
    return mvdr(spec, mics, source, ref=ref, loading=loading, fs=fs, n_fft=n_fft, c=c), srp


def beamform_waves(waves, mics=None, source=None, method="mvdr", noise_mask=None, speech_mask=None, ref=0, loading=1e-6, fs=16000,
                   n_fft=N_FFT, hop=HOP, c=SOUND_SPEED):
    """Waveforms in, a waveform out: waves (B, D, S), float32 or float64 on the GPU -> (B, S) of the same dtype,
    ``front_end.istft(beam.spec, length=S)`` of beam = ``mvdr(spec, mics, source, noise_mask, speech_mask, ...)`` (method
    "mvdr") or ``delay_and_sum(spec, mics, source, ...)`` (method "das") on spec = ``N.stft_complex`` of the B D rows, which
    has F = n_fft / 2 + 1 bins and T = 1 + S / hop frames: the masks are (B, F, T).  Their rules, under this function's name."""
    who = "beamform_waves"
    rules.waves3(who, waves)
    if method not in ("mvdr", "das"):
        raise ValueError("%s: method must be 'mvdr' or 'das', got %r" % (who, method))
    if method == "das" and (noise_mask is not None or speech_mask is not None):
        raise ValueError("%s: method 'das' takes no mask" % who)
    dims = rules.stft_dims(who, waves, n_fft, hop)
    B, D, S = waves.shape
    geometry = True
    if method == "das":
        _geometry_rules(who, dims, True, mics, source, fs, n_fft, c, ref)
    else:
        geometry, noise_mask, speech_mask = _mvdr_rules(who, dims, True, mics, source, noise_mask, speech_mask, ref, loading, fs,
                                                        n_fft, c)
    rules.all_on_gpu(who, waves=waves, mics=mics, source=source, noise_mask=noise_mask, speech_mask=speech_mask)
    spec = N.stft_complex(waves.reshape(B * D, S).contiguous(), n_fft, hop).view(dims)
    if method == "das":
        beam = _das(spec, mics, source, fs, n_fft, c, ref)
    else:
        beam = _mvdr(spec, geometry, mics, source, noise_mask, speech_mask, ref, loading, fs, n_fft, c)
    return N.istft(beam.spec, n_fft, hop, S)
