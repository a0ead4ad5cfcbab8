"""Waveform front end on the device.

The reference prepares its training samples offline (scripts/genereate_dataset.py:35-49): a torchaudio complex
spectrogram of the clean speech, the same of the speech convolved with a room impulse response, and from the two the
"RIR spectrogram", the Wiener estimate and three power spectrograms.  These functions do that arithmetic with the
HIP kernels of csrc/stft.hip, so the train loops can start from waveforms instead of from a pre-generated dataset:

    speech_spec, rir_spec, echoed_spec, wiener_est = specs_from_waveform(wave, h_rir)      # the sample 6-tuple's tensors
    x = speech_input_from_waveform(wave)                                                   # straight into Trainer.step

The way back, to listen to a spectrogram or to what a model makes of it (torchaudio InverseSpectrogram and
functional.griffinlim in the reference's notebooks; HIP kernels of csrc/istft.hip):

    wave = istft(spec, length=S)                                    # exact inverse of N.stft_complex (keeps the phase)
    wave = griffin_lim(power)                                       # power (or magnitude, power=1) -> waveform, 32 iterations
    wave = waveform_from_reconstruction(model(x)[1], raw_power)    # a speech model's standardised output -> waveform

The room impulse response, which the reference takes from the ``rir_generator`` C++ package (genereate_dataset.py:21-29), is
made on the device too (image-source method, csrc/rir.hip), and with it the whole generator: a direction goes in, a sample
6-tuple comes out, and ``SpecsDataset`` reads what ``write_specs_dataset`` writes:

    h = rir_generate(c=340, fs=16000, r=[2.5, 1.5, 1.5], s=[3, 2, 2.5], L=[4, 5, 3], reverberation_time=0.4)  # (nsample, 1)
    samples = generate_samples(wave)                          # theta ~ U(-pi, pi) -> source -> RIR -> echoed -> 6-tuple
    write_specs_dataset("spec_data/train", samples, DATASET_CONFIG)

For data that spans rooms, ``SceneConfig`` / ``sample_scenes`` draw a room, T60, receiver and direction per item, and
``scene_impulse_responses`` makes all their responses in one launch (each row bitwise its one-room response);
``rir_dataset_generator.scene_loader.SceneLoader`` builds training batches from them with no files:

    scenes = sample_scenes(64, SceneConfig(), generator)      # rooms 3-8 m, T60 0.25-0.8 s, receivers, theta
    samples = generate_samples(wave, scenes=scenes)           # the same 6-tuple, a room per item

A microphone array in a room, for ``localization`` (GCC-PHAT, SRP-PHAT) and multi-microphone ``dereverberation.wpe``:

    h = array_impulse_responses(src, mics, room, reverberation_time=0.4, nsample=6400)      # (B, D, nsample)
    spec = array_spectrograms(wave, h)                                                      # (B, D, F, T) complex128

Parity with ``rir_generator`` itself is unpinned (the package is absent and the reference holds no fixture); the RIR is
pinned by the closed-form direct path, reciprocity, scipy's lfilter for the high-pass and a float64 restatement.
Any other (Nh,) or (B, Nh) float64 response can still be passed to ``specs_from_waveform``.
"""
import collections
import math
import os

import numpy as np
import torch

from . import _native as N
from . import _rules as rules
from .data_preprocessing import SPEC_FRAMES

N_FFT, HOP = 400, 160        # genereate_dataset.py:73-74 at fs = 16 kHz
SOUND_SPEED = 340.0          # genereate_dataset.py:54 (C)
# the generator's __main__ constants under SpecsDataset's CONFIG_KEYS names (genereate_dataset.py:54-84)
DATASET_CONFIG = {"fs": 16000, "receiver_position": [2.5, 1.5, 1.5], "room_dimensions": [4, 5, 3], "reverberation_time": 0.4,
                  "n_sample": 6400, "R": 1, "NFFT": 400, "HOP_LENGTH": 160, "Z_LOC_SOURCE": 1}


def specs_from_waveform(wave, h_rir, n_fft=N_FFT, hop=HOP):
    """wave (B,S) float32 on the GPU, h_rir (Nh,) or (B,Nh) float64 ->
    (speech_spec (B,F,T) fp32, rir_spec fp64, echoed_spec fp64, wiener_est (B,F) fp64), all powers, with the
    reference's precisions: the clean branch is complex64, everything touched by the convolution is float64."""
    wave = wave.contiguous()
    echoed_wave = N.fir_same(wave, h_rir.contiguous())                      # :38  ss.convolve(..., mode='same')
    speech = N.stft_complex(wave, n_fft, hop)                               # :37
    echoed = N.stft_complex(echoed_wave, n_fft, hop)                        # :39
    speech_pow, echoed_pow, rir_pow, wiener = N.spec_rir_wiener(speech, echoed)   # :41-49
    return speech_pow, rir_pow, echoed_pow, wiener


def speech_input_from_waveform(wave, n_fft=N_FFT, hop=HOP, frames=SPEC_FRAMES):
    """wave (B,S) float32 -> the raw batch a speech train step takes: power spectrogram cropped to ``frames`` frames
    (the collate's crop, data_preprocessing.py:67-69); ``Trainer.step`` standardises it on the device."""
    power = N.stft_power(wave.contiguous(), n_fft, hop)
    if power.shape[2] < frames:
        raise ValueError("waveform gives %d frames, the collate needs %d" % (power.shape[2], frames))
    return power[:, :, :frames].contiguous()


def istft(spec, n_fft=N_FFT, hop=HOP, length=None):
    """The inverse of ``N.stft_complex``: spec (B, n_fft/2+1, T) complex64 / complex128 on the GPU -> (B, length) waveforms
    (torchaudio InverseSpectrogram(n_fft, hop, center=True, pad=0, normalized=True)).  length defaults to hop*(T-1); a longer
    one is zero-padded, as torch.istft does."""
    return N.istft(spec, n_fft, hop, length)


def griffin_lim(spec, power=2.0, n_iter=32, momentum=0.99, length=None, init=None, generator=None, n_fft=N_FFT, hop=HOP):
    """Waveforms (B, length) from a power spectrogram (power=2, what the dataset stores) or a magnitude (power=1), (B, F, T)
    float32 / float64 on the GPU and normalised as ``N.stft_complex``, by torchaudio.functional.griffinlim's iteration.
    init: complex start phases (B, F, T); by default torchaudio's rand_init, ``torch.rand`` of the complex dtype on the device
    (from ``generator`` if one is given).  length defaults to hop*(T-1)."""
    if spec.dim() != 3 or spec.dtype not in (torch.float32, torch.float64):
        raise ValueError("griffin_lim: expected a float32 / float64 (B, F, T) spectrogram, got %s %s" % (spec.dtype, tuple(spec.shape)))
    B, F, T = spec.shape
    if F != n_fft // 2 + 1:
        raise ValueError("griffin_lim: %d frequency bins, n_fft=%d has %d" % (F, n_fft, n_fft // 2 + 1))
    if not 0.0 <= momentum < 1.0:
        raise ValueError("griffin_lim: momentum must be in [0, 1), got %r" % (momentum,))
    if n_iter < 0:
        raise ValueError("griffin_lim: n_iter must be >= 0, got %r" % (n_iter,))
    if power <= 0:
        raise ValueError("griffin_lim: power must be > 0, got %r" % (power,))
    rules.on_gpu("griffin_lim", spec, "spec")
    cdtype = torch.complex128 if spec.dtype == torch.float64 else torch.complex64
    length = hop * (T - 1) if length is None else int(length)
    mag = (spec if power == 1.0 else spec.pow(1.0 / power)).contiguous()
    if init is None:
        init = torch.rand(spec.shape, dtype=cdtype, device=spec.device, generator=generator)
    elif init.shape != spec.shape or init.dtype != cdtype:
        raise ValueError("griffin_lim: init must be %s of shape %s" % (cdtype, tuple(spec.shape)))
    return N.griffin_lim(mag, init.contiguous(), n_iter, momentum, n_fft, hop, length)


def waveform_from_reconstruction(recon, raw_power, **gl_kwargs):
    """What a speech model sounds like: its standardised output recon (B, F, T') -> (B, length) waveforms.

    The speech loop trains on x = (|raw| - mean) / (std + 1e-8) over the frequency axis of each frame (train_speech.py; the
    Trainer's ``N.standardise(raw, take_abs=True)``, unbiased std).  This undoes that with raw_power's own per-frame statistics,
    crops a longer decoder output to raw_power's T frames (as train_speech.py / train_echoed_speech.py do), clamps the power
    at 0 and runs ``griffin_lim`` on it (gl_kwargs: its keyword arguments)."""
    raw = raw_power.abs()
    T = raw.shape[2]
    if recon.dim() != 3 or recon.shape[:2] != raw.shape[:2] or recon.shape[2] < T:
        raise ValueError("waveform_from_reconstruction: recon %s does not cover raw_power %s" % (tuple(recon.shape), tuple(raw.shape)))
    mean = raw.mean(dim=1, keepdim=True)
    std = raw.std(dim=1, keepdim=True)
    power = (recon.detach()[:, :, :T].to(raw.dtype) * (std + 1e-8) + mean).clamp_min(0.0)
    return griffin_lim(power.contiguous(), power=2.0, **gl_kwargs)


def _sabine_alpha(L, c, reverberation_time):
    """Sabine's absorption 24 V ln10 / (c S T60), in this one expression order for host floats and device tensors alike
    (L: three sides, floats or (B,) tensors), so that a room's beta has the same bits on either side."""
    V = L[0] * L[1] * L[2]
    S = 2.0 * (L[0] * L[2] + L[1] * L[2] + L[0] * L[1])
    return 24.0 * V * math.log(10.0) / (c * S * reverberation_time)


def _sabine_beta(L, c, reverberation_time):
    alpha = _sabine_alpha(L, c, reverberation_time)
    if alpha > 1:
        raise ValueError("the reflection coefficients cannot be calculated for room %s and reverberation time %g (alpha = %g > 1);"
                         " give beta or change the room" % (list(L), reverberation_time, alpha))
    return [math.sqrt(1.0 - alpha)] * 6


def _room_params(L, c, beta, reverberation_time, nsample, dim, fs):
    """(L, beta, nsample) after rir_generator's keyword rules; raises before anything is launched."""
    L = [float(v) for v in np.asarray(L, dtype=np.float64).reshape(-1)]
    if len(L) != 3 or not all(math.isfinite(v) and v > 0 for v in L):
        raise ValueError("room dimensions L must be 3 positive lengths, got %r" % (L,))
    if not (c > 0 and fs > 0):
        raise ValueError("c and fs must be > 0, got c=%r fs=%r" % (c, fs))
    if (beta is None) == (reverberation_time is None):
        raise ValueError("give exactly one of beta and reverberation_time")
    if reverberation_time is not None:
        if not reverberation_time > 0:
            raise ValueError("reverberation_time must be > 0, got %r" % (reverberation_time,))
        beta = _sabine_beta(L, c, float(reverberation_time))
        if nsample is None:
            nsample = int(reverberation_time * fs)
    else:
        beta = [float(v) for v in np.asarray(beta, dtype=np.float64).reshape(-1)]
        if len(beta) != 6 or not all(abs(v) <= 1 for v in beta):
            raise ValueError("beta must be 6 reflection coefficients with |beta| <= 1, got %r" % (beta,))
        if nsample is None:
            raise ValueError("nsample is required with an explicit beta")
    if dim not in (2, 3):
        raise ValueError("dim must be 2 or 3, got %r" % (dim,))
    if dim == 2:
        beta[4] = beta[5] = 0.0
    if int(nsample) <= 0:
        raise ValueError("nsample must be > 0, got %r" % (nsample,))
    return L, beta, int(nsample)


def _positions(x, name, device):
    """float64 (n, 3) tensor on device from a tensor, array or list of one or more positions."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64))
    t = t.to(torch.float64)
    if t.dim() == 1:
        t = t.unsqueeze(0)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("%s must be (3,) or (n, 3) positions, got shape %s" % (name, tuple(t.shape)))
    return t.to(device).contiguous()


def _check_device(t, who):
    if not t.is_cuda:
        raise RuntimeError("%s: tensors must live on the GPU (got %s); the HIP path has no CPU fallback" % (who, t.device))


def room_impulse_responses(src, receiver, room, reverberation_time=None, beta=None, nsample=None, c=SOUND_SPEED, fs=16000,
                           order=-1, dim=3, hp_filter=True):
    """Room impulse responses, (B, nsample) float64 on the GPU, for sources src (B, 3) float64 on the GPU and one receiver (3,)
    or one per source (B, 3): the batched form of ``rir_generate``, with its keyword rules for beta / reverberation_time /
    nsample / dim.  When not inside a graph capture the source-receiver distances are checked (one host sync): a source on
    its receiver raises ValueError; inside a capture there is no check and such a pair gives an infinite response."""
    L, beta, nsample = _room_params(room, c, beta, reverberation_time, nsample, dim, fs)
    if not isinstance(src, torch.Tensor) or src.dim() != 2 or src.shape[1] != 3 or src.dtype != torch.float64:
        raise ValueError("room_impulse_responses: src must be a float64 (B, 3) tensor")
    _check_device(src, "room_impulse_responses")
    rcv = _positions(receiver, "receiver", src.device)
    if rcv.shape[0] == 1:
        rcv = rcv.expand(src.shape[0], 3).contiguous()
    elif rcv.shape[0] != src.shape[0]:
        raise ValueError("room_impulse_responses: %d receivers for %d sources" % (rcv.shape[0], src.shape[0]))
    src = src.contiguous()
    if not torch.cuda.is_current_stream_capturing() and bool((src == rcv).all(dim=1).any()):
        raise ValueError("room_impulse_responses: a source coincides with its receiver (distance 0, infinite gain)")
    return N.rir(src, rcv, L, beta, c, fs, nsample, order, hp_filter)


def array_impulse_responses(src, mics, room, **rir_kwargs):
    """Room impulse responses from every source to every microphone of an array, (B, D, nsample) float64 on the GPU: sources
    src (B, 3) and microphones mics (D, 3) (one array for every source) or (B, D, 3), float64 on the GPU.  One
    ``room_impulse_responses`` call over B D rows (its keywords: rir_kwargs), so row (b, d) is bit for bit the response that
    call gives for source b and receiver mics[b, d]."""
    if not isinstance(src, torch.Tensor) or src.dim() != 2 or src.shape[1] != 3 or src.dtype != torch.float64:
        raise ValueError("array_impulse_responses: src must be a float64 (B, 3) tensor")
    if not isinstance(mics, torch.Tensor) or mics.dim() not in (2, 3) or mics.shape[-1] != 3 or mics.dtype != torch.float64 \
            or mics.shape[-2] < 1 or (mics.dim() == 3 and mics.shape[0] != src.shape[0]):
        raise ValueError("array_impulse_responses: mics must be a float64 (D, 3) or (B, D, 3) tensor for src's B = %d"
                         % src.shape[0])
    _check_device(src, "array_impulse_responses")
    _check_device(mics, "array_impulse_responses")
    B, D = src.shape[0], mics.shape[-2]
    rcv = (mics[None] if mics.dim() == 2 else mics).expand(B, D, 3).reshape(B * D, 3)
    h = room_impulse_responses(src[:, None, :].expand(B, D, 3).reshape(B * D, 3), rcv, room, **rir_kwargs)
    return h.view(B, D, h.shape[1])


def array_spectrograms(wave, h, n_fft=N_FFT, hop=HOP):
    """What the microphones of an array record, as spectrograms: wave (B, S) float32 clean signals and h (B, D, Nh) float64
    impulse responses on the GPU -> (B, D, F, T) complex128, ``N.stft_complex(N.fir_same(wave, h))`` over the B D rows."""
    if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.dtype != torch.float32:
        raise ValueError("array_spectrograms: wave must be a float32 (B, S) tensor")
    if not isinstance(h, torch.Tensor) or h.dim() != 3 or h.dtype != torch.float64 or h.shape[0] != wave.shape[0]:
        raise ValueError("array_spectrograms: h must be a float64 (B, D, Nh) tensor for wave's B = %d" % wave.shape[0])
    _check_device(wave, "array_spectrograms")
    _check_device(h, "array_spectrograms")
    B, D, Nh = h.shape
    rows = wave[:, None, :].expand(B, D, wave.shape[1]).reshape(B * D, wave.shape[1])
    spec = N.stft_complex(N.fir_same(rows, h.reshape(B * D, Nh).contiguous()), n_fft, hop)
    return spec.view(B, D, spec.shape[1], spec.shape[2])


def rir_generate(c, fs, r, s, L, beta=None, reverberation_time=None, nsample=None, mtype="omnidirectional", order=-1, dim=3,
                 orientation=None, hp_filter=True, device="cuda"):
    """``rir_generator.generate`` on the GPU: receivers r (3,) or (M, 3), source s (3,), room L (m) -> (nsample, M) float64 on
    ``device``, the package's layout.

    Exactly one of beta (6 wall reflection coefficients, x0 x1 y0 y1 z0 z1) and reverberation_time (T60, s) is given.  From
    T60, Sabine's formula gives alpha = 24 V ln10 / (c S T60) and all six beta = +sqrt(1 - alpha) (alpha > 1 raises
    ValueError); nsample then defaults to int(T60 fs).  The sign of that beta is this package's choice: the Python package's
    own choice cannot be checked here, and negative explicit beta values (allowed) give the other convention.  With an
    explicit beta, nsample is required.  Only the omnidirectional microphone is supported: another mtype or an orientation
    raises.  dim=2 zeroes beta[4] and beta[5]; order=-1 keeps every reflection order; hp_filter applies the 100 Hz high-pass.
    """
    if str(getattr(mtype, "name", mtype)).lower() not in ("omnidirectional", "o"):
        raise ValueError("rir_generate: only the omnidirectional microphone is supported, got mtype=%r" % (mtype,))
    if orientation is not None:
        raise ValueError("rir_generate: microphone orientation is not supported (omnidirectional only)")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("rir_generate: device must be a GPU (got %s); the HIP path has no CPU fallback" % device)
    L, beta, nsample = _room_params(L, c, beta, reverberation_time, nsample, dim, fs)
    rcv = _positions(r, "r", "cpu")
    src = _positions(s, "s", "cpu")
    if src.shape[0] != 1:
        raise ValueError("rir_generate: one source position s, got %d" % src.shape[0])
    if bool((rcv == src).all(dim=1).any()):
        raise ValueError("rir_generate: the source coincides with a receiver (distance 0, infinite gain)")
    M = rcv.shape[0]
    h = N.rir(src.expand(M, 3).contiguous().to(device), rcv.to(device), L, beta, c, fs, nsample, order, hp_filter)
    return h.t()


def _ring_sources(theta, rcv, room, R, z):
    """min(rcv + (R cos theta, R sin theta, z), room): theta (B,) float64, rcv and room (1, 3) or (B, 3) float64."""
    ring = torch.stack((R * torch.cos(theta), R * torch.sin(theta), torch.full_like(theta, float(z))), dim=1)
    return torch.minimum(rcv + ring, room)


def source_positions(theta, receiver, room, R, z):
    """SpecsDataset.get_source_coordinates on the device: theta (B,) float64 -> (B, 3) float64 sources
    min(receiver + (R cos theta, R sin theta, z), room) (genereate_dataset.py:18-20).  A source on the receiver raises."""
    if not isinstance(theta, torch.Tensor):
        raise ValueError("source_positions: theta must be a tensor")
    _check_device(theta, "source_positions")
    theta = theta.reshape(-1).to(torch.float64)
    rcv = _positions(receiver, "receiver", theta.device)
    src = _ring_sources(theta, rcv, _positions(room, "room", theta.device), R, z)
    if bool((src == rcv).all(dim=1).any()):
        raise ValueError("source_positions: a source coincides with the receiver (distance 0, infinite gain)")
    return src


def generate_samples(wave, theta=None, generator=None, config=DATASET_CONFIG, c=SOUND_SPEED, scenes=None):
    """The dataset generator on the device (genereate_dataset.py:13-51, batched): wave (B, S) float32 clean speech on the GPU
    -> (speech_spec (B,F,T) fp32, rir_spec fp64, echoed_spec fp64, sample_rate int, theta (B,) fp64, wiener_est (B,F) fp64).
    theta: source directions (B,); None draws U(-pi, pi) in float64 on the device (from ``generator`` if given).  config:
    the generator's constants (``DATASET_CONFIG`` keys): source on the ring of radius R at height Z_LOC_SOURCE above the
    receiver, clipped to the room; RIR from reverberation_time with n_sample samples; STFT with NFFT / HOP_LENGTH.
    scenes: a ``Scenes`` of B items (``sample_scenes``) instead of theta: each item's room, receiver, source and beta come
    from it (config then gives fs, n_sample, NFFT and HOP_LENGTH only) and the returned theta is ``scenes.theta``."""
    if wave.dim() != 2 or wave.dtype != torch.float32:
        raise ValueError("generate_samples: wave must be float32 (B, S), got %s %s" % (wave.dtype, tuple(wave.shape)))
    if scenes is not None and theta is not None:
        raise ValueError("generate_samples: give theta or scenes, not both")
    _check_device(wave, "generate_samples")
    B = wave.shape[0]
    if scenes is not None:
        if scenes.theta.shape[0] != B:
            raise ValueError("generate_samples: %d scenes for %d waveforms" % (scenes.theta.shape[0], B))
        return _samples_from_scenes(wave, scenes, config, c, check=not torch.cuda.is_current_stream_capturing())
    if theta is None:
        theta = torch.rand(B, dtype=torch.float64, device=wave.device, generator=generator) * (2.0 * math.pi) - math.pi
    else:
        theta = torch.as_tensor(theta, dtype=torch.float64).reshape(-1).to(wave.device)
        if theta.shape[0] != B:
            raise ValueError("generate_samples: %d angles for %d waveforms" % (theta.shape[0], B))
    fs = int(config["fs"])
    src = source_positions(theta, config["receiver_position"], config["room_dimensions"], config["R"], config["Z_LOC_SOURCE"])
    h = room_impulse_responses(src, config["receiver_position"], config["room_dimensions"],
                               reverberation_time=config["reverberation_time"], nsample=config["n_sample"], c=c, fs=fs)
    speech, rir, echoed, wiener = specs_from_waveform(wave, h, n_fft=int(config["NFFT"]), hop=int(config["HOP_LENGTH"]))
    return speech, rir, echoed, fs, theta, wiener


def _samples_from_scenes(wave, scenes, config, c, check):
    fs = int(config["fs"])
    h = _scene_rirs(scenes.source, scenes.receiver, scenes.room, scenes.beta, None, int(config["n_sample"]), c, fs, -1, True,
                    check, "generate_samples")
    speech, rir, echoed, wiener = specs_from_waveform(wave, h, n_fft=int(config["NFFT"]), hop=int(config["HOP_LENGTH"]))
    return speech, rir, echoed, fs, scenes.theta, wiener


# ------------------------------------------------------------------------------------------------ scenes: a room per item
def _sabine_beta_device(room, c, reverberation_time):
    """Per item on the device: room (B, 3), reverberation_time (B,) float64 -> (alpha (B,), beta (B, 6)), all six beta
    sqrt(1 - alpha) with ``_sabine_beta``'s arithmetic; NaN where alpha > 1 (the kernel flags those items)."""
    alpha = _sabine_alpha((room[:, 0], room[:, 1], room[:, 2]), c, reverberation_time)
    return alpha, torch.sqrt(1.0 - alpha).unsqueeze(1).expand(-1, 6).contiguous()


def _scene_rirs(src, rcv, room, beta, alpha, nsample, c, fs, order, hp_filter, check, who):
    h, status = N.rir_rooms(src, rcv, room, beta, c, fs, nsample, order, hp_filter)
    if check:
        flags = [(src == rcv).all(dim=1).any(), (status != 0).any()]
        if alpha is not None:
            flags.append((alpha > 1).any())
        coincide, flagged, *over = torch.stack(flags).tolist()          # the one host sync
        if coincide:
            raise ValueError("%s: a source coincides with its receiver (distance 0, infinite gain)" % who)
        if any(over):
            raise ValueError("%s: the reflection coefficients cannot be calculated for some room and reverberation time "
                             "(alpha > 1); give beta or change the room" % who)
        if flagged:
            items = torch.nonzero(status).reshape(-1).tolist()
            raise ValueError("%s: items %s have |beta| > 1, a room side that is not a positive length, or more than 4096 "
                             "images along an axis (status %s)" % (who, items, status[items].tolist()))
    return h


def scene_impulse_responses(src, receiver, room, reverberation_time=None, beta=None, nsample=None, c=SOUND_SPEED, fs=16000,
                            order=-1, dim=3, hp_filter=True):
    """Room impulse responses with a room per item, (B, nsample) float64 on the GPU, in one launch (alvq_rir_rooms_f64).

    src (B, 3), room (B, 3) and exactly one of reverberation_time (B,) and beta (B, 6): float64 tensors on the GPU; receiver
    (3,) or (B, 3).  From reverberation_time, Sabine's beta is computed on the device with ``rir_generate``'s expression, so
    row b is bitwise ``room_impulse_responses(src[b:b+1], receiver[b], room[b], ...)``.  nsample is required (it is shared).
    Outside a graph capture, one host sync checks that no source is on its receiver, that alpha <= 1 and the kernel's per-item
    flag (|beta| <= 1, at most 4096 images along an axis) and raises ValueError otherwise; inside a capture there is no check.
    order, dim and hp_filter as in ``rir_generate``."""
    who = "scene_impulse_responses"
    if (beta is None) == (reverberation_time is None):
        raise ValueError("%s: give exactly one of beta and reverberation_time" % who)
    if nsample is None or int(nsample) <= 0:
        raise ValueError("%s: nsample must be given and > 0, got %r" % (who, nsample))
    if not (c > 0 and fs > 0):
        raise ValueError("%s: c and fs must be > 0, got c=%r fs=%r" % (who, c, fs))
    if dim not in (2, 3):
        raise ValueError("%s: dim must be 2 or 3, got %r" % (who, dim))
    for name, t in (("src", src), ("room", room)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float64:
            raise ValueError("%s: %s must be a float64 (B, 3) tensor" % (who, name))
    B = src.shape[0]
    if room.shape[0] != B:
        raise ValueError("%s: %d rooms for %d sources" % (who, room.shape[0], B))
    if reverberation_time is not None:
        t60 = reverberation_time
        if not isinstance(t60, torch.Tensor) or t60.dtype != torch.float64 or t60.reshape(-1).shape[0] != B:
            raise ValueError("%s: reverberation_time must be a float64 (B,) tensor" % who)
    else:
        if not isinstance(beta, torch.Tensor) or beta.dtype != torch.float64 or tuple(beta.shape) != (B, 6):
            raise ValueError("%s: beta must be a float64 (B, 6) tensor" % who)
    _check_device(src, who)
    _check_device(room, who)
    rcv = _positions(receiver, "receiver", src.device)
    if rcv.shape[0] == 1:
        rcv = rcv.expand(B, 3)
    elif rcv.shape[0] != B:
        raise ValueError("%s: %d receivers for %d sources" % (who, rcv.shape[0], B))
    alpha = None
    if reverberation_time is not None:
        _check_device(reverberation_time, who)
        alpha, beta = _sabine_beta_device(room, float(c), reverberation_time.reshape(-1))
    else:
        _check_device(beta, who)
    if dim == 2:
        beta = beta.clone()
        beta[:, 4:] = 0.0
    return _scene_rirs(src.contiguous(), rcv.contiguous(), room.contiguous(), beta.contiguous(), alpha, int(nsample), c, fs,
                       order, hp_filter, not torch.cuda.is_current_stream_capturing(), who)


Scenes = collections.namedtuple("Scenes", "room receiver source reverberation_time beta theta")
Scenes.__doc__ = """A batch of scenes, float64 tensors on the device: room (B, 3) m, receiver (B, 3), source (B, 3), reverberation_time
(B,) s, beta (B, 6) (Sabine's, from room and reverberation_time) and theta (B,), the source's direction seen from the receiver."""


def _range(v, name):
    lo, hi = (v, v) if np.ndim(v) == 0 else tuple(v)
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi):
        raise ValueError("SceneConfig: %s must be a positive length or a range 0 < lo <= hi, got %r" % (name, v))
    return lo, hi


class SceneConfig:
    """What ``sample_scenes`` draws from, checked when it is made (no device work): every draw is then a valid scene.

    room_dimensions: three per-axis [lo, hi] ranges in m (a number is a point); reverberation_time: [lo, hi] s.
    receiver_position: None places the receiver uniformly in the room shrunk by ``margin`` horizontally and by ``margin_z``
    below and ``Z_LOC_SOURCE + margin_z`` above; three numbers fix it.  The source follows ``source_positions``'s rule
    min(receiver + (R cos theta, R sin theta, Z_LOC_SOURCE), room), theta ~ U(-pi, pi); the checks make the clip inactive,
    so every source lies strictly inside its room and theta is its true direction (margin > R is required).  fs, n_sample,
    NFFT and HOP_LENGTH are the shared signal constants, c the sound speed.  Rejected: a room too small for the margins or
    the fixed receiver, a reverberation_time lower bound below Sabine's minimum for the largest room (alpha > 1), and a
    smallest room that needs more than 4096 images along an axis."""

    def __init__(self, room_dimensions=((3.0, 8.0), (3.0, 8.0), (3.0, 8.0)), reverberation_time=(0.25, 0.8),
                 receiver_position=None, margin=1.25, margin_z=0.5, R=1.0, Z_LOC_SOURCE=1.0, fs=16000, n_sample=6400,
                 NFFT=N_FFT, HOP_LENGTH=HOP, c=SOUND_SPEED):
        if len(room_dimensions) != 3:
            raise ValueError("SceneConfig: room_dimensions needs three ranges, got %r" % (room_dimensions,))
        self.room = tuple(_range(v, "room_dimensions[%d]" % a) for a, v in enumerate(room_dimensions))
        self.reverberation_time = _range(reverberation_time, "reverberation_time")
        self.R, self.z, self.c = float(R), float(Z_LOC_SOURCE), float(c)
        self.fs, self.n_sample, self.NFFT, self.HOP_LENGTH = int(fs), int(n_sample), int(NFFT), int(HOP_LENGTH)
        if not (self.R > 0 and math.isfinite(self.R) and self.z >= 0 and math.isfinite(self.z)):
            raise ValueError("SceneConfig: need R > 0 and Z_LOC_SOURCE >= 0, got %r and %r" % (R, Z_LOC_SOURCE))
        if not (self.c > 0 and self.fs > 0 and self.n_sample > 0):
            raise ValueError("SceneConfig: c, fs and n_sample must be > 0")
        lo = [r[0] for r in self.room]
        if receiver_position is None:
            self.receiver, self.margin, self.margin_z = None, float(margin), float(margin_z)
            if not (self.margin > self.R and self.margin_z > 0):
                raise ValueError("SceneConfig: need margin > R (%g) and margin_z > 0, got %r and %r" % (self.R, margin, margin_z))
            if lo[0] < 2 * self.margin or lo[1] < 2 * self.margin or lo[2] < self.z + 2 * self.margin_z:
                raise ValueError("SceneConfig: the smallest room %s leaves no place for the receiver (horizontal margin %g, "
                                 "height margin %g + Z_LOC_SOURCE %g)" % (lo, self.margin, self.margin_z, self.z))
        else:
            self.receiver = tuple(float(v) for v in receiver_position)
            self.margin = self.margin_z = None
            x, y, zr = self.receiver
            if len(self.receiver) != 3 or not (self.R < x and x + self.R < lo[0] and self.R < y and y + self.R < lo[1]
                                               and 0 < zr and zr + self.z < lo[2]):
                raise ValueError("SceneConfig: receiver %r with R %g and Z_LOC_SOURCE %g puts a source outside the smallest "
                                 "room %s" % (receiver_position, self.R, self.z, lo))
        hi = [r[1] for r in self.room]
        alpha = _sabine_alpha(hi, self.c, self.reverberation_time[0])
        if not alpha <= 1.0 - 1e-9:         # alpha grows with every side: the largest room at the lowest T60 is the worst
            raise ValueError("SceneConfig: reverberation_time %g is below Sabine's minimum for the largest room %s (alpha = %g)"
                             % (self.reverberation_time[0], hi, alpha))
        cTs = self.c / self.fs
        if max(math.ceil(self.n_sample / (2.0 * (v / cTs))) for v in lo) > 4096:
            raise ValueError("SceneConfig: n_sample %d needs more than 4096 images along an axis of the room %s"
                             % (self.n_sample, lo))

    @classmethod
    def from_dataset_config(cls, config=DATASET_CONFIG, c=SOUND_SPEED):
        """The degenerate config: every range the point ``config`` holds (by default the generator's one room)."""
        return cls(room_dimensions=[float(v) for v in config["room_dimensions"]],
                   reverberation_time=float(config["reverberation_time"]), receiver_position=config["receiver_position"],
                   R=config["R"], Z_LOC_SOURCE=config["Z_LOC_SOURCE"], fs=config["fs"], n_sample=config["n_sample"],
                   NFFT=config["NFFT"], HOP_LENGTH=config["HOP_LENGTH"], c=c)

    def _tensors(self, device):
        """The ranges as float64 tensors on device, made once per device (so that a draw copies nothing from the host)."""
        cache = self.__dict__.setdefault("_cache", {})
        if device not in cache:
            f64 = dict(dtype=torch.float64, device=device)
            lo = torch.tensor([r[0] for r in self.room], **f64)
            t = {"lo": lo, "span": torch.tensor([r[1] for r in self.room], **f64) - lo}
            if self.receiver is None:
                t["margin"] = torch.tensor([self.margin, self.margin, self.margin_z], **f64)
                t["reserve"] = torch.tensor([2.0 * self.margin, 2.0 * self.margin, 2.0 * self.margin_z + self.z], **f64)
            else:
                t["receiver"] = torch.tensor(self.receiver, **f64)[None]
            cache[device] = t
        return cache[device]

    def signal_config(self):
        """The shared constants under ``DATASET_CONFIG``'s key names, as ``generate_samples`` reads them."""
        return {"fs": self.fs, "n_sample": self.n_sample, "NFFT": self.NFFT, "HOP_LENGTH": self.HOP_LENGTH}


def sample_scenes(B, config, generator=None, device=None):
    """B scenes drawn from a ``SceneConfig``, as a ``Scenes``; no host sync.  One (B, 8) float64 uniform draw from
    ``generator`` (whose device is used; else ``device``, default cuda; plain tensor arithmetic, so a CPU generator works
    too, for inspection): room sides lo + u (hi - lo), T60 likewise, the
    receiver (unless fixed) and theta = u * 2 pi - pi, ``generate_samples``'s expression."""
    if not isinstance(config, SceneConfig):
        raise ValueError("sample_scenes: config must be a SceneConfig")
    B = int(B)
    if B <= 0:
        raise ValueError("sample_scenes: B must be > 0, got %r" % (B,))
    device = torch.device(generator.device if generator is not None else (device or "cuda"))
    t = config._tensors(device)
    u = torch.rand((B, 8), generator=generator, dtype=torch.float64, device=device)
    room = t["lo"] + u[:, 0:3] * t["span"]
    t_lo, t_hi = config.reverberation_time
    t60 = t_lo + u[:, 3] * (t_hi - t_lo)
    if config.receiver is None:
        rcv = t["margin"] + u[:, 4:7] * (room - t["reserve"])
    else:
        rcv = t["receiver"].expand(B, 3)
    theta = u[:, 7] * (2.0 * math.pi) - math.pi
    src = _ring_sources(theta, rcv, room, config.R, config.z)
    _, beta = _sabine_beta_device(room, config.c, t60)
    return Scenes(room, rcv.contiguous(), src, t60, beta, theta)


def write_specs_dataset(dest, samples, config=DATASET_CONFIG, start=0):
    """Write ``generate_samples`` output as the generator does (genereate_dataset.py:97-103): {start+i}.pt 6-tuples
    ((201,T) fp32 / fp64 / fp64 powers, int rate, (1,) fp64 theta, (201,) fp64 Wiener estimate) and dataset_config.npy (a
    pickled dict), so that SpecsDataset and spec_dataset_preprocessing read them unchanged.  Returns the written paths."""
    speech, rir, echoed, fs, theta, wiener = samples
    os.makedirs(dest, exist_ok=True)
    speech, rir, echoed, theta, wiener = (t.detach().cpu() for t in (speech, rir, echoed, theta, wiener))
    paths = []
    for i in range(speech.shape[0]):
        path = os.path.join(dest, "%d.pt" % (start + i))
        torch.save((speech[i].clone(), rir[i].clone(), echoed[i].clone(), int(fs), theta[i].reshape(1).clone(),
                    wiener[i].clone()), path)
        paths.append(path)
    np.save(os.path.join(dest, "dataset_config.npy"), dict(config))
    return paths
