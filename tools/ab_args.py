"""The error surface of the signal and array modules, and of the ``_native`` wrappers below them, as text: one line per bad
call -- function | case | exception type | message.  Run it on two trees and ``diff`` the outputs; a refactor of the argument
rules must leave every line unchanged.  No GPU is needed and nothing is launched: every call ends in an exception on the
host (the workspace-size entry points of libalvq.so are host code), and the last call of every function passes correct CPU
tensors, which must reach its "must live on the GPU" line.

    python tools/ab_args.py > head.txt
    PYTHONPATH=<other tree>/acoustic_locating_vq-vae_amd/src ALVQ_LIB=<a libalvq.so> python tools/ab_args.py > parent.txt

Only public names are imported (modules, functions, and ``_native``'s wrappers), so the same file runs against either tree; a
package found on PYTHONPATH wins over this tree's.  For each function the cases follow the order of its checks, and a case
named ``a + b`` breaks two rules at once: the message tells which check comes first.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "acoustic_locating_vq-vae_amd", "src"))
import torch  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import beamforming as BF, dereverberation as DR, front_end as FE, kmeans as KM  # noqa: E402
from acoustic_locating_vq_vae import localization as LOC, room_acoustics as RA, separation as SEP  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as SM, subspace as SUB, tsne as TS  # noqa: E402

C64, C128, F32, F64, I32, I64 = torch.complex64, torch.complex128, torch.float32, torch.float64, torch.int32, torch.int64
INF, NAN = float("inf"), float("nan")


def z(dtype, *shape):
    return torch.zeros(shape, dtype=dtype)


def many(n):
    """(n, 3) float64 positions that take no memory."""
    return z(F64, 1, 3).expand(n, 3)


def sweep(label, fn, good, cases):
    """``fn(**good)`` with each case's arguments replaced, in the order given; then ``good`` itself, on the CPU."""
    for case, changed in list(cases) + [("cpu tensors", {})]:
        try:
            fn(**dict(good, **changed))
            outcome = "no exception"
        except Exception as e:  # noqa: BLE001 -- the exception is the output
            outcome = "%s | %s" % (type(e).__name__, e)
        print("%s | %s | %s" % (label, case, outcome))


# ------------------------------------------------------------------------------------------------------------- localization
B, D, F, T, NFFT = 2, 3, 5, 4, 8
SPEC, MICS, CAND = z(C128, B, D, F, T), z(F64, D, 3), z(F64, 6, 3)
SPEC_CASES = [("spec None", dict(spec=None)), ("spec 2-d", dict(spec=z(C128, F, T))),
      ("spec float64", dict(spec=z(F64, B, D, F, T))),
              ("T = 0", dict(spec=z(C128, B, D, F, 0))), ("T = 65536", dict(spec=z(C128, 1, 1, 1, 1).expand(1, D, 1, 65536))),
              ("B F = 2^31", dict(spec=z(C128, 1, 1, 1, 1).expand(32768, D, 65536, 1)))]
D_LOW, D_HIGH = ("D = 1", dict(spec=z(C128, B, 1, F, T))), ("D = 9", dict(spec=z(C128, B, 9, F, T)))
NFFT_CASES = [("n_fft True", dict(n_fft=True)), ("n_fft 1", dict(n_fft=1)), ("n_fft 2.0", dict(n_fft=2.0)),
      ("n_fft 16", dict(n_fft=16))]
BAND_CASES = [("band (1,)", dict(band=(1,))), ("band 'ab'", dict(band="ab")), ("band (-1, 2)", dict(band=(-1, 2))),
              ("band (3, 1)", dict(band=(3, 1))), ("band (0, 5)", dict(band=(0, 5))), ("band (0, 1.0)", dict(band=(0, 1.0)))]
RATE_CASES = [("fs 0", dict(fs=0)), ("fs inf", dict(fs=INF)), ("fs '16000'", dict(fs="16000")), ("fs True", dict(fs=True)),
              ("c nan", dict(c=NAN)), ("c -1", dict(c=-1.0))]
GEOMETRY_CASES = [("mics float32", dict(mics=z(F32, D, 3))), ("mics list", dict(mics=[[0.0] * 3] * D)),
      ("mics (D, 2)", dict(mics=z(F64, D, 2))),
                  ("mics 3 items", dict(mics=z(F64, 3, D, 3))), ("mics 2 rows", dict(mics=z(F64, 2, 3))),
                  ("candidates 1-d", dict(candidates=z(F64, 3))), ("candidates 3 items", dict(candidates=z(F64, 3, 6, 3))),
                  ("candidates 0 rows", dict(candidates=z(F64, 0, 3))), ("B G = 2^31", dict(candidates=many(1 << 30))),
                  ("mics float32 + candidates 1-d", dict(mics=z(F32, D, 3), candidates=z(F64, 3)))]

sweep("localization.cross_spectra", LOC.cross_spectra, dict(spec=SPEC, band=None),
      SPEC_CASES + [D_LOW, D_HIGH, ("default band, F = 2", dict(spec=z(C128, B, D, 2, T)))] + BAND_CASES
      + [("spec float64 + band (1,)", dict(spec=z(F64, B, D, F, T), band=(1,))), ("3-d spec", dict(spec=z(C128, D, F, T)))])
sweep("localization.gcc_phat", LOC.gcc_phat, dict(spec=SPEC, max_lag=2, band=None, n_fft=NFFT),
      SPEC_CASES + [D_LOW] + NFFT_CASES + [("max_lag -1", dict(max_lag=-1)), ("max_lag 5", dict(max_lag=5)),
      ("max_lag 1.0", dict(max_lag=1.0))]
      + BAND_CASES + [("n_fft 16 + max_lag -1", dict(n_fft=16, max_lag=-1)), ("max_lag 5 + band (1,)", dict(max_lag=5, band=(1,)))])
sweep("localization.tdoa", LOC.tdoa, dict(spec=SPEC, max_lag=2, fs=16000, band=None, n_fft=NFFT),
      RATE_CASES[:4] + [("fs 0 + spec None", dict(fs=0, spec=None)), ("max_lag 5", dict(max_lag=5))])
SRP = dict(spec=SPEC, mics=MICS, candidates=CAND, fs=16000, n_fft=NFFT, c=343.0, band=None)
sweep("localization.srp_phat", LOC.srp_phat, SRP,
      SPEC_CASES + [D_LOW, D_HIGH] + NFFT_CASES + RATE_CASES + BAND_CASES + GEOMETRY_CASES
      + [("fs 0 + n_fft 16", dict(fs=0, n_fft=16)), ("c nan + band (1,)", dict(c=NAN, band=(1,))),
         ("band (1,) + mics float32", dict(band=(1,), mics=z(F32, D, 3))),
         ("3-d spec, mics 3-d", dict(spec=SPEC[0], mics=z(F64, 2, D, 3)))])
N_SOURCES = [("n_sources 0", dict(n_sources=0)), ("n_sources D", dict(n_sources=D)), ("n_sources 1.0", dict(n_sources=1.0))]
sweep("localization.music", LOC.music, dict(SRP, n_sources=1),
      SPEC_CASES + [D_LOW] + NFFT_CASES + N_SOURCES + RATE_CASES + BAND_CASES + GEOMETRY_CASES
      + [("n_fft 16 + n_sources 0", dict(n_fft=16, n_sources=0)), ("n_sources 0 + fs 0", dict(n_sources=0, fs=0))])
COV = z(C128, B, F, D, D)
sweep("localization.music_from_covariance", LOC.music_from_covariance,
      dict(cov=COV, mics=MICS, candidates=CAND, n_sources=1, fs=16000, n_fft=NFFT, c=343.0, band=None),
      [("cov None", dict(cov=None)), ("cov 2-d", dict(cov=z(C128, D, D))), ("cov complex64", dict(cov=z(C64, B, F, D, D))),
       ("cov not square", dict(cov=z(C128, B, F, D, 2))), ("D = 1", dict(cov=z(C128, B, F, 1, 1))),
       ("D = 9", dict(cov=z(C128, B, F, 9, 9))),
       ("B = 0", dict(cov=z(C128, 0, F, D, D))), ("B F = 2^31", dict(cov=z(C128, 1, 1, 1, 1).expand(32768, 65536, D, D)))]
      + NFFT_CASES + N_SOURCES + RATE_CASES + BAND_CASES + GEOMETRY_CASES
      + [("cov not square + n_fft 1", dict(cov=z(C128, B, F, D, 2), n_fft=1)), ("3-d cov", dict(cov=COV[0]))])
sweep("localization.ring_candidates", LOC.ring_candidates,
      dict(n_angles=8, receiver=[1.0, 1.0, 1.0], room=[4.0, 5.0, 3.0], R=1.0, z=0.0, device="cpu"),
      [("n_angles 0", dict(n_angles=0)), ("n_angles 2.0", dict(n_angles=2.0)), ("n_angles 2^31", dict(n_angles=2 ** 31))])
sweep("localization.locate_on_ring", LOC.locate_on_ring,
      dict(spec=SPEC, mics=MICS, receiver=[1.0, 1.0, 1.0], room=[4.0, 5.0, 3.0], R=1.0, z=0.0, n_angles=8, method="srp", n_sources=1),
      [("spec None", dict(spec=None)), ("method 'gcc'", dict(method="gcc")), ("srp with n_sources 2", dict(n_sources=2)),
       ("spec None + method 'gcc'", dict(spec=None, method="gcc")), ("method music", dict(method="music"))])

# -------------------------------------------------------------------------------------------------------------- beamforming
SRC, MASK = z(F64, B, 3), z(F64, B, F, T)
BF_SPEC_CASES = SPEC_CASES + [("D = 0", dict(spec=z(C128, B, 0, F, T))), D_HIGH]
STEER_KW = NFFT_CASES[:3] + RATE_CASES + [("ref -1", dict(ref=-1)), ("ref D", dict(ref=D)), ("ref 0.0", dict(ref=0.0))]
LOADING = [("loading -1", dict(loading=-1.0)), ("loading nan", dict(loading=NAN)), ("loading '0'", dict(loading="0")),
           ("loading True", dict(loading=True))]
sweep("beamforming.steering_vectors", BF.steering_vectors, dict(mics=MICS, source=SRC, F=F, fs=16000, n_fft=NFFT, c=343.0, ref=0),
      [("mics None", dict(mics=None)), ("mics 1-d", dict(mics=z(F64, 3))), ("mics (D, 2)", dict(mics=z(F64, D, 2))),
      ("mics float32", dict(mics=z(F32, D, 3))),
       ("source None", dict(source=None)), ("source 3-d", dict(source=z(F64, B, 1, 3))),
       ("source float32", dict(source=z(F32, B, 3))),
       ("mics 3 items", dict(mics=z(F64, 3, D, 3))), ("D = 0", dict(mics=z(F64, 0, 3))), ("D = 9", dict(mics=z(F64, 9, 3))),
       ("F 0", dict(F=0)), ("F 5.0", dict(F=5.0)), ("B = 0", dict(source=z(F64, 0, 3))),
       ("B F = 2^31", dict(source=many(32768), F=65536))]
      + STEER_KW + [("mics float32 + source None", dict(mics=z(F32, D, 3), source=None)), ("F 0 + fs 0", dict(F=0, fs=0)),
                    ("fs 0 + ref D", dict(fs=0, ref=D)), ("no batch", dict(source=z(F64, 3))),
                    ("mics 3-d", dict(mics=z(F64, B, D, 3)))])
MASK_CASES = [("mask float32", dict(mask=z(F32, B, F, T))), ("mask (F, T)", dict(mask=z(F64, F, T))),
      ("mask list", dict(mask=[1.0]))]
sweep("beamforming.spatial_covariance", BF.spatial_covariance, dict(spec=SPEC, mask=MASK),
      BF_SPEC_CASES + MASK_CASES + [("spec float64 + mask float32", dict(spec=z(F64, B, D, F, T), mask=z(F32, B, F, T))),
                                    ("3-d spec, 3-d mask", dict(spec=SPEC[0])), ("no mask", dict(mask=None)),
                                    ("3-d spec", dict(spec=SPEC[0], mask=MASK[0]))])
STEER = z(C128, B, D, F)
sweep("beamforming.weights", BF.weights, dict(method="mvdr", noise_cov=COV, steering=STEER, speech_cov=None, ref=0, loading=1e-6),
      [("method 'gev'", dict(method="gev")), ("method None", dict(method=None)), ("mvdr without noise_cov", dict(noise_cov=None)),
       ("mvdr with speech_cov", dict(speech_cov=COV)), ("noise_cov complex64", dict(noise_cov=z(C64, B, F, D, D))),
       ("steering 4-d", dict(steering=z(C128, B, D, F, 1))),
       ("batch mismatch", dict(steering=STEER[0])), ("noise_cov shape", dict(noise_cov=z(C128, B, F, D, 2))),
       ("D = 9", dict(noise_cov=z(C128, B, F, 9, 9), steering=z(C128, B, 9, F))),
       ("B = 0", dict(noise_cov=z(C128, 0, F, D, D), steering=z(C128, 0, D, F))), ("ref D", dict(ref=D)),
       ("ref True", dict(ref=True))] + LOADING
      + [("das", dict(method="das", noise_cov=None)), ("das with noise_cov", dict(method="das")),
         ("souden", dict(method="souden", steering=None, speech_cov=COV)),
         ("souden speech_cov shape", dict(method="souden", steering=None, speech_cov=z(C128, B, F, 2, 2))),
         ("ref D + loading -1", dict(ref=D, loading=-1.0)),
         ("D = 9 + ref -1", dict(noise_cov=z(C128, B, F, 9, 9), steering=z(C128, B, 9, F), ref=-1)),
         ("no batch", dict(noise_cov=COV[0], steering=STEER[0]))])
W = z(C128, B, F, D)
sweep("beamforming.apply", BF.apply, dict(spec=SPEC, w=W),
      BF_SPEC_CASES + [("w None", dict(w=None)), ("w complex64", dict(w=z(C64, B, F, D))), ("w (F, D)", dict(w=W[0])),
                       ("spec None + w None", dict(spec=None, w=None)), ("3-d spec", dict(spec=SPEC[0], w=W[0]))])
GEO_CASES = [("mics None", dict(mics=None)), ("mics float32", dict(mics=z(F32, D, 3))), ("mics 2 rows", dict(mics=z(F64, 2, 3))),
             ("mics 3 items", dict(mics=z(F64, 3, D, 3))), ("source None", dict(source=None)),
             ("source float32", dict(source=z(F32, B, 3))),
             ("source 3 items", dict(source=z(F64, 3, 3)))]
DAS = dict(spec=SPEC, mics=MICS, source=SRC, fs=16000, n_fft=NFFT, c=343.0, ref=0)
sweep("beamforming.delay_and_sum", BF.delay_and_sum, DAS,
      BF_SPEC_CASES + GEO_CASES + STEER_KW + [("3-d spec, 3-d mics", dict(spec=SPEC[0], mics=z(F64, B, D, 3))),
      ("3-d spec, 2-d source", dict(spec=SPEC[0])),
                                              ("mics float32 + fs 0", dict(mics=z(F32, D, 3), fs=0)),
                                              ("source None + ref D", dict(source=None, ref=D)),
                                              ("3-d spec", dict(spec=SPEC[0], source=SRC[0])),
                                              ("mics 3-d", dict(mics=z(F64, B, D, 3)))])
MVDR = dict(DAS, noise_mask=None, speech_mask=None, loading=1e-6)
MVDR_CASES = [("mics without source", dict(source=None)), ("source without mics", dict(mics=None)),
      ("geometry with speech_mask", dict(speech_mask=MASK)),
              ("no geometry, no masks", dict(mics=None, source=None)),
              ("no geometry, one mask", dict(mics=None, source=None, noise_mask=MASK)),
              ("noise_mask float32", dict(noise_mask=z(F32, B, F, T))), ("noise_mask (F, T)", dict(noise_mask=MASK[0])),
              ("speech_mask float32", dict(mics=None, source=None, noise_mask=MASK, speech_mask=z(F32, B, F, T))),
              ("ref D", dict(ref=D))] + LOADING + GEO_CASES[1:4] + GEO_CASES[5:] \
    + NFFT_CASES[:3] + RATE_CASES + [("noise_mask float32 + ref D", dict(noise_mask=z(F32, B, F, T), ref=D)),
    ("loading -1 + mics float32", dict(loading=-1.0, mics=z(F32, D, 3))),
                                     ("ref D + fs 0", dict(ref=D, fs=0)), ("noise mask", dict(noise_mask=MASK)),
                                     ("souden", dict(mics=None, source=None, noise_mask=MASK, speech_mask=MASK))]
sweep("beamforming.mvdr", BF.mvdr, MVDR, BF_SPEC_CASES + MVDR_CASES + [("3-d spec", dict(spec=SPEC[0], source=SRC[0]))])
sweep("beamforming.gev_weights", BF.gev_weights, dict(noise_cov=COV, speech_cov=COV, ref=0, loading=1e-6),
      [("noise_cov None", dict(noise_cov=None)), ("noise_cov 2-d", dict(noise_cov=z(C128, D, D))),
      ("speech_cov complex64", dict(speech_cov=z(C64, B, F, D, D))),
       ("batch mismatch", dict(speech_cov=COV[0])), ("noise_cov not square", dict(noise_cov=z(C128, B, F, D, 2))),
       ("speech_cov shape", dict(speech_cov=z(C128, B, F, 2, 2))),
       ("D = 9", dict(noise_cov=z(C128, B, F, 9, 9), speech_cov=z(C128, B, F, 9, 9))),
       ("B = 0", dict(noise_cov=z(C128, 0, F, D, D), speech_cov=z(C128, 0, F, D, D))),
       ("ref D", dict(ref=D))] + LOADING + [("ref D + loading -1", dict(ref=D, loading=-1.0)),
       ("no batch", dict(noise_cov=COV[0], speech_cov=COV[0]))])
sweep("beamforming.gev", BF.gev, dict(spec=SPEC, noise_mask=MASK, speech_mask=MASK, ref=0, loading=1e-6),
      BF_SPEC_CASES + [("noise_mask None", dict(noise_mask=None)), ("noise_mask float32", dict(noise_mask=z(F32, B, F, T))),
      ("speech_mask (F, T)", dict(speech_mask=MASK[0])),
                       ("ref D", dict(ref=D))] + LOADING + [("speech_mask (F, T) + ref D", dict(speech_mask=MASK[0], ref=D)),
                                                            ("3-d spec", dict(spec=SPEC[0], noise_mask=MASK[0], speech_mask=MASK[0]))])
sweep("beamforming.locate_and_beamform", BF.locate_and_beamform,
      dict(spec=SPEC, mics=MICS, candidates=CAND, ref=0, loading=1e-6, fs=16000, n_fft=NFFT, c=343.0, band=None),
      [D_LOW, ("fs 0", dict(fs=0)), ("candidates 1-d", dict(candidates=z(F64, 3))), ("ref D", dict(ref=D))])
S = 16
WAVES, WMASK = z(F32, B, D, S), z(F64, B, NFFT // 2 + 1, 1 + S // 4)
BW = dict(waves=WAVES, mics=MICS, source=SRC, method="mvdr", noise_mask=None, speech_mask=None, ref=0, loading=1e-6, fs=16000, n_fft=NFFT, hop=4, c=343.0)
WAVE_CASES = [("waves None", dict(waves=None)), ("waves 2-d", dict(waves=z(F32, B, S))),
      ("waves int32", dict(waves=z(I32, B, D, S)))]
WAVE_DIMS = [("B = 0", dict(waves=z(F32, 0, D, S))), ("D = 9", dict(waves=z(F32, B, 9, S))),
      ("S = 0", dict(waves=z(F32, B, D, 0)))] + NFFT_CASES[:3] \
    + [("hop 0", dict(hop=0)), ("hop 9", dict(hop=9)), ("T = 65536", dict(waves=z(F32, 1, 1, 1).expand(1, D, 65535 * 4)))]
sweep("beamforming.beamform_waves", BF.beamform_waves, BW,
      WAVE_CASES + [("method 'gev'", dict(method="gev")), ("das with a mask", dict(method="das", noise_mask=WMASK))] + WAVE_DIMS
      + [(n, dict(c, **{k: WMASK for k in ("noise_mask", "speech_mask") if c.get(k) is MASK})) for n, c in MVDR_CASES[:5] + MVDR_CASES[8:-2]]
      + [("das mics float32", dict(method="das", mics=z(F32, D, 3))), ("das ref D", dict(method="das", ref=D)),
      ("waves 2-d + method 'gev'", dict(waves=z(F32, B, S), method="gev")),
         ("hop 0 + ref D", dict(hop=0, ref=D)), ("das", dict(method="das")),
         ("souden", dict(mics=None, source=None, noise_mask=WMASK, speech_mask=WMASK))])

# ----------------------------------------------------------------------------------------------------------------- subspace
sweep("subspace.eigh", SUB.eigh, dict(cov=COV),
      [("cov None", dict(cov=None)), ("cov 1-d", dict(cov=z(C128, D))), ("cov complex64", dict(cov=z(C64, B, F, D, D))),
      ("not square", dict(cov=z(C128, B, D, 2))),
       ("D = 0", dict(cov=z(C128, B, 0, 0))), ("D = 9", dict(cov=z(C128, B, 9, 9))), ("no matrices", dict(cov=z(C128, 0, D, D))),
       ("2^31 matrices", dict(cov=z(C128, 1, 1, 1, 1).expand(32768, 65536, D, D))),
       ("cov complex64 + not square", dict(cov=z(C64, B, D, 2))), ("one matrix", dict(cov=COV[0, 0]))])

# --------------------------------------------------------------------------------------------------------------- separation
ITER = [("iterations -1", dict(iterations=-1)), ("iterations 257", dict(iterations=257)), ("iterations 2.0", dict(iterations=2.0))]
W0_CASES = [("w0 complex64", dict(w0=z(C64, B, F, D, D))), ("w0 (F, D, D)", dict(w0=COV[0])), ("w0 list", dict(w0=[1.0]))]
sweep("separation.auxiva", SEP.auxiva, dict(spec=SPEC, iterations=2, model="laplace", ref=0, eps=1e-10, w0=COV),
      BF_SPEC_CASES + ITER + [("model 'cauchy'", dict(model="cauchy")), ("model 0", dict(model=0)), ("ref D", dict(ref=D)),
      ("eps -1", dict(eps=-1.0)), ("eps nan", dict(eps=NAN))]
      + W0_CASES + [("iterations -1 + model 0", dict(iterations=-1, model=0)), ("eps -1 + w0 list", dict(eps=-1.0, w0=[1.0])),
      ("no w0", dict(w0=None)),
                    ("3-d spec", dict(spec=SPEC[0], w0=COV[0]))])
L = 2
BASIS, ACT = z(F64, B, D, F, L), z(F64, B, D, L, T)
sweep("separation.ilrma", SEP.ilrma, dict(spec=SPEC, basis0=BASIS, activations0=ACT, iterations=2, ref=0, floor=1e-10, w0=COV),
      BF_SPEC_CASES + [("basis0 None", dict(basis0=None)), ("basis0 float32", dict(basis0=z(F32, B, D, F, L))),
      ("basis0 3-d", dict(basis0=BASIS[0])),
                       ("basis0 shape", dict(basis0=z(F64, B, D, 2, L))), ("L = 0", dict(basis0=z(F64, B, D, F, 0))),
                       ("L = 17", dict(basis0=z(F64, B, D, F, 17))),
                       ("activations0 float32", dict(activations0=z(F32, B, D, L, T))),
                       ("activations0 shape", dict(activations0=z(F64, B, D, 3, T)))]
      + ITER + [("ref D", dict(ref=D)), ("floor 0", dict(floor=0)), ("floor inf", dict(floor=INF))] + W0_CASES
      + [("basis0 float32 + iterations -1", dict(basis0=z(F32, B, D, F, L), iterations=-1)),
      ("floor 0 + w0 list", dict(floor=0, w0=[1.0])),
         ("3-d spec", dict(spec=SPEC[0], basis0=BASIS[0], activations0=ACT[0], w0=COV[0]))])
sweep("separation.nmf_init", SEP.nmf_init, dict(B=B, D=D, F=F, T=T, bases=2, generator=None, device="cpu"),
      [("B 0", dict(B=0)), ("B 65536", dict(B=65536)), ("D 9", dict(D=9)), ("F 2.0", dict(F=2.0)), ("T 65536", dict(T=65536)),
      ("bases 17", dict(bases=17)),
       ("B 0 + bases 17", dict(B=0, bases=17))])
sweep("separation.masks", SEP.masks, dict(sep_spec=SPEC), [(n, dict(sep_spec=c["spec"])) for n, c in BF_SPEC_CASES] + [("3-d",
      dict(sep_spec=SPEC[0]))])
sweep("separation.reorder", SEP.reorder, dict(x=SPEC, perm=z(I32, B, D)),
      [("perm None", dict(perm=None)), ("perm float32", dict(perm=z(F32, B, D))), ("perm 3-d", dict(perm=z(I32, B, D, 1))),
      ("x None", dict(x=None)), ("x 1-d", dict(x=z(F32, B))),
       ("K = 0", dict(perm=z(I32, B, 0))), ("B mismatch", dict(perm=z(I32, 3, D))),
       ("perm None + x None", dict(perm=None, x=None)), ("no batch", dict(x=SPEC[0], perm=z(I64, D)))])
sweep("separation.separate_waves", SEP.separate_waves,
      dict(waves=WAVES, iterations=2, model="laplace", ref=0, n_fft=NFFT, hop=4, method="auxiva", bases=2, generator=None),
      [("method 'ica'", dict(method="ica")),
      ("ilrma with a model", dict(method="ilrma", model="gauss"))] + WAVE_CASES + WAVE_DIMS + ITER
      + [("model 'cauchy'", dict(model="cauchy")), ("ref D", dict(ref=D)), ("bases 0", dict(bases=0)),
      ("generator 1", dict(generator=1)),
         ("method 'ica' + waves None", dict(method="ica", waves=None)), ("hop 0 + iterations -1", dict(hop=0, iterations=-1)),
         ("ilrma", dict(method="ilrma"))])
K = 2
INIT = z(F64, B, K, F, T)
sweep("separation.cacgmm", SEP.cacgmm, dict(spec=SPEC, init=INIT, iterations=2, quadratic0=INIT, floor=1e-10),
      BF_SPEC_CASES + [D_LOW, ("init None", dict(init=None)), ("init float32", dict(init=z(F32, B, K, F, T))),
      ("init 3-d", dict(init=INIT[0])), ("init B", dict(init=z(F64, 3, K, F, T))),
                       ("init F", dict(init=z(F64, B, K, 2, T))), ("init T", dict(init=z(F64, B, K, F, 3))),
                       ("K = 0", dict(init=z(F64, B, 0, F, T), quadratic0=None)),
                       ("K = 9", dict(init=z(F64, B, 9, F, T), quadratic0=None)),
                       ("quadratic0 K", dict(quadratic0=z(F64, B, 3, F, T))),
                       ("quadratic0 float32", dict(quadratic0=z(F32, B, K, F, T))),
                       ("iterations 0", dict(iterations=0))] + ITER[1:] + [("floor -1", dict(floor=-1.0)),
                       ("floor nan", dict(floor=NAN)), ("floor 2", dict(floor=2.0)),
                                                                             ("D = 1 + init None", dict(spec=z(C128, B, 1, F, T), init=None)),
                                                                             ("init None + iterations 0", dict(init=None, iterations=0)),
                                                                             ("iterations 0 + floor 2", dict(iterations=0, floor=2.0)),
                                                                             ("init with F = 1", dict(init=z(F64, B, K, 1, T), quadratic0=None)),
                                                                             ("3-d spec", dict(spec=SPEC[0], init=INIT[0], quadratic0=INIT[0]))])
sweep("separation.time_masks", SEP.time_masks, dict(B=B, K=K, F=F, T=T, generator=None, device="cpu"),
      [("B 0", dict(B=0)), ("K 9", dict(K=9)), ("F True", dict(F=True)), ("T 65536", dict(T=65536)), ("B 0 + K 9", dict(B=0, K=9))])
PERM = z(I32, B, F, K)
ROW_CASES = [("None", None), ("2-d", z(F64, F, T)), ("int32", z(I32, B, K, F, T)), ("B = 0", z(F64, 0, K, F, T)),
      ("K = 9", z(F64, B, 9, F, T)),
             ("T = 65536", z(F64, 1, 1, 1, 1).expand(1, K, 1, 65536)),
             ("B F = 2^31", z(F64, 1, 1, 1, 1).expand(32768, K, 65536, 1))]
sweep("separation.align_permutations", SEP.align_permutations, dict(profile=INIT, iterations=2, perm0=PERM),
      [("profile " + n, dict(profile=t)) for n, t in ROW_CASES] + [("profile float32", dict(profile=z(F32, B, K, F, T))),
      ("T = 1", dict(profile=z(F64, B, K, F, 1))), ("iterations 0", dict(iterations=0))]
      + ITER[1:] + [("perm0 int64", dict(perm0=z(I64, B, F, K))), ("perm0 (F, K)", dict(perm0=PERM[0])),
      ("T = 1 + iterations 0", dict(profile=z(F64, B, K, F, 1), iterations=0)),
                    ("iterations 0 + perm0 int64", dict(iterations=0, perm0=z(I64, B, F, K))), ("no perm0", dict(perm0=None)),
                    ("3-d profile", dict(profile=INIT[0], perm0=PERM[0]))])
sweep("separation.permute_bins", SEP.permute_bins, dict(x=INIT, perm=PERM),
      [("x " + n, dict(x=t)) for n, t in ROW_CASES] + [("perm None", dict(perm=None)), ("perm int64", dict(perm=z(I64, B, F, K))),
      ("perm (B, K, F)", dict(perm=z(I32, B, K, F))),
                                                      ("x None + perm None", dict(x=None, perm=None)),
                                                      ("complex x", dict(x=z(C64, B, K, F, T))),
                                                      ("3-d x", dict(x=INIT[0], perm=PERM[0]))])
sweep("separation.permute_rows", SEP.permute_rows, dict(a=z(C128, B, F, K, K), perm=PERM),
      [("perm None", dict(perm=None)), ("perm int64", dict(perm=z(I64, B, F, K))), ("perm 1-d", dict(perm=z(I32, K))),
      ("a None", dict(a=None)), ("a 2-d", dict(a=z(F64, B, F))),
       ("a shape", dict(a=z(F64, B, F, 3))), ("perm empty", dict(a=z(F64, 0, F, K), perm=z(I32, 0, F, K))),
       ("perm None + a None", dict(perm=None, a=None))])

# ---------------------------------------------------------------------------------------------------------- dereverberation
sweep("dereverberation.wpe", DR.wpe, dict(spec=SPEC, taps=2, delay=1, iterations=1, psd_context=0, eps=1e-10, loading=1e-10),
      [("spec None", dict(spec=None)), ("spec 1-d", dict(spec=z(C128, T))), ("spec float64", dict(spec=z(F64, B, D, F, T))),
      ("taps 0", dict(taps=0)), ("taps 65", dict(taps=65)),
       ("taps 2.0", dict(taps=2.0)), ("delay -1", dict(delay=-1)), ("delay 65", dict(delay=65)),
       ("iterations 0", dict(iterations=0)), ("iterations 17", dict(iterations=17)),
       ("psd_context -1", dict(psd_context=-1)), ("psd_context 65", dict(psd_context=65)), ("eps -1", dict(eps=-1.0)),
       ("eps inf", dict(eps=INF)), ("loading -1", dict(loading=-1.0)),
       ("loading None", dict(loading=None))] + SPEC_CASES[3:] + [("D = 0", dict(spec=z(C128, B, 0, F, T))), D_HIGH,
       ("D taps = 66", dict(taps=22)),
                                                                 ("spec float64 + taps 0", dict(spec=z(F64, B, D, F, T), taps=0)),
                                                                 ("taps 0 + delay -1", dict(taps=0, delay=-1)),
                                                                 ("loading -1 + T = 0", dict(loading=-1.0, spec=z(C128, B, D, F, 0))),
                                                                 ("T = 0 + D = 9", dict(spec=z(C128, B, 9, F, 0))),
                                                                 ("2-d spec", dict(spec=SPEC[0, 0])),
                                                                 ("3-d spec", dict(spec=SPEC[0]))])
sweep("dereverberation.dereverberate", DR.dereverberate, dict(wave=z(F32, B, S), n_fft=NFFT, hop=4),
      [("wave None", dict(wave=None)), ("wave 3-d", dict(wave=WAVES)), ("wave int32", dict(wave=z(I32, B, S))),
      ("wave 3-d, int32", dict(wave=z(I32, B, D, S))), ("1-d wave", dict(wave=z(F64, S)))])

# ----------------------------------------------------------------------------------------------------------- speech_metrics
N_ = 32
X, Y = z(F32, B, N_), z(F32, B, N_)
sweep("speech_metrics.resample_filter", SM.resample_filter, dict(up=2, down=3), [("up 0", dict(up=0)),
      ("down 1.5", dict(down=1.5)), ("up True", dict(up=True)), ("R = 513", dict(up=513, down=1)),
                                                                                ("up 0 + down 0", dict(up=0, down=0))])
ROWS = lambda k: [(k + " None", {k: None}), (k + " 3-d", {k: z(F32, B, 1, N_)}), (k + " int32", {k: z(I32, B, N_)}),
      (k + " B = 0", {k: z(F32, 0, N_)}),  # noqa: E731
                  (k + " B = 65536", {k: z(F32, 1, 1).expand(65536, N_)}),
                  (k + " n = 2^24 + 1", {k: z(F32, 1, 1).expand(B, (1 << 24) + 1)})]
sweep("speech_metrics.resample_poly", SM.resample_poly, dict(x=X, up=2, down=3), [("up 0", dict(up=0)),
      ("R = 513", dict(up=513, down=1))] + ROWS("x")
      + [("n = 0", dict(x=z(F32, B, 0))), ("up 0 + x None", dict(up=0, x=None)), ("1-d x, n = 1", dict(x=z(F64, 1)))])
PAIR = lambda a, b: [(a + " None", {a: None}), (b + " 3-d", {b: z(F32, B, 1, N_)}), ("shapes differ", {b: z(F32, B, N_ + 1)}),
      ("dtypes differ", {b: z(F64, B, N_)})]  # noqa: E731
PAIRED = lambda a, b, bad: [(n, {a: t, b: t}) for n, t in bad]  # noqa: E731
BAD_ROWS = [("int32", z(I32, B, N_)), ("B = 0", z(F32, 0, N_)), ("B = 65536", z(F32, 1, 1).expand(65536, N_)),
      ("n = 1", z(F32, B, 1)), ("n = 2^24 + 1", z(F32, 1, 1).expand(B, (1 << 24) + 1))]
sweep("speech_metrics.stoi", SM.stoi, dict(clean=X, degraded=Y, fs=10000),
      [("fs 0", dict(fs=0)), ("fs 16000.0", dict(fs=16000.0)),
      ("fs True", dict(fs=True))] + PAIR("clean", "degraded") + [("fs 1", dict(fs=1))] + PAIRED("clean", "degraded", BAD_ROWS)
      + [("fs 0 + clean None", dict(fs=0, clean=None)), ("shapes differ + fs 1", dict(degraded=z(F32, B, N_ + 1), fs=1)),
      ("fs 1 + int32", dict(fs=1, clean=z(I32, B, N_), degraded=z(I32, B, N_))),
         ("fs 16000", dict(fs=16000)), ("1-d", dict(clean=X[0], degraded=Y[0]))])
sweep("speech_metrics.si_sdr", SM.si_sdr,
      dict(reference=X, estimate=Y), PAIR("reference", "estimate") + PAIRED("reference", "estimate", BAD_ROWS)
      + [("reference None + estimate 3-d", dict(reference=None, estimate=z(F32, B, 1, N_))),
      ("1-d", dict(reference=X[0], estimate=Y[0]))])
P = z(F32, B, F, T)
sweep("speech_metrics.log_spectral_distance", SM.log_spectral_distance, dict(p=P, q=P, eps=1e-10),
      [("eps -1", dict(eps=-1.0)), ("eps nan", dict(eps=NAN)), ("eps '0'", dict(eps="0")), ("eps True", dict(eps=True)),
      ("p None", dict(p=None)), ("q 1-d", dict(q=z(F32, T))),
       ("shapes differ", dict(q=z(F32, B, F, T + 1))), ("dtypes differ", dict(q=z(F64, B, F, T))),
       ("int32", dict(p=z(I32, B, F, T), q=z(I32, B, F, T))), ("B = 0", dict(p=z(F32, 0, F, T), q=z(F32, 0, F, T))),
       ("F T = 2^30 + 2^15", dict(p=z(F32, 1, 1, 1).expand(B, 32769, 32768), q=z(F32, 1, 1, 1).expand(B, 32769, 32768))),
       ("eps -1 + p None", dict(eps=-1.0, p=None)), ("2-d", dict(p=P[0], q=P[0]))])
REFS, ESTS = z(F32, B, K, N_), z(F32, B, 3, N_)
SOURCE_CASES = [("references None", dict(references=None)), ("estimates 1-d", dict(estimates=z(F32, N_))),
      ("estimates int32", dict(estimates=z(I32, B, 3, N_))), ("ranks differ", dict(estimates=ESTS[0])),
                ("dtypes differ", dict(estimates=z(F64, B, 3, N_))), ("B differs", dict(estimates=z(F32, 3, 3, N_))),
                ("n differs", dict(estimates=z(F32, B, 3, N_ + 1))),
                ("B = 0", dict(references=z(F32, 0, K, N_), estimates=z(F32, 0, 3, N_))),
                ("K = 9", dict(references=z(F32, B, 9, N_), estimates=z(F32, B, 9, N_))),
                ("J = 0", dict(estimates=z(F32, B, 0, N_))),
                ("n = 1", dict(references=z(F32, B, K, 1), estimates=z(F32, B, 3, 1))),
                ("references None + estimates 1-d", dict(references=None, estimates=z(F32, N_)))]
SQUARE = [("K > J", dict(estimates=z(F32, B, 1, N_))),
      ("K > J + n = 1", dict(references=z(F32, B, K, 1), estimates=z(F32, B, 1, 1)))]
sweep("speech_metrics.pairwise_si_sdr", SM.pairwise_si_sdr,
      dict(references=REFS, estimates=ESTS), SOURCE_CASES + [("K > J is fine here", dict(estimates=z(F32, B, 1, N_))),
      ("no batch", dict(references=REFS[0], estimates=ESTS[0]))])
TABLE = z(F64, B, K, 3)
sweep("speech_metrics.assign", SM.assign, dict(table=TABLE, maximize=True),
      [("table None", dict(table=None)), ("table 1-d", dict(table=z(F64, 3))), ("table float32", dict(table=z(F32, B, K, 3))),
      ("maximize 1", dict(maximize=1)), ("B = 0", dict(table=z(F64, 0, K, 3))),
       ("K > J", dict(table=z(F64, B, 3, K))), ("J = 9", dict(table=z(F64, B, K, 9))),
       ("table float32 + maximize 1", dict(table=z(F32, B, K, 3), maximize=1)),
       ("maximize 1 + K > J", dict(table=z(F64, B, 3, K), maximize=1)),
       ("no batch", dict(table=TABLE[0], maximize=False))])
sweep("speech_metrics.pit_si_sdr", SM.pit_si_sdr, dict(references=REFS, estimates=ESTS), SOURCE_CASES + SQUARE + [("no batch",
      dict(references=REFS[0], estimates=ESTS[0]))])
sweep("speech_metrics.si_bss_eval", SM.si_bss_eval, dict(references=REFS, estimates=ESTS, perm=z(I32, B, K)),
      SOURCE_CASES + SQUARE + [("perm int64", dict(perm=z(I64, B, K))), ("perm (K,)", dict(perm=z(I32, K))),
      ("perm list", dict(perm=[0, 1])), ("K > J + perm list", dict(estimates=z(F32, B, 1, N_), perm=[0, 1])),
                               ("no perm", dict(perm=None)),
                               ("no batch", dict(references=REFS[0], estimates=ESTS[0], perm=z(I32, K)))])
sweep("speech_metrics.si_sdr_improvement", SM.si_sdr_improvement, dict(references=REFS, estimates=ESTS, mixture=X),
      SOURCE_CASES + SQUARE + [("mixture None", dict(mixture=None)), ("mixture float64", dict(mixture=z(F64, B, N_))),
      ("mixture (n,)", dict(mixture=X[0])), ("K > J + mixture None", dict(estimates=z(F32, B, 1, N_), mixture=None)),
                               ("no batch", dict(references=REFS[0], estimates=ESTS[0], mixture=X[0]))])

# ----------------------------------------------------------------------------------------------------------- room_acoustics
H_CASES = [("h None", dict(h=None)), ("h 3-d", dict(h=z(F64, B, 1, N_))), ("h int32", dict(h=z(I32, B, N_))),
      ("B = 0", dict(h=z(F64, 0, N_))), ("n = 1", dict(h=z(F64, B, 1))),
           ("n = 2^24 + 1", dict(h=z(F64, 1, 1).expand(B, (1 << 24) + 1))),
           ("B = 65536 is fine here", dict(h=z(F32, 1, 1).expand(65536, N_))), ("h 3-d, int32", dict(h=z(I32, B, 1, N_))),
           ("1-d h", dict(h=z(F32, N_)))]
sweep("room_acoustics.sample_counts", RA.sample_counts, dict(fs=16000), [("fs None", dict(fs=None))])
sweep("room_acoustics.energy_decay_curve", RA.energy_decay_curve, dict(h=z(F64, B, N_)), H_CASES)
FS_CASES = [("fs 0", dict(fs=0)), ("fs inf", dict(fs=INF)), ("fs '16000'", dict(fs="16000")), ("fs True", dict(fs=True)),
      ("fs 0 + h None", dict(fs=0, h=None))]
sweep("room_acoustics.room_acoustic_parameters", RA.room_acoustic_parameters, dict(h=z(F64, B, N_), fs=16000), FS_CASES + H_CASES)
sweep("room_acoustics.reverberation_time", RA.reverberation_time, dict(h=z(F64, B, N_), fs=16000, method="t30"),
      [("method 't60'", dict(method="t60")),
      ("method 't60' + fs 0", dict(method="t60", fs=0))] + FS_CASES + H_CASES[:3] + [("edt", dict(method="edt"))])

# ------------------------------------------------------------------------------------- front_end, tsne, kmeans: the touched parts
sweep("front_end.griffin_lim", FE.griffin_lim,
      dict(spec=z(F32, B, F, T), power=2.0, n_iter=2, momentum=0.99, length=None, init=None, generator=None, n_fft=NFFT, hop=4),
      [("spec 2-d", dict(spec=z(F32, F, T))), ("spec complex", dict(spec=z(C64, B, F, T))), ("n_fft 16", dict(n_fft=16)),
      ("momentum 1", dict(momentum=1.0)), ("n_iter -1", dict(n_iter=-1)),
       ("power 0", dict(power=0)), ("n_fft 16 + momentum 1", dict(n_fft=16, momentum=1.0)),
       ("power 0 + init None", dict(power=0)), ("float64", dict(spec=z(F64, B, F, T)))])
sweep("front_end.array_spectrograms", FE.array_spectrograms, dict(wave=z(F32, B, S), h=z(F64, B, D, 4), n_fft=NFFT, hop=4),
      [("wave float64", dict(wave=z(F64, B, S))), ("h B", dict(h=z(F64, 3, D, 4)))])
sweep("tsne.code_sq_distances", TS.code_sq_distances, dict(codes=z(I32, 4, 3), n_codes=None), [("codes list",
      dict(codes=[[0, 1]]))])
sweep("tsne.TSNE.fit_transform", lambda X, **kw: TS.TSNE(**kw).fit_transform(X), dict(X=z(I32, 4, 3)), [("X None", dict(X=None)),
      ("precomputed", dict(X=z(F32, 4, 4), metric="precomputed"))])
sweep("kmeans.KMeans.fit", lambda X, **kw: KM.KMeans(**kw).fit(X), dict(X=z(F32, 8, 3), n_clusters=2), [("X None", dict(X=None)),
      ("X 1-d", dict(X=z(F32, 8)))])

# ----------------------------------------------------------------------------------------- _native: the signal and array wrappers
WAVE = z(F32, B, S)
SPEC3 = z(C64, B, NFFT // 2 + 1, 5)
sweep("_native.stft_power", N.stft_power, dict(wave=WAVE, n_fft=NFFT, hop=4), [("int32", dict(wave=z(I32, B, S))),
      ("float64", dict(wave=z(F64, B, S)))])
sweep("_native.stft_complex", N.stft_complex, dict(wave=WAVE, n_fft=NFFT, hop=4), [("float16", dict(wave=z(torch.float16, B, S))),
      ("float64", dict(wave=z(F64, B, S)))])
sweep("_native.fir_same", N.fir_same, dict(wave=WAVE, h=z(F64, 4)), [("3 responses", dict(h=z(F64, 3, 4))),
      ("h per row", dict(h=z(F64, B, 4)))])
sweep("_native.spec_rir_wiener", N.spec_rir_wiener, dict(speech_spec=SPEC3, echoed_spec=z(C128, *SPEC3.shape)),
      [("both complex64", dict(echoed_spec=SPEC3)),
      ("shapes differ", dict(echoed_spec=z(C128, B, 5, 4)))])
sweep("_native.istft", N.istft, dict(spec=SPEC3, n_fft=NFFT, hop=4, length=None),
      [("spec 2-d", dict(spec=SPEC3[0])), ("spec float32", dict(spec=z(F32, *SPEC3.shape))), ("n_fft 16", dict(n_fft=16)),
      ("spec 2-d + n_fft 16", dict(spec=SPEC3[0], n_fft=16)), ("complex128", dict(spec=z(C128, *SPEC3.shape)))])
MAG = z(F32, *SPEC3.shape)
sweep("_native.griffin_lim", N.griffin_lim, dict(mag=MAG, angles=SPEC3, n_iter=2, momentum=0.5, n_fft=NFFT, hop=4, length=S),
      [("angles float32", dict(angles=MAG)), ("n_fft 16", dict(n_fft=16)), ("mag float64", dict(mag=z(F64, *SPEC3.shape))),
      ("mag shape", dict(mag=z(F32, B, 5, 4))),
       ("B = 0", dict(mag=z(F32, 0, 5, 5), angles=z(C64, 0, 5, 5))),
       ("mag float64 + B = 0", dict(mag=z(F64, 0, 5, 5), angles=z(C64, 0, 5, 5)))])
sweep("_native.rir", N.rir, dict(src=SRC, rcv=SRC, L=[4.0, 5.0, 3.0], beta=[0.5] * 6, c=343.0, fs=16000.0, nsample=8, order=-1, hp_filter=True),
      [("src 1-d", dict(src=z(F64, 3))), ("rcv shape", dict(rcv=z(F64, 3, 3))), ("L of 2", dict(L=[4.0, 5.0])),
      ("beta of 5", dict(beta=[0.5] * 5)), ("src 1-d + L of 2", dict(src=z(F64, 3), L=[4.0, 5.0])),
      ("float32", dict(src=z(F32, B, 3)))])
sweep("_native.rir_rooms", N.rir_rooms,
      dict(src=SRC, rcv=SRC, room=SRC, beta=z(F64, B, 6), c=343.0, fs=16000.0, nsample=8, order=-1, hp_filter=True),
      [("src 1-d", dict(src=z(F64, 3))), ("room shape", dict(room=z(F64, 3, 3))), ("beta (B, 5)", dict(beta=z(F64, B, 5)))])
HROWS = z(F64, B, N_)
sweep("_native.edc", N.edc, dict(h=HROWS), [("h 1-d", dict(h=HROWS[0])), ("h int32", dict(h=z(I32, B, N_))),
      ("float32", dict(h=z(F32, B, N_)))])
sweep("_native.room_acoustics", N.room_acoustics, dict(h=HROWS, fs=16000.0, k50=800, k80=1280, kdirect=40), [("h 1-d",
      dict(h=HROWS[0])),
      ("h float16", dict(h=z(torch.float16, B, N_))), ("float32", dict(h=z(F32, B, N_)))])
sweep("_native.resample_poly", N.resample_poly, dict(x=X, h=z(F64, 5), up=2, down=3), [("x 1-d", dict(x=X[0])),
      ("h 2-d", dict(h=z(F64, 1, 5))), ("4 taps", dict(h=z(F64, 4))), ("x 1-d + 4 taps", dict(x=X[0], h=z(F64, 4)))])
X64, LO, HI = z(F64, B, N_), list(range(15)), list(range(1, 16))
sweep("_native.stoi", N.stoi, dict(clean=X64, degraded=X64, band_lo=LO, band_hi=HI),
      [("clean 1-d", dict(clean=X64[0])), ("dtypes differ", dict(degraded=X)), ("14 edges", dict(band_lo=LO[:14])),
      ("n = 1", dict(clean=z(F64, B, 1), degraded=z(F64, B, 1))),
       ("B = 65536", dict(clean=z(F64, 1, 1).expand(65536, N_), degraded=z(F64, 1, 1).expand(65536, N_))),
       ("14 edges + n = 1", dict(band_lo=LO[:14], clean=z(F64, B, 1), degraded=z(F64, B, 1))),
       ("float32", dict(clean=X, degraded=X))])
sweep("_native.si_sdr", N.si_sdr, dict(reference=X, estimate=Y), [("reference 1-d", dict(reference=X[0])),
      ("int32", dict(reference=z(I32, B, N_), estimate=z(I32, B, N_))), ("shapes differ", dict(estimate=z(F32, B, 3)))])
sweep("_native.lsd", N.lsd, dict(p=P, q=P, eps=1e-10), [("p 2-d", dict(p=P[0])), ("dtypes differ", dict(q=z(F64, B, F, T))),
      ("complex", dict(p=z(C64, B, F, T), q=z(C64, B, F, T)))])
sweep("_native.pairwise_si_sdr", N.pairwise_si_sdr, dict(references=REFS, estimates=ESTS), [("references 2-d",
      dict(references=REFS[0])),
      ("n differs", dict(estimates=z(F32, B, 3, 3))), ("dtypes differ", dict(estimates=z(F64, B, 3, N_)))])
sweep("_native.assign", N.assign, dict(table=TABLE, maximize=True), [("table 2-d", dict(table=TABLE[0])),
      ("table float32", dict(table=z(F32, B, K, 3)))])
sweep("_native.si_bss_eval", N.si_bss_eval, dict(references=REFS, estimates=ESTS, perm=z(I32, B, K)),
      [("references 2-d", dict(references=REFS[0])), ("perm int64", dict(perm=z(I64, B, K))),
      ("perm shape", dict(perm=z(I32, B, 3))), ("references 2-d + perm int64", dict(references=REFS[0], perm=z(I64, B, K)))])
SPEC4_CASES = [("spec 3-d", dict(spec4d=SPEC[0])), ("spec float64", dict(spec4d=z(F64, B, D, F, T)))]
sweep("_native.wpe", N.wpe, dict(spec4d=SPEC, taps=2, delay=1, iterations=1, psd_context=0, eps=1e-10, loading=1e-10),
      SPEC4_CASES + [("D taps = 66", dict(taps=22)), ("T = 0", dict(spec4d=z(C128, B, D, F, 0))),
      ("spec 3-d + D taps = 66", dict(spec4d=SPEC[0], taps=22)), ("complex64", dict(spec4d=z(C64, B, D, F, T)))])
sweep("_native.phat_cross_spectra", N.phat_cross_spectra, dict(spec4d=SPEC, f_lo=1, f_hi=3), SPEC4_CASES + [("complex64",
      dict(spec4d=z(C64, B, D, F, T)))])
PSI = z(C128, B, 3, F)
sweep("_native.gcc_phat", N.gcc_phat, dict(psi=PSI, n_fft=NFFT, max_lag=2, f_lo=1, f_hi=3), [("psi 2-d", dict(psi=PSI[0])),
      ("psi complex64", dict(psi=z(C64, B, 3, F))), ("n_fft 16", dict(n_fft=16)), ("4 pairs", dict(psi=z(C128, B, 4, F)))])
NATIVE_GEOMETRY = [("mics 1-d", dict(mics=z(F64, 3))), ("mics 2 rows", dict(mics=z(F64, 2, 3))),
      ("mics 3 items", dict(mics=z(F64, 3, D, 3))), ("cand 1-d", dict(cand=z(F64, 3))), ("cand (G, 2)", dict(cand=z(F64, 6, 2))),
                   ("cand 3 items", dict(cand=z(F64, 3, 6, 3))), ("mics 1-d + cand 1-d", dict(mics=z(F64, 3), cand=z(F64, 3))),
                   ("mics float32", dict(mics=z(F32, D, 3))),
                   ("3-d mics and cand", dict(mics=z(F64, B, D, 3), cand=z(F64, B, 6, 3)))]
sweep("_native.srp_phat", N.srp_phat, dict(psi=PSI, mics=MICS, cand=CAND, fs=16000.0, n_fft=NFFT, c=343.0, f_lo=1, f_hi=3),
      [("psi 2-d", dict(psi=PSI[0])),
      ("4 pairs", dict(psi=z(C128, B, 4, F)))] + NATIVE_GEOMETRY + [("4 pairs + mics 1-d",
      dict(psi=z(C128, B, 4, F), mics=z(F64, 3)))])
sweep("_native.spatial_covariance", N.spatial_covariance, dict(spec4d=SPEC, mask=MASK), SPEC4_CASES + [("mask float32",
      dict(mask=z(F32, B, F, T))),
      ("mask shape", dict(mask=z(F64, B, F, 3))),
                                                                                                         ("spec 3-d + mask float32", dict(spec4d=SPEC[0], mask=z(F32, B, F, T))),
                                                                                                         ("no mask", dict(mask=None))])
sweep("_native.steering_vectors", N.steering_vectors, dict(mics=MICS, src=SRC, F=F, fs=16000.0, n_fft=NFFT, c=343.0, ref=0),
      [("src 1-d", dict(src=z(F64, 3))), ("src (B, 2)", dict(src=z(F64, B, 2))), ("mics 1-d", dict(mics=z(F64, 3))),
      ("mics (D, 2)", dict(mics=z(F64, D, 2))), ("mics 3 items", dict(mics=z(F64, 3, D, 3))),
       ("src 1-d + mics 1-d", dict(src=z(F64, 3), mics=z(F64, 3))), ("mics float32", dict(mics=z(F32, D, 3))),
       ("3-d mics", dict(mics=z(F64, B, D, 3)))])
sweep("_native.beamform_weights", N.beamform_weights,
      dict(mode=N.BEAMFORM_MVDR, B=B, D=D, F=F, phi_n=COV, phi_s=None, steering=STEER, ref=0, loading=0.0),
      [("mode 3", dict(mode=3)), ("mvdr without phi_n", dict(phi_n=None)), ("phi_n complex64", dict(phi_n=z(C64, B, F, D, D))),
      ("steering shape", dict(steering=z(C128, B, F, D))),
       ("mode 3 + phi_n None", dict(mode=3, phi_n=None)), ("das", dict(mode=N.BEAMFORM_DAS)),
       ("souden", dict(mode=N.BEAMFORM_SOUDEN, phi_s=COV))])
sweep("_native.beamform_apply", N.beamform_apply, dict(spec4d=SPEC, w=W), SPEC4_CASES + [("w complex64", dict(w=z(C64, B, F, D))),
      ("w shape", dict(w=z(C128, B, D, F))), ("spec 3-d + w shape", dict(spec4d=SPEC[0], w=z(C128, B, D, F)))])
sweep("_native.beamform_gev", N.beamform_gev, dict(phi_n=COV, phi_s=COV, ref=0, loading=0.0), [("phi_n 3-d", dict(phi_n=COV[0])),
      ("phi_n not square", dict(phi_n=z(C128, B, F, D, 2))), ("phi_n complex64", dict(phi_n=z(C64, B, F, D, D))),
                                                                                              ("phi_s shape", dict(phi_s=z(C128, B, F, 2, 2)))])
sweep("_native.auxiva", N.auxiva, dict(spec4d=SPEC, iterations=2, model=N.IVA_LAPLACE, ref=0, eps=1e-10, w0=COV),
      SPEC4_CASES + [("D = 9", dict(spec4d=z(C128, B, 9, F, T), w0=None)), ("w0 complex64", dict(w0=z(C64, B, F, D, D))),
      ("D = 9 + w0 complex64", dict(spec4d=z(C128, B, 9, F, T), w0=z(C64, B, F, D, D))), ("no w0", dict(w0=None))])
sweep("_native.ilrma", N.ilrma, dict(spec4d=SPEC, basis0=BASIS, activations0=ACT, iterations=2, ref=0, floor=1e-10, w0=COV),
      SPEC4_CASES + [("basis0 float32", dict(basis0=z(F32, B, D, F, L))), ("basis0 shape", dict(basis0=z(F64, B, D, 2, L))),
      ("activations0 shape", dict(activations0=z(F64, B, D, 3, T))),
                     ("L = 17", dict(basis0=z(F64, B, D, F, 17), activations0=z(F64, B, D, 17, T))),
                     ("w0 shape", dict(w0=z(C128, B, F, D, 2))),
                     ("L = 17 + w0 shape", dict(basis0=z(F64, B, D, F, 17), activations0=z(F64, B, D, 17, T), w0=z(C128, B, F, D, 2))),
                     ("basis0 float32 + activations0 shape", dict(basis0=z(F32, B, D, F, L), activations0=z(F64, B, D, 3, T)))])
sweep("_native.separation_masks", N.separation_masks, dict(spec4d=SPEC), SPEC4_CASES)
sweep("_native.cacgmm", N.cacgmm, dict(spec4d=SPEC, init=INIT, iterations=2, floor=1e-10, quadratic0=INIT),
      SPEC4_CASES + [("init 3-d", dict(init=INIT[0])), ("init float32", dict(init=z(F32, B, K, F, T))),
      ("init T", dict(init=z(F64, B, K, F, 3))), ("quadratic0 shape", dict(quadratic0=z(F64, B, 3, F, T))),
                     ("K = 9", dict(init=z(F64, B, 9, F, T), quadratic0=None)), ("D = 1", dict(spec4d=z(C128, B, 1, F, T))),
                     ("quadratic0 shape + D = 1", dict(spec4d=z(C128, B, 1, F, T), quadratic0=z(F64, B, 3, F, T))),
                     ("no quadratic0", dict(quadratic0=None))])
sweep("_native.align_permutations", N.align_permutations, dict(profile=INIT, iterations=2, perm0=PERM),
      [("profile 3-d", dict(profile=INIT[0])), ("profile float32", dict(profile=z(F32, B, K, F, T))),
      ("perm0 int64", dict(perm0=z(I64, B, F, K))), ("perm0 shape", dict(perm0=z(I32, B, K, F))),
      ("T = 1", dict(profile=z(F64, B, K, F, 1))),
       ("perm0 int64 + T = 1", dict(profile=z(F64, B, K, F, 1), perm0=z(I64, B, F, K))), ("no perm0", dict(perm0=None))])
sweep("_native.permute_bins", N.permute_bins, dict(x=INIT, perm=PERM), [("x 3-d", dict(x=INIT[0])),
      ("x int32", dict(x=z(I32, B, K, F, T))), ("perm int64", dict(perm=z(I64, B, F, K))),
      ("perm shape", dict(perm=z(I32, B, K, F))), ("x 3-d + perm int64", dict(x=INIT[0], perm=z(I64, B, F, K)))])
sweep("_native.eigh", N.eigh, dict(cov=COV[0]), [("cov 2-d", dict(cov=COV[0, 0])), ("cov not square", dict(cov=z(C128, F, D, 2))),
      ("cov complex64", dict(cov=z(C64, F, D, D)))])
VALUES = z(F64, B, F, D)
sweep("_native.music", N.music, dict(vectors=COV, values=VALUES, mics=MICS, cand=CAND, n_sources=1, fs=16000.0, n_fft=NFFT, c=343.0, f_lo=1, f_hi=3),
      [("vectors 3-d", dict(vectors=COV[0])), ("vectors not square", dict(vectors=z(C128, B, F, D, 2))),
      ("vectors complex64", dict(vectors=z(C64, B, F, D, D))), ("values float32", dict(values=z(F32, B, F, D))),
      ("values shape", dict(values=z(F64, B, F, 2)))]
      + NATIVE_GEOMETRY + [("values shape + mics 1-d", dict(values=z(F64, B, F, 2), mics=z(F64, 3)))])
sweep("_native.tsne_code_sqdist", N.tsne_code_sqdist, dict(codes=z(I32, 4, 3)), [("codes 1-d", dict(codes=z(I32, 4))),
      ("codes int64", dict(codes=z(I64, 4, 3)))])
sweep("_native.tsne_affinities", N.tsne_affinities, dict(P=z(F32, 4, 4), perplexity=2.0), [("P not square", dict(P=z(F32, 4, 3))),
      ("P 1-d", dict(P=z(F32, 4))), ("N = 1", dict(P=z(F32, 1, 1))), ("N = 65537", dict(P=z(F32, 1, 1).expand(65537, 65537)))])
YS = z(F64, 4, 2)
sweep("_native.tsne_descend", N.tsne_descend,
      dict(P=z(F32, 4, 4), Y=YS, update=YS, gains=YS, grad=YS, stats=z(F64, 2), n_iter=1, exaggeration=1.0, momentum=0.5, learning_rate=10.0, workspace=None),
      [("update shape", dict(update=z(F64, 4, 3))), ("grad shape", dict(grad=z(F64, 3, 2))), ("P shape", dict(P=z(F32, 4, 3))),
      ("stats of 1", dict(stats=z(F64, 1))), ("update shape + P shape", dict(update=z(F64, 4, 3), P=z(F32, 4, 3))),
       ("N = 1", dict(P=z(F32, 1, 1), Y=YS[:1], update=YS[:1], gains=YS[:1], grad=YS[:1])),
       ("a workspace", dict(workspace=torch.zeros(1 << 20, dtype=torch.uint8)))])
XS, LAB, CEN = z(F32, 8, 3), z(I64, 8), z(F32, 2, 3)
sweep("_native.kmeans_update", N.kmeans_update,
      dict(x=XS, labels=LAB, labels_old=LAB, centers_old=CEN, centers_new=CEN, counts=None, stats=z(F64, 1), flags=z(I32, 4), tol=0.0, workspace=None),
      [("x 1-d", dict(x=XS[0])), ("centres shape", dict(centers_new=z(F32, 2, 4))), ("labels shape", dict(labels=z(I64, 7))),
      ("labels_old shape", dict(labels_old=z(I64, 7))),
      ("D = 513", dict(x=z(F32, 8, 513), centers_old=z(F32, 2, 513), centers_new=z(F32, 2, 513))),
       ("x 1-d + labels shape", dict(x=XS[0], labels=z(I64, 7))),
       ("labels_old shape + D = 513",
       dict(labels_old=z(I64, 7), x=z(F32, 8, 513), centers_old=z(F32, 2, 513), centers_new=z(F32, 2, 513))),
       ("no labels_old", dict(labels_old=None))])
sweep("_native.kmeans_inertia", N.kmeans_inertia, dict(x=XS, labels=LAB, centers=CEN), [("x 3-d", dict(x=XS[None])),
      ("centres shape", dict(centers=z(F32, 2, 4))), ("labels shape", dict(labels=z(I64, 7)))])
sweep("_native.kmeans_col_stats", N.kmeans_col_stats, dict(x=XS), [("x 1-d", dict(x=XS[0])), ("D = 513", dict(x=z(F32, 8, 513))),
      ("N = 0", dict(x=z(F32, 0, 3)))])
sweep("_native.kmeans_add_rows", N.kmeans_add_rows, dict(x=XS, v=z(F32, 3), alpha=1.0, out=None), [("x 1-d", dict(x=XS[0])),
      ("v shape", dict(v=z(F32, 4))), ("x 1-d + v shape", dict(x=XS[0], v=z(F32, 4)))])
sweep("_native.kmeans_plusplus", N.kmeans_plusplus, dict(x=XS, K=2, first=0, uniforms=z(F64, 1, 2)),
      [("x 1-d", dict(x=XS[0])), ("no uniforms", dict(uniforms=None)), ("uniforms rows", dict(uniforms=z(F64, 2, 2))),
      ("N = 0", dict(x=z(F32, 0, 3))), ("x 1-d + no uniforms", dict(x=XS[0], uniforms=None)), ("K = 1", dict(K=1, uniforms=None))])
