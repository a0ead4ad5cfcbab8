"""Beamforming, the parts that need no GPU: the numpy restatement (tests/helpers/beamform_ref.py) is pinned -- float64 against
np.longdouble on every parity shape, and on the properties that make it a beamformer -- so that the yardstick of
tests/test_beamform_gpu.py is itself one; and the host-side argument rules of acoustic_locating_vq_vae.beamforming.

Float64 against longdouble, u = 1.1e-16:
  covariance   |Phi_64 - Phi_ld| <= (T + 4) u S_ij, S_ij = sum_t m_t |x_i| |x_j| / sum_t m_t: a T-term sum in any order.
  weights      max |w_64 - w_ld| <= 8 D u cond_2(Phi') max |w_ld| from the same Phi: the forward bound c n u kappa of a Cholesky
               solve, with the constant of tests/test_wpe_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import beamform_ref as R  # noqa: E402
from acoustic_locating_vq_vae import beamforming as BF  # noqa: E402

U = R.U
IDS = ["-".join(str(v) for v in s) for s in R.PARITY]


# ------------------------------------------------------------------------------------------------- float64 against longdouble
@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
def test_float64_covariance_against_longdouble(shape):
    B, D, F, T, _ = shape
    c = R.parity_case(shape)
    worst = 0.0
    for kind in R.MASKS:
        ref = R.reference(shape, kind)
        ld, st = R.covariance(c.X, c.masks[kind], dtype=np.longdouble)
        assert ld.dtype == np.clongdouble and not st.any()
        err = np.abs(ref.cov - ld).astype(np.float64)
        bound = R.cov_bound(T, ref.scale)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (kind, float((err / bound).max()))
        assert np.array_equal(ref.cov, np.conj(np.swapaxes(ref.cov, -1, -2)))              # exactly Hermitian
        assert not np.diagonal(ref.cov, axis1=-2, axis2=-1).imag.any()
    null, _ = R.covariance(c.X)                                                            # no mask: every weight 1
    assert np.array_equal(null, R.reference(shape, "ones").cov)
    print("%s: largest |Phi - Phi_ld| / bound %.3g" % (shape[:4], worst))


@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
def test_float64_weights_against_longdouble(shape):
    B, D, F, T, loading = shape
    c = R.parity_case(shape)
    worst = 0.0
    for kind in R.MASKS:
        ref = R.reference(shape, kind)
        lds = {"mpdr": R.weights(R.MVDR, ref.cov, A=c.A, loading=loading, dtype=np.longdouble),
               "mvdr": R.weights(R.MVDR, ref.cov_n, A=c.A, loading=loading, dtype=np.longdouble),
               "souden": R.weights(R.SOUDEN, ref.cov_n, ref.cov_s, loading=loading, dtype=np.longdouble)}
        for name, (ld, st) in lds.items():
            assert ld.dtype == np.clongdouble and not st.any()
            err = np.abs(ref.W[name] - ld).max(axis=-1).astype(np.float64)
            bound = R.weights_bound(D, ref.cond[name], np.abs(ld).max(axis=-1).astype(np.float64))
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (kind, name, float((err / bound).max()))
    print("%s: largest |w - w_ld| / bound %.3g, cond up to %.3g" % (shape[:4], worst, max(v.max() for v in ref.cond.values())))


def test_float64_steering_against_longdouble():
    for shape in R.PARITY:
        B, D, F, T, _ = shape
        c = R.parity_case(shape)
        ld, _ = R.steering(c.mics, c.source, F, dtype=np.longdouble)
        err = float(np.abs(c.A - ld).max())
        assert err <= R.steering_bound(R.theta_max(c.mics, c.source, F)) / 2
        assert (c.A[:, 0] == 1).all()


def test_float64_apply_against_longdouble():
    shape = R.PARITY[4]
    c, ref = R.parity_case(shape), R.reference(shape, "uniform")
    W = ref.W["mpdr"]
    err = np.abs(R.apply(c.X, W) - R.apply(c.X, W, dtype=np.longdouble)).astype(np.float64)
    assert (err <= R.apply_bound(c.X, W)).all()


# ------------------------------------------------------------------------------- what makes the yardstick a beamformer
@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
def test_mvdr_is_distortionless_and_no_worse_than_delay_and_sum(shape):
    B, D, F, T, loading = shape
    c = R.parity_case(shape)
    a = np.moveaxis(c.A, 1, 2)                                                             # (B, F, D)
    worst = 0.0
    for kind in R.MASKS:
        ref = R.reference(shape, kind)
        for name, cov in (("mpdr", ref.cov), ("mvdr", ref.cov_n)):
            w = ref.W[name]
            gain = np.sum(np.conj(w) * a, axis=-1)                                         # w^H a = 1
            bound = 8 * D * U * ref.cond[name]
            worst = max(worst, float((np.abs(gain - 1) / bound).max()))
            assert (np.abs(gain - 1) <= bound).all(), (kind, name)
            P = R.loaded(cov, loading)

            def power(v):
                return np.einsum("bfi,bfij,bfj->bf", np.conj(v), P, v).real
            assert (power(w) <= power(ref.W["das"]) * (1 + 1e-9)).all(), (kind, name)    # the minimum under the constraint
        assert np.abs(np.sum(np.conj(ref.W["das"]) * a, axis=-1) - 1).max() <= 4 * D * U   # which delay-and-sum satisfies
    print("%s: largest |w^H a - 1| / (8 D u cond) %.3g" % (shape[:4], worst))


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_white_noise_gives_delay_and_sum(dtype):
    for shape in R.PARITY[:5]:
        B, D, F, T, _ = shape
        c = R.parity_case(shape)
        eye = np.broadcast_to(np.eye(D, dtype=complex), (B, F, D, D))
        w, st = R.weights(R.MVDR, eye, A=c.A, loading=0.0, dtype=dtype)
        das, _ = R.weights(R.DAS, A=c.A, dtype=dtype)
        assert not st.any() and np.abs(w - das).max() <= 4 * U


@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
def test_souden_with_a_rank_one_speech_covariance_is_mvdr(shape):
    B, D, F, T, loading = shape
    c = R.parity_case(shape)
    a = np.moveaxis(c.A, 1, 2)
    g = np.random.default_rng(T)
    power = g.uniform(0.5, 2.0, (B, F))
    cov_s = power[..., None, None] * a[..., :, None] * np.conj(a[..., None, :])            # sigma_s^2 a a^H, a_ref = 1
    for kind in R.MASKS:
        ref = R.reference(shape, kind)
        w, st = R.weights(R.SOUDEN, ref.cov_n, cov_s, ref=0, loading=loading)
        want = ref.W["mvdr"]
        bound = R.weights_bound(D, ref.cond["mvdr"], np.abs(want).max(axis=-1), c=16)
        assert not st.any() and (np.abs(w - want).max(axis=-1) <= bound).all(), kind


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_restatement_refuses_bad_bins(dtype):
    shape = R.PARITY[1]
    B, D, F, T, loading = shape
    c = R.parity_case(shape)
    zero = np.zeros((B, F, D, D), complex)
    for mode, kwargs in ((R.MVDR, {"A": c.A}), (R.SOUDEN, {"Phi_s": R.reference(shape, "ones").cov_s})):
        w, st = R.weights(mode, zero, ref=1, loading=loading, dtype=dtype, **kwargs)
        assert (st == R.BAD_SOLVE).all() and R.BAD_SOLVE == 2
        assert np.array_equal(w.astype(complex), np.broadcast_to(np.eye(D)[1], (B, F, D)))
    X, mask = c.X.copy(), c.masks["uniform"].copy()
    X[1, 0, 2, 5] = complex(1.0, np.nan)
    mask[0, 3] = 0
    cov, st = R.covariance(X, mask, dtype=dtype)
    want = np.zeros((B, F), np.int32)
    want[1, 2] = want[0, 3] = R.BAD_INPUT
    assert R.BAD_INPUT == 1 and np.array_equal(st, want)
    assert not cov[1, 2].any() and not cov[0, 3].any() and cov[0, 0].any()
    for bad in (-0.5, np.inf, np.nan):
        mask = c.masks["uniform"].copy()
        mask[1, 1, 7] = bad
        assert R.covariance(c.X, mask, dtype=dtype)[1][1, 1] == 1
    negative = R.reference(shape, "ones").cov.copy()                                       # not positive definite
    negative[0, 0] = -negative[0, 0]
    w, st = R.weights(R.MVDR, negative, A=c.A, loading=0.0, dtype=dtype)
    assert st[0, 0] == 2 and st.sum() == 2 and np.array_equal(w[0, 0].astype(complex), np.eye(D)[0])
    _, st = R.steering(np.array([[0.0, 0, 0], [np.inf, 0, 0]]), np.array([[1.0, 1, 1]]), 4, dtype=dtype)
    assert list(st) == [R.BAD_GEOMETRY] and R.BAD_GEOMETRY == 4


def test_case_generator():
    c = R.parity_case(R.PARITY[3])
    assert R.SIGMA >= 0.03 and np.array_equal(c.X, c.speech + c.noise)
    assert (c.masks["ones"] == 1).all() and 0 <= c.masks["uniform"].min() and c.masks["uniform"].max() <= 1
    runs = c.masks["runs"]
    assert (runs == 0).any() and (runs.sum(axis=-1) > 0).all()
    zeros = (runs[0, 0] == 0).astype(int)
    assert np.diff(np.flatnonzero(np.diff(np.concatenate(([0], zeros, [0]))))).max() >= 1 + 65 // 8      # a run, not single zeros
    with pytest.raises(AssertionError):                                                    # the generator's own guard
        R.case(1, 2, 1, 1, 0, 1e-12)


# ---------------------------------------------------------------------------------------------------------- argument rules
SPEC = torch.zeros(2, 3, 5, 20, dtype=torch.complex128)
MICS = torch.zeros(3, 3, dtype=torch.float64)
SRC = torch.zeros(2, 3, dtype=torch.float64)
MASK = torch.ones(2, 5, 20, dtype=torch.float64)
COV = torch.zeros(2, 5, 3, 3, dtype=torch.complex128)
STEER = torch.zeros(2, 3, 5, dtype=torch.complex128)
W = torch.zeros(2, 5, 3, dtype=torch.complex128)
WAVES = torch.zeros(2, 3, 800)
WAVE_MASK = torch.ones(2, 201, 6, dtype=torch.float64)          # 800 samples: 6 frames of 201 bins


def spec_of(D=3, T=20, B=2, dtype=torch.complex64):
    return torch.zeros(B, D, 5, T, dtype=dtype)


BAD_SPECS = [SPEC.real, SPEC.to(torch.complex32), SPEC[0, 0], SPEC[None], "spec", spec_of(D=9), spec_of(D=0), spec_of(T=0),
             spec_of(D=1, T=65536), spec_of(B=0), torch.zeros(2, 3, 0, 20, dtype=torch.complex64)]

RULES = [("spatial_covariance", (s,), {}) for s in BAD_SPECS] + [
    ("spatial_covariance", (SPEC, MASK[:1]), {}), ("spatial_covariance", (SPEC, MASK.float()), {}),
    ("spatial_covariance", (SPEC, MASK[:, :, :19]), {}), ("spatial_covariance", (SPEC[0], MASK), {}),
    ("spatial_covariance", (SPEC, MASK[0]), {}), ("spatial_covariance", (SPEC, "mask"), {}),
] + [("apply", (s, W), {}) for s in BAD_SPECS] + [
    ("apply", (SPEC, W[:1]), {}), ("apply", (SPEC, W.to(torch.complex64)), {}), ("apply", (SPEC, W[0]), {}),
    ("apply", (SPEC[0], W), {}), ("apply", (SPEC, COV), {}), ("apply", (SPEC, None), {}),
    ("steering_vectors", (MICS.float(), SRC, 5), {}), ("steering_vectors", (MICS[0], SRC, 5), {}),
    ("steering_vectors", (MICS[:, :2], SRC, 5), {}), ("steering_vectors", (MICS, SRC.float(), 5), {}),
    ("steering_vectors", (MICS, SRC[None], 5), {}), ("steering_vectors", (MICS[None].expand(3, 3, 3), SRC, 5), {}),
    ("steering_vectors", (torch.zeros(9, 3, dtype=torch.float64), SRC, 5), {}),
    ("steering_vectors", (torch.zeros(0, 3, dtype=torch.float64), SRC, 5), {}),
    ("steering_vectors", (MICS, SRC, 0), {}), ("steering_vectors", (MICS, SRC, 5.0), {}),
    ("steering_vectors", (MICS, SRC, 5), {"fs": 0}), ("steering_vectors", (MICS, SRC, 5), {"fs": float("nan")}),
    ("steering_vectors", (MICS, SRC, 5), {"c": -340.0}), ("steering_vectors", (MICS, SRC, 5), {"n_fft": 1}),
    ("steering_vectors", (MICS, SRC, 5), {"ref": 3}), ("steering_vectors", (MICS, SRC, 5), {"ref": -1}),
    ("steering_vectors", (MICS, SRC, 5), {"ref": True}),
    ("weights", ("gev", COV, STEER), {}), ("weights", (None, COV, STEER), {}), ("weights", (1, COV, STEER), {}),
    ("weights", ("das",), {}), ("weights", ("das", COV, STEER), {}), ("weights", ("mvdr", COV), {}),
    ("weights", ("mvdr", None, STEER), {}), ("weights", ("mvdr", COV, STEER, COV), {}), ("weights", ("souden", COV, STEER), {}),
    ("weights", ("souden", COV), {}), ("weights", ("souden", COV, None, COV[:1]), {}),
    ("weights", ("mvdr", COV.to(torch.complex64), STEER), {}), ("weights", ("mvdr", COV[0], STEER), {}),
    ("weights", ("mvdr", COV, STEER[0]), {}), ("weights", ("mvdr", COV[:, :, :2, :2], STEER), {}),
    ("weights", ("mvdr", COV[:, :4], STEER), {}), ("weights", ("mvdr", COV[0, 0], STEER), {}),
    ("weights", ("das", None, torch.zeros(2, 9, 5, dtype=torch.complex128)), {}),
    ("weights", ("mvdr", COV, STEER), {"loading": -1e-3}), ("weights", ("mvdr", COV, STEER), {"loading": float("inf")}),
    ("weights", ("mvdr", COV, STEER), {"loading": float("nan")}), ("weights", ("mvdr", COV, STEER), {"loading": None}),
    ("weights", ("mvdr", COV, STEER), {"ref": 3}), ("weights", ("mvdr", COV, STEER), {"ref": -1}),
    ("weights", ("mvdr", COV, STEER), {"ref": 1.0}),
] + [("delay_and_sum", (s, MICS, SRC), {}) for s in BAD_SPECS] + [
    ("delay_and_sum", (SPEC, MICS[:2], SRC), {}), ("delay_and_sum", (SPEC, MICS.float(), SRC), {}),
    ("delay_and_sum", (SPEC, MICS, SRC[:1]), {}), ("delay_and_sum", (SPEC[0], MICS, SRC), {}),
    ("delay_and_sum", (SPEC[0], MICS[None], SRC[0]), {}), ("delay_and_sum", (SPEC, MICS, None), {}),
    ("delay_and_sum", (SPEC, MICS, SRC), {"ref": 3}), ("delay_and_sum", (SPEC, MICS, SRC), {"fs": -1.0}),
    ("delay_and_sum", (SPEC, MICS, SRC), {"n_fft": 0}), ("delay_and_sum", (SPEC, MICS, SRC), {"c": 0}),
] + [("mvdr", (s, MICS, SRC), {}) for s in BAD_SPECS] + [
    # every illegal combination of geometry and masks
    ("mvdr", (SPEC,), {}), ("mvdr", (SPEC, MICS), {}), ("mvdr", (SPEC, None, SRC), {}),
    ("mvdr", (SPEC,), {"noise_mask": MASK}), ("mvdr", (SPEC,), {"speech_mask": MASK}),
    ("mvdr", (SPEC, MICS, SRC), {"speech_mask": MASK}), ("mvdr", (SPEC, MICS, SRC), {"noise_mask": MASK, "speech_mask": MASK}),
    ("mvdr", (SPEC, MICS), {"noise_mask": MASK, "speech_mask": MASK}),
    ("mvdr", (SPEC, None, SRC), {"noise_mask": MASK, "speech_mask": MASK}),
    ("mvdr", (SPEC, MICS, SRC), {"noise_mask": MASK[:1]}), ("mvdr", (SPEC, MICS, SRC), {"noise_mask": MASK.float()}),
    ("mvdr", (SPEC,), {"noise_mask": MASK, "speech_mask": MASK[:, :4]}), ("mvdr", (SPEC[0],), {"noise_mask": MASK, "speech_mask": MASK}),
    ("mvdr", (SPEC, MICS[:2], SRC), {}), ("mvdr", (SPEC, MICS, SRC[0, :2]), {}),
    ("mvdr", (SPEC, MICS, SRC), {"ref": 3}), ("mvdr", (SPEC, MICS, SRC), {"ref": -1}),
    ("mvdr", (SPEC, MICS, SRC), {"loading": -1.0}), ("mvdr", (SPEC, MICS, SRC), {"loading": float("nan")}),
    ("mvdr", (SPEC, MICS, SRC), {"fs": 0.0}), ("mvdr", (SPEC, MICS, SRC), {"n_fft": 1}),
    ("beamform_waves", (WAVES[0], MICS, SRC), {}), ("beamform_waves", (WAVES.half(), MICS, SRC), {}),
    ("beamform_waves", ("waves", MICS, SRC), {}), ("beamform_waves", (torch.zeros(2, 9, 800), MICS, SRC), {}),
    ("beamform_waves", (torch.zeros(2, 3, 0), MICS, SRC), {}), ("beamform_waves", (WAVES, MICS, SRC), {"method": "souden"}),
    ("beamform_waves", (WAVES, MICS, SRC), {"method": "das", "noise_mask": MASK}),
    ("beamform_waves", (WAVES, MICS, SRC), {"hop": 0}), ("beamform_waves", (WAVES, MICS, SRC), {"n_fft": 1}),
    # the rules of mvdr and delay_and_sum, under this function's name
    ("beamform_waves", (WAVES, MICS, SRC), {"ref": 9}), ("beamform_waves", (WAVES, MICS, SRC), {"loading": -1.0}),
    ("beamform_waves", (WAVES, MICS, SRC), {"method": "das", "ref": 3}), ("beamform_waves", (WAVES, MICS[:2], SRC), {}),
    ("beamform_waves", (WAVES, MICS, SRC[:1]), {"method": "das"}), ("beamform_waves", (WAVES, MICS), {}),
    ("beamform_waves", (WAVES,), {"noise_mask": MASK}), ("beamform_waves", (WAVES, MICS, SRC), {"speech_mask": MASK}),
    ("beamform_waves", (WAVES, MICS, SRC), {"noise_mask": MASK}),                       # 800 samples are 6 frames of 201 bins, not (5, 20)
    ("beamform_waves", (WAVES, MICS, SRC), {"fs": 0}), ("beamform_waves", (WAVES, MICS, SRC), {"c": float("inf")}),
    ("beamform_waves", (torch.zeros(1, 1, 70000), MICS[:1], SRC[0]), {"hop": 1, "n_fft": 2}),    # 70 001 frames
]


@pytest.mark.parametrize("name,args,kwargs", RULES, ids=["%s-%d" % (r[0], i) for i, r in enumerate(RULES)])
def test_argument_rules(name, args, kwargs):
    with pytest.raises(ValueError, match="^%s: " % name):
        getattr(BF, name)(*args, **kwargs)


def test_locate_and_beamform_argument_rules():
    cand = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="^srp_phat: "):                                   # the localiser's own rules
        BF.locate_and_beamform(SPEC.real, MICS, cand)
    with pytest.raises(ValueError, match="^srp_phat: "):
        BF.locate_and_beamform(torch.zeros(2, 3, 201, 20, dtype=torch.complex64), MICS, cand[:, :2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BF.locate_and_beamform(torch.zeros(2, 3, 201, 20, dtype=torch.complex64), MICS, cand)


def test_cpu_tensors_are_refused_last():
    calls = [lambda: BF.spatial_covariance(SPEC), lambda: BF.spatial_covariance(SPEC[0], MASK[0]),
             lambda: BF.steering_vectors(MICS, SRC, 5), lambda: BF.steering_vectors(MICS, SRC[0], 5),
             lambda: BF.weights("das", steering=STEER), lambda: BF.weights("mvdr", COV, STEER),
             lambda: BF.weights("souden", COV[0], speech_cov=COV[0]), lambda: BF.apply(SPEC, W), lambda: BF.apply(SPEC[1], W[1]),
             lambda: BF.delay_and_sum(SPEC, MICS, SRC), lambda: BF.mvdr(SPEC, MICS, SRC),
             lambda: BF.mvdr(SPEC.to(torch.complex64), MICS, SRC, noise_mask=MASK),
             lambda: BF.mvdr(SPEC, noise_mask=MASK, speech_mask=MASK), lambda: BF.mvdr(SPEC[0], MICS, SRC[0]),
             lambda: BF.beamform_waves(WAVES, MICS, SRC), lambda: BF.beamform_waves(WAVES.double(), noise_mask=WAVE_MASK, speech_mask=WAVE_MASK)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="^mvdr: ref"):                                    # the ranges come first
        BF.mvdr(SPEC, MICS, SRC, ref=5)
    with pytest.raises(ValueError, match="^weights: loading"):
        BF.weights("mvdr", COV, STEER, loading=-1.0)
    with pytest.raises(ValueError, match="^steering_vectors: fs"):
        BF.steering_vectors(MICS, SRC, 5, fs=0)
    with pytest.raises(ValueError, match="^beamform_waves: ref"):
        BF.beamform_waves(WAVES, MICS, SRC, ref=9)
    with pytest.raises(ValueError, match="^beamform_waves: loading"):
        BF.beamform_waves(WAVES, MICS, SRC, loading=float("nan"))
    for name, call in (("delay_and_sum", lambda: BF.delay_and_sum(SPEC, MICS, SRC)), ("mvdr", lambda: BF.mvdr(SPEC, MICS, SRC)),
                       ("beamform_waves", lambda: BF.beamform_waves(WAVES, MICS, SRC))):
        with pytest.raises(RuntimeError, match="^%s: .*no CPU fallback" % name):       # under the name that was called
            call()
