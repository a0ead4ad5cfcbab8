"""The Hermitian eigensolver, MUSIC and the GEV beamformer, the parts that need no GPU: the numpy restatement
(tests/helpers/subspace_ref.py) is pinned -- float64 against np.longdouble to the bounds tests/test_subspace_gpu.py holds the
device to (its docstring derives them), its eigenvalues against numpy.linalg.eigh, on inputs whose sources it must find, on the
items it must flag -- and the constants c1, c2 of those bounds are measured here and held to the rule that set them; then the
host-side argument rules of ``subspace.eigh``, ``localization.music`` / ``music_from_covariance`` / ``locate_on_ring`` and
``beamforming.gev_weights`` / ``gev``."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import beamform_ref as BR  # noqa: E402
import dsp_ref  # noqa: E402
import rir_ref  # noqa: E402
import srp_ref  # noqa: E402
import subspace_ref as R  # noqa: E402
from acoustic_locating_vq_vae import beamforming as BF  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import localization as LOC  # noqa: E402

LD = np.longdouble
U = R.U
SRP_IDS = ["-".join(str(v) for v in s) for s in srp_ref.PARITY]
BF_IDS = ["-".join(str(v) for v in s) for s in BR.PARITY]
N_EACH = 5          # matrices of every (kind, D)


# ------------------------------------------------------------------------------------------------------------ the eigensolver
@functools.lru_cache(maxsize=None)
def eig_pair(kind, D):
    A = R.eig_case(kind, D, N_EACH)
    return A, R.eigh(A), R.eigh(A, LD, 2 * R.MAX_SWEEPS)


@functools.lru_cache(maxsize=None)
def music_ratios(shape, K):
    """The eigensolver's ratios on a MUSIC case's covariances (the projector's among them) and the map's errors against
    longdouble: (ratios to c1 = 1, map alone / bound, chain error, chain bound at c1 = 1 less the map-alone bound)."""
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c, ref = srp_ref.parity_case(shape), R.music_reference(shape, K)
    eld = R.eigh(ref.cov, LD, 2 * R.MAX_SWEEPS)
    assert not eld.status.any()
    band = slice(f_lo, f_hi + 1)
    dP = np.abs(R.projector(ref.V, K).astype(np.clongdouble) - R.projector(eld.V, K))[:, band].max(axis=(-2, -1))
    ratios = R.eig_errors(ref.cov, ref.lam, ref.V, eld.lam) + (float((dP / R.projector_bound(D, ref.norms, ref.gaps, 1)).max()),)
    alone_ld, _, _ = R.music(ref.V, ref.lam, c.mics, c.cand, K, R.FS, n_fft, R.C, f_lo, f_hi, LD)
    chain_ld, best_ld, _ = R.music(eld.V, eld.lam, c.mics, c.cand, K, R.FS, n_fft, R.C, f_lo, f_hi, LD)
    assert np.array_equal(best_ld, ref.best)
    return (ratios, float(np.abs(ref.null - alone_ld).max() / ref.bound_alone), np.abs(ref.null - chain_ld).max(axis=1),
            np.mean(2 * D * U * ref.norms / ref.gaps, axis=1))


@pytest.mark.parametrize("D", range(1, 9))
@pytest.mark.parametrize("kind", R.EIG_KINDS)
def test_eigh_restatement_against_longdouble_and_numpy(kind, D):
    A, e64, eld = eig_pair(kind, D)
    assert not e64.status.any() and not eld.status.any()
    res, orth, err = R.eig_errors(A, e64.lam, e64.V, eld.lam)
    nf = R.frobenius(A)
    e_np = float(np.max(np.abs(e64.lam - np.linalg.eigvalsh(A)).max(axis=-1) / np.where(nf > 0, D * U * nf, 1)))
    print("%s D=%d: residual %.3g, orthogonality %.3g, eigenvalues %.3g (numpy %.3g) of D u ||A||_F; c1 = %d"
          % (kind, D, res, orth, err, e_np, R.C1))
    assert max(res, orth, err, e_np) <= R.C1
    assert (np.diff(e64.lam, axis=-1) >= 0).all()
    top = np.take_along_axis(e64.V, np.argmax(e64.V.real ** 2 + e64.V.imag ** 2, axis=1)[:, None, :], axis=1)
    assert (top.imag == 0).all() and (top.real > 0).all()                 # the phase rule
    if kind in ("identity", "zero"):
        assert (e64.V == np.eye(D)).all() and (e64.lam == (1 if kind == "identity" else 0)).all()


def test_eigh_restatement_reads_the_lower_triangle_and_flags_bad_input():
    A = R.eig_case("full", 4, 3).copy()
    want = R.eigh(A)
    A[:, 0, 3] = np.nan                                                   # above the diagonal: not read
    A[:, 2, 2] += complex(0, np.inf)                                      # the diagonal's imaginary part: not read
    got = R.eigh(A)
    assert np.array_equal(got.lam, want.lam) and np.array_equal(got.V, want.V) and not got.status.any()
    A[1, 3, 1] = np.inf
    got = R.eigh(A)
    assert list(got.status) == [0, R.EIG_BAD_INPUT, 0] and np.isnan(got.lam[1]).all() and np.isnan(got.V[1].real).all()
    assert np.array_equal(got.lam[[0, 2]], want.lam[[0, 2]])
    assert list(R.eigh(R.eig_case("full", 6, 2), max_sweeps=1).status) == [R.EIG_NO_CONVERGENCE] * 2


def test_constants_are_four_times_the_measured_ratio():
    """c1: the worst of residual, orthogonality, eigenvalue error and projector error, float64 against longdouble, over every
    eigensolver kind and every MUSIC case; c2: the worst GEV weight / rtf error over every beamform_ref.PARITY shape, mask,
    variant and reference.  Each constant is the next power of two at or above 4 x the worst ratio."""
    w1 = max(max(R.eig_errors(A, e64.lam, e64.V, eld.lam)) for A, e64, eld in (eig_pair(k, D) for k in R.EIG_KINDS for D in range(1, 9)))
    w1 = max([w1] + [max(music_ratios(s, K)[0]) for s in srp_ref.PARITY for K in R.music_orders(s[1])])
    w2 = max(gev_ratio(s, kind, variant, ref) for s in BR.PARITY for kind in BR.MASKS for variant in R.GEV_VARIANTS
             for ref in sorted({0, s[1] - 1}))
    print("worst ratios: eigensolver %.4g (c1 = %d), GEV %.4g (c2 = %d)" % (w1, R.C1, w2, R.C2))
    for worst, const, noted in ((w1, R.C1, R.C1_MEASURED), (w2, R.C2, R.C2_MEASURED)):
        assert const / 2 < 4 * worst <= const, (worst, const)
        assert abs(worst - noted) <= 0.25 * noted, (worst, noted)      # the figure the helper quotes


# ----------------------------------------------------------------------------------------------------------------------- MUSIC
MUSIC_CASES = [(s, K) for s in srp_ref.PARITY for K in R.music_orders(s[1])]
MUSIC_IDS = ["%s-K%d" % ("-".join(str(v) for v in s), K) for s, K in MUSIC_CASES]


@pytest.mark.parametrize("shape,K", MUSIC_CASES, ids=MUSIC_IDS)
def test_music_restatement_finds_the_true_candidate(shape, K):
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c, ref = srp_ref.parity_case(shape), R.music_reference(shape, K)
    print("%s K=%d: arg-min %s, true %s, margin %s, least relative eigengap %.3g"
          % (shape, K, ref.best, c.true, ref.margin, float((ref.gaps / ref.norms).min())))
    assert not ref.status.any()
    assert np.array_equal(ref.best, c.true) and np.array_equal(ref.best, srp_ref.reference(shape).best)
    single = R.music_reference(shape, K, single=True)
    assert np.array_equal(single.best, c.true)


@pytest.mark.parametrize("shape,K", MUSIC_CASES, ids=MUSIC_IDS)
def test_music_restatement_against_longdouble(shape, K):
    B, D, T, G, f_lo, f_hi, n_fft = shape
    ratios, alone, chain_err, chain_term = music_ratios(shape, K)
    bound = R.music_reference(shape, K).bound_alone + R.C1 * chain_term
    print("%s K=%d: eigensolver ratios %s; map alone / bound %.3g; chain / bound %.3g"
          % (shape, K, ["%.3g" % r for r in ratios], alone, float((chain_err / bound).max())))
    assert max(ratios) <= R.C1 and alone <= 1 and (chain_err <= bound).all()


ROOM_ANGLES = (5, 23, 40, 61)


@pytest.mark.parametrize("k", ROOM_ANGLES)
def test_music_restatement_locates_a_source_in_the_room(k):
    """The room of tests/test_srp_cpu.py (DATASET_CONFIG: T60 0.4 s, four microphones on a tetrahedron of radius 0.05 m, one
    second of noise under an envelope, 72 ring candidates, band (8, 187)): rir_ref.rir -> dsp_ref.fir_same -> dsp_ref.stft ->
    the restatement; the arg-min lies within one ring candidate of the source's, the criterion SRP-PHAT meets there."""
    cfg = FE.DATASET_CONFIG
    fs, n = cfg["fs"], 16000
    g = np.random.default_rng(3)
    t = np.arange(n) / fs
    envelope = (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + 0.3)) * (0.6 + 0.4 * np.sin(2 * np.pi * 1.3 * t))
    wave = (g.standard_normal(n) * envelope).astype(np.float32)
    rcv = np.array(cfg["receiver_position"], dtype=np.float64)
    mics = rcv + 0.05 / np.sqrt(3.0) * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)
    room = np.array(cfg["room_dimensions"], dtype=np.float64)
    cand = np.minimum(srp_ref.ring(72, rcv, cfg["R"], cfg["Z_LOC_SOURCE"]), room)
    beta = rir_ref.sabine_beta(room, FE.SOUND_SPEED, cfg["reverberation_time"])
    h = np.stack([rir_ref.rir(FE.SOUND_SPEED, fs, m, cand[k], room, beta, cfg["n_sample"]) for m in mics])
    echoed = dsp_ref.fir_same(np.broadcast_to(wave.astype(np.float64), (4, wave.size)), h)[0]
    X = dsp_ref.stft(echoed, 400, 160)[0].astype(np.complex128)[None]
    e = R.eigh(BR.covariance(X)[0])
    null, best, status = R.music(e.V, e.lam, mics, cand, 1, fs, 400, FE.SOUND_SPEED, 8, 187)
    dist = min((int(best[0]) - k) % 72, (k - int(best[0])) % 72)
    print("source on candidate %d: arg-min %d, null %.4f" % (k, best[0], null[0].min()))
    assert status[0] == 0 and not e.status.any() and dist <= 1


@pytest.mark.parametrize("D,T,G", R.TWO_SOURCE)
def test_music_restatement_resolves_two_sources(D, T, G):
    c, ref = R.two_source_case(D, T, G), R.two_source_reference(D, T, G)
    mins = R.local_minima(ref.null[0])
    depth = ref.null[0][mins]
    print("D=%d T=%d G=%d: true %s, local minima %s at depths %s" % (D, T, G, c.true, mins[:4], depth[:4]))
    assert sorted(mins[:2]) == list(c.true)
    assert len(mins) == 2 or depth[2] > 100 * depth[1]
    assert not ref.status.any()


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_music_restatement_flags_bad_items(dtype):
    shape = srp_ref.PARITY[1]
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c, ref = srp_ref.parity_case(shape), R.music_reference(shape, 1)
    V = np.concatenate([ref.V, ref.V[:1], ref.V[:1], ref.V[:1]])
    lam = np.concatenate([ref.lam, ref.lam[:1], ref.lam[:1], ref.lam[:1]])
    lam[0, f_lo:f_hi + 1] = 0                         # every bin of the band silent
    V[1, f_lo + 3, 1, 2] = complex(1.0, np.nan)       # one NaN inside the band
    V[2, f_hi + 1, 0, 0] = np.nan                     # a NaN outside the band does not flag
    lam[2, f_lo + 1] = 0                              # one silent bin is left out of the mean
    lam[4, f_hi, 0] = np.inf                          # a non-finite eigenvalue
    mics = np.broadcast_to(c.mics, (5, D, 3)).copy()
    mics[3, 1, 2] = np.nan
    null, best, status = R.music(V, lam, mics, c.cand, 1, R.FS, n_fft, R.C, f_lo, f_hi, dtype)
    assert list(status) == [2, 1, 0, 4, 1] and list(best) == [-1, -1, c.true[0], -1, -1]
    assert (null[0] == 1).all() and np.isnan(null[[1, 3, 4]]).all() and np.isfinite(null[2]).all()
    keep = np.ones(lam.shape[1], bool)
    keep[f_lo + 1] = False
    keep[:f_lo], keep[f_hi + 1:] = False, False
    Fb = f_hi - f_lo + 1
    per_bin = R.music(ref.V[:1], ref.lam[:1], c.mics, c.cand, 1, R.FS, n_fft, R.C, f_lo + 1, f_lo + 1, dtype)[0]
    want = (ref.null[:1].astype(dtype) * Fb - per_bin) / (Fb - 1)
    assert np.abs(null[2] - want[0]).max() <= 1e-12
    cand = c.cand.copy()
    cand[5, 0] = np.inf
    assert list(R.music(V, lam, c.mics, cand, 1, R.FS, n_fft, R.C, f_lo, f_hi, dtype)[2]) == [6, 5, 4, 4, 5]


# ------------------------------------------------------------------------------------------------------------------------- GEV
@functools.lru_cache(maxsize=None)
def gev_ratio(shape, kind, variant, ref):
    """The largest |w - w_ld| and |rtf - rtf_ld| over the bound at c2 = 1."""
    B, D, F, T, loading = shape
    g = R.gev_reference(shape, kind, variant, ref)
    ld = R.gev(g.Phi_n, g.Phi_s, ref, loading, LD)
    assert not ld.status.any()
    worst = 0.0
    for a, b in ((g.out.W, ld.W), (g.out.rtf, ld.rtf)):
        bound = R.gev_bound(D, g.cond, g.normC, g.gapC, np.abs(a).max(axis=-1), 1)
        worst = max(worst, float((np.abs(a - b).max(axis=-1) / bound).max()))
    return worst


@pytest.mark.parametrize("kind", BR.MASKS)
@pytest.mark.parametrize("shape", BR.PARITY, ids=BF_IDS)
def test_gev_restatement_against_longdouble(shape, kind):
    B, D, F, T, loading = shape
    for variant in R.GEV_VARIANTS:
        for ref in sorted({0, D - 1}):
            ratio = gev_ratio(shape, kind, variant, ref)
            out = R.gev_reference(shape, kind, variant, ref).out
            one = np.sum(np.conj(out.W) * out.rtf, axis=-1)
            print("%s %s %s ref %d: largest error / bound at c2 = 1: %.3g; |w^H rtf - 1| %.3g" % (shape[:4], kind, variant, ref, ratio,
                                                                                                  np.abs(one - 1).max()))
            assert ratio <= R.C2
            assert (out.rtf[..., ref] == 1).all()
            if D == 1:
                assert (out.W == 1).all() and (out.rtf == 1).all()


@pytest.mark.parametrize("kind", BR.MASKS)
@pytest.mark.parametrize("shape", BR.PARITY, ids=BF_IDS)
def test_gev_on_rank_one_speech_is_the_mvdr(shape, kind):
    """With Phi_s = sigma a a^H the top eigenvector of the whitened matrix is L^-1 a: w = Phi'^-1 a / (a^H Phi'^-1 a), the MVDR
    weights of beamform_ref, and rtf = a.  Each side lies within its own bound of the exact value: 8 D u cond max |w| for the
    Cholesky solve, c2 D u cond (1 + ||C||_F / gap) max |w| for the GEV; the gain is the maximum of the Rayleigh quotient."""
    B, D, F, T, loading = shape
    c, r, g = BR.parity_case(shape), BR.reference(shape, kind), R.gev_reference(shape, kind, "rank1")
    want = r.W["mvdr"]
    wmax = np.abs(want).max(axis=-1)
    bound = BR.weights_bound(D, g.cond, wmax) + R.gev_bound(D, g.cond, g.normC, g.gapC, wmax, R.C2)
    err = np.abs(g.out.W - want).max(axis=-1)
    A = np.moveaxis(c.A, 1, 2)
    err_a = np.abs(g.out.rtf - A).max(axis=-1)
    print("%s %s: |w_gev - w_mvdr| / bound %.3g (over 0.5 D u cond max |w|: %.3g); |rtf - a| / bound %.3g"
          % (shape[:4], kind, float((err / bound).max()), float((err / (0.5 * D * U * g.cond * wmax)).max()),
             float((err_a / R.gev_bound(D, g.cond, g.normC, g.gapC, 1.0, R.C2)).max())))
    assert (err <= bound).all()
    assert (err_a <= R.gev_bound(D, g.cond, g.normC, g.gapC, 1.0, R.C2)).all()
    P = BR.loaded(g.Phi_n, loading)

    def quotient(w):
        num = np.einsum("bfi,bfij,bfj->bf", np.conj(w), g.Phi_s, w).real
        return num / np.einsum("bfi,bfij,bfj->bf", np.conj(w), P, w).real
    slack = 1 - R.gev_bound(D, g.cond, g.normC, g.gapC, 1.0, R.C2)
    assert (quotient(g.out.W) >= quotient(r.W["souden"]) * slack).all()
    assert (np.abs(quotient(g.out.W) - g.out.gain) <= R.gev_bound(D, g.cond, g.normC, g.gapC, g.out.gain, R.C2)).all()


def test_gev_restatement_flags_bad_bins():
    shape = BR.PARITY[2]
    B, D, F, T, loading = shape
    g = R.gev_reference(shape, "uniform", "full")
    Phi_n, Phi_s = g.Phi_n.copy(), g.Phi_s.copy()
    Phi_n[0, 0] = 0                                   # a pivot of 0
    Phi_s[0, 1] = 0                                   # lambda_max = 0
    Phi_s[0, 2, 1, 0] = np.nan                        # a non-finite whitened matrix
    out = R.gev(Phi_n, Phi_s, D - 1, loading)
    assert list(out.status[0]) == [2, 2, 2, 0]
    e_ref = np.zeros(D)
    e_ref[D - 1] = 1
    for f in range(3):
        assert (out.W[0, f] == e_ref).all() and (out.rtf[0, f] == e_ref).all() and out.gain[0, f] == 0
    assert np.array_equal(out.W[0, 3], R.gev(g.Phi_n, g.Phi_s, D - 1, loading).W[0, 3])


# ----------------------------------------------------------------------------------------------------------------- host checks
SPEC = torch.zeros(2, 4, 201, 6, dtype=torch.complex128)
MICS = torch.zeros(4, 3, dtype=torch.float64)
CAND = torch.zeros(9, 3, dtype=torch.float64)
COV = torch.zeros(2, 201, 4, 4, dtype=torch.complex128)
MASK = torch.ones(2, 201, 6, dtype=torch.float64)


@pytest.mark.parametrize("cov", [COV.real, COV.to(torch.complex64), COV[0, 0, 0], COV[..., :3], "cov", COV[:0],
                                 torch.zeros(3, 9, 9, dtype=torch.complex128), torch.zeros(3, 0, 0, dtype=torch.complex128)])
def test_eigh_argument_rules(cov):
    from acoustic_locating_vq_vae import subspace as SUB
    with pytest.raises(ValueError, match="^eigh: "):
        SUB.eigh(cov)


@pytest.mark.parametrize("spec,mics,cand,kwargs", [
    (SPEC.real, MICS, CAND, {}), (SPEC[0, 0], MICS, CAND, {}), ("spec", MICS, CAND, {}),
    (torch.zeros(1, 1, 201, 6, dtype=torch.complex64), MICS[:1], CAND, {}),           # one microphone
    (torch.zeros(1, 9, 201, 6, dtype=torch.complex64), MICS, CAND, {}),               # nine
    (SPEC, MICS, CAND, {"n_sources": 0}), (SPEC, MICS, CAND, {"n_sources": 4}), (SPEC, MICS, CAND, {"n_sources": 1.0}),
    (SPEC, MICS, CAND, {"n_sources": True}),
    (SPEC, MICS[:3], CAND, {}), (SPEC, MICS.float(), CAND, {}), (SPEC, MICS, CAND[:, :2], {}), (SPEC, MICS, CAND[:0], {}),
    (SPEC, MICS[None].expand(3, 4, 3), CAND, {}), (SPEC, MICS, CAND[None].expand(3, 9, 3), {}),
    (SPEC, MICS, CAND, {"fs": 0.0}), (SPEC, MICS, CAND, {"c": float("nan")}), (SPEC, MICS, CAND, {"n_fft": 402}),
    (SPEC, MICS, CAND, {"band": (9, 3)}), (SPEC, MICS, CAND, {"band": (0, 201)}),
])
def test_music_argument_rules(spec, mics, cand, kwargs):
    with pytest.raises(ValueError, match="^music: "):
        LOC.music(spec, mics, cand, **kwargs)


@pytest.mark.parametrize("cov,kwargs", [
    (COV.real, {}), (COV.to(torch.complex64), {}), (COV[0, 0], {}), (COV[..., :3], {}), ("cov", {}),
    (torch.zeros(2, 201, 1, 1, dtype=torch.complex128), {}), (torch.zeros(2, 201, 9, 9, dtype=torch.complex128), {}),
    (COV[:, :200], {}), (COV[:0], {}),
    (COV, {"n_sources": 4}), (COV, {"n_sources": 0}), (COV, {"band": (5, 4)}), (COV, {"fs": -1.0}), (COV, {"n_fft": 400.0}),
])
def test_music_from_covariance_argument_rules(cov, kwargs):
    with pytest.raises(ValueError, match="^music_from_covariance: "):
        LOC.music_from_covariance(cov, MICS, CAND, **kwargs)


def test_locate_on_ring_method_rules():
    with pytest.raises(ValueError, match="^locate_on_ring: method"):
        LOC.locate_on_ring(SPEC, MICS, [2.5, 1.5, 1.5], [4, 5, 3], 1, 1, method="gcc")
    with pytest.raises(ValueError, match="^locate_on_ring: n_sources"):
        LOC.locate_on_ring(SPEC, MICS, [2.5, 1.5, 1.5], [4, 5, 3], 1, 1, n_sources=2)


@pytest.mark.parametrize("noise,speech,kwargs", [
    (COV.real, COV, {}), (COV, COV.to(torch.complex64), {}), (COV, COV[0], {}), (COV[0, 0], COV[0, 0], {}), (None, COV, {}),
    (COV, COV[:, :5], {}), (COV, COV[..., :3, :3], {}), (torch.zeros(2, 5, 9, 9, dtype=torch.complex128),) * 2 + ({},),
    (COV[..., :3], COV[..., :3], {}),
    (COV, COV, {"ref": 4}), (COV, COV, {"ref": -1}), (COV, COV, {"ref": 1.0}), (COV, COV, {"loading": -1e-3}),
    (COV, COV, {"loading": float("inf")}), (COV, COV, {"loading": "1e-6"}),
])
def test_gev_weights_argument_rules(noise, speech, kwargs):
    with pytest.raises(ValueError, match="^gev_weights: "):
        BF.gev_weights(noise, speech, **kwargs)


@pytest.mark.parametrize("spec,noise,speech,kwargs", [
    (SPEC.real, MASK, MASK, {}), (SPEC[0, 0], MASK, MASK, {}), (SPEC, None, MASK, {}), (SPEC, MASK, None, {}),
    (SPEC, MASK.float(), MASK, {}), (SPEC, MASK, MASK[0], {}), (SPEC, MASK[:, :, :5], MASK, {}), (SPEC[0], MASK, MASK, {}),
    (SPEC, MASK, MASK, {"ref": 4}), (SPEC, MASK, MASK, {"loading": -1.0}),
])
def test_gev_argument_rules(spec, noise, speech, kwargs):
    with pytest.raises(ValueError, match="^gev: "):
        BF.gev(spec, noise, speech, **kwargs)


def test_cpu_tensors_are_refused_last():
    from acoustic_locating_vq_vae import subspace as SUB
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SUB.eigh(COV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SUB.eigh(COV[0, 0])
    for spec in (SPEC, SPEC[0], SPEC.to(torch.complex64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            LOC.music(spec, MICS, CAND, n_sources=3)
    with pytest.raises(ValueError, match="^music: band"):                # the ranges come first
        LOC.music(SPEC, MICS, CAND, band=(9, 3))
    for cov in (COV, COV[0]):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            LOC.music_from_covariance(cov, MICS, CAND, n_sources=2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            BF.gev_weights(cov, cov, ref=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LOC.locate_on_ring(SPEC, MICS, [2.5, 1.5, 1.5], [4, 5, 3], 1, 1, method="music", n_sources=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BF.gev(SPEC, MASK, MASK)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BF.gev(SPEC[0], MASK[0], MASK[0], ref=3)
    with pytest.raises(ValueError, match="method must be one of"):       # the GEV is no mode of weights()
        BF.weights("gev", COV, speech_cov=COV)
