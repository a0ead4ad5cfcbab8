"""Beamforming on the device (csrc/beamform.hip, acoustic_locating_vq_vae.beamforming) against the float64 restatement of
tests/helpers/beamform_ref.py, which tests/test_beamform_cpu.py pins.  u = 1.1e-16.

Covariance, per entry:   |Phi_dev - Phi_ref| <= 2 (T + 4) u S_ij, S_ij = sum_t m_t |x_i| |x_j| / sum_t m_t -- both sides lie within
                         (T + 4) u S_ij, the bound of a T-term sum in any order, of the exact value.  A float32 accumulation
                         is six orders above it.  complex64: the restatement of the promoted input, the same bound.
Steering:                |A_dev - A_ref| <= (16 Theta + 32) u, Theta the largest phase in radians (srp_ref.map_bound's term).
Weights, per bin:        max |w_dev - w_ref| <= 16 D u cond_2(Phi') max |w_ref| from the restatement's own Phi, uploaded, so that
                         only the solve differs: the forward bound 8 D u cond of a Cholesky solve, once for each side.  Every
                         bin's cond is <= 1e6 (beamform_ref.case asserts it), so no bin hides behind its conditioning.
Apply, per output:       |y_dev - y_ref| <= 2 (D + 2) u sum_d |w_d| |x_d[t]| with the device's own W given to the restatement;
                         complex64: 6e-8 |y_ref| more for the one rounding of Y."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import beamform_ref as R  # noqa: E402
import srp_ref  # noqa: E402
from parity_checks import check_cov  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import beamforming as BF  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as SM  # noqa: E402

U = R.U
IDS = ["-".join(str(v) for v in s) for s in R.PARITY]


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()          # a copy: the shared cases are read-only


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    """Two tensors equal bit for bit, NaN included."""
    ra, rb = (torch.view_as_real(t.resolve_conj().contiguous()) if t.is_complex() else t.contiguous() for t in (a, b))
    if ra.shape != rb.shape or ra.dtype != rb.dtype:
        return False
    view = {torch.float64: torch.int64, torch.float32: torch.int32}.get(ra.dtype)
    return torch.equal(ra.view(view), rb.view(view)) if view else torch.equal(ra, rb)


def mask_of(c, kind):
    return None if kind == "ones" else dev(c.masks[kind])         # "ones": the null mask, which the restatement takes as 1


def hermitian_bits(cov):
    """Above the diagonal the conjugate of below it (the real part's bits, the negated imaginary part's bits), on it an
    imaginary part of +0."""
    D = cov.shape[-1]
    i, j = torch.tril_indices(D, D, -1)
    low, up = cov[..., i, j], cov[..., j, i]
    diag = torch.diagonal(cov, dim1=-2, dim2=-1).imag
    return same_bits(up.real, low.real) and same_bits(up.imag, -low.imag) and same_bits(diag, torch.zeros_like(diag))


# ------------------------------------------------------------------------------------------------------- covariance parity
@pytest.mark.parametrize("kind", R.MASKS)
@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
def test_covariance_parity_complex128(shape, kind):
    B, D, F, T, _ = shape
    c, ref = R.parity_case(shape), R.reference(shape, kind)
    got = BF.spatial_covariance(dev(c.X), mask_of(c, kind))
    assert got.cov.dtype == torch.complex128 and got.cov.shape == (B, F, D, D)
    assert got.status.dtype == torch.int32 and got.status.shape == (B, F) and not host(got.status).any()
    assert hermitian_bits(got.cov)
    check_cov(got.cov, ref.cov, ref.scale, T, "complex128 %s %s" % (shape[:4], kind))


@pytest.mark.parametrize("kind", R.MASKS)
@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
def test_covariance_parity_complex64(shape, kind):
    B, D, F, T, _ = shape
    c, ref = R.parity_case(shape), R.reference(shape, kind, single=True)
    got = BF.spatial_covariance(dev(c.X.astype(np.complex64)), mask_of(c, kind))
    assert got.cov.dtype == torch.complex128 and not host(got.status).any() and hermitian_bits(got.cov)
    check_cov(got.cov, ref.cov, ref.scale, T, "complex64 %s %s" % (shape[:4], kind))


# --------------------------------------------------------------------------------------------------------- steering parity
@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
def test_steering_parity(shape):
    B, D, F, T, _ = shape
    c = R.parity_case(shape)
    for ref in (0, D - 1):
        want, _ = R.steering(c.mics, c.source, F, ref=ref)
        A, status = BF.steering_vectors(dev(c.mics), dev(c.source), F, ref=ref)
        assert A.dtype == torch.complex128 and A.shape == (B, D, F) and status.shape == (B,) and not host(status).any()
        err = np.abs(host(A) - want).max()
        bound = R.steering_bound(R.theta_max(c.mics, c.source, F))
        print("%s ref %d: |A - A_ref| %.3g, bound %.3g" % (shape[:4], ref, err, bound))
        assert err <= bound
        assert (host(A)[:, ref] == 1).all()
    batched, _ = BF.steering_vectors(dev(np.broadcast_to(c.mics, (B, D, 3))), dev(c.source), F, ref=D - 1)       # mics per item
    assert same_bits(batched, A)


# ---------------------------------------------------------------------------------------------------------- weights parity
@pytest.mark.parametrize("kind", R.MASKS)
@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
def test_weights_parity(shape, kind):
    B, D, F, T, loading = shape
    c, ref = R.parity_case(shape), R.reference(shape, kind)
    A = dev(c.A)
    runs = {"das": BF.weights("das", steering=A),
            "mpdr": BF.weights("mvdr", dev(ref.cov), A, loading=loading),
            "mvdr": BF.weights("mvdr", dev(ref.cov_n), A, loading=loading),
            "souden": BF.weights("souden", dev(ref.cov_n), speech_cov=dev(ref.cov_s), loading=loading)}
    for name, got in runs.items():
        assert got.w.dtype == torch.complex128 and got.w.shape == (B, F, D) and got.status.shape == (B, F)
        assert not host(got.status).any(), name
        err = np.abs(host(got.w) - ref.W[name]).max(axis=-1)
        if name == "das":
            bound = 2 * U * np.abs(ref.W[name]).max(axis=-1)
        else:
            assert ref.cond[name].max() <= R.COND_CAP
            bound = R.weights_bound(D, ref.cond[name], np.abs(ref.W[name]).max(axis=-1), c=16)
        print("%s %s %s: largest |w - w_ref| / bound %.3g, cond up to %.3g"
              % (shape[:4], kind, name, (err / bound).max(), 1.0 if name == "das" else ref.cond[name].max()))
        assert (err <= bound).all(), (name, (err / bound).max())
        if D == 1 and name != "das":
            assert (host(got.w) == 1).all()
    other = BF.weights("souden", dev(ref.cov_n), speech_cov=dev(ref.cov_s), loading=loading, ref=D - 1)         # another reference
    want, _ = R.weights(R.SOUDEN, ref.cov_n, ref.cov_s, ref=D - 1, loading=loading)
    err = np.abs(host(other.w) - want).max(axis=-1)
    assert (err <= R.weights_bound(D, ref.cond["souden"], np.abs(want).max(axis=-1), c=16)).all()


# ------------------------------------------------------------------------------------------------------------ apply parity
@pytest.mark.parametrize("cdtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
def test_apply_parity(shape, cdtype):
    B, D, F, T, loading = shape
    c = R.parity_case(shape)
    X = c.X.astype(cdtype)
    x = dev(X)
    w = BF.weights("mvdr", BF.spatial_covariance(x).cov, dev(c.A), loading=loading).w
    got = BF.apply(x, w)
    assert got.dtype == x.dtype and got.shape == (B, F, T)
    Xp, W = X.astype(np.complex128), host(w)
    want = R.apply(Xp, W)
    bound = 2 * R.apply_bound(Xp, W) + (6e-8 * np.abs(want) if cdtype == np.complex64 else 0.0)
    err = np.abs(host(got).astype(np.complex128) - want)
    print("%s %s: largest |y - y_ref| / bound %.3g" % (shape[:4], np.dtype(cdtype).name, (err / bound).max()))
    assert (err <= bound).all()


def test_apply_passes_a_microphone_through_bit_for_bit():
    """The two rules of alvq_beamform_apply_* that the restatement does not have, on finite data with a -0.0 in it: a weight
    of exactly 0 adds no term and a weight with an imaginary part of exactly 0 multiplies as a real number, so w = e_ref gives
    x_ref and w = 0 gives +0, as bits; and a NaN under a zero weight does not reach y."""
    shape = R.PARITY[2]
    B, D, F, T, _ = shape
    X = R.parity_case(shape).X.copy()
    X[0, 1, 2, 5] = complex(-0.0, 3.0)
    X[0, 1, 3, 6] = complex(2.0, -0.0)
    X[0, 1, 0, 7] = complex(-0.0, -0.0)
    for cdtype in (np.complex128, np.complex64):
        x = dev(X.astype(cdtype))
        for ref in range(D):
            w = torch.zeros(B, F, D, dtype=torch.complex128, device="cuda")
            w[:, :, ref] = 1
            assert same_bits(BF.apply(x, w), x[:, ref])
        zero = BF.apply(x, torch.zeros(B, F, D, dtype=torch.complex128, device="cuda"))
        assert same_bits(zero, torch.zeros_like(zero))
        poisoned = x.clone()
        poisoned[0, 0] = complex(np.nan, np.inf)
        w = torch.zeros(B, F, D, dtype=torch.complex128, device="cuda")
        w[:, :, 1] = 1
        assert same_bits(BF.apply(poisoned, w), x[:, 1])
        w[:, :, 1] = 0.5                                    # a real weight: both parts halved, exactly
        assert same_bits(BF.apply(poisoned, w), torch.complex(x[:, 1].real * 0.5, x[:, 1].imag * 0.5))


# -------------------------------------------------------------------------------------------------------------- status bins
@pytest.mark.parametrize("cdtype", [np.complex128, np.complex64])
def test_bad_bins_pass_the_reference_microphone_through(cdtype):
    """A bin of zeros, a bin with a NaN and a bin whose mask sums to 0 in one launch: the restatement's status words, the
    reference microphone's row bit for bit; every other bin within the bounds."""
    shape = R.PARITY[1]
    B, D, F, T, loading = shape
    c = R.parity_case(shape)
    X = c.X.astype(cdtype)
    mask = c.masks["uniform"].copy()
    X[0, :, 1] = 0
    X[1, 1, 3, 40] = complex(np.nan, 1.0)               # in the reference microphone's row ...
    X[1, 0, 3, 7] = complex(2.0, np.inf)                # ... and in the other's
    mask[1, 0] = 0
    bad = {(0, 1), (1, 3), (1, 0)}
    Xp = X.astype(np.complex128)
    cov, st = R.covariance(Xp, mask)
    assert st[0, 1] == 0 and st[1, 3] == 1 and st[1, 0] == 1 and st.sum() == 2             # zeros are a valid input ...
    W, st_w = R.weights(R.MVDR, cov, A=c.A, ref=1, loading=loading)
    assert all(st_w[b, f] == 2 for b, f in bad) and st_w.sum() == 6                          # ... that no Cholesky factors
    x, m = dev(X), dev(mask)
    got_cov = BF.spatial_covariance(x, m)
    assert np.array_equal(host(got_cov.status), st)
    for b, f in bad:
        assert not host(got_cov.cov[b, f]).any()
    check_cov(got_cov.cov, cov, R.covariance_scale(Xp, mask), T, "neighbours of the bad bins", skip=bad)
    beam = BF.mvdr(x, dev(c.mics), dev(c.source), noise_mask=m, ref=1, loading=loading)
    assert np.array_equal(host(beam.status), st | st_w)
    # the neighbours' weights: the restatement from the device's own covariance and steering vectors, so that only the solve differs
    A, _ = BF.steering_vectors(dev(c.mics), dev(c.source), F, ref=1)
    dev_cov = host(got_cov.cov)
    want, _ = R.weights(R.MVDR, dev_cov, A=host(A), ref=1, loading=loading)
    w = host(beam.weights)
    for b in range(B):
        for f in range(F):
            if (b, f) in bad:
                assert same_bits(beam.spec[b, f], x[b, 1, f])
                assert np.array_equal(w[b, f], np.eye(D)[1])
            else:
                k = R.cond(dev_cov[b, f], loading)
                assert k <= R.COND_CAP
                assert np.abs(w[b, f] - want[b, f]).max() <= R.weights_bound(D, k, np.abs(want[b, f]).max(), c=16)
    y = R.apply(Xp, w)
    keep = np.array([[(b, f) not in bad for f in range(F)] for b in range(B)])
    err = np.abs(host(beam.spec).astype(np.complex128) - y)[keep]
    bound = (2 * R.apply_bound(Xp, w) + (6e-8 * np.abs(y) if cdtype == np.complex64 else 0.0))[keep]
    assert (err <= bound).all()


def test_non_finite_coordinate():
    shape = R.PARITY[1]
    B, D, F, T, _ = shape
    c = R.parity_case(shape)
    mics = np.broadcast_to(c.mics, (B, D, 3)).copy()
    mics[1, 1, 2] = np.inf
    A, status = BF.steering_vectors(dev(mics), dev(c.source), F)
    want, want_status = R.steering(mics, c.source, F)
    assert np.array_equal(host(status), want_status) and list(want_status) == [0, 4]
    assert np.isnan(host(A)[1].real).all() and np.isnan(host(A)[1].imag).all()
    assert np.abs(host(A)[0] - want[0]).max() <= R.steering_bound(R.theta_max(mics[:1], c.source[:1], F))
    src = c.source.copy()
    src[0, 0] = np.nan
    assert list(host(BF.steering_vectors(dev(c.mics), dev(src), F)[1])) == [4, 0]


# ------------------------------------------------------------------------------------------------ repeatability, isolation
@pytest.mark.parametrize("shape", [R.PARITY[1], R.PARITY[4], R.PARITY[5]], ids=[IDS[1], IDS[4], IDS[5]])
def test_launches_repeat_and_bins_do_not_see_each_other(shape):
    B, D, F, T, loading = shape
    c = R.parity_case(shape)
    x, m, mics, src = dev(c.X), dev(c.masks["runs"]), dev(c.mics), dev(c.source)

    def run(x, m, src):
        return BF.mvdr(x, mics, src, noise_mask=m, loading=loading)
    first, second = run(x, m, src), run(x, m, src)
    for a, b_ in zip(first, second):
        assert same_bits(a, b_)
    for b in range(B):                                  # an item alone
        alone = run(x[b:b + 1], m[b:b + 1], src[b:b + 1])
        assert all(same_bits(a[0], w[b]) for a, w in zip(alone, first))
    f = F // 2                                          # a bin alone: its steering vector comes from the full set
    A, _ = BF.steering_vectors(mics, src, F)
    xa, ma = x[:1, :, f:f + 1], m[:1, f:f + 1]
    cov = BF.spatial_covariance(xa, ma)
    w = BF.weights("mvdr", cov.cov, A[:1, :, f:f + 1], loading=loading)
    assert same_bits(w.w[0, 0], first.weights[0, f]) and same_bits(BF.apply(xa, w.w)[0, 0], first.spec[0, f])
    assert same_bits(cov.cov[0, 0], BF.spatial_covariance(x, m).cov[0, f])


def test_more_bins_than_the_grid_holds():
    """Every launch caps its grid at 65536 workgroups and strides: bins past the first pass have the bits they have alone.
    300 000 one-frame bins pass the cap of the wave-a-bin launches (four bins a workgroup) and of delay-and-sum; 70 000 bins
    of 1025 frames pass that of the workgroup-a-bin covariance, and their 7e7 outputs that of apply."""
    g = torch.Generator(device="cuda").manual_seed(5)

    def gauss(*shape, real=torch.float64):
        return torch.complex(torch.randn(shape, dtype=real, device="cuda", generator=g), torch.randn(shape, dtype=real, device="cuda", generator=g))
    B, D, F = 5, 2, 60000
    x, m = gauss(B, D, F, 3), torch.rand((B, F, 3), dtype=torch.float64, device="cuda", generator=g)
    A = gauss(B, D, F)
    A = A / A.abs()
    cov = BF.spatial_covariance(x, m)
    das, w = BF.weights("das", steering=A), BF.weights("mvdr", cov.cov, A, loading=1e-3)
    sou = BF.weights("souden", cov.cov, speech_cov=cov.cov, loading=1e-3)
    assert not host(cov.status).any() and not host(w.status).any() and not host(sou.status).any()
    tail = slice(F - 7, F)                                # the last bins of the last item, alone
    xa, ma, Aa = x[B - 1:, :, tail], m[B - 1:, tail], A[B - 1:, :, tail]
    cova = BF.spatial_covariance(xa, ma)
    assert same_bits(cova.cov[0], cov.cov[B - 1, tail])
    assert same_bits(BF.weights("das", steering=Aa).w[0], das.w[B - 1, tail])
    assert same_bits(BF.weights("mvdr", cova.cov, Aa, loading=1e-3).w[0], w.w[B - 1, tail])
    assert same_bits(BF.weights("souden", cova.cov, speech_cov=cova.cov, loading=1e-3).w[0], sou.w[B - 1, tail])
    del x, m, A, cov, das, w, sou
    F, T = 70000, 1025
    x = gauss(1, 1, F, T, real=torch.float32)
    cov = BF.spatial_covariance(x)
    assert not host(cov.status).any()
    xa = x[:, :, tail]
    assert same_bits(BF.spatial_covariance(xa).cov[0], cov.cov[0, tail])
    wt = gauss(1, F, 1)
    assert same_bits(BF.apply(xa, wt[:, tail])[0], BF.apply(x, wt)[0, tail])


def test_views_and_ranks():
    shape = R.PARITY[1]
    B, D, F, T, loading = shape
    c = R.parity_case(shape)
    x, m, mics, src = dev(c.X), dev(c.masks["uniform"]), dev(c.mics), dev(c.source)
    four = BF.mvdr(x, mics, src, noise_mask=m, loading=loading)
    view = dev(c.X.transpose(0, 1, 3, 2)).transpose(2, 3)                               # a strided (B, D, F, T) view
    mview = dev(c.masks["uniform"].transpose(0, 2, 1)).transpose(1, 2)
    assert not view.is_contiguous() and not mview.is_contiguous()
    for a, b_ in zip(BF.mvdr(view, mics, src, noise_mask=mview, loading=loading), four):
        assert same_bits(a, b_)
    three = BF.mvdr(x[1], mics, src[1], noise_mask=m[1], loading=loading)              # ranks mirror the input
    assert three.spec.shape == (F, T) and three.weights.shape == (F, D) and three.status.shape == (F,)
    assert all(same_bits(a, b_[1]) for a, b_ in zip(three, four))
    cov4, cov3 = BF.spatial_covariance(x, m), BF.spatial_covariance(x[1], m[1])
    assert cov3.cov.shape == (F, D, D) and cov3.status.shape == (F,) and same_bits(cov3.cov, cov4.cov[1])
    A4, s4 = BF.steering_vectors(mics, src, F)
    A3, s3 = BF.steering_vectors(mics, src[1], F)
    assert A3.shape == (D, F) and s3.shape == () and same_bits(A3, A4[1])
    w3 = BF.weights("mvdr", cov3.cov, A3, loading=loading)
    assert w3.w.shape == (F, D) and w3.status.shape == (F,) and same_bits(w3.w, three.weights)
    assert BF.apply(x[1], w3.w).shape == (F, T) and same_bits(BF.apply(x[1], w3.w), three.spec)
    das = BF.delay_and_sum(x[1], mics, src[1])
    assert das.spec.shape == (F, T) and das.weights.shape == (F, D) and das.status.shape == (F,)


# -------------------------------------------------------------------------------------------------------------- composition
def test_compositions_are_their_chains():
    shape = R.PARITY[2]
    B, D, F, T, loading = shape
    c = R.parity_case(shape)
    x, mics, src = dev(c.X), dev(c.mics), dev(c.source)
    mn, ms = dev(c.masks["uniform"]), dev(c.masks["runs"])
    A, _ = BF.steering_vectors(mics, src, F)
    das = BF.delay_and_sum(x, mics, src)
    w = BF.weights("das", steering=A)
    assert same_bits(das.weights, w.w) and same_bits(das.spec, BF.apply(x, w.w)) and not host(das.status).any()
    for kwargs, chain in (
            ({}, lambda: BF.weights("mvdr", BF.spatial_covariance(x).cov, A, loading=loading)),
            ({"noise_mask": mn}, lambda: BF.weights("mvdr", BF.spatial_covariance(x, mn).cov, A, loading=loading))):
        got, w = BF.mvdr(x, mics, src, loading=loading, **kwargs), chain()
        assert same_bits(got.weights, w.w) and same_bits(got.spec, BF.apply(x, w.w)) and torch.equal(got.status, w.status)
    got = BF.mvdr(x, noise_mask=mn, speech_mask=ms, loading=loading, ref=1)
    w = BF.weights("souden", BF.spatial_covariance(x, mn).cov, speech_cov=BF.spatial_covariance(x, ms).cov, ref=1, loading=loading)
    assert same_bits(got.weights, w.w) and same_bits(got.spec, BF.apply(x, w.w)) and torch.equal(got.status, w.status)


@pytest.mark.parametrize("real", [torch.float64, torch.float32])
def test_beamform_waves_is_stft_beamformer_istft(real):
    g = np.random.default_rng(2400)
    B, D, S = 2, 3, 2400
    waves = dev(g.standard_normal((B, D, S))).to(real)
    mics = dev(srp_ref.CENTRE + 0.05 * g.uniform(-1, 1, (D, 3)))
    src = dev(srp_ref.ring(8)[[1, 5]])
    spec = N.stft_complex(waves.reshape(B * D, S).contiguous())
    spec = spec.view(B, D, spec.shape[1], spec.shape[2])
    got = BF.beamform_waves(waves, mics, src)
    assert got.dtype == real and got.shape == (B, S)
    assert same_bits(got, FE.istft(BF.mvdr(spec, mics, src).spec, length=S))
    assert same_bits(BF.beamform_waves(waves, mics, src, method="das"), FE.istft(BF.delay_and_sum(spec, mics, src).spec, length=S))
    mn = dev(g.uniform(0, 1, spec[:, 0].shape))
    ms = 1.0 - mn
    assert same_bits(BF.beamform_waves(waves, noise_mask=mn, speech_mask=ms),
                     FE.istft(BF.mvdr(spec, noise_mask=mn, speech_mask=ms).spec, length=S))


def test_locate_and_beamform_steers_at_the_arg_max():
    shape = srp_ref.PARITY[2]
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c, ref = srp_ref.parity_case(shape), srp_ref.reference(shape)
    assert ref.gap.min() > 1e-6
    x, mics, cand = dev(c.X), dev(c.mics), dev(c.cand)
    beam, srp = BF.locate_and_beamform(x, mics, cand, band=(f_lo, f_hi))
    assert np.array_equal(host(srp.best), ref.best)
    want = BF.mvdr(x, mics, cand[torch.tensor(ref.best.astype(np.int64)).cuda()])
    for a, b_ in zip(beam, want):
        assert same_bits(a, b_)
    silent = torch.zeros_like(x)                        # best = -1: candidate 0, and the status tells
    beam, srp = BF.locate_and_beamform(silent, mics, cand, band=(f_lo, f_hi))
    assert (host(srp.best) == -1).all() and (host(beam.status) == 2).all() and same_bits(beam.spec, silent[:, 0])


# ---------------------------------------------------------------------------------------------------- an image-source room
def test_beamformers_in_an_image_source_room():
    """Two sources in DATASET_CONFIG's room, each two seconds of noise under a syllable-rate envelope, four microphones 5 cm
    around its receiver, lined up with the clean signal.  What the beamformers gain on image-source rooms is printed, not asserted: nobody has
    measured it."""
    cfg = FE.DATASET_CONFIG
    fs, n, D = cfg["fs"], 32000, 4
    g = np.random.default_rng(15)
    t = np.arange(n) / fs
    envelope = (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + 0.3)) * (0.6 + 0.4 * np.sin(2 * np.pi * 1.3 * t))
    clean = dev((g.standard_normal((2, n)) * envelope).astype(np.float32))
    mics = dev(np.array(cfg["receiver_position"]) + 0.05 * g.uniform(-1, 1, (D, 3)))
    src = dev(np.array([[1.0, 3.5, 1.0], [3.2, 0.8, 1.9]]))
    h = FE.array_impulse_responses(src, mics, cfg["room_dimensions"], reverberation_time=cfg["reverberation_time"],
                                   nsample=cfg["n_sample"])
    spec = FE.array_spectrograms(clean, h)
    assert spec.shape[:2] == (2, D) and spec.dtype == torch.complex128
    das, mpdr = BF.delay_and_sum(spec, mics, src), BF.mvdr(spec, mics, src)
    # the 'same' convolution leaves the recording (Nh - 1) // 2 samples ahead of the clean signal, the direct path to the
    # reference microphone puts it |q - m_0| / c behind: the pair is lined up by the difference, item by item
    lead = (h.shape[2] - 1) // 2
    path = torch.round((src - mics[0]).norm(dim=1) / FE.SOUND_SPEED * fs).to(torch.int64).tolist()
    for name, s in (("microphone 0", spec[:, 0]), ("delay-and-sum", das.spec), ("mpdr", mpdr.spec)):
        assert s.shape == spec[:, 0].shape and s.dtype == torch.complex128
        wave = FE.istft(s, length=n)
        assert wave.shape == (2, n) and bool(torch.isfinite(wave).all())
        for b in range(2):
            shift = lead - path[b]
            c, v = clean[b:b + 1, shift:].double().contiguous(), wave[b:b + 1, :n - shift].contiguous()
            print("%s, source %d: stoi %.4f si_sdr %.2f dB" % (name, b, float(SM.stoi(c, v).value), float(SM.si_sdr(c, v))))
    assert not host(das.status).any() and mpdr.status.shape == spec[:, 0].shape[:2]
