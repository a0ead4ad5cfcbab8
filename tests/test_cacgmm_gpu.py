"""cACGMM on the device (csrc/cacgmm.hip, acoustic_locating_vq_vae.separation.cacgmm) against the float64 restatement of
tests/helpers/cacgmm_ref.py, which tests/test_cacgmm_cpu.py pins.  u = 1.1e-16.

masks, prior:   max |dev - ref| <= tol, tol = max(32 e_ref, 2 (T + F + 8 D) u), e_ref the largest difference of the masks of the
                restatement run forward and with the frames and bins added in the opposite order: the tolerance is measured on
                the reference, never on the device.  tol <= 1e-9 is asserted (a condition on the case), so a float32
                accumulation, at 1e-7 or above, cannot hide.  complex64: the restatement of the promoted input.
quadratic:      the same tol, relative to the case's largest q (masks and priors lie in [0, 1]; q does not).
cov:            |cov_dev - cov_ref| <= c tol cond per class matrix, cond = lambda_max / lambda_min of the reference (<= 1e6,
                asserted on the cases), c = 0.32: the restatement's own forward / reverse pair gives
                |cov_fwd - cov_rev| / (tol cond) between 2.1e-6 and 9.7e-3 over the parity cases and both dtypes; the CPU test
                asserts <= 1e-2 and c is 32 times that.
Agreement, SI-SDR: the device's value equals the restatement's within 1e-6 (1e-6 dB)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import cacgmm_ref as R  # noqa: E402
from parity_checks import check_gmm as check  # noqa: E402
from acoustic_locating_vq_vae import beamforming as BF  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import separation as SEP  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as SM  # noqa: E402

U = R.U
CDTYPES = [np.complex128, np.complex64]
CIDS = ["complex128", "complex64"]


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


def same_gmm(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def device_run(shape, cdtype):
    """(masks, prior, cov, quadratic, status) of a parity or separation shape on the device, downloaded; computed once."""
    c = R.parity_case(shape)
    out = SEP.cacgmm(dev(c.X.astype(cdtype)), dev(c.init), shape[5])
    B, D, K, F, T = shape[:5]
    assert out.masks.shape == (B, K, F, T) and out.masks.dtype == torch.float64
    assert out.prior.shape == (B, K, T) and out.prior.dtype == torch.float64
    assert out.cov.shape == (B, F, K, D, D) and out.cov.dtype == torch.complex128
    assert out.quadratic.shape == (B, K, F, T) and out.quadratic.dtype == torch.float64
    assert out.status.shape == (B, F) and out.status.dtype == torch.int32
    return tuple(host(t) for t in out)


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
@pytest.mark.parametrize("shape", R.PARITY, ids=R.IDS)
def test_parity(shape, cdtype):
    single = cdtype == np.complex64
    got = device_run(shape, cdtype)
    ref = R.reference(shape, single=single)
    assert not got[4].any() and not ref.status.any()
    check("%s %s" % (shape[:5], np.dtype(cdtype).name), got, ref, R.tolerance(shape, single))
    assert (np.abs(got[0].sum(axis=1) - 1.0) <= 8 * U).all() and (got[0] >= 0).all() and (got[3] > 0).all()


@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
@pytest.mark.parametrize("shape", R.PARITY, ids=R.IDS)
def test_cov_parity(shape, cdtype):
    """|cov_dev - cov_ref| <= c tol cond per class matrix with c = R.C_COV = 0.32: 32 times the 1e-2 that bounds the
    restatement's own forward / reverse ratio |cov_fwd - cov_rev| / (tol cond), measured between 2.1e-6 and 9.7e-3 over the
    parity cases (tests/test_cacgmm_cpu.py asserts the bound)."""
    single = cdtype == np.complex64
    cov = device_run(shape, cdtype)[2]
    ref = R.reference(shape, single=single)
    assert ref.cond.max() <= R.COND_CAP
    D = shape[1]
    assert np.array_equal(cov, np.conj(np.swapaxes(cov, -1, -2)))                              # exactly Hermitian
    assert (np.abs(np.trace(cov, axis1=-2, axis2=-1) - D) <= 16 * D * D * U).all()
    err = np.abs(cov - ref.cov).max(axis=(-2, -1))
    bound = R.C_COV * R.tolerance(shape, single) * ref.cond
    print("%s %s: largest |cov - cov_ref| / (c tol cond) %.3g, cond up to %.3g" % (shape[:5], np.dtype(cdtype).name,
                                                                                  (err / bound).max(), ref.cond.max()))
    assert (err <= bound).all()


def test_ranks_views_and_an_init_without_bins():
    shape = R.PARITY[3]
    B, D, K, F, T = shape[:5]
    c = R.parity_case(shape)
    x, init = dev(c.X), dev(c.init)
    first = SEP.cacgmm(x, init, 5)
    three = SEP.cacgmm(x[0], init[0], 5)                                                    # ranks mirror the input
    assert three.masks.shape == (K, F, T) and three.prior.shape == (K, T) and three.cov.shape == (F, K, D, D)
    assert three.quadratic.shape == (K, F, T) and three.status.shape == (F,)
    assert all(same_bits(a, b[0]) for a, b in zip(three, first))
    assert same_gmm(SEP.cacgmm(x, init[:, :, :1], 5), first)                                # (B, K, 1, T): expanded over the bins
    assert same_gmm(SEP.cacgmm(x[0], init[0, :, :1], 5), three)
    view = dev(c.X.transpose(0, 1, 3, 2)).transpose(2, 3)                                   # a strided (B, D, F, T) view
    assert not view.is_contiguous() and same_gmm(SEP.cacgmm(view, init, 5), first)
    assert same_bits(init, dev(c.init))                                                     # the init is not written to
    g = torch.Generator(device="cuda").manual_seed(4)
    tm = SEP.time_masks(2, 3, 5, 70, generator=g)
    assert tm.is_cuda and tm.shape == (2, 3, 5, 70) and tm.dtype == torch.float64
    assert bool((tm == tm[:, :, :1]).all()) and float((tm.sum(dim=1) - 1).abs().max()) <= 4 * U and float(tm.min()) > 0


# ------------------------------------------------------------------------------------------------------------------ status
@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
def test_status_bins(cdtype):
    """One item with a NaN bin, a negative init, a zero quadratic0 and a bin of zeros beside good bins.  The first three get
    status 1, masks = 1 / K, cov = I, quadratic = 1; the bin of zeros is all silent frames and no error: its masks are the
    priors.  The good bins have the bits of a launch without the three bad bins' data (F0 is the same), and agree with the
    restatement."""
    shape = R.PARITY[2]
    B, D, K, F, T = shape[:5]
    c = R.parity_case(shape)
    X, init, q0 = c.X.astype(cdtype), c.init.copy(), np.ones((B, K, F, T))
    X[0, 1, 1, 7] = complex(np.nan, 0.0)
    init[0, 1, 2, 9] = -0.25
    q0[0, 0, 3, 4] = 0.0
    X[0, :, 5] = 0
    X[0, :, 6, 10] = 0                                    # one silent frame in a good bin
    x, g0, qd = dev(X), dev(init), dev(q0)
    got = SEP.cacgmm(x, g0, 5, quadratic0=qd)
    want = np.zeros((B, F), np.int32)
    want[0, 1] = want[0, 2] = want[0, 3] = 1
    assert np.array_equal(host(got.status), want)
    eye = torch.eye(D, dtype=torch.complex128, device="cuda").expand(K, D, D)
    for f in (1, 2, 3):
        assert bool((got.masks[0, :, f] == 1.0 / K).all()) and bool((got.quadratic[0, :, f] == 1).all())
        assert bool((got.cov[0, f] == eye).all())
    assert same_bits(got.masks[0, :, 5], got.prior[0]) and bool((got.quadratic[0, :, 5] == 1).all())
    assert bool((got.cov[0, 5] == eye).all())                # a class without weight keeps B_k = I
    assert same_bits(got.masks[0, :, 6, 10], got.prior[0, :, 10]) and bool((got.quadratic[0, :, 6, 10] == 1).all())
    keep = [f for f in range(F) if f not in (1, 2, 3)]                                     # the item without the bad bins' data
    alone = SEP.cacgmm(x[:1, :, keep].contiguous(), g0[:1, :, keep].contiguous(), 5, quadratic0=qd[:1, :, keep].contiguous())
    assert not host(alone.status).any()
    assert same_bits(alone.masks[0], got.masks[0][:, keep]) and same_bits(alone.quadratic[0], got.quadratic[0][:, keep])
    assert same_bits(alone.prior[0], got.prior[0]) and same_bits(alone.cov[0], got.cov[0][keep])
    Xp = X.astype(np.complex128)
    ref, rev = R.cacgmm(Xp, init, 5, quadratic0=q0), R.cacgmm(Xp, init, 5, quadratic0=q0, reverse=True)
    assert np.array_equal(ref.status, want)
    tol = max(32 * np.abs(ref.masks - rev.masks).max(), 2 * (T + F + 8 * D) * U)
    check("beside the bad bins, %s" % np.dtype(cdtype).name, tuple(host(t) for t in got), ref, tol)


# --------------------------------------------------------------------------------------------------------- reproducibility
def test_runs_repeat_and_items_do_not_see_each_other():
    shape = R.PARITY[2]
    B, D, K, F, T = shape[:5]
    c = R.parity_case(shape)
    other = R.case(1, D, K, F, T, 77)
    x = dev(np.concatenate([other.X, c.X[1:2], c.X[0:1]]))                                  # a batch of three
    init = dev(np.concatenate([other.init, c.init[1:2], c.init[0:1]]))
    first, second = SEP.cacgmm(x, init, 5), SEP.cacgmm(x, init, 5)
    assert same_gmm(first, second)
    alone = SEP.cacgmm(x[1:2].contiguous(), init[1:2].contiguous(), 5)
    assert all(same_bits(a[0], b[1]) for a, b in zip(alone, first))


@pytest.mark.parametrize("shape", [R.PARITY[2], R.PARITY[4]], ids=[R.IDS[2], R.IDS[4]])
def test_continuation_has_the_same_bits(shape):
    c = R.parity_case(shape)
    x, init = dev(c.X), dev(c.init)
    whole = SEP.cacgmm(x, init, 3 + 4)
    first = SEP.cacgmm(x, init, 3)
    again = SEP.cacgmm(x, first.masks, 4, quadratic0=first.quadratic)
    assert same_gmm(whole, again)


def test_graph_capture_replays_the_eager_bits():
    shape = R.PARITY[2]
    c = R.parity_case(shape)
    x, init = dev(c.X), dev(c.init)
    eager = SEP.cacgmm(x, init, 5)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = SEP.cacgmm(x, init, 5)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same_gmm(out, eager)


def test_more_bins_than_the_grid_holds():
    """Every launch over bins caps its grid at 65536 workgroups and strides: 300 000 three-frame bins with two classes pass the
    cap of the check (a wave a bin, four a workgroup), of the M-step (a wave a (bin, k)) and of the E-step (a workgroup a bin),
    and the last item has the bits it has alone, where no launch strides."""
    g = torch.Generator(device="cuda").manual_seed(5)
    B, D, K, F, T = 5, 2, 2, 60000, 3
    x = torch.complex(torch.randn((B, D, F, T), dtype=torch.float64, device="cuda", generator=g),
                      torch.randn((B, D, F, T), dtype=torch.float64, device="cuda", generator=g))
    x[B - 1, 0, F - 2, 1] = float("nan")                  # a status among the strided bins
    init = SEP.time_masks(B, K, F, T, generator=g)
    whole = SEP.cacgmm(x, init, 2)
    alone = SEP.cacgmm(x[B - 1:].contiguous(), init[B - 1:].contiguous(), 2)
    assert all(same_bits(a[0], w[B - 1]) for a, w in zip(alone, whole))
    assert int(whole.status[B - 1, F - 2]) == 1 and int((whole.status != 0).sum()) == 1
    assert float((whole.masks.sum(dim=1) - 1).abs().max()) <= 8 * U


# -------------------------------------------------------------------------------------------------------------- separation
@pytest.mark.parametrize("shape", R.SEPARATION, ids=R.SEP_IDS)
def test_separation_matches_the_restatement(shape):
    c = R.parity_case(shape)
    got = device_run(shape, np.complex128)
    ref = R.reference(shape)
    K = shape[2]
    assert not got[4].any()
    for b in range(shape[0]):
        want, perm = R.agreement(ref.masks[b], c.oracle[b])
        mine, mine_perm = R.agreement(got[0][b], c.oracle[b])
        own, _ = R.agreement(c.oracle[b], c.oracle[b])
        print("%s item %d: agreement %.6f, the restatement's %.6f, the oracle's own %.4f" % (shape[:5], b, mine, want, own))
        assert mine_perm == perm and abs(mine - want) <= 1e-6
        assert mine >= 0.9 * own - 1e-6 and mine >= 1.0 / K + 0.25 - 1e-6


# -------------------------------------------------------------------------------------------------------------- downstream
def test_masks_drive_the_mask_beamformers():
    """The device's masks and the restatement's, both given to BF.mvdr and BF.gev on the device: the SI-SDR of every source
    against its image at the reference microphone agrees within 1e-6 dB.  The improvement over the microphone is printed."""
    shape = R.SEPARATION[0]
    K = shape[2]
    c = R.parity_case(shape)
    x = dev(c.X)
    m_dev = SEP.cacgmm(x, dev(c.init), shape[5]).masks
    m_ref = dev(R.reference(shape).masks)
    _, perm = R.agreement(R.reference(shape).masks[0], c.oracle[0])
    for name, beam in (("mvdr", lambda m: BF.mvdr(x, noise_mask=1 - m, speech_mask=m)), ("gev", lambda m: BF.gev(x, 1 - m, m))):
        for k in range(K):
            image, mix = c.images[0, k], c.X[0, 0]
            out = [beam(m[:, perm[k]].contiguous()) for m in (m_dev, m_ref)]
            assert not host(out[0].status).any() and not host(out[1].status).any()
            got, want = (R.si_sdr(image, host(o.spec)[0]) for o in out)
            before = R.si_sdr(image, mix)
            print("%s source %d: SI-SDR %.6f dB (the restatement's masks: %.6f dB), the microphone's %.3f dB, improvement %.3f dB"
                  % (name, k, got, want, before, got - before))
            assert abs(got - want) <= 1e-6


def test_two_sources_in_an_image_source_room():
    """The chain on real geometry, printed only (nobody has measured what cACGMM gains there): two sources in one generated
    room, four microphones, array_spectrograms -> cacgmm with K = 3 (two talkers and a class for the rest) -> gev -> si_sdr of
    the waveforms."""
    cfg = FE.DATASET_CONFIG
    n, D, K, iterations = 16000, 4, 3, 20
    g = np.random.default_rng(31)
    activity = np.repeat(g.gamma(0.3, size=(2, n // FE.HOP)) + 1e-3, FE.HOP, axis=1)
    clean = dev((g.standard_normal((2, n)) * activity).astype(np.float32))
    centre = np.array(cfg["receiver_position"])
    mics = dev(centre + np.array([[-0.05, 0.0, 0.0], [0.05, 0.0, 0.0], [0.0, 0.05, 0.0], [0.0, -0.05, 0.0]]))
    src = dev(np.array([[1.0, 3.5, 1.0], [3.2, 0.8, 1.9]]))
    h = FE.array_impulse_responses(src, mics, cfg["room_dimensions"], reverberation_time=0.2, nsample=3200)
    images = FE.array_spectrograms(clean, h)                                                # (2, D, F, T): source b at the microphones
    spec = images.sum(dim=0, keepdim=True)                                                  # (1, D, F, T): what the array records
    F, T = spec.shape[2:]
    init = SEP.time_masks(1, K, F, T, generator=torch.Generator(device="cuda").manual_seed(31))
    out = SEP.cacgmm(spec, init, iterations)
    assert out.masks.shape == (1, K, F, T) and bool(torch.isfinite(out.masks).all())
    print("image-source room: status counts %s" % np.bincount(host(out.status).ravel(), minlength=3))
    want = FE.istft(images[:, 0].contiguous(), length=n)                                    # source b as microphone 0 hears it
    mix = FE.istft(spec[:, 0].contiguous(), length=n)
    table = np.zeros((2, K))
    for k in range(K):
        m = out.masks[:, k].contiguous()
        wave = FE.istft(BF.gev(spec, 1 - m, m).spec.contiguous(), length=n)
        assert wave.shape == (1, n)
        for s in range(2):
            table[s, k] = float(SM.si_sdr(want[s], wave[0]))
    for s in range(2):
        before = float(SM.si_sdr(want[s], mix[0]))
        print("image-source room: source %d SI-SDR per class %s dB, the microphone's %.2f dB, best improvement %.2f dB"
              % (s, np.round(table[s], 2), before, np.nanmax(table[s]) - before))
