"""ILRMA on the device (csrc/ilrma.hip, acoustic_locating_vq_vae.separation) against the float64 restatement of
tests/helpers/ilrma_ref.py, which tests/test_ilrma_cpu.py pins.  u = 1.1e-16.

W, basis, activations, per case and array:
                    max |dev - ref| <= tol max |ref|, tol = max(32 e_ref, 2 (T + F + 8 D + L) u), e_ref the largest relative
                    max-norm difference of the three arrays between the restatement run forward and with the frames and bins
                    added in the opposite order in every sum: the tolerance is measured on the reference, never on the device.
                    32: the reason iva_ref.w_tolerance gives.  tol <= 1e-10 is asserted (a condition on the case), so a float32
                    accumulation, at 1e-7 or above, cannot hide.  complex64: the restatement of the promoted input.
Y, per output:      iva_ref.y_bound with the device's own W given to the restatement's projection, as tests/test_iva_gpu.py has it.
SI-SDR:             a relative error delta in Y moves an SI-SDR of S dB by about 8.7 delta 10^(S / 20) dB, delta = 32 e_ref of the
                    30-iteration run."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import iva_ref as IR  # noqa: E402
import ilrma_ref as R  # noqa: E402
from parity_checks import check_three  # noqa: E402
from acoustic_locating_vq_vae import beamforming as BF  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import separation as SEP  # noqa: E402

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


def same_all(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def starts(shape):
    return tuple(dev(a) for a in R.parity_start(shape))


@functools.lru_cache(maxsize=None)
def device_run(shape, cdtype):
    """(W, basis, activations, Y, status) of a parity or separation shape on the device, downloaded; computed once."""
    B, D, F, T, L = shape[:5]
    out = SEP.ilrma(dev(R.parity_case(shape).X.astype(cdtype)), *starts(shape), iterations=shape[5])
    assert out.spec.shape == (B, D, F, T) and out.spec.dtype == (torch.complex64 if cdtype == np.complex64 else torch.complex128)
    assert out.w.shape == (B, F, D, D) and out.w.dtype == torch.complex128
    assert out.basis.shape == (B, D, F, L) and out.activations.shape == (B, D, L, T)
    assert out.basis.dtype == out.activations.dtype == torch.float64
    assert out.status.shape == (B, F) and out.status.dtype == torch.int32
    return host(out.w), host(out.basis), host(out.activations), host(out.spec), host(out.status)


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
@pytest.mark.parametrize("shape", R.PARITY, ids=R.IDS)
def test_parity_of_the_state(shape, cdtype):
    single = cdtype == np.complex64
    got = device_run(shape, cdtype)
    ref = R.reference(shape, single=single)
    assert not got[4].any() and not ref.status.any()
    check_three("%s %s" % (shape[:5], np.dtype(cdtype).name), got[:3], ref[:3], R.tolerance(shape, single))


@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
@pytest.mark.parametrize("shape", R.PARITY, ids=R.IDS)
def test_y_parity(shape, cdtype):
    single = cdtype == np.complex64
    W, _, _, Y, status = device_run(shape, cdtype)
    Xp = R.promoted(R.parity_case(shape).X, single)
    want, _, st = IR.project(Xp, W, status)               # the device's own W: only the projection differs
    assert not st.any()
    bound, cond = IR.y_bound(Xp, W, 0)
    assert cond <= R.COND_CAP
    if single:
        bound = bound + 6e-8 * np.abs(want)
    err = np.abs(Y.astype(np.complex128) - want)
    print("%s %s: largest |Y - Y_ref| / bound %.3g, cond_2(W) up to %.3g" % (shape[:5], np.dtype(cdtype).name, (err / bound).max(), cond))
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------------------ continuation
@pytest.mark.parametrize("shape", [R.PARITY[2], R.PARITY[4]], ids=[R.IDS[2], R.IDS[4]])
def test_continuation_has_the_same_bits(shape):
    x = dev(R.parity_case(shape).X)
    b0, a0 = starts(shape)
    whole = SEP.ilrma(x, b0, a0, 2 + 3)
    part = SEP.ilrma(x, b0, a0, 2)
    again = SEP.ilrma(x, part.basis, part.activations, 3, w0=part.w)
    assert same_all(whole, again)
    assert not same_bits(whole.w, part.w)                 # ... and the three iterations did something


# --------------------------------------------------------------------------------------------------------- reproducibility
def test_runs_repeat_and_items_do_not_see_each_other():
    shape = R.PARITY[2]
    B, D, F, T, L = shape[:5]
    X = R.parity_case(shape).X
    b0, a0 = R.parity_start(shape)
    ob, oa = R.start(1, D, F, T, L, 77)
    x = dev(np.concatenate([R.case(1, D, F, T, 77).X, X[1:2], X[0:1]]))                          # a batch of three
    b3, a3 = dev(np.concatenate([ob, b0[1:2], b0[0:1]])), dev(np.concatenate([oa, a0[1:2], a0[0:1]]))
    first, second = SEP.ilrma(x, b3, a3, 5), SEP.ilrma(x, b3, a3, 5)
    assert same_all(first, second)
    alone = SEP.ilrma(x[1:2].contiguous(), b3[1:2].contiguous(), a3[1:2].contiguous(), 5)
    assert all(same_bits(a[0], b[1]) for a, b in zip(alone, first))


def test_graph_capture_replays_the_eager_bits():
    shape = R.PARITY[2]
    x = dev(R.parity_case(shape).X)
    b0, a0 = starts(shape)
    eager = SEP.ilrma(x, b0, a0, 5)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = SEP.ilrma(x, b0, a0, 5)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same_all(out, eager)


def test_another_reference_microphone_ranks_views_and_no_iteration():
    shape = R.PARITY[3]
    B, D, F, T, L = shape[:5]
    X = R.parity_case(shape).X
    x = dev(X)
    b0, a0 = starts(shape)
    first = SEP.ilrma(x, b0, a0, 5)
    last = SEP.ilrma(x, b0, a0, 5, ref=D - 1)
    assert all(same_bits(a, b) for a, b in zip(first[1:], last[1:]))                           # ref enters the projection alone
    W = host(last.w)
    want, _, _ = IR.project(X, W, host(last.status), D - 1)
    bound, _ = IR.y_bound(X, W, D - 1)
    assert (np.abs(host(last.spec) - want) <= bound).all()
    three = SEP.ilrma(x[0], b0[0], a0[0], 5)                                                  # ranks mirror the input
    assert three.spec.shape == (D, F, T) and three.w.shape == (F, D, D) and three.status.shape == (F,)
    assert three.basis.shape == (D, F, L) and three.activations.shape == (D, L, T)
    assert all(same_bits(a, b[0]) for a, b in zip(three, first))
    again = SEP.ilrma(x[0], three.basis, three.activations, 2, w0=three.w)                    # ... and so does w0's
    assert all(same_bits(a, b[0]) for a, b in zip(again, SEP.ilrma(x, first.basis, first.activations, 2, w0=first.w)))
    view = dev(X.transpose(0, 1, 3, 2)).transpose(2, 3)                                        # strided (B, D, F, T) views
    bview, aview = dev(R.parity_start(shape)[0].transpose(0, 1, 3, 2)).transpose(2, 3), dev(R.parity_start(shape)[1].transpose(0, 1, 3, 2)).transpose(2, 3)
    assert not view.is_contiguous() and not bview.is_contiguous() and same_all(SEP.ilrma(view, bview, aview, 5), first)
    zero = SEP.ilrma(x, b0, a0, 0)                        # no iteration: the start, and W = I, whose "source" ref is microphone ref
    assert bool((zero.w == torch.eye(D, dtype=torch.complex128, device="cuda")).all())
    assert same_bits(zero.basis, b0) and same_bits(zero.activations, a0) and not host(zero.status).any()
    assert torch.equal(zero.spec[:, 0], x[:, 0]) and bool((zero.spec[:, 1:] == 0).all())
    started = SEP.ilrma(x, b0, a0, 0, w0=first.w)         # ... or the w0 it was given, and the projection of it
    assert same_bits(started.w, first.w) and same_bits(started.spec, SEP.ilrma(x, first.basis, first.activations, 0, w0=first.w).spec)
    want, _, _ = IR.project(X, host(first.w), host(first.status), 0)
    assert (np.abs(host(started.spec) - want) <= IR.y_bound(X, host(first.w), 0)[0]).all()


# ------------------------------------------------------------------------------------------------------------------ status
@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
def test_bad_bins_come_back_as_they_came(cdtype):
    """A bin of zeros, a bin with one NaN, a bin whose basis0 row holds a 0 and an item whose activations0 hold a NaN in one
    launch: status 1, Y = X and W = I bit for bit, the basis rows as given; nothing non-finite is left in the activations or in
    any other bin's basis; the other bins have the bits of a launch without the bad bins' data and agree with the restatement."""
    shape = R.PARITY[2]
    B, D, F, T, L = shape[:5]
    X, b0, a0, want = R.bad_inputs(shape)
    X = X.astype(cdtype)
    x, b0d, a0d = dev(X), dev(b0), dev(a0)
    got = SEP.ilrma(x, b0d, a0d, 5)
    assert np.array_equal(host(got.status), want)
    eye = torch.eye(D, dtype=torch.complex128, device="cuda")
    for b, f in zip(*np.nonzero(want)):
        assert same_bits(got.spec[b, :, f], x[b, :, f]) and same_bits(got.w[b, f], eye)
        assert same_bits(got.basis[b, :, f], b0d[b, :, f])
    basis = host(got.basis).transpose(0, 2, 1, 3)                                              # (B, F, D, L)
    assert np.isfinite(host(got.activations)).all() and np.isfinite(basis[want == 0]).all()
    for b in range(B):                                    # the item without the bad bins' data
        keep = [f for f in range(F) if want[b, f] == 0]
        alone = SEP.ilrma(x[b:b + 1, :, keep].contiguous(), b0d[b:b + 1, :, keep].contiguous(), a0d[b:b + 1].contiguous(), 5)
        assert same_bits(alone.w[0], got.w[b, keep]) and same_bits(alone.spec[0], got.spec[b][:, keep])
        assert same_bits(alone.basis[0], got.basis[b][:, keep]) and same_bits(alone.activations[0], got.activations[b])
        assert not host(alone.status).any()
    Xp = X.astype(np.complex128)
    ref, rev = R.ilrma(Xp, b0, a0, 5), R.ilrma(Xp, b0, a0, 5, reverse=True)
    assert np.array_equal(ref.status, want)
    keep = want == 0
    pick = lambda r: (r[0][keep], r[1].transpose(0, 2, 1, 3)[keep], r[2])  # noqa: E731
    tol = R.tolerance_of(R.difference(pick(ref), pick(rev)), D, F, T, L)
    check_three("neighbours of the bad bins, %s" % np.dtype(cdtype).name, pick((host(got.w), host(got.basis), host(got.activations))),
                pick(ref), tol)


def test_identical_microphones_are_refused():
    """A bin whose two microphones are identical is rank-deficient: status 2, W = I, and it comes back as X; its neighbours
    get status 0."""
    shape = R.PARITY[2]
    B, D, F, T = shape[:4]
    X = R.parity_case(shape).X.copy()
    X[1, :, 5] = X[1, 0, 5]
    b0, a0 = starts(shape)
    for cdtype in CDTYPES:
        x = dev(X.astype(cdtype))
        got = SEP.ilrma(x, b0, a0, 5)
        want = np.zeros((B, F), np.int32)
        want[1, 5] = 2
        assert np.array_equal(host(got.status), want)
        assert same_bits(got.spec[1, :, 5], x[1, :, 5])
        assert same_bits(got.w[1, 5], torch.eye(D, dtype=torch.complex128, device="cuda"))
        assert np.array_equal(R.ilrma(X.astype(cdtype).astype(np.complex128), *R.parity_start(shape), 5).status, want)
        for t in (torch.view_as_real(got.spec), got.basis, got.activations):
            assert bool(torch.isfinite(t).all())


def test_more_bins_than_the_grid_holds():
    """Every launch over bins, pairs or rows caps its grid at 65536 workgroups and strides: 300 000 three-frame bins pass the
    cap of each, and the last item has the bits it has alone, where no launch strides, a status-1 bin among the strided ones
    included."""
    g = torch.Generator(device="cuda").manual_seed(5)
    B, D, F, T, L = 5, 2, 60000, 3, 1
    x = torch.complex(torch.randn((B, D, F, T), dtype=torch.float64, device="cuda", generator=g),
                      torch.randn((B, D, F, T), dtype=torch.float64, device="cuda", generator=g))
    x[B - 1, :, F - 2] = 0                                # a status among the strided bins
    b0, a0 = SEP.nmf_init(B, D, F, T, L, generator=g)
    whole = SEP.ilrma(x, b0, a0, 2)
    alone = SEP.ilrma(x[B - 1:].contiguous(), b0[B - 1:].contiguous(), a0[B - 1:].contiguous(), 2)
    assert all(same_bits(a[0], w[B - 1]) for a, w in zip(alone, whole))
    assert int(whole.status[B - 1, F - 2]) == 1 and int((whole.status == 1).sum()) == 1
    assert not same_bits(whole.basis, b0)


# -------------------------------------------------------------------------------------------------------------- separation
@pytest.mark.parametrize("shape", R.SEPARATION, ids=R.SEPARATION_IDS)
def test_separation_matches_the_restatement(shape):
    """The device's per-source SI-SDR under the restatement's best permutation agrees with the restatement's within
    8.7 delta 10^(S / 20) dB, delta = 32 e_ref of the 30-iteration run measured on the restatement: e_ref = 2.6e-12 at
    (2, 2, 16, 200, 2) and 5.4e-10 at (1, 3, 12, 300, 2), so delta = 8.4e-11 and 1.7e-8, and at the S these cases reach, 32.1 to
    33.1 dB and 29.3 to 30.7 dB, the bound is 3.0e-8 to 3.3e-8 dB and 4.3e-6 to 5.1e-6 dB.  The gain itself is at least 20 dB (a
    condition the restatement meets alone: tests/test_ilrma_cpu.py)."""
    c = R.parity_case(shape)
    Y, status = device_run(shape, np.complex128)[3:]
    ref = R.reference(shape)
    assert not status.any()
    delta = 32 * R.e_ref(shape)
    for b in range(shape[0]):
        want, perm = IR.best_permutation_si_sdr(c.images[b], ref.Y[b])
        got = np.array([IR.si_sdr(c.images[b, i], Y[b, perm[i]]) for i in range(shape[1])])
        bound = 8.7 * delta * 10.0 ** (want / 20.0)
        print("%s item %d: SI-SDR %s dB, the restatement's %s dB, |difference| / bound %s"
              % (shape[:5], b, np.round(got, 3), np.round(want, 3), np.abs(got - want) / bound))
        assert (np.abs(got - want) <= bound).all()
    gain = IR.improvement(c.images, c.mix, Y)
    print("%s: SI-SDR improvement %s dB" % (shape[:5], np.round(gain, 2)))
    assert (gain >= 20.0).all()


# --------------------------------------------------------------------------------------------------------------- the chain
def test_started_from_auxiva():
    shape = R.PARITY[2]
    B, D, F, T, L = shape[:5]
    X = R.parity_case(shape).X
    x = dev(X)
    b0, a0 = starts(shape)
    w0 = SEP.auxiva(x, 10).w
    got = SEP.ilrma(x, b0, a0, 5, w0=w0)
    assert not host(got.status).any() and not same_bits(got.w, w0)
    ref = R.ilrma(X, *R.parity_start(shape), 5, w0=host(w0))
    rev = R.ilrma(X, *R.parity_start(shape), 5, w0=host(w0), reverse=True)
    assert not ref.status.any()
    check_three("started from auxiva", (host(got.w), host(got.basis), host(got.activations)), ref[:3],
                R.tolerance_of(R.difference(ref, rev), D, F, T, L), demand=False)


def test_masks_drive_the_mask_beamformers():
    shape = R.SEPARATION[0]
    x = dev(R.parity_case(shape).X)
    sep = SEP.ilrma(x, *starts(shape), iterations=shape[5])
    m = SEP.masks(sep.spec)[:, 0].contiguous()
    mvdr = BF.mvdr(x, noise_mask=1 - m, speech_mask=m)
    gev = BF.gev(x, 1 - m, m)
    assert not host(sep.status).any() and not host(mvdr.status).any() and not host(gev.status).any()


def test_separate_waves_is_stft_ilrma_istft():
    from acoustic_locating_vq_vae import _native as N
    g = np.random.default_rng(2400)
    B, D, S = 2, 2, 2400
    for real in (torch.float64, torch.float32):
        waves = dev(g.standard_normal((B, D, S))).to(real)
        spec = N.stft_complex(waves.reshape(B * D, S).contiguous())
        F, T = spec.shape[1:]
        spec = spec.view(B, D, F, T)
        got = SEP.separate_waves(waves, iterations=3, method="ilrma", bases=3, generator=torch.Generator(device="cuda").manual_seed(9))
        assert got.dtype == real and got.shape == (B, D, S)
        b0, a0 = SEP.nmf_init(B, D, F, T, bases=3, generator=torch.Generator(device="cuda").manual_seed(9))
        assert b0.shape == (B, D, F, 3) and a0.shape == (B, D, 3, T) and b0.is_cuda
        assert bool((b0 >= 1e-3).all()) and bool((b0 < 1.0 + 1e-3).all())
        sep = SEP.ilrma(spec, b0, a0, 3)
        assert same_bits(got, FE.istft(sep.spec.reshape(B * D, F, T), length=S).view(B, D, S))
        assert not same_bits(got, SEP.separate_waves(waves, iterations=3))                    # the default is AuxIVA still


def test_two_sources_in_an_image_source_room():
    """The room of tests/test_iva_gpu.py's test of this name: the device's W, basis and activations against the restatement run
    on the downloaded spectrogram and start.  What ILRMA gains there is printed next to AuxIVA's, not asserted: nobody has
    measured it."""
    cfg = FE.DATASET_CONFIG
    n, D, L, iterations = 16000, 2, 2, 10
    g = np.random.default_rng(31)
    activity = np.repeat(g.gamma(0.3, size=(2, n // FE.HOP)) + 1e-3, FE.HOP, axis=1)
    clean = dev((g.standard_normal((2, n)) * activity).astype(np.float32))
    centre = np.array(cfg["receiver_position"])
    mics = dev(centre + np.array([[-0.05, 0.0, 0.0], [0.05, 0.0, 0.0]]))
    src = dev(np.array([[1.0, 3.5, 1.0], [3.2, 0.8, 1.9]]))
    h = FE.array_impulse_responses(src, mics, cfg["room_dimensions"], reverberation_time=0.2, nsample=3200)
    images = FE.array_spectrograms(clean, h)                                                # (2, D, F, T): source b at the microphones
    spec = images.sum(dim=0, keepdim=True)                                                  # (1, D, F, T): what the array records
    F, T = spec.shape[2:]
    b0, a0 = SEP.nmf_init(1, D, F, T, L, generator=torch.Generator(device="cuda").manual_seed(31))
    got = SEP.ilrma(spec, b0, a0, iterations)
    X = host(spec)
    ref = R.ilrma(X, host(b0), host(a0), iterations)
    rev = R.ilrma(X, host(b0), host(a0), iterations, reverse=True)
    assert np.array_equal(host(got.status), ref.status) and not ref.status.any()
    e_ref = R.difference(ref, rev)
    print("image-source room: kappa up to %.3g, e_ref %.3g" % (ref.kappa.max(), e_ref))
    check_three("image-source room", (host(got.w), host(got.basis), host(got.activations)), ref[:3],
                R.tolerance_of(e_ref, D, F, T, L), demand=False)
    want = FE.istft(images[:, 0].contiguous(), length=n)                                    # source b as microphone 0 hears it
    mix = FE.istft(spec[:, 0].contiguous(), length=n)
    for name, sep in (("ILRMA", got.spec), ("AuxIVA", SEP.auxiva(spec, iterations).spec),
                      ("ILRMA from AuxIVA", SEP.ilrma(spec, b0, a0, iterations, w0=SEP.auxiva(spec, iterations).w).spec)):
        waves = FE.istft(sep[0].contiguous(), length=n)
        assert waves.shape == (D, n) and bool(torch.isfinite(waves).all())
        gain = IR.improvement(host(want)[None], host(mix), host(waves)[None])
        print("image-source room: SI-SDR improvement of the waveforms, %s: %.2f dB" % (name, gain[0]))
