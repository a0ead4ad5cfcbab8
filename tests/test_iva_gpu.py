"""AuxIVA on the device (csrc/iva.hip, acoustic_locating_vq_vae.separation) against the float64 restatement of
tests/helpers/iva_ref.py, which tests/test_iva_cpu.py pins.  u = 1.1e-16.

W, per case:        max |W_dev - W_ref| <= tol max |W_ref|, tol = max(32 e_ref, 2 (T + F + 8 D) u), e_ref the largest relative
                    difference of the restatement run forward and with the frames and bins added in the opposite order: the
                    tolerance is measured on the reference, never on the device.  32: one pair of orders is a single sample of
                    reordering noise and the device's order is a third; it leaves a decade and a half.  tol <= 1e-10 is asserted
                    (a condition on the case), so a float32 accumulation, at 1e-7 or above, cannot hide.  complex64: the
                    restatement of the promoted input.
Y, per output:      |Y_dev - Y_ref| <= (16 D u cond_2(W) + 2 (D + 2) u) max |A[ref]| sum_d |W[k, d]| |x_d[t]| with the device's own
                    W given to the restatement's projection; complex64: 6e-8 |Y_ref| more for the one rounding of Y.
                    cond_2(W) <= 1e6 is asserted.
SI-SDR:             a relative error delta in Y moves an SI-SDR of S dB by about 8.7 delta 10^(S / 20) dB: within 1e-6 dB.
Masks:              8 u."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import iva_ref as R  # noqa: E402
from parity_checks import check_w  # noqa: E402
from acoustic_locating_vq_vae import beamforming as BF  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import separation as SEP  # noqa: E402

U = R.U
CDTYPES = [np.complex128, np.complex64]


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


def same_iva(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def device_run(shape, model, cdtype):
    """(W, Y, status) of a parity or separation shape on the device, downloaded; computed once."""
    out = SEP.auxiva(dev(R.parity_case(shape).X.astype(cdtype)), shape[4], model)
    B, D, F, T = shape[:4]
    assert out.spec.shape == (B, D, F, T) and out.spec.dtype == (torch.complex64 if cdtype == np.complex64 else torch.complex128)
    assert out.w.shape == (B, F, D, D) and out.w.dtype == torch.complex128
    assert out.status.shape == (B, F) and out.status.dtype == torch.int32
    return host(out.w), host(out.spec), host(out.status)


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("cdtype", CDTYPES, ids=["complex128", "complex64"])
@pytest.mark.parametrize("model", R.MODELS)
@pytest.mark.parametrize("shape", R.PARITY, ids=R.IDS)
def test_w_parity(shape, model, cdtype):
    single = cdtype == np.complex64
    W, _, status = device_run(shape, model, cdtype)
    ref = R.reference(shape, model, single=single)
    assert not status.any() and not ref.status.any()
    check_w("%s %s %s" % (shape[:4], model, np.dtype(cdtype).name), W, ref.W, R.w_tolerance(shape, model, single))


@pytest.mark.parametrize("cdtype", CDTYPES, ids=["complex128", "complex64"])
@pytest.mark.parametrize("model", R.MODELS)
@pytest.mark.parametrize("shape", R.PARITY, ids=R.IDS)
def test_y_parity(shape, model, cdtype):
    single = cdtype == np.complex64
    W, Y, status = device_run(shape, model, cdtype)
    Xp = R.promoted(R.parity_case(shape).X, single)
    want, _, st = R.project(Xp, W, status)                # the device's own W: only the projection differs
    assert not st.any()
    bound, cond = R.y_bound(Xp, W, 0)
    assert cond <= R.COND_CAP
    if single:
        bound = bound + 6e-8 * np.abs(want)
    err = np.abs(Y.astype(np.complex128) - want)
    print("%s %s %s: largest |Y - Y_ref| / bound %.3g, cond_2(W) up to %.3g" % (shape[:4], model, np.dtype(cdtype).name,
                                                                              (err / bound).max(), cond))
    assert (err <= bound).all()


def test_another_reference_microphone_and_ranks():
    shape = R.PARITY[3]
    B, D, F, T = shape[:4]
    x = dev(R.parity_case(shape).X)
    first = SEP.auxiva(x, 5)
    last = SEP.auxiva(x, 5, ref=D - 1)
    assert same_bits(first.w, last.w) and torch.equal(first.status, last.status)          # ref enters the projection alone
    W = host(last.w)
    want, _, _ = R.project(R.parity_case(shape).X, W, host(last.status), D - 1)
    bound, _ = R.y_bound(R.parity_case(shape).X, W, D - 1)
    assert (np.abs(host(last.spec) - want) <= bound).all()
    three = SEP.auxiva(x[0], 5)                                                             # ranks mirror the input
    assert three.spec.shape == (D, F, T) and three.w.shape == (F, D, D) and three.status.shape == (F,)
    assert all(same_bits(a, b[0]) for a, b in zip(three, first))
    again = SEP.auxiva(x[0], 2, w0=three.w)                                                 # ... and so does w0's
    assert all(same_bits(a, b[0]) for a, b in zip(again, SEP.auxiva(x, 2, w0=first.w)))
    view = dev(R.parity_case(shape).X.transpose(0, 1, 3, 2)).transpose(2, 3)               # a strided (B, D, F, T) view
    assert not view.is_contiguous() and same_iva(SEP.auxiva(view, 5), first)
    zero = SEP.auxiva(x, 0)                               # no iteration: W = I, whose "source" ref is microphone ref and the others 0
    assert bool((zero.w == torch.eye(D, dtype=torch.complex128, device="cuda")).all())
    assert torch.equal(zero.spec[:, 0], x[:, 0]) and bool((zero.spec[:, 1:] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ status
@pytest.mark.parametrize("cdtype", CDTYPES, ids=["complex128", "complex64"])
def test_bad_bins_come_back_as_they_came(cdtype):
    """A bin of zeros and a bin with one NaN in one launch: status 1, Y = X bit for bit and W = I; the other bins have the
    bits of a launch without those two bins' data, and agree with the restatement, whose p passes such bins over."""
    shape = R.PARITY[2]
    B, D, F, T = shape[:4]
    X = R.parity_case(shape).X.astype(cdtype)
    X[0, :, 1] = 0
    X[1, 1, 3, 40] = complex(np.nan, 1.0)
    x = dev(X)
    got = SEP.auxiva(x, 5)
    want = np.zeros((B, F), np.int32)
    want[0, 1] = want[1, 3] = 1
    assert np.array_equal(host(got.status), want)
    eye = torch.eye(D, dtype=torch.complex128, device="cuda")
    for b, f in ((0, 1), (1, 3)):
        assert same_bits(got.spec[b, :, f], x[b, :, f]) and same_bits(got.w[b, f], eye)
    for b, f in ((0, 1), (1, 3)):                         # the item without the bad bin's data
        keep = [g for g in range(F) if g != f]
        alone = SEP.auxiva(x[b:b + 1, :, keep].contiguous(), 5)
        assert same_bits(alone.w[0], got.w[b, keep]) and same_bits(alone.spec[0], got.spec[b][:, keep])
        assert not host(alone.status).any()
    ref = R.auxiva(X.astype(np.complex128), 5)
    assert np.array_equal(ref.status, want)
    keep = want == 0
    tol = max(32 * np.abs(ref.W - R.auxiva(X.astype(np.complex128), 5, reverse=True).W).max() / np.abs(ref.W).max(),
              2 * (T + F + 8 * D) * U)
    check_w("neighbours of the bad bins, %s" % np.dtype(cdtype).name, host(got.w)[keep], ref.W[keep], tol)


def test_identical_microphones_are_refused():
    """A bin whose two microphones are identical is rank-deficient: status 2, W = I, and it comes back as X; its neighbours
    get status 0."""
    shape = R.PARITY[2]
    B, D, F, T = shape[:4]
    X = R.parity_case(shape).X.copy()
    X[1, :, 5] = X[1, 0, 5]
    for cdtype in CDTYPES:
        x = dev(X.astype(cdtype))
        got = SEP.auxiva(x, 5)
        want = np.zeros((B, F), np.int32)
        want[1, 5] = 2
        assert np.array_equal(host(got.status), want)
        assert same_bits(got.spec[1, :, 5], x[1, :, 5])
        assert same_bits(got.w[1, 5], torch.eye(D, dtype=torch.complex128, device="cuda"))
        assert np.array_equal(R.auxiva(X.astype(cdtype).astype(np.complex128), 5).status, want)
        assert bool(torch.isfinite(torch.view_as_real(got.spec)).all())


# --------------------------------------------------------------------------------------------------------- reproducibility
def test_runs_repeat_and_items_do_not_see_each_other():
    shape = R.PARITY[2]
    X = R.parity_case(shape).X
    other = R.case(1, shape[1], shape[2], shape[3], 77).X
    for model in R.MODELS:
        x = dev(np.concatenate([other, X[1:2], X[0:1]]))                                      # a batch of three
        first, second = SEP.auxiva(x, 5, model), SEP.auxiva(x, 5, model)
        assert same_iva(first, second)
        alone = SEP.auxiva(x[1:2].contiguous(), 5, model)
        assert all(same_bits(a[0], b[1]) for a, b in zip(alone, first))


def test_more_bins_than_the_grid_holds():
    """Every launch over bins caps its grid at 65536 workgroups and strides: 300 000 three-frame bins pass the cap of the
    wave-a-bin launches (four bins a workgroup), of the covariances (a wave a (bin, k)) and of the projection (a workgroup a
    bin), and the last item has the bits it has alone, where no launch strides; 21 000 000 mask outputs pass the cap of the
    elementwise launch."""
    g = torch.Generator(device="cuda").manual_seed(5)

    def gauss(*shape, real=torch.float64):
        return torch.complex(torch.randn(shape, dtype=real, device="cuda", generator=g), torch.randn(shape, dtype=real, device="cuda", generator=g))
    B, D, F, T = 5, 2, 60000, 3
    x = gauss(B, D, F, T)
    x[B - 1, :, F - 2] = 0                                # a status among the strided bins
    whole = SEP.auxiva(x, 2)
    alone = SEP.auxiva(x[B - 1:].contiguous(), 2)
    assert all(same_bits(a[0], w[B - 1]) for a, w in zip(alone, whole))
    assert int(whole.status[B - 1, F - 2]) == 1 and int((whole.status == 1).sum()) == 1
    del x, whole, alone
    F, T = 70000, 300
    y = gauss(1, 1, F, T, real=torch.float32)
    m = SEP.masks(y)
    assert bool((m == 1).all())                           # K = 1: q / q
    y2 = gauss(1, 2, F, T, real=torch.float32)
    tail = slice(F - 7, F)
    assert same_bits(SEP.masks(y2[:, :, tail].contiguous())[0], SEP.masks(y2)[0][:, tail])


@pytest.mark.parametrize("shape", [R.PARITY[2], R.PARITY[5]], ids=[R.IDS[2], R.IDS[5]])
def test_continuation_through_w0_has_the_same_bits(shape):
    x = dev(R.parity_case(shape).X)
    for model in R.MODELS:
        whole = SEP.auxiva(x, 3 + 4, model)
        again = SEP.auxiva(x, 4, model, w0=SEP.auxiva(x, 3, model).w)
        assert same_iva(whole, again)


def test_graph_capture_replays_the_eager_bits():
    shape = R.PARITY[2]
    x = dev(R.parity_case(shape).X)
    eager = SEP.auxiva(x, 5)
    eager_masks = SEP.masks(eager.spec)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = SEP.auxiva(x, 5)
        m = SEP.masks(out.spec)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same_iva(out, eager) and same_bits(m, eager_masks)


# -------------------------------------------------------------------------------------------------------------- separation
@pytest.mark.parametrize("shape", R.SEPARATION, ids=["-".join(str(v) for v in s[:4]) for s in R.SEPARATION])
def test_separation_matches_the_restatement(shape):
    c = R.parity_case(shape)
    _, Y, status = device_run(shape, "laplace", np.complex128)
    ref = R.reference(shape, "laplace")
    assert not status.any()
    for b in range(shape[0]):
        want, perm = R.best_permutation_si_sdr(c.images[b], ref.Y[b])
        got = np.array([R.si_sdr(c.images[b, i], Y[b, perm[i]]) for i in range(shape[1])])
        print("%s item %d: SI-SDR %s dB, the restatement's %s dB" % (shape[:4], b, np.round(got, 3), np.round(want, 3)))
        assert (np.abs(got - want) <= 1e-6).all()
    gain = R.improvement(c.images, c.mix, Y)
    print("%s: SI-SDR improvement %s dB" % (shape[:4], np.round(gain, 2)))
    assert (gain >= 20.0).all()


# ------------------------------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("cdtype", CDTYPES, ids=["complex128", "complex64"])
def test_masks(cdtype):
    shape = R.SEPARATION[0]
    B, D, F, T = shape[:4]
    Y = device_run(shape, "laplace", np.complex128)[1].astype(cdtype)
    Y[0, :, 2, 5] = 0                                     # a silent point: 1 / K
    Y[1, 1, 3, 6] = complex(np.inf, 0.0)                  # a sum that is not finite: 0
    y = dev(Y)
    m = SEP.masks(y)
    assert m.dtype == torch.float64 and m.shape == (B, D, F, T)
    want = R.masks(Y)
    got = host(m)
    assert (np.abs(got - want) <= 8 * U).all()
    assert (got[0, :, 2, 5] == 1.0 / D).all() and (got[1, :, 3, 6] == 0).all()
    total = got.sum(axis=1)
    total[1, 3, 6] = 1.0
    assert (np.abs(total - 1.0) <= 4 * D * U).all()
    assert SEP.masks(y[0]).shape == (D, F, T) and same_bits(SEP.masks(y[0]), m[0])


def test_masks_drive_the_mask_beamformers():
    shape = R.SEPARATION[0]
    x = dev(R.parity_case(shape).X)
    sep = SEP.auxiva(x, shape[4])
    m = SEP.masks(sep.spec)[:, 0].contiguous()
    mvdr = BF.mvdr(x, noise_mask=1 - m, speech_mask=m)
    gev = BF.gev(x, 1 - m, m)
    assert not host(mvdr.status).any() and not host(gev.status).any()


def test_separate_waves_is_stft_auxiva_istft():
    from acoustic_locating_vq_vae import _native as N
    g = np.random.default_rng(2400)
    B, D, S = 2, 2, 2400
    for real in (torch.float64, torch.float32):
        waves = dev(g.standard_normal((B, D, S))).to(real)
        spec = N.stft_complex(waves.reshape(B * D, S).contiguous())
        spec = spec.view(B, D, spec.shape[1], spec.shape[2])
        got = SEP.separate_waves(waves, iterations=3)
        assert got.dtype == real and got.shape == (B, D, S)
        sep = SEP.auxiva(spec, 3)
        assert same_bits(got, FE.istft(sep.spec.reshape(B * D, spec.shape[2], spec.shape[3]), length=S).view(B, D, S))


# ------------------------------------------------------------------------------------------------ the chain, on real geometry
def test_two_sources_in_an_image_source_room():
    """Two sources in one generated room, two microphones 10 cm apart, reverberation_time 0.2, a second of seeded noise shaped
    by a per-frame activity per source: the device's W against the restatement run on the downloaded spectrogram.  What AuxIVA
    gains there is printed, not asserted: nobody has measured it."""
    cfg = FE.DATASET_CONFIG
    n, D, iterations = 16000, 2, 10
    g = np.random.default_rng(31)
    activity = np.repeat(g.gamma(0.3, size=(2, n // FE.HOP)) + 1e-3, FE.HOP, axis=1)
    clean = dev((g.standard_normal((2, n)) * activity).astype(np.float32))
    centre = np.array(cfg["receiver_position"])
    mics = dev(centre + np.array([[-0.05, 0.0, 0.0], [0.05, 0.0, 0.0]]))
    src = dev(np.array([[1.0, 3.5, 1.0], [3.2, 0.8, 1.9]]))
    h = FE.array_impulse_responses(src, mics, cfg["room_dimensions"], reverberation_time=0.2, nsample=3200)
    images = FE.array_spectrograms(clean, h)                                                # (2, D, F, T): source b at the microphones
    spec = images.sum(dim=0, keepdim=True)                                                  # (1, D, F, T): what the array records
    assert spec.dtype == torch.complex128 and spec.shape[1] == D
    got = SEP.auxiva(spec, iterations)
    X = host(spec)
    F, T = X.shape[2:]
    ref = R.auxiva(X, iterations)
    assert np.array_equal(host(got.status), ref.status) and not ref.status.any()
    e_ref = np.abs(ref.W - R.auxiva(X, iterations, reverse=True).W).max() / np.abs(ref.W).max()
    print("image-source room: kappa up to %.3g, e_ref %.3g" % (ref.kappa.max(), e_ref))
    check_w("image-source room", host(got.w), ref.W, max(32 * e_ref, 2 * (T + F + 8 * D) * U))
    want = FE.istft(images[:, 0].contiguous(), length=n)                                    # source b as microphone 0 hears it
    mix = FE.istft(spec[:, 0].contiguous(), length=n)
    waves = FE.istft(got.spec[0].contiguous(), length=n)
    assert waves.shape == (D, n) and bool(torch.isfinite(waves).all())
    gain = R.improvement(host(want)[None], host(mix), host(waves)[None])
    print("image-source room: SI-SDR improvement of the waveforms %.2f dB" % gain[0])
