"""WPE dereverberation on the device (csrc/wpe.hip, acoustic_locating_vq_vae.dereverberation) against the float64 restatement
of tests/helpers/wpe_ref.py, which tests/test_wpe_cpu.py pins.

Tolerance, per bin, with M = D taps, u = 1.1e-16 and cond = the restatement's largest cond_2(R) of that bin:
    max |Y_dev - Y_ref| <= (8 M u cond + 1e-13) max |x|
-- the forward bound c n u kappa of a Cholesky solve, plus a term for the fixed-order sums of T <= 2000 terms, which the two
sides add in different orders.  Every bin's cond is asserted <= 1e6 (the inputs are chosen for it: wpe_ref.case), so no bin
hides behind its conditioning, and the well-conditioned shapes (cond about 10 at (T, D, taps) = (500, 1, 10) with a power
context and (257, 3, 7)) hold the device to about 2e-13: a stray float32 accumulation is five orders above that.
complex64 input: the restatement of the promoted input, and 6e-8 max |y| more for the one rounding of Y."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import wpe_ref as R  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import dereverberation as DV  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as SM  # noqa: E402

U = 1.1e-16
# (B, D, F, T, taps, delay, psd_context, loading)
SMALL = [(2, 1, 9, 64, 1, 1, 0, 1e-10), (2, 1, 9, 96, 5, 3, 0, 1e-10), (1, 1, 5, 200, 10, 3, 0, 1e-10),
         (1, 1, 3, 500, 10, 3, 1, 1e-10), (2, 2, 5, 200, 8, 2, 0, 1e-10),
         (1, 4, 3, 300, 16, 3, 0, 1e-10),          # the M = 64 cap
         (1, 3, 4, 257, 7, 3, 2, 1e-10),
         (1, 1, 3, 12, 10, 3, 0, 1e-3),            # T shorter than the filter
         (1, 2, 3, 40, 32, 1, 0, 1e-3),            # T < M
         (1, 4, 2, 2000, 16, 3, 0, 1e-10)]         # a row that cannot sit in LDS whole
DATASET = (2, 1, 201, 500, 10, 3, 0, 1e-10)        # the dataset's own shape


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()          # a copy: the shared cases are read-only


def same_bits(a, b):
    """Two tensors equal bit for bit, NaN included."""
    ra, rb = (torch.view_as_real(t.contiguous()) if t.is_complex() else t.contiguous() for t in (a, b))
    if ra.shape != rb.shape or ra.dtype != rb.dtype:
        return False
    view = {torch.float64: torch.int64, torch.float32: torch.int32}.get(ra.dtype)
    return torch.equal(ra.view(view), rb.view(view)) if view else torch.equal(ra, rb)


def run(X, case):
    B, D, F, T, taps, delay, ctx, loading = case
    return DV.wpe(dev(X), taps=taps, delay=delay, iterations=3, psd_context=ctx, eps=1e-10, loading=loading)


def check_parity(got, X, Yref, cond, case, rounding=0.0, skip=(), tag=""):
    """The per-bin bound on every bin (but the ``skip`` ones, which the caller checks); prints the largest measured / bound."""
    B, D, F, T, taps = case[:5]
    Y = got.cpu().numpy().astype(np.complex128)
    worst, worst_err = 0.0, 0.0
    for b in range(B):
        for f in range(F):
            if (b, f) in skip:
                continue
            assert cond[b, f] <= R.COND_CAP, (b, f, cond[b, f])
            err = float(np.abs(Y[b, :, f] - Yref[b, :, f]).max())
            bound = (8 * D * taps * U * cond[b, f] + 1e-13) * np.abs(X[b, :, f]).max() + rounding * np.abs(Yref[b, :, f]).max()
            if err / bound > worst:
                worst, worst_err = err / bound, err
            assert err <= bound, (tag, b, f, err, bound, cond[b, f])
    print("%s %s: largest measured / bound %.3g (|Y - Y_ref| %.3g there), cond up to %.3g"
          % (tag, case[:7], worst, worst_err, cond.max()))


# ------------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("case", SMALL + [DATASET], ids=lambda c: "-".join(str(v) for v in c[:7]))
def test_parity_complex128(case):
    c = R.case(*case)
    got = run(c.X, case)
    assert got.spec.dtype == torch.complex128 and got.spec.shape == c.X.shape
    assert got.status.dtype == torch.int32 and got.status.shape == (case[0], case[2])
    assert not got.status.cpu().numpy().any()
    check_parity(got.spec, c.X, c.Y, c.cond, case, tag="complex128")


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "-".join(str(v) for v in c[:7]))
def test_parity_complex64(case):
    B, D, F, T, taps, delay, ctx, loading = case
    X32 = R.case(*case).X.astype(np.complex64)
    Xp = X32.astype(np.complex128)
    Yref, status, cond = R.wpe(Xp, taps, delay, 3, ctx, 1e-10, loading)
    assert not status.any()
    got = run(X32, case)
    assert got.spec.dtype == torch.complex64 and got.spec.shape == X32.shape
    assert not got.status.cpu().numpy().any()
    check_parity(got.spec, Xp, Yref, cond, case, rounding=6e-8, tag="complex64")


# -------------------------------------------------------------------------------------------------------------- status bins
@pytest.mark.parametrize("cdtype", [np.complex128, np.complex64])
def test_zero_and_nan_bins_come_back_unchanged(cdtype):
    """A bin of zeros and a bin with one NaN in a launch: status 1 and Y = X bit for bit there, the other bins as ever."""
    case = SMALL[4]
    B, D, F, T, taps, delay, ctx, loading = case
    X = R.case(*case).X.astype(cdtype)
    X[0, :, 1] = 0
    X[1, 1, 3, 77] = complex(np.nan, 1.0)
    Yref, status, cond = R.wpe(X.astype(np.complex128), taps, delay, 3, ctx, 1e-10, loading)
    assert status[0, 1] == 1 and status[1, 3] == 1 and status.sum() == 2
    got = run(X, case)
    assert np.array_equal(got.status.cpu().numpy(), status)
    x = dev(X)
    for b, f in ((0, 1), (1, 3)):
        assert same_bits(got.spec[b, :, f], x[b, :, f])
    check_parity(got.spec, X.astype(np.complex128), Yref, cond, case, rounding=6e-8 if cdtype == np.complex64 else 0.0,
                 skip={(0, 1), (1, 3)}, tag="neighbours of the bad bins, %s" % np.dtype(cdtype).name)


@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("cdtype", [np.complex128, np.complex64])
def test_no_frame_with_a_past(T, cdtype):
    """T <= delay: R = 0, the first pivot is 0, status 2 and Y = X."""
    X = R.case(*SMALL[4]).X[:, :, :, :T].astype(cdtype)
    got = DV.wpe(dev(X), taps=4, delay=3)
    assert (got.status.cpu().numpy() == 2).all() and same_bits(got.spec, dev(X))


# ------------------------------------------------------------------------------------------------ repeatability, isolation
@pytest.mark.parametrize("case", [SMALL[1], SMALL[4], SMALL[9]], ids=lambda c: "-".join(str(v) for v in c[:7]))
def test_launches_repeat_and_bins_do_not_see_each_other(case):
    B, D, F, T = case[:4]
    X = R.case(*case).X
    first, second = run(X, case), run(X, case)
    assert same_bits(first.spec, second.spec) and torch.equal(first.status, second.status)
    for b in range(B):                                  # an item alone
        alone = run(X[b:b + 1], case)
        assert same_bits(alone.spec[0], first.spec[b]) and torch.equal(alone.status[0], first.status[b])
    alone = run(X[:1, :, F // 2:F // 2 + 1], case)      # a bin alone
    assert same_bits(alone.spec[0, :, 0], first.spec[0, :, F // 2])


def test_ranks_mirror_the_input():
    case = SMALL[1]
    B, D, F, T, taps, delay, ctx, loading = case
    X = R.case(*case).X
    four = run(X, case)
    three = run(X[:, 0], case)
    two = run(X[1, 0], case)
    assert three.spec.shape == (B, F, T) and three.status.shape == (B, F)
    assert two.spec.shape == (F, T) and two.status.shape == (F,)
    assert same_bits(three.spec, four.spec[:, 0]) and torch.equal(three.status, four.status)
    assert same_bits(two.spec, four.spec[1, 0]) and torch.equal(two.status, four.status[1])
    view = DV.wpe(dev(X[:, 0].transpose(0, 2, 1)).transpose(1, 2), taps=taps, delay=delay)      # a strided (B, F, T) view
    assert same_bits(view.spec, three.spec)


# ------------------------------------------------------------------------------------------------------------ dereverberate
def test_dereverberate_is_stft_wpe_istft():
    g = np.random.default_rng(4000)
    wave = dev(g.standard_normal((2, 4000)))
    got = DV.dereverberate(wave)
    want = FE.istft(DV.wpe(N.stft_complex(wave)).spec, length=4000)
    assert got.dtype == torch.float64 and got.shape == (2, 4000) and same_bits(got, want)
    one = DV.dereverberate(wave[1], taps=5, delay=2)
    assert one.shape == (4000,) and same_bits(one, FE.istft(DV.wpe(N.stft_complex(wave[1:]), taps=5, delay=2).spec, length=4000)[0])
    got32 = DV.dereverberate(wave.float())
    assert got32.dtype == torch.float32 and got32.shape == (2, 4000)
    assert same_bits(got32, FE.istft(DV.wpe(N.stft_complex(wave.float())).spec, length=4000))


def test_dereverberate_in_an_image_source_room():
    """Two seconds of noise under a syllable-rate envelope in DATASET_CONFIG's room, lined up with the clean signal.  What WPE
    gains on image-source rooms is printed, not asserted: nobody has measured it."""
    cfg = FE.DATASET_CONFIG
    fs, n = cfg["fs"], 32000
    g = np.random.default_rng(15)
    t = np.arange(n) / fs
    envelope = (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + 0.3)) * (0.6 + 0.4 * np.sin(2 * np.pi * 1.3 * t))
    clean = dev((g.standard_normal(n) * envelope).astype(np.float32))[None]
    h = FE.rir_generate(340.0, fs, cfg["receiver_position"], [1.0, 3.5, 1.0], cfg["room_dimensions"],
                        reverberation_time=cfg["reverberation_time"], nsample=cfg["n_sample"])[:, 0]
    echoed = N.fir_same(clean, h.contiguous())
    derev = DV.dereverberate(echoed)
    assert derev.dtype == torch.float64 and derev.shape == echoed.shape and bool(torch.isfinite(derev).all())
    lead = (h.shape[0] - 1) // 2
    c = clean.double()[:, lead:].contiguous()
    for name, v in (("echoed", echoed), ("dereverberated", derev)):
        v = v[:, :n - lead].contiguous()
        print("%s: stoi %.4f si_sdr %.2f dB" % (name, float(SM.stoi(c, v).value), float(SM.si_sdr(c, v))))
