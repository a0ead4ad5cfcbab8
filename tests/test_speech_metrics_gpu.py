"""Rational resampling, STOI, SI-SDR and the log-spectral distance on the device (csrc/speech_metrics.hip, acoustic_locating_
vq_vae.speech_metrics) against scipy.signal.resample_poly and the float64 restatement of tests/helpers/speech_metrics_ref.py.

Tolerances.  Resampling: max |y - scipy| <= 1e-12 max |x|: each output is a sum of a few dozen products of magnitude
<= max |x|, each rounded to 1.1e-16 relative, in another order than scipy's.  STOI: 1e-10 absolute: every sum has at most 512
non-negative or O(1) terms at about 6e-14 relative, and the mean removal amplifies that by the envelope's mean over its
deviation, below about 1e2 on these inputs; kept_frames and status are exact, and the restatement's margin (the distance of
the nearest frame level to the silent-frame threshold) is asserted >= 1e-6 dB so that the two sides keep the same frames.
SI-SDR: 1e-9 dB: the inputs stay under 60 dB, so the difference a s - e keeps 10 of its 16 digits.  LSD: 1e-10 dB."""
import os
import sys

import numpy as np
import pytest
import scipy.signal
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import speech_metrics_ref as R  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as M  # noqa: E402

RESAMPLE_RTOL, STOI_ATOL, SI_SDR_ATOL, LSD_ATOL = 1e-12, 1e-10, 1e-9, 1e-10
MIN_MARGIN_DB = 1e-6


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a, b):
    """Two STOI tuples (or tensors) equal bit for bit, NaN and inf included."""
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    return all(x.shape == y.shape and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def noisy_pair(n, seed, rows=1):
    """White Gaussian rows and the same plus half as much noise."""
    g = np.random.default_rng(seed)
    clean = g.standard_normal((rows, n))
    return clean, clean + 0.5 * g.standard_normal((rows, n))


def check_stoi(got, clean, degraded, tag=""):
    """got: STOI of (B,) device tensors; clean, degraded: the B rows at 10 kHz on the host.  Returns the restatement's rows."""
    value, kept, status = (t.cpu().numpy() for t in got)
    assert value.dtype == np.float64 and kept.dtype == np.int32 and status.dtype == np.int32
    refs = []
    for b in range(clean.shape[0]):
        ref = R.stoi(clean[b], degraded[b])
        refs.append(ref)
        print("%s row %d: device %.17g restatement %.17g kept %d / %d of %d status %d / %d margin %.3g dB"
              % (tag, b, value[b], ref.value, kept[b], ref.kept_frames, ref.nf, status[b], ref.status, ref.margin))
        assert ref.margin >= MIN_MARGIN_DB, (b, ref.margin)
        assert kept[b] == ref.kept_frames and status[b] == ref.status, (b, kept[b], status[b], ref)
        if np.isnan(ref.value):
            assert np.isnan(value[b]), (b, value[b])
        else:
            assert abs(value[b] - ref.value) <= STOI_ATOL, (b, value[b], ref.value, abs(value[b] - ref.value))
    return refs


# ----------------------------------------------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("n,up,down", [(1, 5, 8), (21, 5, 8), (1000, 5, 8), (1603, 5, 8), (777, 3, 2), (50, 1, 3),
                                       (4099, 160, 441), (4000, 10000, 16000)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resample_poly_is_scipys(n, up, down, dtype):
    x = np.random.default_rng(n + up).standard_normal((3, n)).astype(dtype)
    want = scipy.signal.resample_poly(x.astype(np.float64), up, down, axis=-1)
    got = M.resample_poly(dev(x), up, down)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == want.shape == (3, -(-n * up // down))
    err, bound = np.abs(got.cpu().numpy() - want).max(), RESAMPLE_RTOL * np.abs(x).max()
    print("n %d %d/%d %s: max |y - scipy| = %.3g (bound %.3g)" % (n, up, down, dtype.__name__, err, bound))
    assert err <= bound
    assert same_bits(got, M.resample_poly(dev(x), up, down))
    assert same_bits(M.resample_poly(dev(x[1]), up, down), got[1])          # (n,) in, (n_out,) out


# ------------------------------------------------------------------------------------------------------------ STOI at 10 kHz
@pytest.mark.parametrize("n,kept,status", [(3968, 30, 0), (3967, 29, 2), (4096, 31, 0), (5248, 40, 0), (255, 0, 1)])
def test_stoi_against_the_restatement(n, kept, status):
    clean, degraded = noisy_pair(n, 1000 + n, rows=2)
    got = M.stoi(dev(clean), dev(degraded), fs=10000)
    assert all(t.shape == (2,) and t.is_cuda for t in got)
    refs = check_stoi(got, clean, degraded, "n %d" % n)
    assert all(r.kept_frames == kept and r.status == status for r in refs)
    one = M.stoi(dev(clean[1]), dev(degraded[1]), fs=10000)                 # (n,) in, 0-d out
    assert all(t.dim() == 0 for t in one) and same_bits(tuple(t[None] for t in one), tuple(t[1:2] for t in got))


def masked_rows():
    """n = 5248 (40 frames): clean rows with a stretch scaled down until its frames fall out, with the count kept."""
    g = np.random.default_rng(7)
    rows = []
    for (a, b), scale, kept in (((1280, 2560), 1e-4, 31), ((1280, 2688), 1e-4, 30), ((1280, 2816), 1e-4, 29)):
        x = g.standard_normal(5248)
        x[a:b] *= scale
        rows.append((x, kept))
    x = g.standard_normal(5248)
    x[:1000] *= 1e-5
    x[-700:] *= 1e-5
    rows.append((x, 30))
    return rows


def test_stoi_silent_frame_mask():
    rows = masked_rows()
    clean = np.stack([x for x, _ in rows])
    degraded = clean + 0.5 * np.random.default_rng(8).standard_normal(clean.shape)
    refs = check_stoi(M.stoi(dev(clean), dev(degraded), fs=10000), clean, degraded, "mask")
    assert [r.kept_frames for r in refs] == [kept for _, kept in rows] == [31, 30, 29, 30]
    assert [r.status for r in refs] == [0, 0, 2, 0]


def test_stoi_rows_of_one_batch_keep_different_numbers_of_frames():
    """M = 40, 31, 30, 29 and an all-zero clean row in one batch: each row is its own single-row call bit for bit."""
    rows = masked_rows()
    full = np.random.default_rng(9).standard_normal(5248)
    clean = np.stack([full, rows[0][0], rows[1][0], rows[2][0], np.zeros(5248)])
    degraded = clean + 0.5 * np.random.default_rng(10).standard_normal(clean.shape)
    x, y = dev(clean), dev(degraded)
    got = M.stoi(x, y, fs=10000)
    check_stoi(got, clean, degraded, "batch")
    assert got.kept_frames.tolist() == [40, 31, 30, 29, 0] and got.status.tolist() == [0, 0, 0, 2, 1]
    for b in range(5):
        assert same_bits(tuple(t[b:b + 1] for t in got), M.stoi(x[b:b + 1], y[b:b + 1], fs=10000)), b
    assert same_bits(got, M.stoi(x, y, fs=10000))


def test_stoi_of_a_signal_against_itself_is_one():
    clean, _ = noisy_pair(5248, 11, rows=2)
    clean = np.concatenate([clean, masked_rows()[0][0][None]])
    got = M.stoi(dev(clean), dev(clean), fs=10000)
    print("stoi(x, x) - 1:", (got.value - 1.0).tolist())
    assert got.status.tolist() == [0, 0, 0] and float((got.value - 1.0).abs().max()) <= 1e-12


def test_stoi_float32_input_is_the_float64_call_on_the_widened_rows():
    clean, degraded = noisy_pair(4096, 12, rows=2)
    x, y = dev(clean.astype(np.float32)), dev(degraded.astype(np.float32))
    assert same_bits(M.stoi(x, y, fs=10000), M.stoi(x.double(), y.double(), fs=10000))


def test_stoi_of_rows_without_energy():
    clean, degraded = noisy_pair(5248, 13, rows=3)
    clean[0, 77] = np.inf
    clean[1, 4000] = np.nan
    degraded[2, 300] = np.nan                      # a degraded row's own trouble: NaN value, status 0
    got = M.stoi(dev(clean), dev(degraded), fs=10000)
    assert got.status.tolist() == [1, 1, 0] and got.kept_frames.tolist() == [0, 0, 40]
    assert torch.isnan(got.value).tolist() == [True, True, True]


# ------------------------------------------------------------------------------------------------------------ STOI at 16 kHz
def test_stoi_at_16_khz_resamples_first():
    clean, degraded = noisy_pair(16000, 14, rows=2)
    x, y = dev(clean), dev(degraded)
    got = M.stoi(x, y)                              # fs = 16000
    c10, d10 = (scipy.signal.resample_poly(v, 5, 8, axis=-1) for v in (clean, degraded))
    assert c10.shape == (2, 10000)
    check_stoi(got, c10, d10, "16 kHz")
    assert same_bits(got, M.stoi(M.resample_poly(x, 5, 8), M.resample_poly(y, 5, 8), fs=10000))
    assert same_bits(got, M.stoi(x, y, fs=16000))


# --------------------------------------------------------------------------------------------------- real pipeline data
def test_stoi_falls_in_a_reverberant_room():
    """Two seconds of noise under a syllable-rate envelope at 16 kHz, convolved with the response of DATASET_CONFIG's room."""
    cfg = FE.DATASET_CONFIG
    fs, n = cfg["fs"], 32000
    g = np.random.default_rng(15)
    t = np.arange(n) / fs
    envelope = (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + 0.3)) * (0.6 + 0.4 * np.sin(2 * np.pi * 1.3 * t))
    clean = (g.standard_normal(n) * envelope).astype(np.float32)
    h = FE.rir_generate(340.0, fs, cfg["receiver_position"], [1.0, 3.5, 1.0], cfg["room_dimensions"],
                        reverberation_time=cfg["reverberation_time"], nsample=cfg["n_sample"])[:, 0]
    x = dev(clean)[None]
    echoed = FE.N.fir_same(x, h.contiguous())
    assert echoed.dtype == torch.float64 and echoed.shape == (1, n)
    got = M.stoi(x.double(), echoed)
    same = M.stoi(x.double(), x.double())
    c10, e10 = (scipy.signal.resample_poly(v.cpu().numpy().astype(np.float64), 5, 8, axis=-1) for v in (x, echoed))
    check_stoi(got, c10, e10, "echoed")
    # the 'same' convolution keeps the centre of the full one: the echoed signal runs (Nh - 1) // 2 samples ahead of the clean
    # one, and STOI compares frame against frame.  Lined up again, what is left is the room.
    lead = (h.shape[0] - 1) // 2
    aligned = M.stoi(x.double()[:, lead:].contiguous(), echoed[:, :n - lead].contiguous())
    check_stoi(aligned, scipy.signal.resample_poly(x.double()[:, lead:].cpu().numpy(), 5, 8, axis=-1),
               scipy.signal.resample_poly(echoed[:, :n - lead].cpu().numpy(), 5, 8, axis=-1), "echoed, lined up")
    print("stoi(clean, clean) %.17g stoi(clean, echoed) %.17g lined up %.17g" % (float(same.value), float(got.value),
                                                                                 float(aligned.value)))
    assert float(got.value) < float(same.value) and abs(float(same.value) - 1.0) <= 1e-12
    assert float(got.value) < float(aligned.value) < float(same.value)


# ---------------------------------------------------------------------------------------------------------------------- SI-SDR
@pytest.mark.parametrize("n", [2, 63, 64, 65, 1000, 40000])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_si_sdr_against_the_restatement(n, dtype):
    """Noise at -3, -20 and -50 dB of the reference, an offset and a gain on the estimate: every row stays under 60 dB.  Two
    samples less their means are (a, -a) and (b, -b), always multiples of each other: at n = 2 the distortion is rounding
    alone, so there both sides must say +inf or a ratio no double arithmetic gives otherwise (above 280 dB)."""
    g = np.random.default_rng(2000 + n)
    s = (g.standard_normal((3, n)) + 0.25).astype(dtype)
    e = ((0.7 * s + g.standard_normal((3, n)) * np.array([[0.7], [0.1], [3e-3]]) - 0.5)).astype(dtype)
    got = M.si_sdr(dev(s), dev(e))
    assert got.shape == (3,) and got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    for b in range(3):
        want = R.si_sdr(s[b], e[b])
        print("n %d %s row %d: device %.17g restatement %.17g" % (n, dtype.__name__, b, got[b], want))
        if n == 2:
            assert got[b] > 280.0 and want > 280.0, (b, got[b], want)
        else:
            assert want < 60.0 and abs(got[b] - want) <= SI_SDR_ATOL, (b, got[b], want)
    assert same_bits(M.si_sdr(dev(s[2]), dev(e[2]))[None], M.si_sdr(dev(s), dev(e))[2:3])


def test_si_sdr_edges():
    g = np.random.default_rng(16)
    s = g.standard_normal((5, 777))
    e = s + 0.1 * g.standard_normal((5, 777))
    e[0] = -4.0 * s[0]                     # an exact multiple
    e[1] = 0.5 * s[1] + 0.0
    s[2] = 0.0                             # no reference
    s[3] = 3.25                            # a constant has no energy once its mean is gone
    got = M.si_sdr(dev(s), dev(e)).cpu().numpy()
    want = [R.si_sdr(s[b], e[b]) for b in range(5)]
    print("si_sdr edges: device", got.tolist(), "restatement", want)
    assert got[0] == got[1] == np.inf and np.isnan(got[2]) and np.isnan(got[3]) and abs(got[4] - want[4]) <= SI_SDR_ATOL
    assert want[0] == want[1] == np.inf and np.isnan(want[2]) and np.isnan(want[3])
    assert same_bits(M.si_sdr(dev(s), dev(e)), M.si_sdr(dev(s), dev(e)))


# ------------------------------------------------------------------------------------------------------------------------- LSD
@pytest.mark.parametrize("F,T", [(1, 1), (201, 3), (201, 500), (65, 257)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lsd_against_the_restatement(F, T, dtype):
    g = np.random.default_rng(F * 1000 + T)
    p = (g.standard_normal((3, F, T)) ** 2).astype(dtype)
    q = (p * np.exp(g.standard_normal((3, F, T))) + 1e-3 * g.random((3, F, T))).astype(dtype)
    p[0, 0, 0] = 0.0                        # zeros are legal: eps keeps the logarithm finite
    got = M.log_spectral_distance(dev(p), dev(q))
    assert got.shape == (3,) and got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    for b in range(3):
        want = R.log_spectral_distance(p[b], q[b])
        print("F %d T %d %s row %d: device %.17g restatement %.17g" % (F, T, dtype.__name__, b, got[b], want))
        assert abs(got[b] - want) <= LSD_ATOL, (b, got[b], want)
    one = M.log_spectral_distance(dev(p[1]), dev(q[1]), eps=1e-6)          # (F, T) in, 0-d out; another eps
    assert one.dim() == 0 and abs(float(one) - R.log_spectral_distance(p[1], q[1], eps=1e-6)) <= LSD_ATOL


def test_lsd_bad_rows_do_not_touch_their_neighbours():
    g = np.random.default_rng(17)
    p = g.random((4, 65, 40)) + 0.01
    q = g.random((4, 65, 40)) + 0.01
    good = M.log_spectral_distance(dev(p), dev(q))
    p[1, 64, 39] = -1e-12                   # smaller than eps: only the sign gives it away
    q[2, 0, 0] = np.inf
    got = M.log_spectral_distance(dev(p), dev(q))
    assert torch.isnan(got).tolist() == [False, True, True, False]
    assert same_bits(got[0::3], good[0::3]) and same_bits(got, M.log_spectral_distance(dev(p), dev(q)))


# -------------------------------------------------------------------------------------------------------------- stream capture
def test_graph_replay_gives_the_eager_bits():
    """stoi at 16 kHz -- two resampling launches and the four of STOI -- captured once and replayed on other data twice."""
    a = [dev(v) for v in noisy_pair(8000, 18, rows=3)]
    b = [dev(v) for v in noisy_pair(8000, 19, rows=3)]
    eager = M.stoi(*b)
    static = [v.clone() for v in a]
    M.stoi(*static)                         # the filter is on the device before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = M.stoi(*static)
    for dst, src in zip(static, b):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    first = tuple(t.clone() for t in out)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager) and same_bits(first, eager) and not same_bits(out, M.stoi(*a))
    assert eager.status.tolist() == [0, 0, 0]
