"""Energy decay curves and room-acoustic parameters on the device (csrc/room_acoustics.hip, acoustic_locating_vq_vae.
room_acoustics) against the float64 restatement of tests/helpers/room_acoustics_ref.py.

Tolerances.  A sum of n non-negative terms has a relative error of at most about n 2^-53 in any order, so two tail energies
differ by <= 2 * 4.34 * n * 2^-53 dB: 6e-11 dB at n = 65536, and no row here is longer -- the curve and the dB ratios are held
to 1e-10 dB.  A slope fitted to M samples of such a curve moves by <= 3 delta / M per sample against a slope of about 30 dB / M,
about 1e-11 relative; the decay times are held to 1e-9 relative, which also covers the device's log10.  d50 is a ratio of two
such sums: 1e-12.  The fit sets themselves cannot differ: the restatement's margins (the distance of the nearest level to a
threshold) are asserted to be >= 1e-6 dB on the inputs of the parameter test."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import room_acoustics_ref as RA  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import room_acoustics as M  # noqa: E402

C, FS = 340.0, 16000.0
SMALL_ROOMS = [  # tests/test_rir_gpu.py's: (room, source, receiver, beta, nsample)
    ([1.0, 1.3, 0.9], [0.3, 0.4, 0.5], [0.7, 0.9, 0.2], [0.8, 0.7, 0.6, 0.9, 0.5, 0.7], 700),
    ([2.1, 1.6, 1.2], [1.9, 0.3, 0.4], [0.5, 1.1, 0.9], [0.8, -0.7, 0.6, -0.9, 0.5, -0.75], 900),
]
TIME_RTOL, DB_ATOL, D50_ATOL = 1e-9, 1e-10, 1e-12


def noise_decay(n, seed, decades=6.0):
    """Seeded Gaussian samples under an exponential envelope that falls by `decades` factors of ten in amplitude over the row."""
    g = np.random.default_rng(seed)
    return g.standard_normal(n) * np.exp(-decades * np.log(10.0) * np.arange(n) / n)


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a, b):
    """Two RoomAcoustics (or tensors) equal bit for bit, NaN and inf included."""
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def check_against_restatement(got, rows, fs=FS, min_margin=None):
    """got: RoomAcoustics of (B,) device tensors; rows: the B responses on the host."""
    got = [t.cpu().numpy() for t in got]
    refs = []
    for b, row in enumerate(rows):
        ref = RA.parameters(row, fs)
        refs.append(ref)
        if min_margin is not None:
            assert min(ref.margin.values()) >= min_margin, (b, ref.margin)
        assert got[7][b] == ref.onset and got[8][b] == ref.status, (b, got[7][b], got[8][b], ref.onset, ref.status)
        for i, name in enumerate(RA.COLUMNS):
            g, w = float(got[i][b]), float(ref[i])
            print("row %d %s: device %.17g restatement %.17g" % (b, name, g, w))
            if not np.isfinite(w):
                assert (np.isnan(g) and np.isnan(w)) or g == w, (b, name, g, w)
            elif name in ("t30", "t20", "edt"):
                assert abs(g - w) <= TIME_RTOL * abs(w), (b, name, g, w)
            else:
                assert abs(g - w) <= (D50_ATOL if name == "d50" else DB_ATOL), (b, name, g, w)
    return refs


@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 1000, 4099, 40000])
def test_energy_decay_curve(n):
    """Sizes around the wave (64), the scanned piece (256) and the tile (1024), one of several tiles that is no multiple of
    any of them, and one far longer than the LDS could hold.  The last row ends in exact zeros (100 of them, or half the row
    where it is shorter than 200): its curve ends in -inf."""
    h = np.stack([noise_decay(n, 100 + b) for b in range(3)])
    zeros = min(100, n // 2)
    h[2, n - zeros:] = 0.0
    got = M.energy_decay_curve(torch.from_numpy(h).cuda())
    assert got.shape == (3, n) and got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    for b in range(3):
        want = RA.edc_db(h[b])
        assert np.array_equal(np.isneginf(got[b]), np.isneginf(want)) and not np.isnan(got[b]).any(), b
        assert np.isneginf(want).sum() == (zeros if b == 2 else 0)
        fin = np.isfinite(want)
        err = np.abs(got[b][fin] - want[fin]).max()
        print("n %d row %d: max |edc - restatement| = %.3g dB" % (n, b, err))
        assert err <= DB_ATOL, (b, err)
        assert got[b][0] == 0.0 and (got[b][fin] <= 0.0).all()
    # the same rows one at a time and as (n,): bitwise the batch's
    x = torch.from_numpy(h).cuda()
    assert same_bits(M.energy_decay_curve(x[1]), M.energy_decay_curve(x)[1])


def test_energy_decay_curve_of_rows_without_energy():
    h = torch.from_numpy(np.stack([noise_decay(300, 1), np.zeros(300), noise_decay(300, 2)])).cuda()
    h[2, 17] = float("inf")
    got = M.energy_decay_curve(h).cpu().numpy()
    assert np.isfinite(got[0]).all() and np.isnan(got[1]).all() and np.isnan(got[2]).all()


@pytest.fixture(scope="module")
def parameter_rows():
    """The responses of the parameter test on the host, made once: two small rooms, a Sabine room, two analytic decays."""
    rows = []
    for L, s, r, beta, ns in SMALL_ROOMS:
        rows.append(FE.rir_generate(C, FS, r, s, L, beta=beta, nsample=ns)[:, 0].cpu().numpy())
    rows.append(FE.rir_generate(C, FS, [2.5, 1.5, 1.5], [3, 2, 2.5], [4, 5, 3], reverberation_time=0.2)[:, 0].cpu().numpy())
    assert [r.shape[0] for r in rows] == [700, 900, 3200]
    rows += [RA.analytic_decay(0.05), RA.analytic_decay(0.1)]
    return rows


def test_parameters_match_the_restatement(parameter_rows):
    refs = []
    for row in parameter_rows:
        got = M.room_acoustic_parameters(torch.from_numpy(row).cuda()[None])
        assert all(t.shape == (1,) and t.is_cuda for t in got)
        assert all(t.dtype == torch.float64 for t in got[:7]) and got.onset.dtype == got.status.dtype == torch.int32
        refs += check_against_restatement(got, [row], min_margin=1e-6)
    # both small rooms end before 50 ms: no late energy, c50 = c80 = +inf and bit 4 are part of what was compared
    assert all(r.status & RA.NO_LATE_ENERGY and r.c50 == np.inf for r in refs[:2]) and refs[2].status == 0
    for r, T60 in zip(refs[3:], (0.05, 0.1)):
        assert r.status == 0 and abs(r.t30 / T60 - 1) < 1e-9


def test_layouts_and_the_single_column(parameter_rows):
    """rir_generate's (nsample, M) layout goes in through .t(), strided input is packed; an (n,) response gives 0-d results;
    reverberation_time is one column of the same call."""
    L, s, _, beta, ns = SMALL_ROOMS[1]
    h = FE.rir_generate(C, FS, [[0.5, 1.1, 0.9], [1.0, 0.2, 0.3], [1.7, 1.4, 1.1]], s, L, beta=beta, nsample=ns)
    assert h.shape == (ns, 3)
    got = M.room_acoustic_parameters(h.t())
    packed = h.contiguous()                # (nsample, M) in memory: its .t() is strided
    assert not packed.t().is_contiguous() and same_bits(got, M.room_acoustic_parameters(packed.t()))
    assert same_bits(M.energy_decay_curve(h.t()), M.energy_decay_curve(packed.t()))
    check_against_restatement(got, h.t().cpu().numpy())
    one = M.room_acoustic_parameters(h[:, 1].contiguous())
    assert all(t.dim() == 0 for t in one) and same_bits(tuple(t[None] for t in one), tuple(t[1:2] for t in got))
    for method in ("t30", "t20", "edt"):
        assert same_bits(M.reverberation_time(h.t(), method=method), getattr(got, method))
    # another rate: the sample counts and the time axis follow it
    row = parameter_rows[2]
    check_against_restatement(M.room_acoustic_parameters(torch.from_numpy(row).cuda()[None], fs=44100), [row], fs=44100.0)


def test_status_rows_inside_a_batch_of_good_rows():
    n = 4096
    nan_row = noise_decay(n, 7)
    nan_row[1234] = np.nan
    impulse = np.zeros(n)
    impulse[2000] = -0.5
    rows = [RA.analytic_decay(0.05), np.zeros(n), noise_decay(n, 8), nan_row, impulse, RA.analytic_decay(0.1)]
    x = torch.from_numpy(np.stack(rows)).cuda()
    got = M.room_acoustic_parameters(x)
    check_against_restatement(got, rows)
    assert got.status.tolist() == [0, 1, 0, 1, 6, 0] and got.onset.tolist()[3:5] == [1234, 2000]
    for b in (0, 2, 5):          # a good row is bitwise what it is alone
        assert same_bits(tuple(t[b:b + 1] for t in got), M.room_acoustic_parameters(x[b:b + 1])), b


def test_float32_input_is_the_float64_call_on_the_widened_rows():
    x = torch.from_numpy(np.stack([noise_decay(5000, 20 + b) for b in range(4)])).float().cuda()
    assert same_bits(M.room_acoustic_parameters(x), M.room_acoustic_parameters(x.double()))
    assert same_bits(M.energy_decay_curve(x), M.energy_decay_curve(x.double()))
    check_against_restatement(M.room_acoustic_parameters(x), x.double().cpu().numpy())


def test_two_calls_give_the_same_bits():
    x = torch.from_numpy(np.stack([noise_decay(6400, 30 + b) for b in range(16)])).cuda()
    assert same_bits(M.room_acoustic_parameters(x), M.room_acoustic_parameters(x))
    assert same_bits(M.energy_decay_curve(x), M.energy_decay_curve(x))


def test_onset_at_either_end():
    n = 1500
    first = noise_decay(n, 40) * 0.3
    first[0] = 2.0
    last = noise_decay(n, 41)[::-1].copy() * 0.1
    last[n - 1] = -3.0
    rows = [first, last]
    got = M.room_acoustic_parameters(torch.from_numpy(np.stack(rows)).cuda())
    assert got.onset.tolist() == [0, n - 1]
    check_against_restatement(got, rows)
    assert got.status.tolist() == [0, RA.SHORT_RANGE | RA.NO_LATE_ENERGY]


def test_the_first_of_equal_maxima_is_the_onset():
    """Equal maxima in different waves (300, 1000), in one thread's samples (10, 266), and where the later one belongs to a
    lower thread (300 -> thread 44, 520 -> thread 8); the sign does not matter."""
    n = 2048
    rows = []
    for seed, (i, j) in enumerate(((300, 1000), (10, 266), (300, 520))):
        row = noise_decay(n, 50 + seed) * 0.05
        row[i], row[j] = 1.5, -1.5
        rows.append(row)
    got = M.room_acoustic_parameters(torch.from_numpy(np.stack(rows)).cuda())
    assert got.onset.tolist() == [300, 10, 300]
    check_against_restatement(got, rows)


def test_graph_replay_gives_the_eager_bits():
    a = torch.from_numpy(np.stack([noise_decay(6400, 60 + b) for b in range(4)])).cuda()
    b = torch.from_numpy(np.stack([noise_decay(6400, 70 + b, decades=4.0) for b in range(4)])).cuda()
    eager = M.room_acoustic_parameters(b)
    static = a.clone()
    M.room_acoustic_parameters(static)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):          # one stream, one launch
        out = M.room_acoustic_parameters(static)
    static.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager) and not same_bits(out, M.room_acoustic_parameters(a))


def test_scene_responses():
    """Eight rooms drawn from a SceneConfig: the device's parameters are the restatement's on the copied-back responses and
    every status is 0.  How far they lie from the nominal Sabine T60 is not asserted: tests/bench_room_acoustics.py records it."""
    g = torch.Generator(device="cuda").manual_seed(3)
    scenes = FE.sample_scenes(8, FE.SceneConfig(reverberation_time=(0.25, 0.5)), g)
    h = FE.scene_impulse_responses(scenes.source, scenes.receiver, scenes.room, reverberation_time=scenes.reverberation_time,
                                   nsample=6400)
    got = M.room_acoustic_parameters(h)
    check_against_restatement(got, h.cpu().numpy())
    assert got.status.tolist() == [0] * 8
    print("nominal T60", scenes.reverberation_time.tolist(), "t30", got.t30.tolist(), "edt", got.edt.tolist())
