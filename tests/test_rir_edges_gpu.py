"""The room-response kernels (csrc/rir.hip) at their edges, against the float64 restatement of tests/helpers/rir_ref.py: the
window lengths the sample rate can give (2, 64, 352, 384, the cap 1024), images at exact integer distances (on and next to a
tile's fd_lo / fd_hi and on nsample), flat rooms, a receiver inside the source's first sample, rows around one tile, rigid and
dead walls, and the high-pass kernel's 4096-sample chunk edge.  The cases, their conditions and the bound are
tests/helpers/signal_edge_cases.py's, pinned on the host by tests/test_signal_edges_cpu.py.

Without the high-pass: |h_dev(t) - h_ref(t)| <= (K + N(t)) u A(t) at every sample, u = 2^-53, A(t) and N(t) the sum of |gain| and
the number of the images whose window covers t, and exactly 0 where N(t) = 0.  K_ref = 1.74 measured (recorded 2.0), K = 4 K_ref =
8.  With the high-pass: 1e-12 max |h| (the float64 recurrence is 9.3e-15 max |h| from its longdouble twin), against the
restatement and against the restatement's recurrence on the device's own unfiltered response.  Every case runs through
rir_generate and through scene_impulse_responses, whose rows must be the one-room launch's bit for bit.

Every case prints its largest measured / bound (``-s``); the worst per group on an MI355X is recorded in WORST below.  The
worst of all, 0.13, is a lone direct path (N = 1): 1.2 u A, the restatement's own distance from its twin there."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import rir_ref as R  # noqa: E402
import signal_edge_cases as E  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402

# the largest measured / bound of each group on an MI355X, with K_ref = 2.0 recorded and K = 8
WORST = {"sample rates": 0.131,            # fs250; 0.009 at the other four rates
         "short rows": 0.077,              # order 0: the direct path alone
         "high-pass chunk, unfiltered": 0.131, "high-pass chunk, of 1e-12 max |h|": 0.0115,
         "integer distances": 0.0123, "a lone exact image": 0.132,
         "image grid shapes": 0.049,       # the receiver 1 cm from the source
         "walls": 0.077}                   # dim 2, order 0: the direct path alone; 0.006 with every order


def bits(t):
    return t.contiguous().view(torch.int64)


def launch(case, hp):
    """(nsample, M) of the one-room launch; the scene launch's rows must carry the same bits."""
    one = FE.rir_generate(case.c, case.fs, case.r, case.s, case.L, beta=case.beta, nsample=case.nsample, order=case.order,
                          dim=case.dim, hp_filter=hp)
    M = len(case.r)
    assert one.shape == (case.nsample, M) and one.dtype == torch.float64 and one.is_cuda
    rows = lambda v: torch.tensor([v] * M, dtype=torch.float64).cuda()                      # noqa: E731
    scene = FE.scene_impulse_responses(rows(case.s), torch.tensor(case.r, dtype=torch.float64).cuda(), rows(case.L),
                                       beta=rows(case.beta), nsample=case.nsample, c=case.c, fs=case.fs, order=case.order,
                                       dim=case.dim, hp_filter=hp)
    assert scene.shape == (M, case.nsample) and torch.equal(bits(scene), bits(one.t())), "scene rows differ from the one-room launch"
    return one.cpu().numpy()


def run(name):
    """Every check of a case; returns (the largest measured / bound without the high-pass, with it or None)."""
    case = E.RIR_CASES[name]
    raw = launch(case, False)
    worst = max(E.check_rir(raw[:, m], E.rir_reference(name, m)) for m in range(len(case.r)))
    worst_hp = None
    if case.hp:
        got = launch(case, True)[:, 0]
        worst_hp = max(E.check_rir_highpassed(got, R.highpass(raw[:, 0], case.fs)),          # the recurrence alone
                       E.check_rir_highpassed(got, E.rir_reference_highpassed(name)))
    print("%s: K_ref %.3g K %.3g largest measured / bound %.3g%s"
          % (name, E.K_REF, E.K_DEVICE, worst, "" if worst_hp is None else "; high-pass %.3g of %.3g max |h|" % (worst_hp, E.HP_RTOL)))
    return worst, worst_hp


@pytest.mark.parametrize("name", ["fs250", "fs8000", "fs44100", "fs48000", "fs128000"])
def test_sample_rates(name):
    run(name)


@pytest.mark.parametrize("fs", E.RIR_BAD_RATES)
def test_rates_without_a_window_raise(fs):
    case = E.RIR_CASES["fs8000"]
    with pytest.raises(RuntimeError, match="tap window"):
        FE.rir_generate(case.c, fs, case.r, case.s, case.L, beta=case.beta, nsample=300, hp_filter=False)
    with pytest.raises(RuntimeError, match="tap window"):
        FE.scene_impulse_responses(torch.tensor([case.s], dtype=torch.float64).cuda(), case.r[0],
                                   torch.tensor([case.L], dtype=torch.float64).cuda(),
                                   beta=torch.tensor([case.beta], dtype=torch.float64).cuda(), nsample=300, c=case.c, fs=fs)


@pytest.mark.parametrize("order", [-1, 0])
@pytest.mark.parametrize("nsample", [1, 2, 63, 64, 65])
def test_short_rows(nsample, order):
    run("short%d_order%d" % (nsample, order))


@pytest.mark.parametrize("nsample", [4096, 4097, 8193])
def test_highpass_chunk_edge(nsample):
    run("hp%d" % nsample)


@pytest.mark.parametrize("name", ["exact700", "exact192"])
def test_images_at_integer_distances(name):
    run(name)


def test_a_lone_image_at_an_integer_distance_is_one_exact_tap():
    """beta = 0, order 0, the receiver 40 samples from the source: sample 40 carries the gain times exactly 1, and every
    other tap of the window is sin(pi 0) = 0 times something: exactly +-0."""
    case = E.RIR_CASES["exact_lone"]
    run("exact_lone")
    got = launch(case, False)[:, 0]
    want = R.direct_path(case.c, case.fs, case.r[0], case.s, case.nsample)
    assert got[40] == want[40] == 1.0 / (4.0 * np.pi * 0.625)
    assert not np.delete(got, 40).any()


@pytest.mark.parametrize("name", ["flat_z", "flat_x", "near"])
def test_image_grid_shapes(name):
    run(name)


@pytest.mark.parametrize("name", ["rigid_plus", "rigid_minus", "one_dead_wall", "dim2_order0", "order_all"])
def test_walls(name):
    run(name)


def test_an_order_no_image_reaches_is_every_order():
    run("order1000")
    a, b = (launch(E.RIR_CASES[name], False) for name in ("order1000", "order_all"))
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
