"""The separation scores, the parts that need no GPU: the float64 restatement (tests/helpers/separation_metrics_ref.py) on
inputs whose answer is known, the conditions on the seeded cases that tests/test_separation_metrics_gpu.py relies on, the
host-side argument rules of acoustic_locating_vq_vae.speech_metrics and separation.reorder, and the argument checks of the C
entry points of csrc/separation_metrics.hip."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import separation_metrics_ref as R  # noqa: E402
from acoustic_locating_vq_vae import separation as SEP  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as M  # noqa: E402

SCORED = R.SHAPES[1:]                    # (1, 1, 2) has no SIR / SAR to speak of: two centred samples are always collinear
SCORED_IDS = R.IDS[1:]


# ------------------------------------------------------------------------------------------------------------- assignment
@pytest.mark.parametrize("K,J", [(1, 1), (1, 8), (2, 2), (2, 3), (3, 3), (3, 8), (4, 5), (6, 6), (8, 8)])
def test_assign_is_the_first_best_of_itertools(K, J):
    """Integer tables with entries in {0, 1, 2}: the sums are exact and ties abound.  ``max`` and ``min`` return the first
    extremum, and itertools.permutations(range(J), K) runs in lexicographic order."""
    g = np.random.default_rng([7, K, J])
    for _ in range(2 if K == 8 else 6):
        table = g.integers(0, 3, size=(K, J)).astype(np.float64)
        score = lambda pi: sum(table[k, pi[k]] for k in range(K))  # noqa: E731
        for maximize, pick in ((True, max), (False, min)):
            want = pick(itertools.permutations(range(J), K), key=score)
            perm, total, status = R.assign_one(table, maximize)
            assert tuple(perm) == want and total == score(want) and status == 0 and perm.dtype == np.int32


def test_injections_run_in_lexicographic_order():
    assert list(R.injections(2, 3)) == list(itertools.permutations(range(3), 2))
    assert list(R.injections(3, 3)) == sorted(itertools.permutations(range(3)))
    assert sum(1 for _ in R.injections(8, 8)) == 40320


def test_assign_skips_nan_scores():
    nan, inf = np.nan, np.inf
    perm, total, status = R.assign_one(np.array([[nan, 1.0], [2.0, 5.0]]))
    assert tuple(perm) == (1, 0) and total == 3.0 and status == 0
    perm, total, status = R.assign_one(np.array([[inf, 1.0], [2.0, -inf]]))            # inf - inf is NaN: skipped
    assert tuple(perm) == (1, 0) and total == 3.0 and status == 0
    perm, total, status = R.assign_one(np.array([[inf, 1.0], [2.0, inf]]))
    assert tuple(perm) == (0, 1) and total == inf and status == 0
    perm, total, status = R.assign_one(np.full((2, 3), nan))
    assert tuple(perm) == (0, 1) and np.isnan(total) and status == 1
    a = R.assign(np.stack([np.eye(3), np.full((3, 3), nan), 1.0 - np.eye(3)]))
    assert a.perm.tolist() == [[0, 1, 2], [0, 1, 2], [1, 2, 0]] and a.status.tolist() == [0, 1, 0]
    assert a.total[0] == 3.0 and np.isnan(a.total[1]) and a.total[2] == 3.0


# ------------------------------------------------------------------------------------------------------- SDR, SIR and SAR
@pytest.mark.parametrize("shape", SCORED, ids=SCORED_IDS)
def test_the_three_parts_add_up_to_the_estimate(shape):
    """target, interf and artif are orthogonal where c solves G c = g exactly, so |target|^2 + |interf|^2 + |artif|^2 = |e|^2
    up to the solve's error, cond_2(G) K u relative, and the n roundings of each sum: 8 n u cond_2(G) covers both."""
    r = R.reference(shape)
    assert not r.status.any() and r.cond.max() <= 10.0
    en = r.energies
    gap = np.abs(en[..., 0] + en[..., 2] + en[..., 3] - en[..., 5]) / en[..., 5]
    bound = 8 * shape[2] * R.U * r.cond.max()
    print("%s: largest relative gap %.3g, bound %.3g" % (shape, gap.max(), bound))
    assert (gap <= bound).all()


def test_one_reference_has_no_interference():
    for shape in ((1, 1, 2), (1, 1, 300), (1, 3, 300)):
        g = np.random.default_rng(shape)
        s, e = g.standard_normal((2, 1, shape[2])), g.standard_normal((2, shape[1], shape[2]))
        r = R.si_bss_eval(s, e)
        assert not r.status.any() and (r.sir == np.inf).all()
        assert np.array_equal(r.sdr, R.pit_si_sdr(s, e).value)


def test_an_exact_mix_has_no_artefacts():
    g = np.random.default_rng(250)
    s = g.standard_normal((2, 3, 1000))
    A = np.eye(3) + 0.2 * g.standard_normal((2, 3, 3))
    r = R.si_bss_eval(s, np.einsum("bjk,bkn->bjn", A, s) + 0.3)
    print("exact mix: sar %s dB, sir %s dB" % (np.round(r.sar, 1), np.round(r.sir, 1)))
    assert not r.status.any() and (r.sar > 250.0).all() and (r.sir < 40.0).all()


def test_status_rows_of_the_restatement():
    g = np.random.default_rng(3)
    s, e = g.standard_normal((3, 2, 400)), g.standard_normal((3, 2, 400))
    s[1, 1] = s[1, 0]                                     # identical references: a pivot of 0
    s[2, 0] = 4.0                                         # a reference without centred energy
    perm = np.array([[0, 1], [1, 0], [0, 1]], dtype=np.int32)
    r = R.si_bss_eval(s, e, perm)
    assert r.status.tolist() == [0, R.BAD_SOLVE, R.BAD_INPUT]
    assert np.isfinite(r.sir[0]).all() and np.isnan(r.sir[1:]).all() and np.isnan(r.sar[1:]).all()
    table = R.pairwise_si_sdr(s, e)
    assert np.array_equal(r.sdr, np.take_along_axis(table, perm[:, :, None].astype(np.int64), 2)[:, :, 0], equal_nan=True)
    assert np.isnan(r.sdr[2, 0]) and np.isfinite(r.sdr[2, 1]) and np.isfinite(r.sdr[1]).all()
    bad = e.copy()
    bad[0, 1, 7] = np.inf
    assert R.si_bss_eval(s, bad, perm).status.tolist() == [R.BAD_INPUT, R.BAD_SOLVE, R.BAD_INPUT]
    for row in ([0, 0], [0, 2], [-1, 1]):
        r = R.si_bss_eval(s, e, np.array([[0, 1], row, [1, 0]], dtype=np.int32))
        assert r.status.tolist() == [0, R.BAD_PERM, R.BAD_INPUT] and np.isnan(r.sdr[1]).all() and np.isfinite(r.sdr[0]).all()


# ------------------------------------------------------------------------------------- conditions on the GPU tests' cases
@pytest.mark.parametrize("single", [False, True], ids=["float64", "float32"])
@pytest.mark.parametrize("shape", SCORED, ids=SCORED_IDS)
def test_conditions_on_the_cases(shape, single):
    """What tests/test_separation_metrics_gpu.py relies on, met by the restatement alone: it recovers the scramble, G is well
    conditioned, every value is a moderate number of dB, and the tolerance of the SIR / SAR comparison is far below what a
    float32 accumulation would need (about 4e-7 dB)."""
    c, r = R.case(shape), R.reference(shape, single)
    assert np.array_equal(r.perm, c.scramble) and not r.status.any()
    assert r.cond.max() <= R.COND_CAP
    for v in (r.sdr, r.sir, r.sar):
        assert (np.abs(v) <= R.VALUE_CAP).all()
    gain = R.si_sdr_improvement(R.promoted(c.references, single), R.promoted(c.estimates, single), R.promoted(c.mixture, single))
    assert (np.abs(gain) <= R.VALUE_CAP).all()
    tol = R.tolerance(shape, single)
    print("%s %s: cond_2(G) %.3g, sdr %.1f..%.1f dB, e_ref %.3g dB, tol %.3g dB"
          % (shape, "float32" if single else "float64", r.cond.max(), r.sdr.min(), r.sdr.max(), R.e_ref(shape, single), tol))
    assert tol <= R.TOL_CAP


def test_the_smallest_case_is_collinear():
    r = R.reference((1, 1, 2))
    assert not r.status.any() and (r.sir == np.inf).all() and (r.sdr > 250.0).all()


# ------------------------------------------------------------------------------------------------------------ the host side
def test_host_side_rejections():
    s, e = torch.zeros(2, 3, 100, dtype=torch.float64), torch.zeros(2, 4, 100, dtype=torch.float64)
    mix = torch.zeros(2, 100, dtype=torch.float64)
    calls = (M.pairwise_si_sdr, M.pit_si_sdr, M.si_bss_eval, lambda a, b: M.si_sdr_improvement(a, b, mix))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(s, e)
        for a, b in ((s, e[:, :, :99]), (s, e[:1]), (s, e.float()), (s.half(), e.half()), (s[0], e), (s, e[0]), (s[None], e[None]),
                     (s[0, 0], e[0, 0]), (s.numpy(), e.numpy()), (s[:, :, :1], e[:, :, :1]), (s[:0], e[:0]), (s[:, :0], e),
                     (s, e[:, :0]), (torch.zeros(2, 9, 100, dtype=torch.float64), torch.zeros(2, 9, 100, dtype=torch.float64)),
                     (s.long(), e.long())):
            with pytest.raises(ValueError):
                call(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.pairwise_si_sdr(e, s)                           # more references than estimates: fine for the table alone ...
    for call in calls[1:]:                                # ... but not where every reference takes an estimate of its own
        with pytest.raises(ValueError, match="at least as many"):
            call(e, s)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.pit_si_sdr(s[0].float(), e[0].float())
    for perm in (torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                 [[0, 1, 2]] * 2, torch.zeros(2, 3)):
        with pytest.raises(ValueError, match="perm"):
            M.si_bss_eval(s, e, perm)
    with pytest.raises(ValueError, match="perm"):
        M.si_bss_eval(s[0], e[0], torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.si_bss_eval(s, e, torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.si_bss_eval(s[0], e[0], torch.zeros(3, dtype=torch.int32))
    for bad in (mix[0], mix.float(), mix[:, :99], mix[None], mix.numpy(), None):
        with pytest.raises(ValueError, match="mixture"):
            M.si_sdr_improvement(s, e, bad)
    with pytest.raises(ValueError, match="mixture"):
        M.si_sdr_improvement(s[0], e[0], mix)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.si_sdr_improvement(s[0], e[0], mix[0])

    t = torch.zeros(2, 3, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.assign(t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.assign(t[0], maximize=False)
    for bad in (t.float(), t[0, 0], t[None], t.transpose(1, 2), t.numpy(), t[:0], t[:, :0], torch.zeros(1, 9, 9, dtype=torch.float64),
                torch.zeros(1, 2, 9, dtype=torch.float64)):
        with pytest.raises(ValueError):
            M.assign(bad)
    for maximize in (1, 0, None, "max"):
        with pytest.raises(ValueError, match="maximize"):
            M.assign(t, maximize=maximize)

    x, perm = torch.zeros(2, 4, 5, 6), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        SEP.reorder(x, perm)
    with pytest.raises(RuntimeError, match="GPU"):
        SEP.reorder(x[0], perm[0].long())
    for a, p in ((x, perm.float()), (x, perm[None]), (x, [[0, 1, 2]] * 2), (x.numpy(), perm), (x[:1], perm), (x[0, 0, 0], perm),
                 (x, perm[:, :0]), (x[:, :0], perm), (x, torch.tensor(1))):
        with pytest.raises(ValueError):
            SEP.reorder(a, p)


def test_entry_points_check_their_arguments_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native as N
    lib = N.lib()
    p = 4096            # never dereferenced: every call below is rejected first

    def rejected(name, good, bads):
        fn = getattr(lib, name)
        for pos, bad in bads:
            args = list(good)
            args[pos] = bad
            assert fn(*args, None) == -1, (name, pos, bad)
            assert lib.alvq_last_error().startswith(name.encode()), (name, pos, bad, lib.alvq_last_error())

    for sfx in ("f32", "f64"):
        rejected("alvq_pairwise_si_sdr_" + sfx, [p, p, p, 1, 2, 3, 100],
                 [(0, None), (1, None), (2, None), (3, 0), (3, 65536), (4, 0), (4, 9), (5, 0), (5, 9), (6, 1), (6, (1 << 24) + 1)])
        rejected("alvq_si_bss_eval_" + sfx, [p, p, p, p, p, p, p, 1, 2, 3, 100],
                 [(i, None) for i in range(7)] + [(7, 0), (7, 65536), (8, 0), (8, 9), (8, 4), (9, 0), (9, 9), (9, 1), (10, 1),
                                                  (10, (1 << 24) + 1)])
    rejected("alvq_assign_f64", [p, p, p, p, 1, 2, 3, 1],
             [(0, None), (1, None), (2, None), (3, None), (4, 0), (4, 65536), (5, 0), (5, 4), (6, 9), (6, 1), (7, 2), (7, -1)])
