"""The separation scores on the device (csrc/separation_metrics.hip, acoustic_locating_vq_vae.speech_metrics, separation.reorder)
against ``speech_metrics.si_sdr`` -- bit for bit -- and the float64 restatement of tests/helpers/separation_metrics_ref.py,
which tests/test_separation_metrics_cpu.py pins together with the conditions on the cases.  u = 1.1e-16.

pairwise_si_sdr:    the bits of si_sdr on the K J expanded pairs, NaN included.
assign:             perm equal to, and total the bits of, the restatement's: the same k-rising sum of the same doubles.
pit_si_sdr:         the scramble of the case; value gathered from the table bit for bit.
si_bss_eval:        sdr the bits of the table entry; sir and sar within tol = 32 e_ref + 8.7 n u dB of the restatement on the
                    promoted input, e_ref the largest |forward - reversed| in dB of the restatement on that case: the tolerance
                    is measured on the reference, never on the device.  32: the reason iva_ref.w_tolerance gives.  tol <= 1e-9
                    dB is asserted (a condition on the case), so a float32 accumulation, at about 4e-7 dB, cannot hide."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import iva_ref as IR  # noqa: E402
import ilrma_ref as LR  # noqa: E402
import parity_checks  # noqa: E402
import separation_metrics_ref as R  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import separation as SEP  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as SM  # noqa: E402

DTYPES = [np.float64, np.float32]
DIDS = ["float64", "float32"]
SCORED = R.SHAPES[1:]                    # (1, 1, 2) has no SIR / SAR to compare: two centred samples are always collinear
SCORED_IDS = R.IDS[1:]


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()          # a copy: the shared cases are read-only


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    """Two tensors equal bit for bit, NaN included."""
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {torch.float64: torch.int64, torch.float32: torch.int32}.get(a.dtype)
    return torch.equal(a.view(view), b.view(view)) if view else torch.equal(a, b)


def same_all(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def same_doubles(got, want):
    """Two float64 numpy arrays with NaN in the same places and the same bits elsewhere."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) \
        and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


def sources(shape, dtype):
    c = R.case(shape)
    return dev(c.references.astype(dtype)), dev(c.estimates.astype(dtype))


def gathered(table, perm):
    return torch.gather(table, 2, perm.long()[:, :, None])[:, :, 0]


# ------------------------------------------------------------------------------------------------------------ the pairs' table
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.IDS)
def test_pairwise_has_the_bits_of_si_sdr(shape, dtype):
    """Item 0 as the case has it; item 1 with its last reference and its first estimate zeroed; item 2 with its last estimate
    -4 times its first reference, exact in every sum."""
    K, J, n = shape
    c = R.case(shape)
    s, e = c.references.astype(dtype), c.estimates.astype(dtype)
    s[1, K - 1] = 0
    e[1, 0] = 0
    e[2, J - 1] = -4 * s[2, 0]
    s, e = dev(s), dev(e)
    table = SM.pairwise_si_sdr(s, e)
    assert table.shape == (R.ITEMS, K, J) and table.dtype == torch.float64
    pairs = SM.si_sdr(s[:, :, None].expand(-1, K, J, n).reshape(-1, n), e[:, None].expand(-1, K, J, n).reshape(-1, n))
    assert same_bits(table, pairs.view(R.ITEMS, K, J))
    t = host(table)
    assert np.isnan(t[1, K - 1]).all() and t[2, 0, J - 1] == np.inf
    if n > 2:                                             # two centred samples are always collinear: +inf or near it
        assert np.isfinite(t[0]).all()
    if K > 1:
        assert np.isfinite(t[1, 0, 1:]).all()


# ------------------------------------------------------------------------------------------------------------ the assignment
def check_assign(table, maximize):
    got = SM.assign(dev(table), maximize=maximize)
    B, K, _ = table.shape
    assert got.perm.shape == (B, K) and got.perm.dtype == torch.int32 and got.status.dtype == torch.int32
    assert got.total.shape == (B,) and got.total.dtype == torch.float64 and got.status.shape == (B,)
    return parity_checks.check_assign("assign", (host(got.perm), host(got.total), host(got.status)), table, maximize)


@pytest.mark.parametrize("maximize", [True, False], ids=["max", "min"])
@pytest.mark.parametrize("K,J", [(1, 1), (1, 8), (2, 3), (3, 8), (5, 6), (8, 8)])
def test_assign_matches_the_restatement(K, J, maximize):
    g = np.random.default_rng([11, K, J])
    check_assign(g.standard_normal((4, K, J)) * 20.0, maximize)
    want = check_assign(g.integers(0, 3, size=(4, K, J)).astype(np.float64), maximize)     # exact sums: ties
    assert not want.status.any()


def test_assign_with_nan_and_infinite_entries():
    g = np.random.default_rng(12)
    nan, inf = np.nan, np.inf
    table = g.standard_normal((7, 3, 4))
    table[0, 0, 0] = nan
    table[1, :, :3] = nan                                  # one valid column for three rows: every score is NaN
    table[2] = nan
    table[3, 1, 2], table[3, 2, 1] = inf, -inf             # inf - inf where both are taken
    table[4, 0] = inf
    table[5, 2] = -inf
    table[6] = np.where(g.random((3, 4)) < 0.4, nan, table[6])
    for maximize in (True, False):
        want = check_assign(table, maximize)
        assert want.status[1] == want.status[2] == 1 and want.status[0] == want.status[3] == 0
        assert want.perm[2].tolist() == [0, 1, 2] and np.isnan(want.total[2])
    assert R.assign(table, True).total[4] == inf and R.assign(table, False).total[5] == -inf
    square = np.full((2, 8, 8), nan)
    square[1] = np.where(np.eye(8)[::-1] > 0, 1.0, nan)    # one injection without a NaN, the last in rank
    want = check_assign(square, True)
    assert want.status.tolist() == [1, 0] and want.perm[1].tolist() == list(range(7, -1, -1)) and want.total[1] == 8.0


def test_assign_ranks_and_views():
    g = np.random.default_rng(13)
    table = g.standard_normal((3, 4, 3))                   # (B, J, K): its transpose is a strided (B, K, J) view
    view = dev(table).transpose(1, 2)
    assert not view.is_contiguous()
    got, whole = SM.assign(view), SM.assign(view.contiguous())
    assert same_all(got, whole) and np.array_equal(host(got.perm), R.assign(table.transpose(0, 2, 1)).perm)
    one = SM.assign(view[1])                               # (K, J): the ranks mirror the input
    assert one.perm.shape == (3,) and one.total.shape == () and one.status.shape == ()
    assert same_all(one, [v[1] for v in whole])


# -------------------------------------------------------------------------------------------------- permutation-invariant
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.IDS)
def test_pit_recovers_the_scramble(shape, dtype):
    K, J, n = shape
    c = R.case(shape)
    s, e = sources(shape, dtype)
    table = SM.pairwise_si_sdr(s, e)
    pit = SM.pit_si_sdr(s, e)
    assert pit.value.shape == pit.perm.shape == (R.ITEMS, K) and pit.status.shape == (R.ITEMS,)
    assert pit.value.dtype == torch.float64 and pit.perm.dtype == pit.status.dtype == torch.int32
    assert np.array_equal(host(pit.perm), c.scramble) and not host(pit.status).any()
    assert same_bits(pit.value, gathered(table, pit.perm))
    t = host(table)
    assert same_doubles(host(pit.value), np.take_along_axis(t, c.scramble[:, :, None].astype(np.int64), 2)[:, :, 0])
    mix = dev(c.mixture.astype(dtype))
    gain = SM.si_sdr_improvement(s, e, mix)
    before = SM.pairwise_si_sdr(s, mix[:, None].contiguous())
    assert before.shape == (R.ITEMS, K, 1) and same_bits(before[:, :, 0], SM.si_sdr(s.reshape(-1, n), mix.repeat_interleave(K, 0)).view(-1, K))
    assert gain.shape == (R.ITEMS, K) and same_doubles(host(gain), host(pit.value) - host(before)[:, :, 0])
    if shape != R.SHAPES[0]:
        print("%s %s: SI-SDR %.2f..%.2f dB, improvement %.2f..%.2f dB"
              % (shape, np.dtype(dtype).name, float(pit.value.min()), float(pit.value.max()), float(gain.min()), float(gain.max())))


# ------------------------------------------------------------------------------------------------------ SDR, SIR and SAR
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", SCORED, ids=SCORED_IDS)
def test_si_bss_eval_matches_the_restatement(shape, dtype):
    K, J, n = shape
    single = dtype == np.float32
    s, e = sources(shape, dtype)
    got = SM.si_bss_eval(s, e)
    for v in (got.sdr, got.sir, got.sar):
        assert v.shape == (R.ITEMS, K) and v.dtype == torch.float64
    assert got.perm.shape == (R.ITEMS, K) and got.perm.dtype == torch.int32 and got.status.shape == (R.ITEMS,)
    ref = R.reference(shape, single)
    assert np.array_equal(host(got.perm), ref.perm) and not host(got.status).any() and not ref.status.any()
    assert same_bits(got.sdr, gathered(SM.pairwise_si_sdr(s, e), got.perm))
    assert same_all(got, SM.si_bss_eval(s, e, got.perm))                                       # the permutation given
    tol = R.tolerance(shape, single)
    worst = []
    for name, g, w in (("sir", host(got.sir), ref.sir), ("sar", host(got.sar), ref.sar), ("sdr", host(got.sdr), ref.sdr)):
        err = np.abs(g - w).max()
        print("%s %s: |%s - ref| %.3g dB, tol %.3g dB, measured / tol %.3g" % (shape, np.dtype(dtype).name, name, err, tol, err / tol))
        worst.append((name, err))
    assert tol <= R.TOL_CAP, tol                          # a condition on the case, not a measurement
    for name, err in worst:
        assert err <= tol, (name, err, tol)


def test_one_reference_has_no_interference():
    for shape in (R.SHAPES[0], (1, 3, 300)):
        g = np.random.default_rng(shape)
        s, e = dev(g.standard_normal((2, 1, shape[2]))), dev(g.standard_normal((2, shape[1], shape[2])))
        got = SM.si_bss_eval(s, e)
        assert not host(got.status).any() and bool((got.sir == np.inf).all())
        assert same_bits(got.sdr, SM.pit_si_sdr(s, e).value)
    s, e = sources(R.SHAPES[0], np.float32)
    got = SM.si_bss_eval(s, e)
    assert not host(got.status).any() and bool((got.sir == np.inf).all()) and same_bits(got.sdr, SM.pit_si_sdr(s, e).value)


def test_si_bss_eval_status_rows():
    """Five items in one launch: as the case has it; two identical references; a reference of zeros; a perm row that repeats a
    column; an infinite sample in a selected estimate.  The good item has the bits it has alone."""
    shape = R.SHAPES[3]
    K, J, n = shape
    c = R.case(shape)
    pick = [0, 1, 2, 0, 1]
    s, e = c.references[pick].copy(), c.estimates[pick].copy()
    perm = c.scramble[pick].copy()
    s[1, 2] = s[1, 0]
    s[2, 1] = 0.0
    perm[3, 1] = perm[3, 0]
    e[4, perm[4, 2], 77] = np.inf
    for dtype in DTYPES:
        sd, ed, pd = dev(s.astype(dtype)), dev(e.astype(dtype)), dev(perm)
        got = SM.si_bss_eval(sd, ed, pd)
        want = R.si_bss_eval(R.promoted(s, dtype == np.float32), R.promoted(e, dtype == np.float32), perm)
        assert host(got.status).tolist() == want.status.tolist() == [0, R.BAD_SOLVE, R.BAD_INPUT, R.BAD_PERM, R.BAD_INPUT]
        assert bool(torch.isnan(got.sir[1:]).all()) and bool(torch.isnan(got.sar[1:]).all()) and bool(torch.isnan(got.sdr[3]).all())
        table = SM.pairwise_si_sdr(sd, ed)
        keep = [0, 1, 2, 4]
        assert same_bits(got.sdr[keep], gathered(table, pd)[keep])                             # sdr as the table gives it
        assert bool(torch.isfinite(got.sdr[1]).all()) and np.array_equal(np.isnan(host(got.sdr[2])), [False, True, False])
        alone = SM.si_bss_eval(sd[:1].contiguous(), ed[:1].contiguous(), pd[:1].contiguous())
        assert same_all([v[0] for v in alone], [v[0] for v in got]) and bool(torch.isfinite(got.sir[0]).all())
        for bad in (-1, J):                               # out of range on either side
            pd2 = pd.clone()
            pd2[3, 1] = bad
            again = SM.si_bss_eval(sd, ed, pd2)
            assert host(again.status).tolist() == host(got.status).tolist()
            assert same_bits(again.sdr, got.sdr) and same_bits(again.sir, got.sir) and same_bits(again.sar, got.sar)


# --------------------------------------------------------------------------------------------------------- reproducibility
def test_runs_repeat_items_do_not_see_each_other_and_ranks_mirror():
    shape = R.SHAPES[4]
    K, J, n = shape
    for dtype in DTYPES:
        s, e = sources(shape, dtype)
        first = (SM.pairwise_si_sdr(s, e),) + tuple(SM.pit_si_sdr(s, e)) + tuple(SM.si_bss_eval(s, e))
        second = (SM.pairwise_si_sdr(s, e),) + tuple(SM.pit_si_sdr(s, e)) + tuple(SM.si_bss_eval(s, e))
        assert same_all(first, second)
        s1, e1 = s[1:2].contiguous(), e[1:2].contiguous()
        alone = (SM.pairwise_si_sdr(s1, e1),) + tuple(SM.pit_si_sdr(s1, e1)) + tuple(SM.si_bss_eval(s1, e1))
        assert all(same_bits(a[0], b[1]) for a, b in zip(alone, first))
        flat = (SM.pairwise_si_sdr(s[1], e[1]),) + tuple(SM.pit_si_sdr(s[1], e[1])) + tuple(SM.si_bss_eval(s[1], e[1]))
        assert flat[0].shape == (K, J) and flat[1].shape == (K,) and flat[3].shape == () and flat[4].shape == (K,) and flat[8].shape == ()
        assert all(same_bits(a, b[1]) for a, b in zip(flat, first))
        mix = dev(R.case(shape).mixture.astype(dtype))
        assert same_bits(SM.si_sdr_improvement(s[1], e[1], mix[1]), SM.si_sdr_improvement(s, e, mix)[1])
        assert same_all(SM.si_bss_eval(s[1], e[1], first[2][1]), [v[1] for v in first[4:]])


def test_graph_capture_replays_the_eager_bits():
    s, e = sources(R.SHAPES[4], np.float32)
    eager = tuple(SM.pit_si_sdr(s, e)) + tuple(SM.si_bss_eval(s, e))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tuple(SM.pit_si_sdr(s, e)) + tuple(SM.si_bss_eval(s, e))
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same_all(out, eager)


# --------------------------------------------------------------------------------------------------------------- the chain
def test_reorder():
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((3, 4, 5, 6), device="cuda", generator=g)
    perm = torch.tensor([[2, 0, 3], [1, 3, 0], [0, 1, 2]], dtype=torch.int32, device="cuda")
    out = SEP.reorder(x, perm)
    assert out.shape == (3, 3, 5, 6)
    for b in range(3):
        for k in range(3):
            assert same_bits(out[b, k], x[b, int(perm[b, k])])
    assert same_bits(SEP.reorder(x[1], perm[1].long()), out[1])
    z = torch.complex(x, x.flip(1))
    assert torch.equal(SEP.reorder(z[:, :, 0, 0], perm), torch.complex(out[:, :, 0, 0], SEP.reorder(x.flip(1), perm)[:, :, 0, 0]))


def test_separate_score_and_reorder_on_the_device():
    """ILRMA's two-source case through istft, pit_si_sdr against the istft of the images, and reorder: the permutation is the
    one iva_ref.best_permutation_si_sdr finds on the downloaded waveforms.  The improvement is printed, not asserted: nobody
    has measured it in the waveform domain."""
    shape = LR.SEPARATION[0]
    B, D, F, T = shape[:4]
    n_fft, hop = 2 * (F - 1), F - 1
    length = hop * (T - 1)
    c = LR.parity_case(shape)
    x = dev(c.X)
    sep = SEP.ilrma(x, *(dev(a) for a in LR.parity_start(shape)), iterations=shape[5])
    assert not host(sep.status).any()
    waves = FE.istft(sep.spec.reshape(B * D, F, T), n_fft, hop, length).view(B, D, length)
    clean = FE.istft(dev(c.images).reshape(B * D, F, T), n_fft, hop, length).view(B, D, length)
    mix = FE.istft(dev(c.mix), n_fft, hop, length)
    pit = SM.pit_si_sdr(clean, waves)
    assert not host(pit.status).any()
    w, s = host(waves), host(clean)
    for b in range(B):
        value, perm = IR.best_permutation_si_sdr(s[b], w[b])
        assert host(pit.perm[b]).tolist() == list(perm)
        print("item %d: SI-SDR on the device %s dB, on the host (means kept) %s dB" % (b, np.round(host(pit.value[b]), 3), np.round(value, 3)))
    ordered = SEP.reorder(sep.spec, pit.perm)
    assert ordered.shape == sep.spec.shape
    for b in range(B):
        for k in range(D):
            assert same_bits(torch.view_as_real(ordered[b, k]), torch.view_as_real(sep.spec[b, int(pit.perm[b, k])]))
    again = SM.pit_si_sdr(clean, FE.istft(ordered.reshape(B * D, F, T), n_fft, hop, length).view(B, D, length))
    assert host(again.perm).tolist() == [list(range(D))] * B and same_bits(again.value, pit.value)
    split = SM.si_bss_eval(clean, waves, pit.perm)
    print("ILRMA %s in the waveform domain: SI-SDR %s dB, improvement %s dB, SIR %s dB, SAR %s dB"
          % (shape[:5], np.round(host(pit.value), 2).tolist(), np.round(host(SM.si_sdr_improvement(clean, waves, mix)), 2).tolist(),
             np.round(host(split.sir), 2).tolist(), np.round(host(split.sar), 2).tolist()))
