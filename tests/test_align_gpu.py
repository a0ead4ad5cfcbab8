"""Frequency permutation alignment on the device (csrc/permutation_align.hip, acoustic_locating_vq_vae.separation.align_permutations /
permute_bins / permute_rows) against the float64 restatement of tests/helpers/align_ref.py, which tests/test_align_cpu.py pins.
u = 1.1e-16.

perm, changed, status:  equal to the restatement's EXACTLY, for every parity case and every iteration count 1..8.  The cases are
                        chosen (on the restatement alone) so that the gap between the best and the second-best permutation
                        score is >= 1e-9 in every bin and iteration, nine orders of magnitude above reordering noise.
score:                  |dev - ref| <= tol = max(32 e_ref, 4 (T + F) u), e_ref the largest difference of the scores of the
                        restatement run forward and with the frames and bins added in the opposite order: measured on the
                        reference, never on the device.  tol <= 1e-11 is asserted, so a float32 accumulation cannot hide.
permute_bins:           bit for bit against numpy indexing.
The cACGMM workflow:    the three agreements of the restatement's chain (0.574137, 0.771921, 0.830012) within the chain's own
                        tolerance, max(32 e_ref, 2 (T + F + 8 D) u) with e_ref the masks' forward / reversed difference."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import align_ref as R  # noqa: E402
import cacgmm_ref as C  # noqa: E402
from acoustic_locating_vq_vae import separation as SEP  # noqa: E402

U = R.U


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


def same_align(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def device_run(shape, iterations):
    """(perm, score, changed, status) of a parity shape on the device, downloaded; computed once."""
    B, K, F, T = shape[:4]
    out = SEP.align_permutations(dev(R.parity_case(shape).P), iterations)
    assert out.perm.shape == (B, F, K) and out.perm.dtype == torch.int32
    assert out.score.shape == (B, F) and out.score.dtype == torch.float64
    assert out.changed.shape == (B,) and out.changed.dtype == torch.int32
    assert out.status.shape == (B, F) and out.status.dtype == torch.int32
    return tuple(host(t) for t in out)


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("shape", R.PARITY, ids=R.IDS)
def test_parity(shape):
    tol = R.tolerance(shape)
    assert tol <= R.TOL_CAP                               # a condition on the case, not a measurement
    worst = 0.0
    for n in range(1, R.ITERATIONS + 1):
        perm, score, changed, status = device_run(shape, n)
        ref = R.reference(shape, n)
        assert np.array_equal(status, ref.status) and not status.any()
        assert np.array_equal(perm, ref.perm), (shape, n)
        assert np.array_equal(changed, ref.changed), (shape, n, changed, ref.changed)
        worst = max(worst, float(np.abs(score - ref.score).max()))
    print("%s: |score - ref| %.3g over 1..%d iterations, tol %.3g, measured / tol %.3g" % (shape[:4], worst, R.ITERATIONS, tol, worst / tol))
    assert worst <= tol


def test_ranks_views_and_the_default():
    shape = R.PARITY[5]
    B, K, F, T = shape[:4]
    c = R.parity_case(shape)
    p = dev(c.P)
    first = SEP.align_permutations(p)                                                       # 10 iterations
    assert same_align(first, SEP.align_permutations(p, 10))
    three = SEP.align_permutations(p[0], 10)                                                # ranks mirror the input
    assert three.perm.shape == (F, K) and three.score.shape == (F,) and three.changed.shape == () and three.status.shape == (F,)
    assert all(same_bits(a, b[0]) for a, b in zip(three, first))
    view = dev(c.P.transpose(0, 1, 3, 2)).transpose(2, 3)                                   # a strided (B, K, F, T) view
    assert not view.is_contiguous() and same_align(SEP.align_permutations(view, 10), first)
    assert same_bits(p, dev(c.P))                                                           # the profile is not written to
    start = dev(np.tile(np.arange(K, dtype=np.int32), (F, 1)))
    assert same_align(SEP.align_permutations(p[0], 10, perm0=start), three)                 # the identity is the default start


# --------------------------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("shape", [R.PARITY[3], R.PARITY[5], R.PARITY[7]], ids=[R.IDS[3], R.IDS[5], R.IDS[7]])
def test_continuation_has_the_same_bits(shape):
    p = dev(R.parity_case(shape).P)
    whole = SEP.align_permutations(p, 1 + 2)
    first = SEP.align_permutations(p, 1)
    assert int(first.changed.sum()) > 0
    assert same_align(whole, SEP.align_permutations(p, 2, perm0=first.perm))


def test_runs_repeat_and_items_do_not_see_each_other():
    shape = R.PARITY[3]
    B, K, F, T = shape[:4]
    c = R.parity_case(shape)
    other = R.case(1, K, F, T, 77)
    p = dev(np.concatenate([other.P, c.P[1:2], c.P[0:1]]))                                  # a batch of three
    for n in (1, 3):
        first, second = SEP.align_permutations(p, n), SEP.align_permutations(p, n)
        assert same_align(first, second)
        alone = SEP.align_permutations(p[1:2].contiguous(), n)
        assert all(same_bits(a[0], b[1]) for a, b in zip(alone, first))


def test_graph_capture_replays_the_eager_bits():
    shape = R.PARITY[5]
    p = dev(R.parity_case(shape).P)
    eager = SEP.align_permutations(p, 3)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = SEP.align_permutations(p, 3)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same_align(out, eager)


# ------------------------------------------------------------------------------------------------------------------ status
def test_status_bins():
    """A NaN bin, an infinite bin and two bins whose start is no permutation, beside good bins: status 1, the identity and a NaN
    score; the good bins have the perm of the restatement and the bits of a launch without the bad bins' data."""
    P, perm0, bad, keep = R.status_case()
    B, K, F, T = P.shape
    p, p0 = dev(P), dev(perm0)
    got = SEP.align_permutations(p, 3, perm0=p0)
    ref, rev = R.align(P, 3, perm0=perm0), R.align(P, 3, perm0=perm0, reverse=True)
    assert np.array_equal(host(got.status), ref.status) and int(got.status.sum()) == 4
    assert np.array_equal(host(got.perm), ref.perm) and np.array_equal(ref.perm, rev.perm)
    assert np.array_equal(host(got.changed), ref.changed)
    assert min(ref.margin, rev.margin) >= R.MARGIN_FLOOR
    score = host(got.score)
    assert np.array_equal(np.isnan(score), ref.status == 1)
    live = ref.status == 0
    tol = max(32 * np.abs(ref.score[live] - rev.score[live]).max(), 4 * (T + F) * U)
    assert np.abs(score[live] - ref.score[live]).max() <= tol <= R.TOL_CAP
    for b in bad:
        for f in bad[b]:
            assert host(got.perm[b, f]).tolist() == list(range(K))
        alone = SEP.align_permutations(p[b:b + 1][:, :, keep[b]].contiguous(), 3, perm0=p0[b:b + 1][:, keep[b]].contiguous())
        assert int(alone.status.sum()) == 0
        assert same_bits(alone.perm[0], got.perm[b, keep[b]]) and same_bits(alone.score[0], got.score[b, keep[b]])
        assert int(alone.changed[0]) == int(got.changed[b])


def test_constant_rows_and_more_bins_than_the_grid_holds():
    """A constant row has rn = 0 and produces no NaN; and every launch over bins caps its grid at 65536 workgroups and strides:
    70 000 two-frame bins pass the cap, and the last item has the bits it has alone, where no launch strides."""
    shape = R.PARITY[2]
    P = R.parity_case(shape).P.copy()
    P[0, 1, 3] = 0.25
    P[1, :, 5] = 0.0
    got, ref, rev = SEP.align_permutations(dev(P), 3), R.align(P, 3), R.align(P, 3, reverse=True)
    assert int(got.status.sum()) == 0 and bool(torch.isfinite(got.score).all())
    assert float(got.score[1, 5]) == 0.0 and host(got.perm[1, 5]).tolist() == list(range(shape[1]))
    keep = np.ones(P.shape[2], bool)
    keep[5] = False                                       # the bin of constants ties at 0: the restatement's margin says nothing there
    assert np.array_equal(ref.perm, rev.perm) and np.array_equal(host(got.perm)[:, keep], ref.perm[:, keep])
    g = torch.Generator(device="cuda").manual_seed(5)
    B, K, F, T = 2, 2, 35000, 2
    p = torch.rand((B, K, F, T), dtype=torch.float64, device="cuda", generator=g)
    p[B - 1, 0, F - 2, 1] = float("nan")                  # a status among the strided bins
    whole = SEP.align_permutations(p, 2)
    alone = SEP.align_permutations(p[B - 1:].contiguous(), 2)
    assert all(same_bits(a[0], w[B - 1]) for a, w in zip(alone, whole))
    assert int(whole.status[B - 1, F - 2]) == 1 and int((whole.status != 0).sum()) == 1
    moved = SEP.permute_bins(p, whole.perm)
    index = whole.perm.long().permute(0, 2, 1)[..., None].expand(B, K, F, T)
    assert same_bits(moved, torch.gather(p, 1, index))


# -------------------------------------------------------------------------------------------------------- applying a perm
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


@pytest.mark.parametrize("dtype", DTYPES, ids=[np.dtype(d).name for d in DTYPES])
@pytest.mark.parametrize("dims", [(2, 3, 9, 65), (1, 8, 6, 128)], ids=["2-3-9-65", "1-8-6-128"])
def test_permute_bins(dims, dtype):
    B, K, F, T = dims
    g = np.random.default_rng([7, B, K, F, T])
    x = g.standard_normal(dims)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * g.standard_normal(dims)
    x = x.astype(dtype)
    perm = np.stack([np.stack([g.permutation(K) for _ in range(F)]) for _ in range(B)]).astype(np.int32)
    xd, pd = dev(x), dev(perm)
    out = SEP.permute_bins(xd, pd)
    assert out.shape == xd.shape and out.dtype == xd.dtype and out.data_ptr() != xd.data_ptr()
    want = R.permute_bins(x, perm)
    assert np.array_equal(host(out).view(np.uint8), want.view(np.uint8))                    # bit for bit
    assert same_bits(xd, dev(x))                                                            # x is not written to
    inverse = dev(np.argsort(perm, axis=-1).astype(np.int32))
    assert same_bits(SEP.permute_bins(out, inverse), xd)                                    # the round trip
    assert same_bits(SEP.permute_bins(xd[0], pd[0]), out[0])                                # ranks mirror the input
    odd = perm.copy()
    odd[0, 1, 0] = K                                      # out of range: the bin passes through
    odd[B - 1, F - 1, K - 1] = -1
    got = host(SEP.permute_bins(xd, dev(odd)))
    assert np.array_equal(got.view(np.uint8), R.permute_bins(x, odd).view(np.uint8))
    assert np.array_equal(got[0, :, 1], x[0, :, 1]) and np.array_equal(got[B - 1, :, F - 1], x[B - 1, :, F - 1])
    view = dev(np.ascontiguousarray(x.transpose(0, 1, 3, 2))).transpose(2, 3)               # a strided view
    assert not view.is_contiguous() or T == 1
    assert same_bits(SEP.permute_bins(view, pd), out)


def test_permute_rows():
    g = np.random.default_rng(9)
    B, F, K, D = 2, 5, 3, 4
    perm = np.stack([np.stack([g.permutation(K) for _ in range(F)]) for _ in range(B)]).astype(np.int32)
    for shape in ((B, F, K, K), (B, F, K, D, D)):
        a = g.standard_normal(shape) + 1j * g.standard_normal(shape)
        got = SEP.permute_rows(dev(a), dev(perm))
        assert got.dtype == torch.complex128 and np.array_equal(host(got), R.permute_rows(a, perm))
        one = SEP.permute_rows(dev(a[0]), dev(perm[0]))                                     # ranks mirror the input
        assert np.array_equal(host(one), R.permute_rows(a, perm)[0])
    flat = g.standard_normal((B, F, K))
    assert np.array_equal(host(SEP.permute_rows(dev(flat), dev(perm))), R.permute_rows(flat, perm))


# ------------------------------------------------------------------------------------------------------- the cACGMM workflow
def test_alignment_repairs_a_cacgmm_started_per_bin():
    """The chain of tests/test_align_cpu.py on the device, through SEP.cacgmm, align_permutations and permute_bins: the perm
    is the restatement's, and the three agreements (0.574137, 0.771921, 0.830012) are the restatement's within the chain's
    own tolerance."""
    B, D, K, F, T, seed = R.CHAIN_CASE
    c = C.case(B, D, K, F, T, seed)
    ref = R.chain()
    tol = R.chain_tolerance()
    assert tol <= C.TOL_CAP
    x = dev(c.X)
    first = SEP.cacgmm(x, dev(ref.init), R.CHAIN_ITERATIONS)
    a = SEP.align_permutations(first.masks)
    assert int(a.status.sum()) == 0 and int(a.changed.sum()) == 0
    assert np.array_equal(host(a.perm), ref.perm)
    aligned = SEP.permute_bins(first.masks, a.perm)
    second = SEP.cacgmm(x, aligned, R.CHAIN_ITERATIONS, quadratic0=SEP.permute_bins(first.quadratic, a.perm))
    assert int(first.status.sum()) == 0 and int(second.status.sum()) == 0
    got = tuple(C.agreement(host(m)[0], c.oracle[0])[0] for m in (first.masks, aligned, second.masks))
    print("agreements %.6f %.6f %.6f, the restatement's %.6f %.6f %.6f, tol %.3g, largest difference %.3g"
          % (got + ref.agreements + (tol, max(abs(g - r) for g, r in zip(got, ref.agreements)))))
    assert np.abs(host(first.masks) - ref.first.masks).max() <= tol and np.abs(host(second.masks) - ref.second.masks).max() <= tol
    assert all(abs(g - r) <= tol for g, r in zip(got, ref.agreements))
    assert got[0] < got[1] < got[2]
