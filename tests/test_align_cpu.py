"""Frequency permutation alignment without a GPU: the pins on the numpy restatement tests/helpers/align_ref.py, the conditions its
seeded cases meet (the inputs are chosen so that the restatement alone meets them: they are no measurements of
csrc/permutation_align.hip), the argument rules of acoustic_locating_vq_vae.separation.align_permutations / permute_bins /
permute_rows on CPU tensors, and the three entry points of the C ABI.  u = 1.1e-16.

e_ref, the largest |score_forward - score_reversed| over the iteration counts 1..8, per parity case (B-K-F-T), as
test_parity_cases_meet_their_conditions prints it:
    1-1-1-2 0,  2-2-5-16 4.4e-16,  2-3-17-64 8.9e-16,  2-3-9-65 8.9e-16,  1-2-3-130 2.2e-16,  2-4-24-100 1.3e-15,
    1-5-12-128 8.9e-16,  1-8-6-128 1.8e-15,  3-2-33-40 6.7e-16,  1-2-4-257 4.4e-16
and the smallest margin between the best and the second-best permutation score is 0.0085 (2-4-24-100)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import align_ref as R  # noqa: E402
import cacgmm_ref as C  # noqa: E402

U = R.U
NEW_EXPORTS = ("alvq_align_workspace_bytes", "alvq_align_permutations_f64", "alvq_permute_bins")
E_REF_WRITTEN = {"1-1-1-2": 0.0, "2-2-5-16": 4.4e-16, "2-3-17-64": 8.9e-16, "2-3-9-65": 8.9e-16, "1-2-3-130": 2.2e-16,
                 "2-4-24-100": 1.3e-15, "1-5-12-128": 8.9e-16, "1-8-6-128": 1.8e-15, "3-2-33-40": 6.7e-16, "1-2-4-257": 4.4e-16}


def bits(a):
    """The bits of a float64 array, so that a NaN equals itself."""
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b):
    """Two Align results equal bit for bit in perm, score, changed and status."""
    return (np.array_equal(a.perm, b.perm) and np.array_equal(bits(a.score), bits(b.score)) and np.array_equal(a.changed, b.changed)
            and np.array_equal(a.status, b.status))


@pytest.fixture(scope="module")
def SEP():
    from acoustic_locating_vq_vae import separation
    return separation


# ------------------------------------------------------------------------------------------------ conditions on the cases
@pytest.mark.parametrize("shape", R.PARITY, ids=R.IDS)
def test_parity_cases_meet_their_conditions(shape):
    """After 8 iterations every case with K >= 2 is at a fixed point and its scramble is undone up to one common order; the
    margin is >= 1e-9 forward and reversed and both orders of summation give the same perm after every iteration count: that is
    what lets the device test compare permutations exactly."""
    B, K, F, T = shape[:4]
    c = R.parity_case(shape)
    margin = np.inf
    for n in range(1, R.ITERATIONS + 1):
        fwd, rev = R.reference(shape, n), R.reference(shape, n, reverse=True)
        assert not fwd.status.any() and fwd.perm.shape == (B, F, K) and fwd.perm.dtype == np.int32
        assert np.array_equal(fwd.perm, rev.perm) and np.array_equal(fwd.changed, rev.changed)
        assert all(R.is_permutation(fwd.perm[b, f], K) for b in range(B) for f in range(F))
        margin = min(margin, fwd.margin, rev.margin)
    e, tol = R.e_ref(shape), R.tolerance(shape)
    print("%s: margin %.3g, e_ref %.3g, tol %.3g" % (shape[:4], margin, e, tol))
    assert margin >= R.MARGIN_FLOOR
    assert tol <= R.TOL_CAP                               # a float32 accumulation, at 1e-7 or above, cannot hide
    assert e <= 1.06 * E_REF_WRITTEN["-".join(str(v) for v in shape[:4])]                   # the docstring's figures (2 digits)
    last = R.reference(shape)
    if K >= 2:
        assert not last.changed.any()
        assert all(R.common_order(c.scramble[b], last.perm[b]) for b in range(B))
        assert (np.abs(last.score) <= K * (1 + 4 * (T + F) * U)).all()                      # K correlations of unit vectors
        # the scramble was real: the identity is not a common order
        assert not all(R.common_order(c.scramble[b], np.tile(np.arange(K), (F, 1))) for b in range(B))


# ---------------------------------------------------------------------------------------------------- pins on the restatement
@pytest.mark.parametrize("shape", [R.PARITY[3], R.PARITY[5]], ids=[R.IDS[3], R.IDS[5]])
def test_continuation_has_the_same_bits(shape):
    P = R.parity_case(shape).P
    whole = R.align(P, 1 + 2)
    first = R.align(P, 1)
    assert first.changed.any()                            # the first iteration moved bins: the continuation starts off the identity
    assert same(whole, R.align(P, 2, perm0=first.perm))


def test_permuting_the_classes_of_a_bin_permutes_its_perm():
    """The classes of one bin of the input reordered by q, and the start of that bin set to q's inverse: the centroids of the
    first iteration are the same sums, the table's columns move with the classes, the scores are the same numbers and the
    margins exceed every noise, so that bin's perm is the old one seen through q and nothing else changes."""
    shape = R.PARITY[5]
    B, K, F, T = shape[:4]
    P = R.parity_case(shape).P
    b0, f0, q = 1, 7, np.array([2, 0, 3, 1])
    moved = P.copy()
    moved[b0, :, f0] = P[b0, q, f0]                       # new class j of the bin is old class q[j]
    perm0 = np.tile(np.arange(K, dtype=np.int32), (B, F, 1))
    perm0[b0, f0] = np.argsort(q)                         # q[perm0[k]] = k
    for n in (1, 2, 8):
        ref, got = R.reference(shape, n), R.align(moved, n, perm0=perm0)
        assert np.array_equal(q[got.perm[b0, f0]], ref.perm[b0, f0])
        rest = np.ones((B, F), bool)
        rest[b0, f0] = False
        assert np.array_equal(got.perm[rest], ref.perm[rest])
        assert np.array_equal(bits(got.score), bits(ref.score)) and np.array_equal(got.changed, ref.changed)


def test_restatement_marks_bad_bins():
    P, perm0, bad, keep = R.status_case()
    B, K, F, T = P.shape
    out = R.align(P, 3, perm0=perm0)
    want = np.zeros((B, F), np.int32)
    for b in bad:
        want[b, bad[b]] = 1
    assert np.array_equal(out.status, want)
    for b in bad:
        for f in bad[b]:
            assert np.array_equal(out.perm[b, f], np.arange(K)) and np.isnan(out.score[b, f])
        # a bin of status 1 takes no part in the centroids: the item without its data has the same bits
        alone = R.align(P[b:b + 1][:, :, keep[b]], 3, perm0=perm0[b:b + 1][:, keep[b]])
        assert not alone.status.any()
        assert np.array_equal(alone.perm[0], out.perm[b, keep[b]])
        assert np.array_equal(bits(alone.score[0]), bits(out.score[b, keep[b]])) and alone.changed[0] == out.changed[b]
    assert np.isfinite(out.score[want == 0]).all()


def test_a_constant_row_carries_no_evidence():
    shape = R.PARITY[2]
    B, K, F, T = shape[:4]
    P = R.parity_case(shape).P.copy()
    P[0, 1, 3] = 0.25                                     # a constant row: rn = 0
    P[1, :, 5] = 0.0                                      # a bin of constant rows: every score is 0, rank 0 wins
    out = R.align(P, 3)
    assert not out.status.any() and np.isfinite(out.score).all()
    assert out.score[1, 5] == 0.0 and np.array_equal(out.perm[1, 5], np.arange(K))
    u = R.rows(P[0], out.status[0])
    assert (u[1, 3] == 0).all() and np.isfinite(u).all()
    # an item of nothing but constants: the centroids are 0, nothing moves
    flat = R.align(np.ones((1, 2, 3, 4)), 2)
    assert (flat.score == 0).all() and not flat.changed.any() and not flat.status.any()


def test_the_helpers_that_apply_a_perm():
    g = np.random.default_rng(5)
    x = g.standard_normal((2, 3, 4, 5))
    perm = np.stack([np.stack([g.permutation(3) for _ in range(4)]) for _ in range(2)]).astype(np.int32)
    out = R.permute_bins(x, perm)
    assert all((out[b, k, f] == x[b, perm[b, f, k], f]).all() for b in range(2) for k in range(3) for f in range(4))
    assert np.array_equal(R.permute_bins(out, np.argsort(perm, axis=-1).astype(np.int32)), x)
    perm[1, 2] = [0, 3, 1]
    assert np.array_equal(R.permute_bins(x, perm)[1, :, 2], x[1, :, 2])
    a = g.standard_normal((2, 4, 3, 2))
    perm[1, 2] = [2, 0, 1]
    assert all((R.permute_rows(a, perm)[b, f, k] == a[b, f, perm[b, f, k]]).all() for b in range(2) for f in range(4) for k in range(3))


# ------------------------------------------------------------------------------------------------------- the cACGMM workflow
def test_alignment_repairs_a_cacgmm_started_per_bin():
    """cacgmm_ref.case(1, 4, 2, 33, 100, 7), cACGMM started from an init drawn independently per bin: the agreement with the
    oracle masks is 0.574137 after 10 iterations, 0.771921 once the masks are aligned, and 0.830012 after 10 more iterations
    from the aligned masks and quadratic (the restatement's values; it rises at both steps).  Run forward and with the frames
    and bins added in the opposite order the three values differ by at most 1.9e-14 and the perm is the same (the alignment's
    smallest margin is 0.11), so the six written digits, +- 5e-7, are what the assertion allows: 1e-6."""
    fwd, rev = R.chain(), R.chain(True)
    print("agreements %.6f %.6f %.6f, forward - reversed %s, tolerance of the chain %.3g"
          % (fwd.agreements + ([a - b for a, b in zip(fwd.agreements, rev.agreements)], R.chain_tolerance())))
    assert not fwd.first.status.any() and not fwd.second.status.any()
    assert np.array_equal(fwd.perm, rev.perm)
    assert max(abs(a - b) for a, b in zip(fwd.agreements, rev.agreements)) <= 1e-12
    for got, written in zip(fwd.agreements, (0.574137, 0.771921, 0.830012)):
        assert abs(got - written) <= 1e-6
    assert fwd.agreements[0] < fwd.agreements[1] < fwd.agreements[2]
    assert R.chain_tolerance() <= C.TOL_CAP
    a = R.align(fwd.first.masks, 10)
    assert not a.changed.any() and a.margin >= 1e-3       # far above the masks' tolerance: the device finds the same perm
    assert not np.array_equal(fwd.perm, np.tile(np.arange(2), (1, 33, 1)))


# ------------------------------------------------------------------------------------------------------------ argument rules
def _f64(*shape, dtype=torch.float64):
    return torch.ones(shape, dtype=dtype)


def _perm(*shape, dtype=torch.int32):
    return torch.zeros(shape, dtype=dtype)


RULES = [
    ("align_permutations", (_f64(2, 3, 4, dtype=torch.float32),), {}),
    ("align_permutations", (np.ones((2, 3, 4)),), {}),
    ("align_permutations", (_f64(3, 4),), {}),                                                  # rank
    ("align_permutations", (_f64(1, 2, 2, 3, 4),), {}),
    ("align_permutations", (_f64(9, 3, 4),), {}),                                               # K > 8
    ("align_permutations", (_f64(0, 3, 4),), {}),                                               # K = 0
    ("align_permutations", (_f64(2, 0, 4),), {}),                                               # F = 0
    ("align_permutations", (_f64(2, 3, 1),), {}),                                               # T < 2
    ("align_permutations", (_f64(2, 3, 65536),), {}),
    ("align_permutations", (_f64(0, 2, 3, 4),), {}),                                            # B = 0
    ("align_permutations", (_f64(2, 3, 4),), {"iterations": 0}),
    ("align_permutations", (_f64(2, 3, 4),), {"iterations": 257}),
    ("align_permutations", (_f64(2, 3, 4),), {"iterations": 2.0}),
    ("align_permutations", (_f64(2, 3, 4),), {"perm0": _perm(3, 2, dtype=torch.int64)}),
    ("align_permutations", (_f64(2, 3, 4),), {"perm0": _perm(2, 3)}),                           # (K, F), not (F, K)
    ("align_permutations", (_f64(2, 3, 4),), {"perm0": _perm(1, 3, 2)}),                        # a batch the profile has not
    ("align_permutations", (_f64(5, 2, 3, 4),), {"perm0": _perm(3, 2)}),
    ("align_permutations", (_f64(2, 3, 4),), {"perm0": [[0, 1]] * 3}),
    ("permute_bins", (_f64(2, 3, 4, dtype=torch.float16), _perm(3, 2)), {}),
    ("permute_bins", (_f64(2, 3, 4, dtype=torch.int32), _perm(3, 2)), {}),
    ("permute_bins", (_f64(3, 4), _perm(3, 2)), {}),
    ("permute_bins", (_f64(9, 3, 4), _perm(3, 9)), {}),
    ("permute_bins", (_f64(2, 3, 4), _perm(3, 2, dtype=torch.int64)), {}),
    ("permute_bins", (_f64(2, 3, 4), _perm(2, 3)), {}),
    ("permute_bins", (_f64(1, 2, 3, 4), _perm(3, 2)), {}),
    ("permute_bins", (_f64(2, 3, 4), None), {}),
    ("permute_rows", (_f64(3, 2, 2), _perm(3, 2, dtype=torch.int64)), {}),
    ("permute_rows", (_f64(3, 2, 2), _perm(2)), {}),
    ("permute_rows", (_f64(3, 2, 2), _perm(2, 3)), {}),                                         # a's leading sizes are perm's
    ("permute_rows", (_f64(3), _perm(3, 2)), {}),
    ("permute_rows", (np.ones((3, 2, 2)), _perm(3, 2)), {}),
    ("permute_rows", (_f64(0, 2, 2), _perm(0, 2)), {}),
]


@pytest.mark.parametrize("name,args,kwargs", RULES, ids=["%s-%d" % (r[0], i) for i, r in enumerate(RULES)])
def test_argument_rules(SEP, name, args, kwargs):
    with pytest.raises(ValueError, match="^%s: " % name):
        getattr(SEP, name)(*args, **kwargs)


def test_cpu_tensors_are_refused_last(SEP):
    with pytest.raises(RuntimeError, match="^align_permutations: .*no CPU fallback"):
        SEP.align_permutations(_f64(2, 3, 4))
    with pytest.raises(RuntimeError, match="^align_permutations: .*no CPU fallback"):
        SEP.align_permutations(_f64(1, 2, 3, 4), 3, perm0=_perm(1, 3, 2))
    with pytest.raises(ValueError, match="^align_permutations: iterations"):                    # the ranges come first
        SEP.align_permutations(_f64(2, 3, 4), 300)
    with pytest.raises(RuntimeError, match="^permute_bins: .*no CPU fallback"):
        SEP.permute_bins(torch.zeros((2, 3, 4), dtype=torch.complex64), _perm(3, 2))
    with pytest.raises(RuntimeError, match="^permute_rows: .*no CPU fallback"):
        SEP.permute_rows(torch.zeros((3, 2, 4, 4), dtype=torch.complex128), _perm(3, 2))
    assert SEP.ALIGN._fields == ("perm", "score", "changed", "status")


# ----------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_holds_the_new_entry_points():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native as N
    for name in NEW_EXPORTS:
        assert name in N.EXPORTS and hasattr(N.lib(), name)
    lib = N.lib()
    assert lib.alvq_align_workspace_bytes(64, 2, 201, 500) == 16 * 64 * 2 * 201 + 8 * 64 * 2 * 500 + 4 * 64 * 201
    assert lib.alvq_align_workspace_bytes(1, 1, 1, 2) == 16 + 16 + 4
    for dims in ((0, 2, 5, 10), (65536, 2, 5, 10), (1, 0, 5, 10), (1, 9, 5, 10), (1, 2, 0, 10), (1, 2, 5, 1), (1, 2, 5, 0),
                 (1, 2, 5, 65536), (65535, 2, 65536, 10)):
        assert lib.alvq_align_workspace_bytes(*dims) == -1
    one = 16                                              # any non-null address: every case below is refused before a launch
    ptrs = (one, None, one, one, one, one, one)
    for args, word in ((ptrs + (1, 2, 5, 10, 0, None), b"iterations"),
                       (ptrs + (1, 2, 5, 10, 257, None), b"iterations"),
                       (ptrs + (1, 9, 5, 10, 3, None), b"K=9"),
                       (ptrs + (1, 0, 5, 10, 3, None), b"K=0"),
                       (ptrs + (1, 2, 5, 1, 3, None), b"T=1"),
                       (ptrs + (1, 2, 5, 65536, 3, None), b"T=65536"),
                       (ptrs + (0, 2, 5, 10, 3, None), b"B=0"),
                       ((None,) + ptrs[1:] + (1, 2, 5, 10, 3, None), b"null"),
                       (ptrs[:6] + (None,) + (1, 2, 5, 10, 3, None), b"null")):
        assert lib.alvq_align_permutations_f64(*args) == -1
        msg = lib.alvq_last_error()
        assert msg.startswith(b"alvq_align_permutations_f64") and word in msg, msg
    for args, word in (((one, one, 32, 1, 2, 5, 10, 3, None), b"elem_bytes"),
                       ((one, one, 32, 1, 2, 5, 10, 0, None), b"elem_bytes"),
                       ((one, one, 32, 1, 9, 5, 10, 8, None), b"K=9"),
                       ((one, one, 32, 1, 2, 5, 0, 8, None), b"T=0"),
                       ((one, one, one, 1, 2, 5, 10, 8, None), b"out must not be x"),
                       ((one, None, 32, 1, 2, 5, 10, 8, None), b"null"),
                       ((one, one, None, 1, 2, 5, 10, 8, None), b"null")):
        assert lib.alvq_permute_bins(*args) == -1
        msg = lib.alvq_last_error()
        assert msg.startswith(b"alvq_permute_bins") and word in msg, msg
