"""cACGMM without a GPU: the pins on the numpy restatement tests/helpers/cacgmm_ref.py, the conditions its seeded cases meet (the
inputs are chosen so that the restatement alone meets them: they are no measurements of csrc/cacgmm.hip), the argument rules of
acoustic_locating_vq_vae.separation.cacgmm / time_masks on CPU tensors, and the three entry points of the C ABI.  u = 1.1e-16."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import cacgmm_ref as R  # noqa: E402

U = R.U
NEW_EXPORTS = ("alvq_cacgmm_workspace_bytes", "alvq_cacgmm_f32", "alvq_cacgmm_f64")


def bits(a):
    """The bits of a float64 or complex128 array, so that a NaN equals itself."""
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def SEP():
    from acoustic_locating_vq_vae import separation
    return separation


# ---------------------------------------------------------------------------------------------------- pins on the restatement
@pytest.mark.parametrize("shape", R.PARITY[:6], ids=R.IDS[:6])
def test_masks_add_up_to_one(shape):
    ref = R.reference(shape)
    B, D, K, F, T = shape[:5]
    assert ref.masks.shape == (B, K, F, T) and ref.prior.shape == (B, K, T) and ref.cov.shape == (B, F, K, D, D)
    assert (np.abs(ref.masks.sum(axis=1) - 1.0) <= 8 * U).all() and (ref.masks >= 0).all()
    assert (np.abs(ref.prior.sum(axis=1) - 1.0) <= (8 + F) * U).all()
    assert (ref.quadratic > 0).all()
    assert (np.abs(np.trace(ref.cov, axis1=-2, axis2=-1) - D) <= 16 * D * U * D).all()        # normalised: the trace is D
    assert np.array_equal(ref.cov, np.conj(np.swapaxes(ref.cov, -1, -2)))


def test_permuting_the_init_permutes_the_output():
    shape = R.PARITY[3]
    c = R.parity_case(shape)
    perm = [2, 0, 1]
    ref = R.reference(shape)
    out = R.cacgmm(c.X, c.init[:, perm], shape[5])
    # the softmax adds its K terms in another order, nothing else changes: reordering noise, which the case's tolerance bounds
    tol = R.tolerance(shape)
    assert np.abs(out.masks - ref.masks[:, perm]).max() <= tol
    assert np.abs(out.prior - ref.prior[:, perm]).max() <= tol
    assert np.abs(out.quadratic - ref.quadratic[:, perm]).max() <= tol * ref.quadratic.max()
    bound = R.C_COV * tol * ref.cond[:, :, perm]
    assert (np.abs(out.cov - ref.cov[:, :, perm]).max(axis=(-2, -1)) <= bound).all()


def test_continuation_has_the_same_bits():
    shape = R.PARITY[2]
    c = R.parity_case(shape)
    whole = R.cacgmm(c.X, c.init, 3 + 4)
    first = R.cacgmm(c.X, c.init, 3)
    again = R.cacgmm(c.X, first.masks, 4, quadratic0=first.quadratic)
    for a, b in zip(whole[:4], again[:4]):
        assert np.array_equal(bits(a), bits(b))


def test_two_directions_are_found():
    """D = K = 2 and a bin whose frames point in exactly two directions (with random complex amplitudes): each class takes one."""
    g = np.random.default_rng(11)
    T = 60
    dirs = np.array([[1.0, 0.5 + 0.5j], [1.0, -0.8j]]).T                    # (D, 2)
    which = np.arange(T) % 3 == 0                                           # every third frame points along direction 1
    amp = g.standard_normal(T) + 1j * g.standard_normal(T)
    x = np.where(which, dirs[:, 1:2], dirs[:, 0:1]) * amp                   # (D, T)
    init = R.time_masks(g, 1, 2, 1, T)
    out = R.cacgmm(x[None, :, None, :], init, 20)
    assert not out.status.any()
    m = out.masks[0, :, 0]
    k1 = int(m[1, which].mean() > m[0, which].mean())
    assert (m[k1, which] >= 1 - 1e-6).all() and (m[1 - k1, ~which] >= 1 - 1e-6).all()


def test_restatement_marks_bad_bins_and_silent_frames():
    shape = R.PARITY[2]
    B, D, K, F, T = shape[:5]
    c = R.parity_case(shape)
    X, init, q0 = c.X.copy(), c.init.copy(), np.ones((B, K, F, T))
    X[0, 1, 1, 7] = complex(np.nan, 0.0)
    init[0, 1, 2, 9] = -0.25
    q0[1, 0, 3, 4] = 0.0
    X[1, :, 5] = 0                                        # every frame silent: no error, the masks are the priors
    X[1, :, 6, 10] = 0                                    # one silent frame in a good bin
    out = R.cacgmm(X, init, 3, quadratic0=q0)
    want = np.zeros((B, F), np.int32)
    want[0, 1] = want[0, 2] = want[1, 3] = 1
    assert np.array_equal(out.status, want)
    for b, f in ((0, 1), (0, 2), (1, 3)):
        assert (out.masks[b, :, f] == 1.0 / K).all() and (out.quadratic[b, :, f] == 1).all()
        assert (out.cov[b, f] == np.eye(D)).all()
    assert np.array_equal(out.masks[1, :, 5], out.prior[1]) and (out.quadratic[1, :, 5] == 1).all()
    assert (out.cov[1, 5] == np.eye(D)).all()
    assert np.array_equal(out.masks[1, :, 6, 10], out.prior[1, :, 10]) and (out.quadratic[1, :, 6, 10] == 1).all()
    # a bin of status 1 takes no part in the priors: the item without its data has the same bits
    keep = [f for f in range(F) if f not in (1, 2)]
    alone = R.cacgmm(X[:1, :, keep], init[:1, :, keep], 3, quadratic0=q0[:1, :, keep])
    assert np.array_equal(bits(alone.masks), bits(out.masks[:1, :, keep]))


# ------------------------------------------------------------------------------------------------ conditions on the cases
@pytest.mark.parametrize("shape", R.PARITY, ids=R.IDS)
def test_parity_cases_meet_their_conditions(shape):
    for single in (False, True):
        ref = R.reference(shape, single=single)
        assert not ref.status.any()
        tol = R.tolerance(shape, single)
        print("%s %s: e_ref %.3g, tol %.3g, cond up to %.3g, cov forward/reverse over tol cond %.3g"
              % (shape[:5], "complex64" if single else "complex128", R.e_ref(shape, single), tol, ref.cond.max(),
                 R.cov_ratio(shape, single)))
        assert tol <= R.TOL_CAP                           # a float32 accumulation, at 1e-7 or above, cannot hide
        assert ref.cond.max() <= R.COND_CAP
        assert R.cov_ratio(shape, single) <= R.COV_RATIO_CAP


@pytest.mark.parametrize("shape", R.SEPARATION, ids=R.SEP_IDS)
def test_separation_cases_separate(shape):
    K = shape[2]
    c = R.parity_case(shape)
    ref = R.reference(shape)
    assert not ref.status.any()
    for b in range(shape[0]):
        A, perm = R.agreement(ref.masks[b], c.oracle[b])
        own, _ = R.agreement(c.oracle[b], c.oracle[b])
        print("%s item %d: agreement %.4f under %s, the oracle's own %.4f, chance %.3f" % (shape[:5], b, A, perm, own, 1.0 / K))
        assert A >= 0.9 * own and A >= 1.0 / K + 0.25


# ------------------------------------------------------------------------------------------------------------ argument rules
def _spec(*shape, dtype=torch.complex128):
    return torch.zeros(shape, dtype=dtype)


def _f64(*shape, dtype=torch.float64):
    return torch.ones(shape, dtype=dtype)


RULES = [
    ("cacgmm", (torch.zeros(2, 3, 4), _f64(2, 3, 4)), {}),                                      # not complex
    ("cacgmm", (_spec(3, 4), _f64(2, 3, 4)), {}),                                               # rank
    ("cacgmm", (_spec(1, 9, 3, 4), _f64(1, 2, 3, 4)), {}),                                      # D > 8
    ("cacgmm", (_spec(1, 1, 3, 4), _f64(1, 2, 3, 4)), {}),                                      # D < 2
    ("cacgmm", (_spec(2, 0, 4), _f64(2, 0, 4)), {}),                                            # F = 0
    ("cacgmm", (_spec(2, 3, 4), _f64(2, 3, 4, dtype=torch.float32)), {}),
    ("cacgmm", (_spec(2, 3, 4), np.ones((2, 3, 4))), {}),
    ("cacgmm", (_spec(2, 3, 4), _f64(1, 2, 3, 4)), {}),                                         # a batch the spec has not
    ("cacgmm", (_spec(5, 2, 3, 4), _f64(2, 3, 4)), {}),
    ("cacgmm", (_spec(2, 3, 4), _f64(2, 3, 5)), {}),                                            # T
    ("cacgmm", (_spec(2, 3, 4), _f64(2, 2, 4)), {}),                                            # F neither 1 nor 3
    ("cacgmm", (_spec(2, 3, 4), _f64(9, 3, 4)), {}),                                            # K > 8
    ("cacgmm", (_spec(2, 3, 4), _f64(0, 3, 4)), {}),                                            # K = 0
    ("cacgmm", (_spec(2, 3, 4), _f64(2, 3, 4)), {"iterations": 0}),
    ("cacgmm", (_spec(2, 3, 4), _f64(2, 3, 4)), {"iterations": 257}),
    ("cacgmm", (_spec(2, 3, 4), _f64(2, 3, 4)), {"iterations": 2.0}),
    ("cacgmm", (_spec(2, 3, 4), _f64(2, 3, 4)), {"floor": -1e-3}),
    ("cacgmm", (_spec(2, 3, 4), _f64(2, 3, 4)), {"floor": 1.5}),
    ("cacgmm", (_spec(2, 3, 4), _f64(2, 3, 4)), {"floor": float("nan")}),
    ("cacgmm", (_spec(2, 3, 4), _f64(2, 3, 4)), {"quadratic0": _f64(3, 3, 4)}),                 # another K
    ("cacgmm", (_spec(2, 3, 4), _f64(2, 3, 4)), {"quadratic0": _f64(2, 3, 4, dtype=torch.float32)}),
    ("time_masks", (0, 2, 3, 4), {"device": "cpu"}),
    ("time_masks", (1, 9, 3, 4), {"device": "cpu"}),
    ("time_masks", (1, 2, 3, 65536), {"device": "cpu"}),
    ("time_masks", (1, 2, 3.0, 4), {"device": "cpu"}),
]


@pytest.mark.parametrize("name,args,kwargs", RULES, ids=["%s-%d" % (r[0], i) for i, r in enumerate(RULES)])
def test_argument_rules(SEP, name, args, kwargs):
    with pytest.raises(ValueError, match="^%s: " % name):
        getattr(SEP, name)(*args, **kwargs)


def test_cpu_tensors_are_refused_last(SEP):
    with pytest.raises(RuntimeError, match="^cacgmm: .*no CPU fallback"):
        SEP.cacgmm(_spec(2, 3, 4), _f64(2, 3, 4))
    with pytest.raises(RuntimeError, match="^cacgmm: .*no CPU fallback"):
        SEP.cacgmm(_spec(1, 2, 3, 4), _f64(1, 2, 1, 4))                                         # an init to expand over the bins
    with pytest.raises(ValueError, match="^cacgmm: iterations"):                                # the ranges come first
        SEP.cacgmm(_spec(2, 3, 4), _f64(2, 3, 4), iterations=300)
    assert SEP.CACGMM._fields == ("masks", "prior", "cov", "quadratic", "status") and SEP.MAX_CLASSES == 8


def test_time_masks_is_the_stated_rule(SEP):
    g = torch.Generator().manual_seed(3)
    m = SEP.time_masks(2, 3, 5, 7, generator=g, device="cpu")
    assert m.shape == (2, 3, 5, 7) and m.dtype == torch.float64 and m.is_contiguous()
    assert bool((m == m[:, :, :1]).all())                                                       # constant over the bins
    raw = torch.rand((2, 3, 1, 7), dtype=torch.float64, generator=torch.Generator().manual_seed(3)) + 1e-3
    assert torch.equal(m[:, :, :1], raw / raw.sum(dim=1, keepdim=True))
    assert float((m.sum(dim=1) - 1).abs().max()) <= 4 * U and float(m.min()) > 0
    c = R.parity_case(R.PARITY[2])                                                              # the helper's numpy form of the rule
    assert (c.init == c.init[:, :, :1]).all() and (np.abs(c.init.sum(axis=1) - 1) <= 4 * U).all() and c.init.min() > 0


# ----------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_holds_the_new_entry_points():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native as N
    for name in NEW_EXPORTS:
        assert name in N.EXPORTS and hasattr(N.lib(), name)
    lib = N.lib()
    assert lib.alvq_cacgmm_workspace_bytes(64, 4, 3, 201, 500) == 16 * 64 * 201 * 3 * 16 + 8 * 64 * 201 * 3 + 8 * 64 * 3 * 500
    assert lib.alvq_cacgmm_workspace_bytes(1, 2, 1, 1, 1) == 64 + 8 + 8
    for dims in ((0, 2, 2, 5, 10), (1, 9, 2, 5, 10), (1, 1, 2, 5, 10), (1, 2, 0, 5, 10), (1, 2, 9, 5, 10), (1, 2, 2, 0, 10),
                 (1, 2, 2, 5, 65536), (1, 2, 2, 5, 0), (65536, 2, 2, 5, 10), (65535, 2, 2, 65536, 10)):
        assert lib.alvq_cacgmm_workspace_bytes(*dims) == -1
    one = 1                                               # any non-null address: every case below is refused before a launch
    ptrs = (one, one, None, one, one, one, one, one, one)
    for args, word in ((ptrs + (1, 2, 2, 5, 10, 0, 1e-10, None), b"iterations"),
                       (ptrs + (1, 2, 2, 5, 10, 257, 1e-10, None), b"iterations"),
                       (ptrs + (1, 2, 2, 5, 10, 3, -1.0, None), b"floor"),
                       (ptrs + (1, 2, 2, 5, 10, 3, float("nan"), None), b"floor"),
                       (ptrs + (1, 9, 2, 5, 10, 3, 1e-10, None), b"D=9"),
                       (ptrs + (1, 1, 2, 5, 10, 3, 1e-10, None), b"D=1"),
                       (ptrs + (1, 2, 9, 5, 10, 3, 1e-10, None), b"K=9"),
                       (ptrs + (1, 2, 2, 5, 65536, 3, 1e-10, None), b"T=65536"),
                       ((one, None) + ptrs[2:] + (1, 2, 2, 5, 10, 3, 1e-10, None), b"null"),
                       (ptrs[:8] + (None,) + (1, 2, 2, 5, 10, 3, 1e-10, None), b"null")):
        for fn in (lib.alvq_cacgmm_f32, lib.alvq_cacgmm_f64):
            assert fn(*args) == -1
            msg = lib.alvq_last_error()
            assert msg.startswith(b"alvq_cacgmm_f") and word in msg, msg
