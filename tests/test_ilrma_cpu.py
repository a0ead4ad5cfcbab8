"""ILRMA without a GPU: the pins on the numpy restatement tests/helpers/ilrma_ref.py, the conditions its seeded cases meet (the
inputs are chosen so that the restatement alone meets them: they are no measurements of csrc/ilrma.hip), the argument rules of
acoustic_locating_vq_vae.separation on CPU tensors, and the three entry points of the C ABI.  u = 1.1e-16."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import iva_ref as IR  # noqa: E402
import ilrma_ref as R  # noqa: E402

U = R.U
NEW_EXPORTS = ("alvq_ilrma_workspace_bytes", "alvq_ilrma_f32", "alvq_ilrma_f64")


def bits(a):
    """The bits of a float64 or complex128 array, so that a NaN equals itself."""
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def SEP():
    from acoustic_locating_vq_vae import separation
    return separation


# ---------------------------------------------------------------------------------------------------- pins on the restatement
@pytest.mark.parametrize("shape", R.PARITY[1:4], ids=R.IDS[1:4])
def test_cost_is_kept_by_the_normalisation_and_does_not_rise(shape):
    """sum (P / R + log R) - 2 T sum_f log |det W_f|: step 2 leaves it where it is and an iteration does not raise it, both to a
    relative 1e-12, on cases whose floor is never active (asserted)."""
    B, D, F, T, L = shape[:5]
    X = R.parity_case(shape).X
    basis, act = (a.copy() for a in R.parity_start(shape))
    W = np.broadcast_to(np.eye(D, dtype=np.complex128), (B, F, D, D)).copy()
    status, kappa = np.zeros((B, F), np.int32), np.zeros((B, F))
    seen = {}
    for it in range(shape[5]):
        for b in range(B):
            before = R.cost(X[b], W[b], basis[b], act[b], status[b])
            P = R.power(X[b], W[b], status[b])
            Wn, _, bn = R.normalise(W[b], P, basis[b], R.scale(P, status[b]), status[b], R.FLOOR, seen)
            scaled = R.cost(X[b], Wn, bn, act[b], status[b])
            assert abs(scaled - before) <= 1e-12 * abs(before), (it, b, before, scaled)
            W[b], basis[b], act[b] = R.iterate(X[b], W[b], basis[b], act[b], status[b], kappa[b], R.FLOOR, False, seen)
            after = R.cost(X[b], W[b], basis[b], act[b], status[b])
            print("%s iteration %d item %d: cost %.15g -> %.15g" % (shape[:5], it, b, before, after))
            assert after <= before + 1e-12 * abs(before), (it, b, before, after)
    assert not status.any() and seen.get("floor", 0) == 0


def test_one_basis_has_a_closed_form():
    """L = 1: R = b[f] a[t], so basis <- sqrt(b[f] mean_t(P / a)) and then activations <- sqrt(a[t] mean_f(P / b))."""
    P = np.array([[[1.0, 4.0, 2.0], [0.5, 3.0, 8.0]]])                                        # (D, F, T) = (1, 2, 3)
    b0 = np.array([[[2.0], [0.25]]])
    a0 = np.array([[[1.0, 0.5, 4.0]]])
    status = np.zeros(2, np.int32)
    b1 = R.update_basis(P, b0, a0, status, R.FLOOR)
    want_b = np.sqrt(b0[0, :, 0] * (P[0] / a0[0, 0]).mean(axis=1))
    assert np.abs(b1[0, :, 0] - want_b).max() <= 8 * U * want_b.max()
    a1 = R.update_activations(P, b1, a0, status, R.FLOOR)
    want_a = np.sqrt(a0[0, 0] * (P[0] / b1[0, :, 0, None]).mean(axis=0))
    assert np.abs(a1[0, 0] - want_a).max() <= 8 * U * want_a.max()
    status[1] = 1                                         # a refused bin keeps its row and leaves the sum over f
    assert np.array_equal(R.update_basis(P, b0, a0, status, R.FLOOR)[0, 1], b0[0, 1])
    a2 = R.update_activations(P, b1, a0, status, R.FLOOR)
    want = np.sqrt(a0[0, 0] * P[0, 0] / b1[0, 0, 0])
    assert np.abs(a2[0, 0] - want).max() <= 8 * U * want.max()


def test_the_floor_takes_what_is_not_finite():
    got = R.floored(np.array([np.nan, np.inf, -1.0, 0.0, 1e-11, 1e-9, 3.0]), 1e-10)
    assert np.array_equal(got, [1e-10, 1e-10, 1e-10, 1e-10, 1e-10, 1e-9, 3.0])
    assert np.array_equal(R.updated(np.array([2.0, 2.0]), np.array([0.0, 8.0]), np.array([0.0, 2.0]), 1e-10), [2.0, 4.0])


def test_continuation_has_the_same_bits():
    shape = R.PARITY[2]
    X = R.parity_case(shape).X
    b0, a0 = R.parity_start(shape)
    whole = R.ilrma(X, b0, a0, 2 + 3)
    part = R.ilrma(X, b0, a0, 2)
    again = R.ilrma(X, part.basis, part.activations, 3, w0=part.W)
    for a, b in zip(whole[:5], again[:5]):
        assert np.array_equal(bits(a) if a.dtype != np.int32 else a, bits(b) if b.dtype != np.int32 else b)


def test_no_iteration_returns_the_start():
    shape = R.PARITY[2]
    B, D, F, T = shape[:4]
    X = R.parity_case(shape).X
    b0, a0 = R.parity_start(shape)
    out = R.ilrma(X, b0, a0, 0)
    assert np.array_equal(out.basis, b0) and np.array_equal(out.activations, a0) and not out.status.any()
    assert (out.W == np.eye(D)).all() and np.array_equal(out.Y[:, 0], X[:, 0]) and not out.Y[:, 1:].any()


def test_restatement_refuses_bad_bins():
    shape = R.PARITY[2]
    B, D, F, T = shape[:4]
    X, b0, a0, want = R.bad_inputs(shape)
    out = R.ilrma(X, b0, a0, 3)
    assert np.array_equal(out.status, want)
    for b, f in zip(*np.nonzero(want)):
        assert np.array_equal(out.W[b, f], np.eye(D)) and np.array_equal(bits(out.Y[b, :, f]), bits(X[b, :, f]))
        assert np.array_equal(bits(out.basis[b, :, f]), bits(b0[b, :, f]))                     # as it came
    assert np.isfinite(out.activations).all() and np.isfinite(out.basis.transpose(0, 2, 1, 3)[want == 0]).all()
    # the bins of status 1 take no part in any sum over f: the same item without their data has the same bits
    keep = [f for f in range(F) if want[0, f] == 0]
    alone = R.ilrma(X[:1, :, keep], b0[:1, :, keep], a0[:1], 3)
    assert np.array_equal(bits(alone.W), bits(out.W[:1, keep])) and np.array_equal(bits(alone.basis), bits(out.basis[:1, :, keep]))
    assert np.array_equal(bits(alone.activations), bits(out.activations[:1]))
    X2 = R.parity_case(shape).X.copy()
    X2[1, :, 5] = X2[1, 0, 5]                             # two identical microphones: rank-deficient
    two = R.ilrma(X2, *R.parity_start(shape), 3)
    assert two.status[1, 5] == 2 and int((two.status != 0).sum()) == 1 and np.array_equal(two.W[1, 5], np.eye(D))


# ------------------------------------------------------------------------------------------------ conditions on the cases
@pytest.mark.parametrize("shape", R.PARITY, ids=R.IDS)
def test_parity_cases_are_well_conditioned(shape):
    for single in (False, True):
        ref = R.reference(shape, single=single)
        assert not ref.status.any() and not R.reference(shape, single=single, reverse=True).status.any()
        assert ref.kappa.max() <= R.KAPPA_CAP, ref.kappa.max()
        tol = R.tolerance(shape, single)
        print("%s %s: kappa %.3g, e_ref %.3g, tol %.3g, floored %d" % (shape[:5], "complex64" if single else "complex128",
                                                                      ref.kappa.max(), R.e_ref(shape, single), tol, ref.floored))
        assert tol <= 1e-10
        assert max(np.linalg.cond(w) for w in ref.W.reshape(-1, shape[1], shape[1])) <= R.COND_CAP


@pytest.mark.parametrize("shape", R.SEPARATION, ids=R.SEPARATION_IDS)
def test_separation_cases_separate(shape):
    c = R.parity_case(shape)
    ref = R.reference(shape)
    assert not ref.status.any()
    gain = IR.improvement(c.images, c.mix, ref.Y)
    print("%s: SI-SDR improvement %s dB, e_ref %.3g" % (shape[:5], np.round(gain, 2), R.e_ref(shape)))
    assert (gain >= 20.0).all()


# ------------------------------------------------------------------------------------------------------------ argument rules
def _spec(*shape, dtype=torch.complex128):
    return torch.zeros(shape, dtype=dtype)


def _ones(*shape, dtype=torch.float64):
    return torch.ones(shape, dtype=dtype)


GOOD = (_spec(2, 3, 4), _ones(2, 3, 2), _ones(2, 2, 4))               # (D, F, T) = (2, 3, 4), L = 2
RULES = [
    ("ilrma", (torch.zeros(2, 3, 4),) + GOOD[1:], {}),                                        # not complex
    ("ilrma", (_spec(3, 4),) + GOOD[1:], {}),                                                 # rank
    ("ilrma", (_spec(1, 9, 3, 4), _ones(1, 9, 3, 2), _ones(1, 9, 2, 4)), {}),                 # D > 8
    ("ilrma", (GOOD[0], _ones(2, 3, 2, dtype=torch.float32), GOOD[2]), {}),
    ("ilrma", (GOOD[0], _ones(1, 2, 3, 2), GOOD[2]), {}),                                     # a batch the spec has not
    ("ilrma", (GOOD[0], _ones(2, 4, 2), GOOD[2]), {}),                                        # F
    ("ilrma", (GOOD[0], _ones(2, 3, 17), _ones(2, 17, 4)), {}),                               # L > 16
    ("ilrma", (GOOD[0], _ones(2, 3, 0), _ones(2, 0, 4)), {}),                                 # L = 0
    ("ilrma", (GOOD[0], GOOD[1], _ones(2, 3, 4)), {}),                                        # another L
    ("ilrma", (GOOD[0], GOOD[1], _ones(2, 2, 5)), {}),                                        # T
    ("ilrma", (GOOD[0], GOOD[1], np.ones((2, 2, 4))), {}),
    ("ilrma", (GOOD[0], None, GOOD[2]), {}),
    ("ilrma", GOOD, {"iterations": 257}),
    ("ilrma", GOOD, {"iterations": -1}),
    ("ilrma", GOOD, {"iterations": 2.0}),
    ("ilrma", GOOD, {"ref": 2}),
    ("ilrma", GOOD, {"ref": -1}),
    ("ilrma", GOOD, {"floor": 0.0}),
    ("ilrma", GOOD, {"floor": -1e-3}),
    ("ilrma", GOOD, {"floor": float("nan")}),
    ("ilrma", GOOD, {"floor": float("inf")}),
    ("ilrma", GOOD, {"w0": _spec(3, 2, 2, dtype=torch.complex64)}),
    ("ilrma", GOOD, {"w0": _spec(1, 3, 2, 2)}),
    ("ilrma", GOOD, {"w0": np.zeros((3, 2, 2), np.complex128)}),
    ("nmf_init", (0, 2, 3, 4), {}),
    ("nmf_init", (1, 9, 3, 4), {}),
    ("nmf_init", (1, 2, 0, 4), {}),
    ("nmf_init", (1, 2, 3, 65536), {}),
    ("nmf_init", (1, 2, 3, 4), {"bases": 17}),
    ("nmf_init", (1, 2, 3, 4), {"bases": 0}),
    ("nmf_init", (1, 2, 3, 4), {"bases": 2.0}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"method": "fastica"}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"method": 1}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"method": "ilrma", "model": "gauss"}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"method": "ilrma", "bases": 17}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"method": "ilrma", "bases": 0}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"method": "ilrma", "generator": 5}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"method": "ilrma", "iterations": 300}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"method": "ilrma", "ref": 2}),
]


@pytest.mark.parametrize("name,args,kwargs", RULES, ids=["%s-%d" % (r[0], i) for i, r in enumerate(RULES)])
def test_argument_rules(SEP, name, args, kwargs):
    with pytest.raises(ValueError, match="^%s: " % name):
        getattr(SEP, name)(*args, **kwargs)


def test_cpu_tensors_are_refused_last(SEP):
    with pytest.raises(RuntimeError, match="^ilrma: .*no CPU fallback"):
        SEP.ilrma(*GOOD)
    with pytest.raises(RuntimeError, match="^separate_waves: .*no CPU fallback"):
        SEP.separate_waves(torch.zeros(1, 2, 400), method="ilrma")
    with pytest.raises(ValueError, match="^ilrma: ref"):                                       # the ranges come first
        SEP.ilrma(*GOOD, ref=5)
    assert SEP.MAX_BASES == 16 and SEP.ILRMA._fields == ("spec", "w", "basis", "activations", "status")


def test_nmf_init_on_the_host(SEP):
    b0, a0 = SEP.nmf_init(2, 3, 5, 7, bases=4, generator=torch.Generator().manual_seed(3), device="cpu")
    assert b0.shape == (2, 3, 5, 4) and a0.shape == (2, 3, 4, 7) and b0.dtype == a0.dtype == torch.float64
    for a in (b0, a0):
        assert bool((a >= 1e-3).all()) and bool((a < 1.0 + 1e-3).all())
    again = SEP.nmf_init(2, 3, 5, 7, bases=4, generator=torch.Generator().manual_seed(3), device="cpu")
    assert torch.equal(b0, again[0]) and torch.equal(a0, again[1])
    assert SEP.nmf_init(1, 2, 3, 4, device="cpu")[0].shape == (1, 2, 3, 2)                      # bases defaults to 2


# ----------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_holds_the_new_entry_points():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native as N
    for name in NEW_EXPORTS:
        assert name in N.EXPORTS and hasattr(N.lib(), name)
    lib = N.lib()
    B, D, L, F, T = 64, 2, 2, 201, 500
    assert lib.alvq_ilrma_workspace_bytes(B, D, L, F, T) == 8 * B * D * F * T + 16 * B * F * D ** 3 + 8 * B * D * F + 8 * B * D + 4 * B
    assert lib.alvq_ilrma_workspace_bytes(1, 1, 1, 1, 1) == 5 * 16
    for dims in ((0, 2, 2, 5, 10), (1, 9, 2, 5, 10), (1, 2, 0, 5, 10), (1, 2, 17, 5, 10), (1, 2, 2, 0, 10), (1, 2, 2, 5, 65536),
                 (65536, 2, 2, 5, 10), (65535, 2, 2, 65536, 10)):
        assert lib.alvq_ilrma_workspace_bytes(*dims) == -1
    one = 1                                               # any non-null address: every case below is refused before a launch
    ptrs = (one, None) + (one,) * 8
    for args, word in ((ptrs + (1, 2, 2, 5, 10, 257, 0, 1e-10, None), b"iterations"),
                       (ptrs + (1, 2, 2, 5, 10, 3, 2, 1e-10, None), b"ref"),
                       (ptrs + (1, 2, 2, 5, 10, 3, 0, 0.0, None), b"floor"),
                       (ptrs + (1, 2, 2, 5, 10, 3, 0, float("nan"), None), b"floor"),
                       (ptrs + (1, 2, 17, 5, 10, 3, 0, 1e-10, None), b"L=17"),
                       (ptrs + (1, 9, 2, 5, 10, 3, 0, 1e-10, None), b"D=9"),
                       ((one, None, None) + (one,) * 7 + (1, 2, 2, 5, 10, 3, 0, 1e-10, None), b"null"),
                       ((one, None) + (one,) * 7 + (None,) + (1, 2, 2, 5, 10, 3, 0, 1e-10, None), b"null")):
        for fn in (lib.alvq_ilrma_f32, lib.alvq_ilrma_f64):
            assert fn(*args) == -1
            msg = lib.alvq_last_error()
            assert msg.startswith(b"alvq_ilrma_f") and word in msg, msg
