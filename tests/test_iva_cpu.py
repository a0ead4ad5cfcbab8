"""AuxIVA without a GPU: the pins on the numpy restatement tests/helpers/iva_ref.py, the conditions its seeded cases meet (the
inputs are chosen so that the restatement alone meets them: they are no measurements of csrc/iva.hip), the argument rules of
acoustic_locating_vq_vae.separation on CPU tensors, and the five entry points of the C ABI.  u = 1.1e-16."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import iva_ref as R  # noqa: E402

U = R.U
NEW_EXPORTS = ("alvq_auxiva_workspace_bytes", "alvq_auxiva_f32", "alvq_auxiva_f64", "alvq_separation_masks_f32",
               "alvq_separation_masks_f64")


def bits(a):
    """The bits of a complex128 array, so that a NaN equals itself."""
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def SEP():
    from acoustic_locating_vq_vae import separation
    return separation


# ---------------------------------------------------------------------------------------------------- pins on the restatement
def test_elimination_against_numpy_solve():
    g = np.random.default_rng(3)
    for D in range(1, 9):
        M = g.standard_normal((D, D)) + 1j * g.standard_normal((D, D))
        rhs = g.standard_normal((D, D)) + 1j * g.standard_normal((D, D))
        want = np.linalg.solve(M, rhs)
        assert np.abs(R.solve(M, rhs) - want).max() <= 64 * D * U * np.linalg.cond(M) * np.abs(want).max()
    assert R.solve(np.zeros((2, 2)), np.eye(2)) is None
    assert R.solve(np.array([[1.0, 1.0], [1.0, 1.0]]), np.eye(2)) is None              # an exact zero in the second column
    assert R.solve(np.array([[np.nan, 1.0], [1.0, 1.0]]), np.eye(2)) is None
    assert np.array_equal(R.solve(np.array([[0.0, 2.0], [4.0, 0.0]]), np.array([[2.0], [4.0]])), [[1.0], [1.0]])    # rows exchanged


def test_one_microphone_comes_back():
    shape = R.PARITY[0]
    X = R.parity_case(shape).X
    for model in R.MODELS:
        ref = R.reference(shape, model)
        assert not ref.status.any()
        assert (np.abs(ref.Y - X) <= 4 * U * np.abs(X)).all()


def test_rows_are_normalised_at_convergence():
    """W V_k W^H has a unit (k, k) entry where V_k comes from the converged W's own activity."""
    shape = R.SEPARATION[0]
    B, D, F, T = shape[:4]
    X = R.parity_case(shape).X
    W = R.auxiva(X, 60).W
    worst = 0.0
    for b in range(B):
        phi = R.weights(R.activity(X[b], W[b], np.zeros(F, np.int32)), F, "laplace", 1e-10)
        for f in range(F):
            for k in range(D):
                V = R.weighted_cov(X[b, :, f], phi[k])
                worst = max(worst, abs((W[b, f] @ V @ W[b, f].conj().T)[k, k] - 1.0))
    print("largest |(W V_k W^H)[k, k] - 1| after 60 iterations: %.3g" % worst)
    assert worst <= 1e-6


def test_projection_adds_up_to_the_reference_microphone():
    for shape in (R.PARITY[2], R.PARITY[3], R.PARITY[5]):
        B, D, F, T = shape[:4]
        X = R.parity_case(shape).X
        W = R.reference(shape, "laplace").W
        for ref in (0, D - 1):
            Y, _, status = R.project(X, W, np.zeros((B, F), np.int32), ref)
            assert not status.any()
            bound, cond = R.y_bound(X, W, ref)
            assert cond <= R.COND_CAP
            assert (np.abs(Y.sum(axis=1) - X[:, ref]) <= bound.sum(axis=1)).all()


def test_masks_add_up_to_one():
    shape = R.PARITY[3]
    Y = R.reference(shape, "laplace").Y.copy()
    Y[0, :, 2, 5] = 0                                     # a silent point: 1 / K
    Y[0, 1, 3, 6] = complex(np.inf, 0.0)                  # a sum that is not finite: 0
    m = R.masks(Y)
    assert m.shape == Y.shape and m.dtype == np.float64
    assert (m[0, :, 2, 5] == 1.0 / shape[1]).all() and (m[0, :, 3, 6] == 0).all()
    total = m.sum(axis=1)
    total[0, 3, 6] = 1.0
    assert (np.abs(total - 1.0) <= 4 * shape[1] * U).all() and (m >= 0).all()


def test_continuation_through_w0_has_the_same_bits():
    shape = R.PARITY[2]
    X = R.parity_case(shape).X
    for model in R.MODELS:
        whole = R.auxiva(X, 3 + 4, model)
        again = R.auxiva(X, 4, model, w0=R.auxiva(X, 3, model).W)
        assert np.array_equal(bits(whole.W), bits(again.W))
        assert np.array_equal(bits(whole.Y), bits(again.Y))


def test_restatement_refuses_bad_bins():
    shape = R.PARITY[2]
    B, D, F, T = shape[:4]
    X = R.parity_case(shape).X.copy()
    X[0, :, 1] = 0
    X[1, 1, 3, 40] = complex(np.nan, 1.0)
    X[1, :, 5] = X[1, 0, 5]                               # two identical microphones: rank-deficient
    out = R.auxiva(X, 3)
    want = np.zeros((B, F), np.int32)
    want[0, 1], want[1, 3], want[1, 5] = 1, 1, 2
    assert np.array_equal(out.status, want)
    for b, f in ((0, 1), (1, 3), (1, 5)):
        assert np.array_equal(out.W[b, f], np.eye(D))
        assert np.array_equal(bits(out.Y[b, :, f]), bits(X[b, :, f]))
    # the bins of status 1 take no part in r: the same item without their data has the same bits
    keep = [f for f in range(F) if f != 3]
    alone = R.auxiva(X[1:, :, keep], 3)
    assert np.array_equal(bits(alone.W), bits(out.W[1:, keep]))


# ------------------------------------------------------------------------------------------------ conditions on the cases
@pytest.mark.parametrize("model", R.MODELS)
@pytest.mark.parametrize("shape", R.PARITY, ids=R.IDS)
def test_parity_cases_are_well_conditioned(shape, model):
    for single in (False, True):
        ref = R.reference(shape, model, single=single)
        assert not ref.status.any()
        assert ref.kappa.max() <= R.KAPPA_CAP, ref.kappa.max()
        tol = R.w_tolerance(shape, model, single)
        print("%s %s %s: kappa %.3g, e_ref %.3g, tol %.3g" % (shape[:4], model, "complex64" if single else "complex128",
                                                             ref.kappa.max(), R.e_ref(shape, model, single), tol))
        assert tol <= 1e-10
        assert max(np.linalg.cond(w) for w in ref.W.reshape(-1, shape[1], shape[1])) <= R.COND_CAP


@pytest.mark.parametrize("shape", R.SEPARATION, ids=["-".join(str(v) for v in s[:4]) for s in R.SEPARATION])
def test_separation_cases_separate(shape):
    c = R.parity_case(shape)
    ref = R.reference(shape, "laplace")
    assert not ref.status.any()
    gain = R.improvement(c.images, c.mix, ref.Y)
    print("%s: SI-SDR improvement %s dB" % (shape[:4], np.round(gain, 2)))
    assert (gain >= 20.0).all()


# ------------------------------------------------------------------------------------------------------------ argument rules
def _spec(*shape, dtype=torch.complex128):
    return torch.zeros(shape, dtype=dtype)


RULES = [
    ("auxiva", (torch.zeros(2, 3, 4),), {}),                                                  # not complex
    ("auxiva", (_spec(3, 4),), {}),                                                           # rank
    ("auxiva", (_spec(1, 9, 3, 4),), {}),                                                     # D > 8
    ("auxiva", (_spec(2, 0, 4),), {}),                                                        # F = 0
    ("auxiva", (_spec(2, 3, 4),), {"iterations": 257}),
    ("auxiva", (_spec(2, 3, 4),), {"iterations": -1}),
    ("auxiva", (_spec(2, 3, 4),), {"iterations": 2.0}),
    ("auxiva", (_spec(2, 3, 4),), {"model": "cauchy"}),
    ("auxiva", (_spec(2, 3, 4),), {"model": 0}),
    ("auxiva", (_spec(2, 3, 4),), {"ref": 2}),
    ("auxiva", (_spec(2, 3, 4),), {"ref": -1}),
    ("auxiva", (_spec(2, 3, 4),), {"eps": -1e-3}),
    ("auxiva", (_spec(2, 3, 4),), {"eps": float("nan")}),
    ("auxiva", (_spec(2, 3, 4),), {"w0": _spec(3, 2, 2, dtype=torch.complex64)}),
    ("auxiva", (_spec(2, 3, 4),), {"w0": _spec(1, 3, 2, 2)}),                                 # a batch the spec has not
    ("auxiva", (_spec(5, 2, 3, 4),), {"w0": _spec(3, 2, 2)}),
    ("auxiva", (_spec(2, 3, 4),), {"w0": np.zeros((3, 2, 2), np.complex128)}),
    ("masks", (torch.zeros(2, 3, 4),), {}),
    ("masks", (_spec(3, 4),), {}),
    ("masks", (_spec(1, 9, 3, 4),), {}),
    ("separate_waves", (torch.zeros(2, 400),), {}),
    ("separate_waves", (torch.zeros(1, 2, 400, dtype=torch.float16),), {}),
    ("separate_waves", (torch.zeros(1, 9, 400),), {}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"hop": 0}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"n_fft": 1}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"iterations": 300}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"model": "student"}),
    ("separate_waves", (torch.zeros(1, 2, 400),), {"ref": 2}),
    ("separate_waves", (torch.zeros(1, 2, 70000),), {"hop": 1}),                               # T > 65535
]


@pytest.mark.parametrize("name,args,kwargs", RULES, ids=["%s-%d" % (r[0], i) for i, r in enumerate(RULES)])
def test_argument_rules(SEP, name, args, kwargs):
    with pytest.raises(ValueError, match="^%s: " % name):
        getattr(SEP, name)(*args, **kwargs)


def test_cpu_tensors_are_refused_last(SEP):
    for name, args in (("auxiva", (_spec(2, 3, 4),)), ("masks", (_spec(2, 3, 4),)), ("separate_waves", (torch.zeros(1, 2, 400),))):
        with pytest.raises(RuntimeError, match="^%s: .*no CPU fallback" % name):
            getattr(SEP, name)(*args)
    with pytest.raises(ValueError, match="^auxiva: ref"):                                      # the ranges come first
        SEP.auxiva(_spec(2, 3, 4), ref=5)
    assert SEP.MAX_ITERATIONS == 256 and SEP.IVA._fields == ("spec", "w", "status")


# ----------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_holds_the_new_entry_points():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native as N
    for name in NEW_EXPORTS:
        assert name in N.EXPORTS and hasattr(N.lib(), name)
    lib = N.lib()
    assert lib.alvq_auxiva_workspace_bytes(64, 2, 201, 500) == 8 * 64 * 2 * 500 + 16 * 64 * 201 * 8
    assert lib.alvq_auxiva_workspace_bytes(1, 1, 1, 1) == 16 + 16
    for dims in ((0, 2, 5, 10), (1, 9, 5, 10), (1, 2, 0, 10), (1, 2, 5, 65536), (65536, 2, 5, 10), (65535, 2, 65536, 10)):
        assert lib.alvq_auxiva_workspace_bytes(*dims) == -1
    one = 1                                               # any non-null address: every case below is refused before a launch
    for args, word in (((one, None, one, one, one, one, 1, 2, 5, 10, 2, 3, 0, 1e-10, None), b"model"),
                       ((one, None, one, one, one, one, 1, 2, 5, 10, 0, 257, 0, 1e-10, None), b"iterations"),
                       ((one, None, one, one, one, one, 1, 2, 5, 10, 0, 3, 2, 1e-10, None), b"ref"),
                       ((one, None, one, one, one, one, 1, 2, 5, 10, 0, 3, 0, -1.0, None), b"eps"),
                       ((one, None, one, one, one, one, 1, 9, 5, 10, 0, 3, 0, 1e-10, None), b"D=9"),
                       ((one, None, one, one, one, None, 1, 2, 5, 10, 0, 3, 0, 1e-10, None), b"null")):
        for fn in (lib.alvq_auxiva_f32, lib.alvq_auxiva_f64):
            assert fn(*args) == -1
            msg = lib.alvq_last_error()
            assert msg.startswith(b"alvq_auxiva_f") and word in msg, msg
    assert lib.alvq_separation_masks_f64(one, one, 1, 9, 5, 10, None) == -1 and b"D=9" in lib.alvq_last_error()
    assert lib.alvq_separation_masks_f32(one, None, 1, 2, 5, 10, None) == -1 and b"null" in lib.alvq_last_error()
