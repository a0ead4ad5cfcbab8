"""A numpy float64 restatement of ILRMA as include/alvq.h defines it (alvq_ilrma_*): plain loops over the bins, for
tests/test_ilrma_cpu.py (which pins it) and tests/test_ilrma_gpu.py (which holds csrc/ilrma.hip to it).  The elimination, the
frame terms, the weighted covariance, the projection and the SI-SDR measures are iva_ref's.  The seeded cases of both test files
live here and are computed once."""
import collections
import functools

import numpy as np

import iva_ref as IR

U = IR.U
MAX = IR.MAX
KAPPA_CAP = IR.KAPPA_CAP
COND_CAP = IR.COND_CAP
FLOOR = 1e-10

Ilrma = collections.namedtuple("Ilrma", "W basis activations Y status kappa floored")
Case = collections.namedtuple("Case", "X images mix")


# -------------------------------------------------------------------------------------------------------------- definitions
def positive(a):
    return np.isfinite(a) & (a > 0)


def floored(v, floor, seen=None):
    """v where v > floor and v is finite, floor otherwise; seen["floor"] counts the entries it replaced."""
    with np.errstate(all="ignore"):
        keep = np.isfinite(v) & (v > floor)
    if seen is not None:
        seen["floor"] = seen.get("floor", 0) + int((~keep).sum())
    return np.where(keep, v, floor)


def start_status(X, basis0, activations0):
    """(B, F) int32: iva_ref's status 1, and 1 for a bin whose basis0 rows hold a value that is not finite or not > 0 and for
    every bin of an item whose activations0 do."""
    status = IR.bin_status(X)
    status[~positive(basis0).all(axis=(1, 3))] = 1
    status[~positive(activations0).all(axis=(1, 2, 3))] = 1
    return status


def total(a, axis, reverse):
    """The sum along an axis, taken from the other end with reverse."""
    return np.flip(a, axis).sum(axis=axis) if reverse else a.sum(axis=axis)


def power(Xb, Wb, status_b):
    """P (D, F, T) of one item: |y_k[f, t]|^2 in the bins whose status is not 1 (0 elsewhere; never read)."""
    D, F, T = Xb.shape
    P = np.zeros((D, F, T))
    for f in range(F):
        if status_b[f] != 1:
            y = Wb[f] @ Xb[:, f]
            P[:, f] = y.real ** 2 + y.imag ** 2
    return P


def scale(P, status_b, reverse=False):
    """lam (D,): the mean of P over the bins whose status is not 1 and their frames, f rising; 1 where not finite or not > 0."""
    D, F, T = P.shape
    live = [f for f in range(F) if status_b[f] != 1]
    rows = total(P, 2, reverse)
    s = np.zeros(D)
    for f in (live[::-1] if reverse else live):
        s = s + rows[:, f]
    with np.errstate(all="ignore"):
        lam = s / (float(len(live)) * float(T))
    return np.where(positive(lam), lam, 1.0)


def normalise(Wb, P, basis_b, lam, status_b, floor, seen=None):
    """Step 2: (W, P, basis) of one item, normalised."""
    Wb, P, basis_b = Wb.copy(), P.copy(), basis_b.copy()
    for f in range(P.shape[1]):
        if status_b[f] == 0:
            Wb[f] = Wb[f] / np.sqrt(lam)[:, None]
        if status_b[f] != 1:
            P[:, f] = P[:, f] / lam[:, None]
            basis_b[:, f] = floored(basis_b[:, f] / lam[:, None], floor, seen)
    return Wb, P, basis_b


def variance(basis_b, act_b, floor, seen=None):
    """R (D, F, T) = floor(sum_l basis[k, f, l] activations[k, l, t]), l rising from the first product."""
    L = basis_b.shape[2]
    with np.errstate(all="ignore"):
        R = basis_b[:, :, 0, None] * act_b[:, None, 0]
        for l in range(1, L):
            R = R + basis_b[:, :, l, None] * act_b[:, None, l]
    return floored(R, floor, seen)


def updated(v, num, den, floor, seen=None):
    with np.errstate(all="ignore"):
        ratio = num / den
        new = np.where(np.isfinite(ratio), v * np.sqrt(ratio), v)
    return floored(new, floor, seen)


def update_basis(P, basis_b, act_b, status_b, floor, reverse=False, seen=None):
    """Step 3 on normalised P and basis."""
    R = variance(basis_b, act_b, floor, seen)
    inv = 1.0 / R
    g = (P * inv) * inv
    num = total(g[:, :, None, :] * act_b[:, None], 3, reverse)               # (D, F, L)
    den = total(inv[:, :, None, :] * act_b[:, None], 3, reverse)
    new = updated(basis_b, num, den, floor, seen)
    out = basis_b.copy()
    live = status_b != 1
    out[:, live] = new[:, live]
    return out


def update_activations(P, basis_b, act_b, status_b, floor, reverse=False, seen=None):
    """Step 4: the sums over the bins whose status is not 1, f rising."""
    D, F, T = P.shape
    L = act_b.shape[1]
    R = variance(basis_b, act_b, floor, seen)
    with np.errstate(all="ignore"):
        inv = 1.0 / R
        g = (P * inv) * inv
    num, den = np.zeros((D, L, T)), np.zeros((D, L, T))
    live = [f for f in range(F) if status_b[f] != 1]
    for f in (live[::-1] if reverse else live):
        num = num + g[:, f, None, :] * basis_b[:, f, :, None]
        den = den + inv[:, f, None, :] * basis_b[:, f, :, None]
    return updated(act_b, num, den, floor, seen)


def update_demixing(Xb, Wb, basis_b, act_b, status_b, kappa_b, floor, reverse=False, seen=None):
    """Step 5, in place on (W, status, kappa) of one item: iva_ref.auxiva's update with phi[k, t] = 1 / R[k, f, t]."""
    D, F, T = Xb.shape
    eye = np.eye(D, dtype=np.complex128)
    R = variance(basis_b, act_b, floor, seen)
    for f in range(F):
        if status_b[f] != 0:
            continue
        x = Xb[:, f]
        terms = IR.frame_terms(x)
        for k in range(D):
            V = IR.weighted_cov(x, 1.0 / R[k, f], reverse, terms)
            M = Wb[f] @ V
            w = IR.solve(M, eye[:, k:k + 1])
            q = -1.0
            if w is not None:
                w = w[:, 0]
                with np.errstate(all="ignore"):
                    q = float((w.conj() @ (V @ w)).real)
            if not (q > 0.0 and q <= MAX):
                status_b[f] = 2
                Wb[f] = eye
                break
            kappa_b[f] = max(kappa_b[f], np.linalg.cond(M))
            Wb[f, k] = np.conj(w / np.sqrt(q))


def cost(Xb, Wb, basis_b, act_b, status_b, floor=FLOOR):
    """sum_{f, t, k} (P / R + log R) - 2 T sum_f log |det W_f| of one item, over the bins whose status is not 1."""
    T = Xb.shape[2]
    P = power(Xb, Wb, status_b)
    R = variance(basis_b, act_b, floor)
    live = status_b != 1
    fit = (P[:, live] / R[:, live] + np.log(R[:, live])).sum()
    return fit - 2.0 * T * sum(np.log(abs(np.linalg.det(Wb[f]))) for f in range(len(status_b)) if live[f])


def iterate(Xb, Wb, basis_b, act_b, status_b, kappa_b, floor=FLOOR, reverse=False, seen=None):
    """One iteration of one item: the new (W, basis, activations); status_b and kappa_b are updated in place."""
    P = power(Xb, Wb, status_b)
    lam = scale(P, status_b, reverse)
    Wb, P, basis_b = normalise(Wb, P, basis_b, lam, status_b, floor, seen)
    basis_b = update_basis(P, basis_b, act_b, status_b, floor, reverse, seen)
    act_b = update_activations(P, basis_b, act_b, status_b, floor, reverse, seen)
    update_demixing(Xb, Wb, basis_b, act_b, status_b, kappa_b, floor, reverse, seen)
    return Wb, basis_b, act_b


def ilrma(X, basis0, activations0, iterations, ref=0, floor=FLOOR, w0=None, reverse=False):
    """``Ilrma(W, basis, activations, Y, status, kappa, floored)`` of X (B, D, F, T) complex128: the definitions of
    include/alvq.h.  kappa (B, F): the largest cond_2(W V_k) the bin met; floored: how many values the floor replaced.  reverse:
    the frames and the bins are added in the opposite order in every sum."""
    X = np.asarray(X, dtype=np.complex128)
    B, D, F, T = X.shape
    basis, act = np.array(basis0, dtype=np.float64), np.array(activations0, dtype=np.float64)
    status = start_status(X, basis, act)
    eye = np.eye(D, dtype=np.complex128)
    W = np.broadcast_to(eye, (B, F, D, D)).copy() if w0 is None else np.array(w0, dtype=np.complex128)
    W[status == 1] = eye
    kappa = np.zeros((B, F))
    seen = {}
    for _ in range(iterations):
        for b in range(B):
            W[b], basis[b], act[b] = iterate(X[b], W[b], basis[b], act[b], status[b], kappa[b], floor, reverse, seen)
    Y, W, status = IR.project(X, W, status, ref)
    return Ilrma(W, basis, act, Y, status, kappa, seen.get("floor", 0))


# -------------------------------------------------------------------------------------------------------------------- inputs
# (B, D, F, T, L, iterations, seed): the parity shapes of tests/test_ilrma_gpu.py.  The seeds are the first of 0, 1, ... under
# which the restatement alone meets the conditions tests/test_ilrma_cpu.py asserts.
PARITY = [(1, 1, 4, 50, 1, 5, 0),
          (2, 2, 5, 64, 2, 5, 0),               # a whole 64-frame tile
          (2, 2, 9, 200, 3, 5, 0),
          (1, 3, 8, 300, 2, 5, 0),              # past 256 threads
          (1, 8, 3, 600, 2, 5, 5),              # D at its cap
          (1, 2, 6, 130, 16, 5, 0),             # L at its cap
          (1, 2, 3, 2100, 2, 5, 0),             # T above every tiling
          (1, 2, 201, 500, 2, 3, 2)]            # the dataset's own F and T
SEPARATION = [(2, 2, 16, 200, 2, 30, 0), (1, 3, 12, 300, 2, 30, 0)]
IDS = ["-".join(str(v) for v in s[:5]) for s in PARITY]
SEPARATION_IDS = ["-".join(str(v) for v in s[:5]) for s in SEPARATION]
SOURCE_RANK = 2


@functools.lru_cache(maxsize=None)
def case(B, D, F, T, seed, ref=0):
    """``Case(X, images, mix)``: per source a power of rank 2 over (f, t), its factors gamma(0.3) + 1e-3, whose square root
    scales complex Gaussian noise; mixed by a random complex D x D matrix per bin.  X (B, D, F, T) complex128; images
    (B, D, F, T): source k as microphone ref hears it; mix (B, F, T) = X[:, ref].  Shared between tests: read-only."""
    g = np.random.default_rng([seed, B, D, F, T])

    def gauss(*shape):
        return g.standard_normal(shape) + 1j * g.standard_normal(shape)
    bf = g.gamma(0.3, size=(B, D, F, SOURCE_RANK)) + 1e-3
    at = g.gamma(0.3, size=(B, D, SOURCE_RANK, T)) + 1e-3
    S = np.sqrt(bf @ at) * gauss(B, D, F, T)
    A = gauss(B, F, D, D)
    X = np.einsum("bfdk,bkft->bdft", A, S)
    images = np.moveaxis(A[:, :, ref, :], 2, 1)[..., None] * S
    mix = X[:, ref].copy()
    for a in (X, images, mix):
        a.setflags(write=False)
    return Case(X, images, mix)


@functools.lru_cache(maxsize=None)
def start(B, D, F, T, L, seed):
    """(basis0 (B, D, F, L), activations0 (B, D, L, T)): uniform(0, 1) + 1e-3, as ``separation.nmf_init`` draws; read-only."""
    g = np.random.default_rng([seed, B, D, F, T, L, 1])
    out = g.random((B, D, F, L)) + 1e-3, g.random((B, D, L, T)) + 1e-3
    for a in out:
        a.setflags(write=False)
    return out


def parity_case(shape):
    B, D, F, T, _, _, seed = shape
    return case(B, D, F, T, seed)


def parity_start(shape):
    B, D, F, T, L, _, seed = shape
    return start(B, D, F, T, L, seed)


promoted = IR.promoted


def bad_inputs(shape):
    """The status tests' inputs, one item more than the shape's: a bin of zeros, a bin with one NaN, a bin whose basis0 row
    holds a 0, and (the last item) an item whose activations0 hold a NaN -> (X, basis0, activations0, the status they must get)."""
    B, D, F, T, L = shape[:5]
    X = np.concatenate([parity_case(shape).X, case(1, D, F, T, 77).X])
    b0 = np.concatenate([parity_start(shape)[0], start(1, D, F, T, L, 77)[0]])
    a0 = np.concatenate([parity_start(shape)[1], start(1, D, F, T, L, 77)[1]])
    X[0, :, 1] = 0
    X[1, 1, 3, 40] = complex(np.nan, 1.0)
    b0[0, 1, 6, 0] = 0.0
    a0[B, 0, 1, 7] = np.nan
    want = np.zeros((B + 1, F), np.int32)
    want[0, 1] = want[1, 3] = want[0, 6] = 1
    want[B] = 1
    return X, b0, a0, want


@functools.lru_cache(maxsize=None)
def reference(shape, single=False, reverse=False):
    """The restatement of a parity or separation shape, computed once; its arrays are read-only."""
    out = ilrma(promoted(parity_case(shape).X, single), *parity_start(shape), shape[5], reverse=reverse)
    for a in out[:6]:
        a.setflags(write=False)
    return out


# -------------------------------------------------------------------------------------------------------------------- bounds
def difference(a, b):
    """The largest relative max-norm difference of W, basis and activations between two runs."""
    return max(np.abs(x - y).max() / np.abs(x).max() for x, y in zip(a[:3], b[:3]))


def e_ref(shape, single=False):
    return difference(reference(shape, single), reference(shape, single, reverse=True))


def tolerance_of(e, D, F, T, L):
    """tol = max(32 e_ref, 2 (T + F + 8 D + L) u); 32 for the reason iva_ref.w_tolerance gives."""
    return max(32 * e, 2 * (T + F + 8 * D + L) * U)


def tolerance(shape, single=False):
    _, D, F, T, L = shape[:5]
    return tolerance_of(e_ref(shape, single), D, F, T, L)
