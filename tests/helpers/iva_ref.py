"""A numpy float64 restatement of AuxIVA with iterative projection and of the ratio masks as include/alvq.h defines them
(alvq_auxiva_*, alvq_separation_masks_*): plain loops over the bins, for tests/test_iva_cpu.py (which pins it) and
tests/test_iva_gpu.py (which holds csrc/iva.hip to it).  The seeded cases of both live here and are computed once."""
import collections
import functools
import itertools

import numpy as np

U = 1.1e-16
MAX = np.finfo(np.float64).max
KAPPA_CAP = 1e4          # every parity bin's largest cond_2(W V_k) stays under this (asserted by tests/test_iva_cpu.py)
COND_CAP = 1e6           # cond_2(W) of every bin whose projection is compared
MODELS = ("laplace", "gauss")

Iva = collections.namedtuple("Iva", "W Y status kappa")
Case = collections.namedtuple("Case", "X images mix")


# -------------------------------------------------------------------------------------------------------------- definitions
def bin_status(X):
    """(B, F) int32: 1 for a bin that holds a non-finite value or nothing but zeros."""
    finite = np.isfinite(X.real).all(axis=(1, 3)) & np.isfinite(X.imag).all(axis=(1, 3))
    return (~finite | ~(X != 0).any(axis=(1, 3))).astype(np.int32)


def solve(M, rhs):
    """M z = rhs (D, n) by Gaussian elimination with partial pivoting -- the pivot of the largest re^2 + im^2 among the rows
    i >= j, the lowest row on ties -- and back substitution; None where a pivot's re^2 + im^2 is 0 or not finite."""
    m, z = np.array(M, dtype=np.complex128), np.array(rhs, dtype=np.complex128)
    D = m.shape[0]
    with np.errstate(all="ignore"):
        for j in range(D):
            mag = m[:, j].real ** 2 + m[:, j].imag ** 2
            p, best = j, mag[j]
            for i in range(j + 1, D):
                if mag[i] > best:
                    p, best = i, mag[i]
            if not (best > 0.0 and best <= MAX):
                return None
            if p != j:
                m[[j, p]] = m[[p, j]]
                z[[j, p]] = z[[p, j]]
            l = m[j + 1:, j] / m[j, j]
            m[j + 1:, j:] -= l[:, None] * m[j, j:]
            z[j + 1:] -= l[:, None] * z[j]
        for j in range(D - 1, -1, -1):
            z[j] = z[j] / m[j, j]
            z[:j] -= m[:j, j][:, None] * z[j]
    return z


def activity(Xb, Wb, status_b, reverse=False):
    """p (D, T) of one item: sum_f |y_k[f, t]|^2 over the bins whose status is not 1, f rising (falling with reverse)."""
    D, F, T = Xb.shape
    p = np.zeros((D, T))
    order = range(F - 1, -1, -1) if reverse else range(F)
    for f in order:
        if status_b[f] == 1:
            continue
        y = Wb[f] @ Xb[:, f]
        p += y.real ** 2 + y.imag ** 2
    return p


def weights(p, F, model, eps):
    """phi (D, T) from p (D, T)."""
    phi = np.ones_like(p)
    with np.errstate(all="ignore"):
        for k in range(p.shape[0]):
            top = p[k].max() if np.isfinite(p[k]).all() else np.inf
            if not (top > 0.0 and top <= MAX):
                continue
            if model == "laplace":
                r = np.sqrt(p[k])
                phi[k] = 1.0 / np.maximum(r, eps * np.sqrt(top))
            else:
                phi[k] = F / np.maximum(p[k], eps * top)
    return phi


def frame_terms(x):
    """c[i, j, t] = x_i[t] conj(x_j[t]) of x (D, T) with the parts as include/alvq.h takes them: re = x_i.re x_j.re + x_i.im x_j.im,
    im = x_i.im x_j.re - x_i.re x_j.im, every product rounded, so that two identical microphones give an imaginary part of 0."""
    xr, xi = x.real, x.imag
    re = xr[:, None] * xr[None] + xi[:, None] * xi[None]
    im = xi[:, None] * xr[None] - xr[:, None] * xi[None]
    return re + 1j * im


def weighted_cov(x, phi_k, reverse=False, terms=None):
    """V = (1 / T) sum_t phi[t] x_t x_t^H of x (D, T), exactly Hermitian (the lower triangle counts); reverse adds the frames in
    the opposite order.  terms: ``frame_terms(x)`` where the caller has them."""
    c = frame_terms(x) if terms is None else terms
    if reverse:
        c, phi_k = c[..., ::-1], phi_k[::-1]
    V = (c * phi_k).sum(axis=-1) / x.shape[1]
    low = np.tril(V, -1)
    return low + low.conj().T + np.diag(np.diag(V).real)


def project(X, W, status, ref=0):
    """The projection back onto microphone ref: (Y, W, status) with A = W^-1 by ``solve``; a singular W: status 2, W = I, Y = X."""
    B, D, F, T = X.shape
    W, status, Y = W.copy(), status.copy(), X.copy()
    for b in range(B):
        for f in range(F):
            if status[b, f] != 0:
                continue
            A = solve(W[b, f], np.eye(D))
            if A is None:
                status[b, f] = 2
                W[b, f] = np.eye(D)
                continue
            Y[b, :, f] = A[ref][:, None] * (W[b, f] @ X[b, :, f])
    return Y, W, status


def auxiva(X, iterations, model="laplace", ref=0, eps=1e-10, w0=None, reverse=False):
    """``Iva(W, Y, status, kappa)`` of X (B, D, F, T) complex128: the definitions of include/alvq.h.  kappa (B, F): the largest
    cond_2(W V_k) the bin met.  reverse: the frames (in V_k) and the bins (in p) are added in the opposite order."""
    X = np.asarray(X, dtype=np.complex128)
    B, D, F, T = X.shape
    status = bin_status(X)
    eye = np.eye(D, dtype=np.complex128)
    W = np.broadcast_to(eye, (B, F, D, D)).copy() if w0 is None else np.array(w0, dtype=np.complex128)
    W[status == 1] = eye
    kappa = np.zeros((B, F))
    for _ in range(iterations):
        for b in range(B):
            phi = weights(activity(X[b], W[b], status[b], reverse), F, model, eps)
            for f in range(F):
                if status[b, f] != 0:
                    continue
                x = X[b, :, f]
                terms = frame_terms(x)
                for k in range(D):
                    V = weighted_cov(x, phi[k], reverse, terms)
                    M = W[b, f] @ V
                    w = solve(M, eye[:, k:k + 1])
                    q = -1.0
                    if w is not None:
                        w = w[:, 0]
                        with np.errstate(all="ignore"):
                            q = float((w.conj() @ (V @ w)).real)
                    if not (q > 0.0 and q <= MAX):
                        status[b, f] = 2
                        W[b, f] = eye
                        break
                    kappa[b, f] = max(kappa[b, f], np.linalg.cond(M))
                    W[b, f, k] = np.conj(w / np.sqrt(q))
    Y, W, status = project(X, W, status, ref)
    return Iva(W, Y, status, kappa)


def masks(Y):
    """Ratio masks (B, K, F, T) float64 of Y (B, K, F, T)."""
    q = Y.real.astype(np.float64) ** 2 + Y.imag.astype(np.float64) ** 2
    s = q[:, 0].copy()
    for k in range(1, q.shape[1]):
        s = s + q[:, k]
    with np.errstate(all="ignore"):
        m = q / s[:, None]
    m = np.where(np.isfinite(s)[:, None], m, 0.0)
    return np.where((s == 0)[:, None], 1.0 / q.shape[1], m)


# ------------------------------------------------------------------------------------------------------------------ measures
def si_sdr(reference, estimate):
    """Scale-invariant SDR in dB of complex arrays of one shape (the scale is complex)."""
    r, e = reference.ravel(), estimate.ravel()
    target = (np.vdot(r, e) / np.vdot(r, r)) * r
    return 10.0 * np.log10((np.abs(target) ** 2).sum() / (np.abs(e - target) ** 2).sum())


def best_permutation_si_sdr(images, Y):
    """(the SI-SDR of every source under the permutation of Y's sources with the best mean, that permutation): images and Y
    (D, F, T) of one item."""
    D = images.shape[0]
    table = np.array([[si_sdr(images[i], Y[j]) for j in range(D)] for i in range(D)])
    best = max(itertools.permutations(range(D)), key=lambda perm: sum(table[i, perm[i]] for i in range(D)))
    return np.array([table[i, best[i]] for i in range(D)]), best


def improvement(images, mix, Y):
    """Per item: the mean SI-SDR of the best source permutation minus the mean SI-SDR of the mixture against the same images."""
    out = []
    for b in range(images.shape[0]):
        got, _ = best_permutation_si_sdr(images[b], Y[b])
        before = np.mean([si_sdr(images[b, k], mix[b]) for k in range(images.shape[1])])
        out.append(got.mean() - before)
    return np.array(out)


# -------------------------------------------------------------------------------------------------------------------- bounds
def e_ref(shape, model, single=False):
    """The largest relative difference of W between the restatement run forward and with reverse=True."""
    a, b = reference(shape, model, single=single), reference(shape, model, single=single, reverse=True)
    return np.abs(a.W - b.W).max() / np.abs(a.W).max()


def w_tolerance(shape, model, single=False):
    """tol = max(32 e_ref, 2 (T + F + 8 D) u): 32 because one pair of orders is a single sample of reordering noise and the
    device's order is a third; it leaves a decade and a half over that sample."""
    _, D, F, T = shape[:4]
    return max(32 * e_ref(shape, model, single), 2 * (T + F + 8 * D) * U)


def y_bound(X, W, ref):
    """Per output (B, D, F, T): (16 D u cond_2(W) + 2 (D + 2) u) max |A[ref]| sum_d |W[k, d]| |x_d[t]|, and the largest cond_2(W)."""
    B, D, F, T = X.shape
    bound = np.zeros((B, D, F, T))
    worst = 0.0
    for b in range(B):
        for f in range(F):
            cond = np.linalg.cond(W[b, f])
            worst = max(worst, cond)
            amax = np.abs(np.linalg.inv(W[b, f])[ref]).max()
            bound[b, :, f] = (16 * D * U * cond + 2 * (D + 2) * U) * amax * (np.abs(W[b, f]) @ np.abs(X[b, :, f]))
    return bound, worst


# -------------------------------------------------------------------------------------------------------------------- inputs
# (B, D, F, T, iterations, seed): the parity shapes of tests/test_iva_gpu.py, both models.  The seeds are the first of 0, 1, ...
# under which the restatement alone meets the conditions tests/test_iva_cpu.py asserts (kappa <= KAPPA_CAP under both models).
PARITY = [(1, 1, 4, 50, 5, 0),
          (2, 2, 5, 64, 5, 10),             # a whole frame tile of the activity pass
          (2, 2, 9, 200, 5, 1),
          (1, 3, 8, 300, 5, 18),            # past the 256 threads of the projection's and the weights' strides
          (1, 4, 6, 400, 5, 23),
          (1, 8, 3, 600, 5, 82),            # D at its cap
          (1, 2, 3, 2100, 5, 3),           # T above every frame tiling: 64 (activity, covariance lanes), 256 (weights, projection)
          (1, 2, 201, 500, 3, 1)]          # the dataset's own F and T
SEPARATION = [(2, 2, 9, 200, 30, 0), (1, 3, 8, 300, 30, 0)]      # "laplace"
IDS = ["-".join(str(v) for v in s[:4]) for s in PARITY]


@functools.lru_cache(maxsize=None)
def case(B, D, F, T, seed, ref=0):
    """``Case(X, images, mix)``: per source a per-frame activity shared by all bins, gamma(0.3) + 1e-3, times complex Gaussian
    noise, mixed by a random complex D x D matrix per bin.  X (B, D, F, T) complex128; images (B, D, F, T): source k as
    microphone ref hears it; mix (B, F, T) = X[:, ref].  Shared between tests: read-only."""
    g = np.random.default_rng([seed, B, D, F, T])

    def gauss(*shape):
        return g.standard_normal(shape) + 1j * g.standard_normal(shape)
    act = g.gamma(0.3, size=(B, D, 1, T)) + 1e-3
    S = act * gauss(B, D, F, T)
    A = gauss(B, F, D, D)
    X = np.einsum("bfdk,bkft->bdft", A, S)
    images = np.moveaxis(A[:, :, ref, :], 2, 1)[..., None] * S
    mix = X[:, ref].copy()
    for a in (X, images, mix):
        a.setflags(write=False)
    return Case(X, images, mix)


def parity_case(shape):
    B, D, F, T, _, seed = shape
    return case(B, D, F, T, seed)


def promoted(X, single):
    """The input the kernels see: rounded to complex64 and promoted again where single."""
    return X.astype(np.complex64).astype(np.complex128) if single else X


@functools.lru_cache(maxsize=None)
def reference(shape, model, single=False, reverse=False):
    """The restatement of a parity or separation shape, computed once; its arrays are read-only."""
    out = auxiva(promoted(parity_case(shape).X, single), shape[4], model, reverse=reverse)
    for a in out:
        a.setflags(write=False)
    return out
