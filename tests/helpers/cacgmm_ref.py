"""A numpy float64 restatement of the cACGMM mask estimator as include/alvq.h defines it (alvq_cacgmm_*): plain loops over the
items, bins and classes and numpy.linalg.eigh, for tests/test_cacgmm_cpu.py (which pins it) and tests/test_cacgmm_gpu.py (which
holds csrc/cacgmm.hip to it).  The seeded cases of both live here and are computed once."""
import collections
import functools
import itertools

import numpy as np

U = 1.1e-16
MAX = np.finfo(np.float64).max
TINY = np.finfo(np.float64).tiny
TOL_CAP = 1e-9           # every parity case's tolerance stays under this (asserted by tests/test_cacgmm_cpu.py)
COND_CAP = 1e6           # lambda_max / lambda_min of every class matrix of a parity case
# |cov_dev - cov_ref| <= C_COV tol cond per class matrix.  The restatement's own forward / reverse pair gives
# |cov_fwd - cov_rev| / (tol cond) between 2.1e-6 and 9.7e-3 over the parity cases and both dtypes; C_COV is 32 times the cap
# tests/test_cacgmm_cpu.py asserts on that ratio.
COV_RATIO_CAP = 1e-2
C_COV = 32 * COV_RATIO_CAP

Gmm = collections.namedtuple("Gmm", "masks prior cov quadratic status cond")
Case = collections.namedtuple("Case", "X oracle images init")


# -------------------------------------------------------------------------------------------------------------- definitions
def norms(x):
    """|x|^2 (T,) of x (D, T): re^2 + im^2 added with d rising."""
    n = np.zeros(x.shape[1])
    for d in range(x.shape[0]):
        n = n + (x[d].real * x[d].real + x[d].imag * x[d].imag)
    return n


def bin_status(X, init, quadratic0):
    """(B, F) int32: 1 for a bin with a non-finite value, a frame whose |x|^2 is not finite, an init value that is negative or
    not finite, or a quadratic0 value that is not > 0 and finite."""
    B, D, F, T = X.shape
    st = np.zeros((B, F), np.int32)
    with np.errstate(all="ignore"):
        for b in range(B):
            for f in range(F):
                x = X[b, :, f]
                bad = not (np.isfinite(x.real).all() and np.isfinite(x.imag).all() and np.isfinite(norms(x)).all())
                g = init[b, :, f]
                bad = bad or not ((g >= 0).all() and np.isfinite(g).all())
                if quadratic0 is not None:
                    q = quadratic0[b, :, f]
                    bad = bad or not ((q > 0).all() and np.isfinite(q).all())
                st[b, f] = 1 if bad else 0
    return st


def frame_terms(x):
    """c[i, j, t] = x_i[t] conj(x_j[t]) with the parts as include/alvq.h takes them (iva_ref.frame_terms' rule)."""
    xr, xi = x.real, x.imag
    re = xr[:, None] * xr[None] + xi[:, None] * xi[None]
    im = xi[:, None] * xr[None] - xr[:, None] * xi[None]
    return re + 1j * im


def class_matrix(terms, n, gamma, q, reverse=False):
    """B_k (D, D) = D sum_t (gamma / (q |x|^2)) x x^H / sum_t gamma over the live frames, exactly Hermitian (the lower triangle
    counts), or None where sum_t gamma is not > 0.  reverse adds the frames in the opposite order."""
    D = terms.shape[0]
    live = n > 0
    with np.errstate(all="ignore"):
        w = np.where(live, gamma / (q * np.where(live, n, 1.0)), 0.0)
    g = np.where(live, gamma, 0.0)
    c = terms
    if reverse:
        c, w, g = c[..., ::-1], w[::-1], g[::-1]
    sg = g.sum()
    if not sg > 0:
        return None
    Bk = (c * w).sum(axis=-1) * D / sg
    low = np.tril(Bk, -1)
    return low + low.conj().T + np.diag(np.diag(Bk).real)


def m_step(Bk, D, floor):
    """(lambda (D,) ascending after the floor and the normalisation, V, logdet) of a class matrix, or None for a failure."""
    if Bk is None:
        return np.ones(D), np.eye(D, dtype=np.complex128), 0.0
    if not (np.isfinite(Bk.real).all() and np.isfinite(Bk.imag).all()):
        return None
    lam, V = np.linalg.eigh(Bk)
    top = lam[-1]
    if not (top > 0 and top <= MAX):
        return None
    lam = np.maximum(lam, floor * top)
    s = 0.0
    for i in range(D):
        s = s + lam[i]
    lam = lam * D / s
    logdet = 0.0
    for i in range(D):
        logdet = logdet + np.log(lam[i])
    return lam, V, logdet


def priors(gamma_b, status_b, reverse=False):
    """prior (K, T) of one item: the mean of gamma over its bins of status 0, f rising (falling with reverse); 1 / K without one."""
    K, F, T = gamma_b.shape
    p = np.zeros((K, T))
    order = range(F - 1, -1, -1) if reverse else range(F)
    count = 0
    for f in order:
        if status_b[f] == 0:
            p = p + gamma_b[:, f]
            count += 1
    return p / count if count else np.full((K, T), 1.0 / K)


def cacgmm(X, init, iterations, quadratic0=None, floor=1e-10, reverse=False):
    """``Gmm(masks, prior, cov, quadratic, status, cond)`` of X (B, D, F, T) complex128 and init (B, K, F, T): the definitions of
    include/alvq.h.  cond (B, F, K): lambda_max / lambda_min of the last class matrices.  reverse: the frames (in B_k) and the bins
    (in the priors) are added in the opposite order."""
    X = np.asarray(X, dtype=np.complex128)
    B, D, F, T = X.shape
    K = init.shape[1]
    status = bin_status(X, init, quadratic0)
    gamma = np.array(init, dtype=np.float64)
    q = np.ones((B, K, F, T)) if quadratic0 is None else np.array(quadratic0, dtype=np.float64)
    prior = np.full((B, K, T), 1.0 / K)
    cov = np.broadcast_to(np.eye(D, dtype=np.complex128), (B, F, K, D, D)).copy()
    cond = np.ones((B, F, K))
    for _ in range(iterations):
        for b in range(B):
            prior[b] = priors(gamma[b], status[b], reverse)
            with np.errstate(all="ignore"):
                logp = np.log(prior[b])
            for f in range(F):
                if status[b, f] != 0:
                    continue
                x = X[b, :, f]
                n = norms(x)
                live = n > 0
                terms = frame_terms(x)
                l = np.zeros((K, T))
                qn = np.ones((K, T))
                for k in range(K):
                    out = m_step(class_matrix(terms, n, gamma[b, k, f], q[b, k, f], reverse), D, floor)
                    if out is None:
                        status[b, f] = 2
                        break
                    lam, V, logdet = out
                    vv = frame_terms(V)                                          # vv[r, c, i] = V[r, i] conj(V[c, i])
                    cov[b, f, k] = 0
                    for i in range(D):
                        cov[b, f, k] += lam[i] * vv[:, :, i]
                    cond[b, f, k] = lam[-1] / lam[0]
                    y = (V.conj().T / np.sqrt(lam)[:, None]) @ x                 # row i: v_i^H x / sqrt(lambda_i)
                    s = np.zeros(T)
                    for i in range(D):
                        s = s + (y[i].real * y[i].real + y[i].imag * y[i].imag)
                    with np.errstate(all="ignore"):
                        qn[k] = np.maximum(s / np.where(live, n, 1.0), TINY)
                        l[k] = logp[k] - logdet - D * np.log(qn[k])
                if status[b, f] != 0:
                    continue
                top = l.max(axis=0)
                with np.errstate(all="ignore"):
                    e = np.exp(l - top)
                s = np.zeros(T)
                for k in range(K):
                    s = s + e[k]
                with np.errstate(all="ignore"):
                    g = np.where(top > -MAX, e / s, 1.0 / K)
                gamma[b, :, f] = np.where(live, g, prior[b])
                q[b, :, f] = np.where(live, qn, 1.0)
    dead = status != 0
    gamma = np.moveaxis(gamma, 1, 2)
    gamma[dead] = 1.0 / K
    gamma = np.moveaxis(gamma, 2, 1)
    q = np.moveaxis(q, 1, 2)
    q[dead] = 1.0
    q = np.moveaxis(q, 2, 1)
    cov[dead] = np.eye(D)
    return Gmm(np.ascontiguousarray(gamma), prior, cov, np.ascontiguousarray(q), status, cond)


# ------------------------------------------------------------------------------------------------------------------ measures
def agreement(m, o):
    """(A, permutation) of masks m against oracle masks o, both (K, F, T) of one item: the mean over (f, t) of
    sum_k m[perm[k]] o[k] under the ONE permutation of the item that makes it largest."""
    K = m.shape[0]
    table = np.array([[(m[j] * o[k]).mean() for j in range(K)] for k in range(K)])         # table[k, j]: o_k with m_j
    best = max(itertools.permutations(range(K)), key=lambda perm: sum(table[k, perm[k]] for k in range(K)))
    return sum(table[k, best[k]] for k in range(K)), best


def si_sdr(reference, estimate):
    """Scale-invariant SDR in dB of complex arrays of one shape (the scale is complex)."""
    r, e = reference.ravel(), estimate.ravel()
    target = (np.vdot(r, e) / np.vdot(r, r)) * r
    return 10.0 * np.log10((np.abs(target) ** 2).sum() / (np.abs(e - target) ** 2).sum())


# -------------------------------------------------------------------------------------------------------------------- bounds
def e_ref(shape, single=False):
    """The largest difference of the masks between the restatement run forward and with reverse=True."""
    a, b = reference(shape, single=single), reference(shape, single=single, reverse=True)
    return np.abs(a.masks - b.masks).max()


def tolerance(shape, single=False):
    """tol = max(32 e_ref, 2 (T + F + 8 D) u): 32 because one pair of orders is a single sample of reordering noise and the
    device's order is a third."""
    _, D, _, F, T = shape[:5]
    return max(32 * e_ref(shape, single), 2 * (T + F + 8 * D) * U)


def cov_ratio(shape, single=False):
    """The largest |cov_fwd - cov_rev| / (tol cond) over the class matrices of a case: what the cov bound's factor is measured on."""
    a, b = reference(shape, single=single), reference(shape, single=single, reverse=True)
    d = np.abs(a.cov - b.cov).max(axis=(-2, -1))
    return (d / (tolerance(shape, single) * a.cond)).max()


# -------------------------------------------------------------------------------------------------------------------- inputs
# (B, D, K, F, T, iterations, seed): the parity shapes of tests/test_cacgmm_gpu.py.  The seeds are the first of 0, 1, ... under
# which the restatement alone meets the conditions tests/test_cacgmm_cpu.py asserts (tol <= TOL_CAP, cond <= COND_CAP, both dtypes).
PARITY = [(1, 2, 1, 3, 50, 5, 0),
          (2, 2, 2, 5, 64, 5, 0),
          (2, 3, 2, 9, 200, 5, 0),
          (1, 4, 3, 8, 300, 5, 0),            # past 256-thread strides
          (1, 8, 8, 3, 600, 5, 0),            # both caps
          (1, 2, 2, 3, 2100, 5, 0),           # T above every tiling
          (1, 4, 3, 201, 500, 3, 0)]          # the dataset's own F and T
# the seeds are the first of 0, 1, ... under which the restatement meets the agreement conditions of tests/test_cacgmm_cpu.py
SEPARATION = [(1, 4, 2, 9, 200, 20, 0), (1, 3, 2, 65, 200, 20, 0)]
IDS = ["-".join(str(v) for v in s[:5]) for s in PARITY]
SEP_IDS = ["-".join(str(v) for v in s[:5]) for s in SEPARATION]


def time_masks(g, B, K, F, T):
    """separation.time_masks' rule with a numpy generator: uniform(0, 1) + 1e-3 per (b, k, t), normalised over k, repeated over f."""
    m = g.random((B, K, 1, T)) + 1e-3
    m = m / m.sum(axis=1, keepdims=True)
    return np.ascontiguousarray(np.broadcast_to(m, (B, K, F, T)))


@functools.lru_cache(maxsize=None)
def case(B, D, K, F, T, seed, ref=0):
    """``Case(X, oracle, images, init)``: K sources with a per-frame activity shared by all bins, gamma(0.3) + 1e-3, times complex
    Gaussian noise, mixed by a random complex D x K matrix per bin, plus complex Gaussian noise at 0.05.  X (B, D, F, T)
    complex128; oracle (B, K, F, T): the ratio masks of the sources' powers summed over the microphones; images (B, K, F, T):
    source k as microphone ref hears it; init (B, K, F, T).  Shared between tests: read-only."""
    g = np.random.default_rng([seed, B, D, K, F, T])

    def gauss(*shape):
        return g.standard_normal(shape) + 1j * g.standard_normal(shape)
    act = g.gamma(0.3, size=(B, K, 1, T)) + 1e-3
    S = act * gauss(B, K, F, T)
    A = gauss(B, F, D, K)
    X = np.einsum("bfdk,bkft->bdft", A, S) + 0.05 * gauss(B, D, F, T)
    power = np.einsum("bfdk,bkft->bkft", np.abs(A) ** 2, np.abs(S) ** 2)
    oracle = power / power.sum(axis=1, keepdims=True)
    images = np.moveaxis(A[:, :, ref, :], 2, 1)[..., None] * S
    init = time_masks(g, B, K, F, T)
    for a in (X, oracle, images, init):
        a.setflags(write=False)
    return Case(X, oracle, images, init)


def parity_case(shape):
    B, D, K, F, T, _, seed = shape
    return case(B, D, K, F, T, seed)


def promoted(X, single):
    """The input the kernels see: rounded to complex64 and promoted again where single."""
    return X.astype(np.complex64).astype(np.complex128) if single else X


@functools.lru_cache(maxsize=None)
def reference(shape, single=False, reverse=False):
    """The restatement of a parity or separation shape, computed once; its arrays are read-only."""
    c = parity_case(shape)
    out = cacgmm(promoted(c.X, single), c.init, shape[5], reverse=reverse)
    for a in out:
        a.setflags(write=False)
    return out
