"""WPE dereverberation restated in numpy, straight from the definition on alvq_wpe_* in include/alvq.h: float64 with
numpy's Cholesky and scipy's triangular solves, or np.longdouble with a hand-written Cholesky (the yardstick's yardstick).
Also the generator of the tests' inputs: a clean excitation passed through a stable delayed autoregression, which is exactly
the model WPE inverts."""
import collections
import functools

import numpy as np
import scipy.linalg

BAD_POWER, BAD_PIVOT = 1, 2
COND_CAP = 1e6          # the parity bound grows with cond_2(R): the tests' bins stay under this

Case = collections.namedtuple("Case", "S X Y status cond seeds")


def ar_bin(T, D, order, delay, seed, decay=0.7, total=0.8):
    g = np.random.default_rng(seed)
    env = 0.05 + np.abs(np.sin(np.arange(T) * 0.21 + seed)) ** 4 * (1 + (np.arange(T) // 17 % 3))
    S = (g.standard_normal((D, T)) + 1j * g.standard_normal((D, T))) * np.sqrt(env / 2)
    Gk = [(g.standard_normal((D, D)) + 1j * g.standard_normal((D, D))) * decay ** k for k in range(order)]
    tot = sum(np.linalg.norm(G, 2) for G in Gk); Gk = [G * total / tot for G in Gk]
    X = np.zeros((D, T), complex)
    for t in range(T):
        X[:, t] = S[:, t] + sum(Gk[k] @ X[:, t - delay - k] for k in range(order) if t - delay - k >= 0)
    return S, X          # clean, reverberant; stable because the gains' norms sum to 0.8


def bin_seed(index, T, D):
    """The ``index``-th seed of a test tensor's shape."""
    return 7 * index + T + D


def _cholesky(R):
    """Lower Cholesky factor of a Hermitian matrix in its own precision, or None at a pivot <= 0 or not finite."""
    M = R.shape[0]
    L = np.zeros_like(R)
    for k in range(M):
        piv = (R[k, k] - np.sum(L[k, :k] * np.conj(L[k, :k]))).real
        if not (piv > 0 and np.isfinite(piv)):
            return None
        L[k, k] = np.sqrt(piv)
        for i in range(k + 1, M):
            L[i, k] = (R[i, k] - np.sum(L[i, :k] * np.conj(L[k, :k]))) / L[k, k]
    return L


def _solve_lower(L, Bm, conj_transpose=False):
    """L z = Bm, or L^H z = Bm, by substitution in L's precision."""
    M = L.shape[0]
    Z = np.zeros_like(Bm)
    if not conj_transpose:
        for i in range(M):
            Z[i] = (Bm[i] - L[i, :i] @ Z[:i]) / L[i, i]
    else:
        for i in range(M - 1, -1, -1):
            Z[i] = (Bm[i] - np.conj(L[i + 1:, i]) @ Z[i + 1:]) / L[i, i]
    return Z


def stack_past(X, taps, delay):
    """(D taps, T): entry k D + d at frame t is x_d[t - delay - k], 0 before the first frame."""
    D, T = X.shape
    Xt = np.zeros((D * taps, T), X.dtype)
    for k in range(taps):
        s = delay + k
        if s < T:
            Xt[k * D:(k + 1) * D, s:] = X[:, :T - s]
    return Xt


def wpe_bin(X, taps=10, delay=3, iterations=3, psd_context=0, eps=1e-10, loading=1e-10, dtype=np.float64):
    """One bin: X (D, T) complex -> (Y (D, T) complex of ``dtype``'s precision, status, the largest cond_2 of the loaded R
    over the iterations; the condition number is always taken in float64, and is inf where there was no R to take it of)."""
    cdtype = np.complex128 if dtype == np.float64 else np.clongdouble
    X = np.asarray(X).astype(cdtype)
    D, T = X.shape
    M = D * taps
    Xt = stack_past(X, taps, delay)
    Y = X.copy()
    cond = 0.0
    for _ in range(iterations):
        q = np.sum(Y.real ** 2 + Y.imag ** 2, axis=0)
        p = q / dtype(D)                                # psd_context = 0: the frame itself
        for t in range(T if psd_context else 0):
            lo, hi = max(0, t - psd_context), min(T - 1, t + psd_context)
            p[t] = np.sum(q[lo:hi + 1]) / dtype(D * (hi - lo + 1))
        if not np.all(np.isfinite(p)) or np.max(p) == 0:
            return X.copy(), BAD_POWER, np.inf
        lam = np.maximum(p, dtype(eps) * np.max(p))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            Xw = Xt / lam
            R = Xw @ np.conj(Xt.T)
            P = Xw @ np.conj(X.T)
            R = R + dtype(loading) * (np.trace(R).real / dtype(M)) * np.eye(M, dtype=dtype)
        if not (np.all(np.isfinite(R)) and np.all(np.isfinite(P))):
            return X.copy(), BAD_PIVOT, np.inf
        if dtype == np.float64:
            try:
                L = np.linalg.cholesky(R)
            except np.linalg.LinAlgError:
                return X.copy(), BAD_PIVOT, np.inf
            G = scipy.linalg.solve_triangular(L, P, lower=True)
            G = scipy.linalg.solve_triangular(L, G, lower=True, trans="C")
        else:
            L = _cholesky(R)
            if L is None:
                return X.copy(), BAD_PIVOT, np.inf
            G = _solve_lower(L, _solve_lower(L, P), conj_transpose=True)
        cond = max(cond, float(np.linalg.cond(R.astype(np.complex128), 2)))
        Y = X - np.conj(G.T) @ Xt
    return Y, 0, cond


def wpe(X, taps=10, delay=3, iterations=3, psd_context=0, eps=1e-10, loading=1e-10, dtype=np.float64):
    """A tensor: X (B, D, F, T) complex -> (Y of the same shape, status (B, F) int32, cond (B, F) float64)."""
    B, D, F, T = X.shape
    Y = np.zeros(X.shape, np.complex128 if dtype == np.float64 else np.clongdouble)
    status, cond = np.zeros((B, F), np.int32), np.zeros((B, F))
    for b in range(B):
        for f in range(F):
            Y[b, :, f], status[b, f], cond[b, f] = wpe_bin(X[b, :, f], taps, delay, iterations, psd_context, eps, loading, dtype)
    return Y, status, cond


@functools.lru_cache(maxsize=None)
def case(B, D, F, T, taps, delay, psd_context, loading=1e-10, iterations=3, eps=1e-10):
    """A test tensor and its float64 restatement, computed once per shape: ``Case(S, X, Y, status, cond, seeds)`` with S, X, Y
    (B, D, F, T) complex128 and status, cond, seeds (B, F).  Every bin comes from ``ar_bin`` with order min(taps, 6) and a seed
    of its own: the seeds ``bin_seed(0, T, D)``, ``bin_seed(1, T, D)``, ... in turn, bin after bin, passing over a seed whose
    restatement fails or whose cond_2(R) is above ``COND_CAP`` (about one in thirty at taps = 10, D = 1).  The arrays are
    shared between tests: read-only."""
    S, X, Y = (np.zeros((B, D, F, T), complex) for _ in range(3))
    status, cond, seeds = np.zeros((B, F), np.int32), np.zeros((B, F)), np.zeros((B, F), np.int64)
    index = 0
    for b in range(B):
        for f in range(F):
            while True:
                seed = bin_seed(index, T, D)
                index += 1
                s, x = ar_bin(T, D, min(taps, 6), delay, seed)
                y, st, c = wpe_bin(x, taps, delay, iterations, psd_context, eps, loading)
                if st == 0 and c <= COND_CAP:
                    break
            S[b, :, f], X[b, :, f], Y[b, :, f], status[b, f], cond[b, f], seeds[b, f] = s, x, y, st, c, seed
    for arr in (S, X, Y, status, cond, seeds):
        arr.setflags(write=False)
    return Case(S, X, Y, status, cond, seeds)
