"""The Hermitian eigendecomposition, the MUSIC null spectrum and the GEV beamformer restated in numpy, straight from the
definitions on alvq_eigh_f64 / alvq_music_f64 / alvq_beamform_gev_f64 in include/alvq.h: in float64, or in np.longdouble (the
yardstick's yardstick).  The Jacobi sweeps here run row by row over the pairs, not in the kernel's round-robin order, and
every sum is numpy's own: every bound below holds for any order.  Also the generators of the tests' inputs and the error
bounds the CPU and the GPU tests share.

The bounds, with u = 1.1e-16:
  eigensolver   max |A V - V diag(lam)| <= c1 D u ||A||_F,  max |V^H V - I| <= c1 D u,  max |lam - lam_ref| <= c1 D u ||A||_F;
                eigenvectors are compared only through the projector onto the span of the K last: <= 2 c1 D u ||A||_F / gap, gap
                the distance between the eigenvalues on either side of the split (Davis, Kahan 1970: the sine of the angle
                between the subspaces is at most the perturbation over the gap, and a projector's error is twice that at most)
  map alone     |null - null_ref| <= (D K + 16 Theta + 32 + anchor) u: K sums of D unit-modulus terms against unit vectors, the
                phase error of srp_ref.map_bound (Theta = srp_ref.theta_max), its slack and the K-term of its recurrence
  chain         the map-alone bound plus the mean over the band of 2 c1 D u ||Phi||_F / gap_f
  GEV           max |w - w_ref| <= c2 D u cond_2(Phi') (1 + ||C||_F / gap_C) max |w_ref|, the same for rtf: a Cholesky solve's
                forward bound (beamform_ref.weights_bound) times the eigenvector's sensitivity
How c1 and c2 were set: tests/test_subspace_cpu.py measures float64 against longdouble over every parity case and prints the
worst ratio; the constant is the next power of two at or above 4 x that ratio.  The GPU tests use twice the constant: a bound is
spent once for each side."""
import collections
import functools

import numpy as np

import beamform_ref as BR
import srp_ref

LD = np.longdouble
FS, C = srp_ref.FS, srp_ref.C
U = 1.1e-16
MAX_SWEEPS = 16
EIG_BAD_INPUT, EIG_NO_CONVERGENCE = 1, 2
BAD_SPECTRUM, SILENT, BAD_GEOMETRY = 1, 2, 4
BAD_SOLVE = 2
ANCHOR = srp_ref.ANCHOR

C1_MEASURED = 4.34      # the worst ratio of float64 to longdouble over the eigensolver's cases (the orthogonality of V)
C2_MEASURED = 0.298     # the same over the GEV cases
C1 = 32                 # the next power of two at or above 4 x 4.34 = 17.3
C2 = 2                  # ... at or above 4 x 0.298 = 1.19
# tests/test_subspace_cpu.py::test_constants_are_four_times_the_measured_ratio measures both again and holds C1, C2 to the rule

Eig = collections.namedtuple("Eig", "lam V status")
Gev = collections.namedtuple("Gev", "W rtf gain status")


def _types(dtype):
    return (np.float64, np.complex128) if dtype == np.float64 else (LD, np.clongdouble)


def _unit_roundoff(dtype):
    return 2.0 ** -53 if dtype == np.float64 else LD(2) ** -64


# ---------------------------------------------------------------------------------------------------------- eigendecomposition
def hermitian(A, dtype=np.float64):
    """The matrix the solver works on: the lower triangle, its conjugate above, the real part of the diagonal."""
    real, cplx = _types(dtype)
    M = np.asarray(A).astype(cplx)
    low = np.tril(M, -1)
    D = M.shape[-1]
    eye = np.eye(D, dtype=real)
    return low + np.conj(np.swapaxes(low, -1, -2)) + (np.diagonal(M, axis1=-2, axis2=-1).real[..., None] * eye).astype(cplx)


def eigh(A, dtype=np.float64, max_sweeps=MAX_SWEEPS):
    """A (..., D, D) -> ``Eig(lam (..., D) ascending, V (..., D, D) columns with the phase rule, status (...))`` as the header
    defines them; the pairs are visited row by row."""
    real, cplx = _types(dtype)
    A = np.asarray(A)
    lead, D = A.shape[:-2], A.shape[-1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        H = hermitian(A.reshape((-1, D, D)), dtype)
        n = H.shape[0]
        bad = ~(np.isfinite(H.real) & np.isfinite(H.imag)).all(axis=(1, 2))
        H[bad] = 0
        V = np.broadcast_to(np.eye(D, dtype=cplx), (n, D, D)).copy()
        mx = np.maximum(np.abs(H.real), np.abs(H.imag)).max(axis=(1, 2))
        safe = np.where(mx > 0, mx, real(1))
        S = H / safe[:, None, None]
        nf = mx * np.sqrt(np.sum(S.real * S.real + S.imag * S.imag, axis=(1, 2)))
        thr = real(0.5) * _unit_roundoff(dtype) * nf / real(D)
        done = (mx == 0) | (D == 1) | bad
        for _ in range(max_sweeps):
            rotated = np.zeros(n, bool)
            for p in range(D - 1):
                for q in range(p + 1, D):
                    g = H[:, p, q]
                    absg = np.hypot(g.real, g.imag)
                    idx = np.nonzero((absg > thr) & ~done)[0]
                    if idx.size == 0:
                        continue
                    alpha, beta, gg, ag = H[idx, p, p].real, H[idx, q, q].real, g[idx], absg[idx]
                    zeta = (beta - alpha) / (2 * ag)
                    t = np.where(zeta >= 0, real(1), real(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                    cs = 1 / np.sqrt(1 + t * t)
                    sn = (cs * t) * (gg / ag)
                    cs_, sn_ = cs[:, None], sn[:, None]
                    for M in (H, V):                                       # M <- M J
                        cp, cq = M[idx, :, p].copy(), M[idx, :, q].copy()
                        M[idx, :, p] = cs_ * cp - np.conj(sn_) * cq
                        M[idx, :, q] = sn_ * cp + cs_ * cq
                    rp, rq = H[idx, p, :].copy(), H[idx, q, :].copy()     # H <- J^H H
                    H[idx, p, :] = cs_ * rp - sn_ * rq
                    H[idx, q, :] = np.conj(sn_) * rp + cs_ * rq
                    H[idx, p, q] = 0
                    H[idx, q, p] = 0
                    H[idx, p, p] = alpha - t * ag
                    H[idx, q, q] = beta + t * ag
                    rotated[idx] = True
            done |= ~rotated
            if done.all():
                break
        lam = np.diagonal(H, axis1=1, axis2=2).real.copy()
        order = np.argsort(lam, axis=1, kind="stable")
        lam = np.take_along_axis(lam, order, axis=1)
        V = np.take_along_axis(V, order[:, None, :], axis=2)
        m2 = V.real * V.real + V.imag * V.imag
        top = np.argmax(m2, axis=1)                                       # the first of several maxima
        vm = np.take_along_axis(V, top[:, None, :], axis=1)
        hm = np.hypot(vm.real, vm.imag)                                   # v conj(vm) / |vm|, the parts written out: the
        re = (V.real * vm.real + V.imag * vm.imag) / hm                  # component itself gets an imaginary part of exactly 0
        im = (V.imag * vm.real - V.real * vm.imag) / hm
        V = np.empty(V.shape, cplx)
        V.real, V.imag = re, im
        status = np.where(done, 0, EIG_NO_CONVERGENCE).astype(np.int32)
        status[bad] = EIG_BAD_INPUT
        lam[bad] = np.nan
        V[bad] = complex(np.nan, np.nan)
    return Eig(lam.reshape(lead + (D,)), V.reshape(lead + (D, D)), status.reshape(lead))


def frobenius(A):
    """||A||_F of the matrix the solver works on, float64."""
    H = hermitian(np.asarray(A).astype(np.complex128))
    return np.sqrt(np.sum(np.abs(H) ** 2, axis=(-2, -1)))


def projector(V, K):
    """The projector onto the span of the K last columns of V."""
    E = V[..., :, V.shape[-1] - K:]
    return E @ np.conj(np.swapaxes(E, -1, -2))


def eig_errors(A, lam, V, lam_ref):
    """(residual, orthogonality, eigenvalue error) of a decomposition, each as a multiple of D u ||A||_F (D u for the second);
    a matrix of norm 0 must be reproduced exactly.  The arithmetic is longdouble's."""
    H = hermitian(A, LD)
    D = H.shape[-1]
    nf = np.sqrt(np.sum(H.real ** 2 + H.imag ** 2, axis=(-2, -1)))
    Vl, ll = np.asarray(V).astype(np.clongdouble), np.asarray(lam).astype(LD)
    res = np.abs(H @ Vl - Vl * ll[..., None, :]).max(axis=(-2, -1))
    orth = np.abs(np.conj(np.swapaxes(Vl, -1, -2)) @ Vl - np.eye(D)).max(axis=(-2, -1))
    err = np.abs(ll - np.asarray(lam_ref).astype(LD)).max(axis=-1)
    zero = nf == 0
    assert not (res[zero] > 0).any() and not (err[zero] > 0).any()
    scale = np.where(zero, LD(1), D * U * nf)
    return (float(np.max(res / scale, initial=0)), float(np.max(orth / (D * U), initial=0)), float(np.max(err / scale, initial=0)))


def split_gap(lam, K):
    """lam[D - K] - lam[D - K - 1]: the distance between the signal and the noise eigenvalues."""
    D = lam.shape[-1]
    return lam[..., D - K] - lam[..., D - K - 1]


EIG_KINDS = ("full", "rank1", "short", "identity", "zero", "indefinite", "clustered", "huge", "tiny")


@functools.lru_cache(maxsize=None)
def eig_case(kind, D, n, seed=0):
    """n Hermitian matrices (n, D, D) complex128 of one kind: "full" X X^H / T with T = 2 D frames, "rank1" T = 1, "short"
    T = max(D // 2, 1) < D frames, "identity", "zero", "indefinite" a random Hermitian matrix, "clustered" eigenvalues
    1, 1 + 1e-9, ..., "huge" / "tiny" the "full" ones times 1e150 / 1e-150.  Shared: read-only."""
    g = np.random.default_rng([seed, D, n, EIG_KINDS.index(kind)])

    def gauss(*shape):
        return g.standard_normal(shape) + 1j * g.standard_normal(shape)

    def gram(T):
        X = gauss(n, D, T)
        return X @ np.conj(np.swapaxes(X, 1, 2)) / T
    if kind in ("full", "huge", "tiny"):
        A = gram(2 * D) * {"full": 1.0, "huge": 1e150, "tiny": 1e-150}[kind]
    elif kind == "rank1":
        A = gram(1)
    elif kind == "short":
        A = gram(max(D // 2, 1))
    elif kind == "identity":
        A = np.broadcast_to(np.eye(D, dtype=complex), (n, D, D)).copy()
    elif kind == "zero":
        A = np.zeros((n, D, D), complex)
    elif kind == "indefinite":
        X = gauss(n, D, D)
        A = X + np.conj(np.swapaxes(X, 1, 2))
    else:
        Q = np.linalg.qr(gauss(n, D, D))[0]
        A = (Q * (1 + 1e-9 * np.arange(D))) @ np.conj(np.swapaxes(Q, 1, 2))
    A = hermitian(A)
    A.setflags(write=False)
    return A


# ---------------------------------------------------------------------------------------------------------------------- MUSIC
def music(V, lam, mics, cand, K, fs, n_fft, c, f_lo, f_hi, dtype=np.float64):
    """V (B, F, D, D), lam (B, F, D) -> (null (B, G) of ``dtype``, best (B,) int32, status (B,) int32), as the header defines
    them."""
    real, cplx = _types(dtype)
    B, F, D, _ = V.shape
    band = slice(f_lo, f_hi + 1)
    tau = srp_ref.delays(mics, cand, c, dtype)
    tau = np.broadcast_to(tau, (B,) + tau.shape[1:])                                              # (B, G, D)
    G = tau.shape[1]
    f = np.arange(f_lo, f_hi + 1).astype(real)
    with np.errstate(invalid="ignore", over="ignore"):
        phase = 2 * srp_ref._pi(dtype) * f[None, None, None, :] * (real(fs) / real(n_fft)) * tau[..., None]     # (B, G, D, Fb)
        a = np.exp(-1j * phase.astype(real)).astype(cplx)
        E = np.asarray(V)[:, band, :, D - K:].astype(cplx)                                        # (B, Fb, D, K)
        null = np.zeros((B, G), real)
        lb = np.asarray(lam)[:, band]
        counted = (lb != 0).any(axis=-1)                                                          # (B, Fb)
        for b in range(B):
            p = np.einsum("fdk,gdf->gfk", np.conj(E[b]), a[b])
            term = 1 - np.sum(p.real * p.real + p.imag * p.imag, axis=-1) / real(D)              # (G, Fb)
            null[b] = np.sum(term[:, counted[b]], axis=1) / real(max(int(counted[b].sum()), 1))
    status = np.zeros(B, np.int32)
    best = np.zeros(B, np.int32)
    mb = np.broadcast_to(np.asarray(mics, float) if np.ndim(mics) == 3 else np.asarray(mics, float)[None], (B, D, 3))
    qb = np.broadcast_to(np.asarray(cand, float) if np.ndim(cand) == 3 else np.asarray(cand, float)[None], (B, G, 3))
    for b in range(B):
        Vb = np.asarray(V)[b, band]
        if not (np.isfinite(Vb.real).all() and np.isfinite(Vb.imag).all() and np.isfinite(lb[b]).all()):
            status[b] |= BAD_SPECTRUM
        elif not counted[b].any():
            status[b] |= SILENT
        if not (np.isfinite(mb[b]).all() and np.isfinite(qb[b]).all()):
            status[b] |= BAD_GEOMETRY
        if status[b] & (BAD_SPECTRUM | BAD_GEOMETRY):
            null[b] = np.nan
        elif status[b] & SILENT:
            null[b] = 1
        best[b] = -1 if status[b] else int(np.argmin(null[b]))            # np.argmin: the first of several minima
    return null, best, status


def local_minima(row):
    """The indices of the strict local minima of a ring's row, the deepest first."""
    left, right = np.roll(row, 1), np.roll(row, -1)
    idx = np.nonzero((row < left) & (row < right))[0]
    return idx[np.argsort(row[idx], kind="stable")]


def map_alone_bound(D, K, theta):
    return (D * K + 16 * theta + 32 + ANCHOR) * U


def chain_bound(D, K, theta, norms, gaps, c1):
    """norms, gaps (B, F_band): ||Phi||_F and the split's gap of every bin of the band -> (B,)."""
    return map_alone_bound(D, K, theta) + np.mean(2 * c1 * D * U * norms / gaps, axis=1)


def eig_bound(D, nf, c1):
    return c1 * D * U * nf


def projector_bound(D, nf, gap, c1):
    return 2 * c1 * D * U * nf / gap


MusicRef = collections.namedtuple("MusicRef", "cov lam V null best status norms gaps margin bound_alone")
MUSIC_GAP = 1e-6          # the least relative eigengap at the split the MUSIC cases may have
GEV_GAP = 1e-3            # the same for the GEV cases' whitened matrix


def music_orders(D):
    """The subspace sizes the tests take: 1 and min(2, D - 1)."""
    return sorted({1, min(2, D - 1)})


def _margin(null):
    top = np.sort(null, axis=1)
    return top[:, 1] - top[:, 0] if null.shape[1] > 1 else np.full(null.shape[0], np.inf)


def _music_reference(X, mics, cand, K, n_fft, f_lo, f_hi):
    B, D = X.shape[0], X.shape[1]
    cov, st = BR.covariance(X)
    assert not st.any()
    e = eigh(cov)
    assert not e.status.any()
    null, best, status = music(e.V, e.lam, mics, cand, K, FS, n_fft, C, f_lo, f_hi)
    band = slice(f_lo, f_hi + 1)
    norms, gaps = frobenius(cov)[:, band], split_gap(e.lam, K)[:, band]
    assert (gaps / norms >= MUSIC_GAP).all(), (K, float((gaps / norms).min()))
    theta = srp_ref.theta_max(f_hi, FS, n_fft, mics, cand)
    margin = _margin(null)
    out = MusicRef(cov, e.lam, e.V, null, best, status, norms, gaps, margin, map_alone_bound(D, K, theta))
    for a in out[:9]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def music_reference(shape, K, single=False):
    """The float64 restatement of a srp_ref.PARITY shape with a signal subspace of K dimensions, computed once: the covariances
    (no mask, beamform_ref.covariance), their decomposition, the null spectrum, ||Phi||_F and the split's gap of the band's bins,
    the margin of the minimum over its runner-up (asserted > 4 x the chain's bound at 2 C1, so that best must match) and the
    map-alone bound.  single: of the input rounded to complex64 and promoted again."""
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c = srp_ref.parity_case(shape)
    X = c.X.astype(np.complex64).astype(np.complex128) if single else c.X
    out = _music_reference(X, c.mics, c.cand, K, n_fft, f_lo, f_hi)
    theta = srp_ref.theta_max(f_hi, FS, n_fft, c.mics, c.cand)
    assert (out.margin > 4 * chain_bound(D, K, theta, out.norms, out.gaps, 2 * C1)).all(), (shape, K, out.margin)
    return out


TwoSource = collections.namedtuple("TwoSource", "X mics cand true n_fft f_lo f_hi")
TWO_SOURCE = [(8, 64, 72), (6, 40, 36), (4, 200, 24)]          # (D, T, G)


@functools.lru_cache(maxsize=None)
def two_source_case(D, T, G, seed=5, noise=0.01):
    """One item with two independent free-field sources on two ring candidates at least a sixth of the ring apart, srp_ref.case's
    microphones (aperture 0.05 m) and sensor noise of scale ``noise``: ``TwoSource(X (1, D, F, T), mics, cand, true (2,), n_fft,
    f_lo, f_hi)``, band (8, 187) of n_fft = 400."""
    g = np.random.default_rng([seed, D, T, G])
    n_fft, F = 400, 201
    mics = srp_ref.CENTRE + 0.05 * g.uniform(-1, 1, (D, 3))
    cand = srp_ref.ring(G)
    first = int(g.integers(0, G))
    second = (first + int(g.integers(G // 6 + 1, G - G // 6))) % G
    omega = 2 * np.pi * np.arange(F) * FS / n_fft
    X = noise * (g.standard_normal((D, F, T)) + 1j * g.standard_normal((D, F, T)))
    for k in (first, second):
        S = g.standard_normal((F, T)) + 1j * g.standard_normal((F, T))
        r = np.linalg.norm(cand[k] - mics, axis=1)
        X = X + S[None] * (np.exp(-1j * omega[None, :] * r[:, None] / C) / r[:, None])[:, :, None]
    X = X[None]
    true = np.array(sorted((first, second)))
    for a in (X, mics, cand, true):
        a.setflags(write=False)
    return TwoSource(X, mics, cand, true, n_fft, 8, 187)


@functools.lru_cache(maxsize=None)
def two_source_reference(D, T, G):
    c = two_source_case(D, T, G)
    return _music_reference(c.X, c.mics, c.cand, 2, c.n_fft, c.f_lo, c.f_hi)


# ------------------------------------------------------------------------------------------------------------------------ GEV
def _forward(L, Bm):
    """L^-1 Bm by substitution in L's precision; Bm (..., D, n)."""
    D = L.shape[-1]
    Y = np.zeros_like(Bm)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(D):
            Y[..., i, :] = (Bm[..., i, :] - np.sum(L[..., i, :i, None] * Y[..., :i, :], axis=-2)) / L[..., i, i, None]
    return Y


def _backward(L, Y):
    """L^-H Y by substitution."""
    D = L.shape[-1]
    Z = np.zeros_like(Y)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(D - 1, -1, -1):
            Z[..., i, :] = (Y[..., i, :] - np.sum(np.conj(L[..., i + 1:, i, None]) * Z[..., i + 1:, :], axis=-2)) / L[..., i, i, None]
    return Z


def whitened(Phi_n, Phi_s, loading, dtype=np.float64):
    """(L, ok, C): the Cholesky factor of the loaded Phi_n and C = L^-1 Phi_s L^-H as the header forms it."""
    real, cplx = _types(dtype)
    P = BR.loaded(np.asarray(Phi_n).astype(cplx), loading)
    L, ok = BR._cholesky(P)
    Y = _forward(L, np.asarray(Phi_s).astype(cplx))
    Cm = _forward(L, np.conj(np.swapaxes(Y, -1, -2)))
    return L, ok, Cm


def gev(Phi_n, Phi_s, ref=0, loading=1e-6, dtype=np.float64):
    """Phi_n, Phi_s (B, F, D, D) -> ``Gev(W, rtf (B, F, D) complex of dtype, gain (B, F), status (B, F))`` as the header
    defines them."""
    real, cplx = _types(dtype)
    D = np.shape(Phi_n)[-1]
    L, ok, Cm = whitened(Phi_n, Phi_s, loading, dtype)
    e = eigh(Cm, dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u, lmax = e.V[..., :, -1], e.lam[..., -1]
        v = _backward(L, u[..., None])[..., 0]
        a = (np.tril(L) @ u[..., None])[..., 0]
        aref = a[..., ref]
        den = aref.real * aref.real + aref.imag * aref.imag
        ar, ai = aref.real[..., None], aref.imag[..., None]              # x conj(a_ref) with the parts written out, so that
        rtf, W = np.empty(a.shape, cplx), np.empty(a.shape, cplx)        # rtf_ref = (ar^2 + ai^2) / den is exactly 1
        rtf.real = (a.real * ar + a.imag * ai) / den[..., None]
        rtf.imag = (a.imag * ar - a.real * ai) / den[..., None]
        W.real = v.real * ar + v.imag * ai
        W.imag = v.imag * ar - v.real * ai
        ok = ok & (e.status == 0) & (lmax > 0) & np.isfinite(lmax) & (den > 0) & np.isfinite(den)
    if D == 1:
        W, rtf = np.ones_like(W), np.ones_like(rtf)
    for t in (W, rtf):
        t[~ok] = 0
        t[~ok, ref] = 1
    gain = np.where(ok, lmax, 0).astype(real)
    return Gev(W, rtf, gain, np.where(ok, 0, BAD_SOLVE).astype(np.int32))


def gev_bound(D, cond_, normC, gapC, wmax, c2):
    return c2 * D * U * cond_ * (1 + normC / gapC) * wmax


GEV_VARIANTS = ("rank1", "full")
GevRef = collections.namedtuple("GevRef", "Phi_n Phi_s out cond normC gapC")


@functools.lru_cache(maxsize=None)
def gev_reference(shape, kind, variant, ref=0):
    """The float64 restatement on a beamform_ref.PARITY shape under the mask ``kind``: Phi_n the noise's covariance, Phi_s the
    speech's alone ("rank1": what an oracle mask gives) or the mixture's ("full": the speech mask applied to the mixture);
    cond_2 of the loaded Phi_n, ||C||_F and the gap below C's top eigenvalue (float64, for the bound).  Asserted: cond <=
    beamform_ref.COND_CAP and, for D > 1, a relative gap >= GEV_GAP."""
    B, D, F, T, loading = shape
    r = BR.reference(shape, kind)
    Phi_n, Phi_s = r.cov_n, (r.cov_s if variant == "rank1" else r.cov)
    out = gev(Phi_n, Phi_s, ref, loading)
    assert not out.status.any()
    cond_ = BR.cond(Phi_n, loading)
    assert (cond_ <= BR.COND_CAP).all()
    Cm = whitened(Phi_n, Phi_s, loading)[2]
    normC = frobenius(Cm)
    if D > 1:
        lam = eigh(Cm).lam
        gapC = lam[..., -1] - lam[..., -2]
        assert (gapC / normC >= GEV_GAP).all(), (shape, kind, variant, float((gapC / normC).min()))
    else:
        gapC = np.full(normC.shape, np.inf)
    for a in (cond_, normC, gapC) + tuple(out):
        a.setflags(write=False)
    return GevRef(Phi_n, Phi_s, out, cond_, normC, gapC)
