"""Spatial covariances, steering vectors, beamformer weights and their application restated in numpy, straight from the
definitions on alvq_spatial_covariance_* / alvq_steering_vectors_f64 / alvq_beamform_weights_f64 / alvq_beamform_apply_* in
include/alvq.h: in float64, or in np.longdouble (the yardstick's yardstick).  Every sum is numpy's own over the whole axis and
the Cholesky factorisation is written out (so that it runs in longdouble), with none of the kernel's regrouping.  Also the
generator of the tests' inputs (``case``) and the error bounds the CPU and the GPU tests share."""
import collections
import functools

import numpy as np

import srp_ref

LD = np.longdouble
FS, C, N_FFT = srp_ref.FS, srp_ref.C, 400
U = 1.1e-16
BAD_INPUT, BAD_SOLVE, BAD_GEOMETRY = 1, 2, 4
DAS, MVDR, SOUDEN = 0, 1, 2
COND_CAP = 1e6          # the weights' bound grows with cond_2(Phi'): the tests' bins stay under this
SIGMA = 0.03            # the sensor noise of ``case``: cond_2(Phi') about 1e4
MASKS = ("ones", "uniform", "runs")

Case = collections.namedtuple("Case", "X speech noise mics source interferer A masks")
Reference = collections.namedtuple("Reference", "cov scale cov_n cov_s cond W")


def _types(dtype):
    return (np.float64, np.complex128) if dtype == np.float64 else (LD, np.clongdouble)


def _pi(dtype):
    return np.pi if dtype == np.float64 else np.arccos(LD(-1))


# ------------------------------------------------------------------------------------------------------------- definitions
def covariance(X, mask=None, dtype=np.float64):
    """X (B, D, F, T) complex, mask (B, F, T) or None -> (Phi (B, F, D, D) complex of ``dtype``'s precision, status (B, F)):
    Phi[i][j] = sum_t m_t x_i[t] conj(x_j[t]) / sum_t m_t for i >= j, the upper triangle its conjugate; status 1 and Phi = 0
    where X is not finite, the mask negative or not finite, or its sum not > 0."""
    real, cplx = _types(dtype)
    B, D, F, T = X.shape
    x = np.asarray(X).astype(cplx)
    m = np.ones((B, F, T), real) if mask is None else np.asarray(mask).astype(real)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        bad = ~(np.isfinite(x.real) & np.isfinite(x.imag)).all(axis=(1, 3)) | ~(np.isfinite(m) & (m >= 0)).all(axis=2)
        ms = np.sum(m, axis=2)
        bad |= ~(ms > 0)
        Phi = np.zeros((B, F, D, D), cplx)
        for i in range(D):
            for j in range(i + 1):
                v = np.sum(m * x[:, i] * np.conj(x[:, j]), axis=2) / ms
                if i == j:
                    v = v.real.astype(cplx)
                Phi[:, :, i, j] = v
                Phi[:, :, j, i] = np.conj(v)
    Phi[bad] = 0
    return Phi, np.where(bad, BAD_INPUT, 0).astype(np.int32)


def covariance_scale(X, mask=None):
    """S[i][j] = sum_t m_t |x_i[t]| |x_j[t]| / sum_t m_t, (B, F, D, D) float64: what an entry's rounding error is measured in."""
    B, D, F, T = X.shape
    m = np.ones((B, F, T)) if mask is None else np.asarray(mask, float)
    a = np.abs(np.asarray(X).astype(np.complex128))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.einsum("bft,bift,bjft->bfij", m, a, a) / np.sum(m, axis=2)[:, :, None, None]


def steering(mics, src, F, fs=FS, n_fft=N_FFT, c=C, ref=0, dtype=np.float64):
    """mics (D, 3) or (B, D, 3), src (B, 3) -> (A (B, D, F) complex of ``dtype``, status (B,)):
    a_d[f] = exp(-j 2 pi f (fs / n_fft) (tau_d - tau_ref)), tau_d = |q - m_d| / c; NaN and bit 4 for a non-finite coordinate."""
    real, cplx = _types(dtype)
    q = np.asarray(src).astype(real)
    B = q.shape[0]
    m = np.asarray(mics).astype(real)
    m = np.broadcast_to(m[None] if m.ndim == 2 else m, (B,) + m.shape[-2:])
    with np.errstate(invalid="ignore", over="ignore"):
        d = q[:, None, :] - m
        tau = np.sqrt(np.sum(d * d, axis=-1)) / real(c)                                          # (B, D)
        f = np.arange(F).astype(real)
        phase = 2 * _pi(dtype) * f[None, None, :] * (real(fs) / real(n_fft)) * (tau - tau[:, ref:ref + 1])[:, :, None]
        A = np.exp(-1j * phase.astype(real)).astype(cplx)
    bad = ~(np.isfinite(q).all(axis=1) & np.isfinite(m).all(axis=(1, 2)))
    A[bad] = complex(np.nan, np.nan)
    return A, np.where(bad, BAD_GEOMETRY, 0).astype(np.int32)


def theta_max(mics, src, F, fs=FS, n_fft=N_FFT, c=C):
    """The largest phase in radians: that of the longest path at the top bin (srp_ref.theta_max's term)."""
    m = np.asarray(mics, float)
    m = m[None] if m.ndim == 2 else m
    tau = np.sqrt(np.sum((np.asarray(src, float)[:, None, :] - m) ** 2, axis=-1)) / c
    return float(2 * np.pi * (F - 1) * (fs / n_fft) * tau.max())


def loaded(Phi_n, loading):
    """Phi' = Phi_n + loading (tr Phi_n / D) I."""
    D = Phi_n.shape[-1]
    real = Phi_n.real.dtype.type
    tr = np.trace(Phi_n, axis1=-2, axis2=-1).real
    return Phi_n + (real(loading) * (tr / real(D)))[..., None, None] * np.eye(D, dtype=real)


def cond(Phi_n, loading):
    """cond_2 of the loaded matrices, in float64 (inf where it cannot be taken)."""
    P = loaded(np.asarray(Phi_n).astype(np.complex128), loading)
    out = np.full(P.shape[:-2], np.inf)
    ok = np.isfinite(P.real).all(axis=(-2, -1)) & np.isfinite(P.imag).all(axis=(-2, -1))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        out[ok] = np.linalg.cond(P[ok], 2)
    return out


def _cholesky(R):
    """Lower Cholesky factors of Hermitian matrices (..., D, D) in their own precision, from the lower triangle alone, and
    which of them have every pivot > 0 and finite (the others' factors mean nothing)."""
    D = R.shape[-1]
    L = np.zeros_like(R)
    ok = np.ones(R.shape[:-2], bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(D):
            piv = (R[..., k, k] - np.sum(L[..., k, :k] * np.conj(L[..., k, :k]), axis=-1)).real
            good = (piv > 0) & np.isfinite(piv)
            ok &= good
            d = np.sqrt(np.where(good, piv, 1))
            L[..., k, k] = d
            for i in range(k + 1, D):
                L[..., i, k] = (R[..., i, k] - np.sum(L[..., i, :k] * np.conj(L[..., k, :k]), axis=-1)) / d
    return L, ok


def _solve(L, Bm):
    """Phi^-1 Bm for Phi = L L^H: L y = Bm, then L^H z = y, by substitution in L's precision.  Bm (..., D, n)."""
    D = L.shape[-1]
    Y = np.zeros_like(Bm)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(D):
            Y[..., i, :] = (Bm[..., i, :] - np.sum(L[..., i, :i, None] * Y[..., :i, :], axis=-2)) / L[..., i, i, None]
        Z = np.zeros_like(Bm)
        for i in range(D - 1, -1, -1):
            Z[..., i, :] = (Y[..., i, :] - np.sum(np.conj(L[..., i + 1:, i, None]) * Z[..., i + 1:, :], axis=-2)) / L[..., i, i, None]
    return Z


def weights(mode, Phi_n=None, Phi_s=None, A=None, ref=0, loading=1e-6, dtype=np.float64):
    """Phi_n, Phi_s (B, F, D, D), A (B, D, F) -> (W (B, F, D) complex of ``dtype``, status (B, F)), as the header defines the
    three modes; status 2 and w = e_ref at a pivot or a denominator <= 0 or not finite."""
    real, cplx = _types(dtype)
    if mode == DAS:
        a = np.moveaxis(np.asarray(A).astype(cplx), 1, 2)                                      # (B, F, D)
        return a / real(a.shape[-1]), np.zeros(a.shape[:2], np.int32)
    P = loaded(np.asarray(Phi_n).astype(cplx), loading)
    L, ok = _cholesky(P)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mode == MVDR:
            a = np.moveaxis(np.asarray(A).astype(cplx), 1, 2)
            z = _solve(L, a[..., None])[..., 0]
            den = np.sum(np.conj(a) * z, axis=-1).real
            W = z / den[..., None]
        else:
            G = _solve(L, np.asarray(Phi_s).astype(cplx))
            den = np.trace(G, axis1=-2, axis2=-1).real
            W = G[..., ref] / den[..., None]
    ok &= (den > 0) & np.isfinite(den)
    W[~ok] = 0
    W[~ok, ref] = 1
    return W, np.where(ok, 0, BAD_SOLVE).astype(np.int32)


def apply(X, W, dtype=np.float64):
    """y[b, f, t] = sum_d conj(W[b, f, d]) X[b, d, f, t], of ``dtype``'s precision."""
    _, cplx = _types(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sum(np.conj(np.moveaxis(np.asarray(W).astype(cplx), 2, 1))[..., None] * np.asarray(X).astype(cplx), axis=1)


# ------------------------------------------------------------------------------------------------------------------ bounds
def cov_bound(T, scale):
    """|Phi_64 - Phi_ld| <= (T + 4) u S_ij: a T-term sum in any order, the products, the division."""
    return (T + 4) * U * scale


def weights_bound(D, cond_, wmax, c=8):
    """max |w_64 - w_ld| <= c D u cond_2(Phi') max |w|: the forward bound of a Cholesky solve (tests/test_wpe_cpu.py's)."""
    return c * D * U * cond_ * wmax


def steering_bound(theta):
    """|A - A_ref| <= (16 Theta + 32) u: the phase term of srp_ref.map_bound."""
    return (16 * theta + 32) * U


def apply_bound(X, W):
    """(D + 2) u sum_d |w_d| |x_d[t]|, (B, F, T): one side's error of the D-term sum."""
    D = X.shape[1]
    return (D + 2) * U * np.sum(np.abs(np.moveaxis(W, 2, 1))[..., None] * np.abs(X), axis=1)


# ------------------------------------------------------------------------------------------------------------------- inputs
# (B, D, F, T, loading): the parity shapes of tests/test_beamform_gpu.py, pinned by tests/test_beamform_cpu.py
PARITY = [(2, 2, 5, 1, 1e-3),            # a single frame
          (2, 2, 5, 63, 1e-10), (1, 3, 4, 64, 1e-10), (1, 3, 4, 65, 1e-10),        # the wave edge
          (1, 8, 3, 257, 1e-10),         # D at its cap, the workgroup edge
          (1, 8, 2, 2000, 1e-10),        # a long row: the workgroup sums it
          (1, 1, 3, 100, 1e-10),         # D = 1: w = 1 in every mode
          (2, 4, 201, 500, 1e-10),       # the dataset's shape
          (1, 2, 2, 1024, 1e-10), (1, 2, 2, 1025, 1e-10),                            # the last row a wave sums, the first it does not
          (1, 5, 3, 70, 1e-10), (1, 7, 2, 1030, 1e-10)]                              # D = 5 on a wave, D = 7 on the workgroup
DATASET = PARITY[7]


@functools.lru_cache(maxsize=None)
def case(B, D, F, T, seed, loading=1e-10):
    """``Case(X, speech, noise, mics, source, interferer, A, masks)``: microphones mics (D, 3) = centre + 0.05 U(-1, 1)^3 around
    [2.5, 1.5, 1.5] (srp_ref's), a source and an interferer per item on srp_ref's ring, and X = speech + noise (B, D, F, T)
    complex128 with speech_d = a_d S and noise_d = b_d I + SIGMA N_d: S, I, N_d complex Gaussian of unit scale, a and b the
    steering vectors (ref 0) of the source and the interferer, A = a as (B, D, F).  masks: "ones", "uniform" (U[0, 1]) and
    "runs" (U[0, 1] with runs of zeros), (B, F, T) float64.  Asserted: under every mask, cond_2 of the mixture's and of the
    noise's covariance, loaded with ``loading``, is <= COND_CAP in every bin.  The arrays are shared between tests: read-only."""
    g = np.random.default_rng(seed)
    mics = srp_ref.CENTRE + 0.05 * g.uniform(-1, 1, (D, 3))
    ring = srp_ref.ring(72)
    pick = np.stack([g.choice(72, 2, replace=False) for _ in range(B)])
    source, interferer = ring[pick[:, 0]], ring[pick[:, 1]]
    A, _ = steering(mics, source, F)
    Bv, _ = steering(mics, interferer, F)

    def gauss(*shape):
        return g.standard_normal(shape) + 1j * g.standard_normal(shape)
    speech = A[..., None] * gauss(B, 1, F, T)
    noise = Bv[..., None] * gauss(B, 1, F, T) + SIGMA * gauss(B, D, F, T)
    uniform = g.uniform(0, 1, (B, F, T))
    runs = g.uniform(0, 1, (B, F, T))
    if T > 1:
        for b in range(B):
            for f in range(F):
                for start in g.integers(0, T, 1 + T // 40):
                    runs[b, f, start:start + 1 + T // 8] = 0
                if not runs[b, f].any():
                    runs[b, f, 0] = 0.5
    masks = {"ones": np.ones((B, F, T)), "uniform": uniform, "runs": runs}
    X = speech + noise
    for kind, m in masks.items():
        for name, part in (("mixture", X), ("noise", noise)):
            worst = cond(covariance(part, m)[0], loading).max()
            assert worst <= COND_CAP, (B, D, F, T, seed, kind, name, worst)
    for a in (X, speech, noise, mics, source, interferer, A) + tuple(masks.values()):
        a.setflags(write=False)
    return Case(X, speech, noise, mics, source, interferer, A, masks)


def parity_case(shape):
    B, D, F, T, loading = shape
    return case(B, D, F, T, B + D + F + T, loading)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, single=False):
    """The float64 restatement of a parity shape under the mask ``kind``, computed once: ``Reference(cov, scale, cov_n, cov_s,
    cond, W)``: cov and scale the mixture's covariance and its ``covariance_scale``; cov_n and cov_s the covariances of the
    noise and of the speech alone (what an oracle mask would give); cond (B, F) of the loaded cov, cov_n and cov_n in the order
    of the modes 1 (MPDR on cov), 1 (MVDR on cov_n), 2 (Souden on cov_n, cov_s) -> cond[name], W[name] for name in "mpdr",
    "mvdr", "souden", and W["das"] (``case`` has asserted every cond <= COND_CAP).  single: of the input rounded to complex64 and
    promoted again (cov and scale only differ)."""
    B, D, F, T, loading = shape
    c = parity_case(shape)
    m = c.masks[kind]
    X = c.X.astype(np.complex64).astype(np.complex128) if single else c.X
    cov, st = covariance(X, m)
    assert not st.any()
    cov_n, cov_s = covariance(c.noise, m)[0], covariance(c.speech, m)[0]
    conds = {"mpdr": cond(cov, loading), "mvdr": cond(cov_n, loading), "souden": cond(cov_n, loading)}
    W = {"das": weights(DAS, A=c.A)[0], "mpdr": weights(MVDR, cov, A=c.A, loading=loading)[0],
         "mvdr": weights(MVDR, cov_n, A=c.A, loading=loading)[0],
         "souden": weights(SOUDEN, cov_n, cov_s, loading=loading)[0]}
    out = Reference(cov, covariance_scale(X, m), cov_n, cov_s, conds, W)
    for a in (cov, out.scale, cov_n, cov_s) + tuple(conds.values()) + tuple(W.values()):
        a.setflags(write=False)
    return out
