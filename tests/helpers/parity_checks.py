"""The comparisons the device tests of the array kernels make against their float64 restatements, on numpy arrays alone, so that
a GPU test and a CPU test can call the same function: tests/test_iva_gpu.py, test_ilrma_gpu.py, test_cacgmm_gpu.py,
test_beamform_gpu.py and test_separation_metrics_gpu.py take theirs from here, tests/test_size_sweep_gpu.py runs every family's
on the size sweep, and tests/test_size_sweep_cpu.py shows each rejecting a wrong restatement.  Every function prints measured /
bound, asserts, and returns the largest ratio it measured.  u = 1.1e-16."""
import numpy as np

import align_ref
import beamform_ref
import cacgmm_ref
import iva_ref
import separation_metrics_ref
import srp_ref
import subspace_ref

U = iva_ref.U
NAMES = ("W", "basis", "activations")
GCC_LAGS = 8
C1, C2 = 2 * subspace_ref.C1, 2 * subspace_ref.C2         # the device is held to twice the constants tests/test_subspace_cpu.py measures


def _array(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same_bits(a, b):
    """Two numpy arrays of one shape and type with the same bits, NaN included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------------------ AuxIVA and ILRMA
def check_w(tag, W, ref_W, tol):
    """max |W - W_ref| <= tol max |W_ref|."""
    assert tol <= 1e-10, (tag, tol)                       # a condition on the case, not a measurement
    err = np.abs(W - ref_W).max() / np.abs(ref_W).max()
    print("%s: |W - W_ref| / max |W_ref| %.3g, tol %.3g, measured / tol %.3g" % (tag, err, tol, err / tol))
    assert err <= tol, (tag, err, tol)
    return err / tol


def check_three(tag, got, want, tol, demand=True):
    """max |dev - ref| <= tol max |ref| for each of W, basis and activations."""
    if demand:
        assert tol <= 1e-10, (tag, tol)                   # a condition on the case, not a measurement
    worst = []
    for name, g, w in zip(NAMES, got, want):
        err = np.abs(g - w).max() / np.abs(w).max()
        print("%s: |%s - ref| / max |ref| %.3g, tol %.3g, measured / tol %.3g" % (tag, name, err, tol, err / tol))
        worst.append((name, err))
    for name, err in worst:
        assert err <= tol, (tag, name, err, tol)
    return max(err for _, err in worst) / tol


def check_y(tag, Y, Xp, W, status, ref=0, single=False):
    """|Y - Y_ref| <= iva_ref.y_bound per output, Y_ref the restatement's projection of the given W (the device's own, so that
    only the projection differs) onto microphone ref; complex64: 6e-8 |Y_ref| more for the one rounding of Y."""
    want, _, st = iva_ref.project(Xp, W, status, ref)
    assert not st.any(), tag
    bound, cond = iva_ref.y_bound(Xp, W, ref)
    assert cond <= iva_ref.COND_CAP, (tag, cond)
    if single:
        bound = bound + 6e-8 * np.abs(want)
    err = np.abs(np.asarray(Y).astype(np.complex128) - want)
    ratio = float((err / bound).max())
    print("%s: largest |Y - Y_ref| / bound %.3g, cond_2(W) up to %.3g" % (tag, ratio, cond))
    assert (err <= bound).all(), (tag, ratio)
    return ratio


def check_refused_bins(tag, status, W, Y, X, want):
    """The status words are ``want``, and every bin with one has W = I and Y = X bit for bit."""
    assert np.array_equal(status, want), (tag, status, want)
    D = W.shape[-1]
    eye = np.eye(D, dtype=np.complex128)
    for b, f in zip(*np.nonzero(want)):
        assert same_bits(W[b, f], eye), (tag, b, f)
        assert same_bits(Y[b, :, f], X[b, :, f]), (tag, b, f)


# ---------------------------------------------------------------------------------------------------------------------- cACGMM
def check_gmm(tag, got, ref, tol):
    """masks, prior and quadratic (got[0], got[1], got[3]) of a device run against the restatement's."""
    assert tol <= cacgmm_ref.TOL_CAP, (tag, tol)          # a condition on the case, not a measurement
    qmax = ref.quadratic.max()
    errs = (np.abs(got[0] - ref.masks).max(), np.abs(got[1] - ref.prior).max(), np.abs(got[3] - ref.quadratic).max() / qmax)
    print("%s: |masks - ref| %.3g, |prior - ref| %.3g, |q - ref| / max q %.3g, tol %.3g, measured / tol %.3g"
          % ((tag,) + errs + (tol, max(errs) / tol)))
    assert max(errs) <= tol, (tag, errs, tol)
    return max(errs) / tol


def check_gmm_cov(tag, cov, ref, tol):
    """cov exactly Hermitian, of trace D, and |cov - cov_ref| <= C_COV tol cond per class matrix."""
    assert ref.cond.max() <= cacgmm_ref.COND_CAP, tag
    D = cov.shape[-1]
    assert np.array_equal(cov, np.conj(np.swapaxes(cov, -1, -2))), tag
    assert (np.abs(np.trace(cov, axis1=-2, axis2=-1) - D) <= 16 * D * D * U).all(), tag
    err = np.abs(cov - ref.cov).max(axis=(-2, -1))
    bound = cacgmm_ref.C_COV * tol * ref.cond
    ratio = float((err / bound).max())
    print("%s: largest |cov - cov_ref| / (c tol cond) %.3g, cond up to %.3g" % (tag, ratio, ref.cond.max()))
    assert (err <= bound).all(), (tag, ratio)
    return ratio


# --------------------------------------------------------------------------------------------------------------------- scoring
def si_bss_tolerance(shape, single=False):
    """separation_metrics_ref.tolerance; with one reference (K = 1) there is no interference, SIR is +inf forward and reversed,
    and e_ref is SAR's forward / reverse difference alone."""
    if shape[0] > 1:
        return separation_metrics_ref.tolerance(shape, single)
    a, b = separation_metrics_ref.reference(shape, single), separation_metrics_ref.reference(shape, single, reverse=True)
    assert (a.sir == np.inf).all() and (b.sir == np.inf).all()
    return 32 * float(np.abs(a.sar - b.sar).max()) + 8.7 * shape[2] * U


def check_si_bss(tag, sir, sar, sdr, ref, tol):
    """sir, sar and sdr within tol dB of the restatement's; an infinite value of the restatement (one reference: no
    interference) must be the same infinity."""
    assert tol <= separation_metrics_ref.TOL_CAP, (tag, tol)           # a condition on the case, not a measurement
    worst = []
    for name, g, w in (("sir", sir, ref.sir), ("sar", sar, ref.sar), ("sdr", sdr, ref.sdr)):
        inf = np.isinf(w)
        assert np.array_equal(g[inf], w[inf]), (tag, name)
        err = float(np.abs(g[~inf] - w[~inf]).max()) if (~inf).any() else 0.0
        print("%s: |%s - ref| %.3g dB, tol %.3g dB, measured / tol %.3g" % (tag, name, err, tol, err / tol))
        worst.append((name, err))
    for name, err in worst:
        assert err <= tol, (tag, name, err, tol)
    return max(err for _, err in worst) / tol


def check_assign(tag, got, table, maximize):
    """(perm, total, status) equal to the restatement's: the same k-rising sum of the same doubles."""
    want = separation_metrics_ref.assign(table, maximize)
    perm, total, status = got
    assert np.array_equal(perm, want.perm), (tag, table, perm, want.perm)
    assert np.array_equal(status, want.status), tag
    nan = np.isnan(want.total)
    assert total.shape == want.total.shape and np.array_equal(np.isnan(total), nan), tag
    assert np.array_equal(total[~nan].view(np.int64), want.total[~nan].view(np.int64)), tag
    return want


# ------------------------------------------------------------------------------------------------------------------- alignment
def check_align(tag, runs, refs, tol):
    """runs, refs: per iteration count (perm, score, changed, status) of the device and the restatement's Align: perm, changed
    and status equal, |score - ref| <= tol."""
    assert tol <= align_ref.TOL_CAP, (tag, tol)           # a condition on the case, not a measurement
    worst = 0.0
    for n in sorted(runs):
        perm, score, changed, status = runs[n]
        ref = refs[n]
        assert np.array_equal(status, ref.status) and not np.asarray(status).any(), (tag, n)
        assert np.array_equal(perm, ref.perm), (tag, n)
        assert np.array_equal(changed, ref.changed), (tag, n, changed, ref.changed)
        worst = max(worst, float(np.abs(score - ref.score).max()))
    print("%s: |score - ref| %.3g over %d iteration counts, tol %.3g, measured / tol %.3g" % (tag, worst, len(runs), tol, worst / tol))
    assert worst <= tol, (tag, worst, tol)
    return worst / tol


# -------------------------------------------------------------------------------------------------------- SRP-PHAT and MUSIC
def check_srp(tag, shape, psi, smap, gcc, best, status, ref, c):
    """The cross-spectra, the map and the GCC of a srp_ref shape within psi_bound, map_bound and gcc_bound; no status; the
    reference's arg-max clears twice the map's bound, and ``best`` is it."""
    B, D, T, G, f_lo, f_hi, n_fft = shape
    L = min(GCC_LAGS, n_fft // 2)
    theta = srp_ref.theta_max(f_hi, srp_ref.FS, n_fft, c.mics, c.cand)
    b_psi, b_map, b_gcc = srp_ref.psi_bound(T), srp_ref.map_bound(D, T, f_lo, f_hi, theta), srp_ref.gcc_bound(T, f_lo, f_hi, L)
    e_psi = float(np.abs(psi - ref.psi).max())
    e_map = float(np.abs(smap - ref.map).max())
    e_gcc = float(np.abs(gcc - srp_ref.gcc_phat(ref.psi, n_fft, L, f_lo, f_hi)).max())
    print("%s: measured / bound: psi %.3g (bound %.3g), map %.3g (bound %.3g, Theta %.4g), gcc %.3g (bound %.3g)"
          % (tag, e_psi / b_psi, b_psi, e_map / b_map, b_map, theta, e_gcc / b_gcc, b_gcc))
    assert e_psi <= b_psi and e_map <= b_map and e_gcc <= b_gcc, tag
    assert not np.asarray(status).any(), tag
    assert (ref.gap > 2 * b_map).all(), tag               # the arg-max is beyond the rounding: no item is let off
    assert np.array_equal(best, ref.best), (tag, best, ref.best)
    return max(e_psi / b_psi, e_map / b_map, e_gcc / b_gcc)


def check_music_map(tag, null, best, status, ref, bound):
    """|null - null_ref| <= bound (a number, or one per item), no status, and ``best`` the restatement's."""
    err = np.abs(null - ref.null).max(axis=1)
    ratio = float((err / bound).max())
    print("%s: |null - null_ref| / bound %.3g (bound %.3g)" % (tag, ratio, float(np.max(bound))))
    assert (err <= bound).all(), (tag, ratio)
    assert not np.asarray(status).any(), tag
    assert np.array_equal(best, ref.best), (tag, best, ref.best)
    return ratio


# ------------------------------------------------------------------------------------------------------- beamforming and GEV
def check_cov(got, ref_cov, scale, T, tag, skip=()):
    """|Phi - Phi_ref| <= 2 (T + 4) u S_ij per entry, the bins of ``skip`` left out."""
    err = np.abs(_array(got) - ref_cov)
    bound = 2 * beamform_ref.cov_bound(T, scale)
    keep = np.ones(err.shape[:2], bool)
    for b, f in skip:
        keep[b, f] = False
    ratio = (err[keep] / bound[keep]).max()
    print("%s: largest |Phi - Phi_ref| / bound %.3g" % (tag, ratio))
    assert (err[keep] <= bound[keep]).all(), (tag, ratio)
    return float(ratio)


def check_weights(tag, name, w, want, cond):
    """max |w - w_ref| <= 16 D u cond_2(Phi') max |w_ref| per bin (delay-and-sum: 2 u max |w_ref|)."""
    D = want.shape[-1]
    err = np.abs(w - want).max(axis=-1)
    if name == "das":
        bound = 2 * U * np.abs(want).max(axis=-1)
    else:
        assert cond.max() <= beamform_ref.COND_CAP, (tag, name)
        bound = beamform_ref.weights_bound(D, cond, np.abs(want).max(axis=-1), c=16)
    ratio = float((err / bound).max())
    print("%s %s: largest |w - w_ref| / bound %.3g, cond up to %.3g" % (tag, name, ratio, 1.0 if name == "das" else cond.max()))
    assert (err <= bound).all(), (tag, name, ratio)
    return ratio


def check_apply(tag, y, Xp, W, single=False):
    """|y - y_ref| <= 2 (D + 2) u sum_d |w_d| |x_d[t]| with the given W (the device's own) given to the restatement."""
    want = beamform_ref.apply(Xp, W)
    bound = 2 * beamform_ref.apply_bound(Xp, W) + (6e-8 * np.abs(want) if single else 0.0)
    err = np.abs(np.asarray(y).astype(np.complex128) - want)
    ratio = float((err / bound).max())
    print("%s: largest |y - y_ref| / bound %.3g" % (tag, ratio))
    assert (err <= bound).all(), (tag, ratio)
    return ratio


def check_gev(tag, w, rtf, gain, status, g, ref):
    """tests/test_subspace_gpu.py's GEV comparison: w and rtf within gev_bound at 2 c2 of the GevRef g, w^H rtf = 1, rtf[ref] = 1
    exactly and the gain within its bound."""
    D = w.shape[-1]
    assert not np.asarray(status).any(), tag
    ratios = []
    for mine, want in ((w, g.out.W), (rtf, g.out.rtf)):
        bound = subspace_ref.gev_bound(D, g.cond, g.normC, g.gapC, np.abs(want).max(axis=-1), C2)
        err = np.abs(mine - want).max(axis=-1)
        ratios.append(float((err / bound).max()))
    unit = subspace_ref.gev_bound(D, g.cond, g.normC, g.gapC, 1.0, C2)
    one = np.sum(np.conj(w) * rtf, axis=-1)
    print("%s: |w - w_ref| / bound %.3g, |rtf - rtf_ref| / bound %.3g, |w^H rtf - 1| %.3g"
          % (tag, ratios[0], ratios[1], float(np.abs(one - 1).max())))
    assert max(ratios) <= 1.0, (tag, ratios)
    slack = D * unit * (np.abs(g.out.W).max(axis=-1) * np.abs(g.out.rtf).max(axis=-1)) * 2
    assert (np.abs(one - 1) <= slack).all(), tag
    assert (rtf[..., ref] == 1).all(), tag
    assert (np.abs(gain - g.out.gain) <= unit * np.abs(g.out.gain)).all(), tag
    return max(ratios)
