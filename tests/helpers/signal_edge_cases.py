"""The cases of the kernel-edge tests of csrc/rir.hip, csrc/speech_metrics.hip (STOI) and csrc/wpe.hip, their references and
their checking functions, shared by tests/test_rir_edges_gpu.py, test_stoi_edges_gpu.py and test_wpe_edges_gpu.py (which run
them on the device) and tests/test_signal_edges_cpu.py (which pins the conditions the cases must meet, the measured constants
recorded here, and that each check fails on a deliberately wrong restatement).  numpy only; every case is generated from a
fixed seed or from fixed numbers, every array handed out is read-only and every reference is computed once.

Room responses.  With A(t) the sum of |gain| over the images whose Tw-tap window covers sample t, N(t) their number and
u = 2^-53, a response without the high-pass is held to |h(t) - h_ref(t)| <= (K + N(t)) u A(t) at every t, and to exactly 0
where N(t) = 0.  N(t) pays for the two sides adding in different orders, K for the arithmetic of a tap.  K_REF is the
largest |rir - rir_ld| / (u A) over RIR_CASES (rir_ref.rir against its longdouble twin: what the float64 restatement
itself is off by; hp4097 and hp8193 are left out, whose room is hp4096's and whose twins take 12 s) and the device gets
K = 4 K_REF, since it rotates a table by frac where the restatement takes a cosine per tap: a handful of roundings more.  The twin takes rir_ref.images' float64 (d, gain) as its exact input, as the device
computes them with the same float64 expressions.
With the high-pass the bar is HP_RTOL max |h|: the larger of 1e-12 and four times HP_REF, the largest distance (over
max |h|) between rir_ref.highpass and its longdouble twin on the same unfiltered response."""
import collections
import functools

import numpy as np

import rir_ref as RR
import speech_metrics_ref as SR
import wpe_ref as WR

U53 = 2.0 ** -53


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


# ============================================================================================================ room responses
# measured by tests/test_signal_edges_cpu.py, which asserts them (K_REF / 2 <= measured <= K_REF, the same for HP_REF)
K_REF = 2.0              # measured 1.74 (the case 'near', sample 1)
K_DEVICE = 4.0 * K_REF
HP_REF = 1.0e-14         # measured 9.3e-15 (hp4096, hp4097 and hp8193 alike)
HP_RTOL = max(1e-12, 4.0 * HP_REF)

RirCase = collections.namedtuple("RirCase", "c fs L s r beta nsample order dim hp")
RirRef = collections.namedtuple("RirRef", "h A N")           # the unfiltered float64 restatement, A(t), N(t)

SMALL = dict(L=[1.0, 1.3, 0.9], s=[0.3, 0.4, 0.5], r=[[0.7, 0.9, 0.2]], beta=[0.8, -0.7, 0.6, -0.9, 0.5, -0.75])
BIG = dict(L=[4.0, 5.0, 3.0], s=[1.0, 3.5, 1.0], r=[[2.0, 2.5, 1.5]])
C_EXACT = 250.0                      # with fs = 16000: cTs = 2^-6 m exactly
CTS_EXACT = 2.0 ** -6
EXACT_S = [12, 9, 20]                # in samples
EXACT_R = [[44, 33, 8], [52, 9, 20], [51, 9, 20], [50, 9, 20]]          # s_x + r_x = 64, 63, 62 on the source's y and z


def _case(c=340.0, fs=16000.0, nsample=700, order=-1, dim=3, hp=False, **kw):
    room = dict(SMALL)
    room.update(kw)
    return RirCase(c, fs, room["L"], room["s"], room["r"], [float(v) for v in room["beta"]], nsample, order, dim, hp)


def _exact(nsample, r=EXACT_R, beta=SMALL["beta"], order=-1):
    scale = lambda p: [v * CTS_EXACT for v in p]                          # noqa: E731
    return _case(c=C_EXACT, nsample=nsample, order=order, L=scale([64, 48, 36]), s=scale(EXACT_S), r=[scale(p) for p in r],
                 beta=beta)


def _rir_cases():
    cases = collections.OrderedDict()
    # sample rates: Tw = 2 (the floor), 64, 352 (no multiple of 64), 384 (second pass of the table loop, half > tile), 1024
    cases["fs250"] = _case(fs=250.0, nsample=40, beta=SMALL["beta"], **BIG)
    for fs, ns in ((8000.0, 300), (44100.0, 1500), (48000.0, 1500), (128000.0, 2500)):
        cases["fs%d" % fs] = _case(fs=fs, nsample=ns)
    # rows shorter than or around one tile
    for ns in (1, 2, 63, 64, 65):
        for order in (-1, 0):
            cases["short%d_order%d" % (ns, order)] = _case(nsample=ns, order=order)
    # the high-pass kernel's 4096-sample chunk edge
    sabine = RR.sabine_beta(BIG["L"], 340.0, 0.4)
    for ns in (4096, 4097, 8193):
        cases["hp%d" % ns] = _case(nsample=ns, hp=True, beta=sabine, **BIG)
    # exact geometry: every squared distance an integer
    cases["exact700"] = _exact(700)
    cases["exact192"] = _exact(192)
    cases["exact_lone"] = _exact(192, r=[EXACT_R[1]], beta=[0.0] * 6, order=0)          # |s - r| = 40 samples
    # shapes of the image grid
    cases["flat_z"] = _case(L=[4.0, 4.0, 0.05], s=[1.0, 3.0, 0.02], r=[[2.5, 1.2, 0.03]])
    cases["flat_x"] = _case(L=[0.05, 4.0, 4.0], s=[0.02, 3.0, 1.0], r=[[0.03, 1.2, 2.5]])
    cases["near"] = _case(r=[[0.306, 0.406, 0.505]])                                     # 1 cm: d < 1 sample
    # walls
    cases["rigid_plus"] = _case(beta=[1.0] * 6)
    cases["rigid_minus"] = _case(beta=[-1.0] * 6)
    cases["one_dead_wall"] = _case(beta=[0.9, 0.9, 0.0, 0.9, 0.9, 0.9])
    cases["dim2_order0"] = _case(dim=2, order=0)
    cases["order1000"] = _case(order=1000)
    cases["order_all"] = _case(order=-1)
    return cases


RIR_CASES = _rir_cases()
RIR_BAD_RATES = (124.0, 129000.0)             # Tw = 0 and Tw = 1032: both raise


def rir_images(case, m=0, nsample=None):
    ns = case.nsample if nsample is None else nsample
    return RR.images(case.c, case.fs, case.r[m], case.s, case.L, case.beta, ns, case.order, case.dim)


def _taps(case, d, gain, mutate=None):
    """(h, A, N) by evaluating every tap directly in float64 (rir_ref.rir's loop, with A and N alongside).  mutate names a
    deliberately wrong variant (see rir_mutant)."""
    ns, Tw = case.nsample, RR.window_length(case.fs)
    h, A, N = np.zeros(ns), np.zeros(ns), np.zeros(ns, dtype=np.int64)
    taps = np.arange(Tw)
    for i in range(0, d.size, 1 << 14):
        dd, gg = d[i:i + (1 << 14), None], gain[i:i + (1 << 14), None]
        t = np.floor(dd).astype(np.int64) - Tw // 2 + 1 + taps
        u = t - dd
        uw = u + (taps >= 256) if mutate == "table_off" else u
        v = gg * 0.5 * (1.0 + np.cos(2.0 * np.pi * uw / Tw)) * np.sinc(u)
        ok = (t >= 0) & (t < ns)
        if mutate == "fd_lo":
            ok &= ~((taps == Tw - 1) & (t % 64 == 0))
        h += np.bincount(t[ok], weights=v[ok], minlength=ns)
        A += np.bincount(t[ok], weights=np.broadcast_to(np.abs(gg), t.shape)[ok], minlength=ns)
        N += np.bincount(t[ok], minlength=ns)
    return h, A, N


@functools.lru_cache(maxsize=None)
def rir_reference(name, m=0):
    """RirRef of receiver m of a case: rir_ref.rir without the high-pass (asserted equal to it bit for bit by the CPU test),
    A(t) and N(t)."""
    case = RIR_CASES[name]
    return RirRef(*(_frozen(a) for a in _taps(case, *rir_images(case, m))))


@functools.lru_cache(maxsize=None)
def rir_reference_highpassed(name, m=0):
    return _frozen(RR.highpass(rir_reference(name, m).h, RIR_CASES[name].fs))


def rir_mutant(name, which, m=0):
    """A deliberately wrong unfiltered response of a case:
    table_off     the window table indexed one entry off from entry 256 on (only Tw > 256 has such entries)
    fd_lo         ``fdd <= fd_lo`` in place of ``<``: a tile of 64 samples loses the images whose last tap is its first sample
    keep_nsample  the images with floor(d) == nsample kept"""
    case = RIR_CASES[name]
    if which == "keep_nsample":
        d, gain = rir_images(case, m, case.nsample + 1)
        return _taps(case, d, gain)[0]
    return _taps(case, *rir_images(case, m), mutate=which)[0]


def check_rir(h, ref, K=None):
    """Hold an unfiltered response to the bound; returns the largest measured / bound."""
    K = K_DEVICE if K is None else K
    h = np.asarray(h, dtype=np.float64)
    assert h.shape == ref.h.shape
    empty = ref.N == 0
    assert not np.any(h[empty] != 0.0), "samples no image reaches must be exactly 0: %s" % np.nonzero(empty & (h != 0.0))[0][:8]
    if empty.all():
        return 0.0
    bound = (K + ref.N[~empty]) * U53 * ref.A[~empty]
    ratio = np.abs(h - ref.h)[~empty] / bound
    worst = int(np.argmax(ratio))
    assert ratio[worst] <= 1.0, "sample %d: |h - h_ref| = %.3g is %.3g of the bound" % (
        np.nonzero(~empty)[0][worst], np.abs(h - ref.h)[~empty][worst], ratio[worst])
    return float(ratio[worst])


def check_rir_highpassed(h, want):
    """Hold a high-passed response to HP_RTOL max |want|; returns measured / bound."""
    h, want = np.asarray(h, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ratio = float(np.abs(h - want).max() / (HP_RTOL * np.abs(want).max()))
    assert ratio <= 1.0, "high-pass: %.3g of the bound" % ratio
    return ratio


# ===================================================================================================================== STOI
STOI_ATOL, MIN_MARGIN_DB = 1e-10, 1e-6               # tests/test_speech_metrics_gpu.py's
STOI_N = (32896, 33024, 50000, 77056)                 # 256, 257, 389 and 601 frames at 10 kHz
STOI_TILE = 256                                       # frames per tile of stoi_mask_kernel
# (kept_frames, status) of the rows a, b, c, d; pinned against the restatement by the CPU test
STOI_EXPECT = {32896: [(256, 0), (221, 0), (256, 0), (256, 0)],        # (d): the whole row is scaled, nothing falls out
               33024: [(257, 0), (221, 0), (256, 0), (1, 2)],          # (d): one frame left, too few
               50000: [(389, 0), (346, 0), (256, 0), (133, 0)],
               77056: [(601, 0), (558, 0), (256, 0), (345, 0)]}


@functools.lru_cache(maxsize=None)
def stoi_rows(n):
    """(clean, degraded), each (4, n) at 10 kHz: (a) white noise; (b) a stretch straddling frame 256 and one inside the first
    tile scaled by 1e-4; (c) every frame from 256 on silent; (d) every frame before 256 silent.  Frame t is the samples
    128 t .. 128 t + 255: frame 256 starts at 32768 and frame 255 ends at 32895."""
    g = np.random.default_rng(4100 + n)
    clean = g.standard_normal((4, n))
    clean[1, 30000:34000] *= 1e-4
    clean[1, 5000:7000] *= 1e-4
    clean[2, 32768:] *= 1e-4
    clean[3, :32896] *= 1e-4
    degraded = clean + 0.5 * g.standard_normal((4, n))
    return _frozen(clean), _frozen(degraded)


@functools.lru_cache(maxsize=None)
def stoi_reference(n):
    clean, degraded = stoi_rows(n)
    return tuple(SR.stoi(clean[b], degraded[b]) for b in range(4))


def stoi_mutant_carry_dropped(clean, degraded):
    """stoi_mask_kernel with the carry dropped at the second tile of frames: tile two numbers its kept frames from 0 again.
    Only (kept_frames, status) are restated: the value of a row whose list of frames is wrong is not computed (NaN)."""
    ref = SR.stoi(clean, degraded)
    if ref.status == SR.BAD_ENERGY:
        return ref
    W = SR.window()
    fx = SR.frames(np.asarray(clean, dtype=np.float64)) * W
    e = 20.0 * np.log10(np.sqrt(np.sum(fx * fx, axis=1)) + SR.EPS)
    keep = e > e.max() - SR.DYN_RANGE_DB
    carry = 0
    for tile, base in enumerate(range(0, len(keep), STOI_TILE)):
        count = int(keep[base:base + STOI_TILE].sum())
        carry = count if tile == 1 else carry + count
    if carry == ref.kept_frames:
        return ref
    return SR.Stoi(np.nan, carry, SR.FEW_FRAMES if carry < SR.SEG else 0, ref.nf, ref.margin)


def check_stoi(value, kept, status, refs, tag=""):
    """(value, kept_frames, status) arrays of B rows against the restatement's rows; returns the largest |value - ref|."""
    worst = 0.0
    for b, ref in enumerate(refs):
        print("%s row %d: got %.17g restatement %.17g kept %d / %d of %d status %d / %d margin %.3g dB"
              % (tag, b, value[b], ref.value, kept[b], ref.kept_frames, ref.nf, status[b], ref.status, ref.margin))
        assert ref.margin >= MIN_MARGIN_DB, (b, ref.margin)
        assert kept[b] == ref.kept_frames and status[b] == ref.status, (b, kept[b], status[b], ref)
        if np.isnan(ref.value):
            assert np.isnan(value[b]), (b, value[b])
        else:
            assert abs(value[b] - ref.value) <= STOI_ATOL, (b, value[b], ref.value, abs(value[b] - ref.value))
            worst = max(worst, abs(value[b] - ref.value))
    return worst


# ====================================================================================================================== WPE
WPE_U = 1.1e-16                                       # tests/test_wpe_gpu.py's bound
# (B, D, F, T, taps, delay, psd_context, loading)
WPE_DELAY0 = (2, 2, 3, 200, 8, 0, 0, 1e-10)           # the filter predicts the frame from itself
WPE_CASES = [WPE_DELAY0,
             (2, 1, 3, 40, 4, 1, 64, 1e-10),          # psd_context at its cap, wider than the row: clipped at both ends
             (1, 3, 2, 700, 21, 64, 1, 1e-10),        # delay at its cap
             (1, 8, 2, 300, 8, 3, 0, 1e-10)]          # D at its cap, M = 64
WPE_WORKSPACE = (2, 2, 3, 2200, 30, 2, 3, 1e-10)      # q and w in the caller's workspace, with a power context
WPE_LDS_T = 5111                                      # the largest T whose rows stay in LDS at D = taps = 1
WPE_LDS_LIMIT = 160 * 1024 - 256


def wpe_rows_in_lds(D, T, taps):
    """wpe.hip's budget, restated: A and the bin's x, q and w in 160 KiB less 256 bytes."""
    M = D * taps
    return 2 * (M + D) * M * 8 + 16 * (D + 1) * T <= WPE_LDS_LIMIT


def wpe_boundary_case(T):
    return (1, 1, 2, T, 1, 1, 0, 1e-10)


def wpe_case(case, iterations=3):
    return WR.case(*case, iterations=iterations)


def wpe_bin_mutant(X, taps, delay, iterations, psd_context, eps, loading, unclipped=False, lams=None):
    """wpe_ref.wpe_bin in float64 with one of two defects: ``unclipped``, a power window that runs past the row's ends (zeros
    there, divided by the full 2 psd_context + 1 frames); ``lams``, the per-iteration lambda of another bin in place of the
    bin's own.  Returns (Y, the list of lambdas used)."""
    import scipy.linalg
    X = np.asarray(X).astype(np.complex128)
    D, T = X.shape
    M = D * taps
    Xt = WR.stack_past(X, taps, delay)
    Y, used = X.copy(), []
    for it in range(iterations):
        q = np.sum(Y.real ** 2 + Y.imag ** 2, axis=0)
        p = q / D
        for t in range(T if psd_context else 0):
            lo, hi = max(0, t - psd_context), min(T - 1, t + psd_context)
            p[t] = np.sum(q[lo:hi + 1]) / (D * ((2 * psd_context + 1) if unclipped else (hi - lo + 1)))
        lam = np.maximum(p, eps * np.max(p)) if lams is None else lams[it]
        used.append(lam)
        Xw = Xt / lam
        Rm = Xw @ np.conj(Xt.T)
        P = Xw @ np.conj(X.T)
        Rm = Rm + loading * (np.trace(Rm).real / M) * np.eye(M)
        L = np.linalg.cholesky(Rm)
        G = scipy.linalg.solve_triangular(L, scipy.linalg.solve_triangular(L, P, lower=True), lower=True, trans="C")
        Y = X - np.conj(G.T) @ Xt
    return Y, used


def check_wpe(Y, X, Yref, cond, case, rounding=0.0, tag=""):
    """tests/test_wpe_gpu.py's bound on every bin: max |Y - Y_ref| <= (8 M u cond + 1e-13) max |x| + rounding max |y_ref|, with
    cond <= COND_CAP asserted.  Returns the largest measured / bound."""
    B, D, F, T, taps = case[:5]
    Y = np.asarray(Y).astype(np.complex128)
    worst, worst_err = 0.0, 0.0
    for b in range(B):
        for f in range(F):
            assert cond[b, f] <= WR.COND_CAP, (b, f, cond[b, f])
            err = float(np.abs(Y[b, :, f] - Yref[b, :, f]).max())
            bound = (8 * D * taps * WPE_U * cond[b, f] + 1e-13) * np.abs(X[b, :, f]).max() + rounding * np.abs(Yref[b, :, f]).max()
            if err / bound > worst:
                worst, worst_err = err / bound, err
            assert err <= bound, (tag, b, f, err, bound, cond[b, f])
    print("%s %s: largest measured / bound %.3g (|Y - Y_ref| %.3g there), cond up to %.3g"
          % (tag, case[:7], worst, worst_err, np.max(cond)))
    return worst
