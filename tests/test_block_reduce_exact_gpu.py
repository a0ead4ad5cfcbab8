"""Every kernel that takes its workgroup reduction or scan from csrc/block_reduce.h, on inputs whose result does not depend on
the order of the additions: small integers (float kernels: every partial sum below 2^24; double kernels: below 2^53), so
the device has no rounding freedom and a result is compared with an integer computed in numpy.  What a refactor of the
helpers gets wrong shows as a wrong integer: a wave left out, a lane counted twice, a missing barrier, the wrong number of
waves.  Each maker checks on the host that its input is exactly summable before the device is asked.

Sizes are the smallest at which a helper can go wrong: with W the kernel's workgroup size, n in {1, 63, 65, W - 1, W + 1,
2 W + 1}, one size of grid x W + 1 for the grid-stride kernels, N in {1, 65, 1025} (K = 3, D in {5, 129}) for k-means and
N in {2, 257} for t-SNE.

Where a result is not a bare sum the expectation restates the kernel's few remaining operations on the exact sum in the same
precision (one division, one product), which IEEE arithmetic makes bitwise.  The exceptions, with their derived bounds:
  perplexity of vq_gather_loss     exp(-sum p log p) in fp32 over K <= 7 terms: (K + 16) 2^-23 relative (K additions and the
                                   few-ulp logf / expf of the device library)
  center_shift_tot, scan cases     K terms through a square root: K 2^-50 relative (tests/test_kmeans_edges_gpu.py)
  t-SNE KL, STOI of a signal with itself, LSD of a tenfold spectrum   equal or near-equal terms: n 2^-53 relative for n
                                   non-negative float64 terms in any order, plus 1e-13 for the device's log / log10
  WPE                              the per-bin parity bound of tests/test_wpe_gpu.py; the floor eps max(p) is made to matter
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import kmeans_ref as KR  # noqa: E402
import speech_metrics_ref as SR  # noqa: E402
import wpe_ref as WR  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as SM  # noqa: E402

F32, F64 = np.float32, np.float64


def sizes(W):
    return [1, 63, 65, W - 1, W + 1, 2 * W + 1]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def ints(seed, lo, hi, *shape):
    return np.random.RandomState(seed).randint(lo, hi + 1, size=shape)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def exact_in(total_abs, dtype):
    """Every partial sum of terms whose magnitudes add up to ``total_abs`` is an integer the format holds."""
    return total_abs < (2 ** 24 if dtype == F32 else 2 ** 53)


# ------------------------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("n", sizes(256) + [1024 * 256 + 1])
def test_mse(n):
    """mse_partial_kernel (4 waves, pairwise) and mse_final_kernel (256-thread tree)."""
    b, d = ints(n, -8, 8, n), ints(n + 1, 0, 3, n)
    total = int((d * d).sum())
    assert exact_in(total, F32)
    got = host(N.mse(dev((b + d).astype(F32)), dev(b.astype(F32))))[0]
    assert got == F32(total) / F32(n)


VQ_CASES = [(n, 5) for n in sizes(256)] + [(4 * 1024 + 1, 65)]      # the last: every wave of a workgroup has rows


@pytest.mark.parametrize("n,D", VQ_CASES)
@pytest.mark.parametrize("ema", [False, True])
def test_vq_gather_loss(n, D, ema):
    """vq_gather_loss_kernel (4 waves, pairwise) and both vq_finalize kernels (two 256-thread trees)."""
    K, beta = 7, F32(0.25)
    x, E, idx = ints(n, -2, 2, n, D), ints(n + 1, -2, 2, K, D), ints(n + 2, 0, K - 1, n)
    total = int(((E[idx] - x) ** 2).sum())
    assert exact_in(total, F32)
    q_st, out = N.vq_gather_loss(dev(x.astype(F32)), dev(E.astype(F32)), dev(idx.astype(np.int64)), float(beta), ema=ema)
    out = host(out)
    m = F32(total) / F32(float(n) * float(D))
    assert out[0] == (beta * m if ema else m + beta * m)
    assert np.array_equal(host(q_st), E[idx].astype(F32))
    p = np.bincount(idx, minlength=K) / float(n)
    want = math.exp(-float(np.sum(p * np.log(p + 1e-10))))
    assert abs(out[1] - want) <= (K + 16) * 2.0 ** -23 * want


def exact_scale(nd):
    """A grad_loss value g with fl32(g * fl32(2 / nd)) == 2^-10 exactly: every term of the codebook gradient is then a small
    integer times 2^-10."""
    ce = F32(2.0 / nd)
    g = F32(F32(2.0 ** -10) / ce)
    for cand in (g, np.nextafter(g, F32(0)), np.nextafter(g, F32(np.inf))):
        if F32(cand * ce) == F32(2.0 ** -10):
            return cand
    raise AssertionError("no exact scale for nd = %r" % nd)


@pytest.mark.parametrize("n", [1, 63, 65, 1023, 1025, 2049])        # the scan runs over chunks of W = 1024 rows
@pytest.mark.parametrize("D", [4, 5])                               # float4 lanes; scalar lanes
@pytest.mark.parametrize("one_code", [False, True])                 # True: one code takes every row (the list is flushed)
def test_vq_codebook_grad(n, D, one_code):
    """vq_codebook_grad_kernel: the block scan that compacts a code's rows."""
    K = 3
    x, E = ints(n, -8, 8, n, D), ints(n + 1, -8, 8, K, D)
    idx = np.zeros(n, np.int64) if one_code else ints(n + 2, 0, K - 1, n).astype(np.int64)
    gl = exact_scale(float(n) * float(D))
    cnt = np.bincount(idx, minlength=K)
    sums = np.zeros((K, D), np.int64)
    np.add.at(sums, idx, x)
    want = cnt[:, None] * E - sums
    assert exact_in(int(np.abs(E[idx] - x).sum()), F32)
    _, dE = N.vq_backward(None, dev(np.array([gl], F32)), dev(x.astype(F32)), dev(E.astype(F32)), dev(idx), 0.25, want_dx=False)
    assert np.array_equal(host(dE), (want * 2.0 ** -10).astype(F32))


@pytest.mark.parametrize("n", sizes(256))
def test_conv1d_bias_grad(n):
    """bias_grad_kernel (4 waves, pairwise) behind conv1d_wgrad in fp32."""
    dy, x = ints(n, -3, 3, 1, 3, n), ints(n + 1, -3, 3, 1, 2, n)
    assert exact_in(int(np.abs(dy).sum()), F32)
    _, db = N.conv1d_wgrad(dev(dy.astype(F32)), dev(x.astype(F32)), 3, want_bias=True)
    assert np.array_equal(host(db), dy.sum(axis=(0, 2)).astype(F32))


# ------------------------------------------------------------------------------------------------------- gradient scale / norm
@pytest.mark.parametrize("n", sizes(256))
def test_grad_scale_amax(n):
    """grad_amax_kernel (4 waves, pairwise max): the largest magnitude wherever it lies."""
    for at in sorted({0, n // 2, n - 1}):
        x = np.full(n, 0.75, F32)
        x[at] = -3.0                                                 # amax = 3 -> S = 2^6 (S amax in [2^7, 2^8)); 0.75 -> 2^8
        state = host(N.grad_scale(dev(x)))
        assert state[0] == 64.0 and state[1] == 1.0 / 64.0, (at, state[:2])


@pytest.mark.parametrize("n", sizes(512) + [512 * 512 + 1])
def test_grad_clip_sum_of_squares(n):
    """grad_sumsq_kernel (8 waves, in order) and the ordered sum of its 512 partials."""
    g = ints(n, -5, 5, n)
    total = int((g * g).sum())
    assert exact_in(total, F64)
    sc, ws = torch.zeros(N.ADAM_SCALARS, device="cuda"), N.grad_clip_workspace("cuda")
    N.adam_advance(sc, 1e-3, 0.9, 0.999, 1.0)
    N.grad_clip(dev(g.astype(F32)), sc, float("inf"), workspace=ws)
    ws = host(ws)
    assert ws[-1] == total and ws[:-1].sum() == total
    assert host(sc)[5] == F32(math.sqrt(total))


# --------------------------------------------------------------------------------------------------------------------- k-means
def update(x, labels, old, tol=0.0):
    K = old.shape[0]
    new = torch.full_like(old, float("nan"))
    counts = torch.full((K,), -7, device="cuda", dtype=torch.int32)
    stats = torch.full((1,), float("nan"), device="cuda", dtype=torch.float64)
    flags = torch.full((4,), -7, device="cuda", dtype=torch.int32)
    N.kmeans_update(x, labels, None, old, new, counts, stats, flags, tol)
    return host(new), host(counts), float(stats.item()), host(flags).tolist()


@pytest.mark.parametrize("n", [1, 65, 1025])                         # 1025 crosses a label block of 1024 rows
@pytest.mark.parametrize("D", [5, 129])
@pytest.mark.parametrize("empty", [0, 1])
def test_kmeans_update_scans(n, D, empty):
    """scan_kernel's four block scans and relocate_kernel's (an empty cluster): counts and centres against the restatement."""
    K = 3
    X, C = KR.lattice(n + D, n, D, K)
    labels = ints(n + 3, 0, K - 1 - empty, n).astype(np.int64)
    want, shift, moved, counts_ref, n_empty, _ = KR.update(X.astype(F64), labels, C.astype(F64), K, full=True)
    shift = KR.shift_of_rounded(want, C)
    new, counts, tot, flags = update(dev(X), dev(labels), dev(C))
    assert np.array_equal(counts, counts_ref) and flags[1:] == [1, n_empty, moved]
    assert np.array_equal(bits(new), bits(want.astype(F32)))
    assert abs(tot - shift) <= K * 2.0 ** -50 * shift


def shift_case(n, D):
    """Rows and labels whose clusters hold a power of two of rows each (the centres are dyadic), and old centres that differ
    from the new ones by 2 in exactly four dimensions spread over the workgroup: every shift is sqrt(16) = 4."""
    K = 3
    X, _ = KR.lattice(n + D, n, D, K)
    half = (n - 1) // 2
    labels = np.concatenate([np.zeros(half), np.ones(half), np.full(n - 2 * half, 2)]).astype(np.int64)
    where = sorted({0, D // 2 - 1, D // 2, D - 1} if D > 5 else {0, 1, 2, 4})
    assert len(where) == 4 and (half & (half - 1)) == 0
    guess = KR.update(X.astype(F64), labels, np.full((K, D), 99.0), K)[0]
    old = guess.copy()
    old[:, where] += 2.0
    want, shift_tot, moved = KR.update(X.astype(F64), labels, old, K)
    assert np.array_equal(want, guess) and np.array_equal(want.astype(F32).astype(F64), want) and shift_tot == 16.0 * K
    assert np.array_equal(old.astype(F32).astype(F64), old)
    return X, labels, old.astype(F32), want.astype(F32), moved


@pytest.mark.parametrize("n", [1, 65, 1025])
@pytest.mark.parametrize("D", [5, 129])
def test_kmeans_shift_is_exact(n, D):
    """finalize_kernel (2 waves) and verdict_kernel (4 waves): center_shift_tot = 3 x 16 exactly."""
    X, labels, old, want, moved = shift_case(n, D)
    new, counts, tot, flags = update(dev(X), dev(labels), dev(old), tol=48.0)
    assert np.array_equal(bits(new), bits(want)) and flags[3] == moved
    assert tot == 48.0 and flags[0] == 2                            # 48 <= tol: converged by the shift


@pytest.mark.parametrize("n", sizes(1024))
def test_kmeans_inertia(n):
    """sum_kernel (16 waves, in order) over rowdist_kernel's exact distances."""
    K, D = 3, 5
    X, C = KR.lattice(n, n, D, K)
    labels = ints(n + 1, 0, K - 1, n).astype(np.int64)
    total = int(((X.astype(np.int64) - C.astype(np.int64)[labels]) ** 2).sum())
    assert exact_in(total, F64)
    assert host(N.kmeans_inertia(dev(X), dev(labels), dev(C)))[0] == total


@pytest.mark.parametrize("n", [1, 65, 1025])                         # 1025: 17 blocks of 64 rows
@pytest.mark.parametrize("D", [5, 129])
def test_kmeans_plusplus(n, D):
    """pick_kernel (fp64 block scan, wave scan), ppdist_kernel (4 waves a candidate), select_kernel (16 waves a candidate)."""
    K, T = min(3, n), 4
    X, _ = KR.lattice(n + 7 * D, n, D, K)
    u = np.random.RandomState(n + D).random_sample((max(K - 1, 1), T))
    first = n // 2
    want = KR.kmeans_plusplus(X, K, first, u)
    centers, indices = N.kmeans_plusplus(dev(X), K, first, dev(u) if K > 1 else None)
    assert np.array_equal(host(indices), want) and np.array_equal(host(centers), X[want])


@pytest.mark.parametrize("K", sizes(1024))
def test_ema_cluster_sizes(K):
    """ema_size_kernel (16 waves, in order, every thread uses the sum): decay 1/2 keeps every term a half-integer."""
    D, decay, eps = 2, 0.5, 1e-5
    cs, counts = ints(K, 1, 9, K).astype(F32), ints(K + 1, 0, 9, K).astype(F32)
    v = decay * cs.astype(F64) + (1.0 - decay) * counts.astype(F64)
    n = float(v.sum())
    assert exact_in(int(2 * v.sum()), F64) and 2 * n == int(2 * n)
    want = ((v + eps) / (n + float(K) * eps) * n).astype(F32)
    size = dev(cs)
    N.vq_ema_update(dev(counts), torch.zeros(K, D, device="cuda"), size, torch.ones(K, D, device="cuda"),
                    torch.ones(K, D, device="cuda"), decay, eps)
    assert np.array_equal(bits(host(size)), bits(want))


# ----------------------------------------------------------------------------------------------------------------------- t-SNE
@pytest.mark.parametrize("n", [2, 257])
def test_tsne_of_equidistant_points(n):
    """search_kernel (16 waves, two sums, alternating buffers) and reduce_kernel (256-thread tree).  All rows at squared
    distance 2 from each other and perplexity n - 1: the entropy is log(n - 1) at the first beta, so beta stays 1, the
    conditional P is 1 / (n - 1) (a power of two), the row sums are 2 and their total 2 n."""
    codes = dev(np.arange(n, dtype=np.int32).reshape(n, 1))
    P = N.tsne_code_sqdist(codes)
    assert np.array_equal(host(P), 2.0 * (1 - np.eye(n, dtype=F32)))
    beta, S = N.tsne_affinities(P, float(n - 1))
    s_want = (n - 1) * math.exp(-2.0)
    assert np.all(host(beta) == 1.0) and np.all(np.abs(host(S) - s_want) <= (n * 2.0 ** -53 + 1e-15) * s_want)
    p_cond = F32(1.0 / (n - 1))
    p_want = F32(max(float(p_cond + p_cond) / max(2.0 * n, 2.0 ** -52), 2.0 ** -52))
    assert np.array_equal(host(P), p_want * (1 - np.eye(n, dtype=F32)))
    # descent from one point: every 1 / (1 + |y_i - y_j|^2) is 1, Z = n (n - 1) exactly, and no gradient
    f64 = dict(device="cuda", dtype=torch.float64)
    Y, upd, gains, grad, stats = (torch.zeros(n, 2, **f64), torch.zeros(n, 2, **f64), torch.ones(n, 2, **f64),
                                  torch.full((n, 2), float("nan"), **f64), torch.full((2,), float("nan"), **f64))
    ws = N.tsne_descend(P, Y, upd, gains, grad, stats, 2, 4.0, 0.5, 200.0)
    assert host(ws.view(torch.float64))[5 * n] == float(n * (n - 1))
    assert not host(Y).any() and not host(grad).any() and host(stats)[1] == 0.0
    ep = 4.0 * float(p_want)
    kl = n * (n - 1) * ep * math.log(ep * n * (n - 1))
    assert abs(host(stats)[0] - kl) <= (n * n * 2.0 ** -53 + 1e-13) * kl


# ------------------------------------------------------------------------------------------------------- spectrogram statistics
@pytest.mark.parametrize("T", sizes(256))
def test_spec_rir_wiener(T):
    """spec_stats_kernel: three 256-thread sum trees and the max tree."""
    B, F = 1, 2
    S = ints(T, -4, 4, B, F, T, 2)
    E = ints(T + 1, 1, 5, B, F, T, 2)                                # E + 1e-8 is never near 0
    S[..., 0] += (S[..., 0] == 0) & (S[..., 1] == 0)                 # no zero ratio
    E[0, 1, T - 1] = (1, 0)                                          # the largest |S / E| of bin 1 in its last frame
    S[0, 1, T - 1] = (40, 9)
    sr, si, er, ei = (a.astype(F64) for a in (S[..., 0], S[..., 1], E[..., 0], E[..., 1]))
    nr, ni, den = (er * sr + ei * si).sum(-1), (ei * sr - er * si).sum(-1), (sr * sr + si * si).sum(-1)
    assert exact_in(int(np.abs(er * sr).sum() + np.abs(ei * si).sum() + den.sum()), F64)
    d = den + 1e-8
    wr, wi = nr / d, ni / d
    s_c = torch.view_as_complex(dev(S.astype(F32)))
    e_c = torch.view_as_complex(dev(E.astype(F64)))
    speech, echoed, rir, wiener = (host(t) for t in N.spec_rir_wiener(s_c, e_c))
    assert np.array_equal(bits(wiener), bits(wr * wr + wi * wi))
    assert np.array_equal(speech, (sr * sr + si * si).astype(F32)) and np.array_equal(echoed, er * er + ei * ei)
    ratio = np.abs((sr + 1j * si) / (er + 1e-8 + 1j * ei))
    assert np.unravel_index(np.argmax(ratio), ratio.shape) == (0, 1, T - 1)
    assert np.unravel_index(np.argmax(rir), rir.shape) == (0, 1, T - 1)
    assert abs(rir.max() - 1.0) <= 8 * 2.0 ** -52                    # |r / max|r||^2 at the maximum itself


# -------------------------------------------------------------------------------------------------------------- speech metrics
def si_sdr_rows(n):
    """reference s and estimate 2 s + w in quads (a, -a, a, -a), (b, b, -b, -b): both means 0, s . w = 0, so the projection is
    2 s exactly and every one of the six sums an integer.  A tail of n mod 4 zeros."""
    q = n // 4
    a, b = ints(n, 1, 7, q), ints(n + 1, 1, 7, q)
    s, w = np.zeros(n), np.zeros(n)
    s[:4 * q] = (a[:, None] * np.array([1, -1, 1, -1])).ravel()
    w[:4 * q] = (b[:, None] * np.array([1, 1, -1, -1])).ravel()
    return s, 2 * s + w, float((4 * s * s).sum()), float((w * w).sum())


@pytest.mark.parametrize("n", [2] + sizes(256)[1:])                  # the entry point takes rows of two samples or more
@pytest.mark.parametrize("dtype", [F32, F64])
def test_si_sdr(n, dtype):
    """si_sdr_kernel: three block sums of two values (4 waves, in order, leading barrier)."""
    s, e, num, den = si_sdr_rows(n)
    got = host(N.si_sdr(dev(s[None].astype(dtype)), dev(e[None].astype(dtype))))[0]
    if n < 4:
        assert np.isnan(got)                                         # a reference of no energy
    else:
        assert abs(got - 10.0 * math.log10(num / den)) <= 1e-13 * 10.0


@pytest.mark.parametrize("T", sizes(256))
@pytest.mark.parametrize("dtype", [F32, F64])
def test_lsd(T, dtype):
    """lsd_kernel: one block sum of two values.  p = 10 q: every frame's distance is 10 dB, and so is their mean."""
    q = ints(T, 1, 9, 1, 3, T).astype(dtype)
    got = host(N.lsd(dev(q * dtype(10.0)), dev(q), 0.0))[0]
    assert abs(got - 10.0) <= (T * 2.0 ** -53 + 1e-13) * 10.0
    q[0, 1, T - 1] = -1.0                                            # one bad entry in the last frame: counted, NaN
    assert np.isnan(host(N.lsd(dev(q * dtype(10.0)), dev(q), 0.0))[0])


@pytest.mark.parametrize("nf", sizes(256))
def test_stoi_frames_and_sum(nf):
    """stoi_mask_kernel (max and OR over 4 waves) and stoi_correlate_kernel (block sum of one value)."""
    n = SR.N_FRAME + SR.HOP * (nf - 1)
    x = np.random.RandomState(nf).standard_normal(n)
    value, kept, status = (host(t)[0] for t in N.stoi(dev(x[None]), dev(x[None]), *SM.stoi_band_edges()))
    assert kept == nf and status == (0 if nf >= SR.SEG else SR.FEW_FRAMES)
    if nf >= SR.SEG:
        pairs = SR.NUM_BANDS * (nf - SR.SEG + 1)
        assert abs(value - 1.0) <= pairs * 2.0 ** -53 + 1e-12        # every correlation is 1 up to its own rounding
    # the loudest frame last, 60 dB above the rest: the threshold comes from the last wave's maximum
    y = x * 1e-3
    y[-SR.N_FRAME:] = x[-SR.N_FRAME:]
    want = SR.stoi(y, y)
    assert want.margin > 1.0 and want.kept_frames <= 2
    value, kept, status = (host(t)[0] for t in N.stoi(dev(y[None]), dev(y[None]), *SM.stoi_band_edges()))
    assert kept == want.kept_frames and status == want.status


# ------------------------------------------------------------------------------------------------------------------------- WPE
@pytest.mark.parametrize("T", sizes(256))
@pytest.mark.parametrize("cdtype", [np.complex128, np.complex64])
def test_wpe_power_floor(T, cdtype):
    """wpe_kernel's block max / OR: the floor eps max(p) with eps = 1/4 and the loudest frame last, so that the maximum decides
    most weights."""
    D, taps, delay, its, eps, loading = 1, 2, 1, 2, 0.25, 1e-10
    _, x = WR.ar_bin(T, D, 2, delay, WR.bin_seed(0, T, D))
    X = x[None, :, None, :].astype(cdtype)
    X[..., T - 1] *= 4.0
    Yref, status, cond = WR.wpe(X.astype(np.complex128), taps, delay, its, 0, eps, loading)
    got, st = N.wpe(dev(X), taps, delay, its, 0, eps, loading)
    assert np.array_equal(host(st), status)
    if status[0, 0]:
        assert np.array_equal(host(torch.view_as_real(got)), host(torch.view_as_real(dev(X))))
        return
    assert cond[0, 0] <= WR.COND_CAP
    rounding = 6e-8 if cdtype == np.complex64 else 0.0
    bound = (8 * D * taps * 1.1e-16 * cond[0, 0] + 1e-13) * np.abs(X).max() + rounding * np.abs(Yref).max()
    assert np.abs(host(got).astype(np.complex128) - Yref).max() <= bound
