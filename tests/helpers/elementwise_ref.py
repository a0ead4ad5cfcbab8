"""Float64 restatements (numpy) of csrc/elementwise.hip, the Adam kernels of csrc/pack_weights.hip and csrc/location.hip,
the tolerances the tests hold the kernels to, numpy-float32 emulations of the kernels in their documented summation order
(tests/test_elementwise_ref_cpu.py proves every tolerance on them), and the case grids.  Shared by
tests/test_elementwise_ref_cpu.py and tests/test_elementwise_edges_gpu.py, so both use the same numbers.

u = 2^-24 is the unit roundoff of fp32: one rounding changes a result r by at most u |r| <= ulp(r) / 2.
"""
import math

import numpy as np

U = 2.0 ** -24
F32_MAX = float(np.finfo(np.float32).max)
EW_PARTIALS = 1024
EW_THREADS = EW_PARTIALS * 256           # one element per thread up to here, the stride loop above


def f64(a):
    return np.asarray(a, np.float64)


def f32(a):
    return np.asarray(a, np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def ulp_distance(a, b):
    """Elementwise distance of two fp32 arrays in units in the last place (the number of fp32 values between them)."""
    def key(t):
        i = bits(t).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def ulp(x):
    """Spacing of fp32 at |x| (float64 in, float64 out); the spacing of the denormals below 2^-126."""
    x = np.abs(f64(x))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return 2.0 ** (np.maximum(e, -126) - 23)


# ====================================================================================================== restatements
def standardise(x, take_abs):
    """(B, C, L): per (b, l) column over axis 1, (v - mean) / (std + 1e-8) with the unbiased std; -> (y, mean, std)."""
    v = f64(x)
    if take_abs:
        v = np.abs(v)
    C = v.shape[1]
    mean = v.sum(1, keepdims=True) / C
    std = np.sqrt(((v - mean) ** 2).sum(1, keepdims=True) / (C - 1))
    return (v - mean) / (std + 1e-8), mean, std


def mse(a, b):
    d = f64(a) - f64(b)
    return float((d * d).sum() / d.size)


def mse_backward(a, b, grad_loss):
    return float(np.float32(grad_loss)) * 2.0 / np.asarray(a).size * (f64(a) - f64(b))


def row_mean(x):
    return f64(x).sum(-1) / np.asarray(x).shape[-1]


def row_mean_backward(dy, L):
    return np.repeat(f64(dy).reshape(-1, 1) / L, L, axis=1)


def jitter(x, src, backward):
    x = np.asarray(x)
    src = np.asarray(src)
    if backward:
        return np.where(src == np.arange(src.size), x, np.float32(0.0)).astype(np.float32)
    return x[..., src]


def transpose12(x):
    return np.ascontiguousarray(np.swapaxes(np.asarray(x), 1, 2))


def relu_mask(dy, t):
    """t > 0 ? dy : +0 (a NaN in t compares false)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(t) > 0, np.asarray(dy), np.float32(0.0)).astype(np.float32)


def add(a, b):
    return f32(a) + f32(b)


def adam_scalars(t, lr, beta1, beta2, grad_scale):
    """{lr / (1 - beta1^t), sqrt(1 - beta2^t), grad_scale, t} in float64: what adam_advance_kernel rounds to fp32."""
    return (lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t), float(grad_scale), float(t))


def adam(p, g, m, v, t, lr, beta1, beta2, eps, grad_scale):
    """One step of torch.optim.Adam (no amsgrad, no weight decay) in float64 from the fp32 inputs, in the expression of
    adam_kernel: lerp form of m, sqrt(v) / sqrt(bc2) + eps.  beta1, beta2, eps enter as the kernel receives them (fp32).
    -> (p, m, v, denom)."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    b1, b2, e = float(np.float32(beta1)), float(np.float32(beta2)), float(np.float32(eps))
    lr_bc1, bc2_sqrt, gs, _ = adam_scalars(t, lr, beta1, beta2, float(np.float32(grad_scale)))
    gr = g * gs
    mm = m + (gr - m) * (1.0 - b1)
    vv = v * b2 + (1.0 - b2) * gr * gr
    denom = np.sqrt(vv) / bc2_sqrt + e
    return p - lr_bc1 * (mm / denom), mm, vv, denom


def embedding_bag_fwd(W, bias, idx, L, K):
    """out[b][m] = bias[m] + sum_l W[m][l*K + idx[b][l]]; an index outside [0, K) contributes nothing.
    -> (out, sum of |terms|, flag)."""
    W, idx = f64(W), np.asarray(idx)
    B, M = idx.shape[0], W.shape[0]
    ok = (idx >= 0) & (idx < K)
    col = np.arange(L)[None, :] * K + np.where(ok, idx, 0)
    terms = W[:, col] * ok[None]                              # (M, B, L)
    out = terms.sum(-1).T
    mag = np.abs(terms).sum(-1).T
    if bias is not None:
        out = out + f64(bias)[None]
        mag = mag + np.abs(f64(bias))[None]
    assert out.shape == (B, M)
    return out, mag, int(not ok.all())


def embedding_bag_bwd(dz, idx, L, K):
    """dW[m][l*K + idx[b][l]] += dz[b][m], db[m] = sum_b dz[b][m] -> (dW, db, sum of |terms| of dW, touched columns, flag)."""
    dz, idx = f64(dz), np.asarray(idx)
    B, M = dz.shape
    dW, mag = np.zeros((M, L * K)), np.zeros((M, L * K))
    touched = np.zeros(L * K, bool)
    ok = (idx >= 0) & (idx < K)
    for b in range(B):
        cols = (np.arange(L) * K + idx[b])[ok[b]]
        dW[:, cols] += dz[b][:, None]
        mag[:, cols] += np.abs(dz[b])[:, None]
        touched[cols] = True
    return dW, dz.sum(0), mag, touched, int(not ok.all())


def onehot_to_index(enc):
    """-> (idx, flag): the largest position holding a non-zero (0 for a row of zeros); the flag rises unless every row holds
    exactly one non-zero and that is 1.0 (-0.0 is a zero, NaN is not)."""
    enc = np.asarray(enc)
    nz = enc != 0
    K = enc.shape[1]
    pos = np.where(nz.any(1), K - 1 - np.argmax(nz[:, ::-1], axis=1), 0)
    bad = (nz.sum(1) != 1) | (nz & (enc != 1)).any(1)
    return pos.astype(np.int32), int(bad.any())


# ======================================================================================================== tolerances
def standardise_bound(C, xmax, std, ref):
    """|y - ref| per element <= 2 (C/4 + 7) u (max|x| / (std + 1e-8) + |ref|), per column.
    Two-pass form, n = ceil(C/4) <= C/4 + 3/4 terms per channel-group partial:
      mean   n - 1 adds in a partial, 2 adds of the four partials, 1 division: |dmean| <= (n + 2) u max|x|
      v - mean  carries dmean and its own rounding u |v - mean|
      var    dmean shifts every deviation by the same amount, and the deviations sum to zero, so it enters var only in second
             order; first order: 2 (the deviations' roundings) + 1 (square) + n + 1 (sums) + 1 (division) = (n + 5) u relative
      den    sqrt halves that and adds 1, the + 1e-8 adds 1: (n/2 + 4.5) u relative
      y      the division adds 1:  |y - ref| <= (n + 2) u max|x| / den + (n/2 + 6.5) u |ref|,
    and both counts are <= C/4 + 7.  The factor 2 pays for the second-order terms (the largest is |ref| ((n + 2) u max|x| / std)^2
    from var), which stay below the first-order ones while (C/4 + 7) u (max|x| / std) sqrt(C) <= 1/4: the bound is CONDITIONED on
    max|x| / std, and standardise_precondition checks it."""
    return 2.0 * (C / 4.0 + 7.0) * U * (xmax / (std + 1e-8) + np.abs(ref))


def standardise_precondition(C, xmax, std):
    return (C / 4.0 + 7.0) * U * (xmax / std) * math.sqrt(C) <= 0.25


def mse_bound(n):
    """relative: (ceil(n / 262144) + 23) u.  A thread adds t = ceil(n / 262144) squares (t - 1 roundings), each square carries
    the difference's rounding twice and its own (3); butterfly 6, the four waves 2, mse_final: 4 partials per thread 3, the
    256-wide tree 8, the division 1: t - 1 + 3 + 6 + 2 + 3 + 8 + 1 = t + 22, every term non-negative; one more for (1+u)^k."""
    return (math.ceil(n / EW_THREADS) + 23) * U


MSE_BACKWARD_ULPS = 2     # fl(2/n), the difference, the product (and fl(grad_loss * fl(2/n)), constant over the array): each at
#                           most half an ulp, under 2.5 ulp of the float64 value in sum, so at most 2 from its fp32 rounding


def row_mean_bound(L, mean_abs):
    """(ceil(L / 64) + 7) u mean|x|: t - 1 adds per lane, butterfly 6, division 1, one more for (1+u)^k."""
    return (math.ceil(L / 64) + 7) * U * mean_abs


ROW_MEAN_BACKWARD_ULPS = 2    # fl(1/L) and the product


def adam_bounds(p, g, m, v, t, lr, beta1, beta2, eps, grad_scale):
    """-> (ref p, ref m, ref v, bound p, bound m, bound v) for one step; G = |g grad_scale|, X = max(|m|, G).
      m   fl(g gs) 1; gr - m: |.| <= 2X, 1; times (1 - beta1): 1; + m, the result is a convex combination, |.| <= X: 1.
          Carried through: u (G + 2X) (1 - beta1) + 2X (1 - beta1) u + X u <= 6 u X                         -> 6 u X (+ 4 denormal steps)
      v   all terms non-negative: gr^2 carries gr's rounding twice, (1 - beta2) gr gr two products, v beta2 one, the sum one
                                                                                                            -> 6 u v' (5 + second order)
      p   sqrt(v') 5/2 + 1; / sqrt(bc2) 1, and sqrt(bc2) itself is within 1 ulp = 2 u of the float64 scalar; + eps 1: denom 7.5 u.
          q = m' / denom: 7.5 + 1, plus m's error over denom; lr_bc1 q: 1, and lr_bc1 within 2 u: 11.5 u |q| <= 12 u |m'| / denom;
          p - ...: half an ulp of the result                         -> ulp(p) + u lr_bc1 (12 |m'| + 6 X) / denom (+ the denormal steps)
    A fused multiply-add only removes roundings from these counts."""
    pr, mr, vr, denom = adam(p, g, m, v, t, lr, beta1, beta2, eps, grad_scale)
    lr_bc1 = adam_scalars(t, lr, beta1, beta2, grad_scale)[0]
    X = np.maximum(np.abs(f64(m)), np.abs(f64(g) * float(np.float32(grad_scale))))
    tiny = 4 * 2.0 ** -149
    bm = 6 * U * X + tiny
    bv = 6 * U * vr + tiny
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        bp = np.maximum(ulp(pr), ulp(p)) + lr_bc1 * (U * (12 * np.abs(mr) + 6 * X) + tiny) / denom
    return pr, mr, vr, bp, bm, bv


def bag_fwd_bound(L, mag):
    """(ceil(L / 64) + 7) u sum|terms|: t - 1 adds per lane, butterfly 6, the bias 1, one more for (1+u)^k."""
    return (math.ceil(L / 64) + 7) * U * mag


def bag_bwd_bound(B, mag):
    """B u sum|terms| per column: at most B sequential adds (the first lands on the prefilled value)."""
    return B * U * mag


# =================================================================================== fp32 emulations, the kernels' order
def _butterfly(v):
    """wave_sum over the last axis (64 lanes): v += v[lane ^ o], o = 32 .. 1."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v


def emulate_standardise(x, take_abs):
    """standardise_kernel / standardise_regs_kernel: four interleaved channel-group partials, (r0 + r1) + (r2 + r3)."""
    v = f32(x)
    if take_abs:
        v = np.abs(v)
    B, C, L = v.shape
    Cf = np.float32(C)

    def group_sum(w):
        r = []
        for cg in range(4):
            s = np.zeros((B, L), np.float32)
            for c in range(cg, C, 4):
                s = s + w[:, c]
            r.append(s)
        return (r[0] + r[1]) + (r[2] + r[3])
    mean = (group_sum(v) / Cf)[:, None]
    d = v - mean
    var = group_sum(d * d) / np.float32(C - 1)
    den = (np.sqrt(var) + np.float32(1e-8))[:, None]
    return d / den


def emulate_mse(a, b):
    """mse_partial_kernel + mse_final_kernel: thread partials at stride 262144, butterfly, four waves, 1024 partials summed 4 per
    thread, the 256-wide tree, the division."""
    a, b = f32(a).ravel(), f32(b).ravel()
    n = a.size
    t = math.ceil(n / EW_THREADS)
    d = np.zeros(t * EW_THREADS, np.float32)
    d[:n] = a - b
    sq = (d * d).reshape(t, EW_THREADS)
    s = np.zeros(EW_THREADS, np.float32)
    for k in range(t):
        s = s + sq[k]
    w = _butterfly(s.reshape(EW_PARTIALS, 4, 64))[..., 0]
    parts = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    red = np.zeros(256, np.float32)
    for i in range(4):
        red = red + parts[i * 256:(i + 1) * 256]
    o = 128
    while o:
        red = red[:o] + red[o:2 * o]
        o >>= 1
    return np.float32(red[0] / np.float32(n))


def emulate_mse_backward(a, b, grad_loss):
    n = np.asarray(a).size
    g = np.float32(grad_loss) * np.float32(2.0 / n)
    return g * (f32(a) - f32(b))


def emulate_row_mean(x):
    """row_mean_kernel: lane partials at stride 64, the butterfly, the division."""
    x = f32(x)
    rows, L = x.shape
    t = math.ceil(L / 64)
    pad = np.zeros((rows, t * 64), np.float32)
    pad[:, :L] = x
    s = np.zeros((rows, 64), np.float32)
    for k in range(t):
        s = s + pad[:, k * 64:(k + 1) * 64]
    return _butterfly(s)[:, 0] / np.float32(L)


def emulate_row_mean_backward(dy, L):
    return np.repeat((f32(dy).reshape(-1, 1) * (np.float32(1.0) / np.float32(L))), L, axis=1)


def _fma(a, b, c):
    """float64 emulation of an fp32 fused multiply-add (the product of two fp32 values is exact in float64)."""
    return (f64(a) * f64(b) + f64(c)).astype(np.float32)


def emulate_adam(p, g, m, v, lr_bc1, bc2_sqrt, gscale, beta1, beta2, eps, fma=False):
    """adam_kernel in fp32 from fp32 scalars; ``fma``: with the three contractions a compiler may make."""
    p, g, m, v = f32(p), f32(g), f32(m), f32(v)
    lr_bc1, bc2_sqrt, gscale, beta1, beta2, eps = (np.float32(s) for s in (lr_bc1, bc2_sqrt, gscale, beta1, beta2, eps))
    one = np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        gr = g * gscale
        if fma:
            mm = _fma(gr - m, one - beta1, m)
            vv = _fma((one - beta2) * gr, gr, v * beta2)
        else:
            mm = m + (gr - m) * (one - beta1)
            vv = v * beta2 + (one - beta2) * gr * gr
        denom = np.sqrt(vv) / bc2_sqrt + eps
        q = mm / denom
        pn = _fma(-lr_bc1, q, p) if fma else p - lr_bc1 * q
    return pn, mm, vv


def emulate_bag_fwd(W, bias, idx, L, K):
    """embedding_bag_fwd_kernel: lane partials over l at stride 64, the butterfly, + bias."""
    W, idx = f32(W), np.asarray(idx)
    B, M = idx.shape[0], W.shape[0]
    ok = (idx >= 0) & (idx < K)
    col = np.arange(L)[None, :] * K + np.where(ok, idx, 0)
    terms = np.where(ok[None], W[:, col], np.float32(0.0)).astype(np.float32)         # (M, B, L)
    t = math.ceil(L / 64)
    pad = np.zeros((M, B, t * 64), np.float32)
    pad[..., :L] = terms
    s = np.zeros((M, B, 64), np.float32)
    for k in range(t):
        s = s + pad[..., k * 64:(k + 1) * 64]
    out = _butterfly(s)[..., 0].T
    return out + (f32(bias)[None] if bias is not None else np.float32(0.0))


def emulate_bag_bwd(dz, idx, L, K, dW0, db0=None):
    """embedding_bag_bwd_kernel: b sequential, += into the prefilled dW; db = (db0 +) the sequential sum over b."""
    dz, idx = f32(dz), np.asarray(idx)
    B, M = dz.shape
    dW = f32(dW0).copy()
    sb = np.zeros(M, np.float32)
    for b in range(B):
        sb = sb + dz[b]
        ok = (idx[b] >= 0) & (idx[b] < K)
        cols = (np.arange(L) * K + idx[b])[ok]
        dW[:, cols] = dW[:, cols] + dz[b][:, None]
    return dW, (sb if db0 is None else f32(db0) + sb)


# ============================================================================================================== grids
STD_C = (2, 3, 4, 5, 201, 255, 256, 257, 259, 513)       # 256 | 257: registers | three passes; C % 4 != 0 near it: ragged groups
STD_L = (1, 63, 64, 65, 130)


def standardise_cases():
    """(B, C, L): every C at two values of L, every L at C = 5 and 257; B alternates between 1 and 3."""
    out = []
    for i, C in enumerate(STD_C):
        for L in ((1, 130) if i % 2 == 0 else (63, 65)):
            out.append((C, L))
    for C in (5, 257):
        for L in STD_L:
            if (C, L) not in out:
                out.append((C, L))
    return [((1, 3)[i % 2], C, L) for i, (C, L) in enumerate(out)]


STD_CASES = standardise_cases()
STD_DATA = ("gauss", "offset100", "constant_columns")


def standardise_data(B, C, L, kind, take_abs=False):
    """fp32 (B, C, L) and the mask of its constant columns.  The bound is conditioned on max|x| / std, and the sample std of a
    few Gaussian values can be anything, so every (b, l) column is drawn, then moved in float64 to a chosen sample mean m and
    sample std s of the values the kernel standardises (v = x, or |x| with take_abs: then v >= 0 gets random signs):
      ``gauss``      s in [0.5, 2], |m| <= s (with take_abs: m = s (max|z| + r), r in [0, 1], so that v >= 0);
      ``offset100``  m = 100, s = 1: |mean| / std = 100, the largest ratio the tests use; a one-pass variance would lose it;
      ``constant_columns``  as gauss, with every third column (from the second) constant at 3.0: every fp32 sum of such a column is exact
                     (3 C <= 1539), so mean = 3, every deviation is +0 and y is exactly +0 = 0 / 1e-8."""
    rs = np.random.RandomState(1000 * C + 10 * L + B + (7 if take_abs else 0))
    z = rs.randn(B, C, L)
    z = z - z.mean(1, keepdims=True)
    z = z / np.sqrt((z * z).sum(1, keepdims=True) / (C - 1))
    if kind == "offset100":
        m, s = 100.0, 1.0
    else:
        s = rs.uniform(0.5, 2.0, (B, 1, L))
        m = s * (np.abs(z).max(1, keepdims=True) + rs.rand(B, 1, L)) if take_abs else s * rs.uniform(-1.0, 1.0, (B, 1, L))
    v = m + s * z
    const = np.zeros((B, L), bool)
    if kind == "constant_columns":
        const.ravel()[1::3] = True
        v = np.where(const[:, None, :], 3.0, v)
    if take_abs:
        assert (v >= 0).all()
        v = v * rs.choice([-1.0, 1.0], v.shape)
    return v.astype(np.float32), const


MSE_N = (1, 255, 256, 257, 262143, 262144, 262145, 1000003)       # 262144 = EW_PARTIALS x 256: one element per thread
PAST_GRID = 2 * 524288 + 5                                          # more than 2 x 524288: several passes of every thread's stride loop
PAST_CAP = 2048 * 1024 + 1029                                       # the grid (one block per 1024 elements) is capped at 2048 blocks here
MSE_BACKWARD_N = MSE_N + (PAST_GRID,)
GRAD_LOSS = (0.7, 1.0)


def mse_data(n, kind):
    """``lattice``: integer values with |a - b| <= 4, so n max (a-b)^2 <= 16 000 048 < 2^24 and every fp32 partial is exact."""
    rs = np.random.RandomState(n % 65521 + 7)
    if kind == "lattice":
        b = rs.randint(-8, 9, n)
        a = b + rs.randint(-4, 5, n)
        assert n * 16 < 2 ** 24
        return a.astype(np.float32), b.astype(np.float32)
    return rs.randn(n).astype(np.float32), (rs.randn(n) * 0.5 + 0.25).astype(np.float32)


ROW_MEAN_ROWS = ((1, 1), (1, 3), (2, 2), (1, 5), (5, 205))          # (B, D): rows = 1, 3, 4, 5, 1025
ROW_MEAN_L = (1, 63, 64, 65, 200, 1000)


def row_mean_data(rows, L, kind):
    rs = np.random.RandomState(rows * 1009 + L)
    if kind == "lattice":
        return rs.randint(-64, 65, (rows, L)).astype(np.float32)       # |sum| <= 64 000 < 2^24
    return (rs.randn(rows, L) + 0.5).astype(np.float32)


TRANSPOSE_DIMS = (1, 31, 32, 33, 65)
JITTER_L = (1, 2, 37, 300)
FLAT_N = (1, 255, 257, PAST_GRID, PAST_CAP)
FILL_N = (1, 2, 3, 4, 5, 1023, 1025, 4 * 524288 + 7)
FILL_VALUES = (0.0, -0.0, 1.5)

# Adam: hyper-parameters every form receives identically.  alvq_adam_f32 takes lr and the betas as fp32 and derives its scalars
# from those; values that fp32 holds exactly make its scalars the ones adam_advance derives from the doubles.
ADAM_LR, ADAM_BETA1, ADAM_BETA2, ADAM_EPS, ADAM_GSCALE = 2.0 ** -10, 0.875, 1.0 - 2.0 ** -10, 1e-8, 0.25
ADAM_N = (1, 1023, 1025, PAST_GRID)
ADVANCE_BETAS = ((0.9, 0.999), (0.5, 0.9))


def adam_data(n, seed=0):
    rs = np.random.RandomState(n % 65521 + seed)
    p = rs.randn(n).astype(np.float32)
    g = (rs.randn(n) * 4.0).astype(np.float32)
    m = (rs.randn(n) * 0.5).astype(np.float32)
    v = (rs.rand(n) * 0.5 + 1e-3).astype(np.float32)
    return p, g, m, v


def host_scalars(t, lr=ADAM_LR, beta1=ADAM_BETA1, beta2=ADAM_BETA2, grad_scale=ADAM_GSCALE):
    """The fp32 scalars as alvq_adam_f32 derives them on the host: double arithmetic from the fp32 arguments, rounded once."""
    lr, beta1, beta2 = float(np.float32(lr)), float(np.float32(beta1)), float(np.float32(beta2))
    s = adam_scalars(t, lr, beta1, beta2, grad_scale)
    return np.array([s[0], s[1], s[2], s[3], 0, 0, 0, 0], np.float32)


SEG_LENGTHS = (1, 2, 255, 1023, 1024, 1025, 2049)
SEG_COUNT = 50                                                       # AS_MAX = 48: a second chunk


def segments():
    """50 segments [lo, hi) of a flat buffer: the lengths in turn; adjacent, then a gap of 1, then a gap of 64.  -> (list, size)"""
    out, at = [], 3
    for i in range(SEG_COUNT):
        n = SEG_LENGTHS[i % len(SEG_LENGTHS)]
        out.append((at, at + n))
        at += n + (0, 1, 64)[i % 3]
    return out, max(at + 5, 60000)            # a long untouched tail behind the last segment


PACK_SHAPES = ((1, 1, 1), (32, 64, 3), (33, 65, 3), (5, 64, 1), (7, 128, 3), (7, 68, 3), (3, 66, 1), (40, 200, 3))
PACK_COUNT = 26                                                      # AP_MAX = 24: a second chunk
PACK_IMAGES = ("oik", "iok", "both", "none")
PACK_ALIGN = 64                                                      # floats: every tensor starts on a 256-byte boundary


def pack_descs():
    """26 (dim0, dim1, KW, images): the shapes in turn, the image choice moving one on with every pass through them."""
    return [PACK_SHAPES[i % len(PACK_SHAPES)] + (PACK_IMAGES[(i + i // len(PACK_SHAPES)) % 4],) for i in range(PACK_COUNT)]


BAG_SHAPES = ((1, 1, 1, 1), (2, 63, 4, 3), (3, 64, 5, 4), (3, 65, 7, 5), (256, 64, 8, 6), (5, 201, 16, 9))     # (B, L, K, M)
BAG_MAX_INDICES = 16384


def bag_data(shape, kind, bad=None):
    """W (M, L*K), bias (M), dz (B, M), idx (B, L) int32.  The last sample repeats the first (B > 1).  ``bad`` = -1 or "K": one
    index of sample 0 is out of range.  ``lattice``: integers; |W| <= 8, |dz| <= 8: every sum stays below 2^24."""
    B, L, K, M = shape
    rs = np.random.RandomState(B + 10 * L + 100 * K + M)
    if kind == "lattice":
        W = rs.randint(-8, 9, (M, L * K)).astype(np.float32)
        bias = rs.randint(-8, 9, M).astype(np.float32)
        dz = rs.randint(-8, 9, (B, M)).astype(np.float32)
    else:
        W, bias, dz = (rs.randn(*s).astype(np.float32) for s in ((M, L * K), (M,), (B, M)))
    idx = rs.randint(0, K, (B, L)).astype(np.int32)
    if B > 1:
        idx[-1] = idx[0]
    if bad is not None:
        idx[0, L // 2] = K if bad == "K" else -1
        if B > 1:
            idx[-1] = idx[0]
            idx[-1, L // 2] = 0
    return W, bias, dz, idx


ONEHOT_K = (1, 63, 64, 65, 1024)
