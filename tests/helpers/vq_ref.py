"""The vector quantiser (vq_vae/vector_quantizer.py:29-58, as oracle/vqvae_oracle.py restates it) once more in plain numpy
and float64, with the error bounds the float32 kernels of csrc/vq.hip are held to.  Nothing here is derived from the
kernels' arithmetic except what the bounds name: the float32 scalars the C API forms on the host (2 / (N D), its product with
grad_loss), the float32 quotient count / N of the perplexity, and the lengths of the kernels' summation chains.

u = 2^-24 is the unit roundoff of float32 throughout."""
import numpy as np

U = 2.0 ** -24
DIRECT_LIMIT = 1 << 24     # N K D up to which distances_auto takes the differences themselves
F32 = np.float32


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------ the search
def distances(x, e):
    """|x_n - e_k|^2 in float64 from the differences themselves (no cancellation), (N, K); row-chunked."""
    x64, e64 = _f64(x), _f64(e)
    n, d = x64.shape
    k = e64.shape[0]
    out = np.empty((n, k))
    step = max(1, (1 << 22) // max(1, k * d))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(0, n, step):
            diff = x64[i:i + step, None, :] - e64[None, :, :]
            out[i:i + step] = np.einsum("nkd,nkd->nk", diff, diff)
    return out


def distances_expanded(x, e):
    """|x|^2 + |e|^2 - 2 x.e in float64 (one GEMM): exact on the integer lattice; elsewhere within
    (D + 4) 2^-53 magnitude(x, e) of distances(), 2^-29 of the float32 bound -- for the shapes whose N K D is too large for
    the differences."""
    x64, e64 = _f64(x), _f64(e)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x64 * x64).sum(1)[:, None] + (e64 * e64).sum(1)[None, :] - 2.0 * (x64 @ e64.T)


def distances_auto(x, e):
    big = x.shape[0] * e.shape[0] * x.shape[1] > DIRECT_LIMIT
    return distances_expanded(x, e) if big else distances(x, e)


def magnitude(x, e):
    """|x|^2 + |e|^2 + 2 sum_i |x_i e_i|, (N, K) float64: the sum of the magnitudes of every term of the expanded distance."""
    x64, e64 = np.abs(_f64(x)), np.abs(_f64(e))
    return (x64 * x64).sum(1)[:, None] + (e64 * e64).sum(1)[None, :] + 2.0 * (x64 @ e64.T)


def error_bound(x, e, k=None):
    """The float32 search forms fl(fl(|x|^2 + |e|^2) - 2 x.e), each of the three sums of D float32 terms:
    |d32 - d64| <= (D + 4) u magnitude.  -> (N, K), or (N,) at the codes k[n]."""
    b = (x.shape[1] + 4) * U * magnitude(x, e)
    return b if k is None else b[np.arange(x.shape[0]), np.asarray(k)]


def argmin(x, e, d=None):
    """Lowest index among the exact minima (numpy's argmin returns the first)."""
    return np.argmin(distances_auto(x, e) if d is None else d, axis=1).astype(np.int64)


def margins(d):
    """Second-smallest minus smallest distance per row (K >= 2)."""
    p = np.partition(d, 1, axis=1)
    return p[:, 1] - p[:, 0]


# --------------------------------------------------------------------------------------------- gather, loss, perplexity
def loss_chain(n, d, partials=1024):
    """The longest chain of float32 additions between one squared difference and the loss: the rows of one wave (a quarter
    of a workgroup's ceil(N / 1024) rows) times ceil(D / 64) elements a lane, the workgroup sum (a 6-step butterfly and two
    pairwise steps), 1024 / 256 = 4 strided partials a thread and the 8 levels of the 256-tree."""
    per = -(-n // partials)
    return -(-per // 4) * -(-d // 64) + 8 + partials // 256 + 8


def loss_bound(n, d):
    """Relative: every term is non-negative; 3 u for the float32 difference (twice, squared) and the square."""
    return (loss_chain(n, d) + 3) * U


def perplexity(hist, n, p_float32=True):
    """-> (perplexity, sum |p log(p + 1e-10)|); p = count / N as float32 values (the kernel's), everything after in float64."""
    if p_float32:
        p = (hist.astype(F32) / F32(n)).astype(np.float64)
    else:
        p = hist.astype(np.float64) / float(n)
    t = p * np.log(p + 1e-10)
    return float(np.exp(-t.sum())), float(np.abs(t).sum())


C_LOG = 2    # ulp of the device logf (ROCm device library; not measured here)


def perplexity_bound(k, sum_abs):
    """Relative: the entropy's absolute error (ceil(K / 256) strided adds, 8 tree levels, logf) plus one expf rounding."""
    return (-(-k // 256) + 8 + C_LOG) * U * sum_abs + U


def gather_loss(x, e, idx, beta, ema=False, p_float32=True):
    """-> (q_st float32 = x + (e[idx] - x) in float32 arithmetic, loss float64, histogram int64, perplexity float64,
    sum |p log p| for the bound)."""
    x32, e32 = np.ascontiguousarray(x, F32), np.ascontiguousarray(e, F32)
    q = e32[idx]
    q_st = x32 + (q - x32)
    diff = _f64(e)[idx] - _f64(x)
    m = float((diff * diff).sum()) / (float(x.shape[0]) * float(x.shape[1]))
    loss = beta * m if ema else m + beta * m
    hist = np.bincount(idx, minlength=e.shape[0]).astype(np.int64)
    perp, sum_abs = perplexity(hist, x.shape[0], p_float32)
    return q_st, loss, hist, perp, sum_abs


# ------------------------------------------------------------------------------------------------------------- backward
def backward_scalars(grad_loss, n, d, beta):
    """(sx, se) as the C API forms them: float32(grad_loss) times the float32 constants 2 beta / (N D) and 2 / (N D)."""
    gl = F32(1.0 if grad_loss is None else grad_loss)
    nd = float(n) * float(d)
    return F32(gl * F32(2.0 * float(F32(beta)) / nd)), F32(gl * F32(2.0 / nd))


def backward(g, grad_loss, x, e, idx, beta):
    """-> (dx (N, D), dE (K, D), sum_abs (K, D), dx_mag (N, D)), float64:
      dx = g - sx (e[idx] - x);   dE[k] = se sum_{n: idx_n = k} (e[k] - x_n);   sum_abs[k] = |se| sum |e[k] - x_n|;
      dx_mag = |g| + |sx (e[idx] - x)|.   g and grad_loss may be None (0 and 1)."""
    n, d = x.shape
    k = e.shape[0]
    sx, se = (float(v) for v in backward_scalars(grad_loss, n, d, beta))
    diff = _f64(e)[idx] - _f64(x)
    g64 = np.zeros_like(diff) if g is None else _f64(g)
    dx = g64 - sx * diff
    dx_mag = np.abs(g64) + np.abs(sx * diff)
    order = np.argsort(idx, kind="stable")
    counts = np.bincount(idx, minlength=k)
    starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
    used = counts > 0
    dE = np.zeros((k, d))
    sum_abs = np.zeros((k, d))
    sd = diff[order]
    dE[used] = se * np.add.reduceat(sd, starts[used], axis=0)
    sum_abs[used] = abs(se) * np.add.reduceat(np.abs(sd), starts[used], axis=0)
    return dx, dE, sum_abs, dx_mag


def parts(n):
    """Row segments the codebook gradient splits a code's rows over (vq_parts)."""
    return min(16, max(1, n // 4096))


def groups(d):
    """Thread groups of the codebook-gradient kernel: 256 threads over D / 4 (D % 4 == 0) or D lanes."""
    return 256 // (d // 4 if d % 4 == 0 else d)


def dE_bound(counts, n, d, sum_abs):
    """(n_k + P + G + 2) u sum |term| per entry: n_k serial adds at worst, the G groups, the P segments, and the difference
    and product of each term."""
    return (counts[:, None] + parts(n) + groups(d) + 2) * U * sum_abs


def onehot(idx, k):
    enc = np.zeros((idx.shape[0], k), F32)
    enc[np.arange(idx.shape[0]), idx] = 1.0
    return enc
