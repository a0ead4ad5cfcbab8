"""Float64 numpy restatement of exact t-SNE as acoustic_locating_vq_vae/tsne.py states it (sklearn's TSNE(method="exact",
n_components=2) semantics, items 1-6 of that docstring), written from the description, for the tests of csrc/tsne.hip.
Includes row-subset evaluators (the search, P and gradient of rows S only, O(|S| N)) for the large-N checks."""
import numpy as np

EPS = np.finfo(np.float64).eps
EXPLORATION_N_ITER = 250
N_ITER_CHECK = 50


def code_sqdist(codes, rows=None):
    """d2[i][j] = 2 (L - matches) as fp32, for all rows or the rows given."""
    c = np.asarray(codes)
    sel = c if rows is None else c[np.asarray(rows)]
    L = c.shape[1]
    out = np.empty((sel.shape[0], c.shape[0]), dtype=np.float32)
    for a in range(sel.shape[0]):
        out[a] = 2 * (L - (c == sel[a]).sum(axis=1))
    return out


def onehot_sqdist(codes, K):
    """The same distance from the dense one-hot expansion (the definition)."""
    c = np.asarray(codes)
    x = np.zeros((c.shape[0], c.shape[1] * K), dtype=np.float64)
    x[np.arange(c.shape[0])[:, None], np.arange(c.shape[1]) * K + c] = 1.0
    g = x @ x.T
    sq = np.diag(g)
    return sq[:, None] + sq[None, :] - 2 * g


def search_rows(d2_rows, rows, perplexity, near=1e-12):
    """Item 2 for the given rows (d2_rows[a] is the fp32 distance row of point rows[a]).  Returns (Pc fp32 rows, beta, S,
    entropy H of the last evaluation, flagged): flagged[a] when one of the row's decisions (the stop test or the direction)
    lies within `near` of its threshold, so that rounding elsewhere may flip it."""
    d = np.asarray(d2_rows, dtype=np.float64).copy()
    rows = np.asarray(rows)
    n = d.shape[0]
    mask = np.ones_like(d, dtype=bool)
    mask[np.arange(n), rows] = False
    target = np.log(perplexity)
    beta = np.ones(n)
    bmin = np.full(n, -np.inf)
    bmax = np.full(n, np.inf)
    used = np.ones(n)
    S = np.ones(n)
    H = np.zeros(n)
    active = np.ones(n, dtype=bool)
    flagged = np.zeros(n, dtype=bool)
    for _ in range(100):
        if not active.any():
            break
        a = np.nonzero(active)[0]
        P = np.where(mask[a], np.exp(-d[a] * beta[a][:, None]), 0.0)
        s = P.sum(axis=1)
        sd = (d[a] * P).sum(axis=1)
        s = np.where(s == 0.0, 1e-8, s)
        h = np.log(s) + beta[a] * (sd / s)
        used[a], S[a], H[a] = beta[a], s, h
        dev = h - target
        flagged[a] |= (np.abs(np.abs(dev) - 1e-5) < near) | (np.abs(dev) < near)
        done = np.abs(dev) <= 1e-5
        up = (~done) & (dev > 0)
        dn = (~done) & (dev <= 0)
        bu, bd = a[up], a[dn]
        bmin[bu] = beta[bu]
        beta[bu] = np.where(np.isinf(bmax[bu]), beta[bu] * 2.0, (beta[bu] + bmax[bu]) / 2.0)
        bmax[bd] = beta[bd]
        beta[bd] = np.where(np.isinf(bmin[bd]), beta[bd] / 2.0, (beta[bd] + bmin[bd]) / 2.0)
        active[a[done]] = False
    with np.errstate(over="ignore"):                         # the masked diagonal, exp(0) / S, may overflow
        Pc = np.where(mask, np.exp(-d * used[:, None]) / S[:, None], 0.0).astype(np.float32)
    return Pc, used, S, H, flagged


def conditional_p(d2, perplexity):
    n = d2.shape[0]
    return search_rows(d2, np.arange(n), perplexity)


def joint_p(Pc):
    """Item 3: (Pc + Pc^T) in fp32, normalised by the fp64 sum and clamped, diagonal 0."""
    P = Pc + Pc.T
    np.fill_diagonal(P, 0.0)
    total = max(P.astype(np.float64).sum(), EPS)
    out = np.maximum(P.astype(np.float64) / total, EPS).astype(np.float32)
    np.fill_diagonal(out, 0.0)
    return out


def affinities(d2, perplexity):
    Pc, beta, S, H, flagged = conditional_p(d2, perplexity)
    return joint_p(Pc), beta, S, H, flagged


def num_matrix(Y):
    diff = Y[:, None, :] - Y[None, :, :]
    num = 1.0 / (1.0 + (diff[..., 0] ** 2 + diff[..., 1] ** 2))
    np.fill_diagonal(num, 0.0)
    return num


def z_of(Y, chunk=2048):
    Y = np.asarray(Y, dtype=np.float64)
    z = 0.0
    for a in range(0, Y.shape[0], chunk):
        d = ((Y[a:a + chunk, None, :] - Y[None, :, :]) ** 2).sum(-1)
        num = 1.0 / (1.0 + d)
        idx = np.arange(a, min(a + chunk, Y.shape[0]))
        num[idx - a, idx] = 0.0
        z += num.sum()
    return z


def kl_grad(P, Y, exaggeration, want_kl=True):
    """Item 4 on all rows: (KL or None, grad (N, 2))."""
    P = np.asarray(P, dtype=np.float64)
    num = num_matrix(Y)
    Z = num.sum()
    off = ~np.eye(P.shape[0], dtype=bool)
    Q = np.maximum(num / Z, EPS)
    eP = exaggeration * P
    coef = (eP - Q) * num * off
    grad = 4.0 * (coef.sum(1)[:, None] * Y - coef @ Y)
    kl = None
    if want_kl:
        kl = float((eP * np.log(np.maximum(eP, EPS) / Q))[off].sum())
    return kl, grad


def grad_rows(P_rows, Y, rows, exaggeration, Z=None):
    """The gradient of rows S only, O(|S| N): P_rows[a] is the P row of point rows[a]."""
    Y = np.asarray(Y, dtype=np.float64)
    Z = z_of(Y) if Z is None else Z
    rows = np.asarray(rows)
    diff = Y[rows][:, None, :] - Y[None, :, :]
    num = 1.0 / (1.0 + (diff ** 2).sum(-1))
    num[np.arange(rows.size), rows] = 0.0
    Q = np.maximum(num / Z, EPS)
    coef = (exaggeration * np.asarray(P_rows, dtype=np.float64) - Q) * num
    coef[np.arange(rows.size), rows] = 0.0
    return 4.0 * (coef[..., None] * diff).sum(1)


def apply_step(Y, update, gains, grad, momentum, lr):
    """Item 5's per-iteration update on copies: returns (Y, update, gains, gained grad)."""
    inc = update * grad < 0.0
    gains = np.where(inc, gains + 0.2, gains * 0.8)
    gains = np.maximum(gains, 0.01)
    grad = grad * gains
    update = momentum * update - lr * grad
    return Y + update, update, gains, grad


def descend(P, Y, n_iter, exaggeration, momentum, lr, update=None, gains=None):
    """n_iter iterations of one phase.  Returns (Y, update, gains, last gained grad, KL of the last iteration, |grad|)."""
    Y = np.array(Y, dtype=np.float64)
    update = np.zeros_like(Y) if update is None else np.array(update, dtype=np.float64)
    gains = np.ones_like(Y) if gains is None else np.array(gains, dtype=np.float64)
    kl = grad = None
    for k in range(n_iter):
        kl, g = kl_grad(P, Y, exaggeration, want_kl=k == n_iter - 1)
        Y, update, gains, grad = apply_step(Y, update, gains, g, momentum, lr)
    return Y, update, gains, grad, kl, float(np.linalg.norm(grad))


def gradient_descent(objective, it, n_iter, n_iter_without_progress, min_grad_norm):
    """sklearn's per-iteration loop with an abstract objective: objective(i, compute_error) -> (error or None, grad norm after
    the gains).  Returns (error, last i)."""
    error = None
    best_error, best_iter = np.finfo(float).max, it
    i = it - 1
    for i in range(it, n_iter):
        check = (i + 1) % N_ITER_CHECK == 0
        e, grad_norm = objective(i, check or i == n_iter - 1)
        if e is not None:
            error = e
        if check:
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if grad_norm <= min_grad_norm:
                break
    return error, i


def schedule(objective, max_iter, n_iter_without_progress=300, min_grad_norm=1e-7):
    """Item 5's two phases over objective(phase, i, compute_error).  Returns (kl_divergence_, n_iter_)."""
    kl, it = gradient_descent(lambda i, c: objective(0, i, c), 0, EXPLORATION_N_ITER, EXPLORATION_N_ITER, min_grad_norm)
    kl2, it2 = gradient_descent(lambda i, c: objective(1, i, c), it + 1, max_iter, n_iter_without_progress, min_grad_norm)
    if it2 >= it + 1:
        kl, it = kl2, it2
    return kl, it


def tsne(d2, perplexity, Y0, max_iter=1000, early_exaggeration=12.0, lr=None, n_iter_without_progress=300,
         min_grad_norm=1e-7, P=None):
    """The whole fit from a given init (small N only), from d2 or from a given joint P.  Returns (Y, kl, n_iter_,
    {iteration: KL} at every computed KL)."""
    if P is None:
        P, _, _, _, _ = affinities(np.asarray(d2, dtype=np.float32), perplexity)
    n = P.shape[0]
    lr = max(n / early_exaggeration / 4.0, 50.0) if lr is None else lr
    st = {"Y": np.array(Y0, dtype=np.float64), "phase": -1}
    kls = {}

    def objective(phase, i, compute):
        if phase != st["phase"]:
            st["phase"], st["u"], st["g"] = phase, np.zeros_like(st["Y"]), np.ones_like(st["Y"])
        e, m = (early_exaggeration, 0.5) if phase == 0 else (1.0, 0.8)
        kl, g = kl_grad(P, st["Y"], e, want_kl=compute)
        st["Y"], st["u"], st["g"], gg = apply_step(st["Y"], st["u"], st["g"], g, m, lr)
        if compute:
            kls[i] = kl
        return kl, float(np.linalg.norm(gg))

    kl, it = schedule(objective, max_iter, n_iter_without_progress, min_grad_norm)
    return st["Y"], kl, it, kls
