"""Float64 restatement of VectorQuantizerEMA (acoustic_locating_vq_vae/vq_vae/vector_quantizer.py): the per-code statistics,
the five-step update, the forward's loss / perplexity and the gradient that reaches the encoder rows."""
import numpy as np


def stats(rows, idx, K):
    """c[k] = #rows with idx == k, s[k] = their sum."""
    rows = np.asarray(rows, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    c = np.bincount(idx, minlength=K).astype(np.float64)
    s = np.zeros((K, rows.shape[1]))
    np.add.at(s, idx, rows)
    return c, s


def update(cs, W, c, s, decay, eps):
    """Steps 1-5 -> (cs, W, E)."""
    cs = np.asarray(cs, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    K = cs.shape[0]
    cs = decay * cs + (1.0 - decay) * np.asarray(c, dtype=np.float64)
    n = cs.sum()
    cs = (cs + eps) / (n + K * eps) * n
    W = decay * W + (1.0 - decay) * np.asarray(s, dtype=np.float64)
    return cs, W, W / cs[:, None]


def update_rounded(cs, W, c, s, decay, eps):
    """Steps 1-5 with the roundings the header states: fp64 arithmetic on the fp32 state, the cluster size rounded to fp32
    once (after the smoothing), the moving sum rounded once, and the codebook the fp32 quotient of the two stored values.
    -> (cs, W, E), all fp32."""
    cs = np.asarray(cs, dtype=np.float32).astype(np.float64)
    W = np.asarray(W, dtype=np.float32).astype(np.float64)
    K = cs.shape[0]
    cs = decay * cs + (1.0 - decay) * np.asarray(c, dtype=np.float32).astype(np.float64)
    n = cs.sum()
    cs32 = ((cs + eps) / (n + K * eps) * n).astype(np.float32)
    W32 = (decay * W + (1.0 - decay) * np.asarray(s, dtype=np.float32).astype(np.float64)).astype(np.float32)
    return cs32, W32, (W32 / cs32[:, None]).astype(np.float32)


def step(cs, W, rows, idx, decay, eps):
    c, s = stats(rows, idx, np.asarray(cs).shape[0])
    return update(cs, W, c, s, decay, eps)


def forward(rows, E, idx, beta):
    """(loss = beta * mean((q - x)^2), perplexity, q = E[idx]) with the codebook the rows were quantised with."""
    x = np.asarray(rows, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    q = E[idx]
    m = np.mean((q - x) ** 2)
    p = np.bincount(idx, minlength=E.shape[0]) / float(len(idx))
    return beta * m, float(np.exp(-np.sum(p * np.log(p + 1e-10)))), q


def grad_rows(rows, E, idx, beta, g, gl=1.0):
    """d(gl * loss + <g, q_st>)/d rows = g - gl * 2 beta / (N D) * (E[idx] - x)."""
    x = np.asarray(rows, dtype=np.float64)
    q = np.asarray(E, dtype=np.float64)[np.asarray(idx, dtype=np.int64)]
    return np.asarray(g, dtype=np.float64) - gl * 2.0 * beta / x.size * (q - x)
