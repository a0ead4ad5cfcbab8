"""Numpy restatement of VectorQuantizerEMA's dead-code restarts (acoustic_locating_vq_vae/vq_vae/vector_quantizer.py), built on
vq_ema_ref: ``restart`` in float64, ``restart32`` with the roundings the contract states (fp32 compare against the fp32
threshold, copies, one fp32 product), the EMA step followed by the restart in both, and the planted-collapse problem."""
import numpy as np

import vq_ema_ref as E_


def _restart(cs, W, E, cand, threshold, dt):
    cs, W, E = (np.array(a, dtype=dt) for a in (cs, W, E))
    cand = np.asarray(cand, dtype=dt)
    thr = dt(threshold)
    dead = np.flatnonzero(cs < thr)                      # ascending k
    n = min(len(dead), len(cand))
    k = dead[:n]
    E[k] = cand[:n]
    W[k] = cand[:n] * thr
    cs[k] = thr
    return cs, W, E, n, len(dead)


def restart(cs, W, E, cand, threshold):
    """-> (cs, W, E, n restarted, dead before the cap), float64.  cand: (R, D), R the cap."""
    return _restart(cs, W, E, cand, threshold, np.float64)


def restart32(cs, W, E, cand, threshold):
    """The same on fp32 state with fp32 arithmetic: what the device computes, bit for bit."""
    return _restart(cs, W, E, cand, threshold, np.float32)


def step(cs, W, rows, idx, decay, eps, cand, threshold):
    """vq_ema_ref.step, then the restart (float64)."""
    return restart(*E_.step(cs, W, rows, idx, decay, eps), cand, threshold)


def step32(cs, W, c, s, decay, eps, cand, threshold):
    """vq_ema_ref.update_rounded on the statistics (c, s), then the fp32 restart."""
    return restart32(*E_.update_rounded(cs, W, c, s, decay, eps), cand, threshold)


# ---------------------------------------------------------------------------------------------- the planted collapse
PLANTED = dict(K=64, D=16, N=2048, C=48, steps=40, decay=0.9, eps=1e-5, R=16, threshold=1.0, scale=4.0, noise=0.1)


def planted_stream(seed, on):
    """First (E0, W0), then ``steps`` times (x (N, D), rows (R,) or None): 48 centres ~ N(0, 4^2), rows = a centre plus 0.1
    noise; ``rows`` = permutation(N)[:R], drawn (from the same generator, after the step's data) only when ``on``."""
    p = PLANTED
    g = np.random.default_rng(seed)
    centres = g.normal(size=(p["C"], p["D"])) * p["scale"]
    E0 = g.normal(size=(p["K"], p["D"]))
    W0 = g.normal(size=(p["K"], p["D"]))
    yield E0, W0
    for _ in range(p["steps"]):
        lab = g.integers(0, p["C"], size=p["N"])
        x = centres[lab] + p["noise"] * g.normal(size=(p["N"], p["D"]))
        yield x, (g.permutation(p["N"])[:p["R"]] if on else None)


def planted(seed, on):
    """The float64 restatement on the planted problem -> (codes used on the last step, its mean squared quantisation error,
    codes restarted in all)."""
    p = PLANTED
    stream = planted_stream(seed, on)
    E, W = next(stream)
    cs = np.zeros(p["K"])
    total = 0
    for x, rows in stream:
        d = (x * x).sum(1)[:, None] - 2 * x @ E.T + (E * E).sum(1)[None]
        idx = d.argmin(1)
        mse = float(((E[idx] - x) ** 2).mean())
        used = len(np.unique(idx))
        if on:
            cs, W, E, n, _ = step(cs, W, x, idx, p["decay"], p["eps"], x[rows], p["threshold"])
            total += n
        else:
            cs, W, E = E_.step(cs, W, x, idx, p["decay"], p["eps"])
    return used, mse, total
