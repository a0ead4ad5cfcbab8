"""Exact t-SNE on the device (acoustic_locating_vq_vae.tsne, csrc/tsne.hip) at the analysis' shape: code sequences of L = 201
positions over K = 1024 codes (three planted clusters, 10 % of codes re-drawn), perplexity 100, 1000 iterations.  Reports per N:
distance and affinity time, descent ms/iteration (a whole TSNE fit minus its distances and affinities, over the iterations
run), the achieved HBM rate of descent pass (b) (N^2 fp32 of P read per iteration, over the descent time per iteration: a lower
bound, since passes (a) and the reductions are in that time), and the float64 restatement (tests/helpers/tsne_ref.py) on the
host at small N for a ratio.
    python tests/bench_tsne.py [N ...]        (default 1000 5000 20000)
For the per-kernel split run it once under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench  # noqa: E402,F401  (it puts the repository, the package and tests/helpers on the path)
os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np
import torch

import tsne_ref as R
from acoustic_locating_vq_vae import _native as N
from acoustic_locating_vq_vae import tsne as T

L, K, PERP, ITERS = 201, 1024, 100.0, 1000


def codes_for(n, seed=0):
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, K, (3, L))
    x = centres[np.arange(n) % 3].copy()
    flip = rng.random(x.shape) < 0.1
    x[flip] = rng.integers(0, K, int(flip.sum()))
    return x


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def gpu(n):
    c = torch.from_numpy(codes_for(n)).to("cuda")
    T.code_sq_distances(c[:64])                                   # warm the code objects
    t_d2, d2 = sync_time(lambda: T.code_sq_distances(c))
    t_aff, _ = sync_time(lambda: N.tsne_affinities(d2, PERP))
    d2 = None
    t = T.TSNE(perplexity=PERP, max_iter=ITERS, random_state=0)
    t_fit, _ = sync_time(lambda: t.fit_transform(c))
    iters = t.n_iter_ + 1
    ms_it = (t_fit - t_d2 - t_aff) / iters * 1e3
    return {"N": n, "sqdist_ms": t_d2 * 1e3, "affinities_ms": t_aff * 1e3, "fit_s": t_fit, "iterations": iters,
            "descent_ms_per_iter": ms_it, "pass_b_hbm_tb_s_lower_bound": 4.0 * n * n / (ms_it * 1e-3) / 1e12,
            "kl": t.kl_divergence_}


def cpu(n, iters=20):
    """The restatement (numpy float64, OMP_NUM_THREADS threads for its BLAS) for the affinities and `iters` iterations."""
    d2 = R.code_sqdist(codes_for(n))
    t0 = time.perf_counter()
    P, *_ = R.affinities(d2, PERP)
    t_aff = time.perf_counter() - t0
    Y0 = np.random.default_rng(0).standard_normal((n, 2)) * 1e-4
    t0 = time.perf_counter()
    R.descend(P, Y0, iters, 12.0, 0.5, max(n / 48.0, 50.0))
    return {"N": n, "affinities_s": t_aff, "descent_ms_per_iter": (time.perf_counter() - t0) / iters * 1e3}


def main():
    ns = [int(a) for a in sys.argv[1:]] or [1000, 5000, 20000]
    res = {"gpu": [gpu(n) for n in ns], "cpu": [cpu(n) for n in (1000, 2000)], "cpu_threads": os.environ["OMP_NUM_THREADS"]}
    g = {r["N"]: r for r in res["gpu"]}
    res["ratio_descent_at_1000"] = res["cpu"][0]["descent_ms_per_iter"] / g[1000]["descent_ms_per_iter"] if 1000 in g else None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
