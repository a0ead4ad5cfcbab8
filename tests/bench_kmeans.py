"""k-means on the device (acoustic_locating_vq_vae.kmeans, csrc/kmeans.hip) at the codebook-init shape N = 256 000 rows,
D = 128, K = 1024 (planted clusters).  Reports ms per Lloyd iteration split into the assignment (alvq_vq_argmin_f32, with its
fraction of the fp32 MFMA peak, 157.3 TFLOP/s, at the algorithmic 2 N K D) and the update (alvq_kmeans_update_f32); k-means++
seeding in total and per round; and the float64 restatement (tests/helpers/kmeans_ref.py) on the host at small N for a ratio.
    python tests/bench_kmeans.py [N]        (default 256000)
Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)
os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np
import torch

import kmeans_ref as R
from acoustic_locating_vq_vae import _native as N
from acoustic_locating_vq_vae import kmeans as KM

D, K, PEAK = 128, 1024, 157.3e12


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256000
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.randn(K, D, device="cuda", generator=g) * 3.0
    lab = torch.randint(K, (n,), device="cuda", generator=g)
    x = (centres[lab] + torch.randn(n, D, device="cuda", generator=g)).contiguous()
    mean, var_mean = N.kmeans_col_stats(x)
    xc = N.kmeans_add_rows(x, mean, -1.0)
    T = 2 + int(np.log(K))
    u = torch.rand((K - 1, T), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    seed_ms = FB.event_ms(lambda: KM._kmeans_plusplus(xc, K, 0, u), 3)
    init, _ = KM._kmeans_plusplus(xc, K, 0, u)
    labels = N.vq_argmin(xc, init)
    new = torch.empty_like(init)
    stats = torch.empty(1, device="cuda", dtype=torch.float64)
    flags = torch.empty(4, device="cuda", dtype=torch.int32)
    ws = N.kmeans_update(xc, labels, None, init, new, None, stats, flags, 0.0)
    assign_ms = FB.event_ms(lambda: N.vq_argmin(xc, init), 20)
    update_ms = FB.event_ms(lambda: N.kmeans_update(xc, labels, labels, init, new, None, stats, flags, 0.0, ws), 20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    km = KM.KMeans(n_clusters=K, random_state=0, max_iter=30).fit(x)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    # the float64 restatement on the host at small N: one Lloyd iteration and k-means++ seeding
    ns = 8000
    xs = xc[:ns].double().cpu().numpy()
    t0 = time.perf_counter()
    lab_s, _ = R.assign(xs, init.double().cpu().numpy())
    R.update(xs, lab_s, init.double().cpu().numpy(), K)
    ref_iter_ms = (time.perf_counter() - t0) * 1e3
    small = xc[:ns].contiguous()
    dev_iter_small = FB.event_ms(lambda: N.kmeans_update(small, N.vq_argmin(small, init), None, init, torch.empty_like(init),
                                                         None, stats, flags, 0.0), 10)
    us = u[:63]
    t0 = time.perf_counter()
    R.kmeans_plusplus(xs, 64, 0, us.numpy())
    ref_pp_ms = (time.perf_counter() - t0) * 1e3
    dev_pp_small = FB.event_ms(lambda: KM._kmeans_plusplus(small, 64, 0, us), 5)
    out = {
        "N": n, "D": D, "K": K,
        "lloyd_ms_per_iter": round(assign_ms + update_ms, 4),
        "assign_ms": round(assign_ms, 4), "update_ms": round(update_ms, 4),
        "assign_fp32_mfma_peak_fraction": round(2.0 * n * K * D / (assign_ms * 1e-3) / PEAK, 3),
        "kmeans_pp_ms": round(seed_ms, 2), "kmeans_pp_us_per_round": round(seed_ms * 1e3 / K, 2),
        "fit_s_max_iter_30": round(fit_s, 3), "fit_n_iter": km.n_iter_,
        "ref_f64_small_N": ns, "ref_f64_lloyd_iter_ms": round(ref_iter_ms, 2), "dev_lloyd_iter_ms_small_N": round(dev_iter_small, 4),
        "lloyd_ratio_small_N": round(ref_iter_ms / dev_iter_small, 1),
        "ref_f64_pp_ms_K64": round(ref_pp_ms, 2), "dev_pp_ms_K64": round(dev_pp_small, 3),
        "pp_ratio_small_N": round(ref_pp_ms / dev_pp_small, 1),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
