"""STOI on the device (speech_metrics.stoi, csrc/speech_metrics.hip): the time of one call at B = 64, n = 80000, fs = 16000
(five seconds of speech a row) from device events, the best of 5, and of its stages (the two resampling launches, the four of
STOI at 10 kHz), next to the least time one read of both inputs could take (2 B n 8 bytes at the measured HBM rate of
6.3 TB/s) and to the float64 restatement (tests/helpers/speech_metrics_ref.py, scipy.signal.resample_poly for its resampling)
on host threads.
    python tests/bench_speech_metrics.py [cpu_threads=16]
For the kernels' own times run it once under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)
import numpy as np
import scipy.signal
import torch

import speech_metrics_ref as R
from acoustic_locating_vq_vae import speech_metrics as M

B, N, FS = 64, 80000, 16000


def host_row(pair):
    clean, degraded = (scipy.signal.resample_poly(v, 10000, FS) for v in pair)
    return R.stoi(clean, degraded).value


def host_rows_per_second(clean, degraded, threads, rows):
    pairs = [(clean[i], degraded[i]) for i in range(rows)]
    host_row(pairs[0])
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        values = list(ex.map(host_row, pairs))
    return rows / (time.perf_counter() - t0), values


def main():
    threads = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.arange(N, dtype=torch.float64, device="cuda")[None] / FS
    rate = 3.0 + 2.0 * torch.rand(B, 1, dtype=torch.float64, device="cuda", generator=g)
    clean = torch.randn(B, N, dtype=torch.float64, device="cuda", generator=g) * (0.55 + 0.45 * torch.sin(2 * np.pi * rate * t))
    degraded = clean + 0.5 * torch.randn(B, N, dtype=torch.float64, device="cuda", generator=g)
    c10, d10 = M.resample_poly(clean, 10000, FS), M.resample_poly(degraded, 10000, FS)

    whole = FB.best_seconds(lambda: M.stoi(clean, degraded, fs=FS), 20)
    resample = FB.best_seconds(lambda: (M.resample_poly(clean, 10000, FS), M.resample_poly(degraded, 10000, FS)), 20)
    at_10k = FB.best_seconds(lambda: M.stoi(c10, d10, fs=10000), 20)
    got = M.stoi(clean, degraded, fs=FS)
    assert got.status.tolist() == [0] * B
    rows = 32
    cpu, values = host_rows_per_second(clean.cpu().numpy(), degraded.cpu().numpy(), threads, rows)
    err = float(np.abs(got.value[:rows].cpu().numpy() - np.array(values)).max())
    bound = 2 * B * N * 8 / FB.COPY_BYTES_PER_S
    print(json.dumps({"B": B, "n": N, "fs": FS, "gpu_us_per_call": whole * 1e6, "resample_us": resample * 1e6,
                      "stoi_at_10k_us": at_10k * 1e6, "one_read_bound_us": bound * 1e6, "ratio_to_bound": whole / bound,
                      "gpu_rows_per_s": B / whole, "cpu_rows_per_s": cpu, "cpu_threads": threads, "cpu_rows_timed": rows,
                      "gpu_over_cpu": B / whole / cpu, "kept_frames_mean": float(got.kept_frames.double().mean()),
                      "max_abs_diff_to_restatement": err}), flush=True)


if __name__ == "__main__":
    main()
