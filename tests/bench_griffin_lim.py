"""Utterances/s of Griffin-Lim (front_end.griffin_lim): B = 64 five-second utterances at 16 kHz, n_fft 400, hop 160, 32
iterations, float32, HIP kernels vs the CPU restatement (tests/helpers/griffin_lim_ref.py on torch.stft / torch.istft) on the
host cores, plus the kernel time per iteration.    python tests/bench_griffin_lim.py [batch=64] [n_iter=32]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench  # noqa: E402,F401  (it puts the repository, the package and tests/helpers on the path)
import torch

import griffin_lim_ref as GL
from acoustic_locating_vq_vae import _native as N
from acoustic_locating_vq_vae import front_end as FE


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    n_iter = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    S, n_fft, hop = 80000, 400, 160
    g = torch.Generator().manual_seed(0)
    wave = torch.randn(B, S, generator=g)
    power = N.stft_power(wave.cuda(), n_fft, hop)
    init = torch.rand(power.shape, dtype=torch.complex64, generator=g)
    init_d = init.cuda()
    for _ in range(2):
        FE.griffin_lim(power, n_iter=n_iter, init=init_d)
    torch.cuda.synchronize()
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        FE.griffin_lim(power, n_iter=n_iter, init=init_d)
    torch.cuda.synchronize()
    t_call = (time.perf_counter() - t0) / reps
    # kernel time per iteration: the difference of n_iter and 0 iterations, timed with events on the stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    FE.griffin_lim(power, n_iter=n_iter, init=init_d)
    ev[1].record()
    FE.griffin_lim(power, n_iter=0, init=init_d)
    ev[2].record()
    torch.cuda.synchronize()
    per_iter = (ev[0].elapsed_time(ev[1]) - ev[1].elapsed_time(ev[2])) * 1e-3 / max(n_iter, 1)
    # the CPU restatement on a slice of the batch (it scales linearly in B)
    n_cpu = min(B, 4)
    mag = power[:n_cpu].cpu().sqrt()
    t0 = time.perf_counter()
    GL.griffin_lim(mag, init[:n_cpu], n_iter, 0.99, n_fft, hop)
    cpu = n_cpu / (time.perf_counter() - t0)
    # direct DFT work per iteration: forward + inverse, 2 real MACs per (bin, sample) each way
    F, T = n_fft // 2 + 1, 1 + S // hop
    flop_iter = 2 * 4.0 * B * T * F * n_fft
    print(json.dumps({"batch": B, "n_iter": n_iter, "gpu_utterances_per_s": B / t_call, "gpu_ms_per_call": t_call * 1e3,
                      "kernel_ms_per_iter": per_iter * 1e3, "dft_tflops": flop_iter / per_iter / 1e12,
                      "cpu_utterances_per_s": cpu, "cpu_threads": torch.get_num_threads(), "ratio": B / t_call / cpu}))


if __name__ == "__main__":
    main()
