"""cACGMM on the device (acoustic_locating_vq_vae.separation.cacgmm, csrc/cacgmm.hip): the time of one iteration (priors, M-step,
E-step: the difference of two iteration counts divided by their distance) and of the whole call with the default 20 iterations,
at (B, D, K, F, T) = (64, 4, 3, 201, 500), the dataset's shape on a four-microphone array, and (8, 8, 3, 201, 500), complex128,
from device events, the best of 5 -- next to the two floors an iteration has: its bytes (X twice, gamma three times and q twice)
at the 6.3 TB/s a copy reaches, and the float64 arithmetic of the two passes over X at the vector rate of
78.6 TFLOP/s (datasheet) -- and next to the numpy restatement (tests/helpers/cacgmm_ref.py) on the CPU at a batch of one.  There
is no ratio to pass: nothing did this before.
    python tests/bench_cacgmm.py
Each measurement runs in a child process of its own under a time limit; a child that fails or runs out of time ends the script,
and nothing more is started on the device.  For the kernels' own times run `python tests/bench_cacgmm.py --step 64-4-3` once under
rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)

from family_bench import COPY_BYTES_PER_S, FP64_FLOP_PER_S, ITER_CALL, F, T  # noqa: E402

SHAPES = ((64, 4, 3), (8, 8, 3))
STEPS = tuple("%d-%d-%d" % s for s in SHAPES)


def floors(B, D, K):
    """(the byte floor, the float64 floor) of one iteration in seconds.  Bytes a frame and bin: X twice (M-step and E-step,
    16 D each), gamma read by the priors and the M-step and written by the E-step, q read by the M-step and written by the
    E-step (8 K each).  Arithmetic a frame, bin and class: the M-step's D^2 real sums, a term of 3 flop and a fused multiply-add
    by the weight; the E-step's D^2 complex multiply-adds (8 flop each) plus 4 D for the |y_i|^2."""
    frames = B * F * T
    return frames * (32 * D + 40 * K) / COPY_BYTES_PER_S, frames * K * (5 * D * D + 8 * D * D + 4 * D) / FP64_FLOP_PER_S


def step(name):
    import numpy as np
    import torch
    import cacgmm_ref as R
    from acoustic_locating_vq_vae import separation as SEP
    B, D, K = (int(v) for v in name.split("-"))
    X = FB.mixture(B, D, K, torch.complex128, noise=0.05)
    init = SEP.time_masks(B, K, F, T, generator=torch.Generator(device="cuda").manual_seed(1))
    iteration, call, outside = FB.iteration_ms(lambda n: SEP.cacgmm(X, init, n))
    out = SEP.cacgmm(X, init, ITER_CALL)
    byte_floor, flop_floor = floors(B, D, K)
    x1, i1 = X[:1].cpu().numpy(), init[:1].cpu().numpy()
    t0 = time.perf_counter()
    ref = R.cacgmm(x1, i1, 2)
    cpu = (time.perf_counter() - t0) / 2
    two = SEP.cacgmm(X[:1].contiguous(), init[:1].contiguous(), 2)
    print(json.dumps({"step": name, "B": B, "D": D, "K": K, "F": F, "T": T, "dtype": "complex128",
                      "iteration_ms": iteration,
                      "byte_floor_ms": byte_floor * 1e3, "fp64_floor_ms": flop_floor * 1e3, "call_ms_20_iterations": call,
                      "outside_the_iterations_ms": outside,
                      "bins_with_status": int((out.status != 0).sum()),
                      "restatement_cpu_ms_per_iteration_at_B_1": cpu * 1e3,
                      "max_diff_of_masks_to_restatement_at_B_1": float(np.abs(two.masks.cpu().numpy() - ref.masks).max())}),
          flush=True)


def main():
    FB.main(__file__, STEPS, step)


if __name__ == "__main__":
    main()
