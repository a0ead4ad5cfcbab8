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
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "acoustic_locating_vq-vae_amd")
for p in (ROOT, PKG, os.path.join(PKG, "src"), os.path.join(ROOT, "tests", "helpers")):
    sys.path.insert(0, p)

F, T = 201, 500
SHAPES = ((64, 4, 3), (8, 8, 3))
ITER_LO, ITER_HI, ITER_CALL = 4, 12, 20
COPY_BYTES_PER_S = 6.3e12
FP64_FLOP_PER_S = 78.6e12
STEP_SECONDS = 300
STEPS = tuple("%d-%d-%d" % s for s in SHAPES)


def best_seconds(fn, reps):
    """Seconds per call of fn from device events around reps calls, the best of 5."""
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3 / reps)
    return best


def mixture(B, D, K):
    """(B, D, F, T) complex128 on the device: cacgmm_ref.case's recipe -- per source a per-frame activity gamma(0.3) + 1e-3 shared
    by all bins times complex Gaussian noise, mixed by a random complex D x K matrix per bin, plus noise at 0.05."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)

    def gauss(*shape):
        return torch.complex(torch.randn(shape, dtype=torch.float64, device="cuda", generator=g),
                             torch.randn(shape, dtype=torch.float64, device="cuda", generator=g))
    act = torch.distributions.Gamma(torch.tensor(0.3, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    torch.manual_seed(0)
    activity = act.sample((B, K, 1, T)).cuda() + 1e-3
    S = activity * gauss(B, K, F, T)
    X = torch.einsum("bfdk,bkft->bdft", gauss(B, F, D, K), S) + 0.05 * gauss(B, D, F, T)
    return X.contiguous()


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
    X = mixture(B, D, K)
    init = SEP.time_masks(B, K, F, T, generator=torch.Generator(device="cuda").manual_seed(1))
    lo = best_seconds(lambda: SEP.cacgmm(X, init, ITER_LO), 3)
    hi = best_seconds(lambda: SEP.cacgmm(X, init, ITER_HI), 3)
    call = best_seconds(lambda: SEP.cacgmm(X, init, ITER_CALL), 3)
    out = SEP.cacgmm(X, init, ITER_CALL)
    byte_floor, flop_floor = floors(B, D, K)
    x1, i1 = X[:1].cpu().numpy(), init[:1].cpu().numpy()
    t0 = time.perf_counter()
    ref = R.cacgmm(x1, i1, 2)
    cpu = (time.perf_counter() - t0) / 2
    two = SEP.cacgmm(X[:1].contiguous(), init[:1].contiguous(), 2)
    print(json.dumps({"step": name, "B": B, "D": D, "K": K, "F": F, "T": T, "dtype": "complex128",
                      "iteration_ms": (hi - lo) / (ITER_HI - ITER_LO) * 1e3,
                      "byte_floor_ms": byte_floor * 1e3, "fp64_floor_ms": flop_floor * 1e3, "call_ms_20_iterations": call * 1e3,
                      "outside_the_iterations_ms": (lo - ITER_LO * (hi - lo) / (ITER_HI - ITER_LO)) * 1e3,
                      "bins_with_status": int((out.status != 0).sum()),
                      "restatement_cpu_ms_per_iteration_at_B_1": cpu * 1e3,
                      "max_diff_of_masks_to_restatement_at_B_1": float(np.abs(two.masks.cpu().numpy() - ref.masks).max())}),
          flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        return step(sys.argv[2])
    for name in STEPS:
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], timeout=STEP_SECONDS,
                                  stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            sys.exit("bench_cacgmm: step %s ran out of its %d s; nothing more is started" % (name, STEP_SECONDS))
        if done.returncode != 0:
            sys.exit("bench_cacgmm: step %s ended with status %d; nothing more is started" % (name, done.returncode))
        print(done.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
