"""AuxIVA on the device (acoustic_locating_vq_vae.separation, csrc/iva.hip): the time of one iteration (activity, weights,
update: the difference of two iteration counts divided by their distance) and of the whole call with the default 20 iterations,
at (B, D, F, T) = (64, 2, 201, 500), the dataset's shape, and (8, 8, 201, 500), complex64 and complex128, from device events,
the best of 5 -- next to the two floors an iteration has: X read twice (activity and update) at the 6.3 TB/s a copy reaches
(DESIGN.md), and the float64 arithmetic of the two passes at the vector rate of 78.6 TFLOP/s (datasheet) -- and next to the
numpy restatement (tests/helpers/iva_ref.py) on the CPU at a batch of one.  There is no ratio to pass: nothing did this before.
    python tests/bench_iva.py
Each measurement runs in a child process of its own under a time limit; a child that fails or runs out of time ends the script,
and nothing more is started on the device.  For the kernels' own times run `python tests/bench_iva.py --step 64-2-complex128` once
under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)

from family_bench import COPY_BYTES_PER_S, FP64_FLOP_PER_S, ITER_CALL, F, T  # noqa: E402

SHAPES = ((64, 2), (8, 8))
STEPS = tuple("%d-%d-%s" % (B, D, c) for B, D in SHAPES for c in ("complex64", "complex128"))


def floors(B, D, itemsize):
    """(the byte floor, the float64 floor) of one iteration in seconds.  Bytes: X twice.  Arithmetic: the activity pass is D^2
    complex multiply-adds a frame and bin (8 flop each) plus 4 D for |y|^2; the update's D covariances are D^2 real sums each,
    a term of 3 flop and a fused multiply-add by phi."""
    frames = B * F * T
    return 2 * itemsize * D * frames / COPY_BYTES_PER_S, frames * (8 * D * D + 4 * D + 5 * D ** 3) / FP64_FLOP_PER_S


def step(name):
    import numpy as np
    import torch
    import iva_ref as R
    from acoustic_locating_vq_vae import separation as SEP
    B, D, cname = name.split("-")
    B, D, cdtype = int(B), int(D), getattr(torch, cname)
    X = FB.mixture(B, D, D, cdtype)
    iteration, call, outside = FB.iteration_ms(lambda n: SEP.auxiva(X, n))
    masks = FB.best_seconds(lambda: SEP.masks(X), 10)
    out = SEP.auxiva(X, ITER_CALL)
    byte_floor, flop_floor = floors(B, D, X.element_size())
    x1 = X[:1].to(torch.complex128).cpu().numpy()
    t0 = time.perf_counter()
    ref = R.auxiva(x1, 2)
    cpu = (time.perf_counter() - t0) / 2
    two = SEP.auxiva(X[:1].to(torch.complex128), 2)
    print(json.dumps({"step": name, "B": B, "D": D, "F": F, "T": T, "dtype": cname, "iteration_ms": iteration,
                      "byte_floor_ms": byte_floor * 1e3, "fp64_floor_ms": flop_floor * 1e3, "call_ms_20_iterations": call,
                      "outside_the_iterations_ms": outside, "masks_ms": masks * 1e3,
                      "bins_with_status": int((out.status != 0).sum()),
                      "restatement_cpu_ms_per_iteration_at_B_1": cpu * 1e3,
                      "max_rel_diff_of_w_to_restatement_at_B_1": float(np.abs(two.w.cpu().numpy() - ref.W).max() / np.abs(ref.W).max())}),
          flush=True)


def main():
    FB.main(__file__, STEPS, step)


if __name__ == "__main__":
    main()
