"""ILRMA on the device (acoustic_locating_vq_vae.separation, csrc/ilrma.hip): the time of one iteration (power, lam, basis,
activations, weights, covariances, solves: the difference of two iteration counts divided by their distance) and of the whole
call with the default 20 iterations, at (B, D, F, T) = (64, 2, 201, 500), the dataset's shape, and (8, 8, 201, 500), with L = 2
and L = 10 bases, complex128, from device events, the best of 5 -- next to the two floors an iteration has: X read twice (power
and covariances) and P written once and read twice (basis and activations) at the 6.3 TB/s a copy reaches, and the
float64 arithmetic of its passes at the vector rate of 78.6 TFLOP/s (datasheet) -- and next to AuxIVA's iteration at the same
shape, measured the way tests/bench_iva.py measures it.  There is no ratio to pass: nothing did this before.
    python tests/bench_ilrma.py
Each measurement runs in a child process of its own under a time limit; a child that fails or runs out of time ends the script,
and nothing more is started on the device.  For the kernels' own times run `python tests/bench_ilrma.py --step 64-2-2` once under
rocprofv3 --kernel-trace --stats."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)

from family_bench import COPY_BYTES_PER_S, FP64_FLOP_PER_S, ITER_CALL, F, T  # noqa: E402

SHAPES = ((64, 2), (8, 8))               # tests/bench_iva.py's, so that the two iterations stand side by side
BASES = (2, 10)
STEPS = tuple("%d-%d-%d" % (B, D, L) for B, D in SHAPES for L in BASES)


def floors(B, D, L, itemsize):
    """(the byte floor, the float64 floor) of one iteration in seconds.  Bytes: X twice, P (8 bytes a source, bin and frame)
    written once and read twice.  Arithmetic a frame and bin: the power pass is D^2 complex multiply-adds (8 flop each) and 3 D
    for |y|^2; the basis and the activation update are each 2 L for R, 4 for 1 / R, P / lam and g, and 4 L for the two sums, a
    source; the weights 2 L + 1 a source; the D covariances 5 D^3."""
    frames = B * F * T
    flop = 8 * D * D + 3 * D + D * (2 * (6 * L + 4) + 2 * L + 1) + 5 * D ** 3
    return (2 * itemsize + 3 * 8) * D * frames / COPY_BYTES_PER_S, frames * flop / FP64_FLOP_PER_S


def step(name):
    import torch
    from acoustic_locating_vq_vae import separation as SEP
    B, D, L = (int(v) for v in name.split("-"))
    X = FB.mixture(B, D, D, torch.complex128)
    b0, a0 = SEP.nmf_init(B, D, F, T, L, generator=torch.Generator(device="cuda").manual_seed(0))
    iteration, call, outside = FB.iteration_ms(lambda n: SEP.ilrma(X, b0, a0, n))
    auxiva_iteration, _, _ = FB.iteration_ms(lambda n: SEP.auxiva(X, n), iter_call=None)
    out = SEP.ilrma(X, b0, a0, ITER_CALL)
    byte_floor, flop_floor = floors(B, D, L, X.element_size())
    print(json.dumps({"step": name, "B": B, "D": D, "L": L, "F": F, "T": T, "dtype": "complex128",
                      "iteration_ms": iteration, "byte_floor_ms": byte_floor * 1e3, "fp64_floor_ms": flop_floor * 1e3,
                      "call_ms_20_iterations": call, "outside_the_iterations_ms": outside,
                      "auxiva_iteration_ms": auxiva_iteration, "bins_with_status": int((out.status != 0).sum())}),
          flush=True)


def main():
    FB.main(__file__, STEPS, step)


if __name__ == "__main__":
    main()
