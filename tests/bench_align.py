"""Frequency permutation alignment on the device (acoustic_locating_vq_vae.separation.align_permutations,
csrc/permutation_align.hip): the time of one iteration (centroids, their norms, scores: the difference of two iteration counts
divided by their distance) and of the whole call with the default 10 iterations, at (B, K, F, T) = (64, 2, 201, 500), the
dataset's shape with two classes, and (8, 8, 201, 500), from device events, the best of 5 -- next to the byte floor of an
iteration (two passes over the profile at the 6.3 TB/s a copy reaches) and next to the numpy restatement
(tests/helpers/align_ref.py) on the CPU at a batch of one.  permute_bins, a pure copy, is timed beside it against its own floor
(the array read once and written once).  There is no ratio to pass: nothing did this before.
    python tests/bench_align.py
Each measurement runs in a child process of its own under a time limit; a child that fails or runs out of time ends the script,
and nothing more is started on the device.  For the kernels' own times run `python tests/bench_align.py --step 64-2` once under
rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)

from family_bench import COPY_BYTES_PER_S, F, T  # noqa: E402

SHAPES = ((64, 2), (8, 8))
ITER_CALL = 10                           # align_permutations' default, not the separators' 20 of family_bench
STEPS = tuple("%d-%d" % s for s in SHAPES)


def profile(B, K):
    """(B, K, F, T) float64 on the device, align_ref.case's recipe: per source a block on / off activity shared by all bins, times
    noise and a gain per bin, normalised over k and scrambled by an independent permutation per bin."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    block = T // 16
    on = torch.rand((B, K, 1, (T + block - 1) // block), device="cuda", generator=g) < 0.5
    act = torch.where(on.repeat_interleave(block, dim=3)[..., :T], 1.0, 0.05).double()
    m = act * (0.5 + torch.rand((B, K, F, T), dtype=torch.float64, device="cuda", generator=g))
    m = m * (0.5 + 1.5 * torch.rand((B, K, F, 1), dtype=torch.float64, device="cuda", generator=g))
    m = m / m.sum(dim=1, keepdim=True)
    order = torch.rand((B, K, F, 1), device="cuda", generator=g).argsort(dim=1).expand(B, K, F, T)
    return torch.gather(m, 1, order).contiguous()


def step(name):
    import numpy as np
    import torch
    import align_ref as R
    from acoustic_locating_vq_vae import separation as SEP
    B, K = (int(v) for v in name.split("-"))
    P = profile(B, K)
    iteration, call, outside = FB.iteration_ms(lambda n: SEP.align_permutations(P, n), iter_call=ITER_CALL)
    out = SEP.align_permutations(P, ITER_CALL)
    copy = FB.best_seconds(lambda: SEP.permute_bins(P, out.perm), 3)
    nbytes = P.numel() * 8
    p1 = P[:1].cpu().numpy()
    t0 = time.perf_counter()
    ref = R.align(p1, 2)
    cpu = (time.perf_counter() - t0) / 2
    two = SEP.align_permutations(P[:1].contiguous(), 2)
    print(json.dumps({"step": name, "B": B, "K": K, "F": F, "T": T, "profile_MB": nbytes / 1e6,
                      "iteration_ms": iteration,
                      "byte_floor_ms": 2 * nbytes / COPY_BYTES_PER_S * 1e3, "call_ms_10_iterations": call,
                      "outside_the_iterations_ms": outside,
                      "permute_bins_ms": copy * 1e3, "permute_bins_byte_floor_ms": 2 * nbytes / COPY_BYTES_PER_S * 1e3,
                      "bins_with_status": int((out.status != 0).sum()), "bins_changed_by_the_last_iteration": int(out.changed.sum()),
                      "restatement_cpu_ms_per_iteration_at_B_1": cpu * 1e3,
                      "perm_equals_restatement_at_B_1": bool(np.array_equal(two.perm.cpu().numpy(), ref.perm)),
                      "smallest_margin_of_restatement_at_B_1": float(ref.margin)}),
          flush=True)


def main():
    FB.main(__file__, STEPS, step)


if __name__ == "__main__":
    main()
