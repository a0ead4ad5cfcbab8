"""The separation scores on ONE box (csrc/separation_metrics.hip), HIP events: one ``pairwise_si_sdr`` launch at
(B, K, J, n) = (32, 8, 8, 64000) float32 against ``si_sdr`` called once on the 32 x 64 expanded pairs (the expansion made
beforehand, outside the timed window), the two alternated, the best of 5 windows each; then ``assign`` at K = J = 8
(40320 candidates an item), ``pit_si_sdr`` and ``si_bss_eval`` at the same size.  One JSON line.
    python tools/bench_separation_metrics.py [B] [n]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "helpers"))
from family_bench import best_seconds  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)
import torch  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as SM

K = J = 8
WINDOWS = 5


def best_alternating(fns, reps):
    """Seconds per call of each of fns: windows of reps calls (family_bench's timer, one round, its warm-up done here for all
    candidates first), the candidates taking turns, the best window of each."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    best = [float("inf")] * len(fns)
    for _ in range(WINDOWS):
        for i, fn in enumerate(fns):
            best[i] = min(best[i], best_seconds(fn, reps, rounds=1, warmups=0))
    return best


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64000
    g = torch.Generator(device="cuda").manual_seed(0)
    s = torch.randn((B, K, n), device="cuda", generator=g)
    mix = torch.eye(J, K, device="cuda")[torch.randperm(J, device="cuda", generator=g)] + 0.15 * torch.randn((B, J, K), device="cuda", generator=g)
    e = mix @ s + 0.1 * torch.randn((B, J, n), device="cuda", generator=g)
    s_pairs = s[:, :, None].expand(B, K, J, n).reshape(-1, n).contiguous()
    e_pairs = e[:, None].expand(B, K, J, n).reshape(-1, n).contiguous()
    table = SM.pairwise_si_sdr(s, e)
    pairs = SM.si_sdr(s_pairs, e_pairs).view(B, K, J)
    same = bool(torch.equal(table.view(torch.int64), pairs.view(torch.int64)))
    t_table, t_pairs = best_alternating([lambda: SM.pairwise_si_sdr(s, e), lambda: SM.si_sdr(s_pairs, e_pairs)], 20)
    t_assign, t_pit, t_split = best_alternating([lambda: SM.assign(table), lambda: SM.pit_si_sdr(s, e), lambda: SM.si_bss_eval(s, e)], 20)
    print(json.dumps({"B": B, "K": K, "J": J, "n": n, "dtype": "float32", "table_has_the_bits_of_the_pairs": same,
                      "pairwise_si_sdr_us": t_table * 1e6, "si_sdr_on_expanded_pairs_us": t_pairs * 1e6,
                      "ratio": t_table / t_pairs, "rows_streamed_ratio": (K + K * J) / (2.0 * K * J),
                      "assign_8x8_us": t_assign * 1e6, "pit_si_sdr_us": t_pit * 1e6, "si_bss_eval_us": t_split * 1e6}), flush=True)


if __name__ == "__main__":
    main()
