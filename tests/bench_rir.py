"""Room impulse responses/s (front_end.room_impulse_responses, csrc/rir.hip) at the dataset generator's configuration (room
4 x 5 x 3 m, T60 0.4 s, 16 kHz, 6400 samples, c = 340 m/s, 100 Hz high-pass), B = 64; generate_samples utterances/s for B
five-second utterances; and the float64 restatement (tests/helpers/rir_ref.py) on the host, one response per thread.
    python tests/bench_rir.py [batch=64] [cpu_threads=16]
For the per-kernel split run it once under rocprofv3 --kernel-trace --stats."""
import json
import math
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from family_bench import wall_seconds  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)
import numpy as np
import torch

import rir_ref as R
from acoustic_locating_vq_vae import front_end as FE


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    threads = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    cfg = FE.DATASET_CONFIG
    rcv, room, T60, ns = cfg["receiver_position"], cfg["room_dimensions"], cfg["reverberation_time"], cfg["n_sample"]
    g = torch.Generator(device="cuda").manual_seed(0)
    theta = torch.rand(B, dtype=torch.float64, device="cuda", generator=g) * (2 * math.pi) - math.pi
    src = FE.source_positions(theta, rcv, room, cfg["R"], cfg["Z_LOC_SOURCE"])
    rcv_d = torch.tensor(rcv, dtype=torch.float64, device="cuda")
    t_rir = wall_seconds(lambda: FE.room_impulse_responses(src, rcv_d, room, reverberation_time=T60, nsample=ns), 10)
    # the high-pass share: the same call without it
    t_nohp = wall_seconds(lambda: FE.room_impulse_responses(src, rcv_d, room, reverberation_time=T60, nsample=ns, hp_filter=False), 10)
    wave = torch.randn(B, 80000, device="cuda", generator=g)
    t_gen = wall_seconds(lambda: FE.generate_samples(wave, theta=theta), 5)
    # images that reach the response and their taps (counted from the restatement, one item)
    beta = R.sabine_beta(room, FE.SOUND_SPEED, T60)
    src_h = src.cpu().numpy()
    d, _ = R.images(FE.SOUND_SPEED, float(cfg["fs"]), rcv, src_h[0], room, beta, ns)
    n_cpu = min(B, threads)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda i: R.rir(FE.SOUND_SPEED, float(cfg["fs"]), rcv, src_h[i], room, beta, ns), range(n_cpu)))
    cpu = n_cpu / (time.perf_counter() - t0)
    print(json.dumps({"batch": B, "nsample": ns, "gpu_rirs_per_s": B / t_rir, "gpu_ms_per_call": t_rir * 1e3,
                      "highpass_ms": (t_rir - t_nohp) * 1e3, "images_per_rir": int(d.size),
                      "gtaps_per_s": B * d.size * R.window_length(cfg["fs"]) / t_rir / 1e9,
                      "generate_utterances_per_s": B / t_gen, "generate_ms_per_call": t_gen * 1e3,
                      "cpu_rirs_per_s": cpu, "cpu_threads": threads, "ratio": B / t_rir / cpu}))


if __name__ == "__main__":
    main()
