"""Room-acoustic parameters (room_acoustics.room_acoustic_parameters, csrc/room_acoustics.hip): the time of the parameter
launch from device events at the dataset's own size (B = 64, n = 6400) and at B = 4096, n = 12800, float64 responses, next to
the least time one read of the responses could take (B n 8 bytes at the measured HBM rate of 6.3 TB/s) and to the float64
restatement (tests/helpers/room_acoustics_ref.py) on host threads; then measured T30 and EDT next to the nominal Sabine T60 of
64 scenes drawn from the default SceneConfig.
    python tests/bench_room_acoustics.py [cpu_threads=16]
For the kernel time alone run it once under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)
import numpy as np
import torch

import room_acoustics_ref as R
from acoustic_locating_vq_vae import _native as N
from acoustic_locating_vq_vae import front_end as FE
from acoustic_locating_vq_vae import room_acoustics as RA

FS = 16000.0


def responses(B, n, g):
    """Gaussian noise under exponential envelopes of T60 0.25-0.8 s, a 2 ms silence before the direct sound: (B, n) float64."""
    t60 = 0.25 + 0.55 * torch.rand(B, 1, dtype=torch.float64, device="cuda", generator=g)
    t = torch.arange(n, dtype=torch.float64, device="cuda")[None] - 32.0
    h = torch.randn(B, n, dtype=torch.float64, device="cuda", generator=g) * torch.exp(-3.0 * np.log(10.0) * t / (t60 * FS))
    h[:, :32] = 0.0
    h[:, 32] = 8.0
    return h


def launch_seconds(h, reps):
    """Seconds per alvq_room_acoustics_f64 launch on preallocated outputs, from device events around reps launches."""
    B, n = h.shape
    out = torch.empty((B, 7), dtype=torch.float64, device="cuda")
    onset = torch.empty((B,), dtype=torch.int32, device="cuda")
    status = torch.empty((B,), dtype=torch.int32, device="cuda")
    k50, k80, kd = RA.sample_counts(FS)
    fn, stream = N.lib().alvq_room_acoustics_f64, torch.cuda.current_stream().cuda_stream
    args = (h.data_ptr(), out.data_ptr(), onset.data_ptr(), status.data_ptr(), B, n, FS, k50, k80, kd, stream)
    for _ in range(3):
        assert fn(*args) == 0
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(*args)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3 / reps)
    assert int(status.max()) == 0
    return best


def host_rows_per_second(h, threads, rows):
    x = h[:rows].cpu().numpy()
    R.parameters(x[0], FS)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda i: R.parameters(x[i], FS), range(x.shape[0])))
    return x.shape[0] / (time.perf_counter() - t0)


def main():
    threads = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    g = torch.Generator(device="cuda").manual_seed(0)
    for B, n, reps, rows in ((64, 6400, 200, 64), (4096, 12800, 20, 512)):
        h = responses(B, n, g)
        t = launch_seconds(h, reps)
        bound = B * n * 8 / FB.COPY_BYTES_PER_S
        cpu = host_rows_per_second(h, threads, rows)
        print(json.dumps({"B": B, "n": n, "gpu_us_per_launch": t * 1e6, "one_read_bound_us": bound * 1e6,
                          "ratio_to_bound": t / bound, "gpu_rows_per_s": B / t, "read_GB_per_s": B * n * 8 / t / 1e9,
                          "cpu_rows_per_s": cpu, "cpu_threads": threads, "gpu_over_cpu": B / t / cpu}), flush=True)
        del h
    # what the rooms do against what Sabine was asked for
    cfg = FE.SceneConfig()
    scenes = FE.sample_scenes(64, cfg, torch.Generator(device="cuda").manual_seed(0))
    h = FE.scene_impulse_responses(scenes.source, scenes.receiver, scenes.room, reverberation_time=scenes.reverberation_time,
                                   nsample=cfg.n_sample, c=cfg.c, fs=cfg.fs)
    p = RA.room_acoustic_parameters(h, fs=cfg.fs)
    t60, t30, edt = (v.cpu().numpy() for v in (scenes.reverberation_time, p.t30, p.edt))
    room = scenes.room.cpu().numpy()
    print("scene  room (m)            T60 nominal  T30     EDT     T30/T60  EDT/T60  status")
    for i in np.argsort(t60):
        print("%5d  %4.2f x %4.2f x %4.2f  %10.3f  %6.3f  %6.3f  %7.3f  %7.3f  %d"
              % (i, room[i, 0], room[i, 1], room[i, 2], t60[i], t30[i], edt[i], t30[i] / t60[i], edt[i] / t60[i], int(p.status[i])))
    summary = {"scenes": 64, "nsample": cfg.n_sample}
    for name, v in (("t30_over_t60", t30 / t60), ("edt_over_t60", edt / t60)):
        q = np.quantile(v, [0.0, 0.25, 0.5, 0.75, 1.0])
        summary[name] = {"min": q[0], "q25": q[1], "median": q[2], "q75": q[3], "max": q[4], "mean": float(v.mean())}
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
