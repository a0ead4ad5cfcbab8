"""Dead-code restarts of the EMA codebook (VectorQuantizerEMA(dead_code_threshold > 0)) on the device.  Reports
  * the us of the two launches -- the candidate gather (alvq_vq_restart_gather_f32) and the restart (alvq_vq_restart_dead_f32)
    with no dead code and with R = 64 codes restarted per call -- from device events, at the speech shape of B = 64
    (N = 32 000 rows, K = 1024, D = 128) and the RIR shape of B = 32 (N = 6 432, D = 64);
  * the graph-replayed speech Trainer step at B = 64 in the default mode with decay = 0.99: restarts on (threshold 1, R = 64)
    against restarts off (threshold 0: the path without the feature), plus a second restarts-off trainer as the control, the
    three alternating in blocks in one process (>= 200 timed steps each after warm-up): the median ms per step over the
    blocks, the per-block ratios on / off (median, min, max) and control / off (the noise of identical work).
    python tests/bench_vq_restart.py [blocks] [steps_per_block]      (default 10 x 25)
Prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)
os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np
import torch

from acoustic_locating_vq_vae import _native as N
from acoustic_locating_vq_vae import _ops
from acoustic_locating_vq_vae.train_step import Trainer
from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE

K, R = 1024, 64
SPEECH = (201, 1024, 128, 3, 1024, 0.25, K)


def us_per_call(fn, reps=200, rounds=1, reset=None):
    return FB.event_ms(fn, reps, rounds, reset) * 1e3


def launch_cost(n, D):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(n, D, device="cuda", generator=g)
    E = torch.randn(K, D, device="cuda", generator=g)
    W = E.clone()
    cs = torch.ones(K, device="cuda")
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:R].cuda()
    cand = torch.zeros(R, D, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")

    def gather():
        N.vq_restart_gather(x, rows, cand, status)

    def dead():
        N.vq_restart_dead(cand, cs, W, E, counters, 0.5)

    out = {"N": n, "K": K, "D": D, "R": R, "gather_us": round(us_per_call(gather), 2)}
    cs.fill_(1.0)                                             # above the threshold: the scan alone
    out["dead_idle_us"] = round(us_per_call(dead), 2)
    # every code dead: K / R calls restart R codes each before the codebook is alive again
    out["dead_restarting_us"] = round(us_per_call(dead, reps=K // R, rounds=20, reset=lambda: cs.zero_()), 2)
    assert int(status.item()) == 0 and counters[0].item() > 0
    return out


def trainer(threshold, raw):
    torch.manual_seed(0)
    model = ConvolutionalVQVAE(*SPEECH, decay=0.99, dead_code_threshold=threshold, restart_candidates=R).cuda().train()
    tr = Trainer(model, "speech", range_check_every=0)
    tr.capture(raw)
    return tr


def main():
    blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    out = {"restart_speech_b64": launch_cost(32000, 128), "restart_rir_b32": launch_cost(6432, 64)}
    _ops.set_compute_dtype("x3mx_hb")
    np.random.seed(0)
    raw = torch.randn(64, 201, 500, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    trs = {"off": trainer(0.0, raw), "on": trainer(1.0, raw), "off_control": trainer(0.0, raw)}
    for tr in trs.values():                                   # warm-up beyond the capture's
        for _ in range(20):
            tr.step(raw)
    torch.cuda.synchronize()
    ms = {k: [] for k in trs}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(blocks):
        for name, tr in trs.items():
            ev[0].record()
            for _ in range(per):
                tr.step(raw)
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]) / per)
    out["speech_b64_step_graph"] = {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4),
                                        "max_ms": round(max(v), 4), "timed_steps": blocks * per} for k, v in ms.items()}
    for key, name in (("restart_step_ratio", "on"), ("control_step_ratio", "off_control")):
        ratio = [b / a for a, b in zip(ms["off"], ms[name])]
        out[key] = {"median": round(float(np.median(ratio)), 4), "min": round(min(ratio), 4), "max": round(max(ratio), 4)}
    total, dead = trs["on"].restarted_codes()[0]
    out["restarted_codes"] = {"total": total, "dead_last_step": dead}      # the timed steps did restart codes
    out["mode"] = "x3mx_hb"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
