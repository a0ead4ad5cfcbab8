"""EMA codebook (VectorQuantizerEMA) on the device.  Reports
  * the us of one EMA update -- per-code statistics (alvq_vq_ema_stats_f32) plus the update (alvq_vq_ema_update_f32) -- from
    device events, at the speech shape of B = 64 (N = 32 000 rows, K = 1024, D = 128) and the RIR shape of B = 32 (N = 6 432,
    D = 64), with the two parts apart;
  * the graph-replayed speech Trainer step at B = 64 in the default mode with decay = 0 (the reference's quantiser) and
    decay = 0.99, the two trainers alternating in blocks in one process (>= 200 timed steps each after warm-up): the median
    ms per step over the blocks, their min / max, and the EMA step's ratio to the other.
    python tests/bench_vq_ema.py [blocks] [steps_per_block]      (default 10 x 25)
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

K = 1024
SPEECH = (201, 1024, 128, 3, 1024, 0.25, K)


def us_per_call(fn):
    return FB.event_ms(fn, 200) * 1e3


def update_cost(n, D):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(n, D, device="cuda", generator=g)
    E = torch.randn(K, D, device="cuda", generator=g)
    idx = N.vq_argmin(x, E)
    counts = torch.empty(K, device="cuda")
    sums = torch.empty(K, D, device="cuda")
    cs = torch.ones(K, device="cuda")
    W = E.clone()

    def stats():
        N.vq_ema_stats(x, idx, counts, sums)

    def update():
        N.vq_ema_update(counts, sums, cs, W, E, 0.99, 1e-5)

    def both():
        stats()
        update()
    return {"N": n, "K": K, "D": D, "us": round(us_per_call(both), 2), "stats_us": round(us_per_call(stats), 2),
            "update_us": round(us_per_call(update), 2)}


def trainer(decay, raw):
    torch.manual_seed(0)
    model = ConvolutionalVQVAE(*SPEECH, decay=decay).cuda().train()
    tr = Trainer(model, "speech", range_check_every=0)
    tr.capture(raw)
    return tr


def main():
    blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    out = {"ema_update_speech_b64": update_cost(32000, 128), "ema_update_rir_b32": update_cost(6432, 64)}
    _ops.set_compute_dtype("x3mx_hb")
    np.random.seed(0)
    raw = torch.randn(64, 201, 500, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    trs = {"decay_0": trainer(0.0, raw), "decay_0.99": trainer(0.99, raw)}
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
    step = {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "timed_steps": blocks * per} for k, v in ms.items()}
    ratio = [b / a for a, b in zip(ms["decay_0"], ms["decay_0.99"])]
    out["speech_b64_step_graph"] = step
    out["ema_step_ratio"] = {"median": round(float(np.median(ratio)), 4), "min": round(min(ratio), 4), "max": round(max(ratio), 4)}
    out["mode"] = "x3mx_hb"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
