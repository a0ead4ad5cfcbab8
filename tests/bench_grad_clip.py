"""Global-norm gradient clipping on the device (FlatAdam(max_grad_norm=...), csrc/grad_clip.hip).  Reports
  * the us of the two launches of alvq_grad_clip_f32 together -- the float64 sum of squares over a fixed grid and the
    one-workgroup scalar update -- and of the same call over a 64-float span (the launches with nothing to read), from device
    events around graph replays of 10 calls each, at the speech model's flat gradient buffer (16 836 937 + padding floats,
    67.3 MB: one buffer, which the last-level cache holds, and five taken in turn, which it does not) and the location head's
    (850 MB), with the GB/s the first figure amounts to;
  * the graph-replayed speech Trainer step at B = 64 in the default mode: clipping on (max_grad_norm = 1.0) against clipping
    off (the path without the feature), plus a second clipping-off trainer as the control, the three alternating in blocks in
    one process (>= 200 timed steps each after warm-up): the median ms per step over the blocks, the per-block ratios on / off
    (median, min, max) and control / off (the noise of identical work).
    python tests/bench_grad_clip.py [blocks] [steps_per_block]      (default 10 x 25)
Prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench  # noqa: E402,F401  (it puts the repository, the package and tests/helpers on the path)
os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np
import torch

from acoustic_locating_vq_vae import _native as N
from acoustic_locating_vq_vae import _ops
from acoustic_locating_vq_vae.train_step import Trainer
from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE

SPEECH = (201, 1024, 128, 3, 1024, 0.25, 1024)
SPEECH_FLOATS = 16836937 + 64 * 18            # the speech model's parameters plus their padding in the flat buffer
LOCATION_FLOATS = 212_500_000                 # the location head's flat buffer: 850 MB


def graph_replay_us(fn, calls, inner=10):
    """us per call of ``fn(i)`` on the device: ``inner`` calls captured into one graph (no host launch cost between them),
    replayed until ``calls`` have run."""
    for i in range(inner):
        fn(i)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(inner):
            fn(i)
    graph.replay()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reps = max(1, calls // inner)
    ev[0].record()
    for _ in range(reps):
        graph.replay()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / (reps * inner)


def launch_cost(n, calls, copies):
    """``copies`` buffers taken in turn: 1 = the buffer stays in the 256 MB last-level cache when it fits (the step's case: the
    all-reduce or the backward has just written it), several whose total exceeds the cache = every read comes from HBM."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    gs = [torch.randn(n, device="cuda", generator=gen) for _ in range(copies)]
    sc = torch.zeros(N.ADAM_SCALARS, device="cuda")
    N.adam_advance(sc, 1e-3, 0.9, 0.999, 1.0)
    ws = N.grad_clip_workspace("cuda")
    both = graph_replay_us(lambda i: N.grad_clip(gs[i % copies], sc, float("inf"), workspace=ws), calls)
    tiny = graph_replay_us(lambda i: N.grad_clip(gs[0][:64], sc, float("inf"), workspace=ws), calls)   # the launches with nothing to read
    return {"floats": n, "MB": round(n * 4e-6, 1), "buffers_in_turn": copies, "two_launches_us": round(both, 2),
            "empty_span_us": round(tiny, 2), "GBps": round(n * 4e-3 / both, 1), "norm": float(sc[5])}


def trainer(max_grad_norm, raw):
    torch.manual_seed(0)
    model = ConvolutionalVQVAE(*SPEECH).cuda().train()
    tr = Trainer(model, "speech", range_check_every=0, max_grad_norm=max_grad_norm)
    tr.capture(raw)
    return tr


def main():
    blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    out = {"clip_speech_cached": launch_cost(SPEECH_FLOATS, 400, 1), "clip_speech_hbm": launch_cost(SPEECH_FLOATS, 400, 5),
           "clip_location": launch_cost(LOCATION_FLOATS, 60, 1)}
    torch.cuda.empty_cache()
    _ops.set_compute_dtype("x3mx_hb")
    np.random.seed(0)
    raw = torch.randn(64, 201, 500, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    trs = {"off": trainer(None, raw), "on": trainer(1.0, raw), "off_control": trainer(None, raw)}
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
    for key, name in (("clip_step_ratio", "on"), ("control_step_ratio", "off_control")):
        ratio = [b / a for a, b in zip(ms["off"], ms[name])]
        out[key] = {"median": round(float(np.median(ratio)), 4), "min": round(min(ratio), 4), "max": round(max(ratio), 4)}
    norm, coef = trs["on"].grad_norm()
    out["last_step"] = {"grad_norm": norm, "coef": coef, "clipped_steps": trs["on"].clipped_steps()}
    out["mode"] = "x3mx_hb"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
