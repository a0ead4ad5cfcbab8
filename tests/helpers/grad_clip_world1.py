"""Child process of tests/test_grad_clip_gpu.py: a ONE-rank "nccl" (= RCCL on ROCm) process group on cuda:0 with the Trainer's
all-reduce forced (the pattern of tests/helpers/rccl_world1.py), clipping and the warm-up / cosine schedule on.  A captured
and an eager trainer take the same 6 steps; prints one JSON line: whether their parameters and moments are bit-identical,
the all_reduce calls per step, and what the clip reported.
    python grad_clip_world1.py <max_grad_norm> [buckets]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "acoustic_locating_vq-vae_amd")
for p in (ROOT, PKG, os.path.join(PKG, "src")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    max_norm = float(sys.argv[1])
    buckets = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    steps = 6
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from acoustic_locating_vq_vae import _ops
    from acoustic_locating_vq_vae.train_step import Trainer, WarmupCosine
    from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE
    _ops.set_compute_dtype("f32")
    calls = {"n": 0}
    real = dist.all_reduce

    def counting(t, *a, **k):
        calls["n"] += 1
        return real(t, *a, **k)

    dist.all_reduce = counting
    cfg = (20, 48, 8, 2, 24, 0.25, 64)
    raws = [torch.randn(4, 20, 40, generator=torch.Generator().manual_seed(10 + i)).cuda() for i in range(steps + 1)]

    def run(graph):
        torch.manual_seed(0)
        model = ConvolutionalVQVAE(*cfg, use_jitter=False).cuda().train()
        with torch.no_grad():
            model._vq._embedding.weight.normal_(0, 0.7)
        tr = Trainer(model, "speech", force_collective=True, grad_buckets=buckets, range_check_every=0, max_grad_norm=max_norm,
                     lr_schedule=WarmupCosine(3, 8))
        if graph:
            tr.capture(raws[0], warmup=1)          # one real step on raws[0], then the capture
        else:
            tr.step(raws[0])
        calls["n"] = 0
        norms = []
        for r in raws[1:]:
            tr.step(r)
            norms.append(tr.grad_norm())
        torch.cuda.synchronize()
        return tr, calls["n"] / steps, norms

    ta, na, norms_a = run(False)
    tb, nb, norms_b = run(True)
    out = {"backend": dist.get_backend(), "world": dist.get_world_size(), "captured": tb._graph is not None,
           "allreduce_calls_per_step": [na, nb], "params_bit_identical": bool(torch.equal(ta.buffers.flat, tb.buffers.flat)),
           "moments_bit_identical": bool(torch.equal(ta.opt.exp_avg, tb.opt.exp_avg) and torch.equal(ta.opt.exp_avg_sq, tb.opt.exp_avg_sq)),
           "scalars_bit_identical": bool(torch.equal(ta.opt.scalars, tb.opt.scalars)),
           "finite": bool(torch.isfinite(ta.buffers.flat).all()), "norms_equal": norms_a == norms_b,
           "clipped_steps": [ta.clipped_steps(), tb.clipped_steps()], "coefs": [c for _, c in norms_a],
           "applied_steps": float(ta.opt.scalars[3])}
    print("GRAD_CLIP_WORLD1 " + json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
