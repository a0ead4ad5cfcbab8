"""Child of tests/test_vq_restart_gpu.py::test_two_ranks_restart_the_same_codes -- launched by torch.distributed.run with 2
ranks sharing cuda:0 over gloo.  Trains `steps` steps of an EMA model with dead-code restarts on this rank's shard and writes,
per rank: the quantiser's final state and counters, its state before the last step, the last step's summed statistics and
candidates as the all-reduce left them, and the rows of this rank that it offered as candidates in that step."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "acoustic_locating_vq-vae_amd")
for p in (ROOT, PKG, os.path.join(PKG, "src")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    mode, out, buckets, steps = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from acoustic_locating_vq_vae import _ops
    from acoustic_locating_vq_vae.train_step import Trainer, shard_batch
    from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE
    _ops.set_compute_dtype(mode)
    torch.manual_seed(100 + rank)            # ranks start apart: the Trainer broadcasts rank 0's parameters and EMA state
    model = ConvolutionalVQVAE(40, 128, 16, 2, 64, 0.25, 64, use_jitter=False, decay=0.9, dead_code_threshold=1.0,
                               restart_candidates=7, restart_seed=3).cuda().train()
    vq = model._vq
    tr = Trainer(model, "speech", grad_buckets=buckets)
    seen = {}
    inner = vq.quantize

    def tapped(z):                           # this rank's pre-VQ rows of the step
        seen["rows"] = z.detach().reshape(-1, 16).clone()
        return inner(z)
    vq.quantize = tapped
    before = None
    for s in range(steps):
        full = torch.randn(8, 40, 60, generator=torch.Generator().manual_seed(50 + s)).cuda() * 2.0
        torch.cuda.synchronize()
        before = [t.detach().clone() for t in (vq._ema_cluster_size, vq._ema_w, vq._embedding.weight)]
        tr.step(shard_batch(full, rank, world))
    torch.cuda.synchronize()
    sink = tr._ema_sinks[id(vq)]
    n = len(range(rank, 7, world))
    total, dead = tr.restarted_codes()[0]
    torch.save({"cs": vq._ema_cluster_size.cpu(), "w": vq._ema_w.detach().cpu(), "e": vq._embedding.weight.detach().cpu(),
                "counters": torch.tensor([total, dead]), "cs0": before[0].cpu(), "w0": before[1].cpu(), "e0": before[2].cpu(),
                "counts": sink.counts.cpu().clone(), "sums": sink.sums.cpu().clone(), "cand": sink.cand.cpu().clone(),
                "own": seen["rows"][vq._restart_rows[:n]].cpu(), "positions": vq._restart_rows[:n].cpu(),
                "nrows": torch.tensor(seen["rows"].shape[0])}, "%s.rank%d" % (out, rank))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
