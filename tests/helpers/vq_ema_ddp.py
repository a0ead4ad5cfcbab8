"""Child of tests/test_vq_ema_gpu.py::test_two_ranks_share_one_codebook -- launched by torch.distributed.run with 2 ranks
sharing cuda:0 over gloo, or directly as ONE process (no process group) on the whole batch.  Trains `steps` steps of an EMA
model on this rank's shard and writes the quantiser's state (cluster sizes, moving-average sums, codebook) per rank."""
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
    model = ConvolutionalVQVAE(40, 128, 16, 2, 64, 0.25, 64, use_jitter=False, decay=0.9).cuda().train()
    tr = Trainer(model, "speech", grad_buckets=buckets)
    for s in range(steps):
        full = torch.randn(8, 40, 60, generator=torch.Generator().manual_seed(50 + s)).cuda() * 2.0
        tr.step(shard_batch(full, rank, world))
    torch.cuda.synchronize()
    vq = model._vq
    torch.save({"cs": vq._ema_cluster_size.cpu(), "w": vq._ema_w.detach().cpu(), "e": vq._embedding.weight.detach().cpu()},
               "%s.rank%d" % (out, rank))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
