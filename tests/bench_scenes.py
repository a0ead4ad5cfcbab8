"""Room-per-item synthesis rates: RIRs/s of the per-item kernel (front_end.scene_impulse_responses, alvq_rir_rooms_f64) on B
copies of the dataset scene against the one-room launch (room_impulse_responses, alvq_rir_f64) on the same sources; RIRs/s over
randomised rooms (SceneConfig's defaults: 3-8 m per axis, T60 0.25-0.8 s, 6400 samples); and SceneLoader batches/s (B
five-second crops of a resident pool, scenes drawn per batch, RIR -> FIR -> STFT -> Wiener).
    python tests/bench_scenes.py [batch=64]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from family_bench import wall_seconds  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)
import torch  # noqa: E402

from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae.rir_dataset_generator.scene_loader import SceneLoader  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    cfg = FE.DATASET_CONFIG
    ns = cfg["n_sample"]
    g = torch.Generator(device="cuda").manual_seed(0)
    same = FE.sample_scenes(B, FE.SceneConfig.from_dataset_config(), generator=g)
    t_one = wall_seconds(lambda: FE.room_impulse_responses(same.source, same.receiver, cfg["room_dimensions"],
                                                   reverberation_time=cfg["reverberation_time"], nsample=ns), 10)
    t_same = wall_seconds(lambda: FE.scene_impulse_responses(same.source, same.receiver, same.room, beta=same.beta, nsample=ns), 10)
    rnd = FE.sample_scenes(B, FE.SceneConfig(), generator=g)
    t_rnd = wall_seconds(lambda: FE.scene_impulse_responses(rnd.source, rnd.receiver, rnd.room, beta=rnd.beta, nsample=ns), 10)
    waves = [torch.randn(80000 + 4000 * i, generator=torch.Generator().manual_seed(i)) for i in range(256)]
    loader = SceneLoader(waves, B, FE.SceneConfig(), seed=0)
    t_batch = wall_seconds(lambda: next(loader), 10)
    print(json.dumps({"batch": B, "nsample": ns,
                      "one_room_rirs_per_s": B / t_one, "per_item_dataset_scene_rirs_per_s": B / t_same,
                      "per_item_vs_one_room": t_one / t_same, "random_rooms_rirs_per_s": B / t_rnd,
                      "random_rooms_ms_per_call": t_rnd * 1e3, "scene_loader_batches_per_s": 1.0 / t_batch,
                      "scene_loader_spectrograms_per_s": B / t_batch}))


if __name__ == "__main__":
    main()
