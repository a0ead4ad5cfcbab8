"""A room per item on the device: alvq_rir_rooms_f64 through front_end.scene_impulse_responses (bitwise the one-room launch of
each item, the float64 restatement, batch independence, graph capture), sample_scenes on the device, generate_samples(scenes=)
and the SceneLoader feeding the train loops."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import rir_ref as R  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402

C, FS = 340.0, 16000.0
CFG = FE.DATASET_CONFIG


def mixed_batch(seed, B=16):
    """B items: small rooms (orders 0..2 reach far past nsample there), the dataset room, and 3-8 m rooms; sources and
    receivers drawn inside; per-item beta in [-0.9, 0.95] (item 3 has negative walls) and a T60 each."""
    rng = np.random.default_rng(seed)
    rooms = []
    for b in range(B):
        if b % 3 == 0:
            rooms.append(rng.uniform(0.9, 2.5, 3))
        elif b % 3 == 1:
            rooms.append(np.array([4.0, 5.0, 3.0]))
        else:
            rooms.append(rng.uniform(3.0, 8.0, 3))
    room = np.stack(rooms)
    src = room * rng.uniform(0.1, 0.9, (B, 3))
    rcv = room * rng.uniform(0.1, 0.9, (B, 3))
    beta = rng.uniform(-0.9, 0.95, (B, 6))
    beta[3] = [-0.8, 0.7, -0.6, 0.9, -0.5, 0.75]
    t60 = rng.uniform(0.3, 0.8, B)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    return dev(src), dev(rcv), dev(room), dev(beta), dev(t60)


@pytest.mark.parametrize("order", [0, 1, 2, -1])
@pytest.mark.parametrize("hp", [False, True])
def test_each_row_is_bitwise_the_one_room_launch_explicit_beta(order, hp):
    src, rcv, room, beta, _ = mixed_batch(1)
    ns = 1500
    got = FE.scene_impulse_responses(src, rcv, room, beta=beta, nsample=ns, order=order, hp_filter=hp)
    assert got.shape == (16, ns) and got.dtype == torch.float64
    for b in range(16):
        alone = FE.room_impulse_responses(src[b:b + 1], rcv[b], room[b].tolist(), beta=beta[b].tolist(), nsample=ns,
                                          order=order, hp_filter=hp)
        assert torch.equal(got[b], alone[0]), b


@pytest.mark.parametrize("dim", [2, 3])
def test_each_row_is_bitwise_the_one_room_launch_sabine(dim):
    """From T60, Sabine's beta is computed on the device with the host's expression: the same bits as rir_generate's keyword
    path, at the dataset's 6400 samples."""
    src, rcv, room, _, t60 = mixed_batch(2)
    got = FE.scene_impulse_responses(src, rcv, room, reverberation_time=t60, nsample=CFG["n_sample"], dim=dim)
    for b in range(16):
        alone = FE.room_impulse_responses(src[b:b + 1], rcv[b], room[b].tolist(), reverberation_time=float(t60[b]),
                                          nsample=CFG["n_sample"], dim=dim)
        assert torch.equal(got[b], alone[0]), b


def test_dataset_scene_is_bitwise_room_impulse_responses():
    g = torch.Generator(device="cuda").manual_seed(5)
    scenes = FE.sample_scenes(32, FE.SceneConfig.from_dataset_config(), generator=g)
    got = FE.scene_impulse_responses(scenes.source, scenes.receiver, scenes.room, reverberation_time=scenes.reverberation_time,
                                     nsample=CFG["n_sample"])
    want = FE.room_impulse_responses(scenes.source, CFG["receiver_position"], CFG["room_dimensions"],
                                     reverberation_time=CFG["reverberation_time"], nsample=CFG["n_sample"])
    assert torch.equal(got, want)
    assert torch.equal(scenes.beta[0].cpu(), torch.tensor(FE._sabine_beta(CFG["room_dimensions"], C, 0.4), dtype=torch.float64))


@pytest.mark.parametrize("order", [0, 1, 2, -1])
@pytest.mark.parametrize("hp", [False, True])
def test_small_rooms_match_restatement(order, hp):
    rng = np.random.default_rng(7)
    B, ns = 6, 900
    room = rng.uniform(0.9, 2.2, (B, 3))
    src, rcv = room * rng.uniform(0.1, 0.9, (B, 3)), room * rng.uniform(0.1, 0.9, (B, 3))
    beta = rng.uniform(-0.9, 0.9, (B, 6))
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    got = FE.scene_impulse_responses(dev(src), dev(rcv), dev(room), beta=dev(beta), nsample=ns, order=order,
                                     hp_filter=hp).cpu().numpy()
    for b in range(B):
        want = R.rir(C, FS, rcv[b], src[b], room[b], beta[b], ns, order=order, hp_filter=hp)
        assert np.abs(got[b] - want).max() <= 1e-12 * np.abs(want).max(), b


def test_batch_independence_repeatability_and_graph_capture():
    src, rcv, room, beta, _ = mixed_batch(3)
    kw = dict(beta=beta, nsample=2000)
    a = FE.scene_impulse_responses(src, rcv, room, **kw)
    assert torch.equal(a, FE.scene_impulse_responses(src, rcv, room, **kw))
    perm = torch.randperm(16, generator=torch.Generator().manual_seed(0)).cuda()
    p = FE.scene_impulse_responses(src[perm], rcv[perm], room[perm], beta=beta[perm], nsample=2000)
    assert torch.equal(p, a[perm])
    # item 4 embedded among other rooms (those of another batch)
    o_src, o_rcv, o_room, o_beta, _ = mixed_batch(4, B=9)
    i = 4
    e = FE.scene_impulse_responses(torch.cat((o_src[:5], src[i:i + 1], o_src[5:])), torch.cat((o_rcv[:5], rcv[i:i + 1], o_rcv[5:])),
                                   torch.cat((o_room[:5], room[i:i + 1], o_room[5:])),
                                   beta=torch.cat((o_beta[:5], beta[i:i + 1], o_beta[5:])), nsample=2000)
    assert torch.equal(e[5], a[i])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):             # one stream, two launches in a chain; no check inside the capture
        out = FE.scene_impulse_responses(src, rcv, room, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)


def test_bad_items_raise_outside_capture():
    src, rcv, room, beta, t60 = mixed_batch(6, B=4)
    bad = beta.clone()
    bad[2, 1] = 1.5
    with pytest.raises(ValueError, match=r"items \[2\]"):
        FE.scene_impulse_responses(src, rcv, room, beta=bad, nsample=500)
    tiny = room.clone()
    tiny[1, 0] = 0.01                                   # 6400 / (2 * 0.01 / cTs) images > 4096
    with pytest.raises(ValueError, match=r"items \[1\]"):
        FE.scene_impulse_responses(src, rcv, tiny, beta=beta, nsample=6400)
    with pytest.raises(ValueError, match="alpha"):
        FE.scene_impulse_responses(src, rcv, room, reverberation_time=torch.full_like(t60, 0.01), nsample=500)
    with pytest.raises(ValueError, match="coincides"):
        FE.scene_impulse_responses(rcv, rcv, room, beta=beta, nsample=500)


def test_device_sampler_properties():
    cfg = FE.SceneConfig()
    s = FE.sample_scenes(4096, cfg, generator=torch.Generator(device="cuda").manual_seed(3))
    assert all(t.is_cuda and t.dtype == torch.float64 for t in s)
    for a in range(3):
        assert 3.0 <= float(s.room[:, a].min()) and float(s.room[:, a].max()) <= 8.0
    assert 0.25 <= float(s.reverberation_time.min()) and float(s.reverberation_time.max()) <= 0.8
    assert bool((s.source > 0).all()) and bool((s.source < s.room).all())
    assert bool((s.source != s.receiver).any(dim=1).all())
    off = s.source - s.receiver
    assert float((torch.atan2(off[:, 1], off[:, 0]) - s.theta).abs().max()) <= 1e-12
    again = FE.sample_scenes(4096, cfg, generator=torch.Generator(device="cuda").manual_seed(3))
    assert all(torch.equal(x, y) for x, y in zip(s, again))
    for b in range(0, 4096, 257):                       # the device's Sabine beta is the host's, bit for bit
        want = FE._sabine_beta([float(v) for v in s.room[b]], C, float(s.reverberation_time[b]))
        assert s.beta[b].tolist() == want, b


def chirps(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(S, dtype=torch.float64) / 16000.0
    f0 = 150.0 + 400.0 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    x = torch.sin(2 * np.pi * (f0 + 700.0 * t) * t) + 0.05 * torch.randn(B, S, generator=g, dtype=torch.float64)
    return x.float()


def test_degenerate_scenes_reproduce_generate_samples():
    wave = chirps(3, 80000, 9).cuda()
    scenes = FE.sample_scenes(3, FE.SceneConfig.from_dataset_config(), generator=torch.Generator(device="cuda").manual_seed(2))
    got = FE.generate_samples(wave, scenes=scenes)
    want = FE.generate_samples(wave, theta=scenes.theta)
    assert got[3] == want[3]
    for i in (0, 1, 2, 4, 5):
        assert torch.equal(got[i], want[i]), i


def test_random_scenes_generate_samples_rows_are_their_rooms():
    wave = chirps(4, 80000, 10).cuda()
    scenes = FE.sample_scenes(4, FE.SceneConfig(), generator=torch.Generator(device="cuda").manual_seed(6))
    speech, rir, echoed, fs, theta, wiener = FE.generate_samples(wave, scenes=scenes)
    assert speech.shape == rir.shape == echoed.shape == (4, 201, 501) and wiener.shape == (4, 201) and fs == 16000
    assert theta is scenes.theta
    h = FE.room_impulse_responses(scenes.source[1:2], scenes.receiver[1], scenes.room[1].tolist(),
                                  reverberation_time=float(scenes.reverberation_time[1]), nsample=CFG["n_sample"])
    one = FE.specs_from_waveform(wave[1:2], h)
    assert torch.equal(one[1][0], rir[1]) and torch.equal(one[3][0], wiener[1])


def loader(seed, B=4, **kw):
    from acoustic_locating_vq_vae.rir_dataset_generator.scene_loader import SceneLoader
    waves = [chirps(1, n, 20 + i)[0] for i, n in enumerate((90000, 79839, 120000, 79840, 100000))]
    return SceneLoader(waves, B, FE.SceneConfig(), seed=seed, **kw)


def test_scene_loader_contract_and_determinism():
    a, b = loader(11), loader(11)
    assert a.dropped == 1 and a.num_utterances == 4                      # 79839 samples give 499 frames
    batches_a = [next(iter(a)) for _ in range(3)]
    batches_b = [next(iter(b)) for _ in range(3)]
    speech, rir, echoed, fs, theta, wiener = batches_a[0]
    assert speech.shape == rir.shape == echoed.shape == (4, 201, 500)
    assert speech.dtype == torch.float32 and rir.dtype == echoed.dtype == wiener.dtype == theta.dtype == torch.float64
    assert fs.dtype == torch.int64 and fs.shape == (4,) and bool((fs == 16000).all())
    assert theta.shape == (4, 1) and wiener.shape == (4, 201)
    assert all(t.is_cuda for t in batches_a[0])
    for x, y in zip(batches_a, batches_b):
        assert all(torch.equal(p, q) for p, q in zip(x, y))
    assert not torch.equal(batches_a[0][1], batches_a[1][1])
    s = a.last_scenes
    assert torch.equal(s.theta.reshape(4, 1), batches_a[2][4]) and s.room.shape == (4, 3) and s.beta.shape == (4, 6)
    assert not torch.equal(loader(12).__next__()[1], batches_a[0][1])


def test_scene_loader_batch_step_does_not_sync():
    ld = loader(13)
    next(ld)                                            # first batch: the per-device constants are made once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = [next(ld) for _ in range(3)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(torch.isfinite(b[1]).all() for b in out)


def test_scene_loader_feeds_the_rir_and_location_trainers():
    from acoustic_locating_vq_vae.train_step import LocationTrainer, Trainer
    from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE
    from acoustic_locating_vq_vae.vq_vae.location_model.location_model import LocationModule
    speech, rir, echoed, fs, theta, wiener = next(loader(14))
    torch.manual_seed(3)
    model = ConvolutionalVQVAE(500, 32, 8, 2, 16, 0.25, 32, use_jitter=False, out_channels=1).cuda().train()
    loss, _, _ = Trainer(model, "rir").step(rir, wiener)
    assert torch.isfinite(loss)
    model.eval()
    with torch.no_grad():                              # train_location.py's input: the RIR model's codes of standardise(rir)^T
        x = rir.float().transpose(1, 2)
        x = ((x - x.mean(dim=2, keepdim=True)) / (x.std(dim=2, keepdim=True) + 1e-8)).contiguous()
        idx = model.get_latent_indices(x)[3]
    codes = idx.reshape(rir.shape[0], -1)
    assert int(codes.max()) < 32
    head = LocationModule(codes.shape[1], 32, 1).cuda().train()
    loc_loss = LocationTrainer(head).step(codes, theta)                # (B, 1), as the collate gives it
    assert math.isfinite(float(loc_loss))
