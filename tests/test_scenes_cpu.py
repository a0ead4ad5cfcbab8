"""Scenes with a room per item, without a GPU: SceneConfig's feasibility checks at construction, the sampler's properties on a
CPU generator, the argument errors of scene_impulse_responses / generate_samples(scenes=) / SceneLoader (raised before any
launch) and alvq_rir_rooms_f64's host-side checks."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "acoustic_locating_vq-vae_amd"), os.path.join(ROOT, "acoustic_locating_vq-vae_amd", "src")):
    sys.path.insert(0, _p)


@pytest.fixture(scope="module")
def FE():
    from acoustic_locating_vq_vae import front_end
    return front_end


@pytest.fixture
def no_launch(FE, monkeypatch):
    """Any call that gets as far as the library fails the test."""
    from acoustic_locating_vq_vae import _native

    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(_native, "rir_rooms", boom)
    monkeypatch.setattr(_native, "lib", boom)


def test_infeasible_configs_are_rejected_at_construction(FE, no_launch):
    FE.SceneConfig()                                                                  # the defaults are feasible
    with pytest.raises(ValueError, match="no place for the receiver"):
        FE.SceneConfig(room_dimensions=[(2.0, 8.0), (3.0, 8.0), (3.0, 8.0)])            # 2 m < 2 x 1.25 m margin
    with pytest.raises(ValueError, match="no place for the receiver"):
        FE.SceneConfig(room_dimensions=[(3.0, 8.0), (3.0, 8.0), (1.8, 8.0)])            # 1.8 m < Z 1 + 2 x 0.5
    with pytest.raises(ValueError, match="margin > R"):
        FE.SceneConfig(margin=1.0)                                                     # the ring would reach the wall
    with pytest.raises(ValueError, match="Sabine"):
        FE.SceneConfig(reverberation_time=(0.05, 0.8))                                 # 8 m cube: alpha > 1 at 0.05 s
    with pytest.raises(ValueError, match="outside the smallest room"):
        FE.SceneConfig(room_dimensions=[(3.0, 4.0), (4.0, 5.0), (3.0, 3.0)], receiver_position=[2.5, 1.5, 1.5])
    with pytest.raises(ValueError, match="outside the smallest room"):
        FE.SceneConfig(room_dimensions=[4.0, 5.0, 2.4], reverberation_time=0.4, receiver_position=[2.5, 1.5, 1.5])
    with pytest.raises(ValueError, match="4096"):
        FE.SceneConfig(room_dimensions=[(3.0, 3.0)] * 3, reverberation_time=(2.0, 2.0), margin=1.25, n_sample=10_000_000)
    with pytest.raises(ValueError, match="range"):
        FE.SceneConfig(room_dimensions=[(5.0, 4.0), (3.0, 8.0), (3.0, 8.0)])
    with pytest.raises(ValueError, match="range"):
        FE.SceneConfig(reverberation_time=(0.0, 0.8))
    with pytest.raises(ValueError, match="R > 0"):
        FE.SceneConfig(R=0.0)


def test_sabine_bound_is_the_largest_room(FE):
    """The reverberation_time lower bound is checked against the largest room, where alpha is largest."""
    hi = [8.0, 8.0, 8.0]
    t_min = 24.0 * 512.0 * math.log(10.0) / (FE.SOUND_SPEED * 384.0)
    FE.SceneConfig(reverberation_time=(t_min * 1.001, 0.8))
    with pytest.raises(ValueError, match="Sabine"):
        FE.SceneConfig(reverberation_time=(t_min * 0.999, 0.8))
    assert FE._sabine_alpha(hi, FE.SOUND_SPEED, t_min * 1.001) < 1.0


def test_degenerate_config_is_the_dataset_room(FE):
    cfg = FE.SceneConfig.from_dataset_config()
    d = FE.DATASET_CONFIG
    assert cfg.room == tuple((float(v), float(v)) for v in d["room_dimensions"])
    assert cfg.reverberation_time == (d["reverberation_time"],) * 2 and cfg.receiver == tuple(d["receiver_position"])
    assert cfg.signal_config() == {k: d[k] for k in ("fs", "n_sample", "NFFT", "HOP_LENGTH")}


def test_sampler_properties_on_a_cpu_generator(FE):
    cfg = FE.SceneConfig()
    s = FE.sample_scenes(4096, cfg, generator=torch.Generator().manual_seed(3))
    assert all(t.dtype == torch.float64 for t in s)
    assert s.room.shape == s.receiver.shape == s.source.shape == (4096, 3) and s.beta.shape == (4096, 6)
    for a in range(3):
        assert float(s.room[:, a].min()) >= 3.0 and float(s.room[:, a].max()) <= 8.0
    assert float(s.reverberation_time.min()) >= 0.25 and float(s.reverberation_time.max()) <= 0.8
    assert float(s.theta.abs().max()) <= math.pi
    assert bool((s.source > 0).all()) and bool((s.source < s.room).all())                # strictly inside, no clip
    assert bool((s.receiver > 0).all()) and bool((s.receiver < s.room).all())
    assert float((s.source - s.receiver).norm(dim=1).min()) > 1.0 - 1e-12                # never on the receiver
    off = s.source - s.receiver
    assert float((torch.atan2(off[:, 1], off[:, 0]) - s.theta).abs().max()) <= 1e-12
    assert torch.allclose(off[:, 2], torch.ones(4096, dtype=torch.float64), rtol=0, atol=1e-12)
    alpha = FE._sabine_alpha((s.room[:, 0], s.room[:, 1], s.room[:, 2]), FE.SOUND_SPEED, s.reverberation_time)
    assert bool((alpha <= 1).all()) and torch.equal(s.beta, torch.sqrt(1 - alpha)[:, None].expand(-1, 6))
    again = FE.sample_scenes(4096, cfg, generator=torch.Generator().manual_seed(3))
    assert all(torch.equal(a, b) for a, b in zip(s, again))
    other = FE.sample_scenes(4096, cfg, generator=torch.Generator().manual_seed(4))
    assert not torch.equal(s.room, other.room)


def test_sampler_beta_matches_sabine_beta(FE):
    """Tensor and float Sabine share one expression: on a CPU generator the sampler's beta is _sabine_beta's to the last bit
    (bit equality is pinned on the device, in test_scenes_gpu.py; a host's vectorised CPU kernels may round one step apart)."""
    s = FE.sample_scenes(64, FE.SceneConfig(), generator=torch.Generator().manual_seed(8))
    for b in range(64):
        want = FE._sabine_beta([float(v) for v in s.room[b]], FE.SOUND_SPEED, float(s.reverberation_time[b]))
        np.testing.assert_array_max_ulp(s.beta[b].numpy(), np.array(want), maxulp=1)


def test_degenerate_sampler_is_source_positions_arithmetic(FE):
    """On the CPU, a degenerate config's sources are bit for bit source_positions's expression for the same theta."""
    d = FE.DATASET_CONFIG
    s = FE.sample_scenes(256, FE.SceneConfig.from_dataset_config(), generator=torch.Generator().manual_seed(1))
    rcv = torch.tensor(d["receiver_position"], dtype=torch.float64)[None]
    want = FE._ring_sources(s.theta, rcv, torch.tensor(d["room_dimensions"], dtype=torch.float64)[None], d["R"], d["Z_LOC_SOURCE"])
    assert torch.equal(s.source, want)
    assert bool((s.room == torch.tensor([4.0, 5.0, 3.0], dtype=torch.float64)).all())
    assert bool((s.reverberation_time == 0.4).all())
    assert bool((s.source < s.room).all())                                            # the clip never acts here either


def test_scene_impulse_responses_argument_errors(FE, no_launch):
    src = torch.tensor([[3.0, 2.0, 2.5]], dtype=torch.float64)
    room = torch.tensor([[4.0, 5.0, 3.0]], dtype=torch.float64)
    t60 = torch.tensor([0.4], dtype=torch.float64)
    f = FE.scene_impulse_responses
    with pytest.raises(ValueError, match="exactly one"):
        f(src, [2.5, 1.5, 1.5], room, nsample=100)
    with pytest.raises(ValueError, match="exactly one"):
        f(src, [2.5, 1.5, 1.5], room, reverberation_time=t60, beta=torch.zeros(1, 6, dtype=torch.float64), nsample=100)
    with pytest.raises(ValueError, match="nsample"):
        f(src, [2.5, 1.5, 1.5], room, reverberation_time=t60)
    with pytest.raises(ValueError, match="room"):
        f(src, [2.5, 1.5, 1.5], room[:, :2], reverberation_time=t60, nsample=100)
    with pytest.raises(ValueError, match="rooms for"):
        f(src, [2.5, 1.5, 1.5], room.expand(2, 3), reverberation_time=t60, nsample=100)
    with pytest.raises(ValueError, match="beta"):
        f(src, [2.5, 1.5, 1.5], room, beta=torch.zeros(1, 5, dtype=torch.float64), nsample=100)
    with pytest.raises(ValueError, match="reverberation_time"):
        f(src, [2.5, 1.5, 1.5], room, reverberation_time=t60.float(), nsample=100)
    with pytest.raises(ValueError, match="float64"):
        f(src.float(), [2.5, 1.5, 1.5], room, reverberation_time=t60, nsample=100)
    with pytest.raises(ValueError, match="dim"):
        f(src, [2.5, 1.5, 1.5], room, reverberation_time=t60, nsample=100, dim=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(src, [2.5, 1.5, 1.5], room, reverberation_time=t60, nsample=100)
    scenes = FE.sample_scenes(2, FE.SceneConfig(), generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="not both"):
        FE.generate_samples(torch.zeros(2, 8000), theta=scenes.theta, scenes=scenes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FE.generate_samples(torch.zeros(2, 8000), scenes=scenes)


def test_scene_loader_argument_errors(FE, no_launch):
    from acoustic_locating_vq_vae.rir_dataset_generator.scene_loader import SceneLoader
    with pytest.raises(ValueError, match="SceneConfig"):
        SceneLoader([np.zeros(80000, np.float32)], 4, scene_config=FE.DATASET_CONFIG, device="cpu")
    with pytest.raises(ValueError, match="batch_size"):
        SceneLoader([np.zeros(80000, np.float32)], 0, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SceneLoader([np.zeros(80000, np.float32)], 4, device="cpu")


def test_rooms_entry_point_checks_arguments_before_any_launch():
    """alvq_rir_rooms_f64 with a non-null fake pointer: every call below must fail its host checks before touching it."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native
    lib = _native.lib()
    F = 0x1000

    def call(**kw):
        a = dict(src=F, rcv=F, room=F, beta=F, h=F, status=F, B=2, nsample=100, c=340.0, fs=16000.0, order=-1, hp=1)
        a.update(kw)
        rc = lib.alvq_rir_rooms_f64(a["src"], a["rcv"], a["room"], a["beta"], a["h"], a["status"], a["B"], a["nsample"],
                                    a["c"], a["fs"], a["order"], a["hp"], None)
        return rc, lib.alvq_last_error()
    for k in ("src", "rcv", "room", "beta", "h", "status"):
        rc, msg = call(**{k: None})
        assert rc < 0 and msg.startswith(b"alvq_rir_rooms_f64") and b"null" in msg, k
    for kw, word in ((dict(B=0), b"B=0"), (dict(nsample=0), b"nsample=0"), (dict(nsample=(1 << 24) + 1), b"nsample"),
                     (dict(c=0.0), b"c=0"), (dict(fs=-1.0), b"fs=-1"), (dict(fs=float("nan")), b"fs=nan"),
                     (dict(order=-2), b"order=-2"), (dict(hp=2), b"hp_filter=2"), (dict(fs=300000.0), b"window"),
                     (dict(B=1 << 30), b"too many")):
        rc, msg = call(**kw)
        assert rc < 0 and msg.startswith(b"alvq_rir_rooms_f64") and word in msg, (kw, msg)
