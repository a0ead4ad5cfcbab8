"""Room impulse responses without a GPU: the float64 restatement (tests/helpers/rir_ref.py) against closed forms, reciprocity
and scipy's lfilter, and the argument errors of front_end's RIR functions, which must raise before anything is launched."""
import os
import sys

import numpy as np
import pytest
import scipy.signal as ss
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import rir_ref as R  # noqa: E402

C, FS = 340.0, 16000.0
ROOM = [4.0, 5.0, 3.0]


def test_direct_path_matches_closed_form():
    r, s = [2.5, 1.5, 1.5], [3.1, 2.3, 2.5]
    got = R.rir(C, FS, r, s, ROOM, [0.0] * 6, 1000, hp_filter=False)
    want = R.direct_path(C, FS, r, s, 1000)
    assert np.count_nonzero(want) == R.window_length(FS)
    assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()


def test_order_one_has_seven_pulses_at_the_image_distances():
    r, s = np.array([1.2, 1.7, 1.1]), np.array([2.9, 3.1, 1.9])
    L = np.array(ROOM)
    d, gain = R.images(C, FS, r, s, ROOM, [0.9] * 6, 4000, order=1)
    assert d.size == 7
    want = [np.linalg.norm(s - r)]
    for a in range(3):
        for wall in (0.0, L[a]):                   # mirror the source in each of the six walls
            img = s.copy()
            img[a] = 2 * wall - s[a]
            want.append(np.linalg.norm(img - r))
    np.testing.assert_allclose(np.sort(d * C / FS), np.sort(want), rtol=1e-14)
    np.testing.assert_allclose(np.sort(gain)[::-1][0], 1 / (4 * np.pi * want[0]), rtol=1e-14)


def test_source_receiver_reciprocity():
    r, s = [1.2, 1.7, 1.1], [2.9, 3.1, 1.9]
    beta = [0.8, 0.7, 0.6, 0.9, 0.5, 0.75]
    a = R.rir(C, FS, r, s, ROOM, beta, 2000, hp_filter=False)
    b = R.rir(C, FS, s, r, ROOM, beta, 2000, hp_filter=False)
    assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()


def test_highpass_recurrence_matches_lfilter():
    x = np.random.default_rng(0).standard_normal(3000)
    b, a = R.highpass_coefficients(FS)
    assert np.abs(R.highpass(x, FS) - ss.lfilter(b, a, x)).max() < 1e-12


def test_sabine_beta():
    beta = R.sabine_beta(ROOM, C, 0.4)
    V, S = 60.0, 2 * (12 + 15 + 20)
    assert np.allclose(beta, np.sqrt(1 - 24 * V * np.log(10) / (C * S * 0.4)))
    with pytest.raises(ValueError):
        R.sabine_beta(ROOM, C, 0.01)


@pytest.fixture(scope="module")
def FE():
    for p in (ROOT, os.path.join(ROOT, "acoustic_locating_vq-vae_amd"), os.path.join(ROOT, "acoustic_locating_vq-vae_amd", "src")):
        sys.path.insert(0, p)
    from acoustic_locating_vq_vae import front_end
    return front_end


@pytest.fixture
def no_launch(FE, monkeypatch):
    """Any call that gets as far as the library fails the test."""
    from acoustic_locating_vq_vae import _native

    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(_native, "rir", boom)
    monkeypatch.setattr(_native, "lib", boom)


def test_rir_generate_argument_errors(FE, no_launch):
    ok = dict(c=C, fs=FS, r=[2.5, 1.5, 1.5], s=[3.0, 2.0, 2.5], L=ROOM)
    with pytest.raises(ValueError, match="alpha"):
        FE.rir_generate(**ok, reverberation_time=0.01)                       # alpha > 1
    with pytest.raises(ValueError, match="exactly one"):
        FE.rir_generate(**ok, beta=[0.5] * 6, reverberation_time=0.4)
    with pytest.raises(ValueError, match="exactly one"):
        FE.rir_generate(**ok)
    with pytest.raises(ValueError, match="nsample"):
        FE.rir_generate(**ok, beta=[0.5] * 6)
    with pytest.raises(ValueError, match="beta"):
        FE.rir_generate(**ok, beta=[0.5] * 5, nsample=100)
    with pytest.raises(ValueError, match="beta"):
        FE.rir_generate(**ok, beta=[1.5] * 6, nsample=100)
    with pytest.raises(ValueError, match="omnidirectional"):
        FE.rir_generate(**ok, reverberation_time=0.4, mtype="cardioid")
    with pytest.raises(ValueError, match="orientation"):
        FE.rir_generate(**ok, reverberation_time=0.4, orientation=[0.0, 0.0])
    with pytest.raises(ValueError, match="shape"):
        FE.rir_generate(**dict(ok, r=[1.0, 2.0]), reverberation_time=0.4)
    with pytest.raises(ValueError, match="room"):
        FE.rir_generate(**dict(ok, L=[4.0, 5.0]), reverberation_time=0.4)
    with pytest.raises(ValueError, match="coincides"):
        FE.rir_generate(**dict(ok, s=[2.5, 1.5, 1.5]), reverberation_time=0.4)
    with pytest.raises(ValueError, match="dim"):
        FE.rir_generate(**ok, reverberation_time=0.4, dim=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FE.rir_generate(**ok, reverberation_time=0.4, device="cpu")


def test_batched_entry_points_reject_bad_input(FE, no_launch):
    src = torch.tensor([[3.0, 2.0, 2.5]], dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FE.room_impulse_responses(src, [2.5, 1.5, 1.5], ROOM, reverberation_time=0.4)
    with pytest.raises(ValueError, match="float64"):
        FE.room_impulse_responses(src.float(), [2.5, 1.5, 1.5], ROOM, reverberation_time=0.4)
    with pytest.raises(ValueError, match="float64"):
        FE.room_impulse_responses(src[:, :2], [2.5, 1.5, 1.5], ROOM, reverberation_time=0.4)
    with pytest.raises(ValueError, match="exactly one"):
        FE.room_impulse_responses(src, [2.5, 1.5, 1.5], ROOM)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FE.source_positions(torch.zeros(3, dtype=torch.float64), [2.5, 1.5, 1.5], ROOM, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FE.generate_samples(torch.zeros(2, 8000))
    with pytest.raises(ValueError, match="float32"):
        FE.generate_samples(torch.zeros(2, 8000, dtype=torch.float64))


def test_dataset_config_matches_the_dataset_format(FE):
    from acoustic_locating_vq_vae.rir_dataset_generator.specsdataset import CONFIG_KEYS
    assert tuple(FE.DATASET_CONFIG) == CONFIG_KEYS
    cfg = FE.DATASET_CONFIG
    assert cfg["n_sample"] == int(cfg["reverberation_time"] * cfg["fs"])
