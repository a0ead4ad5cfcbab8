"""Room impulse responses on the device (csrc/rir.hip) and the dataset generator built on them (front_end.generate_samples,
write_specs_dataset).  Parity with rir_generator itself is unpinned (the package is absent): the kernel is checked against the
float64 restatement of tests/helpers/rir_ref.py, which evaluates every tap directly, and against the closed-form direct path."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import rir_ref as R  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from oracle import front_end_oracle as FO  # noqa: E402

C, FS = 340.0, 16000.0
CFG = FE.DATASET_CONFIG


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def chirp(S, seed):
    t = torch.arange(S, dtype=torch.float64) / 16000.0
    g = torch.Generator().manual_seed(seed)
    x = torch.sin(2 * np.pi * (200.0 + 900.0 * t) * t) * (0.3 + 0.7 * torch.rand(1, generator=g)) + \
        0.05 * torch.randn(S, generator=g, dtype=torch.float64)
    return x.float()


SMALL_ROOMS = [  # (room, source, receiver, beta, nsample)
    ([1.0, 1.3, 0.9], [0.3, 0.4, 0.5], [0.7, 0.9, 0.2], [0.8, 0.7, 0.6, 0.9, 0.5, 0.7], 700),
    ([2.1, 1.6, 1.2], [1.9, 0.3, 0.4], [0.5, 1.1, 0.9], [0.8, -0.7, 0.6, -0.9, 0.5, -0.75], 900),
]


@pytest.mark.parametrize("order", [0, 1, 2, -1])
@pytest.mark.parametrize("hp", [False, True])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("room", range(len(SMALL_ROOMS)))
def test_kernel_matches_restatement_on_small_rooms(order, hp, dim, room):
    L, s, r, beta, ns = SMALL_ROOMS[room]
    got = FE.rir_generate(C, FS, r, s, L, beta=beta, nsample=ns, order=order, dim=dim, hp_filter=hp)
    assert got.shape == (ns, 1) and got.dtype == torch.float64 and got.is_cuda
    want = R.rir(C, FS, r, s, L, beta, ns, order=order, dim=dim, hp_filter=hp)
    assert rel(got[:, 0].cpu(), want) <= 1e-12


def test_several_receivers_give_the_package_layout():
    L, s, _, beta, ns = SMALL_ROOMS[1]
    rs = [[0.5, 1.1, 0.9], [1.0, 0.2, 0.3], [1.7, 1.4, 1.1]]
    got = FE.rir_generate(C, FS, rs, s, L, beta=beta, nsample=ns).cpu()
    assert got.shape == (ns, 3)
    for m, r in enumerate(rs):
        assert rel(got[:, m], R.rir(C, FS, r, s, L, beta, ns)) <= 1e-12


def test_dataset_configuration_matches_restatement():
    theta = torch.from_numpy(np.random.default_rng(5).uniform(-np.pi, np.pi, 8)).cuda()
    src = FE.source_positions(theta, CFG["receiver_position"], CFG["room_dimensions"], CFG["R"], CFG["Z_LOC_SOURCE"])
    got = FE.room_impulse_responses(src, CFG["receiver_position"], CFG["room_dimensions"],
                                    reverberation_time=CFG["reverberation_time"], nsample=CFG["n_sample"]).cpu().numpy()
    assert got.shape == (8, 6400)
    beta = R.sabine_beta(CFG["room_dimensions"], C, CFG["reverberation_time"])
    for b in range(8):
        want = R.rir(C, FS, CFG["receiver_position"], src[b].cpu().numpy(), CFG["room_dimensions"], beta, 6400)
        assert rel(got[b], want) <= 1e-10, b


def test_source_positions_follow_the_dataset_reader():
    from acoustic_locating_vq_vae.rir_dataset_generator.specsdataset import SpecsDataset
    theta = torch.linspace(-np.pi, np.pi, 17, dtype=torch.float64)
    got = FE.source_positions(theta.cuda(), CFG["receiver_position"], CFG["room_dimensions"], CFG["R"], CFG["Z_LOC_SOURCE"])
    ds = SpecsDataset.__new__(SpecsDataset)
    for k, v in CFG.items():
        setattr(ds, k, v)
    for i in range(17):
        want = ds.get_source_coordinates(theta[i:i + 1].numpy())
        np.testing.assert_allclose(got[i].cpu().numpy(), want[0], rtol=0, atol=1e-14)     # device cos / sin: last bit
    with pytest.raises(ValueError, match="coincides"):
        FE.source_positions(theta.cuda(), CFG["receiver_position"], CFG["room_dimensions"], 0.0, 0.0)


def test_zero_reflection_is_the_closed_form_direct_path():
    r, s, ns = [2.5, 1.5, 1.5], [3.1, 2.3, 2.5], 1200
    got = FE.rir_generate(C, FS, r, s, CFG["room_dimensions"], beta=[0.0] * 6, nsample=ns, hp_filter=False)[:, 0].cpu()
    assert rel(got, R.direct_path(C, FS, r, s, ns)) <= 1e-12


def test_bitwise_reproducible_and_independent_of_the_batch():
    g = torch.Generator().manual_seed(11)
    theta = (torch.rand(64, generator=g, dtype=torch.float64) * 2 - 1) * np.pi
    src = FE.source_positions(theta.cuda(), CFG["receiver_position"], CFG["room_dimensions"], CFG["R"], CFG["Z_LOC_SOURCE"])
    kw = dict(reverberation_time=CFG["reverberation_time"], nsample=CFG["n_sample"])
    a = FE.room_impulse_responses(src, CFG["receiver_position"], CFG["room_dimensions"], **kw)
    b = FE.room_impulse_responses(src, CFG["receiver_position"], CFG["room_dimensions"], **kw)
    assert torch.equal(a, b)
    for i in (0, 37, 63):
        alone = FE.room_impulse_responses(src[i:i + 1].contiguous(), CFG["receiver_position"], CFG["room_dimensions"], **kw)
        assert torch.equal(alone[0], a[i]), i


def test_generate_samples_match_the_generator_arithmetic():
    S = 80000
    w = torch.stack([chirp(S, 31), chirp(S, 32)])
    theta = torch.tensor([0.7, -2.4], dtype=torch.float64)
    speech, rir, echoed, fs, th, wiener = FE.generate_samples(w.cuda(), theta=theta)
    assert fs == 16000 and torch.equal(th.cpu(), theta)
    assert speech.shape == rir.shape == echoed.shape == (2, 201, 501) and wiener.shape == (2, 201)
    assert speech.dtype == torch.float32 and rir.dtype == echoed.dtype == wiener.dtype == torch.float64
    beta = R.sabine_beta(CFG["room_dimensions"], C, CFG["reverberation_time"])
    src = FE.source_positions(theta.cuda(), CFG["receiver_position"], CFG["room_dimensions"], CFG["R"], CFG["Z_LOC_SOURCE"])
    for b in range(2):
        h = R.rir(C, FS, CFG["receiver_position"], src[b].cpu().numpy(), CFG["room_dimensions"], beta, CFG["n_sample"])
        # scipy convolves this size by FFT in single precision (see test_front_end_gpu.py): loose end to end, then the
        # arithmetic pinned with the echoed waveform taken out of the comparison
        ws, wr, we, ww = FO.convert_speech_to_specs(w[b:b + 1], h)
        assert rel(speech[b].cpu(), ws) < 5e-5 and rel(echoed[b].cpu(), we) < 1e-6 and rel(wiener[b].cpu(), ww) < 1e-4
        echoed_wave = N.fir_same(w[b:b + 1].cuda(), torch.from_numpy(h).cuda())[0].cpu().numpy()
        ws, wr, we, ww = FO.convert_speech_to_specs(w[b:b + 1], h, waveform_h=echoed_wave)
        assert rel(echoed[b].cpu(), we) < 1e-9 and rel(wiener[b].cpu(), ww) < 1e-4 and rel(rir[b].cpu(), wr) < 1e-3


def test_written_dataset_feeds_the_rir_trainer(tmp_path):
    from acoustic_locating_vq_vae.data_preprocessing import spec_dataset_preprocessing
    from acoustic_locating_vq_vae.rir_dataset_generator.specsdataset import SpecsDataset
    from acoustic_locating_vq_vae.train_step import Trainer
    from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE
    w = torch.stack([chirp(80000, 40 + b) for b in range(3)]).cuda()
    samples = FE.generate_samples(w, generator=torch.Generator(device="cuda").manual_seed(2))
    root = str(tmp_path / "specs")
    paths = FE.write_specs_dataset(root, samples, CFG, start=0)
    assert len(paths) == 3
    ds = SpecsDataset(root)
    assert len(ds) == 3 and ds.n_sample == 6400 and list(ds.room_dimensions) == [4, 5, 3]
    items = [ds[i] for i in range(3)]
    sp, rr, ec, fs, th, wi = items[1]
    assert sp.dtype == torch.float32 and rr.dtype == ec.dtype == wi.dtype == th.dtype == torch.float64
    assert sp.shape == (201, 501) and wi.shape == (201,) and th.shape == (1,) and type(fs) is int
    assert torch.equal(rr, samples[1][1].cpu()) and float(th) == float(samples[4][1])
    assert np.abs(th.numpy()) <= np.pi
    speech, rir, echoed, fss, theta, wiener = spec_dataset_preprocessing(items)
    assert rir.shape == (3, 201, 500) and theta.shape == (3, 1)
    torch.manual_seed(3)
    model = ConvolutionalVQVAE(500, 32, 8, 2, 16, 0.25, 32, use_jitter=False, out_channels=1).cuda().train()
    loss, _, _ = Trainer(model, "rir").step(rir.cuda(), wiener.cuda())
    assert torch.isfinite(loss)


def test_graph_capture_replays_the_same_bits():
    theta = torch.tensor([0.3, -1.1, 2.9], dtype=torch.float64).cuda()
    src = FE.source_positions(theta, CFG["receiver_position"], CFG["room_dimensions"], CFG["R"], CFG["Z_LOC_SOURCE"])
    kw = dict(reverberation_time=CFG["reverberation_time"], nsample=CFG["n_sample"])
    eager = FE.room_impulse_responses(src, CFG["receiver_position"], CFG["room_dimensions"], **kw)
    rcv = torch.tensor(CFG["receiver_position"], dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):          # one stream, two launches in a chain
        out = FE.room_impulse_responses(src, rcv, CFG["room_dimensions"], **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
