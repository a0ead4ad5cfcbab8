"""Codebook initialisation by k-means on the device: ConvolutionalVQVAE.init_codebook on the speech model (golden g3_speech_b16
input, 8 000 latent rows, K = 1024) lifts the first forward's perplexity from the uniform init's to >= 256 and the quantiser
then picks the k-means assignment; the RIR model and the encoder_average_pooling path; Trainer.init_codebook zeroes the
codebook's Adam moments and the next eager step and the next replay of a graph captured BEFORE the init both quantise against
the new codebook."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vqvae_oracle as O  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import _ops  # noqa: E402
from acoustic_locating_vq_vae.kmeans import KMeans  # noqa: E402
from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE  # noqa: E402

SPEECH = (201, 1024, 128, 3, 1024, 0.25, 1024)
RIR = (500, 1024, 64, 2, 64, 0.25, 1024)


def speech_model(seed=0, **kw):
    torch.manual_seed(seed)
    return ConvolutionalVQVAE(*SPEECH, **kw).cuda()


def speech_input(B=16):
    """The g3_speech_b16 golden's input (tests/g3_cases.py): hashed uniforms, |.|, standardised."""
    shape = (B, 201, 500)
    return O.speech_preprocess(torch.from_numpy(O.hashed_uniform(int(np.prod(shape)), 21, 2.0).reshape(shape))).cuda()


def rows_of(model, x):
    with torch.no_grad():
        z = model._latent(x)
        if model.encoder_average_pooling:
            z = _ops.MeanPoolFn.apply(z)
        return _ops.dense(z).view(-1, model.get_embedding_dim())


def test_speech_init_lifts_perplexity_and_quantiser_follows_kmeans():
    m = speech_model().train()
    x = speech_input(16)
    with torch.no_grad():
        _, _, perp0, idx0 = m.get_latent_indices(x)
    assert idx0.numel() == 8000
    w = m._vq._embedding.weight
    ptr = w.data_ptr()
    km = m.init_codebook(x, random_state=0)
    assert isinstance(km, KMeans) and w.data_ptr() == ptr
    assert torch.equal(w.detach(), km.cluster_centers_)
    np.random.seed(1)
    with torch.no_grad():
        _, _, perp1 = m(x)
        _, _, _, idx1 = m.get_latent_indices(x)
    assert float(perp1) >= 256 and float(perp1) > 1.5 * float(perp0), (float(perp0), float(perp1))
    rows = rows_of(m, x)
    assert torch.equal(idx1, km.predict(rows))
    # labels_ come from the centred rows: they agree with the quantiser's choice except at fp32 near-ties
    assert float((idx1 == km.labels_).float().mean()) >= 0.999
    assert m._vq._train_vq


def test_rir_model_and_iterable_of_batches():
    torch.manual_seed(1)
    m = ConvolutionalVQVAE(*RIR, use_jitter=False, out_channels=1).cuda().train()
    raw = torch.randn(8, 201, 500, generator=torch.Generator().manual_seed(2)).cuda()
    x = O.standardise(raw).permute(0, 2, 1)
    km = m.init_codebook([x[:4], x[4:]], random_state=3, max_iter=50)
    rows = torch.cat([rows_of(m, x[:4]), rows_of(m, x[4:])])
    assert rows.shape == (8 * 201, 64) and km.labels_.numel() == rows.shape[0]
    ref = KMeans(n_clusters=1024, random_state=3, max_iter=50).fit(rows)
    assert torch.equal(ref.cluster_centers_, m._vq._embedding.weight.detach())


def test_average_pooling_path():
    torch.manual_seed(4)
    m = ConvolutionalVQVAE(20, 48, 8, 2, 24, 0.25, 16, encoder_average_pooling=True).cuda()
    x = torch.randn(64, 20, 40, generator=torch.Generator().manual_seed(5)).cuda()
    km = m.init_codebook(x, random_state=6)
    rows = rows_of(m, x)
    assert rows.shape == (64, 8)
    ref = KMeans(n_clusters=16, random_state=6).fit(rows)
    assert torch.equal(ref.cluster_centers_, m._vq._embedding.weight.detach())
    assert torch.equal(ref.labels_, km.labels_)


def expected_perplexity(tr, raw):
    """The quantiser's perplexity on the trainer's preprocessed batch with the CURRENT codebook, and the indices, checked
    against an argmin over that codebook."""
    x = tr.preprocess(raw)[0]
    with torch.no_grad():
        _, _, perp, idx = tr.model.get_latent_indices(x)
    w = tr.model._vq._embedding.weight.detach()
    assert torch.equal(idx, N.vq_argmin(rows_of(tr.model, x), w))
    return float(perp)


def codebook_moments(tr):
    w = tr.model._vq._embedding.weight
    i = [id(p) for p in tr.buffers.params].index(id(w))
    off = tr.buffers.offsets[i]
    return tr.opt.exp_avg[off:off + w.numel()], tr.opt.exp_avg_sq[off:off + w.numel()]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_trainer_init_codebook_next_step_uses_the_new_codebook(graph):
    from acoustic_locating_vq_vae.train_step import Trainer
    m = speech_model(seed=7).train()
    tr = Trainer(m, "speech", range_check_every=0)
    raw = torch.randn(4, 201, 500, generator=torch.Generator().manual_seed(8)).cuda()
    np.random.seed(3)
    if graph:
        tr.capture(raw, warmup=2)
    else:
        for _ in range(2):
            tr.step(raw)
    tr.step(raw)
    torch.cuda.synchronize()
    m1, m2 = codebook_moments(tr)
    assert float(m2.abs().max()) > 0
    old_perp = expected_perplexity(tr, raw)
    km = tr.init_codebook(raw, random_state=1)
    assert torch.equal(m._vq._embedding.weight.detach(), km.cluster_centers_)
    m1, m2 = codebook_moments(tr)
    assert float(m1.abs().max()) == 0.0 and float(m2.abs().max()) == 0.0
    want = expected_perplexity(tr, raw)
    assert want > 4 * old_perp
    out = tr.step(raw)                              # graph: a replay of the graph captured before the init
    torch.cuda.synchronize()
    assert abs(float(out[2]) - want) <= 1e-4 * want, (float(out[2]), want, old_perp)
