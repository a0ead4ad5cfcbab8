"""VectorQuantizerEMA without a GPU: the float64 restatement on a hand-worked case, the constructor contract
(ConvolutionalVQVAE(decay=...)), draws, keys, flags, argument errors and pickling, and the C ABI's argument checks."""
import os
import pickle
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import vq_ema_ref as R  # noqa: E402
from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE  # noqa: E402
from acoustic_locating_vq_vae.vq_vae.vector_quantizer import VectorQuantizer, VectorQuantizerEMA  # noqa: E402

CFG = (20, 48, 8, 2, 24, 0.25, 64)


def test_restatement_hand_worked():
    """K = 3, D = 2, four rows, decay 1/2, eps 1/2, from cs = 0, W = 0; worked out in fractions."""
    rows = np.array([[1, 0], [3, 2], [0, 4], [2, 2]], dtype=np.float64)
    cs, W = np.zeros(3), np.zeros((3, 2))
    c, s = R.stats(rows, [0, 0, 2, 2], 3)
    assert c.tolist() == [2, 0, 2] and s.tolist() == [[4, 2], [0, 0], [2, 6]]
    cs, W, E = R.step(cs, W, rows, [0, 0, 2, 2], 0.5, 0.5)
    np.testing.assert_allclose(cs, [6 / 7, 2 / 7, 6 / 7], rtol=1e-15)
    np.testing.assert_allclose(W, [[2, 1], [0, 0], [1, 3]], rtol=1e-15)
    np.testing.assert_allclose(E, [[7 / 3, 7 / 6], [0, 0], [7 / 6, 7 / 2]], rtol=1e-15)
    cs, W, E = R.step(cs, W, rows, [0, 2, 2, 1], 0.5, 0.5)
    want_cs = [Fr(20, 21), Fr(16, 21), Fr(9, 7)]
    np.testing.assert_allclose(cs, [float(v) for v in want_cs], rtol=1e-15)
    np.testing.assert_allclose(W, [[1.5, 0.5], [1, 1], [2, 4.5]], rtol=1e-15)
    np.testing.assert_allclose(E, [[63 / 40, 21 / 40], [21 / 16, 21 / 16], [14 / 9, 7 / 2]], rtol=1e-15)
    loss, perp, q = R.forward(rows, E, [0, 2, 2, 1], 0.25)
    assert q.tolist() == [E[0].tolist(), E[2].tolist(), E[2].tolist(), E[1].tolist()]
    np.testing.assert_allclose(loss, 0.25 * np.mean((q - rows) ** 2), rtol=1e-15)
    np.testing.assert_allclose(perp, np.exp(-(2 * 0.25 * np.log(0.25 + 1e-10) + 0.5 * np.log(0.5 + 1e-10))), rtol=1e-12)
    g = np.ones((4, 2))
    np.testing.assert_allclose(R.grad_rows(rows, E, [0, 2, 2, 1], 0.25, g), 1 - 0.5 / 8 * (q - rows), rtol=1e-15)


def test_decay_zero_is_todays_quantiser_bitwise():
    torch.manual_seed(7)
    a = ConvolutionalVQVAE(*CFG)
    after_a = torch.rand(4)
    torch.manual_seed(7)
    b = ConvolutionalVQVAE(*CFG, decay=0.0, epsilon=1e-5)
    assert torch.equal(after_a, torch.rand(4))                               # the same number of draws
    assert type(b._vq) is VectorQuantizer
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert sum(p.numel() for p in a.parameters()) == sum(p.numel() for p in b.parameters())


def test_ema_quantiser_contract():
    torch.manual_seed(3)
    m = ConvolutionalVQVAE(*CFG, decay=0.99)
    vq = m._vq
    assert isinstance(vq, VectorQuantizerEMA)
    keys = [k for k in m.state_dict() if k.startswith("_vq.")]
    assert sorted(keys) == ["_vq._ema_cluster_size", "_vq._ema_w", "_vq._embedding.weight"]
    assert not vq._embedding.weight.requires_grad and not vq._ema_w.requires_grad
    assert isinstance(vq._ema_w, nn.Parameter) and "_ema_cluster_size" in dict(vq.named_buffers())
    assert torch.equal(vq._ema_cluster_size, torch.zeros(64))
    assert (vq._decay, vq._epsilon, vq._commitment_cost, vq._num_embeddings, vq._embedding_dim, vq._train_vq) == \
        (0.99, 1e-5, 0.25, 64, 8, True)
    assert vq.get_embedding_dim() == 8 and m.get_embedding_dim() == 8
    vq.set_train_vq(False)
    assert vq._train_vq is False


def test_ema_draw_order():
    """The Embedding's own init, then weight.normal_(), then _ema_w.normal_()."""
    torch.manual_seed(11)
    vq = VectorQuantizerEMA(32, 6, 0.25, 0.99)
    after = torch.rand(3)
    torch.manual_seed(11)
    emb = nn.Embedding(32, 6)
    emb.weight.data.normal_()
    w = torch.empty(32, 6).normal_()
    assert torch.equal(vq._embedding.weight, emb.weight) and torch.equal(vq._ema_w, w)
    assert torch.equal(after, torch.rand(3))


@pytest.mark.parametrize("decay", [0.0, 1.0, -0.5, 1.5, float("nan")])
def test_ema_rejects_decay_outside_open_interval(decay):
    with pytest.raises(ValueError, match="decay"):
        VectorQuantizerEMA(16, 4, 0.25, decay)
    if decay != 0.0:
        with pytest.raises(ValueError, match="decay"):
            ConvolutionalVQVAE(*CFG, decay=decay)


@pytest.mark.parametrize("eps", [0.0, -1e-5])
def test_ema_rejects_non_positive_epsilon(eps):
    with pytest.raises(ValueError, match="epsilon"):
        VectorQuantizerEMA(16, 4, 0.25, 0.99, epsilon=eps)


def test_ema_model_pickles():
    torch.manual_seed(5)
    m = ConvolutionalVQVAE(*CFG, decay=0.95, epsilon=1e-4)
    m._vq._ema_cluster_size.fill_(2.5)
    r = pickle.loads(pickle.dumps(m))
    assert isinstance(r._vq, VectorQuantizerEMA) and (r._vq._decay, r._vq._epsilon) == (0.95, 1e-4)
    sa, sb = m.state_dict(), r.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not r._vq._embedding.weight.requires_grad and not r._vq._ema_w.requires_grad


def test_ema_abi_argument_checks():
    """The entry points refuse out-of-range arguments before any launch (no GPU here: a launch would fail differently)."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native
    lib = _native.lib()
    assert lib.alvq_vq_ema_stats_workspace_bytes(1000, 1024, 128) > 0
    assert lib.alvq_vq_ema_stats_workspace_bytes(1 << 24, 1024, 128) == -1      # counts travel as fp32
    assert lib.alvq_vq_ema_stats_workspace_bytes(1000, 16385, 128) == -1
    assert lib.alvq_vq_ema_stats_workspace_bytes(1000, 1024, 513) == -1
    fake = 256                                                                 # never dereferenced: the checks come first
    rc = lib.alvq_vq_ema_stats_f32(fake, fake, fake, fake, fake, 1 << 24, 4, 2, None)
    assert rc < 0 and b"2^24" in lib.alvq_last_error()
    for decay, eps in ((1.0, 1e-5), (0.0, 1e-5), (0.99, 0.0)):
        rc = lib.alvq_vq_ema_update_f32(fake, fake, fake, fake, fake, None, 4, 2, decay, eps, None)
        assert rc < 0 and lib.alvq_last_error().startswith(b"alvq_vq_ema_update_f32")
    rc = lib.alvq_vq_ema_update_f32(fake, fake, fake, fake, fake, None, 16385, 2, 0.99, 1e-5, None)
    assert rc < 0 and b"16384" in lib.alvq_last_error()
