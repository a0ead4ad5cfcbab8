"""The layout of the EMA statistics span inside a Trainer's flat gradient buffer, without a GPU: per quantiser the counts
(padded to 64 floats), the K*D sums (padded) and, with dead-code restarts on, the R*D candidate rows.  The all-reduce, the
optimiser's skip list and the checkpoints' ``numel`` all rest on these offsets, so they are pinned here element by element."""
import pytest
import torch

from acoustic_locating_vq_vae import _native as N
from acoustic_locating_vq_vae import train_step as TS
from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        pytest.fail("the native library was reached")
    monkeypatch.setattr(N, "lib", boom)


def _offset(view, grad):
    """Element offset of a view into the flat gradient buffer."""
    assert view.dtype == torch.float32 and view.is_contiguous()
    assert view.untyped_storage().data_ptr() == grad.untyped_storage().data_ptr()
    return view.storage_offset() - grad.storage_offset()


# (K, D, R, threshold) -> span length, then (offset relative to extra_span[0], shape) of counts, sums, cand
CASES = [
    ((40, 16, 7, 1.0), 816, (0, (40,)), (64, (40, 16)), (704, (7, 16))),
    ((40, 16, 7, 0.0), 704, (0, (40,)), (64, (40, 16)), None),
    ((64, 16, 64, 2.0), 2112, (0, (64,)), (64, (64, 16)), (1088, (64, 16))),
    ((100, 24, 9, 1.0), 2776, (0, (100,)), (128, (100, 24)), (2560, (9, 24))),
]


@pytest.mark.parametrize("cfg,length,counts,sums,cand", CASES, ids=["K%d_D%d_R%d_t%g" % c[0] for c in CASES])
def test_span_layout(no_library, cfg, length, counts, sums, cand):
    K, D, R, t = cfg
    model = ConvolutionalVQVAE(40, 32, D, 2, 16, 0.25, K, use_jitter=False, decay=0.9, dead_code_threshold=t,
                               restart_candidates=R)
    tr = TS.Trainer(model, "speech")
    lo, hi = tr.buffers.extra_span
    assert lo % 64 == 0 and TS._ALIGN == 64
    assert hi - lo == length
    assert hi <= tr.buffers.grad.numel() == tr.buffers.flat.numel()
    assert list(tr._ema_sinks) == [id(model._vq)]
    sink = tr._ema_sinks[id(model._vq)]
    assert sink.rank == 0 and sink.world == 1 and sink.written is False
    for view, want in ((sink.counts, counts), (sink.sums, sums)):
        assert (_offset(view, tr.buffers.grad) - lo, tuple(view.shape)) == want
    if cand is None:
        assert sink.cand is None
    else:
        assert (_offset(sink.cand, tr.buffers.grad) - lo, tuple(sink.cand.shape)) == cand
        assert _offset(sink.cand, tr.buffers.grad) + sink.cand.numel() == hi   # the candidates close the span
