"""``VectorQuantizer`` -- nearest-codebook lookup with straight-through gradient.

Reference: vq_vae/vector_quantizer.py:8-58.  Rows are the D-float chunks of the (B,D,L) buffer in memory
order (no permute, :32).  The HIP path keeps the codebook as an index problem: argmin -> gather -> loss /
histogram; the dense one-hot ``encodings`` (N,K) the reference builds (:39-40) is only materialised for the
value this method returns, never used for the matmul (:43 is a gather: SURVEY App. A.4).
"""
import torch
import torch.nn as nn

from .. import _native, _ops

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


class VectorQuantizer(nn.Module):
    def __init__(self, num_embeddings, embedding_dim, commitment_cost, flag_flatten=True):
        super().__init__()
        self._embedding_dim = embedding_dim
        self._num_embeddings = num_embeddings
        self._embedding = nn.Embedding(num_embeddings, embedding_dim)
        self._embedding.weight.data.uniform_(-1 / num_embeddings, 1 / num_embeddings)
        self._commitment_cost = commitment_cost
        self._train_vq = True
        self._flag_flatten = flag_flatten   # stored, never read -- as in the reference (:21)

    def get_embedding_dim(self):
        return self._embedding_dim

    def set_train_vq(self, train_vq):
        self._train_vq = train_vq

    def quantize(self, inputs):
        """(loss, quantized_st, perplexity, indices[N] int64) without the dense one-hot."""
        _ops._need_gpu(inputs, "VectorQuantizer")
        if inputs.numel() % self._embedding_dim != 0:
            raise RuntimeError("shape '[-1, %d]' is invalid for input of size %d" % (self._embedding_dim, inputs.numel()))
        return _ops.VQFn.apply(inputs, self._embedding.weight, float(self._commitment_cost), bool(self._train_vq))

    def forward(self, inputs):
        loss, quantized, perplexity, idx = self.quantize(inputs)
        encodings = _native.onehot(idx, self._num_embeddings)
        return loss, quantized, perplexity, encodings


class VectorQuantizerEMA(nn.Module):
    """The codebook as exponential moving averages of the encoder rows assigned to each code (the ``VectorQuantizerEMA`` of
    the widely used PyTorch VQ-VAE notebook): no codebook gradient, loss = commitment_cost * mean((q - x)^2).

    Same attributes, draws and state_dict keys as the notebook (``_embedding.weight``, ``_ema_cluster_size``, ``_ema_w``);
    rows as ``VectorQuantizer`` takes them (``view(-1, D)`` of the contiguous buffer, no permute).  In training mode with
    ``_train_vq`` the forward updates the state after quantising with the codebook it had (c = rows per code, s = their sum):
    cs = decay cs + (1 - decay) c; n = sum cs; cs = (cs + eps) / (n + K eps) n; W = decay W + (1 - decay) s; E = W / cs.
    Deliberate difference: ``_embedding.weight`` and ``_ema_w`` never require a gradient and are updated IN PLACE (the
    notebook rebinds new Parameters every step), so an optimiser, a Trainer's buffers or a captured graph stay valid.
    Under ``train_step.Trainer`` the forward only gathers c and s; the Trainer sums them over the ranks and applies the
    update after the step's all-reduce (skipped with the step when the fp16-range guard skips it)."""

    def __init__(self, num_embeddings, embedding_dim, commitment_cost, decay, epsilon=1e-5):
        if not 0.0 < decay < 1.0:
            raise ValueError("VectorQuantizerEMA: decay must lie in (0, 1), got %r" % (decay,))
        if not epsilon > 0.0:
            raise ValueError("VectorQuantizerEMA: epsilon must be > 0, got %r" % (epsilon,))
        super().__init__()
        self._embedding_dim = embedding_dim
        self._num_embeddings = num_embeddings
        self._embedding = nn.Embedding(num_embeddings, embedding_dim)
        self._embedding.weight.data.normal_()
        self._embedding.weight.requires_grad_(False)
        self._commitment_cost = commitment_cost
        self.register_buffer("_ema_cluster_size", torch.zeros(num_embeddings))
        self._ema_w = nn.Parameter(torch.Tensor(num_embeddings, embedding_dim), requires_grad=False)
        self._ema_w.data.normal_()
        self._decay = decay
        self._epsilon = epsilon
        self._train_vq = True

    def get_embedding_dim(self):
        return self._embedding_dim

    def set_train_vq(self, train_vq):
        self._train_vq = train_vq

    def quantize(self, inputs):
        """(loss, quantized_st, perplexity, indices[N] int64) without the dense one-hot; updates the state when training."""
        _ops._need_gpu(inputs, "VectorQuantizerEMA")
        D, K = self._embedding_dim, self._num_embeddings
        if inputs.numel() % D != 0:
            raise RuntimeError("shape '[-1, %d]' is invalid for input of size %d" % (D, inputs.numel()))
        rows = inputs.numel() // D
        if K > 16384 or D > 512:
            raise ValueError("VectorQuantizerEMA: K=%d, D=%d outside K <= 16384, D <= 512" % (K, D))
        weight = self._embedding.weight
        beta = float(self._commitment_cost)
        if not (self.training and self._train_vq):
            return _ops.VQEMAFn.apply(inputs, weight, beta, None)
        sink = _ops.ema_sink(self)
        world = sink.world if sink is not None else 1
        if rows * world >= 1 << 24:
            raise ValueError("VectorQuantizerEMA: %d rows per step (over %d rank(s)) >= 2^24: the counts travel as fp32"
                             % (rows * world, world))
        if sink is not None:                     # Trainer: statistics only; it applies the update after the all-reduce
            out = _ops.VQEMAFn.apply(inputs, weight, beta, (sink.counts, sink.sums))
            sink.written = True
            return out
        counts = torch.empty((K,), device=inputs.device, dtype=torch.float32)
        sums = torch.empty((K, D), device=inputs.device, dtype=torch.float32)
        # the backward needs the codebook this forward quantised with: quantise with a copy, then update in place
        out = _ops.VQEMAFn.apply(inputs, weight.detach().clone(), beta, (counts, sums))
        _native.vq_ema_update(counts, sums, self._ema_cluster_size, self._ema_w.data, weight.data, self._decay,
                              self._epsilon)
        return out

    def forward(self, inputs):
        loss, quantized, perplexity, idx = self.quantize(inputs)
        encodings = _native.onehot(idx, self._num_embeddings)
        return loss, quantized, perplexity, encodings
