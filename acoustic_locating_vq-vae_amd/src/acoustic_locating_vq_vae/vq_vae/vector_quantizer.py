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
    update after the step's all-reduce (skipped with the step when the fp16-range guard skips it).

    Dead-code restarts (``dead_code_threshold`` > 0; off by default, and nothing below exists or runs when off).  A training
    forward (``self.training and self._train_vq``) does, after the five-step update and on the values it stored:
      1. dead = [k for k in 0..K-1 if cs[k] < threshold], ascending k (fp32 compare, the threshold rounded to fp32);
      2. n = min(len(dead), R), R = ``restart_candidates``; for j < n, with k = dead[j] and c_j the j-th candidate row:
         codebook[k] = c_j, ema_w[k] = fl32(c_j * fl32(threshold)), cs[k] = fl32(threshold); dead codes past the first R
         wait for a later step;
      3. two device counters: restarts so far (+= n) and the dead count of this step (len(dead), before the cap).
    Everything else is untouched, bit for bit (copies and one fp32 product).  The candidates are R of this step's pre-VQ rows
    (``inputs.view(-1, D)``, the rows the statistics are made from) at distinct, uniformly drawn positions.  The positions
    come from a private ``torch.Generator`` seeded with ``restart_seed`` (plus the rank under a data-parallel Trainer), never
    the global one, drawn on the host into a static device buffer; those of the last forward stay readable as
    ``_restart_rows`` (int64, device).  A forward that runs inside a stream capture draws nothing: the owner of the graph
    (``train_step.Trainer``) refreshes the buffer before every replay, as it refreshes the jitter columns.  Fewer rows than
    candidates is a ValueError.  No restart in ``eval()``, with ``set_train_vq(False)``, or on a step the fp16-range guard
    skips.  Because ``_ema_cluster_size`` starts at zero, every code that won no row of the first batch is below any sensible
    threshold after the first update: the first steps restart R codes each until the codebook sits on data.  That is
    intended -- a data-dependent initialisation at R codes a step.  A restarted code that attracts fewer than ``threshold``
    rows (in the moving average) falls below the threshold again and is restarted again.  Under a Trainer rank r of W
    supplies the slots s % W == r from its own rows (draw number s // W of its generator); the step's all-reduce hands every
    rank the same R candidates and the Trainer restarts after its EMA update.  The counters, positions and candidates are
    non-persistent buffers: the state_dict keys are the three above with restarts on or off."""

    def __init__(self, num_embeddings, embedding_dim, commitment_cost, decay, epsilon=1e-5, dead_code_threshold=0.0,
                 restart_candidates=64, restart_seed=0):
        if not 0.0 < decay < 1.0:
            raise ValueError("VectorQuantizerEMA: decay must lie in (0, 1), got %r" % (decay,))
        if not epsilon > 0.0:
            raise ValueError("VectorQuantizerEMA: epsilon must be > 0, got %r" % (epsilon,))
        if not dead_code_threshold >= 0.0:
            raise ValueError("VectorQuantizerEMA: dead_code_threshold must be >= 0, got %r" % (dead_code_threshold,))
        if dead_code_threshold > 0.0 and not 1 <= int(restart_candidates) <= num_embeddings:
            raise ValueError("VectorQuantizerEMA: restart_candidates must lie in [1, num_embeddings = %d], got %r"
                             % (num_embeddings, restart_candidates))
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
        self._dead_code_threshold = float(dead_code_threshold)
        if self._dead_code_threshold > 0.0:                   # the restart state: nothing of it exists when the feature is off
            R = self._restart_candidates = int(restart_candidates)
            self._restart_seed = int(restart_seed)
            self._restart_gen = torch.Generator().manual_seed(self._restart_seed)
            self._restart_nrows = 0                           # rows of the last training forward (a replay draws for them)
            self.register_buffer("_restart_rows", torch.zeros(R, dtype=torch.int64), persistent=False)
            self.register_buffer("_restart_cand", torch.zeros(R, embedding_dim), persistent=False)
            self.register_buffer("_restart_counters", torch.zeros(2, dtype=torch.int64), persistent=False)
            self.register_buffer("_restart_status", torch.zeros(1, dtype=torch.int32), persistent=False)

    def get_embedding_dim(self):
        return self._embedding_dim

    def set_train_vq(self, train_vq):
        self._train_vq = train_vq

    def restarts_enabled(self):
        return self.__dict__.get("_dead_code_threshold", 0.0) > 0.0

    def draw_restart_rows(self, rows, n=None):
        """Draw ``n`` (default R) distinct positions in [0, rows), uniformly, from the private generator into the first n
        entries of ``_restart_rows``.  One call of the generator per step whatever the outcome (Floyd's sampling on n fp64
        uniforms), so a checkpointed generator state resumes the stream exactly."""
        n = self._restart_candidates if n is None else n
        if rows < n:
            raise ValueError("VectorQuantizerEMA: %d rows in this step but %d restart candidates to draw from them" % (rows, n))
        u = torch.rand(n, generator=self._restart_gen, dtype=torch.float64).tolist()
        chosen, out = set(), []
        for i, v in zip(range(rows - n, rows), u):
            t = min(int(v * (i + 1)), i)
            t = i if t in chosen else t
            chosen.add(t)
            out.append(t)
        self._restart_rows[:n].copy_(torch.tensor(out, dtype=torch.int64), non_blocking=True)

    def restarted_codes(self):
        """(codes restarted so far, dead codes found by the last step, before the cap) as Python ints.  ONE host sync: it
        reads the two device counters (and the gather's status word: a position outside the rows is a RuntimeError)."""
        if not self.restarts_enabled():
            return 0, 0
        total, dead, status = torch.cat([self._restart_counters, self._restart_status.to(torch.int64)]).tolist()
        if status != 0:
            raise RuntimeError("VectorQuantizerEMA: a restart position lay outside the step's rows (status %d)" % status)
        return int(total), int(dead)

    def apply_update(self, sink, skip=None):
        """Apply a step's statistics: the EMA update from ``sink.counts`` / ``sink.sums``, then -- restarts on -- the dead
        codes' restart from ``sink.cand``.  ``skip``: a Trainer's skip slot (non-zero: nothing is written)."""
        weight = self._embedding.weight.data
        _native.vq_ema_update(sink.counts, sink.sums, self._ema_cluster_size, self._ema_w.data, weight, self._decay,
                              self._epsilon, skip=skip)
        if sink.cand is not None:
            _native.vq_restart_dead(sink.cand, self._ema_cluster_size, self._ema_w.data, weight, self._restart_counters,
                                    self._dead_code_threshold, skip=skip)

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
        # a Trainer's sink: statistics and candidates only, it applies the update after the all-reduce; else a sink of our own
        sink = _ops.ema_sink(self)
        local = sink is None
        if local:
            sink = _ops.EMASink.local(self, inputs.device)
        if rows * sink.world >= 1 << 24:
            raise ValueError("VectorQuantizerEMA: %d rows per step (over %d rank(s)) >= 2^24: the counts travel as fp32"
                             % (rows * sink.world, sink.world))
        if rows < sink.slots:
            raise ValueError("VectorQuantizerEMA: %d rows on this rank, fewer than the restart candidates it must supply" % rows)
        # the backward needs the codebook this forward quantised with: updating at once, quantise with a copy
        out = _ops.VQEMAFn.apply(inputs, weight.detach().clone() if local else weight, beta, (sink.counts, sink.sums))
        if sink.cand is not None:                # restarts: draw (unless a capture is recording) and gather this rank's slots
            self._restart_nrows = rows
            if not torch.cuda.is_current_stream_capturing():
                self.draw_restart_rows(rows, sink.slots)
            _native.vq_restart_gather(_ops.dense(inputs.detach()).view(-1, D), self._restart_rows, sink.cand,
                                      self._restart_status, first=sink.rank, stride=sink.world)
        sink.written = True
        if local:
            self.apply_update(sink)
        return out

    def forward(self, inputs):
        loss, quantized, perplexity, idx = self.quantize(inputs)
        encodings = _native.onehot(idx, self._num_embeddings)
        return loss, quantized, perplexity, encodings
