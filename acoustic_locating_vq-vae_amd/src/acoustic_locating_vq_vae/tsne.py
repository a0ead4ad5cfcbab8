"""Exact t-SNE of latent code sequences on the device (csrc/tsne.hip): the analysis of the reference's
scripts/echoe_transfer.py, which embeds each sample's RIR codes in 2-D and colours the map by the source angle.

The contract is sklearn.manifold.TSNE(method="exact", n_components=2) of sklearn >= 1.2:

1. Distances.  metric="euclidean" on codes c (N, L): d2[i][j] = 2 (L - #{l : c[i][l] == c[j][l]}), the squared Euclidean
   distance of the one-hot expansions, exact, stored as fp32.  metric="precomputed": an (N, N) matrix used as given (not
   squared, as sklearn); negative entries and a non-square matrix raise ValueError.
2. Conditional affinities.  Per row i, over j != i, a binary search for beta in fp64 over the fp32 distances: at most 100
   steps from beta = 1, beta_min = -inf, beta_max = +inf; each step P_ij = exp(-d_ij beta), S = sum_j P_ij (1e-8 if 0),
   H = log S + beta sum_j d_ij P_ij / S; stop when |H - log(perplexity)| <= 1e-5; if H > target, beta_min = beta and beta
   doubles (beta_max infinite) or bisects with beta_max; otherwise the mirror image.  P_ij = exp(-d_ij beta) / S (fp32), with
   the beta and S of the last evaluation.
3. Joint P = (Pc + Pc^T) / max(sum, eps), then max(., eps) off the diagonal, eps = 2.220446049250313e-16 (the sum in fp64).
   P is fp32 and exactly symmetric; the diagonal is excluded from every sum.
4. num_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} num_ij, Q_ij = max(num_ij / Z, eps);
   grad_i = 4 sum_{j != i} (e P_ij - Q_ij) num_ij (y_i - y_j), e the current exaggeration;
   KL = sum_{i != j} e P_ij log(max(e P_ij, eps) / Q_ij), computed at check iterations and the last iteration of a phase.
5. Descent, per iteration: inc = update * grad < 0; gains += 0.2 where inc, *= 0.8 elsewhere, clipped to >= 0.01;
   grad *= gains; update = momentum update - lr grad; y += update.  Phase 1: iterations 0..249, e = early_exaggeration,
   momentum 0.5, n_iter_without_progress 250.  Phase 2: from the last iteration of phase 1 plus one (it runs even when
   phase 1 stopped early) to max_iter - 1, e = 1, momentum 0.8, the user's n_iter_without_progress.  update and gains
   restart at 0 and 1 in each phase.  Every iteration i with (i + 1) % 50 == 0 is a check: the best KL (reset per phase,
   best_iter = the phase's first iteration) is tracked, and the phase stops when i - best_iter > n_iter_without_progress
   or when |grad| (after the gains) <= min_grad_norm.  learning_rate="auto" is max(N / early_exaggeration / 4, 50).
   n_iter_ is the index of the last iteration run, kl_divergence_ the last KL computed (so an empty phase 2, at
   max_iter = 250, leaves phase 1's values, where sklearn reports 250 and an unset error).
6. init="random": 1e-4 * standard normal from a torch.Generator seeded by random_state (a different stream from numpy's,
   so embeddings do not match sklearn's for the same seed); or an (N, 2) array / tensor.

Deliberate differences from sklearn: the embedding, gradient, update and gains are float64 (sklearn's exact path keeps them
in float32); init="pca" (sklearn's default), method="barnes_hut" and n_components != 2 raise NotImplementedError.

The N x N matrix stays on the device (one fp32 matrix; 2 <= N <= 65536); the host reads two numbers every 50 iterations.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N_

EPS64 = float(np.finfo(np.float64).eps)
EXPLORATION_N_ITER = 250
N_ITER_CHECK = 50
MAX_N = 65536

__all__ = ["TSNE", "code_sq_distances"]


def _gpu(X, what):
    if not isinstance(X, torch.Tensor) or not X.is_cuda:
        raise RuntimeError("%s must be a tensor on the GPU (got %s); the HIP path has no CPU fallback"
                           % (what, X.device if isinstance(X, torch.Tensor) else type(X).__name__))
    return X


def _codes_i32(X, n_codes=None):
    """(N, L) int32 / int64 codes on the device -> contiguous int32 (int64 narrowed with a range check)."""
    if X.dim() != 2:
        raise ValueError("codes must be (N, L) (got %s)" % (tuple(X.shape),))
    if X.dtype == torch.int32:
        return X.contiguous()
    if X.dtype != torch.int64:
        raise ValueError("codes must be int32 or int64 (got %s)" % X.dtype)
    flag = N_.device_flag(X.device)
    K = int(n_codes) if n_codes is not None else 2 ** 31 - 1
    out = N_.indices_to_i32(X.contiguous(), K, flag)
    if int(flag.item()):
        raise ValueError("codes outside [0, %d)" % K)
    return out


def _onehot_codes(X, n_codes):
    """Dense one-hot floats (N, L, K), or (N, L*K) with n_codes=K -> int32 (N, L) codes."""
    if X.dim() == 3:
        Np, L, K = X.shape
    elif X.dim() == 2 and n_codes is not None:
        Np, K = X.shape[0], int(n_codes)
        if X.shape[1] % K:
            raise ValueError("a (N, L*K) input needs L*K divisible by n_codes=%d (got %d columns)" % (K, X.shape[1]))
        L = X.shape[1] // K
    else:
        raise ValueError("float input must be one-hot (N, L, K), or (N, L*K) with n_codes=K; for general features pass "
                         "squared distances with metric=\"precomputed\"")
    idx, flag = N_.onehot_to_index(X.reshape(Np * L, K).float().contiguous())
    if int(flag.item()):
        raise ValueError("input rows are not exactly one-hot; for general features pass squared distances with "
                         "metric=\"precomputed\"")
    return idx.view(Np, L)


def code_sq_distances(codes, n_codes=None):
    """(N, N) fp32 squared distances between the one-hot expansions of code sequences: codes (N, L) int32 / int64, or dense
    one-hot floats (N, L, K) / (N, L*K) with n_codes=K, on the GPU.  d2[i][j] = 2 (L - matches), exact."""
    X = _gpu(codes, "codes")
    c = _codes_i32(X, n_codes) if not X.is_floating_point() else _onehot_codes(X, n_codes)
    if not 2 <= c.shape[0] <= MAX_N:
        raise ValueError("need 2 <= N <= %d points (got %d)" % (MAX_N, c.shape[0]))
    return N_.tsne_code_sqdist(c)


def _phase(step, it, n_iter, n_iter_without_progress, min_grad_norm, trace):
    """sklearn's _gradient_descent loop over iterations it..n_iter-1 of one phase, check by check.  step(n) runs the next n
    iterations on the device and returns (KL, |grad|) of the last of them.  Returns (kl, last iteration run), or
    (None, it - 1) when the range is empty."""
    best_error, best_iter = np.finfo(float).max, it
    kl, i = None, it - 1
    while i + 1 < n_iter:
        start = i + 1
        stop = min(((start // N_ITER_CHECK) + 1) * N_ITER_CHECK - 1, n_iter - 1)   # next check iteration, or the phase's last
        kl, grad_norm = step(stop - start + 1)
        i = stop
        trace.append((i, kl, grad_norm))
        if (i + 1) % N_ITER_CHECK == 0:
            if kl < best_error:
                best_error, best_iter = kl, i
            elif i - best_iter > n_iter_without_progress:
                break
            if grad_norm <= min_grad_norm:
                break
    return kl, i


def _schedule(run_phase, max_iter, early_exaggeration, n_iter_without_progress, min_grad_norm):
    """The two phases.  run_phase(exaggeration, momentum) resets update and gains and returns step(n) for that phase.
    Returns (kl_divergence_, n_iter_, trace of (iteration, KL, |grad|) at every host read)."""
    trace = []
    kl, it = _phase(run_phase(early_exaggeration, 0.5), 0, EXPLORATION_N_ITER, EXPLORATION_N_ITER, min_grad_norm, trace)
    kl2, it2 = _phase(run_phase(1.0, 0.8), it + 1, max_iter, n_iter_without_progress, min_grad_norm, trace)
    if kl2 is not None:
        kl, it = kl2, it2
    return kl, it, trace


class TSNE:
    """Exact t-SNE on the device; see the module docstring for the contract.  fit_transform(X) -> (N, 2) float64 GPU tensor.

    X: integer codes (N, L) (int32 / int64), dense one-hot floats (N, L, K) or (N, L*K) with n_codes=K, or with
    metric="precomputed" an (N, N) distance matrix; always a GPU tensor."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
                 n_iter=None, n_iter_without_progress=300, min_grad_norm=1e-7, metric="euclidean", init="random",
                 random_state=None, method="exact", n_codes=None):
        if n_components != 2:
            raise NotImplementedError("only n_components=2 is implemented (got %r)" % (n_components,))
        if method == "barnes_hut":
            raise NotImplementedError("method=\"barnes_hut\" is not implemented; use method=\"exact\"")
        if method != "exact":
            raise ValueError("method must be \"exact\" (got %r)" % (method,))
        if n_iter is not None:
            max_iter = n_iter
        if int(max_iter) < EXPLORATION_N_ITER:
            raise ValueError("max_iter should be greater than or equal to %d (got %r)" % (EXPLORATION_N_ITER, max_iter))
        if metric not in ("euclidean", "precomputed"):
            raise ValueError("metric must be \"euclidean\" or \"precomputed\" (got %r)" % (metric,))
        if isinstance(init, str):
            if init == "pca":
                raise NotImplementedError("init=\"pca\" is not implemented; use \"random\" or an (N, 2) array")
            if init != "random":
                raise ValueError("init must be \"random\" or an (N, 2) array (got %r)" % (init,))
        if not float(perplexity) > 0:
            raise ValueError("perplexity must be > 0 (got %r)" % (perplexity,))
        if not float(early_exaggeration) >= 1:
            raise ValueError("early_exaggeration must be >= 1 (got %r)" % (early_exaggeration,))
        if not (learning_rate == "auto" or float(learning_rate) > 0):
            raise ValueError("learning_rate must be \"auto\" or > 0 (got %r)" % (learning_rate,))
        self.n_components, self.perplexity, self.early_exaggeration = 2, float(perplexity), float(early_exaggeration)
        self.learning_rate, self.max_iter, self.n_iter_without_progress = learning_rate, int(max_iter), int(n_iter_without_progress)
        self.min_grad_norm, self.metric, self.init, self.random_state = float(min_grad_norm), metric, init, random_state
        self.method, self.n_codes = method, n_codes

    def _distances(self, X):
        X = _gpu(X, "X")
        if self.metric == "precomputed":
            if X.dim() != 2 or X.shape[0] != X.shape[1]:
                raise ValueError("a precomputed distance matrix must be square (got %s)" % (tuple(X.shape),))
            if not X.is_floating_point():
                raise ValueError("a precomputed distance matrix must be floating point (got %s)" % X.dtype)
            if bool((X < 0).any()):
                raise ValueError("a precomputed distance matrix must be non-negative")
            d2 = X.to(torch.float32).contiguous()
            return d2.clone() if d2.data_ptr() == X.data_ptr() else d2      # the affinities overwrite it
        return code_sq_distances(X, self.n_codes)

    def _init(self, n, device):
        if isinstance(self.init, str):
            g = torch.Generator()
            if self.random_state is None:
                g.seed()
            else:
                g.manual_seed(int(self.random_state))
            return (1e-4 * torch.randn((n, 2), generator=g, dtype=torch.float64)).to(device)
        Y = torch.as_tensor(self.init)
        if tuple(Y.shape) != (n, 2):
            raise ValueError("init must have shape (%d, 2) (got %s)" % (n, tuple(Y.shape)))
        return Y.to(device=device, dtype=torch.float64).contiguous().clone()

    def fit_transform(self, X, y=None):
        P = self._distances(X)
        n = P.shape[0]
        if not 2 <= n <= MAX_N:
            raise ValueError("need 2 <= N <= %d points (got %d)" % (MAX_N, n))
        if self.perplexity >= n:
            raise ValueError("perplexity must be less than n_samples (got %g >= %d)" % (self.perplexity, n))
        Y = self._init(n, P.device)
        self.learning_rate_ = max(n / self.early_exaggeration / 4.0, 50.0) if self.learning_rate == "auto" \
            else float(self.learning_rate)
        N_.tsne_affinities(P, self.perplexity)
        dev, f64 = P.device, torch.float64
        update, gains = torch.zeros((n, 2), device=dev, dtype=f64), torch.ones((n, 2), device=dev, dtype=f64)
        grad, stats = torch.empty((n, 2), device=dev, dtype=f64), torch.empty((2,), device=dev, dtype=f64)
        ws = [None]

        def run_phase(exaggeration, momentum):
            update.zero_()
            gains.fill_(1.0)

            def step(k):
                ws[0] = N_.tsne_descend(P, Y, update, gains, grad, stats, k, exaggeration, momentum, self.learning_rate_, ws[0])
                kl, gn = stats.tolist()                                   # the only host read: once per check
                return kl, gn
            return step

        self.kl_divergence_, self.n_iter_, self._trace = _schedule(run_phase, self.max_iter, self.early_exaggeration,
                                                                   self.n_iter_without_progress, self.min_grad_norm)
        self.embedding_ = Y
        return Y

    def fit(self, X, y=None):
        self.fit_transform(X)
        return self
