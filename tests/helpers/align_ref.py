"""A numpy float64 restatement of the frequency permutation alignment as include/alvq.h defines it (alvq_align_permutations_f64,
alvq_permute_bins): plain loops over the items, bins and iterations, for tests/test_align_cpu.py (which pins it) and
tests/test_align_gpu.py (which holds csrc/permutation_align.hip to it).  The seeded cases of both live here and are computed
once."""
import collections
import functools
import itertools

import numpy as np

U = 1.1e-16
MAX = np.finfo(np.float64).max
TOL_CAP = 1e-11          # every parity case's score tolerance stays under this: a float32 accumulation cannot hide behind it
MARGIN_FLOOR = 1e-9      # the smallest gap between the best and the second-best permutation score a case may have
ITERATIONS = 8           # the iteration counts 1..ITERATIONS of the parity tests

Align = collections.namedtuple("Align", "perm score changed status margin")
Case = collections.namedtuple("Case", "P scramble")


# -------------------------------------------------------------------------------------------------------------- definitions
@functools.lru_cache(maxsize=None)
def permutations(K):
    """(K!, K) int: the permutations of 0..K-1 in lexicographic order, row r the one of rank r."""
    return np.array(list(itertools.permutations(range(K))), dtype=np.int64).reshape(-1, K)


def is_permutation(row, K):
    return sorted(int(v) for v in row) == list(range(K))


def total(a, reverse):
    """The sum over the last axis, the terms added in the opposite order with reverse."""
    return np.ascontiguousarray(a[..., ::-1]).sum(axis=-1) if reverse else a.sum(axis=-1)


def bin_status(P, perm0):
    """(B, F) int32: 1 for a bin with a non-finite value or a perm0 row that is not a permutation of 0..K-1."""
    B, K, F, T = P.shape
    st = np.zeros((B, F), np.int32)
    for b in range(B):
        for f in range(F):
            bad = not np.isfinite(P[b, :, f]).all()
            if perm0 is not None and not is_permutation(perm0[b, f], K):
                bad = True
            st[b, f] = 1 if bad else 0
    return st


def rows(Pb, status_b, reverse=False):
    """u (K, F, T) of one item: every row of a status-0 bin less its mean, times rn = 1 / sqrt(sum_t (P - m)^2), or 0 where
    that sum is not > 0 and finite.  The rows of another bin are 0 and never read."""
    K, F, T = Pb.shape
    u = np.zeros((K, F, T))
    for f in range(F):
        if status_b[f] != 0:
            continue
        for j in range(K):
            with np.errstate(all="ignore"):
                m = total(Pb[j, f], reverse) / T
                d = Pb[j, f] - m
                v = total(d * d, reverse)
                rn = 1.0 / np.sqrt(v) if (v > 0 and v <= MAX) else 0.0
                u[j, f] = d * rn
    return u


def centroids(u, perm_b, status_b, reverse=False):
    """c (K, T) of one item: sum_f u[perm[f, k], f] over the bins of status 0, f rising (falling with reverse) from the first
    term, then scaled to unit length over t (0 where the length is not > 0 and finite)."""
    K, F, T = u.shape
    c = np.zeros((K, T))
    order = [f for f in (range(F - 1, -1, -1) if reverse else range(F)) if status_b[f] == 0]
    for k in range(K):
        for i, f in enumerate(order):
            c[k] = u[perm_b[f, k], f] if i == 0 else c[k] + u[perm_b[f, k], f]
        with np.errstate(all="ignore"):
            n = np.sqrt(total(c[k] * c[k], reverse))
            c[k] = c[k] / n if (n > 0 and n <= MAX) else 0.0
    return c


def assign(table):
    """(rank of the winner or -1, its score, the gap to the second best or inf) of a K x K table under alvq_assign_f64's rule,
    maximising: the score of a permutation is table[0, pi(0)] + table[1, pi(1)] + ..., k rising from the first term; NaN scores
    are skipped; the lowest rank wins among equal scores."""
    K = table.shape[0]
    pis = permutations(K)
    s = table[0, pis[:, 0]]
    for k in range(1, K):
        s = s + table[k, pis[:, k]]
    valid = np.nonzero(~np.isnan(s))[0]
    if valid.size == 0:
        return -1, np.nan, np.inf
    best = valid[np.argmax(s[valid])]                   # argmax: the first among equals, the ranks rising
    rest = s[valid[valid != best]]
    return int(best), s[best], (s[best] - rest.max()) if rest.size else np.inf


def align(P, iterations, perm0=None, reverse=False):
    """``Align(perm (B, F, K) int32, score (B, F), changed (B,) int32, status (B, F) int32, margin)`` of P (B, K, F, T): the
    definitions of include/alvq.h.  margin: the smallest gap, over all bins and iterations, between the best and the second-best
    permutation score (inf for K = 1).  reverse: the frames and the bins are added in the opposite order."""
    P = np.asarray(P, dtype=np.float64)
    B, K, F, T = P.shape
    status = bin_status(P, perm0)
    perm = np.tile(np.arange(K, dtype=np.int32), (B, F, 1))
    if perm0 is not None:
        live = status == 0
        perm[live] = np.asarray(perm0, dtype=np.int32)[live]
    score = np.full((B, F), np.nan)
    changed = np.zeros((B,), np.int32)
    margin = np.inf
    pis = permutations(K)
    for b in range(B):
        u = rows(P[b], status[b], reverse)
        for _ in range(iterations):
            c = centroids(u, perm[b], status[b], reverse)
            moved = 0
            new = perm[b].copy()                        # Jacobi: every bin is scored against the same centroids
            for f in range(F):
                if status[b, f] != 0:
                    continue
                table = np.array([[total(c[k] * u[j, f], reverse) for j in range(K)] for k in range(K)])
                rank, s, gap = assign(table)
                score[b, f] = s
                if rank < 0:
                    continue
                margin = min(margin, gap)
                new[f] = pis[rank]
                moved += int((new[f] != perm[b, f]).any())
            perm[b] = new
            changed[b] = moved
    return Align(perm, score, changed, status, margin)


def permute_bins(x, perm):
    """out[b, k, f, t] = x[b, perm[b, f, k], f, t]; a bin with an entry outside 0..K-1 passes through."""
    B, K, F, T = x.shape
    out = x.copy()
    for b in range(B):
        for f in range(F):
            if ((perm[b, f] >= 0) & (perm[b, f] < K)).all():
                out[b, :, f] = x[b, perm[b, f], f]
    return out


def permute_rows(a, perm):
    """out[b, f, k] = a[b, f, perm[b, f, k]] for a (B, F, K, ...)."""
    out = np.empty_like(a)
    for b in range(a.shape[0]):
        for f in range(a.shape[1]):
            out[b, f] = a[b, f, perm[b, f]]
    return out


def common_order(scramble_b, perm_b):
    """Whether perm undoes the scramble of one item up to ONE order: scramble[f][perm[f]] is the same for all f."""
    first = scramble_b[0][perm_b[0]]
    return all((scramble_b[f][perm_b[f]] == first).all() for f in range(scramble_b.shape[0]))


# -------------------------------------------------------------------------------------------------------------------- inputs
# (B, K, F, T, seed): the parity shapes of tests/test_align_gpu.py, the smallest at which each kernel path can go wrong.  The
# seeds are the first of 0, 1, ... under which the restatement alone meets the conditions tests/test_align_cpu.py asserts
# (a fixed point and one common order after 8 iterations, margin >= 1e-9 forward and reversed, the same perm in both orders).
PARITY = [(1, 1, 1, 2, 0),
          (2, 2, 5, 16, 0),
          (2, 3, 17, 64, 0),             # T a whole tile
          (2, 3, 9, 65, 0),              # a ragged last tile
          (1, 2, 3, 130, 0),             # a ragged last tile after two whole ones
          (2, 4, 24, 100, 0),
          (1, 5, 12, 128, 0),
          (1, 8, 6, 128, 0),             # all 8! ranks
          (3, 2, 33, 40, 0),
          (1, 2, 4, 257, 1)]             # more frames than a workgroup's threads
IDS = ["-".join(str(v) for v in s[:4]) for s in PARITY]


@functools.lru_cache(maxsize=None)
def case(B, K, F, T, seed):
    """``Case(P, scramble)``: K sources, each with a block on / off activity shared by all bins (blocks of max(1, T / 16)
    frames, on with probability 1 / 2, off at 0.05), times uniform(0.5, 1.5) noise per (k, f, t) and a uniform(0.5, 2) gain per
    (k, f), normalised over k, then scrambled by an independent random permutation per bin: class j of bin f is source
    scramble[b, f, j].  P (B, K, F, T) float64, scramble (B, F, K).  Shared between tests: read-only."""
    g = np.random.default_rng([seed, B, K, F, T])
    block = max(1, T // 16)
    on = g.random((B, K, (T + block - 1) // block)) < 0.5
    act = np.where(np.repeat(on, block, axis=2)[:, :, :T], 1.0, 0.05)
    M = act[:, :, None, :] * g.uniform(0.5, 1.5, (B, K, F, T)) * g.uniform(0.5, 2.0, (B, K, F, 1))
    M = M / M.sum(axis=1, keepdims=True)
    scramble = np.stack([np.stack([g.permutation(K) for _ in range(F)]) for _ in range(B)])
    P = np.empty_like(M)
    for b in range(B):
        for f in range(F):
            P[b, :, f] = M[b, scramble[b, f], f]
    P.setflags(write=False)
    scramble.setflags(write=False)
    return Case(P, scramble)


def parity_case(shape):
    return case(*shape)


@functools.lru_cache(maxsize=None)
def reference(shape, iterations=ITERATIONS, reverse=False):
    """The restatement of a parity shape after `iterations` iterations, computed once; its arrays are read-only."""
    out = align(parity_case(shape).P, iterations, reverse=reverse)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def e_ref(shape):
    """The largest |score_forward - score_reversed| over the iteration counts 1..ITERATIONS."""
    worst = 0.0
    for n in range(1, ITERATIONS + 1):
        a, b = reference(shape, n), reference(shape, n, reverse=True)
        worst = max(worst, float(np.abs(a.score - b.score).max()))
    return worst


def tolerance(shape):
    """tol = max(32 e_ref, 4 (T + F) u): 32 because one pair of orders is a single sample of reordering noise and the device's
    order is a third (iva_ref.w_tolerance); the second term bounds an inner product of unit vectors of length T against a
    centroid summed over F bins."""
    _, _, F, T = shape[:4]
    return max(32 * e_ref(shape), 4 * (T + F) * U)


def status_case():
    """PARITY[3] with a NaN in bin (0, 2), an infinity in bin (1, 0) and a start whose rows (0, 4) and (1, 5) are no
    permutations; what is left of each item when those bins are deleted."""
    shape = PARITY[3]
    B, K, F, T = shape[:4]
    P = parity_case(shape).P.copy()
    P[0, 1, 2, 7] = np.nan
    P[1, 2, 0, 64] = np.inf                               # the last frame of a ragged row
    perm0 = np.tile(np.arange(K, dtype=np.int32), (B, F, 1))
    perm0[0, 3] = [1, 2, 0]                               # a good row that is not the identity
    perm0[0, 4] = [0, 0, 1]
    perm0[1, 5] = [0, 1, 3]
    bad = {0: [2, 4], 1: [0, 5]}
    keep = {b: [f for f in range(F) if f not in bad[b]] for b in range(B)}
    return P, perm0, bad, keep


# ------------------------------------------------------------------------------------------------------- the cACGMM workflow
# (B, D, K, F, T, seed) of cacgmm_ref.case: cACGMM started from an init drawn independently per bin, aligned, and continued
CHAIN_CASE = (1, 4, 2, 33, 100, 7)
CHAIN_ITERATIONS = 10
Chain = collections.namedtuple("Chain", "init first aligned second perm agreements")


def per_bin_init(B, K, F, T, seed):
    """An init for cacgmm drawn independently per bin: uniform(0, 1) + 1e-3 per (b, k, f, t), normalised over k."""
    g = np.random.default_rng([seed, B, K, F, T, 1])
    m = g.random((B, K, F, T)) + 1e-3
    return m / m.sum(axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def chain(reverse=False):
    """``Chain(init, first, aligned, second, perm, agreements)``: cacgmm_ref.cacgmm for CHAIN_ITERATIONS iterations from the
    per-bin init (first: its Gmm), ``align`` of its masks with the default 10 iterations (perm), the masks so permuted
    (aligned), and CHAIN_ITERATIONS more from the aligned masks and quadratic (second: its Gmm); agreements: cacgmm_ref.agreement
    of first.masks, aligned and second.masks with the oracle masks.  Computed once; read-only."""
    import cacgmm_ref as C
    B, D, K, F, T, seed = CHAIN_CASE
    c = C.case(B, D, K, F, T, seed)
    init = per_bin_init(B, K, F, T, seed)
    first = C.cacgmm(c.X, init, CHAIN_ITERATIONS, reverse=reverse)
    perm = align(first.masks, 10, reverse=reverse).perm
    aligned = permute_bins(first.masks, perm)
    second = C.cacgmm(c.X, aligned, CHAIN_ITERATIONS, quadratic0=permute_bins(first.quadratic, perm), reverse=reverse)
    agreements = tuple(C.agreement(m[0], c.oracle[0])[0] for m in (first.masks, aligned, second.masks))
    for a in (init, aligned, perm):
        a.setflags(write=False)
    return Chain(init, first, aligned, second, perm, agreements)


def chain_tolerance():
    """cacgmm_ref.tolerance's rule on the chain: max(32 e_ref, 2 (T + F + 8 D) u), e_ref the largest difference of the masks
    (before and after the continuation) between the chain run forward and reversed.  An agreement is a mean of
    sum_k m[perm[k]] o[k] with sum_k o[k] = 1, so it moves by no more than the masks do."""
    _, D, _, F, T, _ = CHAIN_CASE
    a, b = chain(), chain(True)
    e = max(np.abs(a.first.masks - b.first.masks).max(), np.abs(a.second.masks - b.second.masks).max())
    return max(32 * e, 2 * (T + F + 8 * D) * U)
