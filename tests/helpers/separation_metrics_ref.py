"""A numpy float64 restatement of the separation scores as include/alvq.h defines them (alvq_pairwise_si_sdr_*, alvq_assign_f64,
alvq_si_bss_eval_*) and acoustic_locating_vq_vae.speech_metrics composes them: plain loops, for
tests/test_separation_metrics_cpu.py (which pins it) and tests/test_separation_metrics_gpu.py (which holds
csrc/separation_metrics.hip to it).  Every sum over the samples runs one after the other with t rising, or falling with
``reverse=True``; the sums over sources (the assignment's score, the projection) run with the index rising always, as the
definition has them.  The seeded cases of both tests live here and are computed once."""
import collections
import functools

import numpy as np

U = 1.1e-16
MAX = np.finfo(np.float64).max
COND_CAP = 100.0         # cond_2(G) of every case's items (asserted by tests/test_separation_metrics_cpu.py)
VALUE_CAP = 60.0         # |SI-SDR|, |SIR|, |SAR| in dB of every case (asserted there too)
TOL_CAP = 1e-9           # dB: the tolerance of the SIR / SAR comparison must stay under this

BAD_INPUT, BAD_SOLVE, BAD_PERM = 1, 2, 3

Assign = collections.namedtuple("Assign", "perm total status")
Pit = collections.namedtuple("Pit", "value perm status")
SiBss = collections.namedtuple("SiBss", "sdr sir sar perm status energies cond")
Case = collections.namedtuple("Case", "references estimates scramble mixture")


# -------------------------------------------------------------------------------------------------------------- definitions
def total(x, reverse=False):
    """The sum of x along its last axis, one term after the other from the first (from the last with reverse)."""
    x = np.asarray(x, dtype=np.float64)
    return np.cumsum(x[..., ::-1] if reverse else x, axis=-1)[..., -1]


def ratio_db(num, den):
    """10 log10(num / den): NaN where either is NaN, +inf where den is 0."""
    if np.isnan(num) or np.isnan(den):
        return np.nan
    if den == 0.0:
        return np.inf
    with np.errstate(all="ignore"):
        return 10.0 * np.log10(num / den)


def centred(x, reverse=False):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        return x - total(x, reverse)[..., None] / x.shape[-1]


def si_sdr(reference, estimate, reverse=False):
    """alvq_si_sdr_*: NaN for a reference of zero or non-finite centred energy, +inf for an exact multiple."""
    with np.errstate(all="ignore"):
        s, e = centred(reference, reverse), centred(estimate, reverse)
        ss = total(s * s, reverse)
        if not (ss > 0.0 and ss <= MAX):
            return np.nan
        target = (total(e * s, reverse) / ss) * s
        return ratio_db(total(target * target, reverse), total((target - e) * (target - e), reverse))


def pairwise_si_sdr(references, estimates, reverse=False):
    """table (B, K, J) of references (B, K, n) and estimates (B, J, n)."""
    B, K, _ = references.shape
    J = estimates.shape[1]
    return np.array([[[si_sdr(references[b, i], estimates[b, j], reverse) for j in range(J)] for i in range(K)] for b in range(B)])


def injections(K, J):
    """The injections of 0..K-1 into 0..J-1 in lexicographic order of (pi(0), ..., pi(K-1))."""
    def extend(head):
        if len(head) == K:
            yield tuple(head)
            return
        for col in range(J):
            if col not in head:
                yield from extend(head + [col])
    return extend([])


@functools.lru_cache(maxsize=None)
def injection_table(K, J):
    """``injections(K, J)`` as an int array (count, K), row r the injection of rank r."""
    out = np.array(list(injections(K, J)), dtype=np.int64).reshape(-1, K)
    out.setflags(write=False)
    return out


def assign_one(table, maximize=True):
    """(perm, total, status) of one (K, J) table: the first injection of the largest (smallest) score that is not NaN, the
    score table[0, pi(0)] + table[1, pi(1)] + ... with k rising (all injections at once, each its own sum of doubles)."""
    K, J = table.shape
    pis = injection_table(K, J)
    with np.errstate(all="ignore"):
        score = table[0, pis[:, 0]]
        for k in range(1, K):
            score = score + table[k, pis[:, k]]
    valid = np.flatnonzero(~np.isnan(score))
    if valid.size == 0:
        return np.arange(K, dtype=np.int32), np.nan, 1
    pick = np.argmax if maximize else np.argmin           # both return the first extremum: the lowest rank
    rank = valid[pick(score[valid])]
    return pis[rank].astype(np.int32), score[rank], 0


def assign(table, maximize=True):
    out = [assign_one(t, maximize) for t in table]
    return Assign(np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out], dtype=np.float64),
                  np.array([o[2] for o in out], dtype=np.int32))


def pit_si_sdr(references, estimates, reverse=False):
    table = pairwise_si_sdr(references, estimates, reverse)
    a = assign(table)
    value = np.array([[table[b, k, a.perm[b, k]] for k in range(table.shape[1])] for b in range(table.shape[0])])
    return Pit(value, a.perm, a.status)


def solve(G, g):
    """G c = g by Gaussian elimination with partial pivoting -- the pivot of the largest |.| among the rows r >= j, the lowest
    row on ties -- and back substitution; None where a pivot is 0 or not finite."""
    m, z = np.array(G, dtype=np.float64), np.array(g, dtype=np.float64)
    K = m.shape[0]
    with np.errstate(all="ignore"):
        for j in range(K):
            p, top = j, abs(m[j, j])
            for r in range(j + 1, K):
                if abs(m[r, j]) > top:
                    p, top = r, abs(m[r, j])
            if not (top > 0.0 and top <= MAX):
                return None
            if p != j:
                m[[j, p]] = m[[p, j]]
                z[[j, p]] = z[[p, j]]
            for r in range(j + 1, K):
                l = m[r, j] / m[j, j]
                m[r, j:] -= l * m[j, j:]
                z[r] -= l * z[j]
        for j in range(K - 1, -1, -1):
            z[j] = z[j] / m[j, j]
            z[:j] -= m[:j, j] * z[j]
    return z


def is_injection(row, J):
    return all(0 <= v < J for v in row) and len(set(int(v) for v in row)) == len(row)


def si_bss_eval(references, estimates, perm=None, reverse=False):
    """``SiBss(sdr, sir, sar (B, K), perm, status (B,), energies (B, K, 6), cond (B,))``; energies: |target|^2, |target - e|^2,
    |interf|^2, |artif|^2, |proj|^2 and |e|^2; cond: cond_2(G) of the item (NaN where it has a status)."""
    references, estimates = np.asarray(references, dtype=np.float64), np.asarray(estimates, dtype=np.float64)
    B, K, n = references.shape
    J = estimates.shape[1]
    if perm is None:
        perm = pit_si_sdr(references, estimates, reverse).perm
    sdr, sir, sar = (np.full((B, K), np.nan) for _ in range(3))
    energies, cond, status = np.full((B, K, 6), np.nan), np.full(B, np.nan), np.zeros(B, np.int32)
    with np.errstate(all="ignore"):
        for b in range(B):
            if not is_injection(perm[b], J):
                status[b] = BAD_PERM
                continue
            s = centred(references[b], reverse)
            G = np.array([[total(s[min(p, q)] * s[max(p, q)], reverse) for q in range(K)] for p in range(K)])
            chosen = estimates[b, perm[b]]
            if not np.isfinite(chosen).all() or not all(G[p, p] > 0.0 and G[p, p] <= MAX for p in range(K)):
                status[b] = BAD_INPUT
            for i in range(K):
                e = centred(chosen[i], reverse)
                g = np.array([total(e * s[p], reverse) for p in range(K)])
                if not (G[i, i] > 0.0 and G[i, i] <= MAX):
                    continue
                target = (g[i] / G[i, i]) * s[i]
                en = [total(target * target, reverse), total((target - e) * (target - e), reverse)]
                sdr[b, i] = ratio_db(en[0], en[1])
                if status[b] != 0:
                    continue
                c = solve(G, g)
                if c is None:
                    status[b] = BAD_SOLVE
                    continue
                proj = c[0] * s[0]
                for p in range(1, K):
                    proj = proj + c[p] * s[p]
                interf, artif = proj - target, e - proj
                en += [total(interf * interf, reverse), total(artif * artif, reverse), total(proj * proj, reverse), total(e * e, reverse)]
                energies[b, i] = en
                sir[b, i], sar[b, i] = ratio_db(en[0], en[2]), ratio_db(en[4], en[3])
            if status[b] == 0:
                cond[b] = np.linalg.cond(G)
            else:
                sir[b], sar[b] = np.nan, np.nan
    return SiBss(sdr, sir, sar, np.asarray(perm, dtype=np.int32), status, energies, cond)


def si_sdr_improvement(references, estimates, mixture, reverse=False):
    before = pairwise_si_sdr(references, mixture[:, None], reverse)[:, :, 0]
    return pit_si_sdr(references, estimates, reverse).value - before


# -------------------------------------------------------------------------------------------------------------------- inputs
# (K, J, n): around one wave, one workgroup of 256 threads and one stride of it
SHAPES = [(1, 1, 2), (2, 2, 255), (2, 3, 257), (3, 3, 1025), (4, 8, 1025), (8, 8, 2049)]
IDS = ["-".join(str(v) for v in s) for s in SHAPES]
ITEMS = 3
BLOCK = 64               # samples that share one value of the envelope


@functools.lru_cache(maxsize=None)
def case(shape, items=ITEMS):
    """``Case(references (B, K, n), estimates (B, J, n), scramble (B, K), mixture (B, n))``: the references are standard normal
    noise under a blockwise gamma(2) envelope; estimate scramble[b, k] is source k; estimates = A s + 0.1 noise + 0.3 with A
    (J, K) the scrambled identity plus 0.15 standard normal; mixture = the sum of the references.  Shared: read-only."""
    K, J, n = shape
    g = np.random.default_rng([2019, K, J, n])
    envelope = np.repeat(g.gamma(2.0, size=(items, K, -(-n // BLOCK))) + 0.1, BLOCK, axis=2)[:, :, :n]
    s = g.standard_normal((items, K, n)) * envelope
    scramble = np.array([g.permutation(J)[:K] for _ in range(items)], dtype=np.int32)
    A = 0.15 * g.standard_normal((items, J, K))
    for b in range(items):
        A[b, scramble[b], np.arange(K)] += 1.0
    e = np.einsum("bjk,bkn->bjn", A, s) + 0.1 * g.standard_normal((items, J, n)) + 0.3
    mix = s.sum(axis=1)
    for a in (s, e, scramble, mix):
        a.setflags(write=False)
    return Case(s, e, scramble, mix)


def promoted(x, single):
    """The input the kernels see: rounded to float32 and promoted again where single."""
    return x.astype(np.float32).astype(np.float64) if single else x


@functools.lru_cache(maxsize=None)
def reference(shape, single=False, reverse=False):
    """``si_bss_eval`` of a case under the restatement's own permutation, computed once; read-only."""
    c = case(shape)
    out = si_bss_eval(promoted(c.references, single), promoted(c.estimates, single), reverse=reverse)
    for a in out:
        a.setflags(write=False)
    return out


def e_ref(shape, single=False):
    """The largest |forward - reversed| in dB of the restatement's sir and sar on the case."""
    a, b = reference(shape, single), reference(shape, single, reverse=True)
    return max(np.abs(a.sir - b.sir).max(), np.abs(a.sar - b.sar).max())


def tolerance(shape, single=False):
    """tol = 32 e_ref + 8.7 n u dB: 32 for the reason iva_ref.w_tolerance gives; 8.7 n u is the worst case of a sum of n
    rounded terms, n u relative, in dB (10 / ln 10 = 4.34 per energy, two energies a ratio)."""
    return 32 * e_ref(shape, single) + 8.7 * shape[2] * U
