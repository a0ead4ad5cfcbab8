"""The kernels of csrc/kmeans.hip, entry point by entry point, against the float64 restatement (tests/helpers/kmeans_ref.py,
vq_ema_ref.py) at the edges of what they promise: K up to 16384, D up to 512, N from 1 to 130 000, any number of empty
clusters and the defined relocation order.  The grid is tests/helpers/kmeans_edge_cases.py; tests/test_kmeans_cpu.py
checks its preconditions on the host.

The labels are an input here (drawn, not computed), so no fp32 argmin decides anything.  Two families of data:

* an integer lattice (values in [-16, 16], a few far rows at 40): every fp64 sum the kernels take is an integer below
  2^53, exact in any order, so the device has no rounding freedom and must give the restatement's result exactly: centres
  bit for bit, counts, flags, relocated rows and their order, k-means++ indices, inertia;
* Gaussian rows (kmeans_ref.planted), because a lattice cannot show a lost low-order bit.

Every tolerance is derived, none is taken from a device run:
  exact            lattice results (see above)
  1 fp32 ulp       a Gaussian centre / column mean / EMA state value: the order error of an fp64 sum (<= N 2^-53 of the
                   sum of magnitudes) is far below half an fp32 ulp and can only flip the final rounding
  3 fp32 ulp       the EMA codebook = fp32 quotient of two stored values (one ulp per operand, one of its own)
  K 2^-50 rel.     center_shift_tot against the shift recomputed from the fp32-rounded centres: K non-negative fp64 terms
                   in another order, each through a square root and a re-squaring
  N 2^-52 rel.     a Gaussian inertia: N non-negative fp64 terms in another order
  N 2^-50 rel.     var_mean: two more bits for the rounding of the fp64 mean it subtracts
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import kmeans_edge_cases as E  # noqa: E402
import kmeans_ref as R  # noqa: E402
import vq_ema_ref as V  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import kmeans as KM  # noqa: E402

DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def device_update(x, labels, labels_old, c, tol, ws=None, poison=True):
    """One alvq_kmeans_update_f32 -> (centres, counts, center_shift_tot, flags, workspace), on the host."""
    K = c.shape[0]
    new = torch.full_like(c, float("nan")) if poison else torch.empty_like(c)
    counts = torch.full((K,), -7, device=DEV, dtype=torch.int32)
    stats = torch.full((1,), float("nan"), device=DEV, dtype=torch.float64)
    flags = torch.full((4,), -7, device=DEV, dtype=torch.int32)
    ws = N.kmeans_update(x, labels, labels_old, c, new, counts, stats, flags, tol, ws)
    return new.cpu().numpy(), counts.cpu().numpy(), float(stats.item()), flags.cpu().numpy().tolist(), ws


def reference_update(X, C, labels):
    K = C.shape[0]
    centres, _, moved, counts, n_empty, pairs = R.update(X.astype(np.float64), labels, C.astype(np.float64), K, full=True)
    return centres.astype(np.float32), counts, n_empty, moved, pairs, R.shift_of_rounded(centres, C)


# ------------------------------------------------------------------------------------------------ kmeans_update
@pytest.mark.parametrize("case", E.UPDATE_LATTICE, ids=[c[0] for c in E.UPDATE_LATTICE])
def test_update_lattice_is_exact(case):
    name, N_, D, K, maker, arg = case
    X, C, labels, n_empty = E.update_case(case)
    want, counts_ref, ne_ref, moved, pairs, shift_ref = reference_update(X, C, labels)
    assert ne_ref == n_empty
    x, c, lab = dev(X), dev(C), dev(labels)

    # no previous labels; tol just below the shift: go on (verdict 0)
    tol_lo, tol_hi = shift_ref * (1.0 - 1e-9), shift_ref * (1.0 + 1e-9)
    new, counts, tot, flags, _ = device_update(x, lab, None, c, tol_lo)
    print("%s: empty %d relocated %d shift %.17g (ref %.17g)" % (name, flags[2], flags[3], tot, shift_ref))
    assert np.array_equal(bits(new), bits(want)), "centres differ in %d elements" % int((bits(new) != bits(want)).sum())
    assert np.array_equal(counts, counts_ref) and int(counts.sum()) == N_
    assert flags[1:] == [1, n_empty, moved]
    assert abs(tot - shift_ref) <= K * 2.0 ** -50 * shift_ref
    assert flags[0] == (0 if shift_ref > 0 else 2)
    # the relocated rows, in order: row f of pair j is the centre of the j-th empty cluster
    for f, e in pairs[:8] + pairs[-8:]:
        assert counts[e] == 1 and np.array_equal(new[e], X[f])

    # previous labels that differ in the last row only (the ragged block when N is no multiple of 1024); tol just above
    old = labels.copy()
    old[-1] = (old[-1] + 1) % K if K > 1 else -1
    new2, counts2, tot2, flags2, _ = device_update(x, lab, dev(old), c, tol_hi)
    assert flags2 == [2, 1, n_empty, moved] and tot2 == tot
    assert np.array_equal(bits(new2), bits(new)) and np.array_equal(counts2, counts)

    # previous labels equal: strict convergence whatever the shift
    new3, counts3, tot3, flags3, _ = device_update(x, lab, lab.clone(), c, 0.0)
    assert flags3 == [1, 0, n_empty, moved] and tot3 == tot
    assert np.array_equal(bits(new3), bits(new)) and np.array_equal(counts3, counts)


def test_update_counts_may_be_null_and_relocation_count_when_rows_run_out():
    """N < number of empty clusters: every row moves, the pairing stops, flags[3] = N."""
    X, C = R.lattice(77, 5, 3, 64)
    labels = R.labels_one(5, 63)
    want, counts_ref, n_empty, moved, pairs, _ = reference_update(X, C, labels)
    assert n_empty == 63 and moved == 5 and [e for _, e in pairs] == [0, 1, 2, 3, 4]
    new = torch.full((64, 3), float("nan"), device=DEV)
    stats = torch.empty(1, device=DEV, dtype=torch.float64)
    flags = torch.empty(4, device=DEV, dtype=torch.int32)
    N.kmeans_update(dev(X), dev(labels), None, dev(C), new, None, stats, flags, 0.0)
    assert flags.cpu().tolist() == [0, 1, 63, 5]
    assert np.array_equal(bits(new.cpu().numpy()), bits(want))
    assert not new[5:].any()                    # clusters that stay empty keep their zero sum, the source was emptied too


def test_update_workspace_reuse_is_bitwise_a_fresh_one():
    """The workspace of a larger earlier call (other N, K, D: every offset differs, stale contents everywhere)."""
    big = ("ws_big", 5000, 129, 1025, "uniform", None)
    Xb, Cb, lb, _ = E.update_case(big)
    _, _, _, _, ws = device_update(dev(Xb), dev(lb), None, dev(Cb), 0.0)
    for case in [c for c in E.UPDATE_LATTICE if c[0] in ("n1023_k1000", "two_e7", "n64_sorted", "alone_e1")]:
        X, C, labels, n_empty = E.update_case(case)
        x, c, lab = dev(X), dev(C), dev(labels)
        assert N.lib().alvq_kmeans_update_workspace_bytes(case[1], case[3], case[2]) < ws.numel()
        a = device_update(x, lab, None, c, 0.0, ws)
        assert a[4] is ws
        b = device_update(x, lab, None, c, 0.0)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
        assert np.array_equal(bits(a[0]), bits(reference_update(X, C, labels)[0]))


@pytest.mark.parametrize("case", E.UPDATE_GAUSS, ids=[c[0] for c in E.UPDATE_GAUSS])
def test_update_gaussian_within_one_ulp(case):
    name, N_, D, K, maker, arg = case
    X, C, labels, n_empty = E.update_case(case, gauss=True)
    if n_empty:    # the precondition: the reference alone decides the relocation order
        assert R.relocation_order_is_decided(X, labels, C, n_empty)
    want, counts_ref, _, moved, pairs, shift_ref = reference_update(X, C, labels)
    new, counts, tot, flags, _ = device_update(dev(X), dev(labels), None, dev(C), 0.0)
    ulps = R.ulp_distance(new, want)
    print("%s: empty %d relocated %d, centres differ by at most %d ulp (%d of %d elements differ), shift rel. err %.3g"
          % (name, flags[2], flags[3], ulps.max(), int((ulps > 0).sum()), ulps.size, abs(tot - shift_ref) / shift_ref))
    assert flags == [0, 1, n_empty, moved]
    assert np.array_equal(counts, counts_ref) and int(counts.sum()) == N_
    assert ulps.max() <= 1
    for f, e in pairs:
        assert np.array_equal(bits(new[e]), bits(X[f]))             # a relocated centre is the row itself
    # the shift of the device's own fp32 centres: the same K 2^-50 bound as on the lattice
    own = R.shift_of_rounded(new.astype(np.float64), C)
    assert abs(tot - own) <= K * 2.0 ** -50 * own


# --------------------------------------------------------------------- kmeans_inertia / col_stats / add_rows
@pytest.mark.parametrize("shape", E.ROW_SHAPES, ids=["%dx%d_k%d" % s for s in E.ROW_SHAPES])
def test_inertia_col_stats_add_rows(shape):
    N_, D, K = shape
    for family in ("lattice", "gauss"):
        if family == "lattice":
            X, C = R.lattice(N_ + D + K, N_, D, K)
        else:
            X, _ = R.planted(N_ + D + K, N_, D, min(K, N_))
            C = (np.random.RandomState(K).randn(K, D) * 4.0).astype(np.float32)
        labels = R.labels_uniform(N_ + D, N_, K)
        X64, C64 = X.astype(np.float64), C.astype(np.float64)
        x = dev(X)
        inertia = float(N.kmeans_inertia(x, dev(labels), dev(C)).item())
        inertia_ref = float(((X64 - C64[labels]) ** 2).sum())
        mean, var_mean = N.kmeans_col_stats(x)
        mean, var_mean = mean.cpu().numpy(), float(var_mean.item())
        mean_ref = X64.sum(0) / N_
        var_ref = float(np.mean(((X64 - mean_ref) ** 2).sum(0) / N_))
        print("%s %s: inertia %.17g (ref %.17g), var_mean %.17g (ref %.17g), mean ulp %d"
              % (shape, family, inertia, inertia_ref, var_mean, var_ref, R.ulp_distance(mean, mean_ref.astype(np.float32)).max()))
        if family == "lattice":
            assert inertia == inertia_ref
            assert np.array_equal(bits(mean), bits(mean_ref.astype(np.float32)))
        else:
            assert abs(inertia - inertia_ref) <= N_ * 2.0 ** -52 * inertia_ref
            assert R.ulp_distance(mean, mean_ref.astype(np.float32)).max() <= 1
        assert abs(var_mean - var_ref) <= N_ * 2.0 ** -50 * var_ref
        # x + alpha v, out of place and in place; alpha = -1 (the centring) and one that rounds
        for alpha, v in ((-1.0, mean), (0.3, C[0])):
            plain, fused = R.add_rows_both(X, v, alpha)
            y = N.kmeans_add_rows(x, dev(v), alpha).cpu().numpy()
            assert ((bits(y) == bits(plain)) | (bits(y) == bits(fused))).all()
            xin = x.clone()
            out = N.kmeans_add_rows(xin, dev(v), alpha, out=xin)
            assert out is xin and np.array_equal(bits(xin.cpu().numpy()), bits(y))


# ------------------------------------------------------------------------------------------------ kmeans_plusplus
@pytest.mark.parametrize("case", E.PLUSPLUS, ids=[c[0] for c in E.PLUSPLUS])
def test_plusplus_lattice_indices_are_exact(case):
    name, N_, D, K, T, first, dups = case
    X, u = E.plusplus_case(case)
    want = R.kmeans_plusplus(X, K, first, u)
    x = dev(X)
    centers, idx = N.kmeans_plusplus(x, K, first, None if u is None else dev(u))
    idx = idx.cpu().numpy()
    print("%s: %d of %d indices equal" % (name, int((idx == want).sum()), K))
    assert np.array_equal(idx, want)
    assert np.array_equal(bits(centers.cpu().numpy()), bits(X[want]))


# ------------------------------------------------------------------------------------------ vq_ema_stats / update
@pytest.mark.parametrize("case", E.EMA_STATS, ids=["%dx%d_k%d_%s" % c for c in E.EMA_STATS])
def test_vq_ema_stats_lattice_is_exact(case):
    N_, D, K, maker = case
    X, _ = R.lattice(N_ + D + K, N_, D, 1)
    idx, _ = E.make_labels(N_ + K, N_, K, maker, None)
    c_ref, s_ref = V.stats(X, idx, K)
    counts = torch.full((K,), float("nan"), device=DEV)
    sums = torch.full((K, D), float("nan"), device=DEV)
    N.vq_ema_stats(dev(X), dev(idx), counts, sums)
    counts, sums = counts.cpu().numpy(), sums.cpu().numpy()
    assert np.array_equal(counts, c_ref.astype(np.float32)) and counts.sum() == N_
    assert np.array_equal(bits(sums), bits(s_ref.astype(np.float32)))
    unused = c_ref == 0
    assert not sums[unused].any() and (K == 1 or unused.any())      # codes without a row are written as zeros


@pytest.mark.parametrize("shape", E.EMA_UPDATE, ids=["k%d_d%d" % s for s in E.EMA_UPDATE])
def test_vq_ema_update_against_the_rounded_restatement(shape):
    K, D = shape
    rs = np.random.RandomState(K + D)
    cs = (rs.rand(K) * 4 + 0.25).astype(np.float32)
    W = rs.randn(K, D).astype(np.float32)
    c = rs.randint(0, 5, K).astype(np.float32) * (rs.rand(K) < 0.7)          # some codes got no row
    c = c.astype(np.float32)
    s = (rs.randn(K, D) * np.maximum(c, 0)[:, None]).astype(np.float32)
    E0 = rs.randn(K, D).astype(np.float32)
    decay, eps = 0.99, 1e-5
    cs_ref, W_ref, E_ref = V.update_rounded(cs, W, c, s, decay, eps)
    # skip non-zero: nothing is written
    d_cs, d_W, d_E = dev(cs), dev(W), dev(E0)
    N.vq_ema_update(dev(c), dev(s), d_cs, d_W, d_E, decay, eps, skip=torch.ones(1, device=DEV))
    assert np.array_equal(bits(d_cs.cpu().numpy()), bits(cs)) and np.array_equal(bits(d_W.cpu().numpy()), bits(W))
    assert np.array_equal(bits(d_E.cpu().numpy()), bits(E0))
    for skip in (torch.zeros(1, device=DEV), None):
        d_cs, d_W, d_E = dev(cs), dev(W), dev(E0)
        N.vq_ema_update(dev(c), dev(s), d_cs, d_W, d_E, decay, eps, skip=skip)
        u = [int(R.ulp_distance(a.cpu().numpy(), b).max()) for a, b in ((d_cs, cs_ref), (d_W, W_ref), (d_E, E_ref))]
        print("K=%d D=%d: cluster size %d ulp, moving sum %d ulp, codebook %d ulp" % (K, D, u[0], u[1], u[2]))
        assert u[0] <= 1 and u[1] <= 1 and u[2] <= 3
        assert (c == 0).any() or K == 1


# ------------------------------------------------------------------------------------------------ two whole fits
def test_fit_k1_is_the_column_mean():
    X, _ = R.planted(11, 5000, 65, 3)
    init = X[:1].copy()
    _, _, C_ref, n_iter_ref = R.fit(X, init)
    assert n_iter_ref == 2
    km = KM.KMeans(n_clusters=1, init=init).fit(dev(X))
    assert km.n_iter_ == 2 and not km.labels_.any()
    X64 = X.astype(np.float64)
    m = X64.mean(0)
    got = km.cluster_centers_.cpu().numpy().astype(np.float64)[0]
    # three fp32 roundings on the way: the column mean (2^-24 |m|), each centred row (2^-24 max |x - m|, and so their
    # mean) and the centre shifted back (2^-24 |m|)
    bound = 2.0 ** -23 * (np.abs(X64 - m).max(0) + np.abs(m))
    assert (np.abs(got - m) <= bound).all() and (np.abs(got - C_ref[0]) <= bound).all()
    # the inertia of the fp32 centred rows about the fp32 centre: each difference is off by a few 2^-24 of its size
    inertia_ref = float(((X64 - m) ** 2).sum())
    assert abs(km.inertia_ - inertia_ref) <= 2.0 ** -20 * inertia_ref


def test_fit_every_row_its_own_centre():
    X, _ = R.planted(12, 64, 32, 64)
    x = dev(X)
    km = KM.KMeans(n_clusters=64, init=X.copy()).fit(x)
    assert np.array_equal(km.labels_.cpu().numpy(), np.arange(64))
    assert km.inertia_ == 0.0 and km.n_iter_ == 1
    labels_ref, inertia_ref, _, n_iter_ref = R.fit(X, X)
    assert np.array_equal(labels_ref, np.arange(64)) and n_iter_ref == 1 and inertia_ref <= 1e-20
