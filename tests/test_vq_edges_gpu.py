"""The kernels of csrc/vq.hip -- the nearest-code search, the straight-through gather with loss and perplexity, the two
backward kernels and the one-hot expansion -- against the float64 restatement (tests/helpers/vq_ref.py) at their edges.  The
grid is tests/helpers/vq_edge_cases.py; tests/test_vq_ref_cpu.py checks its preconditions on the host.

Two families of data:

* an integer lattice (values in [-16, 16], D <= 512): |x|^2, |e|^2, x.e and the distance are integers below 2^24, exact in
  float32 in any order, so the search has no rounding freedom: index and minimum distance equal the restatement's on every
  row, with bitwise-equal code rows planted across every boundary the kernels reduce over.  With grad_loss chosen so that
  float32(gl) float32(2 / (N D)) is a power of two, every term and every sum of the codebook gradient is exact as well:
  bit for bit, so that a dropped, doubled or misassigned row cannot pass;
* Gaussian rows against a N(0, 0.8) or a U(+-1/K) codebook, because a lattice cannot show a lost low-order bit.

Every tolerance is derived (u = 2^-24), none is taken from a device run:
  exact              lattice index, distance, codebook gradient; q_st (IEEE float32 add and subtract); histogram; one-hot
  search             (D + 4) u (|x|^2 + |e|^2 + 2 sum |x_i e_i|): three sums of D float32 terms and the two final operations;
                     the chosen code is nearest up to the bounds of both codes, on every row
  loss               (c + 3) u relative, c the longest chain of float32 additions (vq_ref.loss_chain)
  perplexity         (ceil(K / 256) + 8 + 2) u sum |p log p| + u relative; 2: ulp of the device logf
  dx                 3 u (|g| + |sx (e - x)|) per element
  dE, Gaussian       (n_k + P + G + 2) u sum |term| per entry
Each test prints its largest measured / bound ratio."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import vq_edge_cases as E  # noqa: E402
import vq_ref as R  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402

DEV = "cuda"
REF_SLACK = 1.0 + 2.0 ** -28     # the restatement's own float64 error where it takes the expanded form (vq_ref.distances_expanded)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def ratio(err, bound):
    """Largest err / bound; a zero bound admits a zero error only."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def search(case, x, e):
    """Index and minimum distance with every vq_reg the case is run with; they must agree bit for bit."""
    xd, ed = dev(x), dev(e)
    outs = []
    prev = N.get_option("vq_reg")
    try:
        for reg in E.regs_of(case):
            N.set_option("vq_reg", reg)
            idx, dist = N.vq_argmin(xd, ed, want_dist=True)
            outs.append((idx.cpu().numpy(), dist.cpu().numpy()))
    finally:
        N.set_option("vq_reg", prev)
    for idx, dist in outs:
        assert idx.min() >= 0 and idx.max() < e.shape[0]
    for idx, dist in outs[1:]:
        assert np.array_equal(idx, outs[0][0]), "vq_reg 1 / 0 differ on %d rows" % int((idx != outs[0][0]).sum())
        assert np.array_equal(dist.view(np.int32), outs[0][1].view(np.int32))
    return outs[0]


# ------------------------------------------------------------------------------------------------------------ the search
@pytest.mark.parametrize("case", E.SEARCH, ids=E.search_id)
def test_search_lattice_is_exact(case):
    for v in range(len(E.tie_variants(case[3]))):
        x, e, planted = E.lattice_case(case, v)
        d = R.distances_auto(x, e)
        want = R.argmin(x, e, d)
        idx, dist = search(case, x, e)
        print("%s variant %d: %d of %d rows equal, %d planted" % (E.search_id(case), v, int((idx == want).sum()), len(want), len(planted)))
        assert np.array_equal(idx, want), "rows %s" % np.flatnonzero(idx != want)[:8]
        assert np.array_equal(dist.astype(np.float64), d.min(1))
        for row, lo, hi, kind in planted:                  # a tie row is at distance 0 from both: the lower code
            assert kind != "tie" or idx[row] <= lo


def check_search(x, e, idx, dist, d, rows=None):
    """The two bounds of the Gaussian families on the given rows -> (optimality ratio, distance ratio)."""
    rows = np.arange(x.shape[0]) if rows is None else rows
    b = R.error_bound(x, e) * REF_SLACK
    best = np.argmin(d, axis=1)
    dg, bg = d[rows, idx[rows]], b[rows, idx[rows]]
    r_opt = ratio(dg - d[rows, best[rows]], bg + b[rows, best[rows]])
    r_dist = ratio(np.abs(dist[rows].astype(np.float64) - dg), bg)
    return r_opt, r_dist


@pytest.mark.parametrize("family", ["gauss", "init"])
@pytest.mark.parametrize("case", E.SEARCH, ids=E.search_id)
def test_search_gaussian_within_the_bound_on_every_row(case, family):
    x, e = E.search_case(case, family)
    d = R.distances_auto(x, e)
    idx, dist = search(case, x, e)
    r_opt, r_dist = check_search(x, e, idx, dist, d)
    print("%s %s: largest measured / bound: optimality %.3g, distance %.3g; %d of %d rows differ from the float64 argmin"
          % (E.search_id(case), family, r_opt, r_dist, int((idx != np.argmin(d, axis=1)).sum()), len(idx)))
    assert r_opt <= 1.0 and r_dist <= 1.0


@pytest.mark.parametrize("case", E.separated_cases(), ids=E.search_id)
def test_search_separated_equals_the_float64_argmin(case):
    x, e = E.search_case(case, "separated")
    d = R.distances_auto(x, e)
    idx, dist = search(case, x, e)
    r_opt, r_dist = check_search(x, e, idx, dist, d)
    print("%s separated: largest measured / bound: distance %.3g" % (E.search_id(case), r_dist))
    assert np.array_equal(idx, np.argmin(d, axis=1)) and r_dist <= 1.0


@pytest.mark.parametrize("spec", E.NONFINITE, ids=[E.search_id(s[0]) for s in E.NONFINITE])
def test_search_nonfinite_rows(spec):
    """A row with a NaN or an infinity has no finite distance: index 0 and distance +inf (include/alvq.h); a code row with an
    infinity is never chosen; and no other row notices."""
    case, r_nan, r_inf, k_inf = spec
    x, e = E.search_case(case, "gauss")
    n, d_ = x.shape
    k = e.shape[0]
    clean_idx, clean_dist = search(case, x, e)
    xb = x.copy()
    xb[r_nan, d_ // 2] = np.nan
    xb[r_inf, d_ - 1] = np.inf
    idx, dist = search(case, xb, e)                   # search() checks the range before anything else reads the indices
    others = np.setdiff1d(np.arange(n), [r_nan, r_inf])
    assert np.array_equal(idx[others], clean_idx[others])
    assert np.array_equal(dist[others].view(np.int32), clean_dist[others].view(np.int32))
    assert idx[r_nan] == 0 and idx[r_inf] == 0 and np.isposinf(dist[r_nan]) and np.isposinf(dist[r_inf])
    # the gather may consume them: the bad rows read code 0
    q, _ = N.vq_gather_loss(dev(xb), dev(e), dev(idx), E.BETA)
    assert np.array_equal(bits(q.cpu().numpy()[others]), bits(R.gather_loss(x, e, idx, E.BETA)[0][others]))

    eb = e.copy()
    eb[k_inf, d_ // 3] = np.inf
    idx2, dist2 = search(case, xb, eb)
    assert idx2[r_nan] == 0 and idx2[r_inf] == 0 and np.isposinf(dist2[r_nan]) and np.isposinf(dist2[r_inf])
    keep = others[clean_idx[others] != k_inf]
    moved = others[clean_idx[others] == k_inf]
    assert np.array_equal(idx2[keep], clean_idx[keep])
    assert np.array_equal(dist2[keep].view(np.int32), clean_dist[keep].view(np.int32))
    assert (idx2[others] != k_inf).all()
    if len(moved):                                    # rows that lost their code: nearest among the finite ones
        e_rest = np.delete(e, k_inf, axis=0)
        back = np.delete(np.arange(k), k_inf)
        d = R.distances_auto(x[moved], e_rest)
        pos = np.searchsorted(back, idx2[moved])
        r_opt, r_dist = check_search(x[moved], e_rest, pos, dist2[moved], d)
        assert r_opt <= 1.0 and r_dist <= 1.0
    print("%s: %d rows had the infinite code" % (E.search_id(case), len(moved)))


# ---------------------------------------------------------------------------------------------- gather, loss, perplexity
def gather_direct(xd, ed, idxd, with_hist, ema=False):
    """The library entries themselves (the wrapper hides the histogram) -> (q_st, partials, hist or None, out or None)."""
    n, d = xd.shape
    k = ed.shape[0]
    q = torch.full_like(xd, float("nan"))
    partials = torch.full((N.VQ_PARTIALS,), float("nan"), device=DEV)
    hist = torch.zeros(k, device=DEV, dtype=torch.int32) if with_hist else None
    L = N.lib()
    N._check(L.alvq_vq_gather_loss_f32(xd.data_ptr(), ed.data_ptr(), idxd.data_ptr(), q.data_ptr(), partials.data_ptr(),
                                       hist.data_ptr() if with_hist else None, n, k, d, N._stream()), "alvq_vq_gather_loss_f32")
    out = None
    if with_hist:
        out = torch.full((2,), float("nan"), device=DEV)
        fin = L.alvq_vq_finalize_ema_f32 if ema else L.alvq_vq_finalize_f32
        N._check(fin(partials.data_ptr(), hist.data_ptr(), out.data_ptr(), n, k, d, E.BETA, N._stream()), "alvq_vq_finalize")
        out = out.cpu().numpy()
    return q.cpu().numpy(), partials.cpu().numpy(), None if hist is None else hist.cpu().numpy(), out


@pytest.mark.parametrize("family", ["lattice", "gauss"])
@pytest.mark.parametrize("case", E.GATHER, ids=[c[0] for c in E.GATHER])
def test_gather_loss_histogram_perplexity(case, family):
    name, n, k, d, draw, arg = case
    x, e, idx = E.gather_case(case, family)
    q_ref, loss_ref, hist_ref, perp_ref, sum_abs = R.gather_loss(x, e, idx, E.BETA)
    xd, ed, idxd = dev(x), dev(e), dev(idx)
    q, partials, hist, out = gather_direct(xd, ed, idxd, True)
    assert np.array_equal(bits(q), bits(q_ref))
    assert np.array_equal(hist, hist_ref) and int(hist.sum()) == n
    q0, partials0, _, _ = gather_direct(xd, ed, idxd, False)                  # hist == NULL: nothing else changes
    assert np.array_equal(bits(q0), bits(q)) and np.array_equal(bits(partials0), bits(partials))
    r_loss = ratio(abs(float(out[0]) - loss_ref), R.loss_bound(n, d) * loss_ref)
    r_perp = ratio(abs(float(out[1]) - perp_ref), R.perplexity_bound(k, sum_abs) * perp_ref)
    out_ema = gather_direct(xd, ed, idxd, True, ema=True)[3]
    loss_ema = R.gather_loss(x, e, idx, E.BETA, ema=True)[1]
    r_ema = ratio(abs(float(out_ema[0]) - loss_ema), R.loss_bound(n, d) * loss_ema)
    print("%s %s: largest measured / bound: loss %.3g, EMA loss %.3g, perplexity %.3g (perplexity %.6g, K %d)"
          % (name, family, r_loss, r_ema, r_perp, perp_ref, k))
    assert r_loss <= 1.0 and r_ema <= 1.0 and r_perp <= 1.0
    assert out_ema[1] == out[1]
    # the wrapper: the same numbers
    qw, outw = N.vq_gather_loss(xd, ed, idxd, E.BETA)
    assert np.array_equal(bits(qw.cpu().numpy()), bits(q)) and np.array_equal(bits(outw.cpu().numpy()), bits(out))
    if family == "lattice":                           # idempotence: rows that are their codes
        xi = dev(e[idx])
        qi, outi = N.vq_gather_loss(xi, ed, idxd, E.BETA)
        assert float(outi[0]) == 0.0 and torch.equal(qi, xi)


# ------------------------------------------------------------------------------------------------------------- backward
def backward_dev(g, gl, x, e, idx, **kw):
    dx, dE = N.vq_backward(None if g is None else dev(g), None if gl is None else dev(np.array([gl], np.float32)),
                           dev(x), dev(e), dev(idx), E.BETA, **kw)
    return None if dx is None else dx.cpu().numpy(), None if dE is None else dE.cpu().numpy()


@pytest.mark.parametrize("case", E.GATHER, ids=[c[0] for c in E.GATHER])
def test_backward_lattice_codebook_gradient_is_exact(case):
    name, n, k, d, draw, arg = case
    x, e, idx = E.gather_case(case, "lattice")
    gl, se = E.exact_grad_loss(n, d)
    dx_ref, dE_ref, _, dx_mag = R.backward(None, gl, x, e, idx, E.BETA)
    want = dE_ref.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), dE_ref)                  # the restatement is a float32 value itself
    dx, dE = backward_dev(None, gl, x, e, idx)
    wrong = np.flatnonzero((bits(dE) != bits(want)).any(1))
    print("%s: se = 2^%d, %d of %d codes differ; dx measured / bound %.3g"
          % (name, int(np.log2(float(se))), len(wrong), k, ratio(np.abs(dx - dx_ref), 3 * R.U * dx_mag)))
    assert len(wrong) == 0, "codes %s" % wrong[:8]
    assert np.array_equal(dx.astype(np.float64), dx_ref)                      # g = None: -sx (e - x), exact here
    dx2, dE2 = backward_dev(None, gl, x, e, idx)                              # the same from run to run
    assert np.array_equal(bits(dE2), bits(dE)) and np.array_equal(bits(dx2), bits(dx))
    _, dE3 = backward_dev(None, gl, x, e, idx, want_dx=False)
    assert np.array_equal(bits(dE3), bits(dE))
    # the accumulate form, against an integer base on the same scale
    base = E.lattice_base(E.case_seed(name) + 7, k, d, se)
    acc = dev(base)
    N.vq_backward(None, dev(np.array([gl], np.float32)), dev(x), dev(e), dev(idx), E.BETA, want_dx=False, dE_out=acc)
    want_acc = (base.astype(np.float64) + dE_ref).astype(np.float32)
    assert np.array_equal(want_acc.astype(np.float64), base.astype(np.float64) + dE_ref)
    assert np.array_equal(bits(acc.cpu().numpy()), bits(want_acc))


@pytest.mark.parametrize("case", E.GATHER, ids=[c[0] for c in E.GATHER])
def test_backward_gaussian_within_the_bounds(case):
    name, n, k, d, draw, arg = case
    x, e, idx = E.gather_case(case, "gauss")
    g = np.random.RandomState(E.case_seed(name) + 3).randn(n, d).astype(np.float32)
    counts = np.bincount(idx, minlength=k)
    worst_dx = worst_dE = 0.0
    first = None
    combos = ((g, 0.37), (None, 0.37), (g, None)) if n * d <= 1 << 22 else ((g, 0.37),)   # the two largest: one form
    for g_, gl in combos:
        dx_ref, dE_ref, sum_abs, dx_mag = R.backward(g_, gl, x, e, idx, E.BETA)
        dx, dE = backward_dev(g_, gl, x, e, idx)
        worst_dx = max(worst_dx, ratio(np.abs(dx - dx_ref), 3 * R.U * dx_mag))
        worst_dE = max(worst_dE, ratio(np.abs(dE - dE_ref), R.dE_bound(counts, n, d, sum_abs)))
        if first is None:
            first = (dx, dE)
    print("%s: largest measured / bound: dx %.3g, dE %.3g (P %d, G %d, largest code %d rows)"
          % (name, worst_dx, worst_dE, R.parts(n), R.groups(d), counts.max()))
    assert worst_dx <= 1.0 and worst_dE <= 1.0
    assert not dE[counts == 0].any()                                          # a code without a row gets a zero gradient
    # either output alone: the same bits
    dx_only, none = backward_dev(g, 0.37, x, e, idx, want_dE=False)
    none2, dE_only = backward_dev(g, 0.37, x, e, idx, want_dx=False)
    assert none is None and none2 is None
    assert np.array_equal(bits(dx_only), bits(first[0])) and np.array_equal(bits(dE_only), bits(first[1]))


# -------------------------------------------------------------------------------------------------------------- one-hot
@pytest.mark.parametrize("n,k", E.ONEHOT)
def test_onehot_is_exact(n, k):
    idx = np.random.RandomState(n + k).randint(0, k, n).astype(np.int64)
    idx[-1] = k - 1
    idx[0] = 0 if n > 1 else idx[0]
    enc = N.onehot(dev(idx), k).cpu().numpy()
    assert enc.shape == (n, k) and np.array_equal(bits(enc), bits(R.onehot(idx, k)))
    assert n * k <= 2048 * 256 * 8 or (n, k) == (4097, 1100)
