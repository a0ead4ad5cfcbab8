"""The kernels of csrc/elementwise.hip, the Adam half of csrc/pack_weights.hip and csrc/location.hip, entry point by entry
point, against the float64 restatements of tests/helpers/elementwise_ref.py at the edges of their launch geometry: the
C = 256 | 257 switch between the two standardise kernels and its ragged channel groups, L = 1, one element per thread
| the stride loop (262144), the capped grid, the last row of a partial workgroup, the AS_MAX / AP_MAX chunking, the 16-byte
| scalar path of the fused Adam + pack, the full 16384-entry index table.  Where a wrapper allocates its own output the C
entry point is called with a pointer into a larger buffer prefilled with a NaN pattern (16-byte aligned offset): every
element outside the output must keep its bits.

Two families of data: an integer lattice, whose fp32 sums are exact in any order, so the device must give the float64 result
bit for bit; and Gaussian values, because a lattice cannot show a lost low-order bit.

Every tolerance is derived (tests/helpers/elementwise_ref.py holds each derivation in full), none is taken from a device
run, and tests/test_elementwise_ref_cpu.py proves each on a numpy-float32 emulation of the kernel's summation order, on the
same arrays.  u = 2^-24:
  exact                        lattice results; transpose, jitter, add, relu_mask, fill; a constant column's standardised 0;
                               the four Adam forms against each other; a skipped step; the images of the fused Adam + pack
  2 (C/4 + 7) u (max|x| / (std + 1e-8) + |ref|)
                               standardise, per element: (n + 2) u max|x| / den from the mean (n = ceil(C/4) terms per partial,
                               2 adds, 1 division) + (n/2 + 6.5) u |ref| from the deviations, var, sqrt, + 1e-8 and the division;
                               factor 2 for the second order.  CONDITIONED on max|x| / std: (C/4 + 7) u (max|x| / std) sqrt(C)
                               <= 1/4, checked; the data keeps |mean| / std <= 100
  (ceil(n / 262144) + 23) u    mse, relative: t - 1 adds per thread, 3 per term, butterfly 6, four waves 2, final 3 + 8, division 1
  2 fp32 ulp                   mse_backward: fl(2/n), (grad_loss times it,) the difference, the product
  (ceil(L / 64) + 7) u mean|x| row_mean: t - 1 adds per lane, butterfly 6, division 1, one for the second order
  2 fp32 ulp                   its adjoint: fl(1/L) and the product
  6 u max(|m|, |g gs|)         Adam m: g gs, gr - m (<= 2X), times (1 - beta1), + m
  6 u v'                       Adam v: all terms non-negative, 5 roundings on the longest path
  ulp(p) + u lr_bc1 (12 |m'| + 6 X) / denom
                               Adam p: denom 7.5 u (sqrt 3.5, / sqrt(bc2) 1 + its own 2, + eps 1), quotient 1 + m's error,
                               times lr_bc1 1 + its own 2, the subtraction half an ulp
  1 fp32 ulp                   adam_advance's scalars: a float64 pow / sqrt / quotient, rounded once
  (ceil(L / 64) + 7) u sum|terms|   bag forward: as row_mean, the bias in place of the division
  B u sum|terms|               bag backward, per column: at most B sequential adds
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import elementwise_ref as E  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from oracle import vqvae_oracle as O  # noqa: E402

DEV = "cuda"
PAD = 64                        # elements on either side of an output: it starts 256 bytes into the buffer
CANARY = 0x7FC0DEAD             # a NaN


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def call(name, *args):
    N._check(getattr(N.lib(), name)(*args, N._stream()), name)


class Guarded:
    """n 4-byte elements inside a larger buffer of CANARY (``init``: their initial values); .ptr for the C entry points,
    .get() checks that nothing outside was written and returns the elements."""

    def __init__(self, n, init=None):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), CANARY, device=DEV, dtype=torch.int32)
        if init is not None:
            self.buf[PAD:PAD + n] = dev(np.ascontiguousarray(init).reshape(-1).view(np.int32))
        self.ptr = self.buf.data_ptr() + 4 * PAD
        assert self.ptr % 16 == 0

    def tensor(self):
        return self.buf[PAD:PAD + self.n].view(torch.float32)

    def get(self, dtype=np.float32):
        torch.cuda.synchronize()
        b = host(self.buf)
        assert (b[:PAD] == CANARY).all(), "written before the output"
        assert (b[PAD + self.n:] == CANARY).all(), "written past the output"
        return b[PAD:PAD + self.n].view(dtype)


def same_bits(a, b):
    a, b = E.bits(a), E.bits(b)
    return a.shape == b.shape and bool((a == b).all())


# ------------------------------------------------------------------------------------------------------ standardise
@pytest.mark.parametrize("take_abs", [False, True], ids=["plain", "abs"])
@pytest.mark.parametrize("case", E.STD_CASES, ids=str)
def test_standardise(case, take_abs):
    B, C, L = case
    for kind in E.STD_DATA:
        x, const = E.standardise_data(B, C, L, kind, take_abs)
        ref, mean, std = E.standardise(x, take_abs)
        xd = dev(x)
        out = Guarded(x.size)
        call("alvq_standardise_f32", xd.data_ptr(), out.ptr, B, C, L, int(take_abs))
        y = out.get().reshape(B, C, L)
        free = np.broadcast_to(~const[:, None], x.shape)
        xmax = np.abs(x).max(1, keepdims=True)
        if free.any():
            assert E.standardise_precondition(C, xmax[~const[:, None]].max(), std[~const[:, None]].min())
        bound = E.standardise_bound(C, xmax, std, ref)
        err = np.abs(y.astype(np.float64) - ref)
        ratio = float(np.nan_to_num((err / bound)[free], nan=np.inf).max()) if free.any() else 0.0
        print("standardise %s %s %s: max error %.3g, at %.3f of the bound (max bound %.3g)"
              % (case, kind, "abs" if take_abs else "plain", err[free].max() if free.any() else 0.0, ratio, bound[free].max() if free.any() else 0.0))
        assert ratio <= 1.0
        if const.any():                                 # mean exact, deviations +0, 0 / (0 + 1e-8): exactly +0
            assert not E.bits(y)[np.broadcast_to(const[:, None], x.shape)].any()
        assert same_bits(host(N.standardise(xd, take_abs=take_abs)), y)        # the wrapper is that call


# -------------------------------------------------------------------------------------------------------------- mse
def device_mse(ad, bd):
    out = Guarded(1)
    ws = torch.empty(N.EW_PARTIALS, device=DEV)
    call("alvq_mse_f32", ad.data_ptr(), bd.data_ptr(), out.ptr, ws.data_ptr(), ad.numel())
    return out.get()[0]


@pytest.mark.parametrize("n", E.MSE_N)
def test_mse(n):
    a, b = E.mse_data(n, "lattice")
    S = ((a.astype(np.float64) - b) ** 2).sum()
    got = device_mse(dev(a), dev(b))
    assert same_bits(got, np.float32(S / n)), (got, S / n)
    a, b = E.mse_data(n, "gauss")
    ad, bd = dev(a), dev(b)
    ref = E.mse(a, b)
    got = device_mse(ad, bd)
    print("mse n=%d: %.9g (ref %.17g), rel. error %.3g, bound %.3g" % (n, got, ref, abs(got - ref) / ref, E.mse_bound(n)))
    assert abs(float(got) - ref) <= E.mse_bound(n) * ref
    assert same_bits(device_mse(ad, bd), got)                                  # two calls, the same bits
    assert same_bits(host(N.mse(ad, bd))[0], got)
    assert same_bits(device_mse(ad, ad), np.float32(0.0))


@pytest.mark.parametrize("n", E.MSE_BACKWARD_N)
def test_mse_backward(n):
    a, b = E.mse_data(n, "gauss")
    ad, bd = dev(a), dev(b)
    for gl in E.GRAD_LOSS:
        gld = dev(np.array([gl], np.float32))
        out = Guarded(n)
        call("alvq_mse_backward_f32", ad.data_ptr(), bd.data_ptr(), gld.data_ptr(), out.ptr, n)
        got = out.get()                                                        # the output ends at its canary
        d = E.ulp_distance(got, E.mse_backward(a, b, gl).astype(np.float32))
        print("mse_backward n=%d grad_loss=%g: at most %d ulp (bound %d)" % (n, gl, d.max(), E.MSE_BACKWARD_ULPS))
        assert d.max() <= E.MSE_BACKWARD_ULPS
    out = Guarded(n)                                                           # grad_loss NULL = 1
    call("alvq_mse_backward_f32", ad.data_ptr(), bd.data_ptr(), None, out.ptr, n)
    assert same_bits(out.get(), got)


# --------------------------------------------------------------------------------------------------------- row_mean
@pytest.mark.parametrize("L", E.ROW_MEAN_L)
def test_row_mean_and_its_adjoint(L):
    for B, D in E.ROW_MEAN_ROWS:
        rows = B * D
        x = E.row_mean_data(rows, L, "lattice")
        out = Guarded(rows)
        xd = dev(x)
        call("alvq_row_mean_f32", xd.data_ptr(), out.ptr, rows, L)
        got = out.get()                                                        # the element after the output is a canary
        want = (x.astype(np.float64).sum(1) / L).astype(np.float32)
        assert same_bits(got, want)
        assert same_bits(got[-1], want[-1])                                    # the last row of a partial workgroup
        x = E.row_mean_data(rows, L, "gauss")
        xd = dev(x)
        out = Guarded(rows)
        call("alvq_row_mean_f32", xd.data_ptr(), out.ptr, rows, L)
        got = out.get()
        err = np.abs(got.astype(np.float64) - E.row_mean(x))
        bound = E.row_mean_bound(L, np.abs(x.astype(np.float64)).mean(1))
        print("row_mean rows=%d L=%d: max error %.3g, at %.3f of the bound" % (rows, L, err.max(), (err / bound).max()))
        assert (err <= bound).all() and err[-1] <= bound[-1]
        assert same_bits(host(N.row_mean(xd.view(B, D, L))).ravel(), got)
        dy = E.row_mean_data(rows, 1, "gauss")[:, 0]
        dyd = dev(dy)
        out = Guarded(rows * L)
        call("alvq_row_mean_backward_f32", dyd.data_ptr(), out.ptr, rows, L)
        dx = out.get().reshape(rows, L)
        d = E.ulp_distance(dx, E.row_mean_backward(dy, L).astype(np.float32))
        assert d.max() <= E.ROW_MEAN_BACKWARD_ULPS and (dx == dx[:, :1]).all()
        assert same_bits(host(N.row_mean(dyd.view(B, D, 1), backward_of=L)).ravel(), dx.ravel())


# ---------------------------------------------------------------------------------------------------- bit-exact ops
@pytest.mark.parametrize("B", [1, 3])
def test_transpose12(B):
    for R in E.TRANSPOSE_DIMS:
        for C in E.TRANSPOSE_DIMS:
            x = np.random.RandomState(R * 100 + C).randn(B, R, C).astype(np.float32)
            xd = dev(x)
            out = Guarded(x.size)
            call("alvq_transpose_f32", xd.data_ptr(), out.ptr, B, R, C)
            assert same_bits(out.get().reshape(B, C, R), E.transpose12(x)), (B, R, C)
    assert same_bits(host(N.transpose12(xd)), E.transpose12(x))


def jitter_sources(L):
    idx = np.arange(L)
    left = np.where(idx > 0, idx - 1, min(1, L - 1))
    right = np.where(idx < L - 1, idx + 1, max(L - 2, 0))
    out = [("identity", idx), ("left", left), ("right", right)]
    if L >= 2:                                         # (the draw for L = 1 may name column 1, which does not exist)
        np.random.seed(L)
        out.append(("oracle", O.jitter_source_index(L, 0.25)))
    return [(k, s.astype(np.int32)) for k, s in out]


@pytest.mark.parametrize("L", E.JITTER_L)
def test_jitter_gather(L):
    for kind, src in jitter_sources(L):
        assert src.min() >= 0 and src.max() < L
        # 15 rows; with the oracle's draw at L = 300 also 7000 rows: rows * L is past the capped grid
        for rows in (15, 7000) if (kind == "oracle" and L == 300) else (15,):
            assert rows == 15 or rows * L > 2048 * 1024
            x = np.random.RandomState(L + rows).randn(rows, L).astype(np.float32)
            xd, sd = dev(x), dev(src)
            for backward in (0, 1):
                out = Guarded(x.size)
                call("alvq_jitter_gather_f32", xd.data_ptr(), sd.data_ptr(), out.ptr, rows, L, backward)
                assert same_bits(out.get().reshape(rows, L), E.jitter(x, src, backward)), (kind, rows, backward)
    x3 = xd.view(5, rows // 5, L)
    assert same_bits(host(N.jitter_gather(x3, sd)).reshape(rows, L), E.jitter(x, src, False))
    assert same_bits(host(N.jitter_gather(x3, sd, backward=True)).reshape(rows, L), E.jitter(x, src, True))


@pytest.mark.parametrize("n", E.FLAT_N)
def test_add_and_relu_mask(n):
    rs = np.random.RandomState(n % 1000)
    a, b = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    t = np.where(rs.rand(n) < 0.1, 0.0, rs.randn(n)).astype(np.float32)
    ad, bd, td = dev(a), dev(b), dev(t)
    out = Guarded(n)
    call("alvq_add_f32", ad.data_ptr(), bd.data_ptr(), out.ptr, n)
    assert same_bits(out.get(), E.add(a, b))
    out = Guarded(n)
    call("alvq_relu_mask_f32", ad.data_ptr(), td.data_ptr(), out.ptr, n)
    assert same_bits(out.get(), E.relu_mask(a, t))
    if n <= 257:
        assert same_bits(host(N.add(ad, bd)), E.add(a, b)) and same_bits(host(N.relu_mask(ad, td)), E.relu_mask(a, t))


def test_relu_mask_specials():
    """t > 0 ? dy : 0 -- where t <= 0 (or NaN) the output is +0 whatever dy holds, NaN and inf included."""
    t = np.array([0.0, -0.0, 1e-45, -1e-45, np.inf, -np.inf, np.nan, 2.0, -2.0, 0.0, -0.0, np.nan, -np.inf], np.float32)
    dy = np.array([np.nan, np.inf, 5.0, np.nan, np.nan, np.inf, np.inf, -0.0, np.nan, -np.inf, 7.0, np.nan, -np.inf], np.float32)
    got = host(N.relu_mask(dev(dy), dev(t)))
    want = E.relu_mask(dy, t)
    assert same_bits(got, want)
    off = ~(t > 0)
    assert not E.bits(got)[off].any() and off.sum() == 10                      # +0, not -0, not NaN
    assert same_bits(got[[2, 4, 7]], dy[[2, 4, 7]])                            # a denormal t is > 0; dy passes with its bits (NaN, -0)


@pytest.mark.parametrize("value", E.FILL_VALUES, ids=["+0", "-0", "1.5"])
def test_fill(value):
    for n in E.FILL_N:
        out = Guarded(n)
        call("alvq_fill_f32", out.ptr, value, n)
        got = out.get()                                                        # canaries on both sides
        assert (E.bits(got) == E.bits(np.float32(value))).all(), n             # -0.0 arrives with its sign
    t = torch.full((1025,), 7.0, device=DEV)
    assert N.fill_(t, value) is t and (E.bits(host(t)) == E.bits(np.float32(value))).all()


# ------------------------------------------------------------------------------------------------------------- Adam
HP = (E.ADAM_LR, E.ADAM_BETA1, E.ADAM_BETA2, E.ADAM_EPS, E.ADAM_GSCALE)


def device_adam(form, p, g, m, v, t, scalars=None, gscale=E.ADAM_GSCALE):
    """One step through ``form`` on guarded copies -> (p, m, v) on the host.  adam_dev reads ``scalars`` (a device tensor)."""
    lr, b1, b2, eps, _ = HP
    n = p.size
    P, M, V = Guarded(n, p), Guarded(n, m), Guarded(n, v)
    gd = dev(g)
    if form == "adam_f32":
        call("alvq_adam_f32", P.ptr, gd.data_ptr(), M.ptr, V.ptr, n, t, lr, b1, b2, eps, gscale)
    else:
        call("alvq_adam_dev_f32", P.ptr, gd.data_ptr(), M.ptr, V.ptr, n, scalars.data_ptr(), b1, b2, eps, None)
    return P.get(), M.get(), V.get()


def check_adam(tag, got, p, g, m, v, t, gscale=E.ADAM_GSCALE):
    lr, b1, b2, eps, _ = HP
    pr, mr, vr, bp, bm, bv = E.adam_bounds(p, g, m, v, t, lr, b1, b2, eps, gscale)
    worst = []
    for name, x, ref, bound in (("p", got[0], pr, bp), ("m", got[1], mr, bm), ("v", got[2], vr, bv)):
        err = np.abs(x.astype(np.float64) - ref)
        worst.append(float((err / bound).max()))
        assert (err <= bound).all(), (tag, name, worst[-1])
    print("%s: p, m, v at %.3f, %.3f, %.3f of their bounds" % (tag, *worst))


@pytest.mark.parametrize("form", ["adam_f32", "adam_dev"])
def test_adam_three_steps_against_float64(form):
    """From non-zero m, v; every step is held against the restatement applied to the fp32 state it started from."""
    lr, b1, b2, eps, gs = HP
    p, _, m, v = E.adam_data(1025)
    scalars = torch.zeros(N.ADAM_SCALARS, device=DEV)
    for t in (1, 2, 3):
        g = E.adam_data(1025, seed=10 + t)[1]
        if form == "adam_dev":
            N.adam_advance(scalars, lr, b1, b2, gs)
        got = device_adam(form, p, g, m, v, t, scalars)
        check_adam("%s step %d" % (form, t), got, p, g, m, v, t)
        assert not same_bits(got[0], p)
        p, m, v = got
    if form == "adam_dev":
        assert float(scalars[3]) == 3.0 and float(scalars[4]) == 0.0


def torch_adam_second_step(p, g, m, v, gscale):
    """torch.optim.Adam in float32 on the CPU: its step 2 from planted p, m, v, grad_scale folded into the gradient."""
    ref = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=E.ADAM_LR, betas=(E.ADAM_BETA1, E.ADAM_BETA2), eps=E.ADAM_EPS)
    ref.grad = torch.from_numpy(g * np.float32(gscale))
    opt.step()
    st = opt.state[ref]
    with torch.no_grad():
        ref.copy_(torch.from_numpy(p))
        st["exp_avg"].copy_(torch.from_numpy(m))
        st["exp_avg_sq"].copy_(torch.from_numpy(v))
    opt.step()
    return ref.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("form", ["adam_f32", "adam_dev"])
def test_adam_specials(form):
    lr, b1, b2, eps, gs = HP
    sc2 = dev(E.host_scalars(2))
    p, g, m, v = E.adam_data(1025, seed=3)
    # g = 0 from m = v = 0: nothing moves
    z = np.zeros_like(p)
    got = device_adam(form, p, z, z, z, 2, sc2)
    assert same_bits(got[0], p) and not E.bits(got[1]).any() and not E.bits(got[2]).any()
    # |g| = 1e20: (1 - beta2) gr gr is evaluated left to right, as torch's addcmul_ does: no overflow, v' ~ 6e35, an ordinary step
    big = np.where(g > 0, 1e20, -1e20).astype(np.float32)
    got = device_adam(form, p, big, m, v, 2, sc2)
    check_adam("%s |g|=1e20" % form, got, p, big, m, v, 2)
    tp, tm, tv = torch_adam_second_step(p, big, m, v, gs)
    check_adam("torch |g|=1e20", (tp, tm, tv), p, big, m, v, 2)
    assert np.isfinite(got[2]).all() and np.isfinite(tv).all() and not same_bits(got[0], p)
    # |g| = 1e25: now it overflows: v' = inf, denom = inf, m' / denom = 0: p keeps its bits; torch in float32 does the same
    huge = np.where(g > 0, 1e25, -1e25).astype(np.float32)
    got = device_adam(form, p, huge, m, v, 2, sc2)
    tp, tm, tv = torch_adam_second_step(p, huge, m, v, gs)
    assert np.isposinf(got[2]).all() and np.isposinf(tv).all()
    assert same_bits(got[0], p) and same_bits(tp, p)
    mr = E.adam(p, huge, m, v, 2, lr, b1, b2, eps, gs)[1]
    assert (np.abs(got[1] - mr) <= 6 * E.U * np.abs(huge) * gs).all() and np.isfinite(got[1]).all()
    # a denormal g (and, on every other element, from m = v = 0: m' is a denormal, v' underflows to 0, denom = eps)
    tiny = np.where(g > 0, 1e-40, -3e-42).astype(np.float32)
    m2, v2 = m.copy(), v.copy()
    m2[::2], v2[::2] = 0, 0
    got = device_adam(form, p, tiny, m2, v2, 2, sc2)
    check_adam("%s denormal g" % form, got, p, tiny, m2, v2, 2)
    assert not got[2][::2].any()


@pytest.mark.parametrize("n", E.ADAM_N)
def test_adam_sizes(n):
    p, g, m, v = E.adam_data(n)
    sc = dev(E.host_scalars(2))
    a = device_adam("adam_f32", p, g, m, v, 2)
    check_adam("adam_f32 n=%d" % n, a, p, g, m, v, 2)
    b = device_adam("adam_dev", p, g, m, v, 2, sc)
    assert all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("betas", E.ADVANCE_BETAS, ids=str)
def test_adam_advance_scalars(betas):
    lr, gs = 1e-3, 0.5
    scalars = torch.zeros(N.ADAM_SCALARS, device=DEV)
    for t in range(1, 7):
        N.adam_advance(scalars, lr, betas[0], betas[1], gs)
        got = host(scalars)
        want = np.array(E.adam_scalars(t, lr, betas[0], betas[1], gs)).astype(np.float32)
        d = E.ulp_distance(got[:4], want)
        print("adam_advance t=%d betas=%s: %s ulp" % (t, betas, d.tolist()))
        assert d[0] <= 1 and d[1] <= 1 and got[2] == np.float32(gs) and got[3] == t and not got[4:].any()


def all_forms(shape, t=2):
    """The four forms on the same p, g, m, v -> [(p, m, v)] on the host."""
    lr, b1, b2, eps, gs = HP
    n = int(np.prod(shape))
    p, g, m, v = E.adam_data(n, seed=n)
    sc = dev(E.host_scalars(t))
    out = [device_adam("adam_f32", p, g, m, v, t), device_adam("adam_dev", p, g, m, v, t, sc)]
    for form in ("segments", "pack"):
        pd, gd, md, vd = dev(p), dev(g), dev(m), dev(v)
        if form == "segments":
            N.adam_segments(pd, gd, md, vd, [(0, n)], sc, b1, b2, eps)
        else:
            N.adam_pack_batch([(pd.view(shape), gd.view(shape), md.view(shape), vd.view(shape), None, None)], 1, sc, b1, b2, eps)
        out.append((host(pd), host(md), host(vd)))
    return out


@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 68, 3), (3, 66, 1), (40, 200, 3)], ids=str)
def test_the_four_adam_forms_agree_bit_for_bit(shape):
    forms = all_forms(shape)
    for other, name in zip(forms[1:], ("adam_dev", "adam_segments", "adam_pack_batch")):
        for x, y, what in zip(forms[0], other, "pmv"):
            assert same_bits(x, y), (name, what, int((E.bits(x) != E.bits(y)).sum()))


def test_adam_segments_chunks_lengths_and_gaps():
    lr, b1, b2, eps, gs = HP
    segs, size = E.segments()
    p, g, m, v = E.adam_data(size)
    sc = dev(E.host_scalars(3))
    inside = np.zeros(size, bool)
    for lo, hi in segs:
        assert not inside[lo:hi].any()
        inside[lo:hi] = True
    pr, mr, vr, gd = dev(p), dev(m), dev(v), dev(g)
    for lo, hi in segs:                                     # the single-tensor kernel, segment by segment
        N.adam_step_dev(pr[lo:hi], gd[lo:hi], mr[lo:hi], vr[lo:hi], sc, b1, b2, eps)
    pd, md, vd = dev(p), dev(m), dev(v)
    N.adam_segments(pd, gd, md, vd, segs, sc, b1, b2, eps)
    for got, ref, before, what in ((pd, pr, p, "p"), (md, mr, m, "m"), (vd, vr, v, "v")):
        got, ref = host(got), host(ref)
        assert same_bits(got[inside], ref[inside]), what
        assert same_bits(got[~inside], before[~inside]), what                  # gaps of 1 and 64, the head, the tail
        assert (E.bits(got[inside]) != E.bits(before[inside])).mean() > 0.9
        for lo, hi in segs:                                                    # each segment's last element and the one after it
            assert E.bits(got[hi - 1]) == E.bits(ref[hi - 1])
            assert inside[hi] or E.bits(got[hi]) == E.bits(before[hi])


def image_geometry(M, C, KW):
    n = N.lib().alvq_packed_weight_elems(M, C, KW)
    Cp = (C + 63) // 64 * 64
    assert n % (KW * Cp) == 0
    return n, n // (KW * Cp), Cp


def pack_setup(planes, seed=0):
    """The 26 descriptors in flat buffers (every tensor on a 256-byte boundary, canaries between), their images packed in full
    from the weights and then poisoned outside each weight's 32 x 64-rounded extent."""
    descs = E.pack_descs()
    at, offs = E.PACK_ALIGN, []
    for d0, d1, KW, _ in descs:
        offs.append(at)
        at += (d0 * d1 * KW + E.PACK_ALIGN - 1) // E.PACK_ALIGN * E.PACK_ALIGN + E.PACK_ALIGN
    p, g, m, v = E.adam_data(at, seed=seed)
    flat = [dev(a) for a in (p, g, m, v)]
    assert all(f.data_ptr() % 256 == 0 for f in flat)
    entries, images = [], []
    for (d0, d1, KW, which), o in zip(descs, offs):
        w, gg, mm, vv = (f[o:o + d0 * d1 * KW].view(d0, d1, KW) for f in flat)
        imgs = {}
        for layout, name in ((N.W_OIK, "oik"), (N.W_IOK, "iok")):
            if which in (name, "both"):
                img, _ = N.pack_weight(w, layout, planes)
                Mi, Ci = (d0, d1) if layout == N.W_OIK else (d1, d0)
                n, Mp, Cp = image_geometry(Mi, Ci, KW)
                rows = (d0 + 31) // 32 * 32 if layout == N.W_OIK else (d1 + 63) // 64 * 64      # the tiles' extent in the image
                cols = (d1 + 63) // 64 * 64 if layout == N.W_OIK else (d0 + 31) // 32 * 32
                assert rows <= Mp and cols <= Cp and img.numel() == min(planes, 2) * n
                mask = torch.zeros((min(planes, 2), KW, Mp, Cp), dtype=torch.bool, device=DEV)
                mask[:, :, :rows, :cols] = True
                mask = mask.view(-1)
                bits16 = img.view(torch.int16)
                bits16[~mask] = 0x7FC1                                         # poison what the fused kernel must not touch
                imgs[name] = (img, mask, layout)
        entries.append((w, gg, mm, vv, imgs["oik"][0] if "oik" in imgs else None, imgs["iok"][0] if "iok" in imgs else None))
        images.append(imgs)
    return descs, offs, (p, g, m, v), flat, entries, images


@pytest.mark.parametrize("planes", [1, 2, 3])
def test_adam_pack_batch(planes):
    lr, b1, b2, eps, gs = HP
    descs, offs, before, flat, entries, images = pack_setup(planes)
    sc = dev(E.host_scalars(2))
    ref = [dev(a) for a in before]
    for (d0, d1, KW, _), o in zip(descs, offs):             # adam_dev, tensor by tensor
        n = d0 * d1 * KW
        N.adam_step_dev(ref[0][o:o + n], ref[1][o:o + n], ref[2][o:o + n], ref[3][o:o + n], sc, b1, b2, eps)
    prefill = [{k: im[0].clone() for k, im in imgs.items()} for imgs in images]
    N.adam_pack_batch(entries, planes, sc, b1, b2, eps)
    torch.cuda.synchronize()
    for i in (0, 2, 3):                                     # w, m, v: adam_dev's bits, the canaries between the tensors included
        assert torch.equal(flat[i].view(torch.int32), ref[i].view(torch.int32)), i
    assert torch.equal(flat[1].view(torch.int32), dev(before[1]).view(torch.int32))
    assert not torch.equal(flat[0].view(torch.int32), dev(before[0]).view(torch.int32))
    for (d0, d1, KW, which), o, imgs, pre in zip(descs, offs, images, prefill):
        w_new = ref[0][o:o + d0 * d1 * KW].view(d0, d1, KW)
        for name, (img, mask, layout) in imgs.items():
            want, _ = N.pack_weight(w_new, layout, planes)
            got, want, was = img.view(torch.int16), want.view(torch.int16), pre[name].view(torch.int16)
            assert torch.equal(got[mask], want[mask]), ((d0, d1, KW), name, int((got[mask] != want[mask]).sum()))
            assert torch.equal(got[~mask], was[~mask]) and bool((got[~mask] == 0x7FC1).all()), ((d0, d1, KW), name)
            if d0 * d1 * KW > 1:
                assert not torch.equal(got[mask], was[mask])                   # the image did move with the weight


# ------------------------------------------------------------------------------------------------------------- skip
def test_a_skipped_step_moves_nothing():
    lr, b1, b2, eps, gs = HP
    sc = dev(E.host_scalars(2))
    skip = dev(np.array([1.0], np.float32))
    p, g, m, v = E.adam_data(5000)
    P, M, V = Guarded(5000, p), Guarded(5000, m), Guarded(5000, v)
    gd = dev(g)
    call("alvq_adam_dev_f32", P.ptr, gd.data_ptr(), M.ptr, V.ptr, 5000, sc.data_ptr(), b1, b2, eps, skip.data_ptr())
    assert same_bits(P.get(), p) and same_bits(M.get(), m) and same_bits(V.get(), v)
    segs, size = E.segments()
    p, g, m, v = E.adam_data(size)
    pd, gd, md, vd = dev(p), dev(g), dev(m), dev(v)
    N.adam_segments(pd, gd, md, vd, segs, sc, b1, b2, eps, skip=skip)
    assert same_bits(host(pd), p) and same_bits(host(md), m) and same_bits(host(vd), v)
    for planes in (1, 2, 3):
        descs, offs, before, flat, entries, images = pack_setup(planes, seed=planes)
        prefill = [{k: im[0].clone() for k, im in imgs.items()} for imgs in images]
        N.adam_pack_batch(entries, planes, sc, b1, b2, eps, skip=skip)
        for f, a in zip(flat, before):
            assert same_bits(host(f), a)
        for imgs, pre in zip(images, prefill):
            for name, (img, _, _) in imgs.items():
                assert torch.equal(img.view(torch.int16), pre[name].view(torch.int16))
    # the same launches with the slot at 0 do move things (the slot is what held them)
    skip.zero_()
    N.adam_segments(pd, gd, md, vd, segs, sc, b1, b2, eps, skip=skip)
    assert not same_bits(host(pd), p)


def test_adam_advance_does_not_count_a_skipped_step():
    lr, b1, b2 = 1e-3, 0.9, 0.999
    scalars = torch.zeros(N.ADAM_SCALARS, device=DEV)
    slot = torch.zeros(1, device=DEV)
    N.adam_advance(scalars, lr, b1, b2, 1.0, prev_skip=slot)
    N.adam_advance(scalars, lr, b1, b2, 1.0, prev_skip=slot)
    at2 = host(scalars).copy()
    assert at2[3] == 2.0 and at2[4] == 0.0
    slot.fill_(1.0)
    N.adam_advance(scalars, lr, b1, b2, 1.0, prev_skip=slot)
    got = host(scalars)
    assert got[3] == 2.0 and got[4] == 1.0 and same_bits(got[:3], at2[:3])     # t stays, skipped steps go up, the scalars are step 2's
    slot.zero_()
    N.adam_advance(scalars, lr, b1, b2, 1.0, prev_skip=slot)
    assert host(scalars)[3] == 3.0 and host(scalars)[4] == 1.0


# ---------------------------------------------------------------------------------------------------- embedding bag
def device_bag_fwd(W, bias, idx, L, K):
    B, M = idx.shape[0], W.shape[0]
    flag = N.device_flag(DEV)
    Wd, bd, idd = dev(W), dev(bias), dev(idx)
    out = Guarded(B * M)
    call("alvq_embedding_bag_fwd_f32", Wd.data_ptr(), bd.data_ptr(), idd.data_ptr(), out.ptr, B, L, K, M, flag.data_ptr())
    got = out.get().reshape(B, M)
    assert same_bits(host(N.embedding_bag_fwd(Wd, bd, idd, L, K)), got)
    return got, int(flag.item())


@pytest.mark.parametrize("shape", E.BAG_SHAPES, ids=str)
def test_embedding_bag_lattice_is_exact(shape):
    B, L, K, M = shape
    for bad in (None, -1, "K"):
        W, bias, dz, idx = E.bag_data(shape, "lattice", bad)
        assert B == 1 or (np.array_equal(idx[-1], idx[0]) if bad is None else (idx[-1] != idx[0]).sum() == 1)
        out, _, flag_ref = E.embedding_bag_fwd(W, bias, idx, L, K)
        got, flag = device_bag_fwd(W, bias, idx, L, K)
        assert flag == flag_ref == int(bad is not None)
        assert same_bits(got, out.astype(np.float32)), bad
        dW_ref, db_ref, _, touched, _ = E.embedding_bag_bwd(dz, idx, L, K)
        flag = N.device_flag(DEV)
        dW, db = N.embedding_bag_bwd(dev(dz), dev(idx), L, K, flag=flag)
        assert int(flag.item()) == flag_ref
        assert same_bits(host(dW), dW_ref.astype(np.float32)) and same_bits(host(db), db_ref.astype(np.float32))
        # the accumulate forms: a sentinel pattern in dW and db
        s_W = (1000 + np.arange(M * L * K) % 13).astype(np.float32).reshape(M, L * K)
        s_b = (-500 + np.arange(M) % 7).astype(np.float32)
        dWo, dbo = dev(s_W), dev(s_b)
        r = N.embedding_bag_bwd(dev(dz), dev(idx), L, K, dW_out=dWo, db_out=dbo)
        assert r[0] is dWo and r[1] is dbo
        assert same_bits(host(dWo), (s_W + dW_ref).astype(np.float32)) and same_bits(host(dbo), (s_b + db_ref).astype(np.float32))
        assert same_bits(host(dWo)[:, ~touched], s_W[:, ~touched])


@pytest.mark.parametrize("shape", E.BAG_SHAPES, ids=str)
def test_embedding_bag_gaussian_bounds(shape):
    B, L, K, M = shape
    W, bias, dz, idx = E.bag_data(shape, "gauss")
    out, mag, _ = E.embedding_bag_fwd(W, bias, idx, L, K)
    got, flag = device_bag_fwd(W, bias, idx, L, K)
    err, bound = np.abs(got.astype(np.float64) - out), E.bag_fwd_bound(L, mag)
    assert flag == 0 and (err <= bound).all()
    dW_ref, db_ref, wmag, touched, _ = E.embedding_bag_bwd(dz, idx, L, K)
    s_W = np.random.RandomState(5).randn(M, L * K).astype(np.float32)
    s_b = np.random.RandomState(6).randn(M).astype(np.float32)
    dWo, dbo = dev(s_W), dev(s_b)
    N.embedding_bag_bwd(dev(dz), dev(idx), L, K, dW_out=dWo, db_out=dbo)
    gW, gb = host(dWo), host(dbo)
    errW = np.abs(gW.astype(np.float64) - (s_W.astype(np.float64) + dW_ref))
    boundW = E.bag_bwd_bound(B, np.abs(s_W.astype(np.float64)) + wmag)
    errb = np.abs(gb.astype(np.float64) - (s_b.astype(np.float64) + db_ref))
    boundb = E.bag_bwd_bound(B, np.abs(s_b.astype(np.float64)) + np.abs(dz.astype(np.float64)).sum(0))
    print("bag %s: forward at %.3f of its bound, dW at %.3f, db at %.3f" % (shape, (err / bound).max(), (errW / boundW).max(), (errb / boundb).max()))
    assert (errW <= boundW).all() and (errb <= boundb).all()
    assert same_bits(gW[:, ~touched], s_W[:, ~touched])


@pytest.mark.parametrize("K", E.ONEHOT_K)
def test_onehot_to_index(K):
    rows = 7                                                 # rows % 4 != 0: a partial workgroup
    pos = np.random.RandomState(K).randint(0, K, rows)
    pos[0], pos[-1] = K - 1, 0
    enc = np.zeros((rows, K), np.float32)
    enc[np.arange(rows), pos] = 1.0
    beside = (pos + 1) % K                                   # another column of each row (K > 1)

    def check(e, flagged):
        ridx, rflag = E.onehot_to_index(e)
        idx, flag = N.onehot_to_index(dev(e))
        idx, flag = host(idx), int(flag.item())
        assert flag == rflag == int(flagged) and np.array_equal(idx, ridx)
        return idx
    assert np.array_equal(check(enc, False), pos)
    e = enc.copy()
    e[rows - 1] = 0.0                                        # an all-zero row (the last, in the partial workgroup): flag, index 0
    assert check(e, True)[rows - 1] == 0
    e = enc.copy()
    e[3, pos[3]] = 0.5                                       # one non-zero that is not 1
    check(e, True)
    e = enc.copy()
    e[1, pos[1] if K == 1 else beside[1]] = np.nan           # a NaN entry
    check(e, True)
    if K > 1:
        e = enc.copy()
        e[2, beside[2]] = e[rows - 1, beside[rows - 1]] = -0.0    # a single -0.0 elsewhere in a good row: still one-hot
        assert np.signbit(e).sum() == 2 and np.array_equal(check(e, False), pos)
        e = enc.copy()
        e[3, beside[3]] = 1.0                                # two ones
        check(e, True)
    if K > 64:                                               # two ones landing in the same lane: k and k + 64
        e = enc.copy()
        k = int(min(pos[4], K - 65))
        e[4] = 0.0
        e[4, k] = e[4, k + 64] = 1.0
        assert check(e, True)[4] == k + 64
