"""tests/helpers/elementwise_ref.py without a GPU:

* every float64 restatement against an independent implementation in float64 (torch.std, F.mse_loss and autograd,
  torch.optim.Adam, x.mean(-1) and autograd, a dense one-hot product);
* every tolerance of the module against a numpy-float32 emulation of the kernel in its documented summation order, on the
  very arrays tests/test_elementwise_edges_gpu.py feeds the device: a bound that is too tight fails here, not on the GPU,
  and none is taken from a device run;
* every argument check of the entry points under test, through the library with fake non-null pointers: each must refuse
  before anything is launched (nothing is dereferenced on the host; no GPU is present)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import elementwise_ref as E  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ------------------------------------------------------------------------------------- restatements, independently
@pytest.mark.parametrize("take_abs", [False, True])
def test_standardise_restatement_equals_torch_std(take_abs):
    for B, C, L in ((2, 2, 3), (1, 5, 7), (3, 257, 4)):
        x, _ = E.standardise_data(B, C, L, "offset100" if C == 5 else "gauss")
        y, mean, std = E.standardise(x, take_abs)
        v = t64(x).abs() if take_abs else t64(x)
        want = (v - v.mean(1, keepdim=True)) / (torch.std(v, dim=1, keepdim=True, unbiased=True) + 1e-8)
        assert np.abs(y - want.numpy()).max() <= 1e-12 * np.abs(y).max()
        assert np.abs(std - torch.std(v, dim=1, keepdim=True, unbiased=True).numpy()).max() <= 1e-13 * std.max()


def test_mse_restatement_equals_mse_loss_and_its_gradient():
    for n in (1, 257, 5003):
        a, b = E.mse_data(n, "gauss")
        ta = t64(a).requires_grad_(True)
        loss = F.mse_loss(ta, t64(b))
        assert abs(E.mse(a, b) - float(loss.detach())) <= 1e-14 * float(loss.detach())
        for gl in E.GRAD_LOSS:
            ta.grad = None
            (loss * float(np.float32(gl))).backward(retain_graph=True)
            want = ta.grad.numpy()
            assert np.abs(E.mse_backward(a, b, gl) - want).max() <= 1e-14 * np.abs(want).max()


def test_row_mean_restatement_equals_mean_and_its_gradient():
    x = E.row_mean_data(5, 65, "gauss")
    tx = t64(x).requires_grad_(True)
    y = tx.mean(-1)
    assert np.abs(E.row_mean(x) - y.detach().numpy()).max() <= 1e-15
    dy = np.random.RandomState(0).randn(5)
    y.backward(t64(dy))
    assert np.abs(E.row_mean_backward(dy, 65) - tx.grad.numpy()).max() <= 1e-16


def test_adam_restatement_equals_torch_adam_in_float64():
    lr, b1, b2, eps, gs = E.ADAM_LR, E.ADAM_BETA1, E.ADAM_BETA2, E.ADAM_EPS, E.ADAM_GSCALE
    p0, _, _, _ = E.adam_data(1025)
    ref = t64(p0).clone().requires_grad_(True)
    # the kernel receives beta1, beta2, eps as fp32; these betas are fp32 values, eps is handed to torch as the kernel sees it
    opt = torch.optim.Adam([ref], lr=lr, betas=(b1, b2), eps=float(np.float32(eps)))
    p, m, v = p0.astype(np.float64), np.zeros(1025), np.zeros(1025)
    for t in range(1, 6):
        g = E.adam_data(1025, seed=t)[1]
        ref.grad = t64(g) * gs                                     # grad_scale folded into the gradient
        opt.step()
        p, m, v, _ = E.adam(p, g, m, v, t, lr, b1, b2, eps, gs)
        assert np.abs(p - ref.detach().numpy()).max() <= 1e-13
    st = opt.state[ref]
    assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-13 and np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-13
    s = E.adam_scalars(3, 1e-3, 0.9, 0.999, 0.5)
    assert s == (1e-3 / (1 - 0.9 ** 3), (1 - 0.999 ** 3) ** 0.5, 0.5, 3.0)
    # exact powers: the fp32 scalars of alvq_adam_f32 (from fp32 arguments) are the ones adam_advance derives from the doubles
    assert float(np.float32(lr)) == lr and float(np.float32(b1)) == b1 and float(np.float32(b2)) == b2


@pytest.mark.parametrize("shape", [s for s in E.BAG_SHAPES if s[0] * s[1] <= 1000], ids=str)
def test_bag_restatement_equals_a_dense_one_hot_product(shape):
    B, L, K, M = shape
    for bad in (None, -1, "K"):
        W, bias, dz, idx = E.bag_data(shape, "gauss", bad)
        ok = (idx >= 0) & (idx < K)
        onehot = np.zeros((B, L * K))
        for b in range(B):
            for l in range(L):
                if ok[b, l]:
                    onehot[b, l * K + idx[b, l]] = 1.0
        tw = t64(W).requires_grad_(True)
        tb = t64(bias).requires_grad_(True)
        out = F.linear(t64(onehot), tw, tb)
        got, mag, flag = E.embedding_bag_fwd(W, bias, idx, L, K)
        assert flag == int(bad is not None)
        assert np.abs(got - out.detach().numpy()).max() <= 1e-13 * max(1.0, np.abs(got).max())
        assert (mag >= np.abs(got) - 1e-12).all()
        out.backward(t64(dz))
        dW, db, _, touched, flag = E.embedding_bag_bwd(dz, idx, L, K)
        assert flag == int(bad is not None)
        assert np.abs(dW - tw.grad.numpy()).max() <= 1e-13 and np.abs(db - tb.grad.numpy()).max() <= 1e-13
        assert np.array_equal(touched, onehot.any(0))
        enc = onehot.reshape(B * L, K).astype(np.float32)
        pos, nflag = E.onehot_to_index(enc)
        assert np.array_equal(pos[ok.ravel()], idx.ravel()[ok.ravel()]) and nflag == int(bad is not None)
        assert not pos[~ok.ravel()].any()


def test_bit_exact_restatements():
    x = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    src = np.array([1, 1, 3, 2])
    assert np.array_equal(E.jitter(x, src, False), torch.from_numpy(x)[:, :, torch.from_numpy(src)].numpy())
    assert np.array_equal(E.jitter(x, src, True)[0, 0], [0, 1, 0, 0])
    assert np.array_equal(E.transpose12(x), torch.from_numpy(x).permute(0, 2, 1).contiguous().numpy())
    t = np.array([0.0, -0.0, 1e-45, np.inf, -np.inf, np.nan, 2.0], np.float32)
    dy = np.array([np.nan, np.inf, 5.0, 6.0, np.nan, np.inf, 7.0], np.float32)
    assert np.array_equal(E.bits(E.relu_mask(dy, t)), E.bits(np.array([0, 0, 5, 6, 0, 0, 7], np.float32)))
    assert E.ulp(1.0) == 2.0 ** -23 and E.ulp(0.0) == 2.0 ** -149 and E.ulp(3.0) == 2.0 ** -22


# ------------------------------------------------------------------------ the bounds hold for the emulated kernels
@pytest.mark.parametrize("case", E.STD_CASES, ids=str)
def test_standardise_bound_holds_for_the_emulation(case):
    B, C, L = case
    worst = 0.0
    for kind in E.STD_DATA:
        for take_abs in (False, True):
            x, const = E.standardise_data(B, C, L, kind, take_abs)
            ref, mean, std = E.standardise(x, take_abs)
            y = E.emulate_standardise(x, take_abs)
            free = ~const
            xmax = np.abs(x).max(1, keepdims=True)
            assert E.standardise_precondition(C, xmax[free[:, None]].max(), std[free[:, None]].min())
            ratio = (np.abs(mean) / np.maximum(std, 1e-300))[free[:, None]]
            assert ratio.max() <= 100.0 * (1 + 1e-5) and (kind != "offset100" or ratio.min() >= 99.0)
            bound = E.standardise_bound(C, xmax, std, ref)
            err = np.abs(y - ref)
            sel = np.broadcast_to(free[:, None], x.shape)
            assert (err[sel] <= bound[sel]).all(), (kind, take_abs, (err / bound)[sel].max())
            worst = max(worst, float((err / bound)[sel].max()))
            if const.any():                                       # exactly +0, finite: the + 1e-8 path
                cs = np.broadcast_to(const[:, None], x.shape)
                assert not E.bits(y)[cs].any() and not ref[cs].any() and not std[const[:, None]].any()
    print("standardise %s: emulation at %.3f of the bound" % (case, worst))


@pytest.mark.parametrize("n", E.MSE_N)
def test_mse_bounds_hold_for_the_emulation(n):
    a, b = E.mse_data(n, "lattice")
    S = ((a.astype(np.float64) - b) ** 2).sum()
    assert S == int(S) and n * float(np.abs(a - b).max()) ** 2 < 2 ** 24
    assert E.bits(E.emulate_mse(a, b)) == E.bits(np.float32(S / n))
    a, b = E.mse_data(n, "gauss")
    ref = E.mse(a, b)
    got = float(E.emulate_mse(a, b))
    print("mse n=%d: emulation rel. error %.3g, bound %.3g" % (n, abs(got - ref) / ref, E.mse_bound(n)))
    assert abs(got - ref) <= E.mse_bound(n) * ref
    assert E.emulate_mse(a, a) == 0.0


@pytest.mark.parametrize("n", E.MSE_BACKWARD_N)
def test_mse_backward_bound_holds_for_the_emulation(n):
    a, b = E.mse_data(n, "gauss")
    for gl in E.GRAD_LOSS:
        d = E.ulp_distance(E.emulate_mse_backward(a, b, gl), E.mse_backward(a, b, gl).astype(np.float32))
        assert d.max() <= E.MSE_BACKWARD_ULPS, (gl, d.max())


@pytest.mark.parametrize("L", E.ROW_MEAN_L)
def test_row_mean_bounds_hold_for_the_emulation(L):
    for B, D in E.ROW_MEAN_ROWS:
        rows = B * D
        x = E.row_mean_data(rows, L, "lattice")
        assert np.array_equal(E.bits(E.emulate_row_mean(x)), E.bits((x.astype(np.float64).sum(1) / L).astype(np.float32)))
        x = E.row_mean_data(rows, L, "gauss")
        err = np.abs(E.emulate_row_mean(x) - E.row_mean(x))
        assert (err <= E.row_mean_bound(L, np.abs(x.astype(np.float64)).mean(1))).all()
        dy = E.row_mean_data(rows, 1, "gauss")[:, 0]
        d = E.ulp_distance(E.emulate_row_mean_backward(dy, L), E.row_mean_backward(dy, L).astype(np.float32))
        assert d.max() <= E.ROW_MEAN_BACKWARD_ULPS


def _adam_special(kind):
    p, g, m, v = E.adam_data(1025, seed=3)
    if kind == "zero":
        g[:], m[:], v[:] = 0, 0, 0
    elif kind == "1e20":
        g[:] = np.where(g > 0, 1e20, -1e20)
    elif kind == "denormal":
        g[:] = np.where(g > 0, 1e-40, -3e-42)
        m[::2], v[::2] = 0, 0
    return p, g, m, v


@pytest.mark.parametrize("fma", [False, True])
def test_adam_bounds_hold_for_the_emulation(fma):
    lr, b1, b2, eps, gs = E.ADAM_LR, E.ADAM_BETA1, E.ADAM_BETA2, E.ADAM_EPS, E.ADAM_GSCALE
    for kind in ("gauss", "zero", "1e20", "denormal"):
        p, g, m, v = E.adam_data(1025) if kind == "gauss" else _adam_special(kind)
        worst = [0.0, 0.0, 0.0]
        for t in (1, 2, 3):
            sc = E.host_scalars(t)
            pn, mn, vn = E.emulate_adam(p, g, m, v, sc[0], sc[1], sc[2], b1, b2, eps, fma)
            pr, mr, vr, bp, bm, bv = E.adam_bounds(p, g, m, v, t, lr, b1, b2, eps, gs)
            for i, (got, ref, bound) in enumerate(((pn, pr, bp), (mn, mr, bm), (vn, vr, bv))):
                err = np.abs(got.astype(np.float64) - ref)
                assert (err <= bound).all(), (kind, t, "pmv"[i], (err / bound).max())
                worst[i] = max(worst[i], float((err / bound).max()))
            if kind == "zero":
                assert np.array_equal(E.bits(pn), E.bits(p)) and not mn.any() and not vn.any()
            p, m, v = pn, mn, vn                         # the next step starts from the fp32 values, as on the device
            g = E.adam_data(1025, seed=10 + t)[1] if kind == "gauss" else g
        print("adam %s fma=%s: p, m, v at %.3f, %.3f, %.3f of their bounds" % (kind, fma, *worst))


def test_adam_overflow_is_what_torch_does():
    """(1 - beta2) gr gr is evaluated left to right, in the kernel as in torch's addcmul_: |g| = 1e20 does not overflow (v = 1e37),
    and the step is an ordinary one; |g| = 1e25 does: v = inf, denom = inf, m / denom = 0, p stays bit for bit."""
    for mag, overflows in ((1e20, False), (1e25, True)):
        p, g, m, v = E.adam_data(257, seed=5)
        g[:] = np.where(g > 0, mag, -mag)
        ref = torch.from_numpy(p.copy()).requires_grad_(True)
        opt = torch.optim.Adam([ref], lr=E.ADAM_LR, betas=(E.ADAM_BETA1, E.ADAM_BETA2), eps=E.ADAM_EPS)
        ref.grad = torch.from_numpy(g)
        opt.step()                                        # initialises the state; now plant m, v and take the step under test
        st = opt.state[ref]
        with torch.no_grad():
            ref.copy_(torch.from_numpy(p))
            st["exp_avg"].copy_(torch.from_numpy(m))
            st["exp_avg_sq"].copy_(torch.from_numpy(v))
        opt.step()                                        # torch's step 2
        sc = E.host_scalars(2, grad_scale=1.0)
        pn, mn, vn = E.emulate_adam(p, g, m, v, sc[0], sc[1], 1.0, E.ADAM_BETA1, E.ADAM_BETA2, E.ADAM_EPS)
        tv = st["exp_avg_sq"].numpy()
        assert np.isinf(vn).all() == overflows and np.isinf(tv).all() == overflows and np.isfinite(mn).all()
        if overflows:
            assert np.array_equal(E.bits(pn), E.bits(p)) and np.array_equal(E.bits(ref.detach().numpy()), E.bits(p))
        else:
            pr, mr, vr, bp, bm, bv = E.adam_bounds(p, g, m, v, 2, E.ADAM_LR, E.ADAM_BETA1, E.ADAM_BETA2, E.ADAM_EPS, 1.0)
            assert (np.abs(pn - pr) <= bp).all() and (np.abs(ref.detach().numpy() - pr) <= bp).all()
            assert (np.abs(vn - vr) <= bv).all() and (np.abs(tv - vr) <= bv).all() and (pn != p).all()


@pytest.mark.parametrize("shape", E.BAG_SHAPES, ids=str)
def test_bag_bounds_hold_for_the_emulation(shape):
    B, L, K, M = shape
    assert B * L <= E.BAG_MAX_INDICES
    for kind in ("lattice", "gauss"):
        W, bias, dz, idx = E.bag_data(shape, kind)
        out, mag, _ = E.embedding_bag_fwd(W, bias, idx, L, K)
        got = E.emulate_bag_fwd(W, bias, idx, L, K)
        dW, db, wmag, touched, _ = E.embedding_bag_bwd(dz, idx, L, K)
        gW, gb = E.emulate_bag_bwd(dz, idx, L, K, np.zeros_like(dW, dtype=np.float32))
        if kind == "lattice":
            assert np.abs(dW).max() < 2 ** 24 and np.abs(out).max() < 2 ** 24
            assert np.array_equal(E.bits(got), E.bits(out.astype(np.float32)))
            assert np.array_equal(E.bits(gW), E.bits(dW.astype(np.float32))) and np.array_equal(gb, db.astype(np.float32))
        else:
            assert (np.abs(got - out) <= E.bag_fwd_bound(L, mag)).all()
            assert (np.abs(gW - dW) <= E.bag_bwd_bound(B, wmag)).all()
            assert (np.abs(gb - db) <= E.bag_bwd_bound(B, np.abs(dz.astype(np.float64)).sum(0))).all()


def test_the_grids_reach_every_edge_the_issue_names():
    cs = {c[1] for c in E.STD_CASES}
    assert cs == set(E.STD_C) and all(sum(1 for c in E.STD_CASES if c[1] == C) >= 2 for C in E.STD_C)
    for C in (5, 257):
        assert {c[2] for c in E.STD_CASES if c[1] == C} == set(E.STD_L)
    assert {c[0] for c in E.STD_CASES} == {1, 3}
    assert E.EW_THREADS == 262144 and N.EW_PARTIALS == E.EW_PARTIALS and E.PAST_GRID > 2 * 524288 and E.PAST_CAP > 2048 * 1024
    assert sorted(b * d for b, d in E.ROW_MEAN_ROWS) == [1, 3, 4, 5, 1025]
    segs, size = E.segments()
    assert len(segs) == 50 > 48 and size == 60000 > segs[-1][1] + 5 and {b - a for a, b in segs} == set(E.SEG_LENGTHS)
    gaps = {segs[i + 1][0] - segs[i][1] for i in range(49)}
    assert gaps == {0, 1, 64} and segs[0][0] > 0
    descs = E.pack_descs()
    assert len(descs) == 26 > 24 and {d[:3] for d in descs} == set(E.PACK_SHAPES)
    assert {d[3] for d in descs if d[:3] == (7, 68, 3)} >= {"oik", "iok"} or {"both"} <= {d[3] for d in descs if d[:3] == (7, 68, 3)}
    assert {d[3] for d in descs} == set(E.PACK_IMAGES)
    assert N.BAG_MAX_INDICES == E.BAG_MAX_INDICES == max(s[0] * s[1] for s in E.BAG_SHAPES)


# -------------------------------------------------------------- argument checks: refused on the host, before any launch
def test_entry_points_refuse_bad_arguments_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    lib = N.lib()
    P = 4096                                   # any non-null, aligned value: nothing is dereferenced
    EINVAL, EUNSUPPORTED = -1, -2

    def refused(name, args, word, code=EINVAL):
        rc = getattr(lib, name)(*args)
        msg = lib.alvq_last_error()
        assert rc == code, (name, args, rc, msg)
        assert msg.startswith(name.encode()) and word in msg, (name, msg)

    refused("alvq_standardise_f32", (P, P, 1, 1, 8, 0, None), b"C must be > 1")
    refused("alvq_standardise_f32", (P, P, 1, 0, 8, 0, None), b"C must be > 1")
    refused("alvq_standardise_f32", (P, P, 0, 5, 8, 0, None), b"bad dims")
    refused("alvq_standardise_f32", (P, P, 1, 5, 0, 1, None), b"bad dims")
    refused("alvq_standardise_f32", (None, P, 1, 5, 8, 0, None), b"null")
    for name, nptr in (("alvq_mse_f32", 4), ("alvq_mse_backward_f32", 4), ("alvq_add_f32", 3), ("alvq_relu_mask_f32", 3)):
        for n in (0, -1):
            refused(name, (P,) * nptr + (n, None), b"n <= 0")
        refused(name, (None,) + (P,) * (nptr - 1) + (4, None), b"null")
    refused("alvq_mse_backward_f32", (P, P, P, None, 4, None), b"null")          # grad_loss may be null, grad may not
    for n in (0, -1):
        refused("alvq_fill_f32", (P, 0.0, n, None), b"n <= 0")
    for off in (4, 8, 12):
        refused("alvq_fill_f32", (P + off, 0.0, 8, None), b"16-byte aligned")
    refused("alvq_fill_f32", (None, 0.0, 8, None), b"null")
    refused("alvq_jitter_gather_f32", (P, P, P, 0, 5, 0, None), b"bad dims")
    refused("alvq_jitter_gather_f32", (P, P, P, 5, 0, 1, None), b"bad dims")
    refused("alvq_jitter_gather_f32", (P, None, P, 5, 5, 1, None), b"null")
    for name in ("alvq_row_mean_f32", "alvq_row_mean_backward_f32"):
        refused(name, (P, P, 0, 5, None), b"bad dims")
        refused(name, (P, P, 5, 0, None), b"bad dims")
        refused(name, (P, None, 5, 5, None), b"null")
    refused("alvq_row_mean_f32", (P, P, 1 << 33, 5, None), b"too many rows", EUNSUPPORTED)
    for dims in ((0, 3, 3), (3, 0, 3), (3, 3, 0)):
        refused("alvq_transpose_f32", (P, P) + dims + (None,), b"bad dims")
    refused("alvq_transpose_f32", (P, P, 1 << 20, 1 << 20, 1 << 20, None), b"too large", EUNSUPPORTED)

    hp = (1e-3, 0.9, 0.999, 1e-8)
    refused("alvq_adam_f32", (P, P, P, P, 8, 0, *hp, 1.0, None), b"bad n/step")            # step < 1
    refused("alvq_adam_f32", (P, P, P, P, 8, -3, *hp, 1.0, None), b"bad n/step")
    refused("alvq_adam_f32", (P, P, P, P, 0, 1, *hp, 1.0, None), b"bad n/step")
    refused("alvq_adam_f32", (P, P, None, P, 8, 1, *hp, 1.0, None), b"null")
    refused("alvq_adam_dev_f32", (P, P, P, P, 0, P, *hp[1:], None, None), b"n <= 0")
    refused("alvq_adam_dev_f32", (P, P, P, P, 8, None, *hp[1:], None, None), b"null")
    refused("alvq_adam_advance_f32", (None, 1e-3, 0.9, 0.999, 1.0, None, None), b"null")

    def i64(*v):
        return (ctypes.c_int64 * len(v))(*v)

    def seg(lo, hi, n=None, p=P, sc=P):
        return (p, P, P, P, lo, hi, len(lo) if n is None else n, sc, *hp[1:], None, None)
    refused("alvq_adam_segments_f32", seg(i64(0, 8), i64(4, 8)), b"bad segment 1")        # hi <= lo
    refused("alvq_adam_segments_f32", seg(i64(5), i64(4)), b"bad segment 0")
    refused("alvq_adam_segments_f32", seg(i64(-1), i64(4)), b"bad segment 0")
    lo = list(range(0, 100, 2))
    hi = [a + 1 for a in lo]
    hi[49] = lo[49]                                        # in the SECOND chunk: still refused before the first launch
    refused("alvq_adam_segments_f32", seg(i64(*lo), i64(*hi)), b"bad segment 49")
    refused("alvq_adam_segments_f32", seg(i64(0), i64(4), n=0), b"no segments")
    refused("alvq_adam_segments_f32", seg(i64(0), i64(4), p=None), b"null")
    refused("alvq_adam_segments_f32", seg(i64(0), i64(4), sc=None), b"null")

    def adam_descs(*rows):
        arr = (N.AdamPackDesc * len(rows))()
        for d, r in zip(arr, rows):
            d.w, d.g, d.m, d.v, d.wp_oik, d.wp_iok, d.dim0, d.dim1, d.KW = r
        return arr, (ctypes.addressof(arr), len(rows))
    good = (P, P, P, P, P, None, 4, 4, 3)

    def with_(i, val):
        return good[:i] + (val,) + good[i + 1:]
    tail = (P, *hp[1:], None, None)
    for planes in (0, 4, -1):
        keep, a = adam_descs(good)
        refused("alvq_adam_pack_batch", a + (planes,) + tail, b"planes")
    for KW in (0, 2, 4):
        keep, a = adam_descs(good, with_(8, KW))
        refused("alvq_adam_pack_batch", a + (1,) + tail, b"bad dims in descriptor 1")
    for i in (6, 7):
        keep, a = adam_descs(with_(i, 0))
        refused("alvq_adam_pack_batch", a + (2,) + tail, b"bad dims in descriptor 0")
    keep, a = adam_descs(good, good, with_(2, None))
    refused("alvq_adam_pack_batch", a + (1,) + tail, b"null pointer in descriptor 2")
    keep, a = adam_descs(good)
    refused("alvq_adam_pack_batch", a + (1, None) + tail[1:], b"scalars")
    refused("alvq_adam_pack_batch", (None, 1, 1) + tail, b"no descriptors")
    refused("alvq_adam_pack_batch", (a[0], 0, 1) + tail, b"no descriptors")
    # the alignment precondition: w, g, m, v and the images are moved in 16-byte vectors
    for i in range(6):
        for off in (4, 8):
            keep, a = adam_descs(good, with_(i, P + off))
            refused("alvq_adam_pack_batch", a + (1,) + tail, b"misaligned")
            assert b"descriptor 1" in lib.alvq_last_error()
    rows = [good] * 25 + [with_(0, P + 4)]                 # in the SECOND chunk: still refused before the first launch
    keep, a = adam_descs(*rows)
    refused("alvq_adam_pack_batch", a + (3,) + tail, b"descriptor 25")

    def pack_descs(*rows):
        arr = (N.PackDesc * len(rows))()
        for d, r in zip(arr, rows):
            d.w, d.wp, d.M, d.C, d.KW, d.w_layout = r
        return arr, (ctypes.addressof(arr), len(rows))
    pgood = (P, P, 4, 4, 3, N.W_OIK)
    for planes in (0, 4):
        keep, a = pack_descs(pgood)
        refused("alvq_pack_weights_bf16_batch", a + (planes, None), b"planes")
    for KW in (0, 2, 5):
        keep, a = pack_descs(pgood, pgood[:4] + (KW, N.W_IOK))
        refused("alvq_pack_weights_bf16_batch", a + (1, None), b"bad dims in descriptor 1")
    keep, a = pack_descs(pgood[:5] + (2,))
    refused("alvq_pack_weights_bf16_batch", a + (1, None), b"w_layout in descriptor 0")
    keep, a = pack_descs(pgood, (P, None) + pgood[2:])
    refused("alvq_pack_weights_bf16_batch", a + (1, None), b"null pointer in descriptor 1")
    for off in (2, 4, 8):
        keep, a = pack_descs(pgood, pgood, (P, P + off) + pgood[2:])
        refused("alvq_pack_weights_bf16_batch", a + (2, None), b"misaligned image in descriptor 2")
    refused("alvq_pack_weights_bf16_batch", (None, 1, 1, None), b"no descriptors")

    for name, args in (("alvq_embedding_bag_fwd_f32", lambda B, L, K, M: (P, P, P, P, B, L, K, M, None, None)),
                       ("alvq_embedding_bag_bwd_f32", lambda B, L, K, M: (P, P, P, P, B, L, K, M, 0, None, None))):
        refused(name, args(16385, 1, 4, 4), b"16385 indices exceed", EUNSUPPORTED)
        refused(name, args(5, 3277, 4, 4), b"16385 indices exceed", EUNSUPPORTED)
        for dims in ((0, 3, 3, 3), (3, 0, 3, 3), (3, 3, 0, 3), (3, 3, 3, 0)):
            refused(name, args(*dims), b"bad dims")
        refused(name, (None,) + args(3, 3, 3, 3)[1:], b"null")
    refused("alvq_onehot_to_index_f32", (P, P, P, 0, 4, None), b"bad dims")
    refused("alvq_onehot_to_index_f32", (P, P, P, 4, 0, None), b"bad dims")
    refused("alvq_onehot_to_index_f32", (P, P, None, 4, 4, None), b"null")
    refused("alvq_onehot_to_index_f32", (P, P, P, 1 << 33, 4, None), b"too many rows", EUNSUPPORTED)
