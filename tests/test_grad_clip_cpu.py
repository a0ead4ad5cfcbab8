"""Gradient clipping and the warm-up / cosine schedule without a GPU: the numpy restatement (tests/helpers/grad_clip_ref.py)
against torch's own clip_grad_norm_ / LinearLR / CosineAnnealingLR, the constructors' argument contract (errors before the
library is touched; CPU buffers refuse the options) and the untouched off path."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import grad_clip_ref as G  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import train_step as TS  # noqa: E402
from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE  # noqa: E402

CFG = (20, 48, 8, 2, 24, 0.25, 64)


def _shards(seed=0):
    g = np.random.default_rng(seed)
    return [g.normal(size=s).astype(np.float32) * sc for s, sc in (((7, 5), 1.0), ((33,), 1e-3), ((4, 3, 2), 30.0))]


@pytest.mark.parametrize("case", ["clipped", "unclipped", "inf_max_norm", "inf_norm", "nan"])
def test_restatement_equals_torch_clip_grad_norm(case):
    """The restatement's coefficient, applied in float64, gives the gradients torch.nn.utils.clip_grad_norm_ leaves."""
    shards = _shards()
    if case == "inf_norm":
        shards[1][3] = np.inf
    if case == "nan":
        shards[2][0, 0, 0] = np.nan
    flat = np.concatenate([s.ravel() for s in shards])
    true_norm = math.sqrt(G.sum_squares(flat)) if case not in ("inf_norm", "nan") else None
    max_norm = {"clipped": 0.5 * (true_norm or 1.0), "unclipped": 2.0 * (true_norm or 1.0), "inf_max_norm": math.inf,
                "inf_norm": 1.0, "nan": 1.0}[case]
    params = [torch.nn.Parameter(torch.zeros(s.shape, dtype=torch.float64)) for s in shards]
    for p, s in zip(params, shards):
        p.grad = torch.from_numpy(s.astype(np.float64))
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    norm, coef, new_scale, clipped = G.clip(flat, 1.0, max_norm)
    if case == "nan":
        assert math.isnan(norm) and math.isnan(coef) and math.isnan(float(new_scale)) and not clipped
        assert all(bool(torch.isnan(p.grad).all()) for p in params)          # torch scales by NaN too
        return
    if case == "inf_norm":
        assert norm == math.inf and coef == 0.0 and float(new_scale) == 0.0 and clipped
        finite = np.isfinite(flat)
        got = torch.cat([p.grad.reshape(-1) for p in params]).numpy()
        assert np.all(got[finite] == 0.0)                                     # inf * 0 is NaN on both sides; the rest is 0
        return
    assert abs(float(total) - norm) <= 1e-15 * norm
    assert clipped == (case == "clipped") and (coef < 1.0) == clipped
    if case != "clipped":
        assert coef == 1.0 and new_scale == np.float32(1.0)
    want = torch.cat([p.grad.reshape(-1) for p in params]).numpy()
    got = flat.astype(np.float64) * coef
    assert np.max(np.abs(got - want)) <= 1e-15 * np.max(np.abs(want))
    # the fp32 product the kernel stores: grad_scale (1/world) times the coefficient rounded to fp32
    _, coef4, scale4, _ = G.clip(flat, 0.25, max_norm * 0.25)                 # the mean over 4 ranks of a 4x sum
    assert scale4 == np.float32(np.float32(0.25) * np.float32(coef4))
    assert abs(coef4 - coef) <= 1e-6 * coef                                   # (only the +1e-6 of the denominator differs)


def test_warmup_equals_linear_lr():
    """LinearLR(start_factor=1/warmup, total_iters=warmup-1) read before step k (1-based) is lr * k / warmup."""
    lr, warmup = 3e-3, 5
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0 / warmup, end_factor=1.0, total_iters=warmup - 1)
    for t in range(1, 12):
        want = opt.param_groups[0]["lr"]
        got = G.scheduled_lr(t, lr, warmup)
        assert abs(got - want) <= 1e-12 * lr, (t, got, want)
        opt.step()
        sched.step()
    assert G.scheduled_lr(1, lr, 0) == lr and G.scheduled_lr(7, lr, 0) == lr  # no warm-up, no total: the constant rate


def test_cosine_equals_cosine_annealing_closed_form():
    lr, warmup, total, lr_min = 2e-3, 4, 10, 1e-5
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=total - warmup, eta_min=lr_min)
    for k in range(0, total - warmup + 1):                 # k = t - warmup steps into the annealing
        want = sched._get_closed_form_lr()[0] if k else lr
        closed = lr_min + (lr - lr_min) * (1 + math.cos(math.pi * k / (total - warmup))) / 2
        got = G.scheduled_lr(warmup + k, lr, warmup, total, lr_min)
        assert abs(want - closed) <= 1e-15 and abs(got - closed) <= 1e-15, (k, got, want, closed)
        assert abs(opt.param_groups[0]["lr"] - got) <= 1e-12                 # the recursive form torch steps with agrees
        opt.step()
        sched.step()
    assert G.scheduled_lr(warmup, lr, warmup, total, lr_min) == lr            # the warm-up ends on the peak
    assert abs(G.scheduled_lr(total, lr, warmup, total, lr_min) - lr_min) <= 1e-18
    assert abs(G.scheduled_lr(total + 5, lr, warmup, total, lr_min) - lr_min) <= 1e-18   # p is clamped at 1
    # scalars[0] is that rate over the bias correction
    assert G.adam_scalar0(3, lr, 0.9, warmup, total, lr_min) == np.float32((lr * 3 / 4) / (1 - 0.9 ** 3))


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        pytest.fail("the native library was reached")
    monkeypatch.setattr(N, "lib", boom)


def _location_model():
    from acoustic_locating_vq_vae.vq_vae.location_model.location_model import LocationModule
    return LocationModule(5, 8, 1)


def test_constructor_validation(no_library):
    for bad in (dict(warmup_steps=-1), dict(warmup_steps=4, total_steps=4), dict(warmup_steps=4, total_steps=2),
                dict(warmup_steps=2, lr_min=-1e-6), dict(warmup_steps=2, lr_min=float("nan"))):
        with pytest.raises(ValueError, match="WarmupCosine"):
            TS.WarmupCosine(**bad)
    s = TS.WarmupCosine(3, 8, 1e-5)
    assert (s.warmup_steps, s.total_steps, s.lr_min) == (3, 8, 1e-5) and TS.WarmupCosine(0).total_steps is None
    model = ConvolutionalVQVAE(*CFG)
    buffers = TS.FlatBuffers(model.parameters())
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            TS.FlatAdam(buffers, max_grad_norm=bad)
        with pytest.raises(ValueError, match="max_grad_norm"):
            TS.Trainer(ConvolutionalVQVAE(*CFG), "speech", max_grad_norm=bad)
        with pytest.raises(ValueError, match="max_grad_norm"):
            TS.LocationTrainer(_location_model(), max_grad_norm=bad)
    with pytest.raises(TypeError, match="WarmupCosine"):
        TS.Trainer(ConvolutionalVQVAE(*CFG), "speech", lr_schedule=(3, 8))


def test_cpu_buffers_refuse_the_options(no_library):
    buffers = TS.FlatBuffers(ConvolutionalVQVAE(*CFG).parameters())
    for kw in (dict(max_grad_norm=1.0), dict(max_grad_norm=float("inf")), dict(schedule=TS.WarmupCosine(3))):
        with pytest.raises(NotImplementedError, match="GPU"):
            TS.FlatAdam(buffers, **kw)
    for kw in (dict(max_grad_norm=1.0), dict(lr_schedule=TS.WarmupCosine(3, 8))):
        with pytest.raises(NotImplementedError, match="GPU"):
            TS.Trainer(ConvolutionalVQVAE(*CFG), "speech", **kw)
        with pytest.raises(NotImplementedError, match="GPU"):
            TS.LocationTrainer(_location_model(), **kw)


def test_the_off_path_is_untouched(no_library, monkeypatch):
    def boom(*a, **k):
        pytest.fail("grad_clip was called with clipping off")
    monkeypatch.setattr(N, "grad_clip", boom)
    monkeypatch.setattr(N, "grad_clip_workspace", boom)
    tr = TS.Trainer(ConvolutionalVQVAE(*CFG), "speech")
    assert tr.opt.max_grad_norm is None and tr.opt.schedule is None
    assert sorted(tr.state_dict()) == ["exp_avg", "exp_avg_sq", "kind", "model", "numel", "step"]
    assert tr.opt.clip(TS._ALIGN, tr.buffers.grad.numel()) is None           # returns without calling into _native
    for read in (tr.grad_norm, tr.clipped_steps, tr.opt.grad_norm, tr.opt.clipped_steps):
        with pytest.raises(RuntimeError, match="max_grad_norm"):
            read()
    loc = TS.LocationTrainer(_location_model())
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        loc.grad_norm()
    assert N.ADAM_SCALARS == 8 and tr.opt.scalars.numel() == 8


def test_entry_points_reject_bad_arguments_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    lib = N.lib()
    assert lib.alvq_grad_clip_workspace_bytes(1) == (N.GRAD_CLIP_PARTIALS + 1) * 8
    assert lib.alvq_grad_clip_workspace_bytes(1 << 28) == (N.GRAD_CLIP_PARTIALS + 1) * 8     # the grid does not depend on n
    assert lib.alvq_grad_clip_workspace_bytes(0) == -1
    one = 256                                                # any non-null, aligned value: nothing is dereferenced
    for args, word in (((None, 4, one, 1.0, one, None, None), b"null"), ((one, 0, one, 1.0, one, None, None), b"n <= 0"),
                       ((one, 4, one, 0.0, one, None, None), b"max_norm"), ((one, 4, one, float("nan"), one, None, None), b"max_norm"),
                       ((one, 4, one, -2.0, one, None, None), b"max_norm"), ((one + 2, 4, one, 1.0, one, None, None), b"misaligned")):
        assert lib.alvq_grad_clip_f32(*args) < 0
        msg = lib.alvq_last_error()
        assert msg.startswith(b"alvq_grad_clip_f32") and word in msg, msg
    for tail, word in (((-1, 0, 0.0), b"negative"), ((4, 4, 0.0), b"total_steps"), ((4, 2, 0.0), b"total_steps"),
                       ((4, 8, -1.0), b"lr_min")):
        assert lib.alvq_adam_advance_sched_f32(one, 1e-3, 0.9, 0.999, 1.0, None, None, *tail) < 0
        msg = lib.alvq_last_error()
        assert msg.startswith(b"alvq_adam_advance_sched_f32") and word in msg, msg
