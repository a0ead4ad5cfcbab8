"""Float64 numpy restatement of what csrc/grad_clip.hip computes (include/alvq.h states the contract): the sum of squares, the
norm of the mean gradient, torch.nn.utils.clip_grad_norm_'s coefficient, the fp32 product that scales grad_scale, and the
learning-rate schedule of alvq_adam_advance_sched_f32.  No torch, no GPU: tests/test_grad_clip_cpu.py pins these functions
to torch's own clip_grad_norm_ / LinearLR / CosineAnnealingLR, tests/test_grad_clip_gpu.py pins the kernels to them."""
import math

import numpy as np


def sum_squares(g):
    """Exact sum of g^2 for fp32 ``g``, correctly rounded to float64 (the squares are exact in float64; fsum adds exactly)."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64).ravel()
    return math.fsum((g * g).tolist())


def clip_scalars(sumsq, grad_scale, max_norm):
    """(norm, coef, new grad_scale as fp32, clipped?) from the float64 sum of squares of the SUMMED gradient buffer and the
    fp32 ``grad_scale`` (1/world) the optimiser state holds."""
    scale32 = np.float32(grad_scale)
    with np.errstate(all="ignore"):
        norm = np.sqrt(np.float64(sumsq)) * np.float64(scale32)
        coef = np.float64(max_norm) / (norm + np.float64(1e-6))
        if coef > 1.0:                                     # torch.clamp(max=1.0): NaN stays NaN
            coef = np.float64(1.0)
        new_scale = np.float32(scale32 * np.float32(coef))  # one fp32 product
    return float(norm), float(coef), new_scale, bool(coef < 1.0)


def clip(g, grad_scale, max_norm):
    return clip_scalars(sum_squares(g), grad_scale, max_norm)


def scheduled_lr(t, lr, warmup_steps=0, total_steps=None, lr_min=0.0):
    """Rate of the 1-based applied step ``t``: linear warm-up, then cosine annealing to ``lr_min`` at ``total_steps``."""
    t, w = float(t), float(warmup_steps)
    if t <= w:
        return lr * t / w
    if total_steps is not None and total_steps > warmup_steps:
        p = min(1.0, (t - w) / (float(total_steps) - w))
        return lr_min + (lr - lr_min) * (0.5 * (1.0 + math.cos(math.pi * p)))
    return lr


def adam_scalar0(t, lr, beta1, warmup_steps=0, total_steps=None, lr_min=0.0):
    """scalars[0] of the FlatAdam state at applied step ``t``: scheduled rate / bias_correction1, rounded to fp32."""
    return np.float32(scheduled_lr(t, lr, warmup_steps, total_steps, lr_min) / (1.0 - beta1 ** t))
