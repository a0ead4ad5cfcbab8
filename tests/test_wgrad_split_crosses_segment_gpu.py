"""A split of a multi-segment weight-gradient launch that STARTS in one (dy, x) pair and ENDS in the next: the segment
walk of the staging shared by the four split-K kernels (csrc/wgrad_tile.h).  Training meets it on every step (speech
B = 64, the 1024 x 1024 width-3 launch), the other multi-segment tests never do: their chunks_per_split is 1.

Shapes (rows = pad256(1 + B (L + 1)), M = C = 1024, three segments):
  width 3: B = 2, L = 100 -> 256 rows = 4 chunks per segment; 64 tiles of 128 x 128 -> 4 splits of 3 chunks;
  width 1: B = 8, L = 120 -> 1024 rows = 16 chunks per segment; the 128 x 256-tile kernels get 8 splits of 6 chunks, the
           256 x 256-tile kernels 16 splits of 3.
Reference and bar per format are those of its own multi-segment test (test_wgrad_bf16_multi_segment_sums_uses,
test_wgrad_f16, test_wgrad_bf16x3_multi_..., test_wgrad_f16mx_multi_...)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from acoustic_locating_vq_vae import _native as N  # noqa: E402

NSEG, M, C = 3, 1024, 1024
DIMS = {3: (2, 100), 1: (8, 120)}            # KW -> (B, L)
MAG = 2.0 ** -20                             # the f16mx / f16 gradients ride on a loss scale (exact: a power of two)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def split_plan(total_rows, tiles):
    """wgrad_split_plan of csrc/nlc_host.h: (splits, chunks_per_split)."""
    nchunks = total_rows // 64
    want = max(1, min((256 + tiles - 1) // tiles, nchunks, 64))
    cps = (nchunks + want - 1) // want
    return (nchunks + cps - 1) // cps, cps


@functools.lru_cache(maxsize=None)
def operands(KW):
    """Three distinct (dy, x) pairs, fp32 on the CPU."""
    B, L = DIMS[KW]
    g = torch.Generator().manual_seed(40 + KW)
    return [(torch.randn(B, M, L, generator=g), torch.randn(B, C, L, generator=g)) for _ in range(NSEG)]


@functools.lru_cache(maxsize=None)
def reference(KW, rounding, S=None):
    """sum_i dW(dy_i, x_i) on the CPU with the operands rounded as the format stores them (None: fp32; "f16": dy is MAG * dy
    under the loss scale S, as in test_wgrad_f16)."""
    rnd = {None: lambda t: t, "bf16": lambda t: t.to(torch.bfloat16).float(), "f16": lambda t: t.to(torch.float16).float()}[rounding]
    rnd_dy = (lambda t: (t * MAG * S).half().float() / S) if rounding == "f16" else rnd
    w = torch.zeros(M, C, KW, requires_grad=True)
    for dy, x in operands(KW):
        F.conv1d(rnd(x), w, None, padding=KW // 2).backward(rnd_dy(dy))
    return w.grad


def tiles_of(fmt, KW, v3):
    mt = 256 if KW == 1 and (fmt == "f16mx" or (fmt in ("bf16", "f16") and v3)) else 128
    ct = 128 if KW == 3 else 256
    return (M // mt) * (C // ct)


# bf16 and f16 reach the v2 kernel with more than one segment only under wgrad_v3 = 0
CASES = [("bf16", 3), ("bf16", 0), ("f16", 3), ("f16", 0), ("bf16x3", None), ("f16mx", None)]


@pytest.mark.parametrize("KW", [3, 1])
@pytest.mark.parametrize("fmt,v3", CASES)
def test_wgrad_split_that_crosses_a_segment_boundary(fmt, v3, KW):
    B, L = DIMS[KW]
    rows = (1 + B * (L + 1) + 255) // 256 * 256
    prev = N.set_option("wgrad_v3", v3) if v3 is not None else None
    try:
        L_ = N.lib()
        if fmt in ("bf16", "f16"):
            splits = L_.alvq_conv1d_wgrad_bf16_splits(B, C, M, L, KW, NSEG, 0)
        else:
            splits = getattr(L_, "alvq_conv1d_wgrad_%s_splits" % fmt)(B, C, M, L, KW, NSEG)
        want_splits, cps = split_plan(NSEG * rows, tiles_of(fmt, KW, v3))
        # the plan this test exists for: if it changes, say so instead of testing nothing
        assert splits == want_splits and splits > 1, (splits, want_splits)
        assert cps > 1 and (rows // 64) % cps != 0, (cps, rows // 64)
        assert (cps, splits) == {3: (3, 4), 1: (3, 16) if tiles_of(fmt, KW, v3) == 16 else (6, 8)}[KW]

        ops = operands(KW)
        if fmt == "bf16":
            pairs = [(N.ncl_to_nlc(dy.cuda()), N.ncl_to_nlc(x.cuda())) for dy, x in ops]
            want, scale = reference(KW, "bf16"), 1.0
        elif fmt == "bf16x3":
            pairs = [(N.ncl_to_nlc(dy.cuda(), 2), N.ncl_to_nlc(x.cuda(), 2)) for dy, x in ops]
            want, scale = reference(KW, None), 1.0
        else:
            planes = 2 if fmt == "f16mx" else 1
            gs = N.grad_scale(torch.stack([dy for dy, _ in ops]).cuda() * MAG)
            pairs = [(N.ncl_to_nlc(dy.cuda() * MAG, planes, fmt, gs), N.ncl_to_nlc(x.cuda(), planes, fmt)) for dy, x in ops]
            want, scale = (reference(KW, "f16", float(gs[0])), 1.0) if fmt == "f16" else (reference(KW, None), MAG)
        got = N.conv1d_wgrad_bf16_multi(pairs, KW, N.W_OIK)
        err = rel(got, want * scale)
        bar = {"bf16": 3e-5, "f16": 3e-5, "bf16x3": 5e-5, "f16mx": 2e-4}[fmt]
        print("%s wgrad_v3=%s KW=%d: %d splits of %d chunks, rel %.3g (bar %.0e)" % (fmt, v3, KW, splits, cps, err, bar))
        assert err < bar
        if fmt in ("bf16x3", "f16mx"):          # as in their multi-segment tests: the launch == the sum of the single launches
            singles = sum(N.conv1d_wgrad_bf16(dy, x, KW, N.W_OIK) for dy, x in pairs)
            assert rel(got, singles) < 1e-6
    finally:
        if prev is not None:
            N.set_option("wgrad_v3", prev)
