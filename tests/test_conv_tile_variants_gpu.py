"""Every tile variant of the five forward / data-gradient convolution kernel families (128 x 128, v2, k3, bf16x3, f16mx) on the
smallest shapes at which the code they share (tile decode, slab swizzle, LDS-DMA staging, rings, fp32-NCL store) can go wrong,
each variant forced through the dispatch options and judged against a float64 convolution on the CPU.

L = 300 puts sample 0 on matrix rows 1..300 and sample 1 on rows 302..601: every 128-row and 256-row tile boundary (128, 256,
384, 512) falls inside a sample, so a width-3 tile needs real data from both halo rows, and the last tile is partly tail rows.
C = 40 -> Cp = 64, two chunks (width 1: two K-tiles, the prologue stages everything and the loop body runs once with every
in-loop issue guarded off); C = 130 -> Cp = 192, six chunks (three two-chunk iterations with the c + 2 < nch guards both true
and false; six K-tiles wrap v2's four-stage ring -- test_16bit_tiles_match_float64 says which shape gets there).  M = 250 is ragged, within 32 of 256 (the wide 16-bit kernels accept it); M = 100 takes
the 128-channel m-tiles and, with an fp32-NCL output, the f16mx narrow tile.

Tolerances are those of each family's own test_conv_*_matches_fp32 / *_epilogue_fusions."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from acoustic_locating_vq_vae import _native as N  # noqa: E402

SHAPES = [(2, 40, 250, 300), (2, 130, 100, 300)]


@contextlib.contextmanager
def forced(**options):
    prev = {k: N.get_option(k) for k in options}
    try:
        for k, v in options.items():
            N.set_option(k, v)
        yield
    finally:
        for k, v in prev.items():
            N.set_option(k, v)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def close_to_rounding(got, ref, ulp):
    """|got - ref| <= one rounding of ref (ulp = 2^-7 bf16, 2^-10 fp16) plus accumulation-order slack."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return bool(((got - ref).abs() <= ref.abs() * ulp + 1e-6 * float(ref.abs().max())).all())


_cases = {}


def case(B, C, M, L, KW):
    """Operands (fp32, CPU) of one shape, made once and shared by the families; never modified."""
    key = (B, C, M, L, KW)
    if key not in _cases:
        g = torch.Generator().manual_seed(B * 1000 + C + M + L + KW)
        r = lambda *s: torch.randn(*s, generator=g)
        _cases[key] = dict(x=r(B, C, L), w=r(M, C, KW) / (C * KW) ** 0.5, b=r(M), s1=r(B, M, L), mk=r(B, M, L), post=r(B, M, L))
    return _cases[key]


def reference(c, KW, rnd):
    """float64: the fp32-NCL output (bias only) and the NLC outputs (bias, one skip, ReLU, mask; + post) of operands
    rounded by rnd."""
    d = {k: rnd(v).double() for k, v in c.items() if k != "b"}
    y = F.conv1d(d["x"], d["w"], c["b"].double(), padding=KW // 2)
    v = F.relu(y + d["s1"])
    v = torch.where(d["mk"] > 0, v, torch.zeros_like(v))
    return y, v, v + d["post"]


def run(c, enter, wplanes):
    """One variant: (fp32-NCL output, NLC output, second NLC output, the NLC outputs' bits)."""
    xn, pk, b = enter(c["x"]), N.pack_weight(c["w"].cuda(), N.W_OIK, wplanes), c["b"].cuda()
    ncl = N.conv1d_bf16(xn, pk, b, out_ncl=True)
    y, y2 = N.conv1d_bf16(xn, pk, b, enter(c["s1"]), None, enter(c["mk"]), enter(c["post"]), relu=True)
    bits = [t.matrix(p).view(torch.int16).clone() for t in (y, y2) for p in range(t.planes)]   # the matrices only: guard rows are never written
    return ncl, N.nlc_to_ncl(y), N.nlc_to_ncl(y2), bits


@pytest.mark.parametrize("KW", [1, 3])
@pytest.mark.parametrize("B,C,M,L", SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_16bit_tiles_match_float64(fmt, B, C, M, L, KW):
    """128 x 128 (conv_v2 = 0), v2 (conv_k3 = 0) and the default k3 / v2 choice, bf16 and fp16 elements.  (M = 100 stays on
    the 128 x 128 tile under every option: the wide kernels take only an M within 32 of a multiple of 256.  So v2 and k3 run at
    C = 40 only, and the wrap of v2's four-stage ring is reached through the six K-tiles of C = 40 at width 3, not through the
    six chunks of C = 130.)"""
    c = case(B, C, M, L, KW)
    if fmt == "bf16":
        rnd, ulp, wplanes = (lambda t: t.to(torch.bfloat16).float()), 2.0 ** -7, 1
        enter = lambda t: N.ncl_to_nlc(t.cuda())
    else:
        rnd, ulp, wplanes = (lambda t: t.to(torch.float16).float()), 2.0 ** -10, 3     # the H image of f16mx packed weights
        enter = lambda t: N.ncl_to_nlc(t.cuda(), 1, "f16")
    ref = reference(c, KW, rnd)
    for opts in (dict(conv_v2=0), dict(conv_k3=0), dict()):
        with forced(wide_min_tiles=1, **opts):
            ncl, y, y2, _ = run(c, enter, wplanes)
        e = rel(ncl, ref[0])
        print("%s %s KW=%d %s: ncl %.2e" % (fmt, (B, C, M, L), KW, opts, e))
        assert e < 2e-5, opts
        assert close_to_rounding(y, ref[1], ulp) and close_to_rounding(y2, ref[2], ulp), opts


@pytest.mark.parametrize("KW", [1, 3])
@pytest.mark.parametrize("B,C,M,L", SHAPES)
def test_bf16x3_tiles_match_float64_and_each_other(B, C, M, L, KW):
    """(fx_narrow, fx_rows) = (0, 0) the 256 x 256 tile; (1, 128) 128 channels x 128 rows; (1, 256) 128 channels x 256 rows
    where M <= 128 (the 256 x 256 tile otherwise).  Same K order per output: the variants are bit-identical."""
    c = case(B, C, M, L, KW)
    ref = reference(c, KW, lambda t: t)
    outs = {}
    for key in ((0, 0), (1, 128), (1, 256)):
        with forced(wide_min_tiles=1, fx_narrow=key[0], fx_rows=key[1]):
            outs[key] = run(c, lambda t: N.ncl_to_nlc(t.cuda(), planes=2), 2)
        e = [rel(o, r) for o, r in zip(outs[key][:3], ref)]
        print("bf16x3 %s KW=%d %s: ncl %.2e y %.2e y2 %.2e" % ((B, C, M, L), KW, key, *e))
        assert max(e) < 3e-5, key
    for key in ((1, 128), (1, 256)):
        assert torch.equal(outs[key][0], outs[(0, 0)][0]), key
        assert all(torch.equal(p, q) for p, q in zip(outs[key][3], outs[(0, 0)][3])), key


@pytest.mark.parametrize("KW", [1, 3])
@pytest.mark.parametrize("B,C,M,L", SHAPES)
def test_f16mx_tiles_match_float64_and_each_other(B, C, M, L, KW):
    """fx_rows 128 / 256 x fx_narrow 0 / 1: the 256-row tile, the 128-row tile and (fp32-NCL output of M <= 128, fx_narrow = 1)
    the 128-row x 128-channel tile.  Same K order per output: the variants are bit-identical."""
    c = case(B, C, M, L, KW)
    ref = reference(c, KW, lambda t: t)
    outs = {}
    for key in ((0, 256), (0, 128), (1, 256), (1, 128)):
        with forced(wide_min_tiles=1, fx_narrow=key[0], fx_rows=key[1]):
            outs[key] = run(c, lambda t: N.ncl_to_nlc(t.cuda(), 2, "f16mx"), 3)
        e = [rel(o, r) for o, r in zip(outs[key][:3], ref)]
        print("f16mx %s KW=%d %s: ncl %.2e y %.2e y2 %.2e" % ((B, C, M, L), KW, key, *e))
        assert max(e) < 2e-4, key
    for key in ((0, 128), (1, 256), (1, 128)):
        assert torch.equal(outs[key][0], outs[(0, 256)][0]), key
        assert all(torch.equal(p, q) for p, q in zip(outs[key][3], outs[(0, 256)][3])), key
