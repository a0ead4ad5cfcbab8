"""The epilogues of the wide forward / data-gradient convolution kernels issue their operand loads in front of their stores
(csrc/conv_tile.h: wave_epilogue_dgrad16).  The order may not change a bit of any output, so every wide variant of the five
families (bf16_k3, bf16_v2, their fp16 twins, bf16x3, f16mx) is compared bit for bit with the narrowest tile of its family --
the 128 x 128 conv1d_bf16_kernel, whose epilogue is untouched, for the 16-bit formats; the 128-row x 128-channel tile (fx_rows
= 128, fx_narrow = 1) for the two-plane ones -- and against a float64 evaluation of the same operands rounded once.

B = 2, L = 130 gives 2 * 131 = 262 matrix rows: two row tiles, a gap row inside a 16-row block, a tail tile that is almost all
padding.  C = 64.  M = 96 (Mop = 128: half of a 256-channel tile lies beyond Mop; 96 % 32 == 0, the vector bias path) and M = 80
(the scalar bias path) reach the wide tiles of bf16x3 and f16mx; the 16-bit dispatch gives the wide kernels only an M within 32
of a multiple of 256 (test_16bit_tiles_names_the_wide_kernels pins that), so M = 250 (ragged bias, Mop = 256) and M = 256 are
here for conv1d_bf16_k3_kernel and conv1d_bf16_v2_kernel, whose data-gradient epilogue needs a wave block inside Mop.

Two kinds of data.  "real": Gaussian activations and weights; bit equality is asserted where the project claims it (v2 and
the 128 x 128 kernel at width 1, the tiles of bf16x3 among themselves, those of f16mx) -- at width 3 both wide 16-bit kernels
(k3, and v2 under conv_k3 = 0) sum the taps in another order than the 128 x 128 kernel, so their accumulators differ in the last
bits, before and after this change, and they are held to float64 alone there.  "exact":
activations in {-2 .. 2} and weights in {-1, 0, 1} (the other operands stay Gaussian), so every partial sum is an integer below
2^9, exact in every format and in any order: all variants of a family, k3 included, must then agree bit for bit.

Tolerances against float64 are those of tests/test_conv_tile_variants_gpu.py (the families' own)."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from acoustic_locating_vq_vae import _native as N  # noqa: E402

B, L, C = 2, 130, 64
MS = [96, 80, 250, 256]

bf16_round = lambda t: t.to(torch.bfloat16).float()
f16_round = lambda t: t.to(torch.float16).float()
# planes / fmt of ncl_to_nlc, weight code, rounding of the operands, (narrowest tile, wide variants), the float64 bound
FAMILIES = {
    "bf16": dict(planes=1, fmt=None, wcode=1, rnd=bf16_round, ulp=2.0 ** -7,
                 ref=dict(conv_v2=0), wide=[dict(), dict(conv_k3=0)]),
    "f16": dict(planes=1, fmt="f16", wcode=3, rnd=f16_round, ulp=2.0 ** -10,
                ref=dict(conv_v2=0), wide=[dict(), dict(conv_k3=0)]),
    "bf16x3": dict(planes=2, fmt=None, wcode=2, rnd=lambda t: t, tol=3e-5,
                   ref=dict(fx_narrow=1, fx_rows=128), wide=[dict(fx_narrow=0, fx_rows=0), dict(fx_narrow=1, fx_rows=256)]),
    "f16mx": dict(planes=2, fmt="f16mx", wcode=3, rnd=lambda t: t, tol=2e-4,
                  ref=dict(fx_narrow=1, fx_rows=128),
                  wide=[dict(fx_narrow=0, fx_rows=256), dict(fx_narrow=0, fx_rows=128), dict(fx_narrow=1, fx_rows=256)]),
}
# operand sets: (bias, skip1, skip2, mask: None / "bits" (of a ReLU'd tensor, where the format keeps sign bits) / "tensor",
# post, relu).  The last four are what the other data gradients of a train step pass.
SETS = {
    "none": (0, 0, 0, None, 0, 0),
    "bias_relu": (1, 0, 0, None, 0, 1),
    "skip1_relu": (0, 1, 0, None, 0, 1),
    "skip1_skip2_bits": (0, 1, 1, "bits", 0, 0),
    "mask_tensor": (0, 0, 0, "tensor", 0, 0),
    "skip1_post": (0, 1, 0, None, 1, 1),
    "bits": (0, 0, 0, "bits", 0, 0),
    "skip1_bits": (0, 1, 0, "bits", 0, 0),
    "skip1_mask_tensor": (0, 1, 0, "tensor", 0, 0),
    "skip1_skip2_mask_tensor": (0, 1, 1, "tensor", 0, 0),
}


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


_cases = {}


def case(M, KW, layout, kind="real"):
    """Operands (fp32, CPU) of one shape, made once and shared by the families; never modified."""
    key = (M, KW, layout, kind)
    if key not in _cases:
        g = torch.Generator().manual_seed(M * 100 + KW * 10 + layout)
        r = lambda *s: torch.randn(*s, generator=g)
        wshape = (M, C, KW) if layout == N.W_OIK else (C, M, KW)
        x, w = r(B, C, L), r(*wshape) / (C * KW) ** 0.5
        if kind == "exact":
            x, w = torch.randint(-2, 3, (B, C, L), generator=g).float(), torch.randint(-1, 2, wshape, generator=g).float()
        _cases[key] = dict(x=x, w=w, b=r(M), s1=r(B, M, L), s2=r(B, M, L), mk=r(B, M, L), post=r(B, M, L), t=r(B, M, L))
    return _cases[key]


def conv64(c, KW, layout, rnd):
    x, w = rnd(c["x"]).double(), rnd(c["w"]).double()
    if layout == N.W_OIK:
        return F.conv1d(x, w, None, padding=KW // 2)
    return F.conv_transpose1d(x, w, None, padding=KW // 2)


def bits_of(t):
    """Everything a launch defines of an output: the planes' matrices and, where valid, the sign bits."""
    out = [t.matrix(p).view(torch.int16).clone() for p in range(t.planes)]
    if t.has_bits:
        off = t.bits_ptr - t.storage.data_ptr()
        out.append(t.storage.view(torch.uint8)[off:off + t.rows * t.Cp // 8].clone())
    return out


def close(fam, got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if "ulp" in fam:    # one rounding of ref plus accumulation-order slack
        return bool(((got - ref).abs() <= ref.abs() * fam["ulp"] + 1e-6 * float(ref.abs().max())).all())
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30)) < fam["tol"]


def operands(fam, c, layout):
    enter = lambda t: N.ncl_to_nlc(t.cuda(), fam["planes"], fam["fmt"])
    ops = {k: enter(c[k]) for k in ("x", "s1", "s2", "mk", "post")}
    ops["w"] = N.pack_weight(c["w"].cuda(), layout, fam["wcode"])
    ops["b"] = c["b"].cuda()
    # a ReLU'd tensor of the output's shape: carries sign bits where the format keeps them (an identity width-1 layer)
    eye = N.pack_weight(torch.eye(c["t"].shape[1]).unsqueeze(-1).cuda(), N.W_OIK, fam["wcode"])
    with forced(wide_min_tiles=1, **fam["ref"]):
        ops["t"] = N.conv1d_bf16(enter(c["t"]), eye, relu=True)
    return ops


def launch(ops, s):
    bias, s1, s2, mask, post, relu = SETS[s]
    m = None if mask is None else (ops["t"] if mask == "bits" else ops["mk"])
    out = N.conv1d_bf16(ops["x"], ops["w"], ops["b"] if bias else None, ops["s1"] if s1 else None, ops["s2"] if s2 else None, m,
                        ops["post"] if post else None, relu=bool(relu))
    return out if post else (out,)


def reference(fam, c, ops, y64, s):
    bias, s1, s2, mask, post, relu = SETS[s]
    rnd = fam["rnd"]
    v = y64 + (c["b"].double().view(1, -1, 1) if bias else 0)
    if s1:
        v = v + rnd(c["s1"]).double()
    if s2:
        v = v + rnd(c["s2"]).double()
    if relu:
        v = F.relu(v)
    if mask == "bits":
        v = torch.where(N.nlc_to_ncl(ops["t"]).cpu() > 0, v, torch.zeros_like(v))
    elif mask == "tensor":
        v = torch.where(rnd(c["mk"]) > 0, v, torch.zeros_like(v))
    return (v, v + rnd(c["post"]).double()) if post else (v,)


@pytest.mark.parametrize("kind", ["real", "exact"])
@pytest.mark.parametrize("layout", [N.W_OIK, N.W_IOK], ids=["oik", "iok"])
@pytest.mark.parametrize("KW", [1, 3])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_wide_epilogues_match_narrow_tile_and_float64(name, M, KW, layout, kind):
    fam, c = FAMILIES[name], case(M, KW, layout, kind)
    ops = operands(fam, c, layout)
    y64 = conv64(c, KW, layout, fam["rnd"])
    rows = N.lib().alvq_nlc_rows(B, L)
    for s in SETS:
        refs = reference(fam, c, ops, y64, s)
        with forced(wide_min_tiles=1, **fam["ref"]):
            narrow = launch(ops, s)
        for got, ref in zip(narrow, refs):
            assert close(fam, N.nlc_to_ncl(got), ref), (s, "narrow tile against float64")
        want = [b for t in narrow for b in bits_of(t)]
        for opts in fam["wide"]:
            with forced(wide_min_tiles=1, **opts):
                wide = launch(ops, s)
                other_order = "ulp" in fam and N._conv16_name(0, 0, KW, M, rows).startswith("conv1d_bf16_k3_kernel")
            for got, ref in zip(wide, refs):
                assert close(fam, N.nlc_to_ncl(got), ref), (s, opts, "against float64")
            if kind == "exact" or not other_order:
                have = [b for t in wide for b in bits_of(t)]
                assert len(have) == len(want) and all(torch.equal(p, q) for p, q in zip(have, want)), (s, opts)


@pytest.mark.parametrize("KW", [1, 3])
def test_16bit_tiles_names_the_wide_kernels(KW):
    """The dispatch the cases above rely on: at wide_min_tiles = 1, M = 250 and 256 go to the 256 x 256 kernels, M = 96 and 80 stay
    on the 128 x 128 one (N._conv16_name mirrors csrc/conv1d_bf16.hip)."""
    rows = N.lib().alvq_nlc_rows(B, L)
    with forced(wide_min_tiles=1):
        for M in (250, 256):
            assert N._conv16_name(0, 0, KW, M, rows).startswith("conv1d_bf16_k3_kernel" if KW == 3 else "conv1d_bf16_v2_kernel")
        for M in (96, 80):
            assert N._conv16_name(0, 0, KW, M, rows).startswith("conv1d_bf16_kernel")


@pytest.mark.parametrize("s", ["skip1_relu", "skip1_bits"])
@pytest.mark.parametrize("KW", [1, 3])
@pytest.mark.parametrize("name", ["f16", "f16mx"])
def test_fp16_limit_still_raises_the_range_flag(name, KW, s):
    """One skip value at 65 504 where the convolution is positive (and the mask open): the stored value reaches fp16's limit,
    and every wide epilogue must report it (bit 2 of the range flag), as the narrow one does; without it none does."""
    fam, c = FAMILIES[name], dict(case(256, KW, N.W_OIK))
    y64 = conv64(c, KW, N.W_OIK, fam["rnd"])
    pos = (y64 > 0.5) & (c["t"] > 0.5)
    b, m, l = [int(i) for i in pos.nonzero()[0]]
    for big in (False, True):
        if big:
            c["s1"] = c["s1"].clone()
            c["s1"][b, m, l] = 65504.0
        ops = operands(fam, c, N.W_OIK)
        for opts in [fam["ref"]] + fam["wide"]:
            N.f16mx_range_flag(reset=True)
            with forced(wide_min_tiles=1, **opts):
                y, = launch(ops, s)
            assert bool(N.f16mx_range_flag(reset=True) & 4) == big, (opts, big)
            if big:
                assert float(N.nlc_to_ncl(y)[b, m, l]) >= 65504.0      # saturated (f16mx: H at the limit plus its Q term)
