"""conv1d_f16mx_kernel has instantiations compiled for ONE epilogue operand set -- no operand, bias alone, skip1 alone
(csrc/conv1d_f16mx.hip: wave_epilogue_fx_set; the dispatch gives them a launch whose output channels fill whole 256-channel
m-tiles) -- next to the general epilogue that tests every operand at run time.  Option fx_epi = 0 sends every launch to the
general one, so each launch here runs twice in one library and every byte it defines must agree: the H plane, the Q plane, the
sign bits a ReLU'd output leaves behind, and the fp32 (B, M, L) output of the launches that leave the format.

Shapes, the smallest that reach every branch.  B = 3, L = 37: 1 + 3 * 38 rows, gap rows inside 32-row blocks, a partial last row
tile.  B = 1, L = 300: one sample crosses a 256-row tile.  C = 64 and 96 (Cp = 64 and 128: one and two pairs of K chunks).
M = 201 (Mop = 256: the specialised kernels, with the scalar bias tail and a 32-channel tile beyond M), M = 512 (two m-tiles of
them), M = 64 and 320 (Mop is no multiple of 256, a second m-tile partly empty: these must stay on the general epilogue and
still agree).  Widths 1 and 3, the 256-row and the 128-row tile (fx_rows), for the fp32 output the 128-channel tile too
(fx_narrow), ReLU on and off.

Values: output channel m is scaled by GAINS[m % 6], so that outputs, biases and skips hold exact zeros, both signs, magnitudes
around 2^-10 (the lower end of the fp8 window) and around 400 and beyond 448 (where the fp8 conversion saturates)."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from acoustic_locating_vq_vae import _native as N  # noqa: E402

SHAPES = [(3, 37), (1, 300)]
CS = [64, 96]
MS = [64, 201, 320, 512]
GAINS = [1.0, 0.0, 2.0 ** -10, 400.0, -1.0, 150.0]
# (bias, skip1): the three specialised sets
SETS = {"none": (0, 0), "bias": (1, 0), "skip1": (0, 1)}
TILES = [dict(fx_rows=256), dict(fx_rows=128)]
TILES_NCL = [dict(fx_rows=256, fx_narrow=0), dict(fx_rows=128, fx_narrow=0), dict(fx_rows=0, fx_narrow=1)]


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


def case(B, L, C, M, KW):
    """Operands of one shape on the device, made once, shared by the tests and never modified."""
    key = (B, L, C, M, KW)
    if key not in _cases:
        g = torch.Generator().manual_seed(B * 7 + L * 11 + C * 13 + M * 17 + KW)
        r = lambda *s: torch.randn(*s, generator=g)
        gain = torch.tensor([GAINS[m % len(GAINS)] for m in range(M)])
        x = r(B, C, L)
        x[:, :, ::5] = 0.0
        enter = lambda t: N.ncl_to_nlc(t.cuda(), 2, "f16mx")
        _cases[key] = dict(x=enter(x), w=N.pack_weight((r(M, C, KW) / (C * KW) ** 0.5 * gain.view(M, 1, 1)).cuda(), N.W_OIK, 3),
                           b=(r(M) * gain).cuda(), s1=enter(r(B, M, L) * gain.view(1, M, 1)), mk=enter(r(B, M, L)))
    return _cases[key]


def bits_of(t):
    """Everything a launch defines of an f16mx output: both planes and, where valid, the sign bits."""
    out = [t.matrix(p).view(torch.int16) for p in range(t.planes)]
    if t.has_bits:
        off = t.bits_ptr - t.storage.data_ptr()
        out.append(t.storage.view(torch.uint8)[off:off + t.rows * t.Cp // 8])
    return out


def both(run):
    """run() under fx_epi = 1 and 0.  Both results stay alive, so neither can sit in the other's memory."""
    with forced(fx_epi=1):
        a = run()
    with forced(fx_epi=0):
        b = run()
    return a, b


@pytest.mark.parametrize("KW", [1, 3])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B,L", SHAPES)
def test_specialised_sets_match_the_general_epilogue(B, L, C, M, KW):
    c, keep = case(B, L, C, M, KW), []
    for tiles in TILES:
        for s, (bias, s1) in SETS.items():
            for relu in (False, True):
                with forced(wide_min_tiles=1, **tiles):
                    a, b = both(lambda: N.conv1d_bf16(c["x"], c["w"], c["b"] if bias else None, c["s1"] if s1 else None, relu=relu))
                keep += [a, b]           # no output of this case reuses the memory of another
                assert a.has_bits == b.has_bits == relu
                for name, p, q in zip(("H plane", "Q plane", "sign bits"), bits_of(a), bits_of(b)):
                    assert torch.equal(p, q), (tiles, s, relu, name)


@pytest.mark.parametrize("KW", [1, 3])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("B,L", SHAPES)
def test_fp32_output_with_bias_is_unchanged(B, L, M, KW):
    """The launches that leave the format (fp32 (B, M, L), bias alone) have no specialised kernel: fx_epi must not move them."""
    c = case(B, L, 64, M, KW)
    for tiles in TILES_NCL:
        with forced(wide_min_tiles=1, **tiles):
            a, b = both(lambda: N.conv1d_bf16(c["x"], c["w"], c["b"], out_ncl=True))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), tiles


@pytest.mark.parametrize("KW", [1, 3])
@pytest.mark.parametrize("M", [201, 512])
def test_other_operand_sets_keep_the_general_epilogue(M, KW):
    """skip1 + bias and a mask tensor are none of the three sets: on shapes the specialised kernels serve, both settings of
    fx_epi give the same bytes, and the mask and the bias have been applied (a misrouted launch would have dropped one)."""
    B, L = SHAPES[0]
    c = case(B, L, 64, M, KW)
    for tiles in TILES:
        for kw in (dict(bias=c["b"], skip1=c["s1"], relu=True), dict(mask=c["mk"]), dict(skip1=c["s1"], mask=c["mk"])):
            with forced(wide_min_tiles=1, **tiles):
                a, b = both(lambda: N.conv1d_bf16(c["x"], c["w"], **kw))
                with forced(fx_epi=1):
                    plain = N.conv1d_bf16(c["x"], c["w"], skip1=kw.get("skip1"), relu=kw.get("relu", False))
            for p, q in zip(bits_of(a), bits_of(b)):
                assert torch.equal(p, q), (tiles, sorted(kw))
            assert not torch.equal(bits_of(a)[0], bits_of(plain)[0]), (tiles, sorted(kw))
