"""Argument errors of the NLC (16-bit) entry points, pinned rule by rule: the four convolutions, the eight weight gradients
and the ten layout / ReLU-mask conversions.  Every call passes non-null fake pointers and breaks exactly one rule, so it must
fail its host checks before any launch (there is no GPU here) with that rule's status code, a message that starts with the
name of the export that was called, and the rule's key phrase."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 0x1000           # a non-null pointer: every call below must fail its host checks before touching it
DEFER = 2               # ALVQ_WGRAD_DEFER


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native
    return _native.lib()


def _expect(lib, name, rc, code, phrase):
    msg = lib.alvq_last_error() or b""
    assert rc == code, (name, phrase, rc, msg)
    assert msg.startswith(name.encode() + b":"), (name, msg)
    assert phrase.encode() in msg, (name, phrase, msg)


# ---------------------------------------------------------------------------------------------------------------- convolutions
# trailing arguments after (B, C, M, L, KW, relu): mask_bits, relu_bits_out[, out_scale], stream
CONVS = {"alvq_conv1d_bf16": 2, "alvq_conv1d_f16": 3, "alvq_conv1d_bf16x3": 0, "alvq_conv1d_f16mx": 3}


def _conv(lib, name, x=FAKE, wp=FAKE, skip1=None, mask=None, post=None, y=FAKE, y2=None, y_ncl=None, B=2, C=7, M=16, L=13, KW=3,
          relu=0, mask_bits=None, bits_out=None):
    tail = [mask_bits, bits_out, None][:CONVS[name]]
    assert CONVS[name] or (mask_bits is None and bits_out is None)
    return getattr(lib, name)(x, wp, None, skip1, None, mask, post, y, y2, y_ncl, B, C, M, L, KW, relu, *tail, None)


CONV_RULES = [
    (dict(x=None), EINVAL, "null x/wp/y"),
    (dict(y_ncl=FAKE), EINVAL, "choose one of y (NLC) and y_ncl (NCL fp32)"),
    (dict(B=0), EINVAL, "bad dims"),
    (dict(KW=2), EUNSUPPORTED, "KW=2 (only 1 and 3)"),
    (dict(y2=FAKE), EINVAL, "y2 and post go together"),
    (dict(y=None, y_ncl=FAKE, relu=1), EUNSUPPORTED, "the NCL fp32 epilogue fuses bias"),
    (dict(B=1 << 20, L=1 << 11), EUNSUPPORTED, "problem too large"),
]
CONV_BITS_RULES = [
    (dict(mask=FAKE, mask_bits=FAKE), EINVAL, "pass the mask as a tensor or as bits, not both"),
    (dict(y=None, y_ncl=FAKE, mask_bits=FAKE), EUNSUPPORTED, "sign bits go with the NLC output"),
]


@pytest.mark.parametrize("name", sorted(CONVS))
def test_conv_argument_rules(lib, name):
    for kw, code, phrase in CONV_RULES + (CONV_BITS_RULES if CONVS[name] else []):
        _expect(lib, name, _conv(lib, name, **kw), code, phrase)


# ------------------------------------------------------------------------------------------------------------ weight gradients
# name -> (takes an inverse loss scale, accepts a null dw under ALVQ_WGRAD_DEFER)
WGRADS = {"alvq_conv1d_wgrad_bf16": (False, True), "alvq_conv1d_wgrad_f16": (True, True),
          "alvq_conv1d_wgrad_bf16x3": (False, False), "alvq_conv1d_wgrad_f16mx": (True, False)}


def _ptrs(*vals):
    """A host array of device pointers, as the _multi forms take it; the caller keeps it alive."""
    return (ctypes.c_void_p * len(vals))(*vals)


def _wgrad(lib, name, multi, dy=FAKE, x=FAKE, nseg=1, dw=FAKE, ws=FAKE, B=2, C=7, M=16, L=13, KW=3, w_layout=0, accumulate=0,
           seg_null=None):
    tail = [None, None] if WGRADS[name][0] else [None]          # [inv_scale,] stream
    if not multi:
        return getattr(lib, name)(dy, x, dw, None, ws, B, C, M, L, KW, w_layout, accumulate, *tail)
    n = max(1, min(nseg, 4))
    dys, xs = _ptrs(*[FAKE] * n), _ptrs(*[FAKE] * n)
    if seg_null is not None:
        xs[seg_null] = None
    return getattr(lib, name + "_multi")(ctypes.addressof(dys) if dy else None, ctypes.addressof(xs) if x else None, nseg, dw, ws,
                                         B, C, M, L, KW, w_layout, accumulate, *tail)


WGRAD_RULES = [
    (dict(dy=None), EINVAL, "null pointer"),
    (dict(M=0), EINVAL, "bad dims"),
    (dict(KW=5), EUNSUPPORTED, "KW=5 (only 1 and 3)"),
    (dict(w_layout=7), EINVAL, "w_layout"),
]
WGRAD_MULTI_RULES = [
    (dict(nseg=0), EUNSUPPORTED, "nseg=0 (1..4)"),
    (dict(nseg=5), EUNSUPPORTED, "nseg=5 (1..4)"),
    (dict(nseg=2, seg_null=1), EINVAL, "null segment 1"),
]


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("name", sorted(WGRADS))
def test_wgrad_argument_rules(lib, name, multi):
    who = name + ("_multi" if multi else "")
    for kw, code, phrase in WGRAD_RULES + (WGRAD_MULTI_RULES if multi else []):
        _expect(lib, who, _wgrad(lib, name, multi, **kw), code, phrase)
    # a null dw with a deferred reduction: the bf16 / fp16 forms take it (the call runs on to its next rule, here the
    # layout), the bf16x3 / f16mx forms, which do not defer, refuse it
    rc = _wgrad(lib, name, multi, dw=None, accumulate=DEFER, w_layout=7)
    _expect(lib, who, rc, EINVAL, "w_layout" if WGRADS[name][1] else "null pointer")
    # ... and without the deferral nobody takes it
    _expect(lib, who, _wgrad(lib, name, multi, dw=None, w_layout=7), EINVAL, "null pointer")


# ------------------------------------------------------------------------------------------- layout and ReLU-mask conversions
# name -> number of pointers before (B, C, L), number of trailing arguments after them (scale, stream)
LAYOUTS = {"alvq_ncl_to_nlc_bf16": (2, 1), "alvq_nlc_to_ncl_f32": (2, 1), "alvq_ncl_to_nlc_f16": (2, 2), "alvq_nlc_to_ncl_f16": (2, 2),
           "alvq_ncl_to_nlc_bf16x3": (2, 1), "alvq_nlc_to_ncl_bf16x3": (2, 1), "alvq_ncl_to_nlc_f16mx": (2, 2),
           "alvq_nlc_to_ncl_f16mx": (2, 2), "alvq_relu_mask_bf16x3": (3, 1), "alvq_relu_mask_f16mx": (3, 1)}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_layout_argument_rules(lib, name):
    nptr, ntail = LAYOUTS[name]
    fn = getattr(lib, name)
    for i in range(nptr):
        ptrs = [FAKE] * nptr
        ptrs[i] = None
        _expect(lib, name, fn(*ptrs, 2, 7, 13, *[None] * ntail), EINVAL, "null pointer")
    for dims in [(0, 7, 13), (2, 0, 13), (2, 7, 0), (-1, 7, 13)]:
        _expect(lib, name, fn(*[FAKE] * nptr, *dims, *[None] * ntail), EINVAL, "bad dims")
