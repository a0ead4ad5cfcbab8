"""WPE (csrc/wpe.hip) at the edges of what its argument check allows, against the float64 restatement of
tests/helpers/wpe_ref.py under test_wpe_gpu.py's bound (max |Y - Y_ref| <= (8 M u cond + 1e-13) max |x| per bin, cond <= 1e6
asserted on every bin; complex64: the restatement of the promoted input and 6e-8 max |y| more): delay = 0, psd_context and
delay at their caps of 64, D = 8, the path that keeps q and w in the caller's workspace with a power context, several items
and 1, 3 and 16 iterations, and the largest T whose rows still fit in LDS (5111 at D = taps = 1, where the launch asks for the
whole 160 KiB less 256 bytes of dynamic LDS) next to T + 1.  The cases are tests/helpers/signal_edge_cases.py's, pinned on
the host by tests/test_signal_edges_cpu.py.

Largest measured / bound on an MI355X: 0.023 in complex128 (T = 5112, the first row in the workspace) and 0.85 in complex64
(16 iterations on the workspace path; the rounding of Y to float32); per group in WORST below."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import signal_edge_cases as E  # noqa: E402
import wpe_ref as R  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import dereverberation as DV  # noqa: E402

# the largest measured / bound on an MI355X; complex64 is the one rounding of Y (half a float32 ulp of 4 is 2.4e-7)
WORST = {"argument limits": (0.0029, 0.63),                   # (complex128, complex64)
         "workspace path, 3 / 1 / 16 iterations": (0.0013, 0.85),
         "T = 5111 (LDS)": (0.0015, 0.57), "T = 5112 (workspace)": (0.023, 0.47)}

DTYPES = [np.complex128, np.complex64]


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()          # a copy: the shared cases are read-only


def same_bits(a, b):
    ra, rb = (torch.view_as_real(t.contiguous()) for t in (a, b))
    if ra.shape != rb.shape or ra.dtype != rb.dtype:
        return False
    view = {torch.float64: torch.int64, torch.float32: torch.int32}[ra.dtype]
    return torch.equal(ra.view(view), rb.view(view))


def run(X, case, iterations=3):
    B, D, F, T, taps, delay, ctx, loading = case
    return DV.wpe(dev(X), taps=taps, delay=delay, iterations=iterations, psd_context=ctx, eps=1e-10, loading=loading)


def parity(case, cdtype, iterations=3):
    """One launch held to the bound; returns (the device's result, the input it got, the restatement's Y)."""
    B, D, F, T, taps, delay, ctx, loading = case
    c = E.wpe_case(case, iterations)
    if cdtype == np.complex128:
        X, Yref, cond, rounding = c.X, c.Y, c.cond, 0.0
    else:
        X = c.X.astype(np.complex64)
        Yref, status, cond = R.wpe(X.astype(np.complex128), taps, delay, iterations, ctx, 1e-10, loading)
        assert not status.any()
        rounding = 6e-8
    got = run(X, case, iterations)
    assert got.spec.dtype == (torch.complex128 if cdtype == np.complex128 else torch.complex64) and got.spec.shape == X.shape
    assert got.status.shape == (B, F) and not got.status.cpu().numpy().any()
    E.check_wpe(got.spec.cpu().numpy(), X.astype(np.complex128), Yref, cond, case, rounding=rounding,
                tag="%s, %d iterations" % (np.dtype(cdtype).name, iterations))
    return got, X, Yref


@pytest.mark.parametrize("cdtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", E.WPE_CASES, ids=lambda c: "-".join(str(v) for v in c[:7]))
def test_argument_limits(case, cdtype):
    got, X, Yref = parity(case, cdtype)
    if case == E.WPE_DELAY0:            # the filter predicts the frame from itself: nothing is left, on either side
        top = np.abs(X).max()
        assert np.abs(Yref).max() <= 1e-4 * top and float(got.spec.abs().max()) <= 1e-4 * top


@pytest.mark.parametrize("cdtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("iterations", [3, 1, 16])
def test_workspace_path(iterations, cdtype):
    case = E.WPE_WORKSPACE
    B, D, F, T, taps = case[:5]
    assert N.lib().alvq_wpe_workspace_bytes(B, D, F, T, taps) == B * F * 2 * T * 8 != 0       # not the LDS path
    got, X, _ = parity(case, cdtype, iterations)
    if iterations != 3:
        return
    again = run(X, case)
    assert same_bits(again.spec, got.spec) and torch.equal(again.status, got.status)
    for b in range(B):                                                       # an item alone
        alone = run(X[b:b + 1], case)
        assert same_bits(alone.spec[0], got.spec[b]) and torch.equal(alone.status[0], got.status[b]), b
    for f in range(F):                                                       # a bin alone
        alone = run(X[1:2, :, f:f + 1], case)
        assert same_bits(alone.spec[0, :, 0], got.spec[1, :, f]), f


@pytest.mark.parametrize("cdtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_largest_row_in_lds_and_the_next(cdtype):
    fits = lambda T: N.lib().alvq_wpe_workspace_bytes(1, 1, 1, T, 1) == 0                     # noqa: E731
    lo, hi = 1, 65535
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    assert lo == E.WPE_LDS_T == 5111
    for T in (lo, lo + 1):              # two inputs of their own: the sums differ in length, the outputs are not compared
        parity(E.wpe_boundary_case(T), cdtype)
