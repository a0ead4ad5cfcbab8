"""STOI (csrc/speech_metrics.hip) on rows of more than one tile of 256 frames, against the float64 restatement of
tests/helpers/speech_metrics_ref.py: stoi_mask_kernel's carry from tile to tile and its second count buffer, and
stoi_correlate_kernel with more band-segment pairs than one pass of its threads.  256, 257, 389 and 601 frames (one tile, one
frame more, the project's own utterances, three tiles); in every batch a row that keeps every frame, one that loses a stretch
across frame 256 and one inside the first tile, one whose later tiles keep nothing and one whose first tile keeps nothing.
The rows, their kept frames and the tolerance (test_speech_metrics_gpu.py's 1e-10, with the mask margin asserted) are
tests/helpers/signal_edge_cases.py's, pinned on the host by tests/test_signal_edges_cpu.py.

Largest |value - restatement| on an MI355X: 4.0e-15 (601 frames) against the bound of 1e-10; per row length in WORST below."""
import os
import sys

import numpy as np
import pytest
import scipy.signal
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import signal_edge_cases as E  # noqa: E402
import speech_metrics_ref as R  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as M  # noqa: E402

# the largest |value - restatement| on an MI355X (the bound is 1e-10)
WORST = {32896: 2.0e-15, 33024: 1.7e-15, 50000: 1.7e-15, 77056: 4.0e-15, "80000 samples at 16 kHz": 1.6e-15}


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()          # a copy: the shared rows are read-only


def same_bits(a, b):
    """Two STOI tuples equal bit for bit, NaN included."""
    view = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t          # noqa: E731
    return all(x.shape == y.shape and torch.equal(view(x), view(y)) for x, y in zip(a, b))


def check(got, refs, tag):
    worst = E.check_stoi(*(t.cpu().numpy() for t in got), refs, tag)
    print("%s: largest |value - restatement| %.3g (bound %.3g)" % (tag, worst, E.STOI_ATOL))


@pytest.mark.parametrize("n", E.STOI_N)
def test_rows_beyond_one_tile_of_frames(n):
    clean, degraded = E.stoi_rows(n)
    x, y = dev(clean), dev(degraded)
    got = M.stoi(x, y, fs=10000)
    refs = E.stoi_reference(n)
    check(got, refs, "n %d" % n)
    assert list(zip(got.kept_frames.tolist(), got.status.tolist())) == E.STOI_EXPECT[n]
    for b in range(4):                                                      # a row alone
        assert same_bits(tuple(t[b:b + 1] for t in got), M.stoi(x[b:b + 1], y[b:b + 1], fs=10000)), b
    assert same_bits(got, M.stoi(x, y, fs=10000))                           # a second launch


def test_the_workloads_utterance_at_16_khz():
    """80000 float32 samples at 16 kHz: 50000 at 10 kHz, 389 frames, against the restatement of scipy's 5/8 resampling."""
    g = np.random.default_rng(4180)
    clean = g.standard_normal((1, 80000)).astype(np.float32)
    degraded = (clean + 0.5 * g.standard_normal((1, 80000))).astype(np.float32)
    got = M.stoi(dev(clean), dev(degraded))                                 # fs = 16000
    c10, d10 = (scipy.signal.resample_poly(v.astype(np.float64), 5, 8, axis=-1) for v in (clean, degraded))
    assert c10.shape == (1, 50000)
    ref = R.stoi(c10[0], d10[0])
    assert ref.nf == ref.kept_frames == 389 and ref.status == 0
    check(got, [ref], "80000 samples at 16 kHz")
    assert same_bits(got, M.stoi(dev(clean), dev(degraded), fs=16000))
