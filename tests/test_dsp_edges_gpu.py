"""The waveform front-end kernels at the edges of their argument range, element by element against float64-or-better references.

csrc/stft.hip (alvq_stft_{power,complex}_{f32,f64}, alvq_fir_same_f64, alvq_spec_rir_wiener_f64) and csrc/istft.hip
(alvq_istft_*, alvq_griffin_lim_*) are called through the C entry points with every output and workspace pre-filled with NaN,
so an element no workgroup writes fails.  The references are tests/helpers/dsp_ref.py (extended precision, pinned to torch and
scipy by tests/test_dsp_ref_cpu.py) and tests/helpers/griffin_lim_ref.py.

Bounds are per element, scaled by the sum of |terms| that make up that element, so a quiet bin or a reflect-padded edge frame
is held to its own scale, not to the loudest element of the batch.  u is the unit roundoff of the kernel's precision:
  STFT     |X - X_ref| <= u ((N + 2) l1 + l1x): (N + 2) l1 is the first-order bound for a sequential N-term accumulation with
           rounded twiddles (l1 = sum |x w| / sqrt(sum w^2) over the frame); l1x = sum |x| / sqrt(sum w^2) covers the window
           values, which the kernel forms as 0.5 - 0.5 cos from its rounded table, an absolute error of about u even where w
           itself is tiny (an impulse at a frame edge).
  power    |P - |X_ref|^2| <= (2 |X_ref| + d) d, d the complex bound.
  iSTFT    |y - y_ref| <= u ((N + 2 + ceil(N/hop)) A + R + 2 |y_ref| W): A = the windowed |irfft terms| over the covering frames
           divided by the envelope, R = the same without the window (window-value error), W = sum w / envelope (its error).
One sample of window or reflect-index error moves a bin by about l1 / N (>= 5e-4 l1 at N = 2048): orders of magnitude above
every bound here.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from acoustic_locating_vq_vae import _native as N  # noqa: E402
from oracle import stft_oracle  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dsp_ref as R  # noqa: E402
import griffin_lim_ref as GL  # noqa: E402

U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
TDT = {"f32": torch.float32, "f64": torch.float64}
WORST = {}          # (kernel, precision) -> largest observed error / bound, printed as the tests go


def _note(key, ratio, where):
    if ratio > WORST.get(key, (-1.0, None))[0]:
        WORST[key] = (ratio, where)
    print("error/bound %-22s %.3e  (worst so far %.3e at %s)" % ("%s %s" % key, ratio, WORST[key][0], WORST[key][1]))


def ratio(err, bound):
    """max err / bound, elementwise; an element whose bound is 0 must be exact."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    safe = np.where(bound > 0, bound, 1.0)
    return float(np.max(np.where(bound > 0, err / safe, np.where(err > 0, np.inf, 0.0))))


def lib():
    return N.lib()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def ok(rc, name):
    assert rc == 0, "%s: rc=%d %s" % (name, rc, lib().alvq_last_error().decode())


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ STFT
def run_stft(x, n_fft, hop, prec, cplx, captured=False):
    """x (B, S) numpy -> (B, F, T) complex (cplx) or real, from the kernel, outputs pre-filled with NaN.  captured: the call is
    not run but captured on the current stream in a graph (one stream, one launch), which is then replayed."""
    B, S = x.shape
    F, T = n_fft // 2 + 1, 1 + S // hop
    xd = dev(x, TDT[prec])
    out = nan((B, F, T, 2) if cplx else (B, F, T), TDT[prec])
    name = "alvq_stft_%s_%s" % ("complex" if cplx else "power", prec)
    if captured:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = getattr(lib(), name)(xd.data_ptr(), out.data_ptr(), B, S, n_fft, hop, stream())
        ok(rc, name)
        assert torch.isnan(out).all(), "%s ran during its capture" % name
        graph.replay()
    else:
        ok(getattr(lib(), name)(xd.data_ptr(), out.data_ptr(), B, S, n_fft, hop, stream()), name)
    o = host(out).astype(np.float64)
    return o[..., 0] + 1j * o[..., 1] if cplx else o


def check_stft(x, n_fft, hop, X, l1, l1x, frames, prec, where):
    """Both kernels of one precision against the reference X (B, F, len(frames)) with its per-frame scales."""
    u = U[prec]
    d = (u * ((n_fft + 2) * l1 + l1x)).astype(np.float64)[:, None, :]
    got = run_stft(x, n_fft, hop, prec, True)
    assert np.isfinite(got).all(), "unwritten STFT elements at %s" % where
    # the twiddle table's sin entries for bins 0 and N/2 are sinpi(0) and sinpi(1): exactly 0
    assert (got[:, 0, :].imag == 0).all() and (got[:, -1, :].imag == 0).all(), where
    r = ratio(np.abs(got[..., frames] - X), d)           # differences in extended precision: X is not rounded first
    _note(("stft complex", prec), r, where)
    assert r <= 1.0, "complex %s %s: error/bound %.3g" % (prec, where, r)
    P = run_stft(x, n_fft, hop, prec, False)
    assert np.isfinite(P).all(), "unwritten power elements at %s" % where
    A = np.abs(X)
    r = ratio(np.abs(P[..., frames] - A * A), (2 * A + d) * d)
    _note(("stft power", prec), r, where)
    assert r <= 1.0, "power %s %s: error/bound %.3g" % (prec, where, r)


def _precs(n_fft):
    return ("f32", "f64") if n_fft <= R.STFT_F64_MAX else ("f32",)


@pytest.mark.parametrize("n_fft,hop,lengths", R.stft_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_stft_per_element(n_fft, hop, lengths):
    for i, S in enumerate(lengths):
        seed = 7919 * n_fft + 31 * hop + S
        B = 3 if i % 2 == 0 else 1
        x = R.stft_signal(B, S, seed)
        frames = R.check_frames(1 + S // hop, seed)
        X, l1, l1x = R.stft(x.astype(np.float64), n_fft, hop, frames)
        for prec in _precs(n_fft):
            check_stft(x, n_fft, hop, X, l1, l1x, frames, prec, "n_fft=%d hop=%d S=%d B=%d" % (n_fft, hop, S, B))
        if i in (0, len(lengths) - 1):                       # impulses, against the closed form (all frames)
            pos = R.impulse_positions(S, n_fft)
            x = np.zeros((len(pos), S), dtype=np.float32)
            x[np.arange(len(pos)), pos] = 1.0
            ref = [R.stft_of_impulse(p, S, n_fft, hop) for p in pos]
            X, l1, l1x = (np.stack([r[j] for r in ref]) for j in range(3))
            frames = np.arange(1 + S // hop)
            for prec in _precs(n_fft):
                check_stft(x, n_fft, hop, X, l1, l1x, frames, prec, "impulses %s n_fft=%d hop=%d S=%d" % (pos, n_fft, hop, S))


@pytest.mark.parametrize("n_fft,hop,S", [(400, 160, 1601), (6, 3, 4), (512, 1, 300), (1024, 1031, 5000), (2048, 3, 1031)])
def test_stft_batch_independent_and_deterministic(n_fft, hop, S):
    x = R.stft_signal(3, S, 5)
    x = np.concatenate([x, -x[:2] * 0.5])                   # B = 5
    for prec in _precs(n_fft):
        for cplx in (False, True):
            a = run_stft(x, n_fft, hop, prec, cplx)
            assert np.array_equal(a, run_stft(x, n_fft, hop, prec, cplx)), (prec, cplx)
            assert np.array_equal(a, run_stft(x, n_fft, hop, prec, cplx, captured=True)), (prec, cplx, "graph replay")
            for b in range(5):
                assert np.array_equal(a[b], run_stft(x[b:b + 1], n_fft, hop, prec, cplx)[0]), (prec, cplx, b)


# -------------------------------------------------------------------------------------------------------------- fir_same
def run_fir(wave, hbuf, B, S, Nh, stride):
    w = dev(wave, torch.float32)
    h = dev(hbuf, torch.float64)
    out = nan((B, S), torch.float64)
    ok(lib().alvq_fir_same_f64(w.data_ptr(), h.data_ptr(), out.data_ptr(), B, S, Nh, stride, stream()), "alvq_fir_same_f64")
    return host(out)


@pytest.mark.parametrize("S,Nh", R.FIR_CASES)
def test_fir_same_per_element(S, Nh):
    rng = np.random.default_rng(S * 8192 + Nh)
    B = 3
    wave = rng.standard_normal((B, S)).astype(np.float32)
    h = rng.standard_normal((B, Nh)) * np.exp(-np.arange(Nh) / max(1.0, Nh / 4.0))
    padded = np.full((B, Nh + 5), np.nan)                    # h_batch_stride = Nh + 5: the gap holds NaN, which must not be read
    padded[:, :Nh] = h
    for label, hbuf, stride, heff in [("shared", h[0], 0, h[0]), ("per-item", h, Nh, h), ("stride Nh+5", padded, Nh + 5, h)]:
        got = run_fir(wave, hbuf, B, S, Nh, stride)
        assert np.isfinite(got).all(), (label, S, Nh)
        ref, mag = R.fir_same(wave, heff)
        bound = (Nh + 1) * 2.0 ** -53 * mag.astype(np.float64)
        err = np.abs(got - ref)
        r = ratio(err, bound)
        _note(("fir_same", "f64"), r, "%s S=%d Nh=%d" % (label, S, Nh))
        assert (err <= bound).all(), "%s S=%d Nh=%d: error/bound %.3g" % (label, S, Nh, r)


# ------------------------------------------------------------------------------------------------------- spec_rir_wiener
def run_rir_wiener(Sc, Ec):
    B, F, T = Sc.shape
    s = dev(np.stack([Sc.real, Sc.imag], -1).astype(np.float32), torch.float32)
    e = dev(np.stack([Ec.real, Ec.imag], -1), torch.float64)
    sp, ep, rp = nan((B, F, T), torch.float32), nan((B, F, T), torch.float64), nan((B, F, T), torch.float64)
    wi, ws = nan((B, F), torch.float64), nan((B, F), torch.float64)
    ok(lib().alvq_spec_rir_wiener_f64(s.data_ptr(), e.data_ptr(), sp.data_ptr(), ep.data_ptr(), rp.data_ptr(), wi.data_ptr(),
                                      ws.data_ptr(), B, F, T, stream()), "alvq_spec_rir_wiener_f64")
    return [host(t).astype(np.float64) for t in (sp, ep, rp, wi)]


def check_rir_wiener(Sc, Ec, where):
    sp, ep, rp, wi = run_rir_wiener(Sc, Ec)
    for a in (sp, ep, rp, wi):
        assert np.isfinite(a).all(), where
    speech, echoed, rir, wiener, wscale = R.spec_rir_wiener(Sc, Ec)
    assert (np.abs(sp - speech) <= 2.0 ** -23 * speech).all(), where        # one float32 ulp at the bottom of a binade
    assert (np.abs(ep - echoed) <= 2.0 ** -51 * echoed).all(), where
    assert float(np.abs(rp - rir).max()) <= 1e-13, (where, float(np.abs(rp - rir).max()))
    assert float(rp.max()) <= 1.0 + 1e-15
    r = ratio(np.abs(wi - wiener), 1e-12 * wscale)
    _note(("spec_rir_wiener", "wiener"), r, where)
    assert (np.abs(wi - wiener) <= 1e-12 * wscale).all(), (where, r)


@pytest.mark.parametrize("F,T", R.RIR_CASES)
def test_spec_rir_wiener_per_bin(F, T):
    rng = np.random.default_rng(F * 1000 + T)
    B = 3
    Sc = (rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T))).astype(np.complex64)
    Sc *= np.array([1.0, 1e-6, 1e6], dtype=np.float32)[:, None, None]     # items far apart: max |r| must be per item
    Ec = rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T))
    if F > 1:                                  # a silent row (not a silent item: max |r| = 0 makes rir 0/0 in any restatement)
        Sc[0, F // 2] = 0                      # wiener = 0 / (0 + 1e-8) exactly
    check_rir_wiener(Sc, Ec, "F=%d T=%d" % (F, T))
    if F > 1:
        assert run_rir_wiener(Sc, Ec)[3][0, F // 2] == 0.0


# ----------------------------------------------------------------------------------------------------------------- iSTFT
def run_istft(spec, n_fft, hop, length, prec):
    """spec (B, F, T) complex numpy -> (rc, wave); wave and workspace pre-filled with NaN."""
    B, F, T = spec.shape
    sd = dev(np.stack([spec.real, spec.imag], -1), TDT[prec])
    wave = nan((B, length), TDT[prec])
    ws = nan((B, T, n_fft), TDT[prec])
    rc = getattr(lib(), "alvq_istft_" + prec)(sd.data_ptr(), wave.data_ptr(), ws.data_ptr(), B, T, n_fft, hop, length, stream())
    return rc, host(wave).astype(np.float64)


ISTFT_CASES = [(n, h) for n in R.ISTFT_NFFT for h in R.istft_hops(n)]


@pytest.mark.parametrize("n_fft,hop", ISTFT_CASES)
def test_istft_per_sample(n_fft, hop):
    checked = 0
    for T in R.ISTFT_T:
        for length in R.istft_lengths(n_fft, hop, T):
            where = "n_fft=%d hop=%d T=%d length=%d" % (n_fft, hop, T, length)
            if not R.istft_env_ok(n_fft, hop, T, length, 5e-12):        # the host NOLA check (1e-11) must refuse it
                for prec in (("f32", "f64") if n_fft <= 1024 else ("f32",)):
                    rc, got = run_istft(np.ones((1, n_fft // 2 + 1, T), dtype=np.complex128), n_fft, hop, length, prec)
                    assert rc == -1 and b"NOLA" in lib().alvq_last_error() and np.isnan(got).all(), (prec, where)
                continue
            if not R.istft_env_ok(n_fft, hop, T, length, 1e-6):
                continue                                      # ill-conditioned inversion: not a test of the kernel
            rng = np.random.default_rng(n_fft * 100 + hop * 10 + T + length)
            F = n_fft // 2 + 1
            spec = rng.standard_normal((2, F, T)) + 1j * rng.standard_normal((2, F, T))
            spec[1] *= 1e-3 * np.exp(-np.arange(F) / 8.0)[:, None]           # a quiet item with a steep spectrum
            for prec in (("f32", "f64") if n_fft <= 1024 else ("f32",)):
                s = spec.astype(np.complex64 if prec == "f32" else np.complex128)
                rc, got = run_istft(s, n_fft, hop, length, prec)
                ok(rc, where)
                assert np.isfinite(got).all(), (prec, where)
                y, A, Rw, W, _ = R.istft(s, n_fft, hop, length)
                nf = -(-n_fft // hop)
                bound = U[prec] * ((n_fft + 2 + nf) * A + Rw + 2 * np.abs(y) * W)
                err = np.abs(got - y)
                r = ratio(err, bound)
                _note(("istft", prec), r, where)
                assert r <= 1.0, "%s %s: error/bound %.3g" % (prec, where, r)
                if length > hop * (T - 1):
                    assert (got[:, hop * (T - 1) + n_fft // 2:] == 0).all(), (prec, where)
                # the imaginary parts at DC and Nyquist are ignored, bit for bit
                s2 = s.copy()
                s2[:, 0] = s2[:, 0].real + 1j * 1e3
                s2[:, -1] = s2[:, -1].real - 1j * 7.0
                assert np.array_equal(run_istft(s2, n_fft, hop, length, prec)[1], got), (prec, where)
                checked += 1
    assert checked > 0


@pytest.mark.parametrize("prec,n_fft,hop,T,bad", [
    ("f32", 2048, 1, 1, 1024),      # T = 1 reaching the frame's last sample: w[2047]^2 = 5.5e-12 < 1e-11
    ("f64", 1024, 1024, 2, 513),    # hop = n_fft: the envelope is w[0]^2 = 0 where the second frame starts
])
def test_istft_nola_rejected_on_the_host(prec, n_fft, hop, T, bad):
    """A length one sample longer than the envelope allows returns ALVQ_EINVAL and writes nothing; one sample shorter runs."""
    assert not R.istft_env_ok(n_fft, hop, T, bad, 1e-11) and R.istft_env_ok(n_fft, hop, T, bad - 1, 1e-11)
    spec = np.ones((1, n_fft // 2 + 1, T), dtype=np.complex128)
    rc, got = run_istft(spec, n_fft, hop, bad, prec)
    assert rc == -1 and b"NOLA" in lib().alvq_last_error()
    assert np.isnan(got).all()
    rc, got = run_istft(spec, n_fft, hop, bad - 1, prec)
    ok(rc, "n_fft=%d length=%d" % (n_fft, bad - 1))
    assert np.isfinite(got).all()


# ----------------------------------------------------------------------------------------------------------- Griffin-Lim
def _gl_problem(S, n_fft, hop, seed):
    t = np.arange(S) / 16000.0
    rng = np.random.default_rng(seed)
    x = np.sin(2 * np.pi * (200.0 + 900.0 * t) * t) + 0.05 * rng.standard_normal((2, S))
    mag = stft_oracle.stft_complex(torch.from_numpy(x), n_fft, hop).abs().contiguous()
    g = torch.Generator().manual_seed(seed)
    init = torch.rand(mag.shape, dtype=torch.complex128, generator=g)
    return mag, init


def _rel_l2(a, b):
    a, b = a.detach().cpu().to(torch.float64), b.detach().cpu().to(torch.float64)
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("hop", [256, 300])
@pytest.mark.parametrize("n_iter", [1, 4])
@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_griffin_lim_f64_at_the_f64_limit(hop, n_iter, momentum):
    S = 8000
    mag, init = _gl_problem(S, 1024, hop, hop + n_iter)
    got = N.griffin_lim(mag.cuda(), init.cuda(), n_iter, momentum, 1024, hop, S)
    want = GL.griffin_lim(mag, init, n_iter, momentum, 1024, hop, S)
    assert torch.isfinite(got).all() and _rel_l2(got, want) <= 1e-9, _rel_l2(got, want)


@pytest.mark.parametrize("n_iter", [1, 4])
@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_griffin_lim_f32_librosa_framing(n_iter, momentum):
    S = 22050
    mag, init = _gl_problem(S, 2048, 512, 3 + n_iter)
    got = N.griffin_lim(mag.float().cuda(), init.to(torch.complex64).cuda(), n_iter, momentum, 2048, 512, S)
    want = GL.griffin_lim(mag, init, n_iter, momentum, 2048, 512, S)
    assert torch.isfinite(got).all() and _rel_l2(got, want) <= 1e-4, _rel_l2(got, want)


# ------------------------------------------------------------------------------- batch count above the 65 535 y-grid size
BIG_B = 65537


def test_fir_same_batch_above_y_grid_limit():
    rng = np.random.default_rng(1)
    S, Nh = 4, 3
    wave = rng.standard_normal((BIG_B, S)).astype(np.float32)
    h = rng.standard_normal((BIG_B, Nh))
    got = run_fir(wave, h, BIG_B, S, Nh, Nh)
    assert np.isfinite(got).all(), "items left unwritten: %s" % np.unique(np.nonzero(~np.isfinite(got))[0])[:8]
    ref, mag = R.fir_same(wave, h)
    assert (np.abs(got - ref) <= (Nh + 1) * 2.0 ** -53 * mag).all()


def test_spec_rir_wiener_batch_above_y_grid_limit():
    rng = np.random.default_rng(2)
    shape = (BIG_B, 1, 1)
    Sc = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    Ec = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    check_rir_wiener(Sc, Ec, "B=%d F=T=1" % BIG_B)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_istft_batch_above_y_grid_limit(prec):
    rng = np.random.default_rng(3)
    spec = (rng.standard_normal((BIG_B, 3, 1)) + 1j * rng.standard_normal((BIG_B, 3, 1)))
    spec = spec.astype(np.complex64 if prec == "f32" else np.complex128)
    rc, got = run_istft(spec, 4, 1, 2, prec)
    ok(rc, "istft B=%d" % BIG_B)
    assert np.isfinite(got).all(), "items left unwritten: %s" % np.unique(np.nonzero(~np.isfinite(got))[0])[:8]
    y, A, Rw, W, _ = R.istft(spec, 4, 1, 2)
    assert (np.abs(got - y) <= U[prec] * (7 * A + Rw + 2 * np.abs(y) * W)).all()
