"""CPU-side checks of the inverse STFT / Griffin-Lim entry points (csrc/istft.hip): argument errors return ALVQ_EINVAL with a
message and launch nothing, the workspace size is the documented formula, and the CPU restatement the GPU tests compare
against (tests/helpers/griffin_lim_ref.py) inverts the forward oracle."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import griffin_lim_ref as GL  # noqa: E402
from oracle import stft_oracle  # noqa: E402

EINVAL = -1
FAKE = 0x1000           # a non-null pointer: every call below must fail its host checks before touching it


@pytest.fixture(scope="module")
def native():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native
    return _native


def _istft(lib, dt, spec=FAKE, wave=FAKE, ws=FAKE, B=1, T=11, n_fft=400, hop=160, length=1600):
    return getattr(lib, "alvq_istft_" + dt)(spec, wave, ws, B, T, n_fft, hop, length, None)


def _gl(lib, dt, mag=FAKE, ang=FAKE, wave=FAKE, ws=FAKE, B=1, T=11, n_fft=400, hop=160, length=1600, n_iter=2, momentum=0.99):
    return getattr(lib, "alvq_griffin_lim_" + dt)(mag, ang, wave, ws, B, T, n_fft, hop, length, n_iter, momentum, None)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_argument_errors_do_not_launch(native, dt):
    lib = native.lib()
    cases = [
        (dict(spec=None), b"null"),
        (dict(wave=None), b"null"),
        (dict(ws=None), b"null"),
        (dict(n_fft=401), b"bad dims"),
        (dict(n_fft=2), b"bad dims"),
        (dict(n_fft=4096 if dt == "f32" else 2048, T=3, length=2 * 160), b"too large"),
        (dict(hop=500, length=5000), b"NOLA"),          # hop > n_fft: gaps between frames
        (dict(hop=400, length=4000), b"NOLA"),          # hop == n_fft: the periodic Hann window is 0 at every frame start
        (dict(length=0), b"bad dims"),
    ]
    for kw, msg in cases:
        assert _istft(lib, dt, **kw) == EINVAL, kw
        assert msg in lib.alvq_last_error(), (kw, lib.alvq_last_error())
        gkw = {{"spec": "mag"}.get(k, k): v for k, v in kw.items()}
        assert _gl(lib, dt, **gkw) == EINVAL, kw
        assert msg in lib.alvq_last_error(), (kw, lib.alvq_last_error())
    for kw, msg in [(dict(ang=None), b"null"), (dict(momentum=1.0), b"momentum"), (dict(momentum=-0.1), b"momentum"),
                    (dict(n_iter=-1), b"n_iter"), (dict(length=1601 + 160), b"frames")]:
        assert _gl(lib, dt, **kw) == EINVAL, kw
        assert msg in lib.alvq_last_error(), (kw, lib.alvq_last_error())


def test_workspace_formula(native):
    lib = native.lib()
    for B, T, n_fft in [(1, 11, 400), (64, 501, 400), (3, 40, 2048), (2, 5, 4)]:
        F = n_fft // 2 + 1
        for eb in (4, 8):
            got = lib.alvq_griffin_lim_workspace_bytes(B, T, n_fft, eb)
            assert got > 0 and got == (4 * B * F * T + B * T * n_fft) * eb
    assert lib.alvq_griffin_lim_workspace_bytes(0, 11, 400, 4) == -1
    assert lib.alvq_griffin_lim_workspace_bytes(1, 11, 401, 4) == -1
    assert lib.alvq_griffin_lim_workspace_bytes(1, 11, 400, 2) == -1


def test_cpu_tensors_rejected(native):
    with pytest.raises(RuntimeError, match="GPU"):
        native.istft(torch.zeros(1, 201, 11, dtype=torch.complex64))
    with pytest.raises(RuntimeError, match="GPU"):
        native.griffin_lim(torch.zeros(1, 201, 11), torch.zeros(1, 201, 11, dtype=torch.complex64), 2, 0.9, 400, 160, 1600)
    from acoustic_locating_vq_vae import front_end as FE
    with pytest.raises(RuntimeError, match="GPU"):
        FE.istft(torch.zeros(1, 201, 11, dtype=torch.complex64))
    with pytest.raises(RuntimeError, match="GPU"):
        FE.griffin_lim(torch.zeros(1, 201, 11))


def test_front_end_argument_checks(native):
    from acoustic_locating_vq_vae import front_end as FE
    with pytest.raises(ValueError, match="frequency bins"):
        FE.griffin_lim(torch.zeros(1, 200, 11))
    with pytest.raises(ValueError, match="momentum"):
        FE.griffin_lim(torch.zeros(1, 201, 11), momentum=1.0)
    with pytest.raises(ValueError, match="n_iter"):
        FE.griffin_lim(torch.zeros(1, 201, 11), n_iter=-1)


@pytest.mark.parametrize("S,n_fft,hop,length", [(16000, 400, 160, None), (16037, 400, 160, 16037), (8000, 2048, 512, 8000)])
def test_restatement_inverts_the_forward_oracle(S, n_fft, hop, length):
    g = torch.Generator().manual_seed(S)
    x = torch.randn(2, S, generator=g, dtype=torch.float64)
    spec = stft_oracle.stft_complex(x, n_fft, hop)
    y = GL.istft(spec, n_fft, hop, length)
    n = y.shape[-1]
    assert n == (length or hop * (spec.shape[-1] - 1))
    assert float((y - x[:, :n]).abs().max() / x.abs().max()) < 1e-13
    # and Griffin-Lim from the true phase of a consistent spectrogram stays there
    ang = spec / (spec.abs() + 1e-16)
    z = GL.griffin_lim(spec.abs(), ang, 3, 0.99, n_fft, hop, n)
    assert float((z - x[:, :n]).abs().max() / x.abs().max()) < 1e-9
