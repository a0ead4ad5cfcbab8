"""Room-acoustic parameters, the parts that need no GPU: the float64 restatement (tests/helpers/room_acoustics_ref.py) pinned
on decays whose answer is known in closed form, and the host-side rules of acoustic_locating_vq_vae.room_acoustics."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import room_acoustics_ref as RA  # noqa: E402
from acoustic_locating_vq_vae import room_acoustics as M  # noqa: E402


@pytest.mark.parametrize("T60", [0.05, 0.1])
def test_restatement_on_an_exponential_decay(T60):
    """h[t] = +-exp(-a t), a = 3 ln10 / (T60 fs): the level falls by exactly 60 dB in T60, so every decay time is T60 (the
    truncation at n = 4096 bends the curve by < 1e-11 dB inside the fit ranges) and c50 is a ratio of geometric series."""
    r = RA.parameters(RA.analytic_decay(T60), 16000.0)
    assert r.onset == 0 and r.status == 0
    for name in ("t30", "t20", "edt"):
        assert abs(getattr(r, name) / T60 - 1.0) <= 1e-9, (name, getattr(r, name))
    assert abs(r.c50 - RA.analytic_c50(T60)) <= 1e-9
    assert 0.0 < r.d50 < 1.0 and np.isfinite(r.c80) and np.isfinite(r.drr)


def test_restatement_status_rows():
    nan_row = RA.analytic_decay(0.05)
    nan_row[7] = np.nan
    impulse = np.zeros(100)
    impulse[40] = -2.0
    for row, onset in ((np.zeros(100), 0), (nan_row, 7)):
        r = RA.parameters(row)
        assert r.status == RA.BAD_ENERGY and r.onset == onset and all(np.isnan(r[i]) for i in range(7))
        assert np.isnan(RA.edc_db(row)).all()
    r = RA.parameters(impulse)
    assert r.status == RA.SHORT_RANGE | RA.NO_LATE_ENERGY and r.onset == 40
    assert np.isnan([r.t30, r.t20, r.edt]).all() and r.c50 == r.c80 == r.drr == np.inf and r.d50 == 1.0
    e = RA.edc_db(impulse)
    assert (e[:41] == 0.0).all() and np.isneginf(e[41:]).all()


def test_sample_counts():
    assert M.sample_counts(16000) == RA.sample_counts(16000.0) == (800, 1280, 40)
    assert M.sample_counts(44100) == (2205, 3528, 110)


def test_host_side_rejections():
    h = torch.zeros(2, 64, dtype=torch.float64)
    for call in (M.energy_decay_curve, M.room_acoustic_parameters, M.reverberation_time):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(h)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(h[0].float())
        for bad in (torch.zeros(2, 3, 64), torch.zeros(()), torch.zeros(2, 1), torch.zeros(0, 64), np.zeros((2, 64)),
                    torch.zeros(2, 64, dtype=torch.float16), torch.zeros(2, 64, dtype=torch.int32)):
            with pytest.raises(ValueError):
                call(bad)
    for call in (M.room_acoustic_parameters, M.reverberation_time):
        for fs in (0, -16000.0, float("nan"), float("inf"), "16000", None):
            with pytest.raises(ValueError, match="fs"):
                call(h, fs=fs)
    with pytest.raises(ValueError, match="method"):
        M.reverberation_time(h, method="t60")


def test_entry_points_check_their_arguments_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from acoustic_locating_vq_vae import _native as N
    lib = N.lib()
    p = 4096            # never dereferenced: every call below is rejected first
    for sfx in ("f32", "f64"):
        edc, ra = getattr(lib, "alvq_edc_" + sfx), getattr(lib, "alvq_room_acoustics_" + sfx)
        for args in ((None, p, 1, 8), (p, None, 1, 8), (p, p, 0, 8), (p, p, 1, 1), (p, p, 1, (1 << 24) + 1)):
            assert edc(*args, None) == -1 and lib.alvq_last_error().startswith(b"alvq_edc_" + sfx.encode())
        good = [p, p, p, p, 1, 8, 16000.0, 800, 1280, 40]
        for pos, bad in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, 1), (6, 0.0), (6, -1.0), (6, float("nan")),
                         (7, -1), (8, -1), (9, -1)):
            args = list(good)
            args[pos] = bad
            assert ra(*args, None) == -1, (sfx, pos, bad)
            assert lib.alvq_last_error().startswith(b"alvq_room_acoustics_" + sfx.encode())
