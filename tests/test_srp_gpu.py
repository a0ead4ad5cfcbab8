"""GCC-PHAT / SRP-PHAT localisation on the device (csrc/srp_phat.hip, acoustic_locating_vq_vae.localization) against the float64
restatement of tests/helpers/srp_ref.py, which tests/test_srp_cpu.py pins against np.longdouble to these same bounds.

Tolerances, with u = 1.1e-16 and Theta = 2 pi f_hi (fs / n_fft) max tau, the phase of the longest path at the top bin (a delay
is rounded relative to itself, not relative to the difference of two delays):
    cross-spectra  |psi_dev - psi_ref| <= (T + 8) u                       products of unit phasors averaged over T
    SRP map        |S_dev - S_ref|     <= (P F_band + T + 16 Theta + 32 + K) u   the summation of P F_band weighted terms of size
                                                                          at most w_f / (P W1), the psi error, the phase error,
                                                                          slack, and K = 8 for the kernel's rotation recurrence
                                                                          along f, re-anchored every 8 bins
    GCC            |r_dev - r_ref|     <= (F_band + T + 8 pi L + 32) u
About 6e-13 for the largest shape: a stray float32 accumulation sits five orders above it.  complex64 input: the restatement
of the promoted input (nothing is rounded on the way out: every output is float64)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import srp_ref as R  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import localization as LOC  # noqa: E402

GCC_LAGS = 8
IDS = ["-".join(str(v) for v in s) for s in R.PARITY]


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()          # a copy: the shared cases are read-only


def same_bits(a, b):
    """Two tensors equal bit for bit, NaN included."""
    ra, rb = (torch.view_as_real(t.contiguous()) if t.is_complex() else t.contiguous() for t in (a, b))
    if ra.shape != rb.shape or ra.dtype != rb.dtype:
        return False
    view = {torch.float64: torch.int64, torch.float32: torch.int32}.get(ra.dtype)
    return torch.equal(ra.view(view), rb.view(view)) if view else torch.equal(ra, rb)


def with_option(name, value, fn):
    prev = N.get_option(name)
    N.set_option(name, value)
    try:
        return fn()
    finally:
        N.set_option(name, prev)


def srp(X, c, shape, mics=None, cand=None):
    B, D, T, G, f_lo, f_hi, n_fft = shape
    return LOC.srp_phat(X, dev(c.mics) if mics is None else mics, dev(c.cand) if cand is None else cand, fs=R.FS, n_fft=n_fft,
                        c=R.C, band=(f_lo, f_hi))


# ------------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("shape", R.PARITY, ids=IDS)
@pytest.mark.parametrize("cdtype", [np.complex128, np.complex64], ids=["complex128", "complex64"])
def test_parity(shape, cdtype):
    B, D, T, G, f_lo, f_hi, n_fft = shape
    P, L = D * (D - 1) // 2, min(GCC_LAGS, n_fft // 2)
    c, ref = R.parity_case(shape), R.reference(shape, single=cdtype == np.complex64)
    X = dev(c.X.astype(cdtype))
    theta = R.theta_max(f_hi, R.FS, n_fft, c.mics, c.cand)
    b_psi, b_map, b_gcc = R.psi_bound(T), R.map_bound(D, T, f_lo, f_hi, theta), R.gcc_bound(T, f_lo, f_hi, L)

    psi = LOC.cross_spectra(X, band=(f_lo, f_hi))
    assert psi.dtype == torch.complex128 and psi.shape == (B, P, n_fft // 2 + 1)
    e_psi = float(np.abs(psi.cpu().numpy() - ref.psi).max())
    outside = np.ones(n_fft // 2 + 1, bool)
    outside[f_lo:f_hi + 1] = False
    assert not torch.view_as_real(psi).cpu().numpy()[:, :, outside].any()           # exactly 0 outside the band

    got = srp(X, c, shape)
    assert got.map.dtype == torch.float64 and got.map.shape == (B, G)
    assert got.best.dtype == torch.int32 and got.best.shape == (B,) and got.status.dtype == torch.int32 and got.status.shape == (B,)
    e_map = float(np.abs(got.map.cpu().numpy() - ref.map).max())

    gcc = LOC.gcc_phat(X, L, band=(f_lo, f_hi), n_fft=n_fft)
    assert gcc.corr.dtype == torch.float64 and gcc.corr.shape == (B, P, 2 * L + 1)
    assert gcc.lags.tolist() == list(range(-L, L + 1))
    e_gcc = float(np.abs(gcc.corr.cpu().numpy() - R.gcc_phat(ref.psi, n_fft, L, f_lo, f_hi)).max())

    print("%s %s: measured / bound: psi %.3g (bound %.3g), map %.3g (bound %.3g, Theta %.4g), gcc %.3g (bound %.3g)"
          % (np.dtype(cdtype).name, shape, e_psi / b_psi, b_psi, e_map / b_map, b_map, theta, e_gcc / b_gcc, b_gcc))
    assert e_psi <= b_psi and e_map <= b_map and e_gcc <= b_gcc
    assert not got.status.cpu().numpy().any()
    assert (ref.gap > 2 * b_map).all()                                              # the arg-max is beyond the rounding: no item is let off
    assert np.array_equal(got.best.cpu().numpy(), ref.best) and np.array_equal(ref.best, c.true)


def test_more_candidates_than_a_workgroup_holds():
    """1100 ring candidates, three workgroups of 512 an item: the map against the restatement, the arg-max, and a slice of the
    grid launched alone against the same candidates inside the full grid."""
    shape = (2, 3, 4, 1100, 8, 60, 400)
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c = R.case(B, D, T, G, 11)
    psi, st = R.cross_spectra(c.X, f_lo, f_hi)
    S, best, status = R.srp_phat(psi, c.mics, c.cand, R.FS, n_fft, R.C, f_lo, f_hi, spectrum_status=st)
    bound = R.map_bound(D, T, f_lo, f_hi, R.theta_max(f_hi, R.FS, n_fft, c.mics, c.cand))
    X = dev(c.X)
    got = srp(X, c, shape)
    err = float(np.abs(got.map.cpu().numpy() - S).max())
    print("%s: measured / bound: map %.3g (bound %.3g)" % (shape, err / bound, bound))
    assert err <= bound and not got.status.cpu().numpy().any()
    top = np.sort(S, axis=1)[:, ::-1]
    assert (top[:, 0] - top[:, 1] > 2 * bound).all()
    assert np.array_equal(got.best.cpu().numpy(), best)
    part = srp(X, c, shape, cand=dev(c.cand[500:530]))
    assert same_bits(part.map, got.map[:, 500:530])


# ------------------------------------------------------------------------------------------------------------------- status
@pytest.mark.parametrize("cdtype", [np.complex128, np.complex64], ids=["complex128", "complex64"])
def test_silent_and_non_finite_items(cdtype):
    """One launch holds a silent item, an item with one NaN inside the band, a healthy item with a NaN outside the band, an
    item with a NaN microphone coordinate and an untouched one."""
    shape = R.PARITY[1]
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c = R.parity_case(shape)
    X = np.concatenate([c.X, c.X, c.X[:1]]).astype(cdtype)
    X[0, :, f_lo:f_hi + 1] = 0
    X[1, 1, f_lo + 3, 2] = complex(1.0, np.nan)
    X[2, 0, f_hi + 1, 0] = np.nan
    mics = np.broadcast_to(c.mics, (5, D, 3)).copy()
    mics[3, 1, 2] = np.nan
    psi, st = R.cross_spectra(X.astype(np.complex128), f_lo, f_hi)
    S, best, status = R.srp_phat(psi, mics, c.cand, R.FS, n_fft, R.C, f_lo, f_hi, spectrum_status=st)
    assert list(status) == [2, 1, 0, 4, 0]
    got = srp(dev(X), c, shape, mics=dev(mics))
    m = got.map.cpu().numpy()
    assert got.status.tolist() == [2, 1, 0, 4, 0] and got.best.tolist() == [-1, -1, int(best[2]), -1, int(best[4])]
    assert not m[0].any() and np.isnan(m[1]).all() and np.isnan(m[3]).all()
    bound = R.map_bound(D, T, f_lo, f_hi, R.theta_max(f_hi, R.FS, n_fft, c.mics, c.cand))
    err = float(np.abs(m[[2, 4]] - S[[2, 4]]).max())
    print("the healthy neighbours, %s: measured / bound %.3g" % (np.dtype(cdtype).name, err / bound))
    assert err <= bound
    # a non-finite candidate flags every item that sees the grid
    cand = c.cand.copy()
    cand[G - 1, 1] = np.inf
    bad = srp(dev(X), c, shape, mics=dev(mics), cand=dev(cand))
    assert bad.status.tolist() == [6, 5, 4, 4, 4] and bad.best.tolist() == [-1] * 5 and bool(torch.isnan(bad.map).all())


# ------------------------------------------------------------------------------------------------ repeatability, isolation
@pytest.mark.parametrize("shape", [R.PARITY[3], R.PARITY[6], R.PARITY[1]], ids=[IDS[3], IDS[6], IDS[1]])
def test_launches_repeat_and_items_and_candidates_do_not_see_each_other(shape):
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c = R.parity_case(shape)
    X = dev(c.X)
    runs = {}
    for lds in (1, 0):                                   # rows / the psi band in LDS where they fit, and always re-read
        def run(lds=lds):
            first, second = srp(X, c, shape), srp(X, c, shape)
            psi = LOC.cross_spectra(X, band=(f_lo, f_hi))
            assert same_bits(first.map, second.map) and torch.equal(first.best, second.best) and torch.equal(first.status, second.status)
            assert same_bits(psi, LOC.cross_spectra(X, band=(f_lo, f_hi)))
            for b in range(B):                           # an item alone
                alone = srp(X[b:b + 1], c, shape)
                assert same_bits(alone.map[0], first.map[b]) and int(alone.best[0]) == int(first.best[b])
                assert same_bits(LOC.cross_spectra(X[b:b + 1], band=(f_lo, f_hi))[0], psi[b])
            one = srp(X, c, shape, cand=dev(c.cand[G // 2:G // 2 + 1]))          # a candidate alone
            assert same_bits(one.map[:, 0], first.map[:, G // 2])
            lo, hi = G // 3, G // 3 + max(1, G // 4)
            part = srp(X, c, shape, cand=dev(c.cand[lo:hi]))                      # a slice of the grid
            assert same_bits(part.map, first.map[:, lo:hi])
            return psi, first
        runs[lds] = with_option("phat_lds", lds, run)
    assert same_bits(runs[1][0], runs[0][0]) and same_bits(runs[1][1].map, runs[0][1].map)      # both paths: the same bits
    assert torch.equal(runs[1][1].best, runs[0][1].best)
    view = dev(np.ascontiguousarray(c.X.transpose(0, 1, 3, 2))).transpose(2, 3)                 # a strided (B, D, F, T) view
    assert not view.is_contiguous() and same_bits(srp(view, c, shape).map, runs[1][1].map)
    assert same_bits(LOC.cross_spectra(view, band=(f_lo, f_hi)), runs[1][0])
    assert same_bits(LOC.cross_spectra(X.conj(), band=(f_lo, f_hi)), LOC.cross_spectra(X.conj().resolve_conj(), band=(f_lo, f_hi)))


def test_ranks_and_broadcast_geometry():
    shape = R.PARITY[1]
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c = R.parity_case(shape)
    X, mics, cand = dev(c.X), dev(c.mics), dev(c.cand)
    shared = srp(X, c, shape)
    each = srp(X, c, shape, mics=mics[None].expand(B, D, 3), cand=cand[None].expand(B, G, 3).contiguous())
    mixed = srp(X, c, shape, mics=mics[None].expand(B, D, 3).contiguous(), cand=cand)
    for other in (each, mixed):
        assert same_bits(other.map, shared.map) and torch.equal(other.best, shared.best) and torch.equal(other.status, shared.status)
    one = srp(X[1], c, shape)
    assert one.map.shape == (G,) and one.best.shape == () and one.status.shape == ()
    assert same_bits(one.map, shared.map[1]) and int(one.best) == int(shared.best[1]) and int(one.status) == 0
    psi = LOC.cross_spectra(X, band=(f_lo, f_hi))
    assert same_bits(LOC.cross_spectra(X[1], band=(f_lo, f_hi)), psi[1])
    gcc = LOC.gcc_phat(X, 5, band=(f_lo, f_hi))
    assert same_bits(LOC.gcc_phat(X[1], 5, band=(f_lo, f_hi)).corr, gcc.corr[1])
    assert LOC.tdoa(X, 5, band=(f_lo, f_hi)).shape == (B, 3) and LOC.tdoa(X[1], 5, band=(f_lo, f_hi)).shape == (3,)
    # the default band leaves out DC and Nyquist
    assert same_bits(LOC.cross_spectra(X), LOC.cross_spectra(X, band=(1, n_fft // 2 - 1)))


def test_lowest_index_wins():
    shape = R.PARITY[2]
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c = R.parity_case(shape)
    k = int(c.true[0])
    other = [g for g in range(G) if g != k]
    order = other[:3] + [k] + other[3:40] + [k] + other[40:] + [k]          # the best candidate three times
    got = srp(dev(c.X), c, shape, cand=dev(c.cand[order]))
    assert int(got.best[0]) == 3
    assert same_bits(got.map[0, 3], got.map[0, 41]) and same_bits(got.map[0, 3], got.map[0, len(order) - 1])


def test_lowest_index_wins_across_trips_lanes_and_waves():
    """600 candidates for the arg-max's 256 threads: every entry is the restatement's worst candidate but for copies of its
    best one, placed so that the thread's own loop, the butterfly and the combine over the waves would each answer
    differently under another tie rule.  (260, 200, 590): index 200 is thread 200 of wave 3, index 260 thread 4 of wave 0 on
    its second trip, so a combine that prefers the lower wave or thread says 260.  (556, 300): both in thread 44, trips 2 and 1.
    On the host the best beats the worst by more than twice the map's bound: the tie is among the copies only."""
    shape = (1, 3, 4, 600, 8, 60, 400)
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c = R.case(B, D, T, G, 11)
    psi, st = R.cross_spectra(c.X, f_lo, f_hi)
    S, _, status = R.srp_phat(psi, c.mics, c.cand, R.FS, n_fft, R.C, f_lo, f_hi, spectrum_status=st)
    good, poor = int(np.argmax(S[0])), int(np.argmin(S[0]))
    bound = R.map_bound(D, T, f_lo, f_hi, R.theta_max(f_hi, R.FS, n_fft, c.mics, c.cand))
    print("%s: best %.6g, worst %.6g, bound %.3g" % (shape, S[0, good], S[0, poor], bound))
    assert not status.any() and S[0, good] - S[0, poor] > 2 * bound
    X = dev(c.X)
    for copies, want in (((260, 200, 590), 200), ((556, 300), 300)):
        grid = np.tile(c.cand[poor], (G, 1))
        grid[list(copies)] = c.cand[good]
        got = srp(X, c, shape, cand=dev(grid))
        assert int(got.status[0]) == 0 and int(got.best[0]) == want, (copies, int(got.best[0]))
        assert all(same_bits(got.map[0, copies[0]], got.map[0, g]) for g in copies[1:])


# --------------------------------------------------------------------------------------------------------------------- tdoa
def test_tdoa_of_a_free_field_pair():
    """Two microphones, no room, no noise: the delay is within half a sample of (r_i - r_j) / c (interpolation cannot do better
    than the band allows; half a sample is the integer-lag guarantee), with the sign of alvq_gcc_phat_f64."""
    n_fft, F, T = 400, 201, 6
    g = np.random.default_rng(11)
    mics = np.array([[2.5, 1.5, 1.5], [2.5, 1.8, 1.5]])
    X, want = [], []
    for src in ([3.5, 3.0, 1.5], [1.0, 0.5, 2.0], [3.0, 1.65, 1.0]):
        r = np.linalg.norm(np.array(src) - mics, axis=1)
        S = g.standard_normal((F, T)) + 1j * g.standard_normal((F, T))
        omega = 2 * np.pi * np.arange(F) * R.FS / n_fft
        X.append(np.stack([S * np.exp(-1j * omega * rd / R.C)[:, None] / rd for rd in r]))
        want.append((r[0] - r[1]) / R.C)
    got = LOC.tdoa(dev(np.stack(X)), 20, fs=R.FS, band=(1, 199))
    assert got.dtype == torch.float64 and got.shape == (3, 1)
    err = np.abs(got.cpu().numpy()[:, 0] - np.array(want)) * R.FS
    print("tdoa: wanted %s samples, error %s samples" % (np.array(want) * R.FS, err))
    assert (err <= 0.5).all()
    edge = LOC.tdoa(dev(np.stack(X)), 4, fs=R.FS, band=(1, 199))             # the peak outside the lags: no interpolation
    assert bool(torch.isfinite(edge).all()) and float(edge.abs().max()) <= 4 / R.FS


# ----------------------------------------------------------------------------------------------------------------- the room
def test_locate_on_ring_in_the_room():
    """The room case of tests/test_srp_cpu.py on the device, all four angles in one batch: array_impulse_responses ->
    array_spectrograms -> locate_on_ring."""
    cfg = FE.DATASET_CONFIG
    fs, n = cfg["fs"], 16000
    g = np.random.default_rng(3)
    t = np.arange(n) / fs
    envelope = (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + 0.3)) * (0.6 + 0.4 * np.sin(2 * np.pi * 1.3 * t))
    wave = dev((g.standard_normal(n) * envelope).astype(np.float32))[None].expand(4, n).contiguous()
    rcv = np.array(cfg["receiver_position"], dtype=np.float64)
    mics = dev(rcv + 0.05 / np.sqrt(3.0) * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64))
    angles = [5, 23, 40, 61]
    theta_grid, points = LOC.ring_candidates(72, cfg["receiver_position"], cfg["room_dimensions"], cfg["R"], cfg["Z_LOC_SOURCE"])
    assert theta_grid.shape == (72,) and points.shape == (72, 3) and abs(float(theta_grid[0]) + np.pi) < 1e-15
    assert same_bits(points, FE.source_positions(theta_grid, cfg["receiver_position"], cfg["room_dimensions"], cfg["R"],
                                                 cfg["Z_LOC_SOURCE"]))
    src = points[angles].contiguous()
    h = FE.array_impulse_responses(src, mics, cfg["room_dimensions"], reverberation_time=cfg["reverberation_time"],
                                   nsample=cfg["n_sample"])
    assert h.shape == (4, 4, cfg["n_sample"]) and h.dtype == torch.float64
    for b in range(4):                                   # per-microphone rir_generate, bit for bit
        want = FE.rir_generate(FE.SOUND_SPEED, fs, mics.cpu().numpy(), src[b].cpu().numpy(), cfg["room_dimensions"],
                               reverberation_time=cfg["reverberation_time"], nsample=cfg["n_sample"])
        assert same_bits(h[b], want.t())
    each = FE.array_impulse_responses(src, mics[None].expand(4, 4, 3), cfg["room_dimensions"],
                                      reverberation_time=cfg["reverberation_time"], nsample=cfg["n_sample"])
    assert same_bits(each, h)
    spec = FE.array_spectrograms(wave, h)
    assert spec.shape == (4, 4, 201, 101) and spec.dtype == torch.complex128
    assert same_bits(spec[2, 1], N.stft_complex(N.fir_same(wave[2:3], h[2, 1:2].contiguous()))[0])
    ring = LOC.locate_on_ring(spec, mics, cfg["receiver_position"], cfg["room_dimensions"], cfg["R"], cfg["Z_LOC_SOURCE"],
                              n_angles=72, band=(8, 187))
    assert ring.theta.shape == (4,) and ring.source.shape == (4, 3) and ring.map.shape == (4, 72) and ring.status.shape == (4,)
    found = torch.round((ring.theta + np.pi) / (2 * np.pi / 72)).to(torch.int64).tolist()
    print("sources on candidates %s: arg-max %s, peaks %s" % (angles, found, ring.map.amax(dim=1).tolist()))
    assert ring.status.tolist() == [0, 0, 0, 0]
    for k, f in zip(angles, found):
        assert same_bits(ring.source[angles.index(k)], points[f])
        assert min((f - k) % 72, (k - f) % 72) <= 1
