"""The cases of tests/helpers/signal_edge_cases.py on the host: the conditions each case is there for (which code path of
csrc/rir.hip, speech_metrics.hip or wpe.hip it reaches), the measured constants the helper records (K_REF, HP_REF, the STOI
rows' kept frames), and that each GPU test's checking function fails on a deliberately wrong restatement of the defect its
cases were chosen for.  Nothing here touches the device or its code."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import rir_ref as RR  # noqa: E402
import signal_edge_cases as E  # noqa: E402
import speech_metrics_ref as SR  # noqa: E402
import wpe_ref as WR  # noqa: E402


def receivers(name):
    return range(len(E.RIR_CASES[name].r))


def restated(case, m, **kw):
    return RR.rir(case.c, case.fs, case.r[m], case.s, case.L, case.beta, case.nsample, case.order, case.dim, **kw)


def twin(case, m, **kw):
    return RR.rir_ld(case.c, case.fs, case.r[m], case.s, case.L, case.beta, case.nsample, case.order, case.dim, **kw)


# ============================================================================================================ room responses
def test_window_lengths_and_rate_limits():
    Tw = {name: RR.window_length(E.RIR_CASES[name].fs) for name in ("fs250", "fs8000", "fs44100", "fs48000", "fs128000")}
    assert Tw == {"fs250": 2, "fs8000": 64, "fs44100": 352, "fs48000": 384, "fs128000": 1024}
    assert Tw["fs44100"] % 64 != 0 and Tw["fs48000"] > 256 and Tw["fs48000"] // 2 > 64
    assert [RR.window_length(fs) for fs in E.RIR_BAD_RATES] == [0, 1032]
    for name in Tw:
        assert 1000 <= len(E.rir_images(E.RIR_CASES[name])[0]) <= 12000, name


@pytest.mark.parametrize("name", [n for n in E.RIR_CASES if n != "hp8193"])
def test_reference_is_the_restatement_bit_for_bit(name):
    case = E.RIR_CASES[name]
    for m in receivers(name):
        assert np.array_equal(E.rir_reference(name, m).h, restated(case, m, hp_filter=False))
    if case.hp:
        assert np.array_equal(E.rir_reference_highpassed(name), restated(case, 0, hp_filter=True))


def test_measured_k_ref_and_highpass_distance():
    """K_REF: the float64 restatement against its longdouble twin over the cases (hp4097 and hp8193 left out: hp4096's room
    again, and 12 s).  HP_REF: the float64 recurrence against its twin on the same unfiltered response, the three high-pass
    cases.  The recorded values may be up to twice the measured ones: numpy's cos and sinc differ in the last bit between
    processors."""
    k_ref, hp_ref = 0.0, 0.0
    for name, case in E.RIR_CASES.items():
        if name in ("hp4097", "hp8193"):             # hp4096's room and images, one and 4097 samples further
            continue
        for m in receivers(name):
            ref = E.rir_reference(name, m)
            reached = ref.N > 0
            if not reached.any():
                continue
            k = float((np.abs(ref.h - twin(case, m, hp_filter=False))[reached] / (E.U53 * ref.A[reached])).max())
            print("%s receiver %d: K_ref %.3g" % (name, m, k))
            k_ref = max(k_ref, k)
    for name in ("hp4096", "hp4097", "hp8193"):
        h = E.rir_reference(name).h
        a = E.rir_reference_highpassed(name)
        hp = float(np.abs(a - RR.highpass_ld(h, E.RIR_CASES[name].fs)).max() / np.abs(a).max())
        print("%s: high-pass float64 - longdouble = %.3g max |h|" % (name, hp))
        hp_ref = max(hp_ref, hp)
    print("K_ref %.4g (recorded %.4g, device K %.4g); high-pass %.3g (recorded %.3g, bar %.3g)"
          % (k_ref, E.K_REF, E.K_DEVICE, hp_ref, E.HP_REF, E.HP_RTOL))
    assert 0.5 * E.K_REF <= k_ref <= E.K_REF and E.K_DEVICE == 4.0 * E.K_REF
    assert 0.5 * E.HP_REF <= hp_ref <= E.HP_REF and E.HP_RTOL == max(1e-12, 4.0 * E.HP_REF)


def test_short_rows():
    for ns in (1, 2):           # floor(d) < nsample keeps no image of this room: the response is exactly zero
        for order in (-1, 0):
            ref = E.rir_reference("short%d_order%d" % (ns, order))
            assert not ref.N.any() and not ref.h.any()
    for ns in (63, 64, 65):
        assert E.rir_reference("short%d_order0" % ns).N.max() == 1 and E.rir_reference("short%d_order-1" % ns).N.max() == 7


def test_exact_geometry():
    case = E.RIR_CASES["exact700"]
    assert case.c / case.fs == E.CTS_EXACT
    d, _ = E.rir_images(case, 0)
    assert len(d) == 12953 and int((d == np.floor(d)).sum()) == 68
    for m, offset in ((1, 64), (2, 63), (3, 62)):        # the q = 1 images on the source's y and z: |128 m_x - offset|
        d, _ = E.rir_images(case, m)
        whole = set(d[d == np.floor(d)].astype(int).tolist())
        want = {abs(128 * mx - offset) for mx in range(-6, 7) if abs(128 * mx - offset) < 700}
        assert want <= whole and len(want) >= 5, (m, sorted(want - whole))
        assert {v % 64 for v in want} == {offset % 64, (-offset) % 64}
    seen = set()
    for m in receivers("exact700"):
        d, _ = E.rir_images(case, m)
        seen |= {int(v) % 64 for v in d[d == np.floor(d)]}
    assert {0, 1, 2, 62, 63} <= seen                      # on and next to every tile's fd_lo = t0 - 64 and fd_hi = t1 - 2 + 64
    # nsample = 192: an image exactly at 191 is kept, one exactly at 192 is dropped
    short = E.RIR_CASES["exact192"]
    kept = np.concatenate([E.rir_images(short, m)[0] for m in receivers("exact192")])
    wider = np.concatenate([E.rir_images(short, m, 193)[0] for m in receivers("exact192")])
    assert (kept == 191.0).any() and not (kept >= 192.0).any() and (wider == 192.0).any()
    # the lone image: 40 samples away, and nothing else
    d, g = E.rir_images(E.RIR_CASES["exact_lone"])
    assert d.tolist() == [40.0] and g[0] == 1.0 / (4.0 * np.pi * 0.625)
    ref = E.rir_reference("exact_lone")
    assert ref.h[40] == g[0] and np.count_nonzero(ref.N) == 40 + 64 + 1          # the window 40 - 63 .. 40 + 64, cut at 0


def test_image_grid_shapes():
    def ranges(case):
        Ls = np.asarray(case.L) / (case.c / case.fs)
        return [int(np.ceil(case.nsample / (2.0 * Ls[a]))) for a in range(3)]
    n = ranges(E.RIR_CASES["flat_z"])
    assert n[2] == 149 and (2 * n[0] + 1) * 2 * (2 * n[1] + 1) * 2 == 100       # hundreds of m_z in each of 100 columns
    n = ranges(E.RIR_CASES["flat_x"])
    assert n[0] == 149 and (2 * n[0] + 1) * 2 * (2 * n[1] + 1) * 2 == 5980 > 4 * 256 and n[2] == 2
    d, _ = E.rir_images(E.RIR_CASES["near"])
    assert np.floor(d.min()) == 0 and 0 < d.min() < 1


def test_walls():
    assert E.RIR_CASES["rigid_plus"].beta == [1.0] * 6 and E.RIR_CASES["rigid_minus"].beta == [-1.0] * 6
    assert E.RIR_CASES["one_dead_wall"].beta.count(0.0) == 1
    _, g = E.rir_images(E.RIR_CASES["one_dead_wall"])
    assert (g == 0.0).any() and (g != 0.0).sum() > 1000                         # 0^0 = 1 keeps the images that miss the wall
    d, g = E.rir_images(E.RIR_CASES["dim2_order0"])
    assert len(d) == 1 and g[0] > 0                                              # beta_z = 0 and the direct path: 0^0 again
    assert np.array_equal(E.rir_reference("order1000").h, E.rir_reference("order_all").h)


# ------------------------------------------------------------------------------------------------- does the net hold: rooms
def test_the_restatement_passes_its_own_check():
    for name in ("fs48000", "exact192", "short64_order-1"):
        assert E.check_rir(E.rir_reference(name).h, E.rir_reference(name)) == 0.0


@pytest.mark.parametrize("name,which", [("fs48000", "table_off"), ("fs128000", "table_off"), ("fs8000", "fd_lo"),
                                        ("exact700", "fd_lo"), ("exact192", "keep_nsample"), ("fs8000", "keep_nsample")])
def test_rir_check_sees_the_defect(name, which):
    wrong = E.rir_mutant(name, which)
    assert not np.array_equal(wrong, E.rir_reference(name).h)
    with pytest.raises(AssertionError):
        E.check_rir(wrong, E.rir_reference(name))


def test_rir_check_sees_a_sample_that_should_be_zero():
    ref = E.rir_reference("exact_lone")
    wrong = ref.h.copy()
    wrong[150] = 1e-300
    with pytest.raises(AssertionError):
        E.check_rir(wrong, ref)


def test_highpass_check_sees_a_state_lost_at_the_chunk_edge():
    """The recurrence restarted from zero state at sample 4096."""
    h, fs = E.rir_reference("hp4097").h, E.RIR_CASES["hp4097"].fs
    wrong = np.concatenate([RR.highpass(h[:4096], fs), RR.highpass(h[4096:], fs)])
    with pytest.raises(AssertionError):
        E.check_rir_highpassed(wrong, E.rir_reference_highpassed("hp4097"))
    assert E.check_rir_highpassed(E.rir_reference_highpassed("hp4097"), E.rir_reference_highpassed("hp4097")) == 0.0


# ===================================================================================================================== STOI
@pytest.mark.parametrize("n", E.STOI_N)
def test_stoi_rows(n):
    refs = E.stoi_reference(n)
    frames = (n - SR.N_FRAME) // SR.HOP + 1
    assert frames == {32896: 256, 33024: 257, 50000: 389, 77056: 601}[n]
    assert [(r.kept_frames, r.status) for r in refs] == E.STOI_EXPECT[n]
    for r in refs:
        assert r.nf == frames and r.margin >= E.MIN_MARGIN_DB
    assert refs[0].kept_frames == frames                                        # (a) keeps every frame
    clean, _ = E.stoi_rows(n)
    level = 20.0 * np.log10(np.sqrt(np.sum((SR.frames(clean[1]) * SR.window()) ** 2, axis=1)) + SR.EPS)
    keep_b = level > level.max() - SR.DYN_RANGE_DB
    assert not keep_b[:E.STOI_TILE].all() and keep_b[:E.STOI_TILE].any()        # (b) drops frames inside the first tile
    assert not keep_b[250:E.STOI_TILE].any() and (frames == 256 or not keep_b[E.STOI_TILE])     # ... and across frame 256
    if frames > E.STOI_TILE:
        assert refs[2].kept_frames == E.STOI_TILE                                # (c) the second tile keeps nothing
        assert refs[3].kept_frames == frames - E.STOI_TILE                       # (d) the first tile keeps nothing
        assert (refs[3].kept_frames >= SR.SEG and refs[3].status == 0) or refs[3].status == SR.FEW_FRAMES
    assert refs[2].kept_frames >= 30 and refs[2].status == 0


@pytest.mark.parametrize("n", E.STOI_N)
def test_stoi_check_sees_a_dropped_carry(n):
    clean, degraded = E.stoi_rows(n)
    refs = E.stoi_reference(n)
    wrong = [E.stoi_mutant_carry_dropped(clean[b], degraded[b]) for b in range(4)]

    def check(rows):
        return E.check_stoi(np.array([r.value for r in rows]), np.array([r.kept_frames for r in rows]),
                            np.array([r.status for r in rows]), refs)
    assert check(refs) == 0.0
    if n == 32896:              # one tile of frames: there is no carry to drop
        assert check(wrong) == 0.0
        return
    assert wrong[3].kept_frames == refs[3].kept_frames                          # (d): the carry into tile two is 0 anyway
    for b in (0, 1, 2):
        rows = list(refs)
        rows[b] = wrong[b]
        with pytest.raises(AssertionError):
            check(rows)


# ====================================================================================================================== WPE
def test_wpe_cases():
    for case in E.WPE_CASES + [E.WPE_WORKSPACE]:
        c = E.wpe_case(case)
        assert not c.status.any() and c.cond.max() <= WR.COND_CAP, case
    c = E.wpe_case(E.WPE_DELAY0)
    assert np.abs(c.Y).max() <= 1e-4 * np.abs(c.X).max()                         # the filter predicts the frame from itself
    B, D, F, T, taps, delay, ctx, _ = E.WPE_CASES[1]
    assert ctx == 64 > T                                                         # clipped at both ends of every frame
    assert E.WPE_CASES[2][5] == 64 and E.WPE_CASES[3][1] == 8 and E.WPE_CASES[3][1] * E.WPE_CASES[3][4] == 64
    B, D, F, T, taps = E.WPE_WORKSPACE[:5]
    assert not E.wpe_rows_in_lds(D, T, taps) and E.WPE_WORKSPACE[6] > 0 and B * F > 1
    for it in (1, 16):
        c = E.wpe_case(E.WPE_WORKSPACE, it)
        assert not c.status.any() and c.cond.max() <= WR.COND_CAP


def test_wpe_lds_boundary():
    lo, hi = 1, 65535                                    # the largest T whose rows stay in LDS at D = taps = 1
    assert E.wpe_rows_in_lds(1, lo, 1) and not E.wpe_rows_in_lds(1, hi, 1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if E.wpe_rows_in_lds(1, mid, 1) else (lo, mid)
    assert lo == E.WPE_LDS_T == 5111
    for T in (lo, lo + 1):
        c = E.wpe_case(E.wpe_boundary_case(T))
        assert not c.status.any() and c.cond.max() <= WR.COND_CAP


def test_wpe_check_sees_an_unclipped_power_window():
    """On the workspace case (psd_context = 3).  The psd_context = 64 case cannot see this defect: its window always covers
    the whole row of 40 frames, so an unclipped divisor scales every lambda alike, which WPE does not notice; that case is
    there for the window's bounds themselves (reads before the row's first and after its last frame)."""
    case = E.WPE_WORKSPACE
    B, D, F, T, taps, delay, ctx, loading = case
    c = E.wpe_case(case)
    assert E.check_wpe(c.Y, c.X, c.Y, c.cond, case) == 0.0
    right, wrong = c.Y.copy(), c.Y.copy()
    right[0, :, 0], _ = E.wpe_bin_mutant(c.X[0, :, 0], taps, delay, 3, ctx, 1e-10, loading)  # the mutant's own arithmetic is right
    E.check_wpe(right, c.X, c.Y, c.cond, case)
    wrong[0, :, 0], _ = E.wpe_bin_mutant(c.X[0, :, 0], taps, delay, 3, ctx, 1e-10, loading, unclipped=True)
    with pytest.raises(AssertionError):
        E.check_wpe(wrong, c.X, c.Y, c.cond, case)


def test_wpe_check_sees_a_neighbours_workspace():
    """Bin 1 reading q and w from bin 0's workspace: bin 0's weights in bin 1's normal equations."""
    case = E.WPE_WORKSPACE
    B, D, F, T, taps, delay, ctx, loading = case
    c = E.wpe_case(case)
    _, lams = E.wpe_bin_mutant(c.X[0, :, 0], taps, delay, 3, ctx, 1e-10, loading)
    wrong = c.Y.copy()
    wrong[0, :, 1], _ = E.wpe_bin_mutant(c.X[0, :, 1], taps, delay, 3, ctx, 1e-10, loading, lams=lams)
    with pytest.raises(AssertionError):
        E.check_wpe(wrong, c.X, c.Y, c.cond, case)
