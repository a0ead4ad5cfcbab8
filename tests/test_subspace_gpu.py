"""The Hermitian eigensolver, MUSIC and the GEV beamformer on the device (csrc/herm_eig.h, csrc/subspace.hip, csrc/beamform.hip;
acoustic_locating_vq_vae.subspace / .localization / .beamforming) against the float64 restatement of
tests/helpers/subspace_ref.py, which tests/test_subspace_cpu.py pins.  u = 1.1e-16; c1 = 32 and c2 = 2 are the constants that
file measures, and the device is held to twice each: a bound is spent once for each side.

Eigensolver:   max |A V - V diag(lam)| <= 2 c1 D u ||A||_F, max |V^H V - I| <= 2 c1 D u (both taken in longdouble from the
               device's own output), max |lam - lam_ref| <= 2 c1 D u ||A||_F.  Eigenvectors are never compared one by one.
Map alone:     the restatement's V and lambda uploaded: |null - null_ref| <= (D K + 16 Theta + 32 + anchor) u.
Chain:         the restatement's covariances uploaded, device eigh into device map: the map-alone bound plus the mean over the
               band of 2 (2 c1) D u ||Phi||_F / gap_f.  ``best`` equals the restatement's, hence the true candidate: the
               builders assert a margin of more than 4 x this bound.
GEV:           the restatement's covariances uploaded: max |w - w_ref| <= 2 c2 D u cond_2(Phi') (1 + ||C||_F / gap_C) max |w_ref|,
               the same for rtf."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import beamform_ref as BR  # noqa: E402
import srp_ref  # noqa: E402
import subspace_ref as R  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import beamforming as BF  # noqa: E402
from acoustic_locating_vq_vae import front_end as FE  # noqa: E402
from acoustic_locating_vq_vae import localization as LOC  # noqa: E402
from acoustic_locating_vq_vae import subspace as SUB  # noqa: E402

U = R.U
C1, C2 = 2 * R.C1, 2 * R.C2
GRID_CAP_MATRICES = 65536 * 4          # the eigensolver's grid holds this many matrices at once (csrc/subspace.hip)


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()          # a copy: the shared cases are read-only


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    """Two tensors equal bit for bit, NaN included."""
    ra, rb = (torch.view_as_real(t.resolve_conj().contiguous()) if t.is_complex() else t.contiguous() for t in (a, b))
    if ra.shape != rb.shape or ra.dtype != rb.dtype:
        return False
    view = {torch.float64: torch.int64, torch.float32: torch.int32}.get(ra.dtype)
    return torch.equal(ra.view(view), rb.view(view)) if view else torch.equal(ra, rb)


def eig_same_bits(a, b):
    return same_bits(a.values, b.values) and same_bits(a.vectors, b.vectors) and same_bits(a.status, b.status)


def phase_rule_holds(V):
    """Every column has a real, positive component whose re^2 + im^2 is the column's largest (to within the rounding of the
    phasor's multiplication, which may reorder moduli that agree to the last bits)."""
    m2 = V.real ** 2 + V.imag ** 2
    anchor = (V.imag == 0) & (V.real > 0) & (m2 >= m2.max(axis=-2, keepdims=True) * (1 - 8 * U))
    return bool(anchor.any(axis=-2).all())


# ------------------------------------------------------------------------------------------------------------ the eigensolver
@pytest.mark.parametrize("D", range(1, 9))
def test_eigh_parity(D):
    n = 5
    A = np.concatenate([R.eig_case(kind, D, n) for kind in R.EIG_KINDS])
    ref = R.eigh(A)
    got = SUB.eigh(dev(A))
    assert got.values.dtype == torch.float64 and got.values.shape == (len(A), D)
    assert got.vectors.dtype == torch.complex128 and got.vectors.shape == (len(A), D, D)
    assert got.status.dtype == torch.int32 and got.status.shape == (len(A),) and not host(got.status).any()
    lam, V = host(got.values), host(got.vectors)
    for k, kind in enumerate(R.EIG_KINDS):
        rows = slice(k * n, (k + 1) * n)
        res, orth, err = R.eig_errors(A[rows], lam[rows], V[rows], ref.lam[rows])
        print("D=%d %s: residual %.3g, orthogonality %.3g, eigenvalues %.3g of D u ||A||_F; bound %d" % (D, kind, res, orth, err, C1))
        assert max(res, orth, err) <= C1, (kind, res, orth, err)
    assert (np.diff(lam, axis=-1) >= 0).all()
    assert phase_rule_holds(V)
    for kind in ("identity", "zero"):
        rows = slice(R.EIG_KINDS.index(kind) * n, (R.EIG_KINDS.index(kind) + 1) * n)
        assert (V[rows] == np.eye(D)).all() and (lam[rows] == (1 if kind == "identity" else 0)).all()


@pytest.mark.parametrize("D", [1, 3, 8])
def test_eigh_batches_launches_and_neighbours(D):
    """Batches of 1, 3, 4, 5 and 257 matrices (a wave, a workgroup less one, a workgroup, one more, many workgroups): a matrix
    has the same bits alone, in any batch and on any run."""
    kinds = [k for k in R.EIG_KINDS if k not in ("identity", "zero")]
    pool = np.concatenate([R.eig_case(kind, D, 37, seed=1) for kind in kinds])[:257]
    A = dev(pool)
    whole = SUB.eigh(A)
    assert not host(whole.status).any()
    assert eig_same_bits(SUB.eigh(A), whole)                             # a second launch
    for n in (1, 3, 4, 5):
        for first in (0, 100, 257 - n):
            part = SUB.eigh(A[first:first + n].clone())
            assert eig_same_bits(part, SUB.Eigh(whole.values[first:first + n], whole.vectors[first:first + n],
                                                whole.status[first:first + n])), (n, first)
    lead = SUB.eigh(A[:256].reshape(4, 8, 8, D, D))                      # leading dimensions are the caller's
    assert lead.values.shape == (4, 8, 8, D) and lead.vectors.shape == (4, 8, 8, D, D) and lead.status.shape == (4, 8, 8)
    assert same_bits(lead.vectors.reshape(256, D, D), whole.vectors[:256])


def test_eigh_more_matrices_than_the_grid_holds():
    """One more matrix than the capped grid holds at once: the waves stride, and every copy of a matrix has the same bits."""
    D, reps = 2, GRID_CAP_MATRICES // 256
    pool = dev(np.concatenate([R.eig_case(kind, D, 64, seed=2) for kind in ("full", "rank1", "indefinite", "clustered")]))
    A = torch.cat([pool.repeat(reps, 1, 1), pool[7:8]])
    assert A.shape[0] == GRID_CAP_MATRICES + 1
    got, base = SUB.eigh(A), SUB.eigh(pool)
    assert not bool(got.status.any())
    assert same_bits(got.vectors[:-1].view(reps, 256, D, D), base.vectors[None].expand(reps, 256, D, D))
    assert same_bits(got.values[:-1].view(reps, 256, D), base.values[None].expand(reps, 256, D))
    assert same_bits(got.vectors[-1], base.vectors[7]) and same_bits(got.values[-1], base.values[7])


@pytest.mark.parametrize("D", [2, 5, 8])
def test_eigh_flags_a_non_finite_entry_and_reads_the_lower_triangle(D):
    A = R.eig_case("full", D, 9, seed=3).copy()
    clean = SUB.eigh(dev(A))
    A[:, 0, D - 1] = np.nan                                              # above the diagonal: not read
    A[:, 1, 1] += complex(0, np.inf)                                     # the diagonal's imaginary part: not read
    assert eig_same_bits(SUB.eigh(dev(A)), clean)
    A[2, D - 1, 0] = complex(np.nan, 0)
    A[4, 1, 1] = np.inf
    A[7, 1, 0] = complex(1, -np.inf)
    got = SUB.eigh(dev(A))
    assert got.status.tolist() == [0, 0, 1, 0, 1, 0, 0, 1, 0]
    bad, good = [2, 4, 7], [0, 1, 3, 5, 6, 8]
    assert bool(torch.isnan(got.values[bad]).all()) and bool(torch.isnan(torch.view_as_real(got.vectors[bad])).all())
    assert same_bits(got.values[good], clean.values[good]) and same_bits(got.vectors[good], clean.vectors[good])


# ----------------------------------------------------------------------------------------------------------------------- MUSIC
MUSIC_CASES = [(s, K) for s in srp_ref.PARITY for K in R.music_orders(s[1])]
MUSIC_IDS = ["%s-K%d" % ("-".join(str(v) for v in s), K) for s, K in MUSIC_CASES]


@pytest.mark.parametrize("shape,K", MUSIC_CASES, ids=MUSIC_IDS)
def test_music_parity(shape, K):
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c, ref = srp_ref.parity_case(shape), R.music_reference(shape, K)
    theta = srp_ref.theta_max(f_hi, R.FS, n_fft, c.mics, c.cand)
    mics, cand = dev(c.mics), dev(c.cand)
    # the map alone: the restatement's decomposition uploaded
    null, best, status = N.music(dev(ref.V), dev(ref.lam), mics, cand, K, R.FS, n_fft, R.C, f_lo, f_hi)
    assert null.dtype == torch.float64 and null.shape == (B, G) and best.dtype == torch.int32 and status.dtype == torch.int32
    e_alone = float(np.abs(host(null) - ref.null).max())
    assert not host(status).any() and np.array_equal(host(best), ref.best)
    # the chain: the restatement's covariances uploaded, device eigh into device map
    got = LOC.music_from_covariance(dev(ref.cov), mics, cand, K, n_fft=n_fft, band=(f_lo, f_hi))
    bound = R.chain_bound(D, K, theta, ref.norms, ref.gaps, C1)
    e_chain = np.abs(host(got.null) - ref.null).max(axis=1)
    res, orth, err = R.eig_errors(ref.cov, host(got.values), host(SUB.eigh(dev(ref.cov)).vectors), ref.lam)
    print("%s K=%d: map alone / bound %.3g; chain / bound %.3g (bound %.3g); eigensolver ratios %.3g %.3g %.3g of %d"
          % (shape, K, e_alone / ref.bound_alone, float((e_chain / bound).max()), float(bound.max()), res, orth, err, C1))
    assert e_alone <= ref.bound_alone
    assert (e_chain <= bound).all() and max(res, orth, err) <= C1
    assert not host(got.status).any() and np.array_equal(host(got.best), ref.best) and np.array_equal(ref.best, c.true)
    # the whole way from the spectrogram, complex128 and complex64: the same candidate; batched geometry: the same bits
    for cdtype, single in ((np.complex128, False), (np.complex64, True)):
        full = LOC.music(dev(c.X.astype(cdtype)), mics, cand, K, n_fft=n_fft, band=(f_lo, f_hi))
        want = R.music_reference(shape, K, single=single)
        assert not host(full.status).any() and np.array_equal(host(full.best), c.true)
        assert full.values.shape == (B, n_fft // 2 + 1, D)
        e_full = np.abs(host(full.null) - want.null).max(axis=1)
        # the covariance's own rounding: an entry of either side within (T + 4) u S_ij of the exact one (beamform_ref.cov_bound),
        # ||S||_F <= tr Phi <= sqrt(D) ||Phi||_F, and a projector moves by at most twice the perturbation over the gap
        extra = np.mean(4 * np.sqrt(D) * (T + 4) * U * want.norms / want.gaps, axis=1)
        assert (e_full <= R.chain_bound(D, K, theta, want.norms, want.gaps, C1) + extra).all()
    each = LOC.music_from_covariance(dev(ref.cov), dev(np.broadcast_to(c.mics, (B, D, 3))), dev(np.broadcast_to(c.cand, (B, G, 3))),
                                     K, n_fft=n_fft, band=(f_lo, f_hi))
    assert same_bits(each.null, got.null) and same_bits(each.best, got.best) and same_bits(each.status, got.status)
    one = LOC.music_from_covariance(dev(ref.cov[B - 1]), mics, cand, K, n_fft=n_fft, band=(f_lo, f_hi))     # an item alone
    assert one.null.shape == (G,) and same_bits(one.null, got.null[B - 1]) and int(one.best) == int(got.best[B - 1])


def test_music_status_bits_and_healthy_neighbours():
    shape = srp_ref.PARITY[1]
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c, ref = srp_ref.parity_case(shape), R.music_reference(shape, 1)
    V = np.concatenate([ref.V, ref.V[:1], ref.V[:1], ref.V[:1], ref.V[1:]])
    lam = np.concatenate([ref.lam, ref.lam[:1], ref.lam[:1], ref.lam[:1], ref.lam[1:]])
    lam[0, f_lo:f_hi + 1] = 0                         # every bin of the band silent
    V[1, f_lo + 3, 1, 2] = complex(1.0, np.nan)       # one NaN inside the band
    V[2, f_hi + 1, 0, 0] = np.nan                     # a NaN outside the band does not flag
    lam[2, f_lo + 1] = 0                              # one silent bin is left out of the mean
    lam[4, f_hi, 0] = np.inf                          # a non-finite eigenvalue
    mics = np.broadcast_to(c.mics, (6, D, 3)).copy()
    mics[3, 1, 2] = np.nan
    want, best, status = R.music(V, lam, mics, c.cand, 1, R.FS, n_fft, R.C, f_lo, f_hi)
    null, gbest, gstatus = N.music(dev(V), dev(lam), dev(mics), dev(c.cand), 1, R.FS, n_fft, R.C, f_lo, f_hi)
    m = host(null)
    assert gstatus.tolist() == [2, 1, 0, 4, 1, 0] == list(status) and gbest.tolist() == [-1, -1, int(best[2]), -1, -1, int(best[5])]
    assert (m[0] == 1).all() and np.isnan(m[[1, 3, 4]]).all()
    assert np.abs(m[[2, 5]] - want[[2, 5]]).max() <= ref.bound_alone
    alone = N.music(dev(ref.V[1:]), dev(ref.lam[1:]), dev(c.mics), dev(c.cand), 1, R.FS, n_fft, R.C, f_lo, f_hi)[0]
    assert same_bits(null[5], alone[0])                                  # the healthy neighbour: as if alone
    cand = c.cand.copy()
    cand[5, 0] = np.inf
    assert N.music(dev(V), dev(lam), dev(c.mics), dev(cand), 1, R.FS, n_fft, R.C, f_lo, f_hi)[2].tolist() == [6, 5, 4, 4, 5, 4]
    # through the public layer: a spectrogram with a NaN, and a silent one
    X = np.concatenate([c.X, c.X[:1], c.X[:1]])
    X[1, 1, f_lo + 2, 0] = np.nan
    X[2, :, f_lo:f_hi + 1] = 0
    X[3, 0, f_hi + 1, 0] = np.nan                     # outside the band
    got = LOC.music(dev(X), dev(c.mics), dev(c.cand), 1, n_fft=n_fft, band=(f_lo, f_hi))
    assert got.status.tolist() == [0, 1, 2, 0] and got.best.tolist() == [int(c.true[0]), -1, -1, int(c.true[0])]
    assert bool(torch.isnan(got.null[1]).all()) and bool((got.null[2] == 1).all())
    assert same_bits(got.null[3], got.null[0])


def test_music_lowest_index_on_ties():
    shape = srp_ref.PARITY[2]
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c, ref = srp_ref.parity_case(shape), R.music_reference(shape, 1)
    k = int(ref.best[0])
    dup = (k + 30) % G
    cand = c.cand.copy()
    cand[dup] = cand[k]                                # the same position twice: the same bits twice
    got = N.music(dev(ref.V), dev(ref.lam), dev(c.mics), dev(cand), 1, R.FS, n_fft, R.C, f_lo, f_hi)
    assert same_bits(got[0][0, k], got[0][0, dup]) and int(got[1][0]) == min(k, dup)
    cand[(k + 1) % G], cand[(k + 2) % G] = cand[k], cand[k]
    many = N.music(dev(ref.V), dev(ref.lam), dev(c.mics), dev(np.tile(cand, (5, 1))), 1, R.FS, n_fft, R.C, f_lo, f_hi)   # 360 candidates
    assert int(many[1][0]) == min(k, dup, (k + 1) % G, (k + 2) % G)


def test_music_lowest_index_across_trips_lanes_and_waves():
    """600 candidates for the arg-min's 256 threads: every entry is the restatement's shallowest candidate but for copies of
    its deepest one, placed so that the thread's own loop, the butterfly and the combine over the waves would each answer
    differently under another tie rule.  (260, 200, 590): index 200 is thread 200 of wave 3, index 260 thread 4 of wave 0 on
    its second trip, so a combine that prefers the lower wave or thread says 260.  (556, 300): both in thread 44, trips 2 and 1.
    On the host the deepest lies below the shallowest by more than twice the map's bound: the tie is among the copies only."""
    B, D, T, G, f_lo, f_hi, n_fft = 1, 3, 4, 600, 8, 60, 400
    c = srp_ref.case(B, D, T, G, 11)
    cov, st = BR.covariance(c.X)
    e = R.eigh(cov)
    null, _, status = R.music(e.V, e.lam, c.mics, c.cand, 1, R.FS, n_fft, R.C, f_lo, f_hi)
    good, poor = int(np.argmin(null[0])), int(np.argmax(null[0]))
    bound = R.map_alone_bound(D, 1, srp_ref.theta_max(f_hi, R.FS, n_fft, c.mics, c.cand))
    print("deepest %.6g, shallowest %.6g, bound %.3g" % (null[0, good], null[0, poor], bound))
    assert not st.any() and not e.status.any() and not status.any() and null[0, poor] - null[0, good] > 2 * bound
    V, lam, mics = dev(e.V), dev(e.lam), dev(c.mics)
    for copies, want in (((260, 200, 590), 200), ((556, 300), 300)):
        grid = np.tile(c.cand[poor], (G, 1))
        grid[list(copies)] = c.cand[good]
        got, best, gstatus = N.music(V, lam, mics, dev(grid), 1, R.FS, n_fft, R.C, f_lo, f_hi)
        assert int(gstatus[0]) == 0 and int(best[0]) == want, (copies, int(best[0]))
        assert all(same_bits(got[0, copies[0]], got[0, g]) for g in copies[1:])


def test_music_locates_on_the_ring_in_the_room():
    """The room case of tests/test_subspace_cpu.py on the device, all four angles in one batch: array_impulse_responses ->
    array_spectrograms -> locate_on_ring(method="music"), within one candidate."""
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
    src = points[angles].contiguous()
    h = FE.array_impulse_responses(src, mics, cfg["room_dimensions"], reverberation_time=cfg["reverberation_time"],
                                   nsample=cfg["n_sample"])
    spec = FE.array_spectrograms(wave, h)
    ring = LOC.locate_on_ring(spec, mics, cfg["receiver_position"], cfg["room_dimensions"], cfg["R"], cfg["Z_LOC_SOURCE"],
                              n_angles=72, method="music", fs=fs, band=(8, 187))
    direct = LOC.music(spec, mics, points, 1, fs=fs, band=(8, 187))
    assert ring.map.shape == (4, 72) and ring.status.tolist() == [0, 0, 0, 0]
    assert same_bits(ring.map, direct.null) and same_bits(ring.theta, theta_grid[direct.best.long()])
    picks = direct.best.tolist()
    print("sources on candidates %s: arg-min %s" % (angles, picks))
    for k, p in zip(angles, picks):
        assert min((p - k) % 72, (k - p) % 72) <= 1
    srp = LOC.locate_on_ring(spec, mics, cfg["receiver_position"], cfg["room_dimensions"], cfg["R"], cfg["Z_LOC_SOURCE"],
                             n_angles=72, fs=fs, band=(8, 187))      # the default method is unchanged
    assert same_bits(srp.map, LOC.srp_phat(spec, mics, points, fs=fs, band=(8, 187)).map)


def test_music_resolves_two_sources():
    D, T, G = R.TWO_SOURCE[0]
    c, ref = R.two_source_case(D, T, G), R.two_source_reference(D, T, G)
    got = LOC.music(dev(c.X), dev(c.mics), dev(c.cand), 2, n_fft=c.n_fft, band=(c.f_lo, c.f_hi))
    row = host(got.null)[0]
    mins = R.local_minima(row)
    print("true %s, local minima %s at depths %s; values of bin 100: %s" % (c.true, mins[:4], row[mins[:4]], host(got.values)[0, 100]))
    assert got.status.tolist() == [0] and sorted(mins[:2]) == list(c.true)
    assert len(mins) == 2 or row[mins[2]] > 100 * row[mins[1]]
    assert int(got.best[0]) == int(mins[0]) == int(ref.best[0])
    one = LOC.music(dev(c.X[0]), dev(c.mics), dev(c.cand), 2, n_fft=c.n_fft, band=(c.f_lo, c.f_hi))          # no batch dimension
    assert one.null.shape == (G,) and one.values.shape == (201, D) and same_bits(one.null, got.null[0])


# ------------------------------------------------------------------------------------------------------------------------- GEV
GEV_SHAPES = [s for s in BR.PARITY if s != BR.DATASET]
GEV_IDS = ["-".join(str(v) for v in s) for s in GEV_SHAPES]


@pytest.mark.parametrize("kind", BR.MASKS)
@pytest.mark.parametrize("shape", GEV_SHAPES, ids=GEV_IDS)
def test_gev_parity(shape, kind):
    B, D, F, T, loading = shape
    souden = BR.reference(shape, kind).W["souden"]
    for variant in R.GEV_VARIANTS:
        for ref in sorted({0, D - 1}):
            g = R.gev_reference(shape, kind, variant, ref)
            got = BF.gev_weights(dev(g.Phi_n), dev(g.Phi_s), ref=ref, loading=loading)
            assert got.w.dtype == torch.complex128 and got.w.shape == (B, F, D) and got.rtf.shape == (B, F, D)
            assert got.gain.dtype == torch.float64 and got.gain.shape == (B, F) and got.status.shape == (B, F)
            assert not host(got.status).any()
            w, rtf, gain = host(got.w), host(got.rtf), host(got.gain)
            ratios = []
            for mine, want in ((w, g.out.W), (rtf, g.out.rtf)):
                bound = R.gev_bound(D, g.cond, g.normC, g.gapC, np.abs(want).max(axis=-1), C2)
                err = np.abs(mine - want).max(axis=-1)
                ratios.append(float((err / bound).max()))
                assert (err <= bound).all(), (variant, ref, ratios)
            unit = R.gev_bound(D, g.cond, g.normC, g.gapC, 1.0, C2)
            # w^H rtf = 1: D products, each side within its bound
            one = np.sum(np.conj(w) * rtf, axis=-1)
            slack = D * unit * (np.abs(g.out.W).max(axis=-1) * np.abs(g.out.rtf).max(axis=-1)) * 2
            assert (np.abs(one - 1) <= slack).all()
            assert (rtf[..., ref] == 1).all()
            # the Rayleigh quotient: no weights do better, Souden's included; the gain is the quotient
            P = BR.loaded(g.Phi_n, loading)

            def quotient(v):
                num = np.einsum("bfi,bfij,bfj->bf", np.conj(v), g.Phi_s, v).real
                return num / np.einsum("bfi,bfij,bfj->bf", np.conj(v), P, v).real
            if D > 1 and ref == 0:
                assert (quotient(w) >= quotient(souden) * (1 - unit)).all()
            assert (np.abs(gain - g.out.gain) <= unit * np.abs(g.out.gain)).all()      # C's entries carry D u cond; lambda_max >= ||C||_F / sqrt(D)
            print("%s %s %s ref %d: |w - w_ref| / bound %.3g, |rtf - rtf_ref| / bound %.3g, |w^H rtf - 1| %.3g"
                  % (shape[:4], kind, variant, ref, ratios[0], ratios[1], float(np.abs(one - 1).max())))
            if D == 1:
                assert (w == 1).all() and (rtf == 1).all()


def test_gev_fallbacks_are_the_reference_microphone_as_bits():
    shape = BR.PARITY[2]
    B, D, F, T, loading = shape
    g = R.gev_reference(shape, "uniform", "full")
    Phi_n, Phi_s = g.Phi_n.copy(), g.Phi_s.copy()
    Phi_n[0, 0] = 0                                   # a pivot of 0
    Phi_s[0, 1] = 0                                   # lambda_max = 0
    Phi_s[0, 2, 1, 0] = np.nan                        # a non-finite whitened matrix
    want = R.gev(Phi_n, Phi_s, D - 1, loading)
    got = BF.gev_weights(dev(Phi_n[0]), dev(Phi_s[0]), ref=D - 1, loading=loading)          # no batch dimension
    assert got.w.shape == (F, D) and got.gain.shape == (F,) and got.status.tolist() == [2, 2, 2, 0] == list(want.status[0])
    e_ref = torch.zeros(D, dtype=torch.complex128, device="cuda")
    e_ref[D - 1] = 1
    for f in range(3):
        assert same_bits(got.w[f], e_ref) and same_bits(got.rtf[f], e_ref) and float(got.gain[f]) == 0
    clean = BF.gev_weights(dev(g.Phi_n), dev(g.Phi_s), ref=D - 1, loading=loading)
    assert same_bits(got.w[3], clean.w[0, 3]) and same_bits(got.rtf[3], clean.rtf[0, 3])         # the healthy neighbour
    again = BF.gev_weights(dev(g.Phi_n), dev(g.Phi_s), ref=D - 1, loading=loading)
    assert same_bits(again.w, clean.w) and same_bits(again.rtf, clean.rtf) and same_bits(again.gain, clean.gain)


@pytest.mark.parametrize("cdtype", [np.complex128, np.complex64])
def test_gev_is_its_chain(cdtype):
    shape = BR.PARITY[10]                             # D = 5
    B, D, F, T, loading = shape
    c = BR.parity_case(shape)
    X = dev(c.X.astype(cdtype))
    noise_mask = dev(c.masks["runs"])
    speech_mask = dev(1 - c.masks["uniform"])
    beam = BF.gev(X, noise_mask, speech_mask, ref=2, loading=1e-6)
    noise, speech = BF.spatial_covariance(X, noise_mask), BF.spatial_covariance(X, speech_mask)
    w = BF.gev_weights(noise.cov, speech.cov, ref=2, loading=1e-6)
    assert beam.spec.dtype == X.dtype and beam.spec.shape == (B, F, T)
    assert same_bits(beam.weights, w.w) and same_bits(beam.spec, BF.apply(X, w.w))
    assert same_bits(beam.status, noise.status | speech.status | w.status) and not host(beam.status).any()
    bad = speech_mask.clone()
    bad[0, 1] = 0                                     # a speech mask that sums to 0: status 1 from the covariance, 2 from the weights
    flagged = BF.gev(X, noise_mask, bad, ref=2)
    assert flagged.status[0].tolist() == [0, 3, 0]
    assert same_bits(flagged.spec[0, 1], X[0, 2, 1])                     # the reference microphone passes through
    one = BF.gev(X[0], noise_mask[0], speech_mask[0], ref=2, loading=1e-6)
    assert same_bits(one.spec, beam.spec[0])
