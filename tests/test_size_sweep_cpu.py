"""The size sweep without a GPU (tests/helpers/size_sweep_cases.py): that its lists hold every size the array kernels are
compiled for, that every case meets its family's conditions on the restatement alone (the assertions the families' own CPU tests
make on their parity cases: conditions on the inputs, no measurements of a kernel), and that the checking functions of
tests/helpers/parity_checks.py, which tests/test_size_sweep_gpu.py calls, reject a restatement made wrong the way one size of a
kernel could be wrong.  Every tolerance is the family's: 32 times the restatement's own forward / reverse difference."""
import contextlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import align_ref as AR  # noqa: E402
import beamform_ref as BR  # noqa: E402
import cacgmm_ref as CR  # noqa: E402
import ilrma_ref as LR  # noqa: E402
import iva_ref as IR  # noqa: E402
import parity_checks as PC  # noqa: E402
import separation_metrics_ref as MR  # noqa: E402
import size_sweep_cases as S  # noqa: E402
import srp_ref as SR  # noqa: E402
import subspace_ref as UR  # noqa: E402


# ------------------------------------------------------------------------------------------------- coverage by construction
def test_every_compiled_size_has_a_case():
    assert {s[1] for s in S.IVA if s[3] == 70} == set(range(1, 9))
    assert {s[:4] for s in S.IVA} >= {(1, 3, 2, 33), (1, 1, 2, 1)} and not [s for s in S.IVA if s[3] == 1 and s[1] > 1]
    assert len(S.ILRMA_WALK) == 16 and [s[4] for s in S.ILRMA_WALK] == list(range(1, 17))
    assert {s[1] for s in S.ILRMA_WALK} == set(range(1, 9))
    late = [s for s in S.ILRMA if s[1] * s[4] > 64]
    assert {(s[1], s[4]) for s in late} >= {(8, 16), (5, 13)} and all(c in late for c, _ in S.ILRMA_LATE_VALUES)
    for shape, values in S.ILRMA_LATE_VALUES:
        assert values and all(64 <= i < shape[1] * shape[4] for i in values)
        assert any(v == 0.0 for v in values.values()) or any(np.isnan(v) for v in values.values())
    assert {v == 0.0 for _, values in S.ILRMA_LATE_VALUES for v in values.values()} == {True, False}      # a zero and a NaN
    assert {s[2] for s in S.ILRMA if s[1] == 2} >= {65, 128}
    assert [s for s in S.ILRMA if s[1] == 3 and s[3] == 33]
    assert {s[1] for s in S.CACGMM} == set(range(2, 9)) and {s[2] for s in S.CACGMM} == set(range(1, 9))
    assert len({s[1] - s[2] for s in S.CACGMM}) > 2                                                        # D and K move apart
    assert [s for s in S.CACGMM if s[2] * s[1] * s[1] > 256 and s[1:3] != (8, 8)]
    assert {s[0] for s in S.SCORING} == set(range(1, 9)) and {s[1] for s in S.SCORING} == set(range(1, 9))
    assert all(K <= J for K, J, _ in S.SCORING) and {s[2] for s in S.SCORING} == {63, 65, 257}
    assert len(S.ASSIGN_PAIRS) == len(set(S.ASSIGN_PAIRS)) == 36 and all(1 <= K <= J <= 8 for K, J in S.ASSIGN_PAIRS)
    assert [s[:4] for s in S.ALIGN] == [(1, K, 5, 66) for K in range(1, 9)]
    assert S.SRP == [(1, D, 5, 37, 8, 60, 400) for D in range(2, 9)]
    assert S.BEAMFORM == [(1, 6, 2, 65, 1e-10)] and set(S.GEV_REFS) == {0, 5}
    everything = S.IVA + S.ILRMA + S.CACGMM + S.ALIGN
    assert all(s[0] == 1 for s in everything)                                                              # one item a case


def test_the_sweep_adds_what_the_parity_lists_leave_out():
    """The sizes the families' own lists never reach, as DESIGN.md's table has them: a later edit of either list shows here."""
    assert set(range(1, 9)) - {s[1] for s in IR.PARITY} == {5, 6, 7}
    assert set(range(1, 9)) - {s[1] for s in LR.PARITY} == {4, 5, 6, 7}
    assert set(range(1, 17)) - {s[4] for s in LR.PARITY} == set(range(4, 16))
    assert set(range(2, 9)) - {s[1] for s in CR.PARITY} == {5, 6, 7} and set(range(1, 9)) - {s[2] for s in CR.PARITY} == {4, 5, 6, 7}
    assert set(range(1, 9)) - {s[1] for s in MR.SHAPES} == {4, 5, 6, 7}
    assert set(range(1, 9)) - {s[0] for s in MR.SHAPES[1:]} == {1, 5, 6, 7}      # SI-BSS eval: K = 1 has no SIR to compare
    assert set(range(1, 9)) - {s[1] for s in AR.PARITY} == {6, 7}
    assert set(range(2, 9)) - {s[1] for s in SR.PARITY} == {5, 6, 7}
    assert set(range(1, 9)) - {s[1] for s in BR.PARITY} == {6}
    assert max(s[1] * s[4] for s in LR.PARITY) <= 64 and not {64, 65, 128} & {s[2] for s in LR.PARITY}


# ------------------------------------------------------------------------------------------------- conditions on the cases
@pytest.mark.parametrize("model", IR.MODELS)
@pytest.mark.parametrize("shape", S.IVA, ids=S.IVA_IDS)
def test_auxiva_cases_are_well_conditioned(shape, model):
    for single in (False, True):
        ref = IR.reference(shape, model, single=single)
        assert not ref.status.any()
        assert ref.kappa.max() <= IR.KAPPA_CAP, ref.kappa.max()
        tol = IR.w_tolerance(shape, model, single)
        print("%s %s %s: kappa %.3g, e_ref %.3g, tol %.3g" % (shape[:4], model, "complex64" if single else "complex128",
                                                             ref.kappa.max(), IR.e_ref(shape, model, single), tol))
        assert tol <= 1e-10
        for ref_mic in sorted({0, shape[1] - 1}):
            assert IR.y_bound(IR.promoted(IR.parity_case(shape).X, single), ref.W, ref_mic)[1] <= IR.COND_CAP


@pytest.mark.parametrize("shape", S.ILRMA, ids=S.ILRMA_IDS)
def test_ilrma_cases_are_well_conditioned(shape):
    for single in (False, True):
        ref = LR.reference(shape, single=single)
        assert not ref.status.any() and not LR.reference(shape, single=single, reverse=True).status.any()
        assert ref.kappa.max() <= LR.KAPPA_CAP, ref.kappa.max()
        tol = LR.tolerance(shape, single)
        print("%s %s: kappa %.3g, e_ref %.3g, tol %.3g, floored %d" % (shape[:5], "complex64" if single else "complex128",
                                                                      ref.kappa.max(), LR.e_ref(shape, single), tol, ref.floored))
        assert tol <= 1e-10
        assert max(np.linalg.cond(w) for w in ref.W.reshape(-1, shape[1], shape[1])) <= LR.COND_CAP


@pytest.mark.parametrize("shape", S.CACGMM, ids=S.CACGMM_IDS)
def test_cacgmm_cases_meet_their_conditions(shape):
    for single in (False, True):
        ref = CR.reference(shape, single=single)
        assert not ref.status.any()
        tol = CR.tolerance(shape, single)
        print("%s %s: e_ref %.3g, tol %.3g, cond up to %.3g, cov forward/reverse over tol cond %.3g"
              % (shape[:5], "complex64" if single else "complex128", CR.e_ref(shape, single), tol, ref.cond.max(),
                 CR.cov_ratio(shape, single)))
        assert tol <= CR.TOL_CAP
        assert ref.cond.max() <= CR.COND_CAP
        assert CR.cov_ratio(shape, single) <= CR.COV_RATIO_CAP


@pytest.mark.parametrize("single", [False, True], ids=["float64", "float32"])
@pytest.mark.parametrize("shape", S.SCORING, ids=S.SCORING_IDS)
def test_scoring_cases_meet_their_conditions(shape, single):
    """tests/test_separation_metrics_cpu.py's conditions; with one reference there is no interference, SIR is +inf on both
    sides and only SDR and SAR carry a number."""
    K = shape[0]
    c, r = MR.case(shape), MR.reference(shape, single)
    assert np.array_equal(r.perm, c.scramble) and not r.status.any()
    assert r.cond.max() <= MR.COND_CAP
    if K == 1:
        assert (r.sir == np.inf).all() and (MR.reference(shape, single, reverse=True).sir == np.inf).all()
    for v in (r.sdr, r.sar) + (() if K == 1 else (r.sir,)):
        assert (np.abs(v) <= MR.VALUE_CAP).all()
    assert PC.si_bss_tolerance(shape, single) <= MR.TOL_CAP


@pytest.mark.parametrize("shape", S.ALIGN, ids=S.ALIGN_IDS)
def test_alignment_cases_meet_their_conditions(shape):
    B, K, F, T = shape[:4]
    c = AR.parity_case(shape)
    margin = np.inf
    for n in range(1, AR.ITERATIONS + 1):
        fwd, rev = AR.reference(shape, n), AR.reference(shape, n, reverse=True)
        assert not fwd.status.any() and fwd.perm.shape == (B, F, K)
        assert np.array_equal(fwd.perm, rev.perm) and np.array_equal(fwd.changed, rev.changed)
        margin = min(margin, fwd.margin, rev.margin)
    tol = AR.tolerance(shape)
    print("%s: margin %.3g, e_ref %.3g, tol %.3g" % (shape[:4], margin, AR.e_ref(shape), tol))
    assert margin >= AR.MARGIN_FLOOR
    assert tol <= AR.TOL_CAP
    last = AR.reference(shape)
    if K >= 2:
        assert not last.changed.any()
        assert all(AR.common_order(c.scramble[b], last.perm[b]) for b in range(B))
        assert not all(AR.common_order(c.scramble[b], np.tile(np.arange(K), (F, 1))) for b in range(B))


@pytest.mark.parametrize("shape", S.SRP, ids=S.SRP_IDS)
def test_srp_and_music_cases_meet_their_conditions(shape):
    """The restatement's arg-max clears twice the map's bound and is the true candidate; MUSIC's builder asserts its own
    conditions (the eigengap, a margin of four chain bounds).  With two microphones a candidate and its mirror image in the
    vertical plane through the pair have the same delay difference: at D = 2 the mirror (candidate 16 for the true 20) wins
    the SRP map by 1.8e-5, far above the bound, and is what the device must find; MUSIC finds the true one."""
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c = SR.parity_case(shape)
    bound = SR.map_bound(D, T, f_lo, f_hi, SR.theta_max(f_hi, SR.FS, n_fft, c.mics, c.cand))
    for single in (False, True):
        ref = SR.reference(shape, single=single)
        assert not ref.status.any() and (ref.gap > 2 * bound).all()
        if D > 2:
            assert np.array_equal(ref.best, c.true)
        else:
            axis = (c.mics[1] - c.mics[0])[:2]
            theta = -np.pi + 2 * np.pi * np.arange(G) / G
            mirror = (2 * np.arctan2(axis[1], axis[0]) - theta[c.true[0]] + np.pi) % (2 * np.pi) / (2 * np.pi / G)
            assert int(ref.best[0]) == int(round(mirror)) % G and np.argsort(ref.map[0])[-2] == c.true[0]
        for K in UR.music_orders(D):
            m = UR.music_reference(shape, K, single=single)
            assert not m.status.any() and np.array_equal(m.best, c.true)


def test_beamform_and_gev_cases_meet_their_conditions():
    for shape in S.BEAMFORM:
        for kind in BR.MASKS:
            ref = BR.reference(shape, kind)                                   # the builder asserts cond <= COND_CAP under every mask
            assert max(v.max() for v in ref.cond.values()) <= BR.COND_CAP
            for variant in UR.GEV_VARIANTS:
                for mic in S.GEV_REFS:
                    assert not UR.gev_reference(shape, kind, variant, mic).out.status.any()      # ... and the gap >= GEV_GAP


# ------------------------------------------------------------------------------------------------------ the checks can fail
@contextlib.contextmanager
def replaced(module, name, value):
    """A module's function replaced for the length of the block: a restatement made wrong on purpose."""
    kept = getattr(module, name)
    setattr(module, name, value)
    try:
        yield kept
    finally:
        setattr(module, name, kept)


def case_of(cases, **sizes):
    index = {"D": 1, "F": 2, "T": 3, "L": 4}
    return next(s for s in cases if all(s[index[k]] == v for k, v in sizes.items()))


def test_check_y_sees_a_microphone_left_out():
    """y = sum_d W[k, d] x_d without the last microphone, at D = 6: the per-source path of the projection with a short loop."""
    shape = case_of(S.IVA, D=6)
    D = shape[1]
    X, ref = IR.parity_case(shape).X, IR.reference(shape, "laplace")
    PC.check_y("as it is", ref.Y, X, ref.W, ref.status)
    short = ref.W.copy()
    short[..., D - 1] = 0
    A0 =np.array([[IR.solve(ref.W[0, f], np.eye(D))[0] for f in range(shape[2])]])              # (1, F, D)
    Y = np.moveaxis(A0, 2, 1)[..., None] * np.einsum("bfkd,bdft->bkft", short, X)
    with pytest.raises(AssertionError):
        PC.check_y("the last microphone left out", Y, X, ref.W, ref.status)


def test_check_w_sees_an_upper_entry_that_is_no_conjugate():
    """One entry above the diagonal of the weighted covariance equal to, not the conjugate of, its twin below, at D = 5."""
    shape = case_of(S.IVA, D=5)
    D = shape[1]
    X = IR.parity_case(shape).X
    for model in IR.MODELS:
        ref, tol = IR.reference(shape, model), IR.w_tolerance(shape, model)
        PC.check_w("the other order", IR.reference(shape, model, reverse=True).W, ref.W, tol)
        kept = IR.weighted_cov

        def wrong(x, phi_k, reverse=False, terms=None):
            V = kept(x, phi_k, reverse, terms)
            V[1, D - 1] = V[D - 1, 1]
            return V
        with replaced(IR, "weighted_cov", wrong):
            got = IR.auxiva(X, shape[4], model)
        with pytest.raises(AssertionError):                # (a bin may also lose its positive w^H V w and take status 2: W = I)
            PC.check_w("V[1, D - 1] not conjugated, %s" % model, got.W, ref.W, tol)


def test_check_y_sees_a_projection_scaled_by_the_wrong_source():
    """Source k >= 4 scaled by A[ref, k - 4], at D = 7 and ref = D - 1: the per-source pass indexing As from 0 in every pass."""
    shape = case_of(S.IVA, D=7)
    D, F = shape[1], shape[2]
    X, ref = IR.parity_case(shape).X, IR.reference(shape, "laplace")
    want, _, _ = IR.project(X, ref.W, ref.status, D - 1)
    PC.check_y("as it is", want, X, ref.W, ref.status, D - 1)
    Y = want.copy()
    for f in range(F):
        A = IR.solve(ref.W[0, f], np.eye(D))
        y = ref.W[0, f] @ X[0, :, f]
        for k in range(4, D):
            Y[0, k, f] = A[D - 1, k - 4] * y[k]
    with pytest.raises(AssertionError):
        PC.check_y("A[ref, k - 4]", Y, X, ref.W, ref.status, D - 1)


def test_check_three_sees_a_basis_left_out_of_the_model():
    """R = sum_l basis act without l = L - 1, at L = 13."""
    shape = case_of(S.ILRMA, L=13)
    L = shape[4]
    ref, tol = LR.reference(shape), LR.tolerance(shape)
    PC.check_three("the other order", LR.reference(shape, reverse=True)[:3], ref[:3], tol)
    kept = LR.variance
    with replaced(LR, "variance", lambda basis_b, act_b, floor, seen=None: kept(basis_b[:, :, :L - 1], act_b[:, :L - 1], floor, seen)):
        got = LR.ilrma(LR.parity_case(shape).X, *LR.parity_start(shape), shape[5])
    assert not got.status.any()
    with pytest.raises(AssertionError):
        PC.check_three("l = L - 1 left out", got[:3], ref[:3], tol)


def late_values(shape, values):
    """(X, basis0, activations0, the status they must get) of a case of ILRMA_LATE_VALUES: bin 1's basis0 values at the flat
    indices k L + l replaced."""
    B, D, F, T, L = shape[:5]
    b0, a0 = (a.copy() for a in LR.parity_start(shape))
    for i, v in values.items():
        b0[0, i // L, 1, i % L] = v
    want = np.zeros((B, F), np.int32)
    want[0, 1] = 1
    return LR.parity_case(shape).X, b0, a0, want


@pytest.mark.parametrize("shape,values", S.ILRMA_LATE_VALUES, ids=[S.ILRMA_IDS[S.ILRMA.index(c)] for c, _ in S.ILRMA_LATE_VALUES])
def test_check_refused_bins_sees_a_scan_that_stops_after_64_values(shape, values):
    """The scan of a bin's D L basis0 values for one that is not > 0 and finite, stopped after the first 64."""
    B, D, F, T, L = shape[:5]
    X, b0, a0, want = late_values(shape, values)
    ref = LR.ilrma(X, b0, a0, shape[5])
    PC.check_refused_bins("as it is", ref.status, ref.W, ref.Y, X, want)
    assert np.isfinite(ref.basis[:, :, [0, 2]]).all() and np.isfinite(ref.activations).all()

    def first_64(X, basis0, activations0):
        flat = np.moveaxis(basis0, 2, 1).reshape(B, F, D * L)[:, :, :64]                       # (B, F, k L + l)
        status = IR.bin_status(X)
        status[~LR.positive(flat).all(axis=2)] = 1
        status[~LR.positive(activations0).all(axis=(1, 2, 3))] = 1
        return status
    with replaced(LR, "start_status", first_64):
        got = LR.ilrma(X, b0, a0, shape[5])
    with pytest.raises(AssertionError):
        PC.check_refused_bins("64 values scanned", got.status, got.W, got.Y, X, want)


def test_check_three_sees_a_row_sum_chain_that_stops_at_bin_63():
    """lam from the first 64 bins alone, at F = 65."""
    shape = case_of(S.ILRMA, F=65)
    ref, tol = LR.reference(shape), LR.tolerance(shape)
    kept = LR.scale

    def first_chunk(P, status_b, reverse=False):
        return kept(P[:, :64], status_b[:64], reverse)
    with replaced(LR, "scale", first_chunk):
        got = LR.ilrma(LR.parity_case(shape).X, *LR.parity_start(shape), shape[5])
    assert not got.status.any()
    with pytest.raises(AssertionError):
        PC.check_three("lam of 64 bins", got[:3], ref[:3], tol)


def test_check_si_bss_sees_a_gram_matrix_without_its_last_source():
    """The projection onto the references solved without the last row and column of G, at K = 6."""
    shape = next(s for s in S.SCORING if s[0] == 6)
    K = shape[0]
    c, ref = MR.case(shape), MR.reference(shape)
    tol = PC.si_bss_tolerance(shape)
    rev = MR.reference(shape, reverse=True)
    PC.check_si_bss("the other order", rev.sir, rev.sar, rev.sdr, ref, tol)
    kept = MR.solve

    def smaller(G, g):
        z = kept(G[:K - 1, :K - 1], g[:K - 1])
        return None if z is None else np.append(z, 0.0)
    with replaced(MR, "solve", smaller):
        got = MR.si_bss_eval(c.references, c.estimates)
    assert not got.status.any() and np.array_equal(got.perm, ref.perm)
    with pytest.raises(AssertionError):
        PC.check_si_bss("G without its last row and column", got.sir, got.sar, got.sdr, ref, tol)


def test_check_align_sees_a_search_over_the_first_256_prefixes():
    """The search of the K! permutations cut after 256 prefixes of six, at K = 7: a thread that takes one trip."""
    shape = next(s for s in S.ALIGN if s[1] == 7)
    P = AR.parity_case(shape).P
    counts = range(1, AR.ITERATIONS + 1)
    refs = {n: AR.reference(shape, n) for n in counts}
    tol = AR.tolerance(shape)
    PC.check_align("the other order", {n: AR.reference(shape, n, reverse=True)[:4] for n in counts}, refs, tol)
    kept = AR.permutations
    with replaced(AR, "permutations", lambda K: kept(K)[:256 * 6]):
        runs = {n: AR.align(P, n)[:4] for n in counts}
    with pytest.raises(AssertionError):
        PC.check_align("256 prefixes", runs, refs, tol)


def test_check_assign_sees_the_last_rank_among_equals():
    """A repeated score: the lowest rank wins; a search that keeps the last of the equals is seen."""
    table = np.zeros((1, 3, 4))
    want = MR.assign(table)
    PC.check_assign("as it is", (want.perm, want.total, want.status), table, True)
    assert want.perm.tolist() == [[0, 1, 2]]
    with pytest.raises(AssertionError):
        PC.check_assign("the last of the equals", (np.array([[3, 2, 1]], np.int32), want.total, want.status), table, True)
