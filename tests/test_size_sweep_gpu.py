"""Every compiled size of the array kernels on the device -- the microphone count D, the class or source count K, the estimate
count J and ILRMA's rank L each select an unrolled kernel of their own (csrc/iva.hip, ilrma.hip, cacgmm.hip,
separation_metrics.hip, permutation_align.hip, srp_phat.hip, subspace.hip, beamform.hip) -- against the families' float64
restatements, on the cases of tests/helpers/size_sweep_cases.py, which tests/test_size_sweep_cpu.py pins.  Each comparison is the
one the family's own parity test makes, through the functions of tests/helpers/parity_checks.py and with the family's own
tolerance or bound (32 times the restatement's forward / reverse difference, or the bound the family's ``*_ref.py`` derives);
tests/test_size_sweep_cpu.py shows each of them rejecting a size-specific fault.  Beside the sizes:

AuxIVA, ILRMA:  for D >= 5, the projection's one pass per source onto the last microphone: W has the bits of the ref = 0 run.
ILRMA:          D L > 64 with a 0 and a NaN among a bin's basis0 values past the first 64: status 1, W = I, Y = X as bits, and
                the other bins as if the bin were not there.
assign:         all 36 pairs K <= J <= 8, max and min, with repeated scores (the lowest rank wins).
Every family:   one case inside a batch of three different items has the bits it has alone."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

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
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import beamforming as BF  # noqa: E402
from acoustic_locating_vq_vae import localization as LOC  # noqa: E402
from acoustic_locating_vq_vae import separation as SEP  # noqa: E402
from acoustic_locating_vq_vae import speech_metrics as SM  # noqa: E402
from acoustic_locating_vq_vae import subspace as SUB  # noqa: E402

U = IR.U
CDTYPES = [np.complex128, np.complex64]
CIDS = ["complex128", "complex64"]
OTHER = (77, 78)                         # the seeds of the two items a case shares a batch with


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


def alone_in_the_middle(whole, alone):
    """Item 1 of every tensor of a batched result has the bits of the run of that item alone."""
    return all(same_bits(a[0], w[1]) for a, w in zip(alone, whole))


def ratio_line(family, tag, ratio):
    print("sweep %s %s: measured / bound %.3g" % (family, tag, ratio))


# ---------------------------------------------------------------------------------------------------------------------- AuxIVA
@functools.lru_cache(maxsize=None)
def iva_run(shape, model, cdtype, ref=0):
    """(W, Y, status) of an AuxIVA case on the device, downloaded; computed once."""
    B, D, F, T = shape[:4]
    out = SEP.auxiva(dev(IR.parity_case(shape).X.astype(cdtype)), shape[4], model, ref=ref)
    assert out.spec.shape == (B, D, F, T) and out.spec.dtype == (torch.complex64 if cdtype == np.complex64 else torch.complex128)
    assert out.w.shape == (B, F, D, D) and out.w.dtype == torch.complex128
    assert out.status.shape == (B, F) and out.status.dtype == torch.int32
    return host(out.w), host(out.spec), host(out.status)


@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
@pytest.mark.parametrize("model", IR.MODELS)
@pytest.mark.parametrize("shape", S.IVA, ids=S.IVA_IDS)
def test_auxiva(shape, model, cdtype):
    single = cdtype == np.complex64
    tag = "%s %s %s" % (shape[:4], model, np.dtype(cdtype).name)
    W, Y, status = iva_run(shape, model, cdtype)
    ref = IR.reference(shape, model, single=single)
    assert not status.any() and not ref.status.any()
    r_w = PC.check_w(tag, W, ref.W, IR.w_tolerance(shape, model, single))
    r_y = PC.check_y(tag, Y, IR.promoted(IR.parity_case(shape).X, single), W, status, 0, single)
    ratio_line("auxiva", tag, max(r_w, r_y))


@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
@pytest.mark.parametrize("shape", [s for s in S.IVA if s[1] >= 5], ids=[i for s, i in zip(S.IVA, S.IVA_IDS) if s[1] >= 5])
def test_auxiva_projects_onto_the_last_microphone(shape, cdtype):
    """The one pass per source of the projection (D >= 5) with ref = D - 1: ref enters the projection alone."""
    D = shape[1]
    single = cdtype == np.complex64
    first, last = iva_run(shape, "laplace", cdtype), iva_run(shape, "laplace", cdtype, D - 1)
    assert PC.same_bits(first[0], last[0]) and np.array_equal(first[2], last[2]) and not last[2].any()
    tag = "%s %s ref %d" % (shape[:4], np.dtype(cdtype).name, D - 1)
    ratio_line("auxiva", tag, PC.check_y(tag, last[1], IR.promoted(IR.parity_case(shape).X, single), last[0], last[2], D - 1, single))


def test_auxiva_item_in_a_batch_of_three():
    shape = next(s for s in S.IVA if s[1] == 7)
    B, D, F, T = shape[:4]
    x = dev(np.concatenate([IR.case(1, D, F, T, OTHER[0]).X, IR.parity_case(shape).X, IR.case(1, D, F, T, OTHER[1]).X]))
    for model in IR.MODELS:
        whole = SEP.auxiva(x, shape[4], model, ref=D - 1)
        assert alone_in_the_middle(whole, SEP.auxiva(x[1:2].contiguous(), shape[4], model, ref=D - 1))
        assert PC.same_bits(host(whole.w[1:2]), iva_run(shape, model, np.complex128)[0])


# ----------------------------------------------------------------------------------------------------------------------- ILRMA
def ilrma_starts(shape):
    return tuple(dev(a) for a in LR.parity_start(shape))


@functools.lru_cache(maxsize=None)
def ilrma_run(shape, cdtype, ref=0):
    """(W, basis, activations, Y, status) of an ILRMA case on the device, downloaded; computed once."""
    B, D, F, T, L = shape[:5]
    out = SEP.ilrma(dev(LR.parity_case(shape).X.astype(cdtype)), *ilrma_starts(shape), iterations=shape[5], ref=ref)
    assert out.spec.shape == (B, D, F, T) and out.spec.dtype == (torch.complex64 if cdtype == np.complex64 else torch.complex128)
    assert out.w.shape == (B, F, D, D) and out.w.dtype == torch.complex128
    assert out.basis.shape == (B, D, F, L) and out.activations.shape == (B, D, L, T)
    assert out.basis.dtype == out.activations.dtype == torch.float64
    assert out.status.shape == (B, F) and out.status.dtype == torch.int32
    return host(out.w), host(out.basis), host(out.activations), host(out.spec), host(out.status)


@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
@pytest.mark.parametrize("shape", S.ILRMA, ids=S.ILRMA_IDS)
def test_ilrma(shape, cdtype):
    single = cdtype == np.complex64
    tag = "%s %s" % (shape[:5], np.dtype(cdtype).name)
    got = ilrma_run(shape, cdtype)
    ref = LR.reference(shape, single=single)
    assert not got[4].any() and not ref.status.any()
    r_w = PC.check_three(tag, got[:3], ref[:3], LR.tolerance(shape, single))
    r_y = PC.check_y(tag, got[3], LR.promoted(LR.parity_case(shape).X, single), got[0], got[4], 0, single)
    ratio_line("ilrma", tag, max(r_w, r_y))


@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
@pytest.mark.parametrize("shape", [s for s in S.ILRMA_WALK if s[1] >= 5],
                         ids=[i for s, i in zip(S.ILRMA_WALK, S.ILRMA_IDS) if s[1] >= 5])
def test_ilrma_projects_onto_the_last_microphone(shape, cdtype):
    D = shape[1]
    single = cdtype == np.complex64
    first, last = ilrma_run(shape, cdtype), ilrma_run(shape, cdtype, D - 1)
    assert all(PC.same_bits(a, b) for a, b in zip(first[:3], last[:3])) and np.array_equal(first[4], last[4]) and not last[4].any()
    tag = "%s %s ref %d" % (shape[:5], np.dtype(cdtype).name, D - 1)
    ratio_line("ilrma", tag, PC.check_y(tag, last[3], LR.promoted(LR.parity_case(shape).X, single), last[0], last[4], D - 1, single))


@pytest.mark.parametrize("shape,values", S.ILRMA_LATE_VALUES, ids=[S.ILRMA_IDS[S.ILRMA.index(c)] for c, _ in S.ILRMA_LATE_VALUES])
def test_ilrma_refuses_a_bad_basis_value_past_the_first_64(shape, values):
    """A 0 or a NaN among bin 1's basis0 values at a flat index k L + l >= 64, where the start's scan is on its second trip: the
    bin gets status 1, W = I and Y = X bit for bit and keeps its basis rows as given; the other bins have the bits of a launch
    without that bin's data, and the restatement gives the same status words."""
    B, D, F, T, L = shape[:5]
    b0, a0 = (a.copy() for a in LR.parity_start(shape))
    for i, v in values.items():
        assert i >= 64
        b0[0, i // L, 1, i % L] = v
    X = LR.parity_case(shape).X
    want = np.zeros((B, F), np.int32)
    want[0, 1] = 1
    x, b0d, a0d = dev(X), dev(b0), dev(a0)
    got = SEP.ilrma(x, b0d, a0d, shape[5])
    PC.check_refused_bins("%s with %s" % (shape[:5], values), host(got.status), host(got.w), host(got.spec), X, want)
    assert same_bits(got.basis[0, :, 1], b0d[0, :, 1])
    keep = [0, 2]
    assert bool(torch.isfinite(got.activations).all()) and bool(torch.isfinite(got.basis[:, :, keep]).all())
    alone = SEP.ilrma(x[:, :, keep].contiguous(), b0d[:, :, keep].contiguous(), a0d, shape[5])
    assert not host(alone.status).any()
    assert same_bits(alone.w[0], got.w[0, keep]) and same_bits(alone.spec[0], got.spec[0][:, keep])
    assert same_bits(alone.basis[0], got.basis[0][:, keep]) and same_bits(alone.activations, got.activations)
    assert np.array_equal(LR.ilrma(X, b0, a0, shape[5]).status, want)


def test_ilrma_item_in_a_batch_of_three():
    shape = next(s for s in S.ILRMA if s[1:5] == (5, 3, 70, 13))
    B, D, F, T, L = shape[:5]
    starts = [LR.start(1, D, F, T, L, OTHER[0]), LR.parity_start(shape), LR.start(1, D, F, T, L, OTHER[1])]
    x = dev(np.concatenate([LR.case(1, D, F, T, OTHER[0]).X, LR.parity_case(shape).X, LR.case(1, D, F, T, OTHER[1]).X]))
    b3, a3 = dev(np.concatenate([s[0] for s in starts])), dev(np.concatenate([s[1] for s in starts]))
    whole = SEP.ilrma(x, b3, a3, shape[5], ref=D - 1)
    assert alone_in_the_middle(whole, SEP.ilrma(x[1:2].contiguous(), b3[1:2].contiguous(), a3[1:2].contiguous(), shape[5], ref=D - 1))
    assert PC.same_bits(host(whole.w[1:2]), ilrma_run(shape, np.complex128)[0])


# ---------------------------------------------------------------------------------------------------------------------- cACGMM
@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
@pytest.mark.parametrize("shape", S.CACGMM, ids=S.CACGMM_IDS)
def test_cacgmm(shape, cdtype):
    B, D, K, F, T = shape[:5]
    single = cdtype == np.complex64
    tag = "%s %s" % (shape[:5], np.dtype(cdtype).name)
    c = CR.parity_case(shape)
    out = SEP.cacgmm(dev(c.X.astype(cdtype)), dev(c.init), shape[5])
    assert out.masks.shape == (B, K, F, T) and out.prior.shape == (B, K, T) and out.cov.shape == (B, F, K, D, D)
    assert out.quadratic.shape == (B, K, F, T) and out.status.shape == (B, F)
    got = tuple(host(t) for t in out)
    ref = CR.reference(shape, single=single)
    assert not got[4].any() and not ref.status.any()
    tol = CR.tolerance(shape, single)
    r_m = PC.check_gmm(tag, got, ref, tol)
    assert (np.abs(got[0].sum(axis=1) - 1.0) <= 8 * U).all() and (got[0] >= 0).all() and (got[3] > 0).all()
    r_c = PC.check_gmm_cov(tag, got[2], ref, tol)
    ratio_line("cacgmm", tag, max(r_m, r_c))


def test_cacgmm_item_in_a_batch_of_three():
    shape = next(s for s in S.CACGMM if s[1:3] == (7, 6))
    B, D, K, F, T = shape[:5]
    cases = [CR.case(1, D, K, F, T, OTHER[0]), CR.parity_case(shape), CR.case(1, D, K, F, T, OTHER[1])]
    x, init = dev(np.concatenate([c.X for c in cases])), dev(np.concatenate([c.init for c in cases]))
    whole = SEP.cacgmm(x, init, shape[5])
    assert alone_in_the_middle(whole, SEP.cacgmm(x[1:2].contiguous(), init[1:2].contiguous(), shape[5]))


# --------------------------------------------------------------------------------------------------------------------- scoring
DTYPES = [np.float64, np.float32]
DIDS = ["float64", "float32"]


def gathered(table, perm):
    return torch.gather(table, 2, perm.long()[:, :, None])[:, :, 0]


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("shape", S.SCORING, ids=S.SCORING_IDS)
def test_scores(shape, dtype):
    """The pairs' table has the bits of si_sdr on the K J expanded pairs; the permutation-invariant score recovers the case's
    scramble and gathers its values from the table; SIR and SAR stay within the case's tolerance of the restatement.  The case
    holds three items: each has the bits it has alone."""
    K, J, n = shape
    single = dtype == np.float32
    tag = "%s %s" % (shape, np.dtype(dtype).name)
    c = MR.case(shape)
    s, e = dev(c.references.astype(dtype)), dev(c.estimates.astype(dtype))
    table = SM.pairwise_si_sdr(s, e)
    assert table.shape == (MR.ITEMS, K, J) and table.dtype == torch.float64
    pairs = SM.si_sdr(s[:, :, None].expand(-1, K, J, n).reshape(-1, n), e[:, None].expand(-1, K, J, n).reshape(-1, n))
    assert same_bits(table, pairs.view(MR.ITEMS, K, J)) and bool(torch.isfinite(table).all())
    pit = SM.pit_si_sdr(s, e)
    assert np.array_equal(host(pit.perm), c.scramble) and not host(pit.status).any()
    assert same_bits(pit.value, gathered(table, pit.perm))
    got = SM.si_bss_eval(s, e)
    ref = MR.reference(shape, single)
    assert np.array_equal(host(got.perm), ref.perm) and not host(got.status).any() and not ref.status.any()
    assert same_bits(got.sdr, gathered(table, got.perm))
    tol = PC.si_bss_tolerance(shape, single)
    ratio_line("scoring", tag, PC.check_si_bss(tag, host(got.sir), host(got.sar), host(got.sdr), ref, tol))
    s1, e1 = s[1:2].contiguous(), e[1:2].contiguous()
    whole = (table,) + tuple(pit) + tuple(got)
    alone = (SM.pairwise_si_sdr(s1, e1),) + tuple(SM.pit_si_sdr(s1, e1)) + tuple(SM.si_bss_eval(s1, e1))
    assert alone_in_the_middle(whole, alone)


@pytest.mark.parametrize("maximize", [True, False], ids=["max", "min"])
@pytest.mark.parametrize("K,J", S.ASSIGN_PAIRS, ids=["%d-%d" % p for p in S.ASSIGN_PAIRS])
def test_assign(K, J, maximize):
    """Seeded tables of every K <= J <= 8: Gaussian scores; small integers, whose exact sums repeat (the lowest rank wins); and
    Gaussian scores with one score repeated in another cell of the same table."""
    g = np.random.default_rng([21, K, J])
    tables = [g.standard_normal((4, K, J)) * 20.0, g.integers(0, 3, size=(4, K, J)).astype(np.float64)]
    twice = g.standard_normal((4, K, J))
    twice[:, K - 1, J - 1] = twice[:, 0, 0]
    tables.append(twice)
    for table in tables:
        got = SM.assign(dev(table), maximize=maximize)
        assert got.perm.shape == (4, K) and got.perm.dtype == torch.int32 and got.total.dtype == torch.float64
        want = PC.check_assign("assign %d-%d" % (K, J), (host(got.perm), host(got.total), host(got.status)), table, maximize)
        assert not want.status.any()
        alone = SM.assign(dev(table[1:2]), maximize=maximize)
        assert alone_in_the_middle(got, alone)


# ------------------------------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("shape", S.ALIGN, ids=S.ALIGN_IDS)
def test_alignment(shape):
    B, K, F, T = shape[:4]
    p = dev(AR.parity_case(shape).P)
    counts = range(1, AR.ITERATIONS + 1)
    runs = {}
    for n in counts:
        out = SEP.align_permutations(p, n)
        assert out.perm.shape == (B, F, K) and out.perm.dtype == torch.int32 and out.score.shape == (B, F)
        runs[n] = tuple(host(t) for t in out)
    ratio_line("alignment", shape[:4], PC.check_align(str(shape[:4]), runs, {n: AR.reference(shape, n) for n in counts}, AR.tolerance(shape)))


def test_alignment_item_in_a_batch_of_three():
    shape = next(s for s in S.ALIGN if s[1] == 7)
    B, K, F, T = shape[:4]
    p = dev(np.concatenate([AR.case(1, K, F, T, OTHER[0]).P, AR.parity_case(shape).P, AR.case(1, K, F, T, OTHER[1]).P]))
    for n in (1, 3):
        assert alone_in_the_middle(SEP.align_permutations(p, n), SEP.align_permutations(p[1:2].contiguous(), n))


# --------------------------------------------------------------------------------------------------------- SRP-PHAT and MUSIC
def srp(X, c, shape):
    B, D, T, G, f_lo, f_hi, n_fft = shape
    return LOC.srp_phat(X, dev(c.mics), dev(c.cand), fs=SR.FS, n_fft=n_fft, c=SR.C, band=(f_lo, f_hi))


@pytest.mark.parametrize("cdtype", CDTYPES, ids=CIDS)
@pytest.mark.parametrize("shape", S.SRP, ids=S.SRP_IDS)
def test_srp_phat(shape, cdtype):
    """``best`` is the restatement's arg-max, which tests/test_size_sweep_cpu.py shows to be the true candidate for D >= 3 and
    its mirror image through the pair's plane for D = 2."""
    B, D, T, G, f_lo, f_hi, n_fft = shape
    P, L = D * (D - 1) // 2, min(PC.GCC_LAGS, n_fft // 2)
    tag = "%s %s" % (shape, np.dtype(cdtype).name)
    c, ref = SR.parity_case(shape), SR.reference(shape, single=cdtype == np.complex64)
    X = dev(c.X.astype(cdtype))
    psi = LOC.cross_spectra(X, band=(f_lo, f_hi))
    assert psi.dtype == torch.complex128 and psi.shape == (B, P, n_fft // 2 + 1)
    got = srp(X, c, shape)
    assert got.map.dtype == torch.float64 and got.map.shape == (B, G) and got.best.dtype == torch.int32
    gcc = LOC.gcc_phat(X, L, band=(f_lo, f_hi), n_fft=n_fft)
    assert gcc.corr.shape == (B, P, 2 * L + 1)
    ratio_line("srp", tag, PC.check_srp(tag, shape, host(psi), host(got.map), host(gcc.corr), host(got.best), host(got.status), ref, c))
    if D > 2:
        assert np.array_equal(host(got.best), c.true)


MUSIC_CASES = [(s, K) for s in S.SRP for K in UR.music_orders(s[1])]
MUSIC_IDS = ["%s-K%d" % (i, K) for s, i in zip(S.SRP, S.SRP_IDS) for K in UR.music_orders(s[1])]


@pytest.mark.parametrize("shape,K", MUSIC_CASES, ids=MUSIC_IDS)
def test_music(shape, K):
    """The map alone (the restatement's decomposition uploaded), the chain (its covariances uploaded, device eigh into device
    map) and the whole way from the spectrogram, as tests/test_subspace_gpu.py has them; ``best`` is the true candidate."""
    B, D, T, G, f_lo, f_hi, n_fft = shape
    tag = "%s K=%d" % (shape, K)
    c, ref = SR.parity_case(shape), UR.music_reference(shape, K)
    theta = SR.theta_max(f_hi, UR.FS, n_fft, c.mics, c.cand)
    mics, cand = dev(c.mics), dev(c.cand)
    null, best, status = N.music(dev(ref.V), dev(ref.lam), mics, cand, K, UR.FS, n_fft, UR.C, f_lo, f_hi)
    assert null.dtype == torch.float64 and null.shape == (B, G)
    r_alone = PC.check_music_map(tag + " map alone", host(null), host(best), host(status), ref, ref.bound_alone)
    got = LOC.music_from_covariance(dev(ref.cov), mics, cand, K, n_fft=n_fft, band=(f_lo, f_hi))
    r_chain = PC.check_music_map(tag + " chain", host(got.null), host(got.best), host(got.status), ref,
                                 UR.chain_bound(D, K, theta, ref.norms, ref.gaps, PC.C1))
    res, orth, err = UR.eig_errors(ref.cov, host(got.values), host(SUB.eigh(dev(ref.cov)).vectors), ref.lam)
    print("%s: eigensolver ratios %.3g %.3g %.3g of %d" % (tag, res, orth, err, PC.C1))
    assert max(res, orth, err) <= PC.C1 and np.array_equal(ref.best, c.true)
    ratios = [r_alone, r_chain, max(res, orth, err) / PC.C1]
    for cdtype, single in ((np.complex128, False), (np.complex64, True)):
        full = LOC.music(dev(c.X.astype(cdtype)), mics, cand, K, n_fft=n_fft, band=(f_lo, f_hi))
        want = UR.music_reference(shape, K, single=single)
        assert full.values.shape == (B, n_fft // 2 + 1, D) and np.array_equal(host(full.best), c.true)
        # the covariance's own rounding, as tests/test_subspace_gpu.py derives it
        extra = np.mean(4 * np.sqrt(D) * (T + 4) * U * want.norms / want.gaps, axis=1)
        ratios.append(PC.check_music_map("%s from the %s spectrogram" % (tag, np.dtype(cdtype).name), host(full.null), host(full.best),
                                         host(full.status), want, UR.chain_bound(D, K, theta, want.norms, want.gaps, PC.C1) + extra))
    ratio_line("music", tag, max(ratios))


def test_srp_and_music_item_in_a_batch_of_three():
    """Three different items over one geometry (the case's, then two more draws of its builder): the middle one has the bits it
    has alone, at D = 7."""
    shape = next(s for s in S.SRP if s[1] == 7)
    B, D, T, G, f_lo, f_hi, n_fft = shape
    c = SR.parity_case(shape)
    others = [SR.case(1, D, T, G, seed, n_fft) for seed in OTHER]
    X = dev(np.concatenate([others[0].X, c.X, others[1].X]))
    assert alone_in_the_middle(srp(X, c, shape), srp(X[1:2].contiguous(), c, shape))
    assert same_bits(LOC.cross_spectra(X, band=(f_lo, f_hi))[1], LOC.cross_spectra(X[1:2].contiguous(), band=(f_lo, f_hi))[0])
    for K in UR.music_orders(D):
        whole = LOC.music(X, dev(c.mics), dev(c.cand), K, n_fft=n_fft, band=(f_lo, f_hi))
        alone = LOC.music(X[1:2].contiguous(), dev(c.mics), dev(c.cand), K, n_fft=n_fft, band=(f_lo, f_hi))
        assert alone_in_the_middle(whole, alone)


# ------------------------------------------------------------------------------------------------------- beamforming and GEV
def mask_of(c, kind):
    return None if kind == "ones" else dev(c.masks[kind])         # "ones": the null mask, which the restatement takes as 1


def hermitian_bits(cov):
    """Above the diagonal the conjugate of below it, on it an imaginary part of +0, as bits."""
    D = cov.shape[-1]
    i, j = torch.tril_indices(D, D, -1)
    low, up = cov[..., i, j], cov[..., j, i]
    diag = torch.diagonal(cov, dim1=-2, dim2=-1).imag
    return same_bits(up.real, low.real) and same_bits(up.imag, -low.imag) and same_bits(diag, torch.zeros_like(diag))


@pytest.mark.parametrize("kind", BR.MASKS)
@pytest.mark.parametrize("shape", S.BEAMFORM, ids=S.BEAMFORM_IDS)
def test_beamform(shape, kind):
    """The covariance (complex128 and complex64), the four weight solves from the restatement's covariances, and apply."""
    B, D, F, T, loading = shape
    c = BR.parity_case(shape)
    ratios = []
    for cdtype in CDTYPES:
        single = cdtype == np.complex64
        ref = BR.reference(shape, kind, single=single)
        got = BF.spatial_covariance(dev(c.X.astype(cdtype)), mask_of(c, kind))
        assert got.cov.dtype == torch.complex128 and got.cov.shape == (B, F, D, D) and not host(got.status).any()
        assert hermitian_bits(got.cov)
        ratios.append(PC.check_cov(got.cov, ref.cov, ref.scale, T, "%s %s %s" % (np.dtype(cdtype).name, shape[:4], kind)))
    ref = BR.reference(shape, kind)
    A = dev(c.A)
    runs = {"das": BF.weights("das", steering=A),
            "mpdr": BF.weights("mvdr", dev(ref.cov), A, loading=loading),
            "mvdr": BF.weights("mvdr", dev(ref.cov_n), A, loading=loading),
            "souden": BF.weights("souden", dev(ref.cov_n), speech_cov=dev(ref.cov_s), loading=loading)}
    tag = "%s %s" % (shape[:4], kind)
    for name, got in runs.items():
        assert got.w.shape == (B, F, D) and not host(got.status).any(), name
        ratios.append(PC.check_weights(tag, name, host(got.w), ref.W[name], None if name == "das" else ref.cond[name]))
    other = BF.weights("souden", dev(ref.cov_n), speech_cov=dev(ref.cov_s), loading=loading, ref=D - 1)         # another reference
    want, _ = BR.weights(BR.SOUDEN, ref.cov_n, ref.cov_s, ref=D - 1, loading=loading)
    ratios.append(PC.check_weights(tag, "souden ref %d" % (D - 1), host(other.w), want, ref.cond["souden"]))
    for cdtype in CDTYPES:
        x = dev(c.X.astype(cdtype))
        w = BF.weights("mvdr", BF.spatial_covariance(x, mask_of(c, kind)).cov, A, loading=loading).w
        y = BF.apply(x, w)
        assert y.dtype == x.dtype and y.shape == (B, F, T)
        ratios.append(PC.check_apply("%s %s apply" % (tag, np.dtype(cdtype).name), host(y), c.X.astype(cdtype).astype(np.complex128),
                                     host(w), cdtype == np.complex64))
    ratio_line("beamform", tag, max(ratios))


@pytest.mark.parametrize("kind", BR.MASKS)
@pytest.mark.parametrize("shape", S.BEAMFORM, ids=S.BEAMFORM_IDS)
def test_gev(shape, kind):
    B, D, F, T, loading = shape
    souden = BR.reference(shape, kind).W["souden"]
    for variant in UR.GEV_VARIANTS:
        for ref in S.GEV_REFS:
            tag = "%s %s %s ref %d" % (shape[:4], kind, variant, ref)
            g = UR.gev_reference(shape, kind, variant, ref)
            got = BF.gev_weights(dev(g.Phi_n), dev(g.Phi_s), ref=ref, loading=loading)
            assert got.w.dtype == torch.complex128 and got.w.shape == (B, F, D) and got.rtf.shape == (B, F, D)
            w = host(got.w)
            ratio_line("gev", tag, PC.check_gev(tag, w, host(got.rtf), host(got.gain), host(got.status), g, ref))
            if ref == 0:                                  # the Rayleigh quotient: no weights do better, Souden's included
                P = BR.loaded(g.Phi_n, loading)
                unit = UR.gev_bound(D, g.cond, g.normC, g.gapC, 1.0, PC.C2)

                def quotient(v):
                    num = np.einsum("bfi,bfij,bfj->bf", np.conj(v), g.Phi_s, v).real
                    return num / np.einsum("bfi,bfij,bfj->bf", np.conj(v), P, v).real
                assert (quotient(w) >= quotient(souden) * (1 - unit)).all()


def test_beamform_and_gev_item_in_a_batch_of_three():
    shape = S.BEAMFORM[0]
    B, D, F, T, loading = shape
    cases = [BR.case(1, D, F, T, OTHER[0], loading), BR.parity_case(shape), BR.case(1, D, F, T, OTHER[1], loading)]
    x = dev(np.concatenate([c.X for c in cases]))
    noise, speech = (dev(np.concatenate([c.masks[kind] for c in cases])) for kind in ("runs", "uniform"))
    for ref in S.GEV_REFS:
        whole = BF.gev(x, noise, speech, ref=ref, loading=loading)
        alone = BF.gev(x[1:2].contiguous(), noise[1:2].contiguous(), speech[1:2].contiguous(), ref=ref, loading=loading)
        assert not host(whole.status).any() and alone_in_the_middle(whole, alone)
    A = dev(np.concatenate([c.A for c in cases]))
    cov = BF.spatial_covariance(x, noise)
    w = BF.weights("mvdr", cov.cov, A, loading=loading)
    cov1 = BF.spatial_covariance(x[1:2].contiguous(), noise[1:2].contiguous())
    w1 = BF.weights("mvdr", cov1.cov, A[1:2].contiguous(), loading=loading)
    assert same_bits(cov1.cov[0], cov.cov[1]) and same_bits(w1.w[0], w.w[1])
    assert same_bits(BF.apply(x[1:2].contiguous(), w1.w)[0], BF.apply(x, w.w)[1])
