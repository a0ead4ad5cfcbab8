"""The size sweep of the array kernels: one case for every size a kernel is compiled for -- the microphone count D, the class or
source count K, the estimate count J, ILRMA's rank L -- in the tuple format of the family's own ``*_ref.py``, so that its
``reference``, ``tolerance``, ``w_tolerance``, ``y_bound``, ``gev_bound`` and ``chain_bound`` take the cases as they are.  The
families' PARITY / SHAPES lists were chosen for frame-tiling edges; these are chosen for the template size, and are small: one
item, 2 to 5 bins, about 70 frames (one whole 64-frame tile and a ragged one) unless a comment says otherwise.
tests/test_size_sweep_cpu.py asserts that every compiled size is here and that every case meets its family's conditions on the
restatement alone; tests/test_size_sweep_gpu.py holds the kernels to them.

Seeds are literals: for each case the first of 0, 1, 2, ... under which the restatement alone meets the family's conditions (the
rule of iva_ref.PARITY and cacgmm_ref.PARITY).  The families whose case builders take no seed have none here."""

SIZES_D = range(1, 9)            # AuxIVA, ILRMA, beamforming
SIZES_D2 = range(2, 9)           # cACGMM, SRP-PHAT, MUSIC: a pair of microphones at the least
SIZES_K = range(1, 9)            # classes, sources, estimates
SIZES_L = range(1, 17)           # ILRMA's rank

# ---------------------------------------------------------------------------------------------------------------------- AuxIVA
# (B, D, F, T, iterations, seed) of iva_ref.  A well-conditioned W V_k (kappa <= 1e4) of D = 8 microphones from 70 frames is
# rare: seed 1423 is the first.
IVA = [(1, 1, 2, 70, 5, 0),
       (1, 2, 2, 70, 5, 0),
       (1, 3, 2, 70, 5, 0),
       (1, 4, 2, 70, 5, 4),
       (1, 5, 2, 70, 5, 12),              # the projection's one pass per source starts here
       (1, 6, 2, 70, 5, 31),
       (1, 7, 2, 70, 5, 197),
       (1, 8, 2, 70, 5, 1423),
       (1, 3, 2, 33, 5, 6),               # a row shorter than a wave with D >= 2: the lanes past the row
       (1, 1, 2, 1, 5, 0)]                # one frame; D = 1 only: with D >= 2 such a bin's covariance has rank one, and whether
#                                           its pivot is exactly 0 depends on the rounding
IVA_IDS = ["-".join(str(v) for v in s[:4]) for s in IVA]

# ----------------------------------------------------------------------------------------------------------------------- ILRMA
# (B, D, F, T, L, iterations, seed) of ilrma_ref: a diagonal walk, every L once with D cycling -- (5, 13) and (8, 16) have
# D L > 64, the second trip of the start's scan of a bin's basis values -- then the row-sum chain of lam past its 64-bin chunk
# (F = 65, F = 128) and a row shorter than a wave.
ILRMA = [(1, 1, 3, 70, 1, 5, 0),
         (1, 2, 3, 70, 2, 5, 0),
         (1, 3, 3, 70, 3, 5, 0),
         (1, 4, 3, 70, 4, 5, 0),
         (1, 5, 3, 70, 5, 5, 2),
         (1, 6, 3, 70, 6, 5, 2),
         (1, 7, 3, 70, 7, 5, 3),
         (1, 8, 3, 70, 8, 5, 7),
         (1, 1, 3, 70, 9, 5, 0),
         (1, 2, 3, 70, 10, 5, 0),
         (1, 3, 3, 70, 11, 5, 0),
         (1, 4, 3, 70, 12, 5, 0),
         (1, 5, 3, 70, 13, 5, 2),         # D L = 65
         (1, 6, 3, 70, 14, 5, 2),         # D L = 84
         (1, 7, 3, 70, 15, 5, 3),         # D L = 105
         (1, 8, 3, 70, 16, 5, 7),         # D L = 128: a whole second trip
         (1, 2, 65, 70, 9, 5, 2),         # one bin past the chunk
         (1, 2, 128, 70, 12, 5, 0),       # two whole chunks
         (1, 3, 3, 33, 11, 5, 0)]
ILRMA_IDS = ["-".join(str(v) for v in s[:5]) for s in ILRMA]
ILRMA_WALK = ILRMA[:16]
# two of the cases whose D L > 64, and per case the flat indices (k L + l, all >= 64) of the basis0 values of bin 1 that the status test
# replaces, with what
ILRMA_LATE_VALUES = [(ILRMA[12], {64: float("nan")}), (ILRMA[15], {64: 0.0, 127: float("nan")})]

# ---------------------------------------------------------------------------------------------------------------------- cACGMM
# (B, D, K, F, T, iterations, seed) of cacgmm_ref: D and K vary independently; K is a run-time size (waves per workgroup, LDS
# columns), and (7, 6) and (8, 5) have K D D > 256 beside the family's own (8, 8).
CACGMM = [(1, 2, 3, 3, 70, 5, 0),
          (1, 3, 7, 3, 70, 5, 0),
          (1, 4, 8, 3, 70, 5, 0),
          (1, 5, 4, 3, 70, 5, 0),
          (1, 6, 5, 3, 70, 5, 0),
          (1, 7, 6, 3, 70, 5, 0),
          (1, 8, 5, 3, 70, 5, 1),
          (1, 4, 1, 3, 70, 5, 0),
          (1, 6, 2, 3, 70, 5, 0)]
CACGMM_IDS = ["-".join(str(v) for v in s[:5]) for s in CACGMM]

# --------------------------------------------------------------------------------------------------------------------- scoring
# (K, J, n) of separation_metrics_ref (three items a case; its builder needs K <= J and takes no seed): n below a wave, above it,
# above a workgroup.  At n = 63 and 65 the envelope has one or two blocks and many (K, J) miss the family's conditions
# (cond_2(G) <= 100, the scramble recovered); these are combinations that meet them, the large K at n = 257.
SCORING = [(1, 4, 63), (2, 5, 63), (3, 6, 257), (4, 7, 257), (5, 8, 65), (6, 6, 65), (7, 8, 65), (8, 8, 257),
           (7, 7, 257), (1, 1, 257), (2, 2, 65), (3, 3, 65), (5, 5, 63)]
SCORING_IDS = ["-".join(str(v) for v in s) for s in SCORING]
ASSIGN_PAIRS = [(K, J) for J in SIZES_K for K in range(1, J + 1)]          # all 36

# ------------------------------------------------------------------------------------------------------------------- alignment
# (B, K, F, T, seed) of align_ref.  The search hands K! / 6 prefixes to a workgroup's threads: beside K = 8, K = 7 (840
# prefixes) is the one size at which a thread takes more than one trip.
ALIGN = [(1, 1, 5, 66, 0), (1, 2, 5, 66, 1), (1, 3, 5, 66, 0), (1, 4, 5, 66, 0), (1, 5, 5, 66, 0), (1, 6, 5, 66, 0),
         (1, 7, 5, 66, 0), (1, 8, 5, 66, 0)]
ALIGN_IDS = ["-".join(str(v) for v in s[:4]) for s in ALIGN]

# --------------------------------------------------------------------------------------------------------- SRP-PHAT and MUSIC
# (B, D, T, G, f_lo, f_hi, n_fft) of srp_ref (its builder derives the seed from the shape); MUSIC takes each with the
# signal-subspace sizes of subspace_ref.music_orders(D).  At D = 2 a candidate and its mirror image through the pair have the
# same delay difference, and the mirror wins the restatement's SRP map: the device is held to the restatement's arg-max.
SRP = [(1, D, 5, 37, 8, 60, 400) for D in SIZES_D2]
SRP_IDS = ["-".join(str(v) for v in s) for s in SRP]

# ------------------------------------------------------------------------------------------------------- beamforming and GEV
# (B, D, F, T, loading) of beamform_ref: the one D its PARITY leaves out, under all three masks, both GEV variants, ref 0 and 5.
BEAMFORM = [(1, 6, 2, 65, 1e-10)]
BEAMFORM_IDS = ["-".join(str(v) for v in s[:4]) for s in BEAMFORM]
GEV_REFS = (0, 5)
