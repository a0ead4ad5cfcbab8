"""The eigendecomposition of small Hermitian matrices on the device (csrc/subspace.hip, csrc/herm_eig.h): what the subspace
methods of the array chain stand on -- ``localization.music`` reads the eigenvectors of the spatial covariances,
``beamforming.gev_weights`` runs the same solver inside its kernel.  One problem per matrix, a wave each; float64 cyclic
Jacobi in a fixed order, no host sync, no solver library.

    from acoustic_locating_vq_vae import beamforming as BF, subspace as SUB
    cov = BF.spatial_covariance(spec).cov                  # (B, F, D, D) complex128
    values, vectors, status = SUB.eigh(cov)                # (B, F, D) ascending, (B, F, D, D) columns, (B, F) int32

Definition (in full: include/alvq.h).  Only the lower triangle and the real part of the diagonal are read.  Round-robin
cyclic Jacobi; a pair is rotated while |a_pq| > 0.5 u ||A||_F / D, u = 2^-53; a sweep without a rotation ends the run, after
16 sweeps at the latest.  ``values`` ascend (numpy's order) and column k of ``vectors`` belongs to ``values[k]``, scaled by a
unit phasor so that its component of the largest modulus (the lowest index on ties) is real and positive.  A = 0 gives
values 0 and vectors I.  ``status`` (int32 per matrix) is 0, 1 = a non-finite entry was read (values and vectors are NaN) or
2 = no convergence in 16 sweeps (the results as they stand).  Nothing here reads it: the caller does, when it can sync.  A
matrix has the same bits alone, in any batch and on any run.
"""
import collections

import torch

from . import _native as N
from . import _rules as rules

Eigh = collections.namedtuple("Eigh", "values vectors status")

MAX_ORDER = 8


def eigh(cov):
    """cov (..., D, D) complex128 on the GPU, 1 <= D <= 8, Hermitian (the lower triangle is read) -> ``Eigh(values (..., D)
    float64, vectors (..., D, D) complex128, status (...) int32)``."""
    who = "eigh"
    if not isinstance(cov, torch.Tensor) or cov.dim() < 2 or cov.dtype != torch.complex128:
        raise ValueError("%s: cov must be a complex128 (..., D, D) tensor" % who)
    D = cov.shape[-1]
    if cov.shape[-2] != D or D < 1 or D > MAX_ORDER:
        raise ValueError("%s: need square matrices of order 1 <= D <= 8, got shape %s" % (who, tuple(cov.shape)))
    lead = tuple(cov.shape[:-2])
    n = 1
    for s in lead:
        n *= s
    if n < 1 or n > 2 ** 31 - 1:
        raise ValueError("%s: need 1 <= the number of matrices <= 2^31 - 1, got shape %s" % (who, tuple(cov.shape)))
    rules.on_gpu(who, cov, "cov")
    values, vectors, status = N.eigh(cov.reshape(n, D, D))
    return Eigh(values.view(lead + (D,)), vectors.view(lead + (D, D)), status.view(lead))
