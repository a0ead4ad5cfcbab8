"""ctypes binding of libalvq.so (include/alvq.h) -- the only door from Python to the HIP kernels.

PyTorch is used for device memory and streams only: every function here takes torch CUDA(=HIP) tensors,
checks shape/dtype/contiguity on the host, and passes raw ``data_ptr()``s plus the current HIP stream to
the C ABI.  There is no CPU fallback: if the library is missing or a tensor is not on the GPU the call
raises.
"""
from __future__ import annotations

import collections
import ctypes
import functools
import os

import torch

_LIB = None
_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB = os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libalvq.so"))

W_OIK = 0
W_IOK = 1
VQ_PARTIALS = 1024
EW_PARTIALS = 1024

_c_void_p = ctypes.c_void_p
_i32 = ctypes.c_int
_i64 = ctypes.c_int64
_f32 = ctypes.c_float

def _signatures(table):
    """``alvq_<stem>_f32|f64`` stands for two entry points of one signature, ``alvq_<stem>_f32`` and ``alvq_<stem>_f64``."""
    return {name: sig for key, sig in table.items()
            for name in ([key[:-7] + "f32", key[:-7] + "f64"] if key.endswith("f32|f64") else [key])}


_SIGNATURES = _signatures({
    "alvq_version": (ctypes.c_char_p, []),
    "alvq_last_error": (ctypes.c_char_p, []),
    "alvq_set_option": (_i32, [ctypes.c_char_p, _i64]),
    "alvq_get_option": (_i64, [ctypes.c_char_p]),
    "alvq_conv1d_f32": (_i32, [_c_void_p] * 9 + [_i32] * 7 + [_c_void_p]),
    "alvq_conv1d_wgrad_workspace_bytes": (_i64, [_i32] * 5),
    "alvq_conv1d_wgrad_f32": (_i32, [_c_void_p] * 5 + [_i32] * 7 + [_c_void_p]),
    "alvq_vq_argmin_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "alvq_vq_argmin_f32": (_i32, [_c_void_p] * 5 + [_i64, _i32, _i32, _c_void_p]),
    "alvq_vq_gather_loss_f32": (_i32, [_c_void_p] * 6 + [_i64, _i32, _i32, _c_void_p]),
    "alvq_vq_finalize_f32": (_i32, [_c_void_p] * 3 + [_i64, _i32, _i32, _f32, _c_void_p]),
    "alvq_vq_finalize_ema_f32": (_i32, [_c_void_p] * 3 + [_i64, _i32, _i32, _f32, _c_void_p]),
    "alvq_vq_backward_workspace_bytes": (_i64, [_i32, _i32]),
    "alvq_vq_backward_f32": (_i32, [_c_void_p] * 8 + [_i64, _i32, _i32, _f32, _c_void_p]),
    "alvq_onehot_f32": (_i32, [_c_void_p, _c_void_p, _i64, _i32, _c_void_p]),
    "alvq_jitter_gather_f32": (_i32, [_c_void_p] * 3 + [_i64, _i32, _i32, _c_void_p]),
    "alvq_standardise_f32": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p]),
    "alvq_mse_f32": (_i32, [_c_void_p] * 4 + [_i64, _c_void_p]),
    "alvq_mse_backward_f32": (_i32, [_c_void_p] * 4 + [_i64, _c_void_p]),
    "alvq_fill_f32": (_i32, [_c_void_p, _f32, _i64, _c_void_p]),
    "alvq_add_f32": (_i32, [_c_void_p] * 3 + [_i64, _c_void_p]),
    "alvq_relu_mask_f32": (_i32, [_c_void_p] * 3 + [_i64, _c_void_p]),
    "alvq_row_mean_f32": (_i32, [_c_void_p] * 2 + [_i64, _i32, _c_void_p]),
    "alvq_row_mean_backward_f32": (_i32, [_c_void_p] * 2 + [_i64, _i32, _c_void_p]),
    "alvq_transpose_f32": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p]),
    "alvq_adam_f32": (_i32, [_c_void_p] * 4 + [_i64, _i32, _f32, _f32, _f32, _f32, _f32, _c_void_p]),
    "alvq_adam_dev_f32": (_i32, [_c_void_p] * 4 + [_i64, _c_void_p, _f32, _f32, _f32, _c_void_p, _c_void_p]),
    "alvq_adam_advance_f32": (_i32, [_c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _c_void_p, _c_void_p]),
    "alvq_range_flag_to_slot": (_i32, [_c_void_p, _c_void_p]),
    "alvq_stft_power_f32|f64": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p]),
    "alvq_stft_complex_f32|f64": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p]),
    "alvq_fir_same_f64": (_i32, [_c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p]),
    "alvq_spec_rir_wiener_f64": (_i32, [_c_void_p] * 7 + [_i32, _i32, _i32, _c_void_p]),
    "alvq_rows_to_nlc": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i32, _i32, _c_void_p]),
    "alvq_rows_to_nlc_max_std_rows": (_i32, []),
    "alvq_nlc_rows": (_i64, [_i32, _i32]),
    "alvq_nlc_channels": (_i32, [_i32]),
    "alvq_nlc_guard_rows": (_i32, []),
    "alvq_packed_weight_elems": (_i64, [_i32, _i32, _i32]),
    "alvq_pack_weight_bf16": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p]),
    "alvq_pack_weights_bf16_batch": (_i32, [_c_void_p, _i32, _i32, _c_void_p]),
    "alvq_adam_pack_batch": (_i32, [_c_void_p, _i32, _i32, _c_void_p, _f32, _f32, _f32, _c_void_p, _c_void_p]),
    "alvq_adam_segments_f32": (_i32, [_c_void_p] * 4 + [_c_void_p, _c_void_p, _i32, _c_void_p, _f32, _f32, _f32, _c_void_p, _c_void_p]),
    "alvq_ncl_to_nlc_bf16": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p]),
    "alvq_nlc_to_ncl_f32": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p]),
    "alvq_relu_mask_bf16": (_i32, [_c_void_p] * 3 + [_i64, _c_void_p]),
    "alvq_conv1d_bf16": (_i32, [_c_void_p] * 10 + [_i32] * 6 + [_c_void_p] * 3),
    "alvq_conv1d_wgrad_bf16_workspace_bytes": (_i64, [_i32] * 5),
    "alvq_conv1d_wgrad_bf16": (_i32, [_c_void_p] * 5 + [_i32] * 7 + [_c_void_p]),
    "alvq_conv1d_wgrad_bf16_multi": (_i32, [_c_void_p, _c_void_p, _i32, _c_void_p, _c_void_p] + [_i32] * 7 + [_c_void_p]),
    "alvq_nlc_plane_bytes": (_i64, [_i32, _i32, _i32]),
    "alvq_pack_weight_bf16x3": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p]),
    "alvq_ncl_to_nlc_bf16x3": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p]),
    "alvq_nlc_to_ncl_bf16x3": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p]),
    "alvq_relu_mask_bf16x3": (_i32, [_c_void_p] * 3 + [_i32, _i32, _i32, _c_void_p]),
    "alvq_conv1d_bf16x3": (_i32, [_c_void_p] * 10 + [_i32] * 6 + [_c_void_p]),
    "alvq_conv1d_wgrad_bf16x3_workspace_bytes": (_i64, [_i32] * 5),
    "alvq_conv1d_wgrad_bf16x3": (_i32, [_c_void_p] * 5 + [_i32] * 7 + [_c_void_p]),
    "alvq_grad_scale_f32": (_i32, [_c_void_p, _i64, _c_void_p, _c_void_p]),
    "alvq_f16mx_range_flag": (_i32, [_c_void_p, _i32, _c_void_p]),
    "alvq_ncl_to_nlc_f16mx": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p, _c_void_p]),
    "alvq_nlc_to_ncl_f16mx": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p, _c_void_p]),
    "alvq_relu_mask_f16mx": (_i32, [_c_void_p] * 3 + [_i32, _i32, _i32, _c_void_p]),
    "alvq_conv1d_f16mx": (_i32, [_c_void_p] * 10 + [_i32] * 6 + [_c_void_p] * 4),
    "alvq_conv1d_wgrad_f16mx_workspace_bytes": (_i64, [_i32] * 5),
    "alvq_conv1d_wgrad_f16mx": (_i32, [_c_void_p] * 5 + [_i32] * 7 + [_c_void_p, _c_void_p]),
    "alvq_conv1d_wgrad_bf16x3_multi": (_i32, [_c_void_p, _c_void_p, _i32, _c_void_p, _c_void_p] + [_i32] * 7 + [_c_void_p]),
    "alvq_conv1d_wgrad_f16mx_multi": (_i32, [_c_void_p, _c_void_p, _i32, _c_void_p, _c_void_p] + [_i32] * 7 + [_c_void_p, _c_void_p]),
    "alvq_conv1d_wgrad_bf16_splits": (_i32, [_i32] * 7),
    "alvq_conv1d_wgrad_bf16x3_splits": (_i32, [_i32] * 6),
    "alvq_conv1d_wgrad_f16mx_splits": (_i32, [_i32] * 6),
    "alvq_ncl_to_nlc_f16": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p, _c_void_p]),
    "alvq_nlc_to_ncl_f16": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p, _c_void_p]),
    "alvq_conv1d_f16": (_i32, [_c_void_p] * 10 + [_i32] * 6 + [_c_void_p] * 4),
    "alvq_conv1d_wgrad_f16": (_i32, [_c_void_p] * 5 + [_i32] * 7 + [_c_void_p, _c_void_p]),
    "alvq_conv1d_wgrad_f16_multi": (_i32, [_c_void_p, _c_void_p, _i32, _c_void_p, _c_void_p] + [_i32] * 7 + [_c_void_p, _c_void_p]),
    "alvq_conv1d_wgrad_bf16_bias_offset": (_i64, [_i32] * 5),
    "alvq_wgrad_reduce_batch": (_i32, [_c_void_p, _i32, _c_void_p]),
    "alvq_onehot_to_index_f32": (_i32, [_c_void_p] * 3 + [_i64, _i32, _c_void_p]),
    "alvq_indices_to_i32": (_i32, [_c_void_p] * 3 + [_i64, _i32, _c_void_p]),
    "alvq_embedding_bag_fwd_f32": (_i32, [_c_void_p] * 4 + [_i32] * 4 + [_c_void_p] * 2),
    "alvq_embedding_bag_bwd_f32": (_i32, [_c_void_p] * 4 + [_i32] * 5 + [_c_void_p] * 2),
    "alvq_istft_f32|f64": (_i32, [_c_void_p] * 3 + [_i32] * 5 + [_c_void_p]),
    "alvq_griffin_lim_workspace_bytes": (_i64, [_i32] * 4),
    "alvq_griffin_lim_f32|f64": (_i32, [_c_void_p] * 4 + [_i32] * 6 + [ctypes.c_double, _c_void_p]),
    "alvq_rir_f64": (_i32, [_c_void_p] * 3 + [_i32] * 2 + [ctypes.c_double] * 3 + [_c_void_p] + [ctypes.c_double] * 2
                     + [_i32] * 2 + [_c_void_p]),
    "alvq_rir_rooms_f64": (_i32, [_c_void_p] * 6 + [_i32] * 2 + [ctypes.c_double] * 2 + [_i32] * 2 + [_c_void_p]),
    "alvq_edc_f32|f64": (_i32, [_c_void_p] * 2 + [_i32] * 2 + [_c_void_p]),
    "alvq_room_acoustics_f32|f64": (_i32, [_c_void_p] * 4 + [_i32] * 2 + [ctypes.c_double] + [_i32] * 3 + [_c_void_p]),
    "alvq_resample_poly_f32|f64": (_i32, [_c_void_p] * 3 + [_i32] * 5 + [_c_void_p]),
    "alvq_stoi_workspace_bytes": (_i64, [_i32] * 2),
    "alvq_stoi_f64": (_i32, [_c_void_p] * 8 + [_i32] * 2 + [_c_void_p]),
    "alvq_si_sdr_f32|f64": (_i32, [_c_void_p] * 3 + [_i32] * 2 + [_c_void_p]),
    "alvq_lsd_f32|f64": (_i32, [_c_void_p] * 3 + [_i32] * 3 + [ctypes.c_double, _c_void_p]),
    "alvq_pairwise_si_sdr_f32|f64": (_i32, [_c_void_p] * 3 + [_i32] * 4 + [_c_void_p]),
    "alvq_assign_f64": (_i32, [_c_void_p] * 4 + [_i32] * 4 + [_c_void_p]),
    "alvq_si_bss_eval_f32|f64": (_i32, [_c_void_p] * 7 + [_i32] * 4 + [_c_void_p]),
    "alvq_wpe_workspace_bytes": (_i64, [_i32] * 5),
    "alvq_wpe_f32|f64": (_i32, [_c_void_p] * 4 + [_i32] * 8 + [ctypes.c_double] * 2 + [_c_void_p]),
    "alvq_phat_cross_spectra_f32|f64": (_i32, [_c_void_p] * 3 + [_i32] * 6 + [_c_void_p]),
    "alvq_gcc_phat_f64": (_i32, [_c_void_p] * 2 + [_i32] * 6 + [_c_void_p]),
    "alvq_srp_phat_f64": (_i32, [_c_void_p] * 6 + [_i32] * 3 + [_i64] * 2 + [ctypes.c_double, _i32, ctypes.c_double, _i32, _i32,
                                                                            _c_void_p]),
    "alvq_spatial_covariance_f32|f64": (_i32, [_c_void_p] * 4 + [_i32] * 4 + [_c_void_p]),
    "alvq_steering_vectors_f64": (_i32, [_c_void_p] * 4 + [_i32] * 3 + [ctypes.c_double, _i32, ctypes.c_double, _i32, _i32, _c_void_p]),
    "alvq_beamform_weights_f64": (_i32, [_c_void_p] * 5 + [_i32] * 5 + [ctypes.c_double, _c_void_p]),
    "alvq_beamform_apply_f32|f64": (_i32, [_c_void_p] * 3 + [_i32] * 4 + [_c_void_p]),
    "alvq_beamform_gev_f64": (_i32, [_c_void_p] * 6 + [_i32] * 4 + [ctypes.c_double, _c_void_p]),
    "alvq_eigh_f64": (_i32, [_c_void_p] * 4 + [_i64, _i32, _c_void_p]),
    "alvq_music_f64": (_i32, [_c_void_p] * 7 + [_i32] * 5 + [ctypes.c_double, _i32, ctypes.c_double] + [_i32] * 4 + [_c_void_p]),
    "alvq_auxiva_workspace_bytes": (_i64, [_i32] * 4),
    "alvq_auxiva_f32|f64": (_i32, [_c_void_p] * 6 + [_i32] * 7 + [ctypes.c_double, _c_void_p]),
    "alvq_separation_masks_f32|f64": (_i32, [_c_void_p] * 2 + [_i32] * 4 + [_c_void_p]),
    "alvq_ilrma_workspace_bytes": (_i64, [_i32] * 5),
    "alvq_ilrma_f32|f64": (_i32, [_c_void_p] * 10 + [_i32] * 7 + [ctypes.c_double, _c_void_p]),
    "alvq_cacgmm_workspace_bytes": (_i64, [_i32] * 5),
    "alvq_cacgmm_f32|f64": (_i32, [_c_void_p] * 9 + [_i32] * 6 + [ctypes.c_double, _c_void_p]),
    "alvq_align_workspace_bytes": (_i64, [_i32] * 4),
    "alvq_align_permutations_f64": (_i32, [_c_void_p] * 7 + [_i32] * 5 + [_c_void_p]),
    "alvq_permute_bins": (_i32, [_c_void_p] * 3 + [_i32] * 5 + [_c_void_p]),
    "alvq_tsne_code_sqdist_f32": (_i32, [_c_void_p] * 2 + [_i32] * 2 + [_c_void_p]),
    "alvq_tsne_affinities_workspace_bytes": (_i64, [_i32]),
    "alvq_tsne_affinities_f32": (_i32, [_c_void_p] * 4 + [_i32, ctypes.c_double, _c_void_p]),
    "alvq_tsne_descend_workspace_bytes": (_i64, [_i32]),
    "alvq_tsne_descend_f64": (_i32, [_c_void_p] * 7 + [_i32] * 2 + [ctypes.c_double] * 3 + [_c_void_p]),
    "alvq_kmeans_update_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "alvq_kmeans_update_f32": (_i32, [_c_void_p] * 9 + [_i64, _i32, _i32, ctypes.c_double, _c_void_p]),
    "alvq_kmeans_inertia_workspace_bytes": (_i64, [_i64]),
    "alvq_kmeans_inertia_f32": (_i32, [_c_void_p] * 5 + [_i64, _i32, _i32, _c_void_p]),
    "alvq_kmeans_col_stats_workspace_bytes": (_i64, [_i64, _i32]),
    "alvq_kmeans_col_stats_f32": (_i32, [_c_void_p] * 4 + [_i64, _i32, _c_void_p]),
    "alvq_kmeans_add_rows_f32": (_i32, [_c_void_p] * 3 + [_i64, _i32, _f32, _c_void_p]),
    "alvq_kmeans_plusplus_workspace_bytes": (_i64, [_i64, _i32]),
    "alvq_kmeans_plusplus_f32": (_i32, [_c_void_p] * 5 + [_i64, _i32, _i32, _i32, _i64, _c_void_p]),
    "alvq_vq_ema_stats_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "alvq_vq_ema_stats_f32": (_i32, [_c_void_p] * 5 + [_i64, _i32, _i32, _c_void_p]),
    "alvq_vq_ema_update_f32": (_i32, [_c_void_p] * 6 + [_i32, _i32, ctypes.c_double, ctypes.c_double, _c_void_p]),
    "alvq_vq_restart_gather_f32": (_i32, [_c_void_p] * 4 + [_i64, _i32, _i32, _i32, _i32, _c_void_p]),
    "alvq_vq_restart_dead_f32": (_i32, [_c_void_p] * 6 + [_i32, _i32, _i32, _f32, _c_void_p]),
    "alvq_adam_advance_sched_f32": (_i32, [_c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _c_void_p,
                                           _c_void_p, _i64, _i64, ctypes.c_double]),
    "alvq_grad_clip_workspace_bytes": (_i64, [_i64]),
    "alvq_grad_clip_f32": (_i32, [_c_void_p, _i64, _c_void_p, ctypes.c_double, _c_void_p, _c_void_p, _c_void_p]),
})

EXPORTS = tuple(_SIGNATURES)


def lib_path():
    return os.environ.get("ALVQ_LIB", _DEFAULT_LIB)


def lib():
    """Open libalvq.so once per process (module-global, so nn.Modules stay picklable)."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                "libalvq.so not found at %s -- build it with `python acoustic_locating_vq-vae_amd/build.py` "
                "(there is no CPU fallback for the HIP path)" % path)
        handle = ctypes.CDLL(path)
        for name, (res, args) in _SIGNATURES.items():
            if os.environ.get("ALVQ_LIB_ALLOW_MISSING") == "1" and not hasattr(handle, name):
                continue                             # tools/ab_bits.py against an OLDER build of the library
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = handle
    return _LIB


def version():
    return lib().alvq_version().decode()


def set_option(name, value):
    """Dispatch option of the library (include/alvq.h: alvq_set_option); returns the previous value."""
    prev = get_option(name)
    _check(lib().alvq_set_option(name.encode(), int(value)), "alvq_set_option")
    return prev


def get_option(name):
    v = lib().alvq_get_option(name.encode())
    if v == -(1 << 63):
        raise KeyError(name)
    return v


def _check(rc, name):
    if rc != 0:
        raise RuntimeError("%s failed (rc=%d): %s" % (name, rc, lib().alvq_last_error().decode()))


def _ptr(t, dtype=torch.float32, name="tensor"):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (got %s); the HIP path has no CPU fallback" % (name, t.device))
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional HIP-event timing of individual launches (bench.py's live roofline measurement).

    Events are recorded on the stream the kernels are launched on (torch's current stream).  Usage:
    ``with KernelTimer() as kt: ...``; then ``kt.summary()`` -> {family: (launches, seconds, flops)}.
    """
    active = None

    def __init__(self):
        self.records = []

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for family, flops, e0, e1 in self.records:
            n, t, f = out.get(family, (0, 0.0, 0.0))
            out[family] = (n + 1, t + e0.elapsed_time(e1) * 1e-3, f + flops)
        return out


class _timed:
    __slots__ = ("family", "flops", "e0")

    def __init__(self, family, flops):
        self.family, self.flops = family, flops

    def __enter__(self):
        if KernelTimer.active is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        kt = KernelTimer.active
        if kt is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            kt.records.append((self.family, self.flops, self.e0, e1))


# ----------------------------------------------------------------------------------------------- conv
def conv1d(x, w, bias=None, skip1=None, skip2=None, mask=None, post=None, relu=False, w_layout=W_OIK,
           want_y2=False):
    """Fused conv (see alvq_conv1d_f32).  x (B,C,L); w (M,C,KW) for W_OIK or (C,M,KW) for W_IOK.
    Returns y or (y, y2)."""
    B, C, L = x.shape
    if w_layout == W_OIK:
        M, Cw, KW = w.shape
    else:
        Cw, M, KW = w.shape
    if Cw != C:
        raise RuntimeError("conv1d: weight expects %d input channels, x has %d" % (Cw, C))
    y = torch.empty((B, M, L), device=x.device, dtype=torch.float32)
    y2 = torch.empty_like(y) if post is not None else None
    for t, nm in ((skip1, "skip1"), (skip2, "skip2"), (mask, "mask"), (post, "post")):
        if t is not None and tuple(t.shape) != (B, M, L):
            raise RuntimeError("conv1d: %s has shape %s, expected %s" % (nm, tuple(t.shape), (B, M, L)))
    if bias is not None and bias.numel() != M:
        raise RuntimeError("conv1d: bias has %d elements, expected %d" % (bias.numel(), M))
    with _timed("conv1d_f32_kernel", 2.0 * B * L * M * C * KW):
        rc = lib().alvq_conv1d_f32(_ptr(x, name="x"), _ptr(w, name="w"), _ptr(bias, name="bias"), _ptr(skip1, name="skip1"),
                                   _ptr(skip2, name="skip2"), _ptr(mask, name="mask"), _ptr(post, name="post"),
                                   _ptr(y), _ptr(y2), B, C, M, L, KW, w_layout, int(bool(relu)), _stream())
    _check(rc, "alvq_conv1d_f32")
    return (y, y2) if post is not None else y


_WS = {}
_WS_RETIRED = []


def _workspace(nbytes, device):
    """Grow-only scratch per (device, stream), caller-owned from the library's point of view.

    A buffer that has been handed out is never released: a captured hipGraph records the raw pointer of the
    scratch its launches used (weight-gradient split partials, VQ norms, codebook-gradient partials), so when a
    later, larger request outgrows the buffer the old one is parked in ``_WS_RETIRED`` instead of going back to
    the caching allocator, where a replay would scribble over whoever owns the memory next.  Keyed by stream as
    well: launches on different streams are not ordered against each other and must not share scratch."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _WS_RETIRED.append(buf)
        buf = torch.empty(max(nbytes, 1 << 20), device=device, dtype=torch.uint8)
        _WS[key] = buf
    return buf


# ---- deferred split reductions (alvq_wgrad_reduce_batch): every deferred launch needs scratch of its own until the batch
# launch at the end of the backward pass has summed it.  The arena is a bump allocator over grow-only buffers per
# (device, stream) -- reset at the start of a step, never released (a captured graph keeps the raw pointers).
WGRAD_DEFER = 2
_ARENA = {}


class ReduceDesc(ctypes.Structure):
    """struct alvq_reduce_desc (include/alvq.h)"""
    _fields_ = [("partial", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("scale", ctypes.c_void_p), ("splits", ctypes.c_int32),
                ("KW", ctypes.c_int32), ("M", ctypes.c_int32), ("C", ctypes.c_int32), ("w_layout", ctypes.c_int32),
                ("accumulate", ctypes.c_int32), ("stride", ctypes.c_int64)]


def arena_reset(device):
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    st = _ARENA.get(key)
    if st is not None:
        st["chunk"], st["off"] = 0, 0


def arena_alloc(nbytes, device):
    """256-byte aligned scratch that stays valid until the next ``arena_reset`` of this (device, stream)."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    st = _ARENA.setdefault(key, {"chunks": [], "chunk": 0, "off": 0})
    nbytes = (nbytes + 255) // 256 * 256
    while True:
        if st["chunk"] >= len(st["chunks"]):
            st["chunks"].append(torch.empty(max(nbytes, 256 << 20), device=device, dtype=torch.uint8))
            st["off"] = 0
        buf = st["chunks"][st["chunk"]]
        if st["off"] + nbytes <= buf.numel():
            ptr = buf.data_ptr() + st["off"]
            st["off"] += nbytes
            return ptr
        st["chunk"] += 1
        st["off"] = 0


class DeferredReductions(list):
    """The descriptors of a backward pass's deferred reductions, plus the tensors their raw pointers refer to that nobody
    else keeps alive until the batch launch -- the loss-scale state of a gradient chain is freed with the chain's last
    tensor, and the next chain's state would be allocated (and written) at the same address before the reduction ran."""

    def __init__(self):
        super().__init__()
        self.keep = []


def wgrad_reduce_batch(descs):
    """descs: list of ReduceDesc -- one launch sums them all (dst (+)= scale * sum_s partial[s], split order)."""
    if not descs:
        return
    arr = (ReduceDesc * len(descs))(*descs)
    _check(lib().alvq_wgrad_reduce_batch(ctypes.addressof(arr), len(descs), _stream()), "alvq_wgrad_reduce_batch")
    if isinstance(descs, DeferredReductions):
        descs.keep.clear()       # the launch is queued: stream order protects the memory from here on


def _defer_descs(defer, ws_ptr, dw, dbias, scale, nseg, B, C, M, L, KW, w_layout):
    """``scale``: the 4-float loss-scale state of the gradient chain (its 1/S is read by the reduction), or None."""
    L_ = lib()
    scale_ptr = _sptr(scale, 1)
    # the batch launch sums its descriptors in concurrent workgroups: two descriptors accumulating into ONE destination
    # (a shared residual weight used by more than four layers, i.e. outside the fused multi-segment launch) would race on
    # ``dst += sum``.  Sum what is pending first -- stream order then serialises the two accumulations, as the
    # per-launch reductions did (round-3 advisor finding).
    dsts = {dw.data_ptr()} | ({dbias.data_ptr()} if dbias is not None else set())
    if any(d.dst in dsts for d in defer):
        wgrad_reduce_batch(defer)
        del defer[:]
    if scale is not None and hasattr(defer, "keep"):
        defer.keep.append(scale)
    splits = L_.alvq_conv1d_wgrad_bf16_splits(B, C, M, L, KW, nseg, int(dbias is not None))
    defer.append(ReduceDesc(ws_ptr, dw.data_ptr(), scale_ptr, splits, KW, M, C, w_layout, 1, KW * M * C))
    if dbias is not None:
        off = L_.alvq_conv1d_wgrad_bf16_bias_offset(B, C, M, L, KW)
        defer.append(ReduceDesc(ws_ptr + off, dbias.data_ptr(), scale_ptr, splits, 1, 1, M, W_OIK, 1, (M + 63) // 64 * 64))


def conv1d_wgrad(dy, x, KW, w_layout=W_OIK, want_bias=False, dw_out=None, dbias_out=None, accumulate=False):
    """dw (and dbias) of the conv whose input was x (B,C,L) and output-grad is dy (B,M,L)."""
    B, C, L = x.shape
    Bd, M, Ld = dy.shape
    if (Bd, Ld) != (B, L):
        raise RuntimeError("conv1d_wgrad: dy %s does not match x %s" % (tuple(dy.shape), tuple(x.shape)))
    shape = (M, C, KW) if w_layout == W_OIK else (C, M, KW)
    if dw_out is None:
        dw_out = torch.empty(shape, device=x.device, dtype=torch.float32)
        accumulate = False
    elif tuple(dw_out.shape) != shape:
        raise RuntimeError("conv1d_wgrad: dw_out has shape %s, expected %s" % (tuple(dw_out.shape), shape))
    if want_bias and dbias_out is None:
        dbias_out = torch.empty((M,), device=x.device, dtype=torch.float32)
    nbytes = lib().alvq_conv1d_wgrad_workspace_bytes(B, C, M, L, KW)
    if nbytes < 0:
        raise RuntimeError("conv1d_wgrad: unsupported shape")
    ws = _workspace(nbytes, x.device)
    with _timed("conv1d_wgrad_f32_kernel", 2.0 * B * L * M * C * KW):
        rc = lib().alvq_conv1d_wgrad_f32(_ptr(dy, name="dy"), _ptr(x, name="x"), _ptr(dw_out, name="dw"),
                                         _ptr(dbias_out, name="dbias") if want_bias else None, ws.data_ptr(),
                                         B, C, M, L, KW, w_layout, int(bool(accumulate)), _stream())
    _check(rc, "alvq_conv1d_wgrad_f32")
    return (dw_out, dbias_out) if want_bias else dw_out


# ----------------------------------------------------------------------------------------------- VQ
def vq_argmin(flat, codebook, want_dist=False):
    N, D = flat.shape
    K, Dc = codebook.shape
    if D != Dc:
        raise RuntimeError("vq_argmin: row width %d != codebook dim %d" % (D, Dc))
    idx = torch.empty((N,), device=flat.device, dtype=torch.int64)
    dist = torch.empty((N,), device=flat.device, dtype=torch.float32) if want_dist else None
    ws = _workspace(lib().alvq_vq_argmin_workspace_bytes(N, K, D), flat.device)
    with _timed("vq_argmin_f32_kernel", 2.0 * N * K * D):
        rc = lib().alvq_vq_argmin_f32(_ptr(flat, name="x"), _ptr(codebook, name="codebook"), idx.data_ptr(),
                                      _ptr(dist), ws.data_ptr(), N, K, D, _stream())
    _check(rc, "alvq_vq_argmin_f32")
    return (idx, dist) if want_dist else idx


def vq_gather_loss(flat, codebook, idx, beta, ema=False):
    """-> (q_st (N,D), out[2] = (loss, perplexity)).  ``ema``: the loss is beta * m alone (VectorQuantizerEMA)."""
    N, D = flat.shape
    K = codebook.shape[0]
    q_st = torch.empty_like(flat)
    partials = torch.empty((VQ_PARTIALS,), device=flat.device, dtype=torch.float32)
    hist = torch.empty((K,), device=flat.device, dtype=torch.float32)
    fill_(hist, 0.0)                                 # the library's own fill (bit pattern 0 == int 0): no ATen op on the step path
    hist = hist.view(torch.int32)
    out = torch.empty((2,), device=flat.device, dtype=torch.float32)
    L = lib()
    _check(L.alvq_vq_gather_loss_f32(_ptr(flat, name="x"), _ptr(codebook, name="codebook"),
                                     _ptr(idx, torch.int64, "idx"), _ptr(q_st), _ptr(partials),
                                     _ptr(hist, torch.int32), N, K, D, _stream()), "alvq_vq_gather_loss_f32")
    fin = "alvq_vq_finalize_ema_f32" if ema else "alvq_vq_finalize_f32"
    _check(getattr(L, fin)(_ptr(partials), _ptr(hist, torch.int32), _ptr(out), N, K, D, float(beta), _stream()), fin)
    return q_st, out


def vq_ema_stats(flat, idx, counts, sums):
    """Per-code statistics of one step into the caller's buffers (alvq_vq_ema_stats_f32): counts (K,) fp32 = rows per code,
    sums (K, D) fp32 = their sum (fp64 in row order, rounded once)."""
    N, D = flat.shape
    K = counts.numel()
    if idx.shape != (N,) or sums.shape != (K, D):
        raise RuntimeError("vq_ema_stats: idx must be (%d,) and sums (%d, %d)" % (N, K, D))
    nbytes = lib().alvq_vq_ema_stats_workspace_bytes(N, K, D)
    if nbytes < 0:
        raise RuntimeError("vq_ema_stats: N=%d, K=%d, D=%d out of range (N < 2^24, K <= 16384, D <= 512)" % (N, K, D))
    ws = _workspace(nbytes, flat.device)
    _check(lib().alvq_vq_ema_stats_f32(_ptr(flat, name="x"), _ptr(idx, torch.int64, "idx"), _ptr(counts, name="counts"),
                                       _ptr(sums, name="sums"), ws.data_ptr(), N, K, D, _stream()), "alvq_vq_ema_stats_f32")


def vq_ema_update(counts, sums, cluster_size, ema_w, codebook, decay, epsilon, skip=None):
    """The EMA update of steps 1-5 (alvq_vq_ema_update_f32), in place; ``skip``: the Trainer's skip slot (non-zero: no write)."""
    K, D = codebook.shape
    if counts.numel() != K or cluster_size.numel() != K or sums.shape != (K, D) or ema_w.shape != (K, D):
        raise RuntimeError("vq_ema_update: counts / cluster_size must be (%d,) and sums / ema_w (%d, %d)" % (K, K, D))
    _check(lib().alvq_vq_ema_update_f32(_ptr(counts, name="counts"), _ptr(sums, name="sums"),
                                        _ptr(cluster_size, name="cluster_size"), _ptr(ema_w, name="ema_w"),
                                        _ptr(codebook, name="codebook"), _ptr(skip, name="skip"), K, D, float(decay),
                                        float(epsilon), _stream()), "alvq_vq_ema_update_f32")


def vq_restart_gather(flat, rows, cand, status, first=0, stride=1):
    """cand[s] = flat[rows[s // stride]] for the slots s % stride == first (alvq_vq_restart_gather_f32); the other slots are
    left as they are.  ``status``: device int32[1]; bit 1 is raised by a position outside [0, N) (its slot is zeroed)."""
    N, D = flat.shape
    R = cand.shape[0]
    if cand.shape != (R, D) or status.numel() != 1:
        raise RuntimeError("vq_restart_gather: cand must be (R, %d) and status one int32" % D)
    if not 0 <= first < stride or rows.numel() < len(range(first, R, stride)):
        raise RuntimeError("vq_restart_gather: first=%d, stride=%d need 0 <= first < stride and %d positions (got %d)"
                           % (first, stride, len(range(first, R, stride)), rows.numel()))
    _check(lib().alvq_vq_restart_gather_f32(_ptr(flat, name="x"), _ptr(rows, torch.int64, "rows"), _ptr(cand, name="cand"),
                                            _ptr(status, torch.int32, "status"), N, D, R, int(first), int(stride), _stream()),
           "alvq_vq_restart_gather_f32")


def vq_restart_dead(cand, cluster_size, ema_w, codebook, counters, threshold, skip=None):
    """Move the first R = cand.shape[0] codes whose cluster size is below ``threshold`` onto the candidate rows, in place
    (alvq_vq_restart_dead_f32); ``counters``: device int64[2] = (restarts so far, dead codes of this step); ``skip``: the
    Trainer's skip slot (non-zero: nothing is written, the counters included)."""
    K, D = codebook.shape
    R = cand.shape[0]
    if cluster_size.numel() != K or ema_w.shape != (K, D) or cand.shape != (R, D) or counters.numel() != 2:
        raise RuntimeError("vq_restart_dead: cluster_size must be (%d,), ema_w (%d, %d), cand (R, %d) and counters int64[2]"
                           % (K, K, D, D))
    _check(lib().alvq_vq_restart_dead_f32(_ptr(cand, name="cand"), _ptr(cluster_size, name="cluster_size"),
                                          _ptr(ema_w, name="ema_w"), _ptr(codebook, name="codebook"), _ptr(skip, name="skip"),
                                          _ptr(counters, torch.int64, "counters"), K, D, R, float(threshold), _stream()),
           "alvq_vq_restart_dead_f32")


def vq_backward(g, grad_loss, flat, codebook, idx, beta, want_dx=True, want_dE=True, dE_out=None):
    """dE_out: accumulate the codebook gradient into this (K,D) tensor instead of a fresh zeroed one."""
    N, D = flat.shape
    K = codebook.shape[0]
    dx = torch.empty_like(flat) if want_dx else None
    dE = (dE_out if dE_out is not None else torch.zeros_like(codebook)) if want_dE else None
    ws = _workspace(lib().alvq_vq_backward_workspace_bytes(K, D), flat.device).data_ptr() if want_dE else None
    _check(lib().alvq_vq_backward_f32(_ptr(g, name="g"), _ptr(grad_loss, name="grad_loss"), _ptr(flat, name="x"),
                                      _ptr(codebook, name="codebook"), _ptr(idx, torch.int64, "idx"), _ptr(dx), _ptr(dE),
                                      ws, N, K, D, float(beta), _stream()), "alvq_vq_backward_f32")
    return dx, dE


def onehot(idx, K):
    N = idx.numel()
    enc = torch.empty((N, K), device=idx.device, dtype=torch.float32)
    _check(lib().alvq_onehot_f32(_ptr(idx, torch.int64, "idx"), _ptr(enc), N, K, _stream()), "alvq_onehot_f32")
    return enc


def onehot_to_index(enc):
    """(rows, K) fp32 one-hot rows -> (idx int32 [rows], flag int32 [1]); flag != 0 iff some row is not exactly one-hot."""
    rows, K = enc.shape
    idx = torch.empty((rows,), device=enc.device, dtype=torch.int32)
    flag = torch.empty((1,), device=enc.device, dtype=torch.float32)
    fill_(flag, 0.0)                                 # bit pattern 0 == int 0
    flag = flag.view(torch.int32)
    _check(lib().alvq_onehot_to_index_f32(_ptr(enc, name="encodings"), idx.data_ptr(), flag.data_ptr(), rows, K, _stream()),
           "alvq_onehot_to_index_f32")
    return idx, flag


BAG_MAX_INDICES = 16384          # indices per embedding-bag launch (its 64 KB LDS table); larger batches are chunked over B


def device_flag(device):
    """A zeroed sticky int32 flag on the device (out-of-range indices, ...)."""
    flag = torch.empty((1,), device=device, dtype=torch.float32)
    fill_(flag, 0.0)                                 # bit pattern 0 == int 0
    return flag.view(torch.int32)


def indices_to_i32(idx, K, flag):
    """int64 indices -> int32 with the range check a plain cast lacks; ORs 1 into ``flag`` for any value outside [0, K)."""
    out = torch.empty(idx.shape, device=idx.device, dtype=torch.int32)
    _check(lib().alvq_indices_to_i32(_ptr(idx, torch.int64, "idx"), out.data_ptr(), flag.data_ptr(), idx.numel(), K, _stream()),
           "alvq_indices_to_i32")
    return out


def embedding_bag_fwd(W, bias, idx, L, K, flag=None):
    """out (B, M) = bias + sum_l W[:, l*K + idx[b, l]];  W (M, L*K) fp32, idx (B, L) int32.  ``flag``: sticky device int
    that receives 1 if an index lies outside [0, K) (such terms contribute nothing).  Any B: chunked over samples."""
    B = idx.shape[0]
    M = W.shape[0]
    if W.shape[1] != L * K or tuple(idx.shape) != (B, L):
        raise RuntimeError("embedding_bag_fwd: W %s / idx %s do not match L=%d, K=%d" % (tuple(W.shape), tuple(idx.shape), L, K))
    if L > BAG_MAX_INDICES:
        raise RuntimeError("embedding_bag_fwd: L = %d exceeds the %d-index table" % (L, BAG_MAX_INDICES))
    out = torch.empty((B, M), device=W.device, dtype=torch.float32)
    step = max(1, BAG_MAX_INDICES // L)
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        _check(lib().alvq_embedding_bag_fwd_f32(_ptr(W, name="W"), _ptr(bias, name="bias"), _ptr(idx[b0:b0 + nb], torch.int32, "idx"),
                                                _ptr(out[b0:b0 + nb]), nb, L, K, M, flag.data_ptr() if flag is not None else None,
                                                _stream()), "alvq_embedding_bag_fwd_f32")
    return out


def embedding_bag_bwd(dz, idx, L, K, want_bias=True, flag=None, dW_out=None, db_out=None):
    """(dW (M, L*K) dense with the touched columns filled, dbias (M,)) from dz (B, M) and idx (B, L) int32.
    ``dW_out`` / ``db_out``: accumulate into these (a zeroed gradient sink) instead of fresh tensors."""
    B, M = dz.shape
    if dW_out is not None:
        if tuple(dW_out.shape) != (M, L * K):
            raise RuntimeError("embedding_bag_bwd: dW_out has shape %s, expected %s" % (tuple(dW_out.shape), (M, L * K)))
        dW = dW_out
    else:
        dW = torch.empty((M, L * K), device=dz.device, dtype=torch.float32)
        fill_(dW, 0.0)
    db = None
    if want_bias:
        db = db_out if db_out is not None else torch.empty((M,), device=dz.device, dtype=torch.float32)
    step = max(1, BAG_MAX_INDICES // L)
    for b0 in range(0, B, step):                     # later chunks accumulate into the same dW / dbias
        nb = min(step, B - b0)
        _check(lib().alvq_embedding_bag_bwd_f32(_ptr(dz[b0:b0 + nb], name="dz"), _ptr(idx[b0:b0 + nb], torch.int32, "idx"), _ptr(dW), _ptr(db),
                                                nb, L, K, M, int(b0 > 0 or db_out is not None),
                                                flag.data_ptr() if flag is not None else None, _stream()),
               "alvq_embedding_bag_bwd_f32")
    return dW, db


# ----------------------------------------------------------------------------------------------- misc
def jitter_gather(x, src, backward=False):
    """x (B,C,L) contiguous, src int32[L] on device."""
    L = x.shape[-1]
    y = torch.empty_like(x)
    _check(lib().alvq_jitter_gather_f32(_ptr(x, name="x"), _ptr(src, torch.int32, "src"), _ptr(y), x.numel() // L, L,
                                        int(bool(backward)), _stream()), "alvq_jitter_gather_f32")
    return y


def standardise(x, take_abs=False):
    B, C, L = x.shape
    y = torch.empty_like(x)
    _check(lib().alvq_standardise_f32(_ptr(x, name="x"), _ptr(y), B, C, L, int(bool(take_abs)), _stream()),
           "alvq_standardise_f32")
    return y


def mse(a, b):
    if a.shape != b.shape:
        raise RuntimeError("mse: shapes differ %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    loss = torch.empty((1,), device=a.device, dtype=torch.float32)
    ws = torch.empty((EW_PARTIALS,), device=a.device, dtype=torch.float32)
    _check(lib().alvq_mse_f32(_ptr(a, name="a"), _ptr(b, name="b"), _ptr(loss), _ptr(ws), a.numel(), _stream()), "alvq_mse_f32")
    return loss


def mse_backward(a, b, grad_loss):
    grad = torch.empty_like(a)
    _check(lib().alvq_mse_backward_f32(_ptr(a, name="a"), _ptr(b, name="b"), _ptr(grad_loss, name="grad_loss"), _ptr(grad),
                                       a.numel(), _stream()), "alvq_mse_backward_f32")
    return grad


def fill_(t, value=0.0):
    """t[...] = value in place (fp32, contiguous, 16-byte aligned start)."""
    if t.numel():
        _check(lib().alvq_fill_f32(_ptr(t, name="t"), float(value), t.numel(), _stream()), "alvq_fill_f32")
    return t


def add(a, b):
    out = torch.empty_like(a)
    _check(lib().alvq_add_f32(_ptr(a, name="a"), _ptr(b, name="b"), _ptr(out), a.numel(), _stream()), "alvq_add_f32")
    return out


def relu_mask(dy, t):
    """t > 0 ? dy : 0."""
    out = torch.empty_like(dy)
    _check(lib().alvq_relu_mask_f32(_ptr(dy, name="dy"), _ptr(t, name="t"), _ptr(out), dy.numel(), _stream()), "alvq_relu_mask_f32")
    return out


def row_mean(x, backward_of=None):
    """mean over the last dimension, keepdim: (B, D, L) -> (B, D, 1).  ``backward_of`` = L: the adjoint, (B, D, 1) -> (B, D, L)."""
    if backward_of is None:
        B, D, L = x.shape
        y = torch.empty((B, D, 1), device=x.device, dtype=torch.float32)
        _check(lib().alvq_row_mean_f32(_ptr(x, name="x"), _ptr(y), B * D, L, _stream()), "alvq_row_mean_f32")
        return y
    B, D, _ = x.shape
    dx = torch.empty((B, D, backward_of), device=x.device, dtype=torch.float32)
    _check(lib().alvq_row_mean_backward_f32(_ptr(x, name="dy"), _ptr(dx), B * D, backward_of, _stream()), "alvq_row_mean_backward_f32")
    return dx


def transpose12(x):
    """(B,R,C) -> (B,C,R) dense."""
    B, R, C = x.shape
    y = torch.empty((B, C, R), device=x.device, dtype=torch.float32)
    _check(lib().alvq_transpose_f32(_ptr(x, name="x"), _ptr(y), B, R, C, _stream()), "alvq_transpose_f32")
    return y


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    _check(lib().alvq_adam_f32(_ptr(param, name="param"), _ptr(grad, name="grad"), _ptr(exp_avg, name="exp_avg"),
                               _ptr(exp_avg_sq, name="exp_avg_sq"), param.numel(), int(step), float(lr), float(beta1),
                               float(beta2), float(eps), float(grad_scale), _stream()), "alvq_adam_f32")


def adam_step_dev(param, grad, exp_avg, exp_avg_sq, scalars, beta1=0.9, beta2=0.999, eps=1e-8, skip=None):
    """Adam with {lr/bc1, sqrt(bc2), grad_scale} read from the first 3 floats of the device tensor ``scalars``
    (graph-replayable; ``adam_advance`` maintains them).  ``skip``: the skip slot (a device float tensor; non-zero = leave
    everything untouched), or None."""
    _check(lib().alvq_adam_dev_f32(_ptr(param, name="param"), _ptr(grad, name="grad"), _ptr(exp_avg, name="exp_avg"),
                                   _ptr(exp_avg_sq, name="exp_avg_sq"), param.numel(), _ptr(scalars, name="scalars"),
                                   float(beta1), float(beta2), float(eps), _ptr(skip, name="skip"), _stream()), "alvq_adam_dev_f32")


ADAM_SCALARS = 8     # floats of the device state: {lr/bc1, sqrt(bc2), grad_scale, step, skipped steps, grad norm, clip coef,
#                      clipped steps} -- the last three are written by ``grad_clip`` only
GRAD_CLIP_PARTIALS = 512   # workgroups of the norm's first pass; the workspace holds that many doubles plus the sum


def adam_advance(scalars, lr, beta1=0.9, beta2=0.999, grad_scale=1.0, prev_skip=None, warmup_steps=None, total_steps=None,
                 lr_min=0.0):
    """Device-side ``step += 1`` on the 8-float tensor ``scalars`` = {lr/bc1, sqrt(bc2), grad_scale, step, skipped, ...}.
    ``prev_skip``: the skip slot still holding the previous step's verdict -- a skipped step does not count.
    ``warmup_steps`` / ``total_steps`` / ``lr_min``: a schedule (include/alvq.h: alvq_adam_advance_sched_f32) -- linear warm-up
    over ``warmup_steps`` applied steps, then cosine annealing to ``lr_min`` at ``total_steps`` (None: constant after the
    warm-up).  Without them the call is the unscheduled entry point's, as before."""
    if scalars.numel() != ADAM_SCALARS:
        raise RuntimeError("adam_advance: scalars must hold %d floats" % ADAM_SCALARS)
    if warmup_steps is None and total_steps is None:
        _check(lib().alvq_adam_advance_f32(_ptr(scalars, name="scalars"), float(lr), float(beta1), float(beta2),
                                           float(grad_scale), _ptr(prev_skip, name="prev_skip"), _stream()), "alvq_adam_advance_f32")
        return
    _check(lib().alvq_adam_advance_sched_f32(_ptr(scalars, name="scalars"), float(lr), float(beta1), float(beta2),
                                             float(grad_scale), _ptr(prev_skip, name="prev_skip"), _stream(),
                                             int(warmup_steps or 0), int(total_steps or 0), float(lr_min)),
           "alvq_adam_advance_sched_f32")


def grad_clip_workspace(device):
    """A workspace for ``grad_clip``: float64, GRAD_CLIP_PARTIALS partial sums and, last, their sum."""
    nbytes = lib().alvq_grad_clip_workspace_bytes(1)
    return torch.empty(nbytes // 8, device=device, dtype=torch.float64)


def grad_clip(grad_span, scalars, max_norm, skip=None, workspace=None):
    """Global-norm clipping as an update of ``scalars`` (between ``adam_advance`` and the Adam launches): with
    norm = sqrt(sum(grad_span^2)) * scalars[2] and coef = min(1, max_norm / (norm + 1e-6)),
    scalars[5] = norm, scalars[6] = coef, scalars[2] *= coef, scalars[7] += 1 if coef < 1.  Deterministic (a fixed grid, float64
    partial sums added in index order).  ``max_norm`` = inf measures without clipping.  ``skip``: the skip slot; non-zero =
    only the norm is written.  ``workspace``: a ``grad_clip_workspace`` tensor (its last element is left holding the float64
    sum of squares); default: the stream's scratch."""
    if scalars.numel() != ADAM_SCALARS:
        raise RuntimeError("grad_clip: scalars must hold %d floats" % ADAM_SCALARS)
    n = grad_span.numel()
    if workspace is None:
        workspace = _workspace(lib().alvq_grad_clip_workspace_bytes(max(n, 1)), grad_span.device)
        ws = _ptr(workspace, torch.uint8)
    else:
        if workspace.numel() * workspace.element_size() < (GRAD_CLIP_PARTIALS + 1) * 8:
            raise RuntimeError("grad_clip: workspace too small")
        ws = _ptr(workspace, torch.float64, "workspace")
    _check(lib().alvq_grad_clip_f32(_ptr(grad_span, name="grad_span"), n, _ptr(scalars, name="scalars"), float(max_norm), ws,
                                    _ptr(skip, name="skip"), _stream()), "alvq_grad_clip_f32")


def range_flag_to_slot(slot):
    """slot[0] = 1.0 if the fp16-range flag holds a bit raised since the step's guarded ``adam_advance``, else 0.0."""
    _check(lib().alvq_range_flag_to_slot(_ptr(slot, name="slot"), _stream()), "alvq_range_flag_to_slot")


# ----------------------------------------------------------------------------------------------- signal and array wrappers
def _call(name, *args):
    """The checked call of the entry point ``name`` on the current stream (its last argument)."""
    _check(getattr(lib(), name)(*args, _stream()), name)


def _call_real(stem, real, *args):
    """``_call`` of ``alvq_<stem>_f32`` or ``alvq_<stem>_f64``, chosen by the real dtype of the call's tensors."""
    sfx = {torch.float32: "f32", torch.float64: "f64"}.get(real)
    if sfx is None:
        raise RuntimeError("alvq_%s: float32 or float64 only (got %s)" % (stem, real))
    _call("alvq_%s_%s" % (stem, sfx), *args)


def _empty(like, dtype, *shape):
    """An uninitialised output on like's device."""
    return torch.empty(shape, device=like.device, dtype=dtype)


def _scratch(nbytes, like, bad_dims, reuse=None):
    """nbytes of scratch on like's device, ``reuse`` where that is large enough.  nbytes is what a ``*_workspace_bytes``
    entry point returned: negative is its verdict on the dims, raised with the caller's ``bad_dims`` text."""
    if nbytes < 0:
        raise RuntimeError(bad_dims)
    if reuse is not None and reuse.numel() >= nbytes:
        return reuse
    return torch.empty((nbytes,), device=like.device, dtype=torch.uint8)


def _spec4_real(spec4d, who):
    """(real dtype, (B, D, F, T), the contiguous interleaved view) of a complex (B, D, F, T) spectrogram."""
    if spec4d.dim() != 4 or spec4d.dtype not in (torch.complex64, torch.complex128):
        raise RuntimeError("%s: expected a complex64 / complex128 (B, D, F, T) spectrogram (got %s %s)"
                           % (who, spec4d.dtype, tuple(spec4d.shape)))
    real = torch.float64 if spec4d.dtype == torch.complex128 else torch.float32
    return real, tuple(spec4d.shape), torch.view_as_real(spec4d.resolve_conj().contiguous())


def _c128(t, shape, who, name):
    """The contiguous interleaved view of a complex128 tensor of the given shape."""
    if t.dtype != torch.complex128 or tuple(t.shape) != tuple(shape):
        raise RuntimeError("%s: %s must be complex128 %s (got %s %s)" % (who, name, tuple(shape), t.dtype, tuple(t.shape)))
    return torch.view_as_real(t.resolve_conj().contiguous())


def _positions(who, name, t, B, n):
    """Positions (n, 3) that serve every item, or (B, n, 3) -- n a count, or a letter where any will do -> (the contiguous
    tensor, whether it holds a row per item)."""
    if t.dim() not in (2, 3) or t.shape[-1] != 3 or (t.dim() == 3 and t.shape[0] != B) or (isinstance(n, int) and t.shape[-2] != n):
        raise RuntimeError("%s: %s must be (%s, 3) or (%d, %s, 3) (got %s)" % (who, name, n, B, n, tuple(t.shape)))
    return t.contiguous(), t.dim() == 3


def stft_power(wave, n_fft=400, hop=160):
    """Power spectrogram of (B,S) waveforms, fp32 or fp64 (the reference's echoed signal is float64)."""
    B, S = wave.shape
    power = _empty(wave, wave.dtype, B, n_fft // 2 + 1, 1 + S // hop)
    _call_real("stft_power", wave.dtype, _ptr(wave, wave.dtype, "wave"), _ptr(power, wave.dtype), B, S, n_fft, hop)
    return power


def stft_complex(wave, n_fft=400, hop=160):
    """Complex STFT (B, n_fft/2+1, T) of (B,S) waveforms: complex64 for fp32 input, complex128 for fp64."""
    B, S = wave.shape
    F, T = n_fft // 2 + 1, 1 + S // hop
    out = _empty(wave, wave.dtype, B, F, T, 2)
    _call_real("stft_complex", wave.dtype, _ptr(wave, wave.dtype, "wave"), _ptr(out, wave.dtype), B, S, n_fft, hop)
    return torch.view_as_complex(out)


def fir_same(wave, h):
    """scipy.signal.convolve(wave, h, mode='same') in float64: wave (B,S) fp32, h (Nh,) or (B,Nh) fp64."""
    B, S = wave.shape
    if h.dim() == 1:
        stride, Nh = 0, h.shape[0]
    else:
        if h.shape[0] != B:
            raise RuntimeError("fir_same: %d impulse responses for %d waveforms" % (h.shape[0], B))
        stride, Nh = h.shape[1], h.shape[1]
    out = _empty(wave, torch.float64, B, S)
    _call("alvq_fir_same_f64", _ptr(wave, name="wave"), _ptr(h, torch.float64, "h"), _ptr(out, torch.float64), B, S, Nh, stride)
    return out


def spec_rir_wiener(speech_spec, echoed_spec):
    """complex64 S and complex128 E, both (B,F,T) -> (speech_pow fp32, echoed_pow fp64, rir_pow fp64, wiener (B,F) fp64)."""
    if speech_spec.dtype != torch.complex64 or echoed_spec.dtype != torch.complex128 or speech_spec.shape != echoed_spec.shape:
        raise RuntimeError("spec_rir_wiener: expected complex64 and complex128 tensors of one shape")
    B, F, T = speech_spec.shape
    sr, er = torch.view_as_real(speech_spec), torch.view_as_real(echoed_spec)
    speech_pow = _empty(speech_spec, torch.float32, B, F, T)
    echoed_pow = _empty(speech_spec, torch.float64, B, F, T)
    rir_pow = _empty(speech_spec, torch.float64, B, F, T)
    wiener = _empty(speech_spec, torch.float64, B, F)
    ws = _empty(speech_spec, torch.float64, B, F)
    _call("alvq_spec_rir_wiener_f64", _ptr(sr, name="speech_spec"), _ptr(er, torch.float64, "echoed_spec"), _ptr(speech_pow),
          _ptr(echoed_pow, torch.float64), _ptr(rir_pow, torch.float64), _ptr(wiener, torch.float64), _ptr(ws, torch.float64),
          B, F, T)
    return speech_pow, echoed_pow, rir_pow, wiener


def _spec_dims(spec, n_fft, who):
    if spec.dim() != 3 or spec.dtype not in (torch.complex64, torch.complex128):
        raise RuntimeError("%s: expected a complex64 / complex128 (B, F, T) spectrogram (got %s %s)"
                           % (who, spec.dtype, tuple(spec.shape)))
    B, F, T = spec.shape
    if F != n_fft // 2 + 1:
        raise RuntimeError("%s: %d frequency bins, n_fft=%d has %d" % (who, F, n_fft, n_fft // 2 + 1))
    return B, T, torch.float64 if spec.dtype == torch.complex128 else torch.float32


def istft(spec, n_fft=400, hop=160, length=None):
    """Inverse of ``stft_complex``: (B, n_fft/2+1, T) complex64 / complex128 -> (B, length) float32 / float64 waveforms
    (alvq_istft_*; length defaults to hop*(T-1))."""
    B, T, real = _spec_dims(spec, n_fft, "istft")
    length = hop * (T - 1) if length is None else int(length)
    sr = torch.view_as_real(spec.resolve_conj().contiguous())
    wave = _empty(spec, real, B, length)
    ws = _empty(spec, real, B, T, n_fft)
    _call_real("istft", real, _ptr(sr, real, "spec"), _ptr(wave, real), _ptr(ws, real), B, T, n_fft, hop, length)
    return wave


def griffin_lim(mag, angles, n_iter, momentum, n_fft, hop, length):
    """Griffin-Lim (alvq_griffin_lim_*): magnitude mag (B, n_fft/2+1, T) float32 / float64 normalised as ``stft_complex``,
    complex start phases angles of the matching complex dtype and shape -> (B, length) waveforms."""
    B, T, real = _spec_dims(angles, n_fft, "griffin_lim")
    if mag.shape != angles.shape or mag.dtype != real:
        raise RuntimeError("griffin_lim: mag must be %s of shape %s (got %s %s)" % (real, tuple(angles.shape), mag.dtype,
                                                                                   tuple(mag.shape)))
    ar = torch.view_as_real(angles.resolve_conj().contiguous())
    wave = _empty(mag, real, B, length)
    ws = _scratch(lib().alvq_griffin_lim_workspace_bytes(B, T, n_fft, 8 if real == torch.float64 else 4), mag,
                  "griffin_lim: bad dims (B=%d T=%d n_fft=%d)" % (B, T, n_fft))
    _call_real("griffin_lim", real, _ptr(mag, real, "mag"), _ptr(ar, real, "angles"), _ptr(wave, real), _ptr(ws, torch.uint8), B, T,
               n_fft, hop, int(length), int(n_iter), float(momentum))
    return wave


def rir(src, rcv, L, beta, c, fs, nsample, order=-1, hp_filter=True):
    """Room impulse responses (alvq_rir_f64): src, rcv (B,3) float64 positions on the GPU, room L (3 floats), six wall
    reflection coefficients beta -> (B, nsample) float64."""
    if src.dim() != 2 or src.shape[1] != 3 or rcv.shape != src.shape:
        raise RuntimeError("rir: src and rcv must both be (B, 3) (got %s and %s)" % (tuple(src.shape), tuple(rcv.shape)))
    L = [float(v) for v in L]
    beta = [float(v) for v in beta]
    if len(L) != 3 or len(beta) != 6:
        raise RuntimeError("rir: need 3 room dimensions and 6 reflection coefficients (got %d and %d)" % (len(L), len(beta)))
    B = src.shape[0]
    h = _empty(src, torch.float64, B, int(nsample))
    beta_c = (ctypes.c_double * 6)(*beta)
    _call("alvq_rir_f64", _ptr(src, torch.float64, "src"), _ptr(rcv, torch.float64, "rcv"), _ptr(h, torch.float64), B,
          int(nsample), L[0], L[1], L[2], ctypes.cast(beta_c, _c_void_p), float(c), float(fs), int(order), int(bool(hp_filter)))
    return h


def rir_rooms(src, rcv, room, beta, c, fs, nsample, order=-1, hp_filter=True):
    """Room impulse responses with a room and six reflection coefficients per item (alvq_rir_rooms_f64): src, rcv, room (B,3)
    and beta (B,6) float64 on the GPU -> (h (B, nsample) float64, status (B,) int32).  status is the kernel's per-item flag
    (0 = fine; 1 = some |beta| > 1; 2 = a bad room or an image range above 4096) and is not read here."""
    B = src.shape[0] if src.dim() == 2 else -1
    if src.dim() != 2 or src.shape[1] != 3 or rcv.shape != src.shape or room.shape != src.shape or tuple(beta.shape) != (B, 6):
        raise RuntimeError("rir_rooms: src, rcv, room must be (B, 3) and beta (B, 6) (got %s, %s, %s, %s)"
                           % (tuple(src.shape), tuple(rcv.shape), tuple(room.shape), tuple(beta.shape)))
    h = _empty(src, torch.float64, B, int(nsample))
    status = _empty(src, torch.int32, B)
    _call("alvq_rir_rooms_f64", _ptr(src, torch.float64, "src"), _ptr(rcv, torch.float64, "rcv"),
          _ptr(room, torch.float64, "room"), _ptr(beta, torch.float64, "beta"), _ptr(h, torch.float64),
          _ptr(status, torch.int32, "status"), B, int(nsample), float(c), float(fs), int(order), int(bool(hp_filter)))
    return h, status


def _responses(h, who):
    if h.dim() != 2 or h.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("%s: h must be a float32 or float64 (B, n) tensor (got %s %s)" % (who, h.dtype, tuple(h.shape)))
    return h.shape[0], h.shape[1]


def edc(h):
    """Energy decay curves (alvq_edc_f32 / _f64): h (B, n) float32 or float64 on the GPU -> (B, n) float64 dB."""
    B, n = _responses(h, "edc")
    out = _empty(h, torch.float64, B, n)
    _call_real("edc", h.dtype, _ptr(h, h.dtype, "h"), _ptr(out, torch.float64), B, n)
    return out


def room_acoustics(h, fs, k50, k80, kdirect):
    """Room-acoustic parameters (alvq_room_acoustics_f32 / _f64): h (B, n) float32 or float64 on the GPU -> (out (B, 7)
    float64 with columns t30 t20 edt c50 c80 d50 drr, onset (B,) int32, status (B,) int32).  status is the kernel's per-row
    flag (include/alvq.h) and is not read here."""
    B, n = _responses(h, "room_acoustics")
    out = _empty(h, torch.float64, B, 7)
    onset, status = _empty(h, torch.int32, B), _empty(h, torch.int32, B)
    _call_real("room_acoustics", h.dtype, _ptr(h, h.dtype, "h"), _ptr(out, torch.float64), _ptr(onset, torch.int32),
               _ptr(status, torch.int32), B, n, float(fs), int(k50), int(k80), int(kdirect))
    return out, onset, status


# ----------------------------------------------------------------------------------------------- speech measures
def _row_pair(a, b, who):
    if a.dim() != 2 or a.dtype not in (torch.float32, torch.float64) or b.shape != a.shape or b.dtype != a.dtype:
        raise RuntimeError("%s: expected two float32 or two float64 (B, n) tensors of one shape (got %s %s and %s %s)"
                           % (who, a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
    return a.shape[0], a.shape[1]


def resample_poly(x, h, up, down):
    """Rational resampling (alvq_resample_poly_f32 / _f64): x (B, n) float32 or float64 on the GPU, h the (2 half + 1) float64
    taps on the GPU, up and down coprime -> (B, ceil(n up / down)) float64."""
    B, n = _responses(x, "resample_poly")
    if h.dim() != 1 or h.shape[0] % 2 != 1:
        raise RuntimeError("resample_poly: h must hold an odd number of taps (got %s)" % (tuple(h.shape),))
    y = _empty(x, torch.float64, B, -(-n * up // down))
    _call_real("resample_poly", x.dtype, _ptr(x, x.dtype, "x"), _ptr(h, torch.float64, "h"), _ptr(y, torch.float64), B, n, int(up),
               int(down), h.shape[0] // 2)
    return y


def stoi(clean, degraded, band_lo, band_hi):
    """STOI at 10 kHz (alvq_stoi_f64): clean, degraded (B, n) float64 on the GPU, band_lo / band_hi 15 DFT bins each ->
    (value (B,) float64, kept_frames (B,) int32, status (B,) int32).  status is the kernel's per-row flag (include/alvq.h) and
    is not read here."""
    B, n = _row_pair(clean, degraded, "stoi")
    if len(band_lo) != 15 or len(band_hi) != 15:
        raise RuntimeError("stoi: need 15 band edges each (got %d and %d)" % (len(band_lo), len(band_hi)))
    ws = _scratch(lib().alvq_stoi_workspace_bytes(B, n), clean,
                  "stoi: bad dims (B=%d n=%d; need 1 <= B <= 65535, 2 <= n <= 2^24)" % (B, n))
    value, kept, status = _empty(clean, torch.float64, B), _empty(clean, torch.int32, B), _empty(clean, torch.int32, B)
    lo_c, hi_c = (ctypes.c_int * 15)(*[int(v) for v in band_lo]), (ctypes.c_int * 15)(*[int(v) for v in band_hi])
    _call("alvq_stoi_f64", _ptr(clean, torch.float64, "clean"), _ptr(degraded, torch.float64, "degraded"),
          ctypes.cast(lo_c, _c_void_p), ctypes.cast(hi_c, _c_void_p), _ptr(value, torch.float64), _ptr(kept, torch.int32),
          _ptr(status, torch.int32), _ptr(ws, torch.uint8), B, n)
    return value, kept, status


def si_sdr(reference, estimate):
    """Scale-invariant SDR (alvq_si_sdr_f32 / _f64): two (B, n) tensors of one real dtype on the GPU -> (B,) float64 dB."""
    B, n = _row_pair(reference, estimate, "si_sdr")
    out = _empty(reference, torch.float64, B)
    _call_real("si_sdr", reference.dtype, _ptr(reference, reference.dtype, "reference"), _ptr(estimate, reference.dtype, "estimate"),
               _ptr(out, torch.float64), B, n)
    return out


def lsd(p, q, eps):
    """Log-spectral distance (alvq_lsd_f32 / _f64): power spectrograms p, q (B, F, T) of one real dtype on the GPU -> (B,)
    float64 dB."""
    if p.dim() != 3 or p.dtype not in (torch.float32, torch.float64) or q.shape != p.shape or q.dtype != p.dtype:
        raise RuntimeError("lsd: expected two float32 or two float64 (B, F, T) tensors of one shape (got %s %s and %s %s)"
                           % (p.dtype, tuple(p.shape), q.dtype, tuple(q.shape)))
    B, F, T = p.shape
    out = _empty(p, torch.float64, B)
    _call_real("lsd", p.dtype, _ptr(p, p.dtype, "p"), _ptr(q, p.dtype, "q"), _ptr(out, torch.float64), B, F, T, float(eps))
    return out


# ----------------------------------------------------------------------------------------------- separation scores
def _source_rows(references, estimates, who):
    if references.dim() != 3 or estimates.dim() != 3 or references.dtype not in (torch.float32, torch.float64) \
            or estimates.dtype != references.dtype or estimates.shape[0] != references.shape[0] \
            or estimates.shape[2] != references.shape[2]:
        raise RuntimeError("%s: expected float32 or float64 (B, K, n) references and (B, J, n) estimates of one dtype (got %s %s "
                           "and %s %s)" % (who, references.dtype, tuple(references.shape), estimates.dtype, tuple(estimates.shape)))
    return references.shape[0], references.shape[1], estimates.shape[1], references.shape[2]


def pairwise_si_sdr(references, estimates):
    """The SI-SDR of every pair (alvq_pairwise_si_sdr_f32 / _f64): references (B, K, n) and estimates (B, J, n) of one real
    dtype on the GPU -> (B, K, J) float64 dB."""
    B, K, J, n = _source_rows(references, estimates, "pairwise_si_sdr")
    table = _empty(references, torch.float64, B, K, J)
    _call_real("pairwise_si_sdr", references.dtype, _ptr(references, references.dtype, "references"),
               _ptr(estimates, references.dtype, "estimates"), _ptr(table, torch.float64), B, K, J, n)
    return table


def assign(table, maximize):
    """The best assignment of columns to rows (alvq_assign_f64): table (B, K, J) float64 on the GPU, K <= J -> (perm (B, K)
    int32, total (B,) float64, status (B,) int32).  status is the kernel's per-item flag (include/alvq.h) and is not read
    here."""
    if table.dim() != 3 or table.dtype != torch.float64:
        raise RuntimeError("assign: expected a float64 (B, K, J) table (got %s %s)" % (table.dtype, tuple(table.shape)))
    B, K, J = table.shape
    perm = _empty(table, torch.int32, B, K)
    total = _empty(table, torch.float64, B)
    status = _empty(table, torch.int32, B)
    _call("alvq_assign_f64", _ptr(table, torch.float64, "table"), _ptr(perm, torch.int32), _ptr(total, torch.float64),
          _ptr(status, torch.int32), B, K, J, 1 if maximize else 0)
    return perm, total, status


def si_bss_eval(references, estimates, perm):
    """Scale-invariant SDR, SIR and SAR (alvq_si_bss_eval_f32 / _f64): references (B, K, n), estimates (B, J, n) of one real
    dtype and perm (B, K) int32 on the GPU -> (sdr, sir, sar (B, K) float64, status (B,) int32)."""
    B, K, J, n = _source_rows(references, estimates, "si_bss_eval")
    if perm.dtype != torch.int32 or tuple(perm.shape) != (B, K):
        raise RuntimeError("si_bss_eval: expected an int32 (%d, %d) perm (got %s %s)" % (B, K, perm.dtype, tuple(perm.shape)))
    sdr, sir, sar = (_empty(references, torch.float64, B, K) for _ in range(3))
    status = _empty(references, torch.int32, B)
    _call_real("si_bss_eval", references.dtype, _ptr(references, references.dtype, "references"),
               _ptr(estimates, references.dtype, "estimates"), _ptr(perm, torch.int32, "perm"), _ptr(sdr, torch.float64),
               _ptr(sir, torch.float64), _ptr(sar, torch.float64), _ptr(status, torch.int32), B, K, J, n)
    return sdr, sir, sar, status


# ----------------------------------------------------------------------------------------------- dereverberation
def wpe(spec4d, taps, delay, iterations, psd_context, eps, loading):
    """WPE dereverberation (alvq_wpe_f32 / _f64): spec4d (B, D, F, T) complex64 / complex128 on the GPU -> (out of the same
    shape and dtype, status (B, F) int32).  status is the kernel's per-bin flag (include/alvq.h) and is not read here."""
    real, (B, D, F, T), xr = _spec4_real(spec4d, "wpe")
    nbytes = lib().alvq_wpe_workspace_bytes(B, D, F, T, int(taps))
    ws = _scratch(nbytes, spec4d, "wpe: bad dims (B=%d D=%d F=%d T=%d taps=%d; need 1 <= B <= 65535, 1 <= D <= 8, D taps <= 64, "
                  "1 <= T <= 65535)" % (B, D, F, T, taps))
    out = torch.empty_like(xr)
    status = _empty(spec4d, torch.int32, B, F)
    _call_real("wpe", real, _ptr(xr, real, "spec"), _ptr(out, real), _ptr(status, torch.int32),
               _ptr(ws if nbytes else None, torch.uint8), B, D, F, T, int(taps), int(delay), int(iterations), int(psd_context),
               float(eps), float(loading))
    return torch.view_as_complex(out), status


# ----------------------------------------------------------------------------------------------- source localisation
def phat_cross_spectra(spec4d, f_lo, f_hi):
    """PHAT-weighted cross-spectra of the microphone pairs (alvq_phat_cross_spectra_f32 / _f64): spec4d (B, D, F, T) complex64 /
    complex128 on the GPU -> (psi (B, D (D - 1) / 2, F) complex128, 0 outside the bins f_lo .. f_hi; status (B,) int32).
    status is the kernel's per-item flag (include/alvq.h) and is not read here."""
    real, (B, D, F, T), xr = _spec4_real(spec4d, "phat_cross_spectra")
    psi = _empty(spec4d, torch.float64, B, D * (D - 1) // 2, F, 2)
    status = _empty(spec4d, torch.int32, B)
    _call_real("phat_cross_spectra", real, _ptr(xr, real, "spec"), _ptr(psi, torch.float64), _ptr(status, torch.int32), B, D, F, T,
               int(f_lo), int(f_hi))
    return torch.view_as_complex(psi), status


def _psi_dims(psi, n_fft, who):
    if psi.dim() != 3 or psi.dtype != torch.complex128 or psi.shape[2] != n_fft // 2 + 1:
        raise RuntimeError("%s: expected complex128 (B, P, n_fft / 2 + 1) cross-spectra (got %s %s, n_fft=%d)"
                           % (who, psi.dtype, tuple(psi.shape), n_fft))
    B, P, F = psi.shape
    D = next((d for d in range(2, 9) if d * (d - 1) // 2 == P), None)
    if D is None:
        raise RuntimeError("%s: %d pairs are not those of 2 .. 8 microphones" % (who, P))
    return B, D, torch.view_as_real(psi.resolve_conj().contiguous())


def gcc_phat(psi, n_fft, max_lag, f_lo, f_hi):
    """GCC-PHAT at the integer lags -max_lag .. max_lag (alvq_gcc_phat_f64): psi (B, P, F) complex128 on the GPU ->
    (B, P, 2 max_lag + 1) float64."""
    B, D, pr = _psi_dims(psi, int(n_fft), "gcc_phat")
    r = _empty(psi, torch.float64, B, psi.shape[1], 2 * int(max_lag) + 1)
    _call("alvq_gcc_phat_f64", _ptr(pr, torch.float64, "psi"), _ptr(r, torch.float64), B, D, int(n_fft), int(max_lag),
          int(f_lo), int(f_hi))
    return r


def srp_phat(psi, mics, cand, fs, n_fft, c, f_lo, f_hi):
    """The SRP-PHAT map (alvq_srp_phat_f64): psi (B, P, F) complex128, microphones mics (D, 3) or (B, D, 3) and candidates
    cand (G, 3) or (B, G, 3), float64, all on the GPU -> (map (B, G) float64, best (B,) int32, status (B,) int32).  A
    two-dimensional mics / cand serves every item.  status is the kernel's per-item flag (include/alvq.h) and is not read here."""
    B, D, pr = _psi_dims(psi, int(n_fft), "srp_phat")
    mics, mics_per_item = _positions("srp_phat", "mics", mics, B, D)
    cand, cand_per_item = _positions("srp_phat", "cand", cand, B, "G")
    G = cand.shape[-2]
    out, best, status = _empty(psi, torch.float64, B, G), _empty(psi, torch.int32, B), _empty(psi, torch.int32, B)
    _call("alvq_srp_phat_f64", _ptr(pr, torch.float64, "psi"), _ptr(mics, torch.float64, "mics"),
          _ptr(cand, torch.float64, "cand"), _ptr(out, torch.float64), _ptr(best, torch.int32), _ptr(status, torch.int32), B, D,
          G, 3 * D if mics_per_item else 0, 3 * G if cand_per_item else 0, float(fs), int(n_fft), float(c), int(f_lo), int(f_hi))
    return out, best, status


# ----------------------------------------------------------------------------------------------- beamforming
def spatial_covariance(spec4d, mask=None):
    """Mask-weighted spatial covariances (alvq_spatial_covariance_f32 / _f64): spec4d (B, D, F, T) complex64 / complex128 and
    mask (B, F, T) float64 or None on the GPU -> (Phi (B, F, D, D) complex128, status (B, F) int32).  status is the kernel's
    per-bin flag (include/alvq.h) and is not read here."""
    real, (B, D, F, T), xr = _spec4_real(spec4d, "spatial_covariance")
    if mask is not None:
        if mask.dtype != torch.float64 or tuple(mask.shape) != (B, F, T):
            raise RuntimeError("spatial_covariance: mask must be float64 (%d, %d, %d) (got %s %s)"
                               % (B, F, T, mask.dtype, tuple(mask.shape)))
        mask = mask.contiguous()
    phi = _empty(spec4d, torch.float64, B, F, D, D, 2)
    status = _empty(spec4d, torch.int32, B, F)
    _call_real("spatial_covariance", real, _ptr(xr, real, "spec"), _ptr(mask, torch.float64, "mask"), _ptr(phi, torch.float64),
               _ptr(status, torch.int32), B, D, F, T)
    return torch.view_as_complex(phi), status


def steering_vectors(mics, src, F, fs, n_fft, c, ref):
    """Steering vectors (alvq_steering_vectors_f64): microphones mics (D, 3) or (B, D, 3) and positions src (B, 3), float64 on
    the GPU -> (A (B, D, F) complex128, status (B,) int32).  A two-dimensional mics serves every item."""
    if src.dim() != 2 or src.shape[1] != 3:
        raise RuntimeError("steering_vectors: src must be (B, 3) (got %s)" % (tuple(src.shape),))
    B = src.shape[0]
    mics, per_item = _positions("steering_vectors", "mics", mics, B, "D")
    src, D = src.contiguous(), mics.shape[-2]
    A = _empty(src, torch.float64, B, D, int(F), 2)
    status = _empty(src, torch.int32, B)
    _call("alvq_steering_vectors_f64", _ptr(mics, torch.float64, "mics"), _ptr(src, torch.float64, "src"),
          _ptr(A, torch.float64), _ptr(status, torch.int32), B, D, int(F), float(fs), int(n_fft), float(c), int(ref),
          int(per_item))
    return torch.view_as_complex(A), status


BEAMFORM_DAS, BEAMFORM_MVDR, BEAMFORM_SOUDEN = 0, 1, 2


def beamform_weights(mode, B, D, F, phi_n=None, phi_s=None, steering=None, ref=0, loading=0.0):
    """Beamformer weights (alvq_beamform_weights_f64): mode BEAMFORM_DAS (steering), BEAMFORM_MVDR (phi_n, steering) or
    BEAMFORM_SOUDEN (phi_n, phi_s); phi_* (B, F, D, D) and steering (B, D, F), complex128 on the GPU -> (W (B, F, D)
    complex128, status (B, F) int32).  What a mode does not read is not passed on."""
    who = "beamform_weights"
    need = {BEAMFORM_DAS: (False, False, True), BEAMFORM_MVDR: (True, False, True), BEAMFORM_SOUDEN: (True, True, False)}.get(mode)
    if need is None:
        raise RuntimeError("%s: mode must be 0, 1 or 2 (got %r)" % (who, mode))
    given = ((phi_n, (B, F, D, D), "phi_n"), (phi_s, (B, F, D, D), "phi_s"), (steering, (B, D, F), "steering"))
    views = []
    for wanted, (t, shape, name) in zip(need, given):
        if wanted and t is None:
            raise RuntimeError("%s: mode %d needs %s" % (who, mode, name))
        views.append(_c128(t, shape, who, name) if wanted else None)
    first = next(v for v in views if v is not None)
    W, status = _empty(first, torch.float64, B, F, D, 2), _empty(first, torch.int32, B, F)
    _call("alvq_beamform_weights_f64", _ptr(views[0], torch.float64, "phi_n"), _ptr(views[1], torch.float64, "phi_s"),
          _ptr(views[2], torch.float64, "steering"), _ptr(W, torch.float64), _ptr(status, torch.int32), B, D, F, int(mode),
          int(ref), float(loading))
    return torch.view_as_complex(W), status


def beamform_apply(spec4d, w):
    """y = w^H x (alvq_beamform_apply_f32 / _f64): spec4d (B, D, F, T) complex64 / complex128 and w (B, F, D) complex128 on the
    GPU -> (B, F, T) of spec4d's dtype."""
    real, (B, D, F, T), xr = _spec4_real(spec4d, "beamform_apply")
    wr = _c128(w, (B, F, D), "beamform_apply", "w")
    out = _empty(spec4d, real, B, F, T, 2)
    _call_real("beamform_apply", real, _ptr(xr, real, "spec"), _ptr(wr, torch.float64, "w"), _ptr(out, real), B, D, F, T)
    return torch.view_as_complex(out)


def beamform_gev(phi_n, phi_s, ref=0, loading=0.0):
    """GEV weights and the covariance-whitening steering estimate (alvq_beamform_gev_f64): phi_n, phi_s (B, F, D, D) complex128
    on the GPU -> (W (B, F, D) complex128, RTF (B, F, D) complex128, gain (B, F) float64, status (B, F) int32)."""
    who = "beamform_gev"
    if phi_n.dim() != 4 or phi_n.shape[-1] != phi_n.shape[-2]:
        raise RuntimeError("%s: phi_n must be (B, F, D, D) (got %s)" % (who, tuple(phi_n.shape)))
    B, F, D, _ = phi_n.shape
    pn, ps = _c128(phi_n, (B, F, D, D), who, "phi_n"), _c128(phi_s, (B, F, D, D), who, "phi_s")
    W, rtf = _empty(phi_n, torch.float64, B, F, D, 2), _empty(phi_n, torch.float64, B, F, D, 2)
    gain, status = _empty(phi_n, torch.float64, B, F), _empty(phi_n, torch.int32, B, F)
    _call("alvq_beamform_gev_f64", _ptr(pn, torch.float64, "phi_n"), _ptr(ps, torch.float64, "phi_s"), _ptr(W, torch.float64),
          _ptr(rtf, torch.float64), _ptr(gain, torch.float64), _ptr(status, torch.int32), B, D, F, int(ref), float(loading))
    return torch.view_as_complex(W), torch.view_as_complex(rtf), gain, status


# ----------------------------------------------------------------------------------------------- source separation
IVA_LAPLACE, IVA_GAUSS = 0, 1


def auxiva(spec4d, iterations, model, ref, eps, w0=None):
    """AuxIVA (alvq_auxiva_f32 / _f64): spec4d (B, D, F, T) complex64 / complex128 and w0 (B, F, D, D) complex128 or None on the
    GPU -> (Y of spec4d's shape and dtype, W (B, F, D, D) complex128, status (B, F) int32).  status is the kernels' per-bin
    flag (include/alvq.h) and is not read here."""
    real, (B, D, F, T), xr = _spec4_real(spec4d, "auxiva")
    ws = _scratch(lib().alvq_auxiva_workspace_bytes(B, D, F, T), spec4d,
                  "auxiva: bad dims (B=%d D=%d F=%d T=%d; need 1 <= B <= 65535, B F <= 2^31 - 1, 1 <= D <= 8, 1 <= T <= 65535)"
                  % (B, D, F, T))
    w0r = None if w0 is None else _c128(w0, (B, F, D, D), "auxiva", "w0")
    out = torch.empty_like(xr)
    W, status = _empty(spec4d, torch.float64, B, F, D, D, 2), _empty(spec4d, torch.int32, B, F)
    _call_real("auxiva", real, _ptr(xr, real, "spec"), _ptr(w0r, torch.float64, "w0"), _ptr(W, torch.float64), _ptr(out, real),
               _ptr(status, torch.int32), _ptr(ws, torch.uint8), B, D, F, T, int(model), int(iterations), int(ref), float(eps))
    return torch.view_as_complex(out), torch.view_as_complex(W), status


def ilrma(spec4d, basis0, activations0, iterations, ref, floor, w0=None):
    """ILRMA (alvq_ilrma_f32 / _f64): spec4d (B, D, F, T) complex64 / complex128, basis0 (B, D, F, L) and activations0
    (B, D, L, T) float64 and w0 (B, F, D, D) complex128 or None on the GPU -> (Y of spec4d's shape and dtype, W (B, F, D, D)
    complex128, basis, activations, status (B, F) int32).  status is the kernels' per-bin flag (include/alvq.h) and is not
    read here."""
    real, (B, D, F, T), xr = _spec4_real(spec4d, "ilrma")
    if basis0.dim() != 4 or basis0.dtype != torch.float64 or tuple(basis0.shape[:3]) != (B, D, F):
        raise RuntimeError("ilrma: basis0 must be float64 (%d, %d, %d, L) (got %s %s)" % (B, D, F, basis0.dtype, tuple(basis0.shape)))
    L = basis0.shape[3]
    if activations0.dtype != torch.float64 or tuple(activations0.shape) != (B, D, L, T):
        raise RuntimeError("ilrma: activations0 must be float64 (%d, %d, %d, %d) (got %s %s)"
                           % (B, D, L, T, activations0.dtype, tuple(activations0.shape)))
    ws = _scratch(lib().alvq_ilrma_workspace_bytes(B, D, L, F, T), spec4d,
                  "ilrma: bad dims (B=%d D=%d L=%d F=%d T=%d; need 1 <= B <= 65535, B F <= 2^31 - 1, 1 <= D <= 8, 1 <= L <= 16, "
                  "1 <= T <= 65535)" % (B, D, L, F, T))
    w0r = None if w0 is None else _c128(w0, (B, F, D, D), "ilrma", "w0")
    b0, a0 = basis0.contiguous(), activations0.contiguous()
    out = torch.empty_like(xr)
    W, status = _empty(spec4d, torch.float64, B, F, D, D, 2), _empty(spec4d, torch.int32, B, F)
    basis, activations = torch.empty_like(b0), torch.empty_like(a0)
    _call_real("ilrma", real, _ptr(xr, real, "spec"), _ptr(w0r, torch.float64, "w0"), _ptr(b0, torch.float64, "basis0"),
               _ptr(a0, torch.float64, "activations0"), _ptr(W, torch.float64), _ptr(basis, torch.float64),
               _ptr(activations, torch.float64), _ptr(out, real), _ptr(status, torch.int32), _ptr(ws, torch.uint8),
               B, D, L, F, T, int(iterations), int(ref), float(floor))
    return torch.view_as_complex(out), torch.view_as_complex(W), basis, activations, status


def separation_masks(spec4d):
    """Ratio masks (alvq_separation_masks_f32 / _f64): spec4d (B, K, F, T) complex64 / complex128 on the GPU -> (B, K, F, T)
    float64."""
    real, (B, K, F, T), yr = _spec4_real(spec4d, "separation_masks")
    M = _empty(spec4d, torch.float64, B, K, F, T)
    _call_real("separation_masks", real, _ptr(yr, real, "spec"), _ptr(M, torch.float64), B, K, F, T)
    return M


def cacgmm(spec4d, init, iterations, floor, quadratic0=None):
    """cACGMM mask estimation (alvq_cacgmm_f32 / _f64): spec4d (B, D, F, T) complex64 / complex128, init and quadratic0 (or
    None) (B, K, F, T) float64 on the GPU -> (masks (B, K, F, T), prior (B, K, T), cov (B, F, K, D, D) complex128, quadratic
    (B, K, F, T), status (B, F) int32).  status is the kernels' per-bin flag (include/alvq.h) and is not read here."""
    real, (B, D, F, T), xr = _spec4_real(spec4d, "cacgmm")
    if init.dim() != 4 or init.dtype != torch.float64 or tuple(init.shape) != (B, init.shape[1], F, T):
        raise RuntimeError("cacgmm: init must be float64 (%d, K, %d, %d) (got %s %s)" % (B, F, T, init.dtype, tuple(init.shape)))
    K = init.shape[1]
    if quadratic0 is not None and (quadratic0.dtype != torch.float64 or quadratic0.shape != init.shape):
        raise RuntimeError("cacgmm: quadratic0 must be float64 %s (got %s %s)" % (tuple(init.shape), quadratic0.dtype,
                                                                                 tuple(quadratic0.shape)))
    ws = _scratch(lib().alvq_cacgmm_workspace_bytes(B, D, K, F, T), spec4d,
                  "cacgmm: bad dims (B=%d D=%d K=%d F=%d T=%d; need 1 <= B <= 65535, B F <= 2^31 - 1, 2 <= D <= 8, 1 <= K <= 8, "
                  "1 <= T <= 65535)" % (B, D, K, F, T))
    masks, quadratic = _empty(spec4d, torch.float64, B, K, F, T), _empty(spec4d, torch.float64, B, K, F, T)
    prior, cov = _empty(spec4d, torch.float64, B, K, T), _empty(spec4d, torch.float64, B, F, K, D, D, 2)
    status = _empty(spec4d, torch.int32, B, F)
    g0, q0 = init.contiguous(), None if quadratic0 is None else quadratic0.contiguous()
    _call_real("cacgmm", real, _ptr(xr, real, "spec"), _ptr(g0, torch.float64, "init"),
               _ptr(q0, torch.float64, "quadratic0"), _ptr(masks, torch.float64), _ptr(prior, torch.float64),
               _ptr(cov, torch.float64), _ptr(quadratic, torch.float64), _ptr(status, torch.int32), _ptr(ws, torch.uint8),
               B, D, K, F, T, int(iterations), float(floor))
    return masks, prior, torch.view_as_complex(cov), quadratic, status


def align_permutations(profile, iterations, perm0=None):
    """Frequency permutation alignment (alvq_align_permutations_f64): profile (B, K, F, T) float64 and perm0 None or (B, F, K)
    int32 on the GPU -> (perm (B, F, K) int32, score (B, F) float64, changed (B,) int32, status (B, F) int32).  status is the
    kernels' per-bin flag (include/alvq.h) and is not read here."""
    if profile.dim() != 4 or profile.dtype != torch.float64:
        raise RuntimeError("align_permutations: profile must be float64 (B, K, F, T) (got %s %s)" % (profile.dtype, tuple(profile.shape)))
    B, K, F, T = profile.shape
    if perm0 is not None and (perm0.dtype != torch.int32 or tuple(perm0.shape) != (B, F, K)):
        raise RuntimeError("align_permutations: perm0 must be int32 %s (got %s %s)" % ((B, F, K), perm0.dtype, tuple(perm0.shape)))
    ws = _scratch(lib().alvq_align_workspace_bytes(B, K, F, T), profile,
                  "align_permutations: bad dims (B=%d K=%d F=%d T=%d; need 1 <= B <= 65535, B F <= 2^31 - 1, 1 <= K <= 8, "
                  "2 <= T <= 65535)" % (B, K, F, T))
    p, p0 = profile.contiguous(), None if perm0 is None else perm0.contiguous()
    perm, score = _empty(profile, torch.int32, B, F, K), _empty(profile, torch.float64, B, F)
    changed, status = _empty(profile, torch.int32, B), _empty(profile, torch.int32, B, F)
    _call("alvq_align_permutations_f64", _ptr(p, torch.float64, "profile"), _ptr(p0, torch.int32, "perm0"),
          _ptr(perm, torch.int32), _ptr(score, torch.float64), _ptr(changed, torch.int32), _ptr(status, torch.int32),
          _ptr(ws, torch.uint8), B, K, F, T, int(iterations))
    return perm, score, changed, status


def permute_bins(x, perm):
    """out[b, k, f, t] = x[b, perm[b, f, k], f, t] (alvq_permute_bins): x (B, K, F, T) float32, float64, complex64 or complex128
    and perm (B, F, K) int32 on the GPU -> a new tensor of x's shape and dtype."""
    if x.dim() != 4 or x.dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128):
        raise RuntimeError("permute_bins: x must be a real or complex (B, K, F, T) tensor of 4, 8 or 16 byte elements (got %s %s)"
                           % (x.dtype, tuple(x.shape)))
    B, K, F, T = x.shape
    if perm.dtype != torch.int32 or tuple(perm.shape) != (B, F, K):
        raise RuntimeError("permute_bins: perm must be int32 %s (got %s %s)" % ((B, F, K), perm.dtype, tuple(perm.shape)))
    xc, pc = x.resolve_conj().contiguous(), perm.contiguous()
    out = torch.empty_like(xc)
    _call("alvq_permute_bins", _ptr(xc, x.dtype, "x"), _ptr(pc, torch.int32, "perm"), _ptr(out, x.dtype), B, K, F, T,
          x.element_size())
    return out


# ----------------------------------------------------------------------------------------------- subspace methods
def eigh(cov):
    """Hermitian eigendecomposition (alvq_eigh_f64): cov (n, D, D) complex128 on the GPU, 1 <= D <= 8 -> (values (n, D) float64
    ascending, vectors (n, D, D) complex128, status (n,) int32).  status is the kernel's per-matrix flag (include/alvq.h) and
    is not read here."""
    if cov.dim() != 3 or cov.shape[1] != cov.shape[2]:
        raise RuntimeError("eigh: cov must be (n, D, D) (got %s)" % (tuple(cov.shape),))
    n, D, _ = cov.shape
    ar = _c128(cov, (n, D, D), "eigh", "cov")
    lam, V, status = _empty(cov, torch.float64, n, D), _empty(cov, torch.float64, n, D, D, 2), _empty(cov, torch.int32, n)
    _call("alvq_eigh_f64", _ptr(ar, torch.float64, "cov"), _ptr(lam, torch.float64), _ptr(V, torch.float64),
          _ptr(status, torch.int32), n, D)
    return lam, torch.view_as_complex(V), status


def music(vectors, values, mics, cand, n_sources, fs, n_fft, c, f_lo, f_hi):
    """The MUSIC null spectrum (alvq_music_f64): vectors (B, F, D, D) complex128 and values (B, F, D) float64 as ``eigh``
    returns them, microphones mics (D, 3) or (B, D, 3) and candidates cand (G, 3) or (B, G, 3), float64, all on the GPU ->
    (null (B, G) float64, best (B,) int32, status (B,) int32).  A two-dimensional mics / cand serves every item."""
    if vectors.dim() != 4 or vectors.shape[-1] != vectors.shape[-2]:
        raise RuntimeError("music: vectors must be (B, F, D, D) (got %s)" % (tuple(vectors.shape),))
    B, F, D, _ = vectors.shape
    vr = _c128(vectors, (B, F, D, D), "music", "vectors")
    if values.dtype != torch.float64 or tuple(values.shape) != (B, F, D):
        raise RuntimeError("music: values must be float64 %s (got %s %s)" % ((B, F, D), values.dtype, tuple(values.shape)))
    mics, mics_per_item = _positions("music", "mics", mics, B, D)
    cand, cand_per_item = _positions("music", "cand", cand, B, "G")
    values, G = values.contiguous(), cand.shape[-2]
    out, best, status = _empty(vectors, torch.float64, B, G), _empty(vectors, torch.int32, B), _empty(vectors, torch.int32, B)
    _call("alvq_music_f64", _ptr(vr, torch.float64, "vectors"), _ptr(values, torch.float64, "values"),
          _ptr(mics, torch.float64, "mics"), _ptr(cand, torch.float64, "cand"), _ptr(out, torch.float64),
          _ptr(best, torch.int32), _ptr(status, torch.int32), B, D, F, G, int(n_sources), float(fs), int(n_fft), float(c),
          int(f_lo), int(f_hi), int(mics_per_item), int(cand_per_item))
    return out, best, status


# ----------------------------------------------------------------------------------------------- t-SNE
def tsne_code_sqdist(codes):
    """int32 (N, L) code sequences -> (N, N) fp32 squared distances of their one-hot expansions (alvq_tsne_code_sqdist_f32)."""
    if codes.dim() != 2:
        raise RuntimeError("tsne_code_sqdist: codes must be (N, L) (got %s)" % (tuple(codes.shape),))
    N, L = codes.shape
    d2 = _empty(codes, torch.float32, N, N)
    _call("alvq_tsne_code_sqdist_f32", _ptr(codes, torch.int32, "codes"), _ptr(d2), N, L)
    return d2


def tsne_affinities(P, perplexity):
    """In place: (N, N) fp32 distances -> the joint affinities (alvq_tsne_affinities_f32).  Returns (beta, S), (N,) fp64 each."""
    N = P.shape[0]
    if P.dim() != 2 or P.shape[1] != N:
        raise RuntimeError("tsne_affinities: P must be (N, N) (got %s)" % (tuple(P.shape),))
    ws = _scratch(lib().alvq_tsne_affinities_workspace_bytes(N), P, "tsne_affinities: N=%d out of range" % N)
    beta, S = _empty(P, torch.float64, N), _empty(P, torch.float64, N)
    _call("alvq_tsne_affinities_f32", _ptr(P, name="P"), _ptr(beta, torch.float64), _ptr(S, torch.float64),
          _ptr(ws, torch.uint8), N, float(perplexity))
    return beta, S


def tsne_descend(P, Y, update, gains, grad, stats, n_iter, exaggeration, momentum, learning_rate, workspace=None):
    """n_iter iterations of one t-SNE descent phase (alvq_tsne_descend_f64): Y, update, gains (N, 2) fp64 in place; grad (N, 2)
    and stats (2,) fp64 out (the last iteration's gained gradient, and its KL and gradient norm)."""
    N = Y.shape[0]
    for name, t in (("Y", Y), ("update", update), ("gains", gains), ("grad", grad)):
        if t.shape != (N, 2):
            raise RuntimeError("tsne_descend: %s must be (%d, 2) (got %s)" % (name, N, tuple(t.shape)))
    if P.shape != (N, N) or stats.numel() < 2:
        raise RuntimeError("tsne_descend: P must be (%d, %d) and stats hold 2 values" % (N, N))
    workspace = _scratch(lib().alvq_tsne_descend_workspace_bytes(N), Y, "tsne_descend: N=%d out of range" % N, workspace)
    f64 = torch.float64
    _call("alvq_tsne_descend_f64", _ptr(P, name="P"), _ptr(Y, f64, "Y"), _ptr(update, f64, "update"), _ptr(gains, f64, "gains"),
          _ptr(grad, f64, "grad"), _ptr(stats, f64, "stats"), _ptr(workspace, torch.uint8, "workspace"), N, int(n_iter),
          float(exaggeration), float(momentum), float(learning_rate))
    return workspace


# ----------------------------------------------------------------------------------------------- bf16 path
# KernelTimer names follow rocprofv3's kernel names -- function plus its leading template arguments -- so that bench.py's
# per-kernel figures can be laid beside `rocprofv3 --kernel-trace --stats` line by line: conv1d_f16mx_kernel<OUT, KW, ...>,
# conv1d_bf16x3_kernel<OUT, KW, ...>, conv1d_bf16_k3_kernel<OUT, F16>, conv1d_bf16_v2_kernel<OUT, F16>,
# conv1d_bf16_kernel<KW, OUT, F16> (OUT: 0 = NLC output, 1 = fp32 NCL; F16: the fp16 opcodes of the bf16 kernels).  The "..."
# of the f16mx name stands for <DBG, NIN, MIN, EPI>: rocprofv3 prints e.g. conv1d_f16mx_kernel<0, 3, 0, 2, 4, 2> for the
# bias-alone epilogue (EPI = 1 / 2 / 3: no operand / bias / skip1, 0 the general one), all under the one <OUT, KW, ...> name here.
def _conv16_name(f16, out, KW, M, rows):
    """Mirrors the dispatch in csrc/conv1d_bf16.hip: wide layers go to the 256x256-tile kernels (k3 for width 3)."""
    min_tiles = get_option("wide_min_tiles")
    if ((M + 255) // 256 * 256 - M) <= 32 and (rows // 256) * ((M + 255) // 256) >= min_tiles:
        return ("conv1d_bf16_k3_kernel<%d, %d>" if KW == 3 else "conv1d_bf16_v2_kernel<%d, %d>") % (out, f16)
    return "conv1d_bf16_kernel<%d, %d, %d>" % (KW, out, f16)


def _wgrad16_name(KW, with_bias, f16):
    """rocprofv3's name of the 16-bit weight-gradient kernel a launch gets (mirrors csrc/conv1d_wgrad_bf16_v2.hip: the v3
    kernels serve the launches without a bias gradient, option wgrad_v3)."""
    sel = get_option("wgrad_v3")
    if not with_bias and ((KW == 1 and sel & 1) or (KW == 3 and sel & 2)):
        return "conv1d_wgrad_bf16_v3_kernel<%s, %d>" % ("3, 1, 2" if KW == 3 else "1, 2, 4", f16)
    return "conv1d_wgrad_bf16_v2_kernel<%s, %d>" % ("3, 2" if KW == 3 else "1, 4", f16)


# One row per activation format: everything the functions below need to know about it.
#   planes       planes of an activation (the second one at +alvq_nlc_plane_bytes)
#   bits         the buffer ends in rows*Cp/8 bytes for the sign bits a ReLU'd convolution can leave behind; the forward
#                conv then takes (mask_bits, bits_out)
#   scaled       fp16 range: gradients carry a loss scale (NLC.gscale); every launch then takes one more pointer to S or 1/S
#   defer        the weight gradient may leave its split reduction to wgrad_reduce_batch
#   wcode/wreads packed-weight code the format packs to (alvq_pack_weights_bf16_batch) / the codes a launch may read: an f16
#                launch reads the H image of an f16mx weight, a bf16 launch may read the hi image of a bf16x3 one
#   operands     formats whose tensors serve as an operand: an f16 launch reads an f16mx tensor through its H plane, a bf16
#                launch a bf16x3 tensor through its hi plane (the backward of the _hb modes)
#   rows_code    format code of alvq_rows_to_nlc, None where it does not serve the format
#   relu_flat    the ReLU mask takes a flat element count (else B, C, L); pack: None = only the batched launch packs it
#   *_family     KernelTimer family of a launch (bench.py keys its roofline on them)
_Format = collections.namedtuple("_Format", (
    "name", "planes", "bits", "scaled", "defer", "wcode", "wreads", "operands", "rows_code", "to_nlc", "to_ncl", "relu",
    "relu_flat", "pack", "conv", "wgrad", "wgrad_multi", "wgrad_ws", "conv_family", "wgrad_family"))
_FORMATS = {f.name: f for f in (
    _Format("bf16", planes=1, bits=True, scaled=False, defer=True, wcode=1, wreads=(1, 2), operands=("bf16", "bf16x3"),
            rows_code=1, to_nlc="alvq_ncl_to_nlc_bf16", to_ncl="alvq_nlc_to_ncl_f32", relu="alvq_relu_mask_bf16",
            relu_flat=True, pack="alvq_pack_weight_bf16", conv="alvq_conv1d_bf16", wgrad="alvq_conv1d_wgrad_bf16",
            wgrad_multi="alvq_conv1d_wgrad_bf16_multi", wgrad_ws="alvq_conv1d_wgrad_bf16_workspace_bytes",
            conv_family=functools.partial(_conv16_name, 0),
            wgrad_family=lambda KW, with_bias: _wgrad16_name(KW, with_bias, 0)),
    _Format("bf16x3", planes=2, bits=False, scaled=False, defer=False, wcode=2, wreads=(2,), operands=("bf16x3",),
            rows_code=2, to_nlc="alvq_ncl_to_nlc_bf16x3", to_ncl="alvq_nlc_to_ncl_bf16x3", relu="alvq_relu_mask_bf16x3",
            relu_flat=False, pack="alvq_pack_weight_bf16x3", conv="alvq_conv1d_bf16x3", wgrad="alvq_conv1d_wgrad_bf16x3",
            wgrad_multi="alvq_conv1d_wgrad_bf16x3_multi", wgrad_ws="alvq_conv1d_wgrad_bf16x3_workspace_bytes",
            conv_family=lambda out, KW, M, rows: "conv1d_bf16x3_kernel<%d, %d, ...>" % (out, KW),
            wgrad_family=lambda KW, with_bias: "conv1d_wgrad_bf16x3_kernel"),
    _Format("f16mx", planes=2, bits=True, scaled=True, defer=False, wcode=3, wreads=(3,), operands=("f16mx",),
            rows_code=3, to_nlc="alvq_ncl_to_nlc_f16mx", to_ncl="alvq_nlc_to_ncl_f16mx", relu="alvq_relu_mask_f16mx",
            relu_flat=False, pack=None, conv="alvq_conv1d_f16mx", wgrad="alvq_conv1d_wgrad_f16mx",
            wgrad_multi="alvq_conv1d_wgrad_f16mx_multi", wgrad_ws="alvq_conv1d_wgrad_f16mx_workspace_bytes",
            conv_family=lambda out, KW, M, rows: "conv1d_f16mx_kernel<%d, %d, ...>" % (out, KW),
            wgrad_family=lambda KW, with_bias: "conv1d_wgrad_f16mx_kernel"),
    # one fp16 plane: the bf16 kernels with fp16 opcodes (their ReLU mask tests the sign of a 16-bit pattern, whichever type)
    _Format("f16", planes=1, bits=True, scaled=True, defer=True, wcode=3, wreads=(3,), operands=("f16", "f16mx"),
            rows_code=None, to_nlc="alvq_ncl_to_nlc_f16", to_ncl="alvq_nlc_to_ncl_f16", relu="alvq_relu_mask_bf16",
            relu_flat=True, pack=None, conv="alvq_conv1d_f16", wgrad="alvq_conv1d_wgrad_f16",
            wgrad_multi="alvq_conv1d_wgrad_f16_multi", wgrad_ws="alvq_conv1d_wgrad_bf16_workspace_bytes",
            conv_family=functools.partial(_conv16_name, 1),
            wgrad_family=lambda KW, with_bias: _wgrad16_name(KW, with_bias, 1)))}
_PACKERS = {f.wcode: f.pack for f in _FORMATS.values()}      # by weight code: what pack_weight launches


def _format(planes, fmt):
    """The door: the (planes, fmt) pair of the public signatures -> the row.  Without a name the plane count picks the bf16 family."""
    f = _FORMATS[fmt or ("bf16x3" if planes == 2 else "bf16")]
    if f.planes != planes:
        raise ValueError("format %s has %d plane(s), not %d" % (f.name, f.planes, planes))
    return f


class NLC:
    """An activation in the NLC-padded layout (see include/alvq.h): storage = guard rows + matrix + guard rows.

    ``fmt``: "bf16" (one plane), "bf16x3" (hi + lo bf16 planes), "f16mx" (fp16 H plane + fp8 Q plane; same bytes and
    geometry as bf16x3) or "f16" (one fp16 plane: the gradients of the f16mx_hb mode) -- a row of ``_FORMATS``.
    ``has_bits``: the sign bits behind the planes are valid.  ``gscale``: for a gradient in the f16mx / f16 formats, the
    4-float device state of its loss scale ({S, 1/S, ...}, alvq_grad_scale_f32) -- inherited by everything computed from it
    and divided out where the chain leaves the format; None for forward tensors."""
    __slots__ = ("storage", "B", "L", "C", "Cp", "rows", "guard", "planes", "has_bits", "fmt", "gscale")

    def _shape(self, B, L, C, planes, fmt):
        """Sets the geometry; returns (format row, elements of a buffer of it, the sign-bit tail included)."""
        f = _format(planes, fmt)
        L_ = lib()
        self.B, self.L, self.C, self.planes, self.fmt = B, L, C, f.planes, f.name
        self.Cp, self.rows, self.guard = L_.alvq_nlc_channels(C), L_.alvq_nlc_rows(B, L), L_.alvq_nlc_guard_rows()
        return f, f.planes * (self.rows + 2 * self.guard) * self.Cp + (self.rows * self.Cp // 16 if f.bits else 0)

    def __init__(self, B, L, C, device, planes=1, fmt=None, gscale=None):
        _, n = self._shape(B, L, C, planes, fmt)
        self.gscale, self.has_bits = gscale, False
        self.storage = torch.empty((n,), device=device, dtype=torch.bfloat16)

    @classmethod
    def wrap(cls, storage, B, L, C, planes=1, has_bits=False, fmt=None):
        self = cls.__new__(cls)
        f, n = self._shape(B, L, C, planes, fmt)
        self.gscale, self.storage = None, storage
        self.has_bits = bool(has_bits) and f.bits and storage.numel() >= n
        return self

    @property
    def ptr(self):
        return self.storage.data_ptr() + self.guard * self.Cp * 2

    @property
    def bits_ptr(self):
        """Sign-bit area behind the plane(s)."""
        return self.storage.data_ptr() + self.planes * (self.rows + 2 * self.guard) * self.Cp * 2

    def matrix(self, plane=0):
        g = (self.guard + plane * (self.rows + 2 * self.guard)) * self.Cp
        return self.storage[g:g + self.rows * self.Cp].view(self.rows, self.Cp)

    def to_ncl(self):
        """(B,C,L) fp32 copy -- test/debug helper (torch indexing, not on the hot path)."""
        if self.fmt in ("f16mx", "f16"):
            return nlc_to_ncl(self)
        m = self.matrix(0).float()
        if self.planes == 2:
            m = m + self.matrix(1).float()
        m = m[1:1 + self.B * (self.L + 1)].view(self.B, self.L + 1, self.Cp)
        return m[:, :self.L, :self.C].permute(0, 2, 1).contiguous()


def nlc_like(ref, C):
    return NLC(ref.B, ref.L, C, ref.storage.device, ref.planes, ref.fmt, ref.gscale)


def _sptr(gscale, which):
    """Device pointer to S (which = 0) or 1/S (which = 1) of a loss-scale state, or None."""
    return None if gscale is None else gscale.data_ptr() + 4 * which


def grad_scale(x):
    """Loss scale of a backward chain in the f16mx format: 4-float device state {S, 1/S, -, -} with S the power of two
    that puts amax|x| in [2^7, 2^8) -- chosen on the device, no host round trip (graph-capturable)."""
    state = torch.empty((4,), device=x.device, dtype=torch.float32)
    fill_(state, 0.0)
    _check(lib().alvq_grad_scale_f32(_ptr(x, name="x"), x.numel(), state.data_ptr(), _stream()), "alvq_grad_scale_f32")
    return state


def f16mx_range_flag(reset=True, device="cuda"):
    """Sticky range flag of the f16mx / fp16 formats on the current device (one host sync): bit 0 = a value >= 65504 in
    magnitude entered the format (it was stored saturated), bit 1 = a NaN did, bit 2 = a convolution PRODUCED such a value
    (an activation, or a scaled gradient that outgrew its headroom).  The formats carry fp16's range: standardised
    spectrograms and Kaiming-scale weights stay orders of magnitude below; gradients are brought into range by the
    device-chosen loss scale.  0 = nothing saturated since the last reset."""
    out = device_flag(torch.device(device))
    _check(lib().alvq_f16mx_range_flag(out.data_ptr(), int(bool(reset)), _stream()), "alvq_f16mx_range_flag")
    return int(out.item())


def _fmt_serves(t, ref):
    """Can ``t`` be read as an operand of ``ref``'s format?"""
    return t.fmt in _FORMATS[ref.fmt].operands


def _nlc_ptr(t, ref, C, name):
    if t is None:
        return None
    if not isinstance(t, NLC) or (t.B, t.L, t.C) != (ref.B, ref.L, C) or not _fmt_serves(t, ref):
        raise RuntimeError("%s: expected an NLC activation of (B=%d, L=%d, C=%d, %s)" % (name, ref.B, ref.L, C, ref.fmt))
    return t.ptr


def ncl_to_nlc(x, planes=1, fmt=None, gscale=None):
    """(B,C,L) fp32 dense -> NLC (planes=2: split hi/lo; fmt="f16mx": fp16 + fp8 planes; the loss-scaled formats multiply
    by the S of ``gscale`` when given)."""
    B, C, L = x.shape
    out = NLC(B, L, C, x.device, planes, fmt, gscale)
    f = _FORMATS[out.fmt]
    _check(getattr(lib(), f.to_nlc)(_ptr(x, name="x"), out.ptr, B, C, L, *((_sptr(gscale, 0),) if f.scaled else ()), _stream()),
           f.to_nlc)
    return out


def rows_to_nlc_supported(fmt, L, standardise=False):
    return _FORMATS[fmt].rows_code is not None and (not standardise or 2 <= L <= lib().alvq_rows_to_nlc_max_std_rows())


def rows_to_nlc(x_blc, planes=1, fmt=None, standardise=False, take_abs=False):
    """(B, L, C) fp32 contiguous -- the model input (B, C, L) seen through ``permute(0, 2, 1)`` -- straight into the NLC
    layout (channels are already contiguous: no transposition either way), optionally standardised over L per (b, c) in the
    same pass (train_rir.py:43-44; bit-identical to standardise -> transpose -> ncl_to_nlc)."""
    B, L, C = x_blc.shape
    out = NLC(B, L, C, x_blc.device, planes, fmt)
    if not rows_to_nlc_supported(out.fmt, L, standardise):
        raise RuntimeError("rows_to_nlc: format %s / L = %d not supported" % (out.fmt, L))
    _check(lib().alvq_rows_to_nlc(_ptr(x_blc, name="x"), out.ptr, B, C, L, _FORMATS[out.fmt].rows_code, int(bool(standardise)),
                                  int(bool(take_abs)), _stream()), "alvq_rows_to_nlc")
    return out


def nlc_to_ncl(a):
    """NLC -> (B,C,L) fp32 dense (a loss-scaled gradient: divided by its S)."""
    f = _FORMATS[a.fmt]
    y = torch.empty((a.B, a.C, a.L), device=a.storage.device, dtype=torch.float32)
    _check(getattr(lib(), f.to_ncl)(a.ptr, _ptr(y), a.B, a.C, a.L, *((_sptr(a.gscale, 1),) if f.scaled else ()), _stream()),
           f.to_ncl)
    return y


def pack_weight(w, w_layout, planes=1):
    """fp32 weight (M,C,KW) [OIK] or (C,M,KW) [IOK] -> packed bf16 image(s) + (M, C, KW, planes).  ``planes``: the weight
    code of the format that will read it (``wcode`` in _FORMATS)."""
    wp, tag = packed_weight_alloc(w, w_layout, planes)
    symbol = _PACKERS[planes]
    if symbol is None:
        pack_weights_batch([(w, wp, w_layout)], planes)
    else:
        M, C, KW, _ = tag
        _check(getattr(lib(), symbol)(_ptr(w, name="w"), wp.data_ptr(), M, C, KW, w_layout, _stream()), symbol)
    return wp, tag


class PackDesc(ctypes.Structure):
    """struct alvq_pack_desc (include/alvq.h)"""
    _fields_ = [("w", ctypes.c_void_p), ("wp", ctypes.c_void_p), ("M", ctypes.c_int32), ("C", ctypes.c_int32),
                ("KW", ctypes.c_int32), ("w_layout", ctypes.c_int32)]


def packed_weight_alloc(w, w_layout, planes=1):
    """Uninitialised packed image(s) for ``w`` + the (M, C, KW, planes) tag ``pack_weight`` returns."""
    if w_layout == W_OIK:
        M, C, KW = w.shape
    else:
        C, M, KW = w.shape
    n = lib().alvq_packed_weight_elems(M, C, KW)
    return torch.empty((min(planes, 2) * n,), device=w.device, dtype=torch.bfloat16), (M, C, KW, planes)


def pack_weights_batch(entries, planes=1):
    """entries: [(w fp32 cuda tensor, packed image from packed_weight_alloc, w_layout)] -- one launch for all."""
    if not entries:
        return
    arr = (PackDesc * len(entries))()
    for d, (w, wp, w_layout) in zip(arr, entries):
        if w_layout == W_OIK:
            M, C, KW = w.shape
        else:
            C, M, KW = w.shape
        need = min(planes, 2) * lib().alvq_packed_weight_elems(M, C, KW)
        if wp.numel() != need or wp.dtype != torch.bfloat16:
            raise RuntimeError("pack_weights_batch: packed image has %d elements, expected %d" % (wp.numel(), need))
        d.w, d.wp, d.M, d.C, d.KW, d.w_layout = _ptr(w, name="w"), wp.data_ptr(), M, C, KW, w_layout
    _check(lib().alvq_pack_weights_bf16_batch(ctypes.addressof(arr), len(entries), planes, _stream()),
           "alvq_pack_weights_bf16_batch")


class AdamPackDesc(ctypes.Structure):
    """struct alvq_adam_pack_desc (include/alvq.h)"""
    _fields_ = [("w", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("wp_oik", ctypes.c_void_p), ("wp_iok", ctypes.c_void_p), ("dim0", ctypes.c_int32), ("dim1", ctypes.c_int32),
                ("KW", ctypes.c_int32)]


def adam_pack_batch(entries, planes, scalars, beta1=0.9, beta2=0.999, eps=1e-8, skip=None):
    """entries: [(w, g, m, v fp32 views of one conv weight and its Adam state, packed OIK image or None, packed IOK image or
    None)] -- Adam's update and the re-pack of every image in one launch."""
    if not entries:
        return
    arr = (AdamPackDesc * len(entries))()
    for d, (w, g, m, v, oik, iok) in zip(arr, entries):
        d.w, d.g, d.m, d.v = _ptr(w, name="w"), _ptr(g, name="g"), _ptr(m, name="m"), _ptr(v, name="v")
        d.wp_oik = oik.data_ptr() if oik is not None else None
        d.wp_iok = iok.data_ptr() if iok is not None else None
        d.dim0, d.dim1, d.KW = w.shape
    _check(lib().alvq_adam_pack_batch(ctypes.addressof(arr), len(entries), planes, _ptr(scalars, name="scalars"), float(beta1),
                                      float(beta2), float(eps), _ptr(skip, name="skip"), _stream()), "alvq_adam_pack_batch")


def adam_segments(param, grad, exp_avg, exp_avg_sq, segments, scalars, beta1=0.9, beta2=0.999, eps=1e-8, skip=None):
    """Adam over the element ranges [(lo, hi), ...] of the flat buffers, one launch."""
    segments = [(int(a), int(b)) for a, b in segments if b > a]
    if not segments:
        return
    lo = (ctypes.c_int64 * len(segments))(*[a for a, _ in segments])
    hi = (ctypes.c_int64 * len(segments))(*[b for _, b in segments])
    _check(lib().alvq_adam_segments_f32(_ptr(param, name="param"), _ptr(grad, name="grad"), _ptr(exp_avg, name="exp_avg"),
                                        _ptr(exp_avg_sq, name="exp_avg_sq"), lo, hi, len(segments), _ptr(scalars, name="scalars"),
                                        float(beta1), float(beta2), float(eps), _ptr(skip, name="skip"), _stream()),
           "alvq_adam_segments_f32")


def relu_mask_bf16(dy, t):
    f = _FORMATS[dy.fmt]
    out = nlc_like(dy, dy.C)
    dims = (dy.rows * dy.Cp,) if f.relu_flat else (dy.B, dy.C, dy.L)
    _check(getattr(lib(), f.relu)(dy.ptr, _nlc_ptr(t, dy, dy.C, "t"), out.ptr, *dims, _stream()), f.relu)
    return out


USE_SIGN_BITS = os.environ.get("ALVQ_SIGN_BITS", "1") != "0"


def conv1d_bf16(x, packed, bias=None, skip1=None, skip2=None, mask=None, post=None, relu=False, out_ncl=False):
    """x: NLC; packed = pack_weight(...).  Returns NLC y, (y, y2) with post, or a (B,M,L) fp32 tensor if out_ncl."""
    f = _FORMATS[x.fmt]
    wp, (M, C, KW, wcode) = packed
    if C != x.C:
        raise RuntimeError("conv1d_bf16: weight expects %d input channels, x has %d" % (C, x.C))
    if wcode not in f.wreads:
        raise RuntimeError("conv1d_bf16: weight packed for format %d, activation is %s" % (wcode, x.fmt))
    if bias is not None and bias.numel() != M:
        raise RuntimeError("conv1d_bf16: bias has %d elements, expected %d" % (bias.numel(), M))
    y = y2 = y_ncl = None
    if out_ncl:
        y_ncl = torch.empty((x.B, M, x.L), device=wp.device, dtype=torch.float32)
    else:
        y = nlc_like(x, M)
        y2 = nlc_like(x, M) if post is not None else None
    family = f.conv_family(int(bool(out_ncl)), KW, M, x.rows)
    # sign bits: a ReLU'd output records them; a mask operand that carries valid bits is passed as bits
    extra = ()
    mask_ptr = _nlc_ptr(mask, x, M, "mask")
    bits_out = f.bits and y is not None and relu and USE_SIGN_BITS
    if f.bits:
        mask_bits = None
        if mask is not None and mask.has_bits and USE_SIGN_BITS:
            mask_bits, mask_ptr = mask.bits_ptr, None
        extra = (mask_bits, y.bits_ptr if bits_out else None)
    if f.scaled:
        extra += (_sptr(x.gscale, 1) if out_ncl else None,)     # a gradient leaving the format: divide the loss scale out
    with _timed(family, 2.0 * x.B * x.L * M * C * KW):
        rc = getattr(lib(), f.conv)(x.ptr, wp.data_ptr(), _ptr(bias, name="bias"), _nlc_ptr(skip1, x, M, "skip1"),
                                    _nlc_ptr(skip2, x, M, "skip2"), mask_ptr, _nlc_ptr(post, x, M, "post"),
                                    y.ptr if y is not None else None, y2.ptr if y2 is not None else None, _ptr(y_ncl),
                                    x.B, C, M, x.L, KW, int(bool(relu)), *extra, _stream())
    if bits_out:
        y.has_bits = True
    _check(rc, f.conv)
    if out_ncl:
        return y_ncl
    return (y, y2) if post is not None else y


def _wgrad_out(who, dy, x, KW, w_layout, dw_out, accumulate):
    """fp32 dw in the weight's native layout -> (the caller's, shape-checked, or a fresh one; whether the launch adds to it)."""
    shape = (dy.C, x.C, KW) if w_layout == W_OIK else (x.C, dy.C, KW)
    if dw_out is None:
        return torch.empty(shape, device=x.storage.device, dtype=torch.float32), False
    if tuple(dw_out.shape) != shape:
        raise RuntimeError("%s: dw_out has shape %s, expected %s" % (who, tuple(dw_out.shape), shape))
    return dw_out, accumulate


def _wgrad_scratch(f, dy, x, KW, deferred):
    """The split partials of one launch: arena scratch, which lives until the batch reduction, when the reduction is deferred,
    else the grow-only workspace."""
    nbytes = getattr(lib(), f.wgrad_ws)(x.B, x.C, dy.C, x.L, KW)
    dev = x.storage.device
    return arena_alloc(nbytes, dev) if deferred else _workspace(nbytes, dev).data_ptr()


def _wgrad_launch(f, symbol, family, head, ws_ptr, nseg, dy, x, KW, w_layout, dw, dbias, accumulate, defer):
    """``head``: the operands in front of the workspace -- all that differs between the single- and the multi-segment ABI.
    ``defer``: None, or the list that receives the descriptors of the reduction this launch leaves undone."""
    B, C, M, L = x.B, x.C, dy.C, x.L
    scale = dy.gscale if f.scaled else None
    with _timed(family, 2.0 * nseg * B * L * M * C * KW):
        rc = getattr(lib(), symbol)(*head, ws_ptr, B, C, M, L, KW, w_layout,
                                    WGRAD_DEFER if defer is not None else int(bool(accumulate)),
                                    *((_sptr(scale, 1),) if f.scaled else ()), _stream())
    _check(rc, symbol)
    if defer is not None:
        _defer_descs(defer, ws_ptr, dw, dbias, scale, nseg, B, C, M, L, KW, w_layout)


def conv1d_wgrad_bf16(dy, x, KW, w_layout=W_OIK, want_bias=False, dw_out=None, dbias_out=None, accumulate=False, defer=None):
    """dy, x: NLC.  fp32 dw in the weight's native layout (and dbias).  ``defer`` (a list; bf16 / fp16 formats, with
    ``accumulate`` into caller-owned dw_out / dbias_out): launch the contraction only and append the reduction's descriptors
    -- the caller sums them all later with ``wgrad_reduce_batch``."""
    f = _FORMATS[dy.fmt]
    dw_out, accumulate = _wgrad_out("conv1d_wgrad_bf16", dy, x, KW, w_layout, dw_out, accumulate)
    if want_bias and dbias_out is None:
        dbias_out = torch.empty((dy.C,), device=x.storage.device, dtype=torch.float32)
    if not _fmt_serves(x, dy):
        raise RuntimeError("conv1d_wgrad_bf16: dy and x differ in format")
    if not (accumulate and f.defer):
        defer = None
    family = f.wgrad_family(KW, want_bias)
    dbias = dbias_out if want_bias else None
    _wgrad_launch(f, f.wgrad, family, (dy.ptr, x.ptr, _ptr(dw_out, name="dw"), _ptr(dbias, name="dbias")),
                  _wgrad_scratch(f, dy, x, KW, defer is not None), 1, dy, x, KW, w_layout, dw_out, dbias, accumulate, defer)
    return (dw_out, dbias_out) if want_bias else dw_out


def conv1d_wgrad_bf16_multi(pairs, KW, w_layout=W_OIK, dw_out=None, accumulate=False, defer=None):
    """dw (+)= sum_i wgrad(dy_i, x_i) in one launch (shared residual weights).  pairs: [(dy NLC, x NLC), ...] (1..4)."""
    dy0, x0 = pairs[0]
    f = _FORMATS[dy0.fmt]
    for dy, x in pairs:
        if (dy.B, dy.L, dy.C, dy.fmt, x.B, x.L, x.C) != (dy0.B, dy0.L, dy0.C, dy0.fmt, x0.B, x0.L, x0.C) or not _fmt_serves(x, dy):
            raise RuntimeError("conv1d_wgrad_bf16_multi: all segments must share one shape and format")
        if f.scaled and dy.gscale is not dy0.gscale:
            raise RuntimeError("conv1d_wgrad_bf16_multi: the segments belong to different loss-scale chains")
    dw_out, accumulate = _wgrad_out("conv1d_wgrad_bf16_multi", dy0, x0, KW, w_layout, dw_out, accumulate)
    n = len(pairs)
    dys = (ctypes.c_void_p * n)(*[dy.ptr for dy, _ in pairs])
    xs = (ctypes.c_void_p * n)(*[x.ptr for _, x in pairs])
    if not (accumulate and f.defer):
        defer = None
    ws_ptr = _wgrad_scratch(f, dy0, x0, KW, defer is not None)
    _wgrad_launch(f, f.wgrad_multi, f.wgrad_family(KW, False), (dys, xs, n, _ptr(dw_out, name="dw")), ws_ptr, n, dy0, x0, KW,
                  w_layout, dw_out, None, accumulate, defer)
    return dw_out


# ----------------------------------------------------------------------------------------------- k-means
def _rows(x, name):
    if x.dim() != 2:
        raise RuntimeError("%s must be (N, D) (got %s)" % (name, tuple(x.shape)))
    return x.shape


def kmeans_update(x, labels, labels_old, centers_old, centers_new, counts, stats, flags, tol, workspace=None):
    """One Lloyd update (alvq_kmeans_update_f32): centers_new (K, D) fp32, counts (K,) int32 (or None), stats (1,) fp64 and
    flags (4,) int32 out.  Returns the workspace (reuse it for the next iteration)."""
    N, D = _rows(x, "kmeans_update: x")
    K = centers_old.shape[0]
    if centers_old.shape != (K, D) or centers_new.shape != (K, D) or labels.shape != (N,):
        raise RuntimeError("kmeans_update: centres must be (%d, %d) and labels (%d,)" % (K, D, N))
    if labels_old is not None and labels_old.shape != (N,):
        raise RuntimeError("kmeans_update: labels_old must be (%d,)" % N)
    workspace = _scratch(lib().alvq_kmeans_update_workspace_bytes(N, K, D), x,
                         "kmeans_update: N=%d, K=%d, D=%d out of range" % (N, K, D), workspace)
    i64 = torch.int64
    _call("alvq_kmeans_update_f32", _ptr(x, name="x"), _ptr(labels, i64, "labels"), _ptr(labels_old, i64, "labels_old"),
          _ptr(centers_old, name="centers_old"), _ptr(centers_new, name="centers_new"), _ptr(counts, torch.int32, "counts"),
          _ptr(stats, torch.float64, "stats"), _ptr(flags, torch.int32, "flags"), _ptr(workspace, torch.uint8, "workspace"), N,
          K, D, float(tol))
    return workspace


def kmeans_inertia(x, labels, centers):
    """(1,) fp64 device tensor: sum_n |x_n - centers[labels_n]|^2 (alvq_kmeans_inertia_f32)."""
    N, D = _rows(x, "kmeans_inertia: x")
    K = centers.shape[0]
    if centers.shape != (K, D) or labels.shape != (N,):
        raise RuntimeError("kmeans_inertia: centres must be (K, %d) and labels (%d,)" % (D, N))
    out = _empty(x, torch.float64, 1)
    ws = torch.empty((lib().alvq_kmeans_inertia_workspace_bytes(N),), device=x.device, dtype=torch.uint8)
    _call("alvq_kmeans_inertia_f32", _ptr(x, name="x"), _ptr(labels, torch.int64, "labels"), _ptr(centers, name="centers"),
          _ptr(out, torch.float64), _ptr(ws, torch.uint8), N, K, D)
    return out


def kmeans_col_stats(x):
    """(mean (D,) fp32, var_mean (1,) fp64) of the rows of x (alvq_kmeans_col_stats_f32)."""
    N, D = _rows(x, "kmeans_col_stats: x")
    ws = _scratch(lib().alvq_kmeans_col_stats_workspace_bytes(N, D), x, "kmeans_col_stats: N=%d, D=%d out of range" % (N, D))
    mean, var_mean = _empty(x, torch.float32, D), _empty(x, torch.float64, 1)
    _call("alvq_kmeans_col_stats_f32", _ptr(x, name="x"), _ptr(mean), _ptr(var_mean, torch.float64), _ptr(ws, torch.uint8), N,
          D)
    return mean, var_mean


def kmeans_add_rows(x, v, alpha, out=None):
    """out = x + alpha * v[None, :] (alvq_kmeans_add_rows_f32); out may be x."""
    N, D = _rows(x, "kmeans_add_rows: x")
    if v.shape != (D,):
        raise RuntimeError("kmeans_add_rows: v must be (%d,)" % D)
    out = torch.empty_like(x) if out is None else out
    _call("alvq_kmeans_add_rows_f32", _ptr(x, name="x"), _ptr(v, name="v"), _ptr(out, name="out"), N, D, float(alpha))
    return out


def kmeans_plusplus(x, K, first, uniforms):
    """Greedy k-means++ seeding (alvq_kmeans_plusplus_f32) -> (centers (K, D) fp32, indices (K,) int64); uniforms (K-1, T)
    fp64 on the device."""
    N, D = _rows(x, "kmeans_plusplus: x")
    T = uniforms.shape[1] if uniforms is not None and uniforms.dim() == 2 else 0
    if K > 1 and (uniforms is None or uniforms.shape[0] != K - 1):
        raise RuntimeError("kmeans_plusplus: uniforms must be (%d, T)" % (K - 1))
    T = max(T, 1)
    ws = _scratch(lib().alvq_kmeans_plusplus_workspace_bytes(N, T), x, "kmeans_plusplus: N=%d, T=%d out of range" % (N, T))
    centers, indices = _empty(x, torch.float32, K, D), _empty(x, torch.int64, K)
    _call("alvq_kmeans_plusplus_f32", _ptr(x, name="x"), _ptr(uniforms if K > 1 else None, torch.float64, "uniforms"),
          _ptr(centers), indices.data_ptr(), _ptr(ws, torch.uint8), N, K, D, T, int(first))
    return centers, indices
