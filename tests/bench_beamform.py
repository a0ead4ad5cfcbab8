"""Beamforming on the device (acoustic_locating_vq_vae.beamforming, csrc/beamform.hip): the time of each of the three
launches of an MVDR beamformer -- mask-weighted spatial covariance, weights, application -- at B = 64, D = 8, F = 201, T = 500,
complex128 (an 823 MB spectrogram), from device events, the best of 5 -- next to the same arithmetic composed from stock torch
ops on the device (matmul, einsum, torch.linalg.cholesky, torch.cholesky_solve, batched over the B F bins), which is what a user had
before the kernels.  The covariance and the application stream the spectrogram once, so their bytes a second are printed next
to the 6.3 TB/s a copy reaches.
    python tests/bench_beamform.py
Each measurement runs in a child process of its own under a time limit; a child that fails or runs out of time ends the script,
and nothing more is started on the device.  For a kernel's own time run `python tests/bench_beamform.py --step fused_cov`
(or fused_weights, fused_apply) once under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)

from family_bench import COPY_BYTES_PER_S, F, T  # noqa: E402

B, D = 64, 8
LOADING = 1e-6
STEPS = ("fused_cov", "torch_cov", "fused_weights", "torch_weights", "fused_apply", "torch_apply")


def scene():
    """(X (B, D, F, T) complex128, mask (B, F, T), A (B, D, F)) on the device: a source and an interferer seen through steering
    vectors of a 5 cm array plus sensor noise of scale 0.03, and a uniform mask."""
    import torch
    from acoustic_locating_vq_vae import beamforming as BF
    g = torch.Generator(device="cuda").manual_seed(0)
    centre, mics = FB.array_centre(), FB.array_microphones(g, D)
    angle = 6.283185307179586 * torch.rand((2, B), dtype=torch.float64, device="cuda", generator=g)
    points = centre + torch.stack((torch.cos(angle), torch.sin(angle), torch.ones_like(angle)), dim=-1)       # (2, B, 3)
    A, _ = BF.steering_vectors(mics, points[0], F)
    Bv, _ = BF.steering_vectors(mics, points[1], F)
    X = A[..., None] * FB.gauss(g, B, 1, F, T) + Bv[..., None] * FB.gauss(g, B, 1, F, T) + 0.03 * FB.gauss(g, B, D, F, T)
    mask = torch.rand((B, F, T), dtype=torch.float64, device="cuda", generator=g)
    return X, mask, A


def torch_cov(X, mask):
    """The definition of include/alvq.h from stock torch ops."""
    xp = X.permute(0, 2, 1, 3)                                                                                # (B, F, D, T)
    return ((xp * mask[:, :, None, :]) @ xp.mH) / mask.sum(-1)[:, :, None, None]


def torch_weights(cov, A):
    import torch
    eye = torch.eye(D, dtype=torch.float64, device=cov.device)
    loaded = cov + (LOADING / D) * torch.diagonal(cov, dim1=-2, dim2=-1).real.sum(-1)[:, :, None, None] * eye
    a = A.permute(0, 2, 1)[..., None]                                                                         # (B, F, D, 1)
    z = torch.cholesky_solve(a, torch.linalg.cholesky(loaded))
    return (z / (a.conj() * z).sum(-2, keepdim=True).real)[..., 0]


def torch_apply(X, w):
    import torch
    return torch.einsum("bfd,bdft->bft", w.conj(), X)


def step(name):
    import torch
    from acoustic_locating_vq_vae import beamforming as BF
    X, mask, A = scene()
    cov = BF.spatial_covariance(X, mask)
    w = BF.weights("mvdr", cov.cov, A, loading=LOADING)
    y = BF.apply(X, w.w)
    out = {"step": name, "B": B, "D": D, "F": F, "T": T, "spectrogram_bytes": X.numel() * 16}
    what = name.split("_", 1)[1]
    if name.startswith("fused"):
        fn = {"cov": lambda: BF.spatial_covariance(X, mask), "weights": lambda: BF.weights("mvdr", cov.cov, A, loading=LOADING),
              "apply": lambda: BF.apply(X, w.w)}[what]
        out["bins_with_status"] = int((cov.status != 0).sum() + (w.status != 0).sum())
    else:
        fn = {"cov": lambda: torch_cov(X, mask), "weights": lambda: torch_weights(cov.cov, A), "apply": lambda: torch_apply(X, w.w)}[what]
        ours = {"cov": cov.cov, "weights": w.w, "apply": y}[what]
        out["max_abs_diff_to_fused"] = float((fn() - ours).abs().max())
        out["max_abs_fused"] = float(ours.abs().max())
    out["seconds"] = FB.best_seconds(fn, 10)
    # the bytes the launch has to move: the spectrogram once, plus the mask (covariance) or the output (application)
    moved = {"cov": X.numel() * 16 + mask.numel() * 8 + cov.cov.numel() * 16, "apply": X.numel() * 16 + w.w.numel() * 16 + y.numel() * 16,
             "weights": cov.cov.numel() * 16 + A.numel() * 16 + w.w.numel() * 16}[what]
    out["bytes"] = moved
    out["bytes_per_s"] = moved / out["seconds"]
    out["share_of_copy_rate"] = out["bytes_per_s"] / COPY_BYTES_PER_S
    print(json.dumps(out), flush=True)


def summarise(results):
    for what in ("cov", "weights", "apply"):
        fused, composed = results["fused_" + what], results["torch_" + what]
        print(json.dumps({"launch": what, "fused_ms": fused["seconds"] * 1e3, "torch_ms": composed["seconds"] * 1e3,
                          "torch_over_fused": composed["seconds"] / fused["seconds"],
                          "fused_TB_per_s": fused["bytes_per_s"] * 1e-12, "copy_TB_per_s": COPY_BYTES_PER_S * 1e-12,
                          "max_abs_diff": composed["max_abs_diff_to_fused"]}), flush=True)


def main():
    FB.main(__file__, STEPS, step, summarise)


if __name__ == "__main__":
    main()
