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
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "acoustic_locating_vq-vae_amd")
for p in (ROOT, PKG, os.path.join(PKG, "src")):
    sys.path.insert(0, p)

B, D, F, T = 64, 8, 201, 500
LOADING = 1e-6
COPY_BYTES_PER_S = 6.3e12
STEP_SECONDS = 300
STEPS = ("fused_cov", "torch_cov", "fused_weights", "torch_weights", "fused_apply", "torch_apply")


def best_seconds(fn, reps):
    """Seconds per call of fn from device events around reps calls, the best of 5."""
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3 / reps)
    return best


def scene():
    """(X (B, D, F, T) complex128, mask (B, F, T), A (B, D, F)) on the device: a source and an interferer seen through steering
    vectors of a 5 cm array plus sensor noise of scale 0.03, and a uniform mask."""
    import torch
    from acoustic_locating_vq_vae import beamforming as BF
    g = torch.Generator(device="cuda").manual_seed(0)

    def gauss(*shape):
        return torch.complex(torch.randn(shape, dtype=torch.float64, device="cuda", generator=g),
                             torch.randn(shape, dtype=torch.float64, device="cuda", generator=g))
    centre = torch.tensor([2.5, 1.5, 1.5], dtype=torch.float64, device="cuda")
    mics = centre + 0.05 * (2 * torch.rand((D, 3), dtype=torch.float64, device="cuda", generator=g) - 1)
    angle = 6.283185307179586 * torch.rand((2, B), dtype=torch.float64, device="cuda", generator=g)
    points = centre + torch.stack((torch.cos(angle), torch.sin(angle), torch.ones_like(angle)), dim=-1)       # (2, B, 3)
    A, _ = BF.steering_vectors(mics, points[0], F)
    Bv, _ = BF.steering_vectors(mics, points[1], F)
    X = A[..., None] * gauss(B, 1, F, T) + Bv[..., None] * gauss(B, 1, F, T) + 0.03 * gauss(B, D, F, T)
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
    out["seconds"] = best_seconds(fn, 10)
    # the bytes the launch has to move: the spectrogram once, plus the mask (covariance) or the output (application)
    moved = {"cov": X.numel() * 16 + mask.numel() * 8 + cov.cov.numel() * 16, "apply": X.numel() * 16 + w.w.numel() * 16 + y.numel() * 16,
             "weights": cov.cov.numel() * 16 + A.numel() * 16 + w.w.numel() * 16}[what]
    out["bytes"] = moved
    out["bytes_per_s"] = moved / out["seconds"]
    out["share_of_copy_rate"] = out["bytes_per_s"] / COPY_BYTES_PER_S
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        return step(sys.argv[2])
    results = {}
    for name in STEPS:
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], timeout=STEP_SECONDS,
                                  stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            sys.exit("bench_beamform: step %s ran out of its %d s; nothing more is started" % (name, STEP_SECONDS))
        if done.returncode != 0:
            sys.exit("bench_beamform: step %s ended with status %d; nothing more is started" % (name, done.returncode))
        results[name] = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps(results[name]), flush=True)
    for what in ("cov", "weights", "apply"):
        fused, composed = results["fused_" + what], results["torch_" + what]
        print(json.dumps({"launch": what, "fused_ms": fused["seconds"] * 1e3, "torch_ms": composed["seconds"] * 1e3,
                          "torch_over_fused": composed["seconds"] / fused["seconds"],
                          "fused_TB_per_s": fused["bytes_per_s"] * 1e-12, "copy_TB_per_s": COPY_BYTES_PER_S * 1e-12,
                          "max_abs_diff": composed["max_abs_diff_to_fused"]}), flush=True)


if __name__ == "__main__":
    main()
