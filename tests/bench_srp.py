"""SRP-PHAT localisation on the device (localization.srp_phat, csrc/srp_phat.hip): the time of the cross-spectra launch and of
the SRP launch at B = 64, D = 8, F = 201, T = 500, band (8, 187), complex128, for (a) the 360-angle ring and (b) the 0.1 m grid
of the 4 x 5 x 3 m room (60 000 points), from device events, the best of 5 -- next to the same arithmetic composed from stock
torch ops on the device (unit phasors and an einsum for the cross-spectra; per-microphone steering phasors and an einsum over
the pair matrix for the map, in chunks of candidates so that it fits in memory), which is what a user had before the kernels.
    python tests/bench_srp.py
Each measurement runs in a child process of its own under a time limit; a child that fails or runs out of time ends the
script, and nothing more is started on the device.  No threshold is asserted: there is no earlier kernel to compare with.
The achieved float64 rate counts 8 flops per rotation (the four fused multiply-adds of psi conj(z_j) accumulated; the
sincospi of the D phasors per candidate and bin and the D products with z_i are not counted)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)

from family_bench import F, T  # noqa: E402

B, D = 64, 8
N_FFT, FS, C = 400, 16000.0, 340.0
BAND = (8, 187)
P, F_BAND = D * (D - 1) // 2, BAND[1] - BAND[0] + 1
FLOPS_PER_ROTATION = 8
CHUNK = 1024                 # candidates per step of the torch composition
STEPS = ("phat", "ring", "grid", "torch_phat", "torch_ring", "torch_grid")
WARMUPS = 1                  # not family_bench's two: this script's figures in DESIGN.md were taken after one warm-up call


def scene():
    """(X (B, D, F, T) complex128, mics (D, 3), ring (360, 3), grid (60000, 3)) on the device: a source per item on the ring,
    free-field delays to eight microphones within 5 cm of the receiver, complex Gaussian noise of scale 0.1."""
    import math
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    mics, ring = FB.array_microphones(g, D), FB.candidate_ring(360)
    ax = [0.05 + 0.1 * torch.arange(n, dtype=torch.float64, device="cuda") for n in (40, 50, 30)]
    grid = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
    true = torch.randint(0, 360, (B,), device="cuda", generator=g)
    r = (ring[true][:, None, :] - mics[None]).norm(dim=-1)                                    # (B, D)
    omega = 2 * math.pi * torch.arange(F, dtype=torch.float64, device="cuda") * FS / N_FFT
    S = FB.gauss(g, B, 1, F, T)
    phase = -omega[None, None, :] * r[:, :, None] / C                                         # (B, D, F)
    X = S * torch.polar((1.0 / r)[:, :, None].expand_as(phase).contiguous(), phase)[..., None]
    X = X + 0.1 * FB.gauss(g, B, D, F, T)
    return X, mics, ring, grid, true


def band_weights():
    import torch
    f = torch.arange(BAND[0], BAND[1] + 1, device="cuda")
    return torch.where((f == 0) | (2 * f == N_FFT), 1.0, 2.0).to(torch.float64)


def torch_phat(X):
    """psi (B, D, D, F_band) from stock torch ops: entry (i, j) = mean_t u_i conj(u_j)."""
    import torch
    x = X[:, :, BAND[0]:BAND[1] + 1]
    mag = x.abs()
    u = torch.where(mag == 0, torch.zeros_like(x), x / torch.where(mag == 0, torch.ones_like(mag), mag))
    return torch.einsum("bift,bjft->bijf", u, u.conj()) / T


def torch_srp(psi_full, mics, cand):
    """The map (B, G) from stock torch ops: per-microphone steering phasors, the pair matrix (upper triangle, weighted), an
    einsum, in chunks of candidates."""
    import math
    import torch
    f = torch.arange(BAND[0], BAND[1] + 1, dtype=torch.float64, device="cuda")
    upper = torch.triu(torch.ones(D, D, dtype=torch.float64, device="cuda"), diagonal=1)
    M = psi_full * (upper[None, :, :, None] * band_weights()[None, None, None, :])            # (B, D, D, Fb)
    out = []
    for g0 in range(0, cand.shape[0], CHUNK):
        tau = (cand[g0:g0 + CHUNK, None, :] - mics[None]).norm(dim=-1) / C                    # (G', D)
        phase = 2 * math.pi * (FS / N_FFT) * tau[:, :, None] * f                             # (G', D, Fb)
        z = torch.polar(torch.ones_like(phase), phase)
        y = torch.einsum("bijf,gjf->bgif", M, z.conj())
        out.append((y * z[None]).sum(dim=(2, 3)).real)
    return torch.cat(out, dim=1) / (P * band_weights().sum())


def step(name):
    import torch
    from acoustic_locating_vq_vae import _native as N
    from acoustic_locating_vq_vae import localization as LOC
    X, mics, ring, grid, true = scene()
    out = {"step": name, "B": B, "D": D, "F": F, "T": T, "band": BAND}
    psi, _ = N.phat_cross_spectra(X, *BAND)
    cand = grid if name.endswith("grid") else ring
    if name == "phat":
        out["seconds"] = FB.best_seconds(lambda: N.phat_cross_spectra(X, *BAND), 10, warmups=WARMUPS)
    elif name in ("ring", "grid"):
        run = lambda: N.srp_phat(psi, mics, cand, FS, N_FFT, C, *BAND)                        # noqa: E731
        m, best, status = run()
        out["G"] = cand.shape[0]
        out["seconds"] = FB.best_seconds(run, 10 if name == "ring" else 3, warmups=WARMUPS)
        out["items_with_status"] = int((status != 0).sum())
        rotations = B * cand.shape[0] * P * F_BAND
        out["rotations_per_s"] = rotations / out["seconds"]
        out["float64_flops_per_s"] = FLOPS_PER_ROTATION * rotations / out["seconds"]
        if name == "ring":
            out["items_on_the_true_angle"] = int((best == true).sum())
    elif name == "torch_phat":
        full = torch_phat(X)
        i, j = torch.triu_indices(D, D, offset=1)
        out["max_abs_diff_to_fused"] = float((full[:, i, j] - psi[:, :, BAND[0]:BAND[1] + 1]).abs().max())
        out["seconds"] = FB.best_seconds(lambda: torch_phat(X), 3, warmups=WARMUPS)
    else:
        full = torch_phat(X)
        composed = torch_srp(full, mics, cand)
        out["G"] = cand.shape[0]
        out["max_abs_diff_to_fused"] = float((composed - LOC.srp_phat(X, mics, cand, FS, N_FFT, C, BAND).map).abs().max())
        out["seconds"] = FB.best_seconds(lambda: torch_srp(full, mics, cand), 1, rounds=3, warmups=WARMUPS)
    print(json.dumps(out), flush=True)


def summarise(results):
    ms = {k: v["seconds"] * 1e3 for k, v in results.items()}
    print(json.dumps({"phat_ms": ms["phat"], "torch_phat_ms": ms["torch_phat"], "ring_ms": ms["ring"], "torch_ring_ms": ms["torch_ring"],
                      "grid_ms": ms["grid"], "torch_grid_ms": ms["torch_grid"],
                      "torch_over_fused": {k: ms["torch_" + k] / ms[k] for k in ("phat", "ring", "grid")},
                      "grid_float64_tflops": results["grid"]["float64_flops_per_s"] / 1e12,
                      "max_abs_diff": {k: results["torch_" + k]["max_abs_diff_to_fused"] for k in ("phat", "ring", "grid")}}), flush=True)


def main():
    FB.main(__file__, STEPS, step, summarise)


if __name__ == "__main__":
    main()
