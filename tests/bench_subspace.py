"""The subspace methods on the device (acoustic_locating_vq_vae.subspace / .localization / .beamforming; csrc/herm_eig.h,
csrc/subspace.hip, csrc/beamform.hip): the time of the Hermitian eigensolver, of the MUSIC map and of the GEV weights at
B = 64, D = 8, F = 201, T = 500 (12 864 covariances of order 8) and G = 360 ring candidates, from device events, the best of 5.
There was no such path before, so the yardsticks are what a user had: ``torch.linalg.eigh`` on the same device tensor for
the eigensolver (a solver library behind a host sync; if this build of torch has none for the device, the step says so and
the ratio is left out) and ``srp_phat``'s three launches on the same spectrogram for the map.  Both are reported as ratios;
neither is a gate.
    python tests/bench_subspace.py
Each measurement runs in a child process of its own under a time limit; a child that fails or runs out of time ends the script,
and nothing more is started on the device.  For a kernel's own time run `python tests/bench_subspace.py --step fused_eigh`
(or fused_music, fused_gev) once under rocprofv3 --kernel-trace --stats."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "acoustic_locating_vq-vae_amd")
for p in (ROOT, PKG, os.path.join(PKG, "src")):
    sys.path.insert(0, p)

B, D, F, T, G = 64, 8, 201, 500, 360
K = 2
BAND = (8, 187)
LOADING = 1e-6
STEP_SECONDS = 300
STEPS = ("fused_eigh", "torch_eigh", "fused_music", "srp_map", "fused_gev", "fused_souden", "music_whole", "srp_whole")


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
    """(X (B, D, F, T) complex128, mask (B, F, T), mics (D, 3), cand (G, 3)) on the device: a source and an interferer on the
    candidates' ring seen through steering vectors of a 5 cm array plus sensor noise of scale 0.03, and a uniform mask."""
    import torch
    from acoustic_locating_vq_vae import beamforming as BF
    g = torch.Generator(device="cuda").manual_seed(0)

    def gauss(*shape):
        return torch.complex(torch.randn(shape, dtype=torch.float64, device="cuda", generator=g),
                             torch.randn(shape, dtype=torch.float64, device="cuda", generator=g))
    centre = torch.tensor([2.5, 1.5, 1.5], dtype=torch.float64, device="cuda")
    mics = centre + 0.05 * (2 * torch.rand((D, 3), dtype=torch.float64, device="cuda", generator=g) - 1)
    theta = -3.141592653589793 + 6.283185307179586 * torch.arange(G, dtype=torch.float64, device="cuda") / G
    cand = centre + torch.stack((torch.cos(theta), torch.sin(theta), torch.ones_like(theta)), dim=-1)        # (G, 3)
    pick = torch.randint(0, G, (2, B), device="cuda", generator=g)
    A, _ = BF.steering_vectors(mics, cand[pick[0]], F)
    Bv, _ = BF.steering_vectors(mics, cand[pick[1]], F)
    X = A[..., None] * gauss(B, 1, F, T) + Bv[..., None] * gauss(B, 1, F, T) + 0.03 * gauss(B, D, F, T)
    mask = torch.rand((B, F, T), dtype=torch.float64, device="cuda", generator=g)
    return X, mask, mics, cand


def step(name):
    import torch
    from acoustic_locating_vq_vae import _native as N
    from acoustic_locating_vq_vae import beamforming as BF
    from acoustic_locating_vq_vae import localization as LOC
    from acoustic_locating_vq_vae import subspace as SUB
    X, mask, mics, cand = scene()
    cov = BF.spatial_covariance(X).cov
    cov_n, cov_s = BF.spatial_covariance(X, mask).cov, BF.spatial_covariance(X, 1 - mask).cov
    eig = SUB.eigh(cov)
    out = {"step": name, "B": B, "D": D, "F": F, "T": T, "G": G, "K": K, "matrices": B * F}
    reps = 10
    if name == "fused_eigh":
        fn = lambda: SUB.eigh(cov)                                                                            # noqa: E731
        out["matrices_with_status"] = int((eig.status != 0).sum())
    elif name == "torch_eigh":
        try:
            values, vectors = torch.linalg.eigh(cov)
            torch.cuda.synchronize()
        except Exception as e:                                           # no solver for the device in this build of torch
            out["unavailable"] = "%s: %s" % (type(e).__name__, str(e).splitlines()[0] if str(e) else "")
            print(json.dumps(out), flush=True)
            return
        fn, reps = (lambda: torch.linalg.eigh(cov)), 1
        out["max_abs_diff_of_values"] = float((values - eig.values).abs().max())
        out["max_abs_value"] = float(eig.values.abs().max())
    elif name == "fused_music":
        fn = lambda: N.music(eig.vectors, eig.values, mics, cand, K, 16000.0, 400, 340.0, *BAND)              # noqa: E731
        out["items_with_status"] = int((fn()[2] != 0).sum())
    elif name == "srp_map":
        psi, _ = N.phat_cross_spectra(X, *BAND)
        fn = lambda: N.srp_phat(psi, mics, cand, 16000.0, 400, 340.0, *BAND)                                  # noqa: E731
    elif name == "fused_gev":
        fn = lambda: BF.gev_weights(cov_n, cov_s, loading=LOADING)                                            # noqa: E731
        out["bins_with_status"] = int((fn().status != 0).sum())
    elif name == "fused_souden":
        fn = lambda: BF.weights("souden", cov_n, speech_cov=cov_s, loading=LOADING)                           # noqa: E731
    elif name == "music_whole":
        fn = lambda: LOC.music(X, mics, cand, K, c=340.0, band=BAND)                                          # noqa: E731
    elif name == "srp_whole":
        fn = lambda: LOC.srp_phat(X, mics, cand, c=340.0, band=BAND)                                          # noqa: E731
    else:
        sys.exit("bench_subspace: no step %r" % name)
    out["seconds"] = best_seconds(fn, reps)
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
            sys.exit("bench_subspace: step %s ran out of its %d s; nothing more is started" % (name, STEP_SECONDS))
        if done.returncode != 0:
            sys.exit("bench_subspace: step %s ended with status %d; nothing more is started" % (name, done.returncode))
        results[name] = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps(results[name]), flush=True)

    def ms(name):
        return results[name]["seconds"] * 1e3
    eigh = {"launch": "eigh", "fused_ms": ms("fused_eigh"), "matrices_per_s": B * F / results["fused_eigh"]["seconds"]}
    if "unavailable" in results["torch_eigh"]:
        eigh["torch"] = "unavailable: " + results["torch_eigh"]["unavailable"]
    else:
        eigh.update(torch_ms=ms("torch_eigh"), torch_over_fused=ms("torch_eigh") / ms("fused_eigh"),
                    max_abs_diff_of_values=results["torch_eigh"]["max_abs_diff_of_values"])
    print(json.dumps(eigh), flush=True)
    print(json.dumps({"launch": "map", "music_ms": ms("fused_music"), "srp_ms": ms("srp_map"),
                      "music_over_srp": ms("fused_music") / ms("srp_map")}), flush=True)
    print(json.dumps({"launch": "weights", "gev_ms": ms("fused_gev"), "souden_ms": ms("fused_souden"),
                      "gev_over_souden": ms("fused_gev") / ms("fused_souden")}), flush=True)
    print(json.dumps({"launch": "spectrogram to map", "music_ms": ms("music_whole"), "srp_ms": ms("srp_whole"),
                      "music_over_srp": ms("music_whole") / ms("srp_whole")}), flush=True)


if __name__ == "__main__":
    main()
