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
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)

from family_bench import F, T  # noqa: E402

B, D, G = 64, 8, 360
K = 2
BAND = (8, 187)
LOADING = 1e-6
STEPS = ("fused_eigh", "torch_eigh", "fused_music", "srp_map", "fused_gev", "fused_souden", "music_whole", "srp_whole")


def scene():
    """(X (B, D, F, T) complex128, mask (B, F, T), mics (D, 3), cand (G, 3)) on the device: a source and an interferer on the
    candidates' ring seen through steering vectors of a 5 cm array plus sensor noise of scale 0.03, and a uniform mask."""
    import torch
    from acoustic_locating_vq_vae import beamforming as BF
    g = torch.Generator(device="cuda").manual_seed(0)
    mics, cand = FB.array_microphones(g, D), FB.candidate_ring(G)
    pick = torch.randint(0, G, (2, B), device="cuda", generator=g)
    A, _ = BF.steering_vectors(mics, cand[pick[0]], F)
    Bv, _ = BF.steering_vectors(mics, cand[pick[1]], F)
    X = A[..., None] * FB.gauss(g, B, 1, F, T) + Bv[..., None] * FB.gauss(g, B, 1, F, T) + 0.03 * FB.gauss(g, B, D, F, T)
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
    out["seconds"] = FB.best_seconds(fn, reps)
    print(json.dumps(out), flush=True)


def summarise(results):
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


def main():
    FB.main(__file__, STEPS, step, summarise)


if __name__ == "__main__":
    main()
