"""WPE dereverberation on the device (dereverberation.wpe, csrc/wpe.hip): the time of one launch at the dataset's shape,
B = 64, D = 1, F = 201, T = 500, the defaults (taps 10, delay 3, 3 iterations), complex128, from device events, the best of 5 --
next to the same arithmetic composed from stock torch ops on the device (unfold, matmul, torch.linalg.cholesky,
torch.cholesky_solve, batched over the B F bins), which is what a user had before the kernel.
    python tests/bench_wpe.py
Each of the two measurements runs in a child process of its own under a time limit; a child that fails or runs out of time ends
the script, and nothing more is started on the device.  For the kernel's own time run
`python tests/bench_wpe.py --step fused` once under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import family_bench as FB  # noqa: E402  (it puts the repository, the package and tests/helpers on the path)

from family_bench import F, T  # noqa: E402

B, D = 64, 1
TAPS, DELAY, ITERATIONS, PSD_CONTEXT, EPS, LOADING = 10, 3, 3, 0, 1e-10, 1e-10
STEPS = ("fused", "torch")


def reverberant_spectrogram():
    """(B, D, F, T) complex128 on the device: a complex Gaussian excitation under a syllable-rate envelope plus eight delayed,
    decaying copies of itself per bin."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    shape = (B, D, F, T)
    env = 0.05 + torch.sin(torch.arange(T, dtype=torch.float64, device="cuda") * 0.21).abs() ** 4
    s = FB.gauss(g, *shape) * torch.sqrt(env / 2)
    x = s.clone()
    for k in range(8):
        gain = 0.4 * 0.7 ** k * FB.gauss(g, B, D, F, 1)
        x[..., DELAY + k:] += gain * s[..., :T - DELAY - k]
    return x


def torch_wpe(X):
    """The definition of include/alvq.h from stock torch ops, batched over the bins."""
    import torch
    x = X.permute(0, 2, 1, 3).reshape(B * F, D, T)
    past = torch.nn.functional.pad(torch.view_as_real(x), (0, 0, DELAY + TAPS - 1, 0))
    past = torch.view_as_complex(past).unfold(2, TAPS, 1)[:, :, :T].flip(-1)          # (bins, D, T, taps): x_d[t - delay - k]
    xt = past.permute(0, 3, 1, 2).reshape(B * F, TAPS * D, T)
    eye = torch.eye(TAPS * D, dtype=torch.float64, device=X.device)
    y = x
    for _ in range(ITERATIONS):
        q = (y.real ** 2 + y.imag ** 2).sum(1, keepdim=True)                           # (bins, 1, T)
        if PSD_CONTEXT:
            ones = torch.ones(1, 1, 2 * PSD_CONTEXT + 1, dtype=torch.float64, device=X.device)
            count = torch.nn.functional.conv1d(torch.ones(1, 1, T, dtype=torch.float64, device=X.device), ones, padding=PSD_CONTEXT)
            q = torch.nn.functional.conv1d(q, ones, padding=PSD_CONTEXT) / count
        p = q / D
        lam = torch.maximum(p, EPS * p.amax(2, keepdim=True))
        xw = xt / lam
        r = xw @ xt.mH
        pm = xw @ x.mH
        r = r + (LOADING / (TAPS * D)) * torch.diagonal(r, dim1=1, dim2=2).real.sum(1)[:, None, None] * eye
        g = torch.cholesky_solve(pm, torch.linalg.cholesky(r))
        y = x - g.mH @ xt
    return y.reshape(B, F, D, T).permute(0, 2, 1, 3)


def step(name):
    import torch
    from acoustic_locating_vq_vae import dereverberation as DV
    X = reverberant_spectrogram()
    fused = DV.wpe(X, TAPS, DELAY, ITERATIONS, PSD_CONTEXT, EPS, LOADING)
    out = {"step": name, "B": B, "D": D, "F": F, "T": T, "taps": TAPS, "delay": DELAY, "iterations": ITERATIONS}
    if name == "fused":
        out["seconds"] = FB.best_seconds(lambda: DV.wpe(X, TAPS, DELAY, ITERATIONS, PSD_CONTEXT, EPS, LOADING), 10)
        out["bins_with_status"] = int((fused.status != 0).sum())
        terms = B * F * ITERATIONS * T * (TAPS * D * (TAPS * D + 1) / 2 + 2 * TAPS * D * D)   # correlation build and filter
        out["complex_macs_per_s"] = terms / out["seconds"]
    else:
        composed = torch_wpe(X)
        out["max_abs_diff_to_fused"] = float((composed - fused.spec).abs().max())
        out["max_abs_x"] = float(X.abs().max())
        out["seconds"] = FB.best_seconds(lambda: torch_wpe(X), 3)
    print(json.dumps(out), flush=True)


def summarise(results):
    print(json.dumps({"fused_ms": results["fused"]["seconds"] * 1e3, "torch_ms": results["torch"]["seconds"] * 1e3,
                      "torch_over_fused": results["torch"]["seconds"] / results["fused"]["seconds"],
                      "max_abs_diff": results["torch"]["max_abs_diff_to_fused"]}), flush=True)


def main():
    FB.main(__file__, STEPS, step, summarise)


if __name__ == "__main__":
    main()
