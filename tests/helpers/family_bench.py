"""What the stand-alone benchmark scripts (tests/bench_*.py, tools/bench_separation_metrics.py) share: the import paths, the
rates and shapes they quote, their timers, the child-per-step driver, the iteration arithmetic and the pieces their inputs are
made of.  A script puts tests/helpers on the path, imports this module, and keeps what is its own: its shapes, its floors, its
scene and its JSON keys.  Importing this module imports no torch: the timers and recipes import it when they are called."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "acoustic_locating_vq-vae_amd")
for p in (ROOT, PKG, os.path.join(PKG, "src"), os.path.join(ROOT, "tests", "helpers")):
    sys.path.insert(0, p)

COPY_BYTES_PER_S = 6.3e12                # what a device copy reaches
FP64_FLOP_PER_S = 78.6e12                # the float64 vector rate (datasheet)
STEP_SECONDS = 300                       # the time limit of one child step
F, T = 201, 500                          # the dataset's spectrogram
ITER_LO, ITER_HI, ITER_CALL = 4, 12, 20  # the two iteration counts an iteration's time is taken from, and a whole call's
ARRAY_CENTRE = (2.5, 1.5, 1.5)


# ---- timers -------------------------------------------------------------------------------------------------------------------

def best_seconds(fn, reps, rounds=5, warmups=2):
    """Seconds per call of fn from device events around reps calls, the best of ``rounds``, after ``warmups`` calls."""
    import torch
    for _ in range(warmups):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3 / reps)
    return best


def event_ms(fn, reps, rounds=1, reset=None):
    """Milliseconds per call of fn from device events around reps calls, the mean over ``rounds`` (``reset()`` before each,
    outside the events), after one warm-up call."""
    import torch
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = 0.0
    for _ in range(rounds):
        if reset is not None:
            reset()
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms += ev[0].elapsed_time(ev[1])
    return ms / (reps * rounds)


def wall_seconds(fn, reps):
    """Seconds per call of fn on the host's clock: one warm-up call, then reps calls between two synchronisations."""
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def iteration_ms(call, iter_call=ITER_CALL):
    """(ms of one iteration, ms of a whole call of iter_call iterations, ms a call spends outside its iterations) of
    ``call(iterations)``, measured at ITER_LO, ITER_HI and iter_call in that order, 3 calls a round.  ``iter_call=None`` leaves
    the whole call out (and its figure None)."""
    lo = best_seconds(lambda: call(ITER_LO), 3)
    hi = best_seconds(lambda: call(ITER_HI), 3)
    whole = None if iter_call is None else best_seconds(lambda: call(iter_call), 3) * 1e3
    return (hi - lo) / (ITER_HI - ITER_LO) * 1e3, whole, (lo - ITER_LO * (hi - lo) / (ITER_HI - ITER_LO)) * 1e3


# ---- the child-per-step driver ------------------------------------------------------------------------------------------------

def run_steps(script, steps, seconds=STEP_SECONDS):
    """Each of steps as ``python script --step NAME`` in a child process of its own under ``seconds``.  The last line of a
    step's stdout is printed and parsed; {name: parsed line} is returned.  A child that runs out of time or ends with a status
    ends this process with a message, and nothing more is started on the device."""
    script = os.path.abspath(script)
    who = os.path.splitext(os.path.basename(script))[0]
    results = {}
    for name in steps:
        try:
            done = subprocess.run([sys.executable, script, "--step", name], timeout=seconds, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            sys.exit("%s: step %s ran out of its %d s; nothing more is started" % (who, name, seconds))
        if done.returncode != 0:
            sys.exit("%s: step %s ended with status %d; nothing more is started" % (who, name, done.returncode))
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results[name] = json.loads(line)
    return results


def main(script, steps, step, summarise=None):
    """A script's command line: ``--step NAME`` runs ``step(NAME)`` in this process; no argument runs every step in a child of
    its own and hands the parsed lines to ``summarise``."""
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        return step(sys.argv[2])
    results = run_steps(script, steps)
    if summarise is not None:
        summarise(results)


# ---- input recipes (each draws from the generator it is given, in the order written here) -------------------------------------

def gauss(generator, *shape):
    """Complex normal noise on the device, complex128: the real parts drawn first, then the imaginary parts."""
    import torch
    return torch.complex(torch.randn(shape, dtype=torch.float64, device="cuda", generator=generator),
                         torch.randn(shape, dtype=torch.float64, device="cuda", generator=generator))


def array_centre():
    import torch
    return torch.tensor(ARRAY_CENTRE, dtype=torch.float64, device="cuda")


def array_microphones(generator, D):
    """(D, 3): D microphones within 5 cm (per axis) of the array's centre; one draw of (D, 3) uniforms."""
    import torch
    return array_centre() + 0.05 * (2 * torch.rand((D, 3), dtype=torch.float64, device="cuda", generator=generator) - 1)


def candidate_ring(G):
    """(G, 3): G candidates on the unit circle around the array's centre, one metre above it, from -pi on."""
    import math
    import torch
    theta = -math.pi + 2 * math.pi * torch.arange(G, dtype=torch.float64, device="cuda") / G
    return array_centre() + torch.stack((torch.cos(theta), torch.sin(theta), torch.ones_like(theta)), dim=-1)


def mixture(B, D, K, cdtype, noise=0.0):
    """(B, D, F, T) on the device, the recipe of iva_ref.case and cacgmm_ref.case: per source a per-frame activity
    gamma(0.3) + 1e-3 shared by all bins times complex Gaussian noise, K sources mixed by a random complex D x K matrix per bin,
    plus sensor noise of scale ``noise`` (not drawn when 0)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    act = torch.distributions.Gamma(torch.tensor(0.3, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    torch.manual_seed(0)
    activity = act.sample((B, K, 1, T)).cuda() + 1e-3
    S = activity * gauss(g, B, K, F, T)
    X = torch.einsum("bfdk,bkft->bdft", gauss(g, B, F, D, K), S)
    if noise:
        X = X + noise * gauss(g, B, D, F, T)
    return X.to(cdtype).contiguous()
