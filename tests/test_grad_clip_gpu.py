"""Global-norm gradient clipping and the warm-up / cosine schedule on the device (csrc/grad_clip.hip) against the float64
restatement (tests/helpers/grad_clip_ref.py, itself pinned to torch in tests/test_grad_clip_cpu.py), against
torch.nn.utils.clip_grad_norm_ inside the CPU oracle's training loop, and through the trainers: exactness of the clipped step,
the EMA span kept out of the norm, graph replay (with a forced one-rank RCCL all-reduce too), the schedule's rates, skipped
steps and resume."""
import json
import math
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import grad_clip_ref as G  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import _ops  # noqa: E402
from acoustic_locating_vq_vae.train_step import _ALIGN, FlatAdam, FlatBuffers, LocationTrainer, Trainer, WarmupCosine  # noqa: E402
from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE  # noqa: E402
from oracle import location_oracle as LO  # noqa: E402
from oracle import vqvae_oracle as O  # noqa: E402

CFG = (20, 48, 8, 2, 24, 0.25, 64)          # in, H, D, R, RH, beta, K: the tiny speech config of the trainer tests
INF = float("inf")


@pytest.fixture(autouse=True)
def f32_mode():
    prev = _ops.get_compute_dtype()
    _ops.set_compute_dtype("f32")
    yield
    _ops.set_compute_dtype(prev)


def scalars(grad_scale=1.0):
    sc = torch.zeros(N.ADAM_SCALARS, device="cuda")
    N.adam_advance(sc, 1e-3, 0.9, 0.999, grad_scale)
    return sc


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def mixed(n, seed):
    """fp32 values of both signs with magnitudes from 1e-20 to 1e18 in one buffer."""
    g = np.random.default_rng(seed)
    v = g.uniform(1.0, 10.0, n) * 10.0 ** g.integers(-20, 18, n) * g.choice([-1.0, 1.0], n)
    return v.astype(np.float32)


# ------------------------------------------------------------------------------------------------------ 1. the norm kernel
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2 ** 20 + 3, 16836937])
def test_sum_of_squares_against_the_restatement(n):
    """The relative error of the float64 sum is at most n * 2^-53 -- the bound of ANY order of float64 additions of
    non-negative terms that are exact (squares of fp32 values are): derived, not tuned.  Two calls give the same bits, and so
    does the same data at another offset of a larger allocation, 16-byte aligned or not."""
    host = mixed(n, n)
    want = G.sum_squares(host)
    data = torch.from_numpy(host).cuda()
    sc, ws = scalars(), N.grad_clip_workspace("cuda")
    results = []
    for off, pad in ((0, 0), (0, 0), (64, 96), (65, 128), (3, 7)):      # (offset, slack) in floats
        big = torch.full((off + n + pad,), 3.0e19, device="cuda")       # what surrounds the span must not enter the sum
        big[off:off + n].copy_(data)
        ws.fill_(-1.0)
        N.grad_clip(big[off:off + n], sc, INF, workspace=ws)
        results.append(ws.clone())
    S = float(results[0][-1])
    err = abs(S - want) / want
    print("n=%d: sum of squares %.17g, restatement %.17g, relative error %.3g (bound %.3g)" % (n, S, want, err, n * 2.0 ** -53))
    assert err <= n * 2.0 ** -53
    for r in results[1:]:
        assert torch.equal(r, results[0])                               # every partial and the sum, bit for bit
    assert float(sc[5]) == float(np.float32(math.sqrt(S)))
    assert float(sc[6]) == 1.0 and float(sc[7]) == 0.0


# ----------------------------------------------------------------------------------------------------------- 2. the scalars
def test_scalars_follow_the_restatement_exactly():
    n = 1000
    g = torch.full((n,), 0.5, device="cuda")                 # sum of squares 250, exactly, in any order
    g[::2] *= -1.0
    host = g.cpu().numpy()
    third = float(np.float32(1.0 / 3.0))
    sc = scalars(third)
    clipped = 0
    for step, max_norm in enumerate([3.0, 100.0, 1.0, INF, 5.270462, 0.25]):
        if step:
            N.adam_advance(sc, 1e-3, 0.9, 0.999, third)      # a step's prepare: grad_scale is set afresh
        before = sc.clone()
        N.grad_clip(g, sc, max_norm)
        norm, coef, scale, was = G.clip(host, third, max_norm)
        clipped += was
        got = sc.cpu().numpy()
        assert bits(got[5]) == bits(np.float32(norm)) and bits(got[6]) == bits(np.float32(coef)), (step, got, norm, coef)
        assert bits(got[2]) == bits(scale), (step, got[2], scale)
        assert got[7] == clipped
        assert torch.equal(sc[:2], before[:2]) and torch.equal(sc[3:5], before[3:5])      # nothing else moves
        if max_norm in (100.0, INF):
            assert not was and got[6] == 1.0 and bits(got[2]) == bits(np.float32(third))   # bit-identical grad_scale
    assert clipped == 4                                      # (5.270462 is just below the norm: a coefficient of 1 - 1.6e-7)
    # a non-zero skip word: only the norm is written
    skip = torch.ones(1, device="cuda")
    N.adam_advance(sc, 1e-3, 0.9, 0.999, 0.5)
    sc[6] = 0.125
    N.grad_clip(g, sc, 0.25, skip=skip)
    got = sc.cpu().numpy()
    assert got[2] == 0.5 and got[7] == clipped and got[6] == 1.0 and bits(got[5]) == bits(np.float32(math.sqrt(250.0) * 0.5))
    skip.zero_()
    N.grad_clip(g, sc, 0.25, skip=skip)                      # a zero skip word clips
    assert float(sc[7]) == clipped + 1 and float(sc[2]) < 0.5
    # non-finite buffers: torch's arithmetic
    for bad, check in ((INF, lambda c: c == 0.0), (float("nan"), math.isnan)):
        h = g.clone()
        h[17] = bad
        sc = scalars(1.0)
        N.grad_clip(h, sc, 2.0)
        got = sc.cpu().numpy()
        norm, coef, scale, was = G.clip(h.cpu().numpy(), 1.0, 2.0)
        assert check(float(got[6])) and check(coef) and check(float(got[2])) and got[7] == float(was), (bad, got)
        assert (math.isnan(norm) and math.isnan(got[5])) or got[5] == np.float32(norm)
    with pytest.raises(RuntimeError, match="max_norm"):
        N.grad_clip(g, sc, 0.0)


# ----------------------------------------------------------------------------------------------------- 3. simulated ranks
def test_buffer_summed_over_four_ranks_gives_the_mean_gradients_norm():
    W, n = 4, 5003
    gen = torch.Generator().manual_seed(3)
    shards = [torch.randn(n, generator=gen) * (1.0 + r) for r in range(W)]
    total = shards[0].clone()
    for s in shards[1:]:
        total += s                                           # what the all-reduce(sum) leaves in the flat buffer
    mean = total.double() / W                                # exact: a power of two
    p = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
    p.grad = mean.clone()
    c = 0.5 * float(mean.norm())
    want_norm = float(torch.nn.utils.clip_grad_norm_([p], c))
    want_coef = float(p.grad[0] / mean[0]) if float(mean[0]) != 0.0 else None
    sc = scalars(1.0 / W)
    N.grad_clip(total.cuda(), sc, c)
    norm, coef, scale, was = G.clip(total.numpy(), 1.0 / W, c)
    got = sc.cpu().numpy()
    assert was and bits(got[5]) == bits(np.float32(norm)) and bits(got[6]) == bits(np.float32(coef)) and bits(got[2]) == bits(scale)
    assert abs(norm - want_norm) <= 1e-14 * want_norm and abs(got[5] - want_norm) <= 2.0 ** -23 * want_norm
    assert want_coef is not None and abs(coef - want_coef) <= 1e-12 and abs(got[6] - want_coef) <= 2.0 ** -23
    assert abs(float(got[2]) - want_coef / W) <= 2.0 ** -23 / W      # the factor Adam applies: coef / world


# ---------------------------------------------------------------------------------- the oracle loop with clip_grad_norm_
def tiny_model(seed=7, use_jitter=True, **kw):
    torch.manual_seed(seed)
    m = ConvolutionalVQVAE(*CFG, use_jitter=use_jitter, **kw).cuda().train()
    with torch.no_grad():
        m._vq._embedding.weight.normal_(0, 0.7)
    return m


def oracle_params(m, dtype=torch.float32):
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in m.state_dict().items()
            if "_layers." not in k or "_layers.0." in k}


def oracle_speech_loop(p, raws, max_norm, seeds, use_jitter=True, lr=1e-3):
    """scripts/train_speech.py:62-74,88-91 as tests/test_script_loop_gpu.py restates it, with clip_grad_norm_ between
    backward and Adam.step.  Returns [(loss, recon_error, perplexity)], [norm before clipping]."""
    params = list(p.values())
    opt = torch.optim.Adam(params, lr=lr, amsgrad=False)
    log, norms = [], []
    for raw, seed in zip(raws, seeds):
        np.random.seed(seed)
        x = O.speech_preprocess(raw.to(params[0].dtype))
        opt.zero_grad()
        src = O.jitter_source_index(x.shape[2], 0.25) if use_jitter else None
        out = O.vqvae_forward(x, p, CFG[3], CFG[5], src)
        recon_error = F.mse_loss(out["recon"], x, reduction="mean")
        loss = recon_error + out["vq_loss"]
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
        log.append((float(loss), float(recon_error), float(out["perplexity"])))
    return log, norms


def raw_batches(k, seed0=40):
    return [torch.randn(4, 20, 40, generator=torch.Generator().manual_seed(seed0 + s)) for s in range(k)]


# ------------------------------------------------------------------------------------ 4. exactness of the clipped step
def test_clipped_step_is_the_unclipped_step_with_the_scaled_factor_bitwise():
    """One Trainer(max_grad_norm=c) step against a twin from the same initial state on the same batch that runs UNCLIPPED with
    its grad_scale replaced by the scalars[2] the first one computed: parameters and both moments bit for bit.  c is half the
    float64 oracle's own first-step norm, and the oracle's coefficient is asserted < 1, so the step compared is a clipped one."""
    raw = raw_batches(1)[0]
    ref = tiny_model()
    _, norms64 = oracle_speech_loop(oracle_params(ref, torch.float64), [raw], INF, [5])
    c = 0.5 * norms64[0]
    assert c / (norms64[0] + 1e-6) < 1.0
    ta, tb, tc = (Trainer(tiny_model(), "speech", range_check_every=0, **kw) for kw in (dict(max_grad_norm=c), {}, {}))
    assert torch.equal(ta.buffers.flat, tb.buffers.flat)
    np.random.seed(5)
    ta.step(raw.cuda())
    norm, coef = ta.grad_norm()
    factor = ta.opt.scalars[2].item()
    print("oracle float64 norm %.9g, device norm %.9g, coef %.9g, grad_scale used %.9g" % (norms64[0], norm, coef, factor))
    assert coef < 1.0 and ta.clipped_steps(reset=False) == 1 and abs(norm - norms64[0]) <= 1e-3 * norms64[0]
    assert bits(factor) == bits(np.float32(coef)) and abs(coef - 0.5) < 1e-3
    tb.grad_scale = factor                                   # a Python float holds the fp32 value exactly
    np.random.seed(5)
    tb.step(raw.cuda())
    np.random.seed(5)
    tc.step(raw.cuda())                                      # the plain unclipped step: must differ, or nothing was shown
    torch.cuda.synchronize()
    assert torch.equal(ta.buffers.flat, tb.buffers.flat)
    assert torch.equal(ta.opt.exp_avg, tb.opt.exp_avg) and torch.equal(ta.opt.exp_avg_sq, tb.opt.exp_avg_sq)
    assert not torch.equal(ta.opt.exp_avg, tc.opt.exp_avg) and not torch.equal(ta.opt.exp_avg_sq, tc.opt.exp_avg_sq)


def test_a_bound_never_reached_is_the_default_trainer_bitwise():
    raws = raw_batches(4)
    ta, tb = Trainer(tiny_model(), "speech", range_check_every=0, max_grad_norm=1e9), Trainer(tiny_model(), "speech", range_check_every=0)
    for s, raw in enumerate(raws):
        for tr in (ta, tb):
            np.random.seed(100 + s)
            tr.step(raw.cuda())
        assert ta.grad_norm()[1] == 1.0
    torch.cuda.synchronize()
    assert torch.equal(ta.buffers.flat, tb.buffers.flat)
    assert torch.equal(ta.opt.exp_avg, tb.opt.exp_avg) and torch.equal(ta.opt.exp_avg_sq, tb.opt.exp_avg_sq)
    assert ta.clipped_steps() == 0 and 0.0 < ta.grad_norm()[0] < 1e9


# ------------------------------------------------------------------------------------------------------- 5. against torch
def _norm_margin(n32, n64):
    """1e-3 relative, unless the oracle's own float32-versus-float64 gap on the batch is wider: then 4x that gap."""
    gap = abs(n32 - n64) / n64
    return gap, (1e-3 if gap <= 1e-3 else 4.0 * gap)


def test_speech_trainer_tracks_the_oracle_loop_with_clip_grad_norm():
    """4 steps of the CPU oracle loop with clip_grad_norm_ between backward and Adam.step against Trainer(max_grad_norm=c), f32
    mode: the loss curve to the 2e-4 tests/test_script_loop_gpu.py holds the unclipped f32 loop to, the reported norm of
    step 0 within 1e-3 of the oracle's.  Measured on an MI355X: the oracle's own float32 norm against its float64 norm on this
    batch differs by 3.6e-8 (inside the margin, which therefore stays 1e-3); the device's norm equals the float32 oracle's to
    the nine digits printed; the oracle's coefficients are 0.5, 0.755, 1, 1 (the first two steps are clipped ones) and the
    device's agree to the four digits printed; the worst loss-curve difference is 2.5e-6 relative."""
    steps, tol = 4, 2e-4
    shapes = O.vqvae_param_shapes(20, 48, 8, 24, 64)
    p0 = O.closed_form_params(shapes, 0.8)
    raws = [torch.from_numpy(O.hashed_uniform(3 * 20 * 33, 50 + i, 2.0).reshape(3, 20, 33)) for i in range(steps)]
    seeds = [11 + i for i in range(steps)]
    p64 = {k: v.double().clone().requires_grad_(True) for k, v in p0.items()}
    _, norms64 = oracle_speech_loop(p64, raws[:1], INF, seeds[:1])
    c = 0.5 * norms64[0]
    p32 = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    want, norms32 = oracle_speech_loop(p32, raws, c, seeds)
    assert all(c / (n + 1e-6) < 1.0 for n in norms32[:1])
    gap, margin = _norm_margin(norms32[0], norms64[0])
    m = ConvolutionalVQVAE(*CFG)
    m.load_state_dict({k.replace("_layers.0.", "_layers.%d." % r): v for k, v in p0.items() for r in
                       (range(CFG[3]) if "_layers.0." in k else [0])})
    tr = Trainer(m.cuda().train(), "speech", range_check_every=0, max_grad_norm=c)
    got, norms = [], []
    for raw, seed in zip(raws, seeds):
        np.random.seed(seed)
        out = tr.step(raw.cuda())
        got.append(tuple(float(v) for v in out))
        norms.append(tr.grad_norm())
    worst = max(abs(a - b) / max(abs(b), 1e-3) for g, w in zip(got, want) for a, b in zip(g, w))
    print("oracle f32-vs-f64 norm gap %.3g (margin %.3g); device norm %.9g, oracle %.9g (rel %.3g); oracle coefs %s, device coefs %s; "
          "worst loss-curve difference %.3g" % (gap, margin, norms[0][0], norms32[0], abs(norms[0][0] - norms32[0]) / norms32[0],
                                                [round(min(1.0, c / (n + 1e-6)), 4) for n in norms32], [round(k, 4) for _, k in norms], worst))
    assert abs(norms[0][0] - norms32[0]) <= margin * norms32[0]
    assert norms[0][1] < 1.0 and tr.clipped_steps(reset=False) >= 1
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert abs(a - b) <= tol * max(abs(b), 1e-3), (got, want)


def test_location_trainer_tracks_the_oracle_loop_with_clip_grad_norm():
    """The setup of tests/test_location_gpu.py::test_location_trainer_flat_adam_tracks_oracle with clip_grad_norm_ in the oracle
    loop and LocationTrainer(max_grad_norm=c): the same loss curve to that test's tolerance, the norm of step 0 within 1e-3.
    Measured on an MI355X: the oracle's float32 norm against its float64 norm differs by 5.3e-6 (the margin stays 1e-3), the
    device's norm by 5.1e-6 from the float32 oracle's; all four steps are clipped (coefficients 0.5, 0.68, 0.75, 0.72)."""
    L, K, od, B = 21, 32, 1, 8
    p = LO.closed_form_location_params(LO.location_param_shapes(L, K, od), gain=3.0)

    def batch(step):
        return LO.hashed_indices(B, L, K, 40 + step), torch.from_numpy(O.hashed_uniform(B, 50 + step, 3.0))

    idx, theta = batch(0)
    p64 = {k: v.double().clone().requires_grad_(True) for k, v in p.items()}
    loss64 = F.mse_loss(LO.location_forward(LO.onehot_codes(idx, K).double(), p64), theta.double() / math.pi)
    loss64.backward()
    n64 = math.sqrt(sum(float(v.grad.square().sum()) for v in p64.values()))
    c = 0.5 * n64
    from acoustic_locating_vq_vae.vq_vae.location_model.location_model import LocationModule
    m = LocationModule(L, K, od)
    m.load_state_dict(p)
    tr = LocationTrainer(m.cuda().train(), lr=1e-3, max_grad_norm=c)
    po = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    opt_o = torch.optim.Adam(list(po.values()), lr=1e-3)
    for step in range(4):
        idx, theta = batch(step)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            opt_o.zero_grad()
            want = LO.location_loss(LO.location_forward(LO.onehot_codes(idx, K), po), theta)
            want.backward()
            n32 = float(torch.nn.utils.clip_grad_norm_(list(po.values()), c))
            opt_o.step()
            got = tr.step(torch.from_numpy(idx).cuda(), theta)
        norm, coef = tr.grad_norm()
        print("step %d: loss %.9g (oracle %.9g), norm %.9g (oracle %.9g), coef %.6g" % (step, float(got), float(want), norm, n32, coef))
        assert abs(float(got) - float(want)) < 1e-4 * abs(float(want)) + 1e-7, (step, float(got), float(want))
        if step == 0:
            gap, margin = _norm_margin(n32, n64)
            print("oracle f32-vs-f64 norm gap %.3g (margin %.3g), device-vs-oracle %.3g" % (gap, margin, abs(norm - n32) / n32))
            assert c / (n32 + 1e-6) < 1.0 and coef < 1.0
            assert abs(norm - n32) <= margin * n32
    assert tr.clipped_steps() >= 1


# ------------------------------------------------------------------------------------------------ 6. the EMA span excluded
def test_ema_statistics_and_restart_candidates_stay_out_of_the_norm():
    m = tiny_model(use_jitter=False, decay=0.99, dead_code_threshold=1.0, restart_candidates=16)
    tr = Trainer(m, "speech", range_check_every=0, max_grad_norm=INF)
    lo, hi = tr.buffers.extra_span
    assert hi > lo
    tr.step(raw_batches(1)[0].cuda())
    torch.cuda.synchronize()
    want = math.sqrt(sum(float(p.grad.double().square().sum()) for p in tr.buffers.params))
    leaked = float(tr.buffers.grad[_ALIGN:].double().norm())
    norm, coef = tr.grad_norm()
    print("norm of the p.grad tensors %.9g, reported %.9g, with the statistics span %.9g" % (want, norm, leaked))
    assert want > 0.0 and leaked > 2.0 * want                # the span (counts of order N) would dominate had it leaked in
    assert abs(norm - want) <= 2.0 ** -23 * want and coef == 1.0
    # padding between parameters is zero: the span [_ALIGN, extra_span[0]) holds exactly the p.grad tensors
    assert abs(float(tr.buffers.grad[_ALIGN:lo].double().norm()) - want) <= 1e-12 * want


# ----------------------------------------------------------------------------------------------------------- 7. graph replay
def test_captured_and_eager_trainers_agree_bitwise_with_clipping_and_schedule():
    raws = [r.cuda() for r in raw_batches(7)]
    ref = Trainer(tiny_model(use_jitter=False), "speech", range_check_every=0, max_grad_norm=INF)
    ref.step(raws[1])
    c = 0.7 * ref.grad_norm()[0]
    ta, tb = (Trainer(tiny_model(use_jitter=False), "speech", range_check_every=0, max_grad_norm=c, lr_schedule=WarmupCosine(3, 8))
              for _ in range(2))
    ta.step(raws[0])
    tb.capture(raws[0], warmup=1)               # one real step on the same batch, then the capture
    coefs = []
    for r in raws[1:]:
        ta.step(r)
        tb.step(r)
        coefs.append((ta.grad_norm(), tb.grad_norm()))
    torch.cuda.synchronize()
    assert tb._graph is not None and all(a == b for a, b in coefs)
    assert torch.equal(ta.buffers.flat, tb.buffers.flat)
    assert torch.equal(ta.opt.exp_avg, tb.opt.exp_avg) and torch.equal(ta.opt.exp_avg_sq, tb.opt.exp_avg_sq)
    assert torch.equal(ta.opt.scalars, tb.opt.scalars) and float(ta.opt.scalars[3]) == 7.0
    assert ta.clipped_steps(reset=False) == tb.clipped_steps(reset=False) >= 1
    # the schedule ran: step 7 of WarmupCosine(3, 8) is past the peak
    lr7 = float(ta.opt.scalars[0]) * (1 - 0.9 ** 7)
    assert abs(lr7 - G.scheduled_lr(7, 1e-3, 3, 8)) <= 1e-9 and lr7 < 0.5e-3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("buckets", [1, 2])
def test_graph_replay_with_a_forced_one_rank_collective(buckets):
    """The same comparison in a child process with a one-rank RCCL group and force_collective=True: the clip sits between the
    all-reduce wait(s) and the Adam launch, outside the graphs."""
    env = dict(os.environ)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0", RANK="0", WORLD_SIZE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "grad_clip_world1.py"), "0.05", str(buckets)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith("GRAD_CLIP_WORLD1 ")][-1][len("GRAD_CLIP_WORLD1 "):])
    print(json.dumps(r))
    assert r["backend"] == "nccl" and r["world"] == 1 and r["captured"] and r["finite"]
    assert r["allreduce_calls_per_step"] == [buckets, buckets]
    assert r["params_bit_identical"] and r["moments_bit_identical"] and r["scalars_bit_identical"] and r["norms_equal"]
    assert r["clipped_steps"][0] == r["clipped_steps"][1] >= 1 and min(r["coefs"]) < 1.0 and r["applied_steps"] == 7.0


# ------------------------------------------------------------------------------------------------------------ 8. the schedule
def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def test_schedule_rates_skipped_steps_and_resume():
    lr, b1, warmup, total, lr_min = 2e-3, 0.9, 4, 10, 1e-5
    w = torch.nn.Parameter(torch.zeros(100, device="cuda"))
    opt = FlatAdam(FlatBuffers([w]), lr=lr, betas=(b1, 0.999), guard=True, schedule=WarmupCosine(warmup, total, lr_min))
    for t in range(1, 13):
        opt.prepare(0.5)
        sc = opt.scalars.cpu().numpy()
        want = G.scheduled_lr(t, lr, warmup, total, lr_min)
        got = float(np.float64(sc[0]) * (1.0 - b1 ** t))
        assert abs(got - want) <= 2 * ulp32(want), (t, got, want)
        assert sc[3] == t and sc[2] == 0.5 and abs(float(sc[1]) - math.sqrt(1 - 0.999 ** t)) <= ulp32(sc[1])
        # next to the unscheduled entry point: the same state but for the rate
        plain = torch.zeros(N.ADAM_SCALARS, device="cuda")
        plain[3] = t - 1
        N.adam_advance(plain, want, b1, 0.999, 0.5)
        assert abs(float(plain[0]) - float(sc[0])) <= 2 * ulp32(float(sc[0])) and torch.equal(plain[1:5].cpu(), torch.from_numpy(sc[1:5]))
    assert abs(float(opt.scalars[0]) * (1 - b1 ** 12) - lr_min) <= 2 * ulp32(lr_min)      # past total_steps: lr_min
    # a skipped step does not advance the schedule
    opt = FlatAdam(FlatBuffers([w]), lr=lr, betas=(b1, 0.999), guard=True, schedule=WarmupCosine(warmup, total, lr_min))
    opt.prepare()
    opt.prepare()
    at2 = opt.scalars.clone()
    opt.b.skip_slot.fill_(1.0)                               # step 2's verdict: saturated
    opt.prepare()                                            # the retry carries the same number and the same rate
    assert torch.equal(opt.scalars[:4], at2[:4]) and float(opt.scalars[4]) == 1.0
    opt.b.skip_slot.zero_()
    opt.prepare()
    assert float(opt.scalars[3]) == 3.0
    assert abs(float(opt.scalars[0]) * (1 - b1 ** 3) - lr * 3 / 4) <= 2 * ulp32(lr * 3 / 4)
    # warm-up only (no total): the rate stays at lr
    opt = FlatAdam(FlatBuffers([w]), lr=lr, betas=(b1, 0.999), schedule=WarmupCosine(2))
    for t in range(1, 6):
        opt.prepare()
        want = lr * min(t, 2) / 2
        assert abs(float(opt.scalars[0]) * (1 - b1 ** t) - want) <= 2 * ulp32(want)


def test_a_resumed_trainer_lands_on_the_same_rate_and_parameters(tmp_path):
    raws = [r.cuda() for r in raw_batches(5)]
    sched = dict(max_grad_norm=0.05, lr_schedule=WarmupCosine(3, 8, 1e-5))
    full = Trainer(tiny_model(use_jitter=False), "speech", range_check_every=0, **sched)
    for r in raws:
        full.step(r)
    first = Trainer(tiny_model(use_jitter=False), "speech", range_check_every=0, **sched)
    for r in raws[:3]:
        first.step(r)
    state = first.state_dict()
    assert sorted(state) == ["exp_avg", "exp_avg_sq", "kind", "model", "numel", "step"]     # nothing new is saved
    path = str(tmp_path / "trainer.pt")
    torch.save(state, path)
    resumed = Trainer(tiny_model(seed=8, use_jitter=False), "speech", range_check_every=0, **sched)
    resumed.load_state_dict(torch.load(path))
    for r in raws[3:]:
        resumed.step(r)
    torch.cuda.synchronize()
    assert torch.equal(resumed.opt.scalars[:4], full.opt.scalars[:4]) and float(full.opt.scalars[3]) == 5.0
    lr5 = float(full.opt.scalars[0]) * (1 - 0.9 ** 5)
    assert abs(lr5 - G.scheduled_lr(5, 1e-3, 3, 8, 1e-5)) <= 2 * ulp32(lr5)
    assert torch.equal(resumed.buffers.flat, full.buffers.flat) and torch.equal(resumed.opt.exp_avg_sq, full.opt.exp_avg_sq)
