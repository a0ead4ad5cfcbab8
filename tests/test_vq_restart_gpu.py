"""Dead-code restarts of VectorQuantizerEMA on the device (csrc/vq_restart.hip: alvq_vq_restart_gather_f32 /
alvq_vq_restart_dead_f32): the kernels against the fp32 restatement tests/helpers/vq_restart_ref.py bit for bit, the gather's
slot patterns and its bounds guard, the module's training forwards step by step, the cases that must restart nothing, the
planted collapse through the real quantiser, and the Trainer (eager against graph replay, the fp16-range skip guard,
checkpoints, run-to-run identity, two gloo ranks)."""
import io
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import vq_ema_ref as E_  # noqa: E402
import vq_restart_ref as R  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import _ops  # noqa: E402
from acoustic_locating_vq_vae.train_step import Trainer  # noqa: E402
from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE  # noqa: E402
from acoustic_locating_vq_vae.vq_vae.vector_quantizer import VectorQuantizerEMA  # noqa: E402

SPEECH = (201, 1024, 128, 3, 1024, 0.25, 1024)
SMALL = (40, 64, 16, 2, 32, 0.25, 64)
DECAY, EPS = 0.99, 1e-5


@pytest.fixture(params=["x3mx_hb", "f32"])
def mode(request):
    _ops.set_compute_dtype(request.param)
    yield request.param
    _ops.set_compute_dtype("f32")


def state(vq):
    return [t.detach().clone() for t in (vq._ema_cluster_size, vq._ema_w, vq._embedding.weight)]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def close(dev, ref, rtol=1e-5):
    """The tolerance tests/test_vq_ema_gpu.py uses for the EMA update: |dev - ref| <= rtol |ref| + 0.1 rtol max |ref[row]|."""
    d = dev.detach().double().cpu().numpy()
    r = np.asarray(ref, dtype=np.float64)
    scale = np.abs(r).max(axis=-1, keepdims=True) if r.ndim > 1 else np.abs(r).max()
    bad = np.abs(d - r) > rtol * np.abs(r) + 0.1 * rtol * scale
    assert not bad.any(), (int(bad.sum()), float(np.abs(d - r).max()))


# ------------------------------------------------------------------------------------------------------- the kernels
def kernel_case(K, D, R_, n_dead, thr, seed, skip=None):
    """Random state with ``n_dead`` codes below ``thr`` (zeros, denormal-sized and just-below values among them) and a few
    alive ones exactly AT the threshold; the device against restart32, bit for bit, counters included."""
    g = np.random.default_rng(seed)
    thr32 = np.float32(thr)
    cs = g.uniform(2.0, 50.0, size=K).astype(np.float32) * thr32
    at = g.choice(K, size=min(K, 3), replace=False)
    cs[at] = thr32                                           # cs == threshold is alive
    dead = np.sort(g.choice(K, size=n_dead, replace=False))
    low = (g.uniform(0.0, 1.0, size=n_dead).astype(np.float32) * thr32).astype(np.float32)
    low[low >= thr32] = 0.0
    low[::3] = 0.0
    if n_dead > 1:
        low[1] = np.nextafter(thr32, np.float32(0.0))
    cs[dead] = low
    W = g.normal(size=(K, D)).astype(np.float32)
    E = g.normal(size=(K, D)).astype(np.float32)
    cand = g.normal(size=(R_, D)).astype(np.float32)
    d_cs, d_W, d_E, d_cand = (torch.from_numpy(a).cuda() for a in (cs, W, E, cand))
    counters = torch.tensor([5, 9], dtype=torch.int64, device="cuda")
    slot = None if skip is None else torch.tensor([skip], dtype=torch.float32, device="cuda")
    N.vq_restart_dead(d_cand, d_cs, d_W, d_E, counters, thr, skip=slot)
    torch.cuda.synchronize()
    if skip:
        want = (cs, W, E, 0, 9)
    else:
        want = R.restart32(cs, W, E, cand, thr)
        assert want[4] == n_dead and want[3] == min(n_dead, R_)
    assert torch.equal(d_cs.cpu(), torch.from_numpy(want[0])), (K, D, R_, n_dead)
    assert torch.equal(d_W.cpu(), torch.from_numpy(want[1])), (K, D, R_, n_dead)
    assert torch.equal(d_E.cpu(), torch.from_numpy(want[2])), (K, D, R_, n_dead)
    assert counters.tolist() == [5 + want[3], want[4]], (K, D, R_, n_dead, counters.tolist())
    if not skip and n_dead:                                   # the lowest min(n_dead, R) dead codes, on their candidates
        k = dead[:min(n_dead, R_)]
        assert np.array_equal(d_E.cpu().numpy()[k], cand[:len(k)])


@pytest.mark.parametrize("K,D,R_", [(64, 16, 16), (1024, 128, 64), (1000, 50, 7), (1, 4, 1), (16384, 8, 64), (16384, 8, 16384),
                                    (2500, 512, 300), (130, 3, 130)])
def test_restart_kernel_is_the_fp32_restatement_bitwise(K, D, R_):
    counts = sorted({0, 1, max(R_ - 1, 0), R_, min(K, R_ + 1), min(K, R_ + 37), K})      # none, below, at, above the cap, all
    for i, n_dead in enumerate(c for c in counts if c <= K):
        kernel_case(K, D, R_, n_dead, 1.0, 100 * i + K)
    kernel_case(K, D, R_, min(K, R_), 0.7, 7)                # a threshold that fp32 rounds
    kernel_case(K, D, R_, K, 2.5e-3, 8)


def test_restart_kernel_skip_slot_leaves_everything():
    for K, D, R_ in ((64, 16, 16), (1000, 50, 7)):
        kernel_case(K, D, R_, K // 2, 1.0, 3, skip=1.0)      # non-zero: nothing moves, the counters neither
        kernel_case(K, D, R_, K // 2, 1.0, 3, skip=2.0)
        kernel_case(K, D, R_, K // 2, 1.0, 3, skip=0.0)      # a zero slot is no skip


@pytest.mark.parametrize("D,offset", [(128, 0), (50, 0), (16, 0), (16, 1), (3, 0), (512, 0)])
def test_gather_slot_patterns(D, offset):
    """first / stride as ranks 0..W-1 of W = 1, 2, 4 use them: a rank writes its slots from its own positions, in draw order,
    and leaves every other slot alone.  offset = 1: x starts 4 bytes off a 16-byte boundary (the scalar path at D % 4 == 0)."""
    n, R_ = 777, 13
    g = torch.Generator(device="cuda").manual_seed(D)
    base = torch.randn(n * D + 4, device="cuda", generator=g)
    x = base[offset:offset + n * D].view(n, D)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for W in (1, 2, 4):
        full = torch.full((R_, D), -7.0, device="cuda")
        want = torch.full((R_, D), -7.0, device="cuda")
        for r in range(W):
            slots = list(range(r, R_, W))
            rows = torch.randperm(n, generator=torch.Generator().manual_seed(10 * W + r))[:len(slots)].cuda()
            alone = torch.full((R_, D), -7.0, device="cuda")
            N.vq_restart_gather(x, rows, alone, status, first=r, stride=W)
            N.vq_restart_gather(x, rows, full, status, first=r, stride=W)
            want[slots] = x[rows]
            mine = torch.full((R_, D), -7.0, device="cuda")
            mine[slots] = x[rows]
            assert torch.equal(alone, mine), (W, r)           # the other slots keep the sentinel
        assert torch.equal(full, want), W
    assert int(status.item()) == 0


def test_gather_rejects_positions_outside_the_rows():
    n, D, R_ = 100, 12, 6
    x = torch.randn(n, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    rows = torch.tensor([3, -1, 99, 100, 1 << 40, 0], dtype=torch.int64, device="cuda")
    cand = torch.full((R_, D), -7.0, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    N.vq_restart_gather(x, rows, cand, status)
    assert int(status.item()) == 1
    assert torch.equal(cand[[0, 2, 5]], x[[3, 99, 0]])
    assert torch.equal(cand[[1, 3, 4]], torch.zeros(3, D, device="cuda"))        # left zero, nothing read out of bounds
    with pytest.raises(RuntimeError, match="positions"):
        N.vq_restart_gather(x, rows[:2], cand, status)                           # too few positions: refused on the host
    vq = VectorQuantizerEMA(8, 4, 0.25, 0.9, dead_code_threshold=1.0, restart_candidates=2).cuda()
    vq._restart_status.fill_(1)
    with pytest.raises(RuntimeError, match="outside"):
        vq.restarted_codes()


# ---------------------------------------------------------------------------------------------------- the module API
def tap(vq):
    """Record the rows and indices of every quantize call (ConvolutionalVQVAE.forward calls the method, not the module)."""
    seen, inner, D = {}, vq.quantize, vq._embedding_dim

    def tapped(z):
        out = inner(z)
        seen["rows"], seen["idx"] = z.detach().reshape(-1, D).clone(), out[3].clone()
        return out
    vq.quantize = tapped
    return seen


def small_model(seed=0, **kw):
    torch.manual_seed(seed)
    return ConvolutionalVQVAE(*SMALL, use_jitter=False, **kw).cuda().train()


def small_batch(s, B=8):
    return torch.randn(B, 40, 60, generator=torch.Generator().manual_seed(300 + s)).cuda() * 2.0


def test_module_five_training_forwards_follow_the_restatement(mode):
    m = small_model(decay=0.9, dead_code_threshold=1.0, restart_candidates=8, restart_seed=4)
    vq, seen = m._vq, tap(m._vq)
    total = 0
    for step in range(5):
        cs0, w0, _ = [t.double().cpu().numpy() for t in state(vq)]
        loss, recon, _ = m(small_batch(step))
        (loss + recon.square().mean()).backward()            # the backward still has the codebook the forward quantised with
        torch.cuda.synchronize()
        rows32 = seen["rows"].cpu().numpy()
        pos = vq._restart_rows.cpu().numpy()
        assert len(set(pos.tolist())) == 8 and pos.min() >= 0 and pos.max() < rows32.shape[0]
        cand = rows32[pos]
        cs, w, e, n, dead = R.step(cs0, w0, rows32.astype(np.float64), seen["idx"].cpu().numpy(), 0.9, 1e-5, cand, 1.0)
        close(vq._ema_cluster_size, cs)
        close(vq._ema_w, w)
        close(vq._embedding.weight, e)
        total += n
        assert vq.restarted_codes() == (total, dead), (step, vq.restarted_codes(), total, dead)
        ucs, _, _ = E_.step(cs0, w0, rows32.astype(np.float64), seen["idx"].cpu().numpy(), 0.9, 1e-5)
        k = np.flatnonzero(ucs < 1.0)[:n]
        got = vq._embedding.weight.detach().cpu().numpy()
        assert np.array_equal(got[k], cand[:n])              # restarted rows ARE the candidate rows, bit for bit
        assert np.array_equal(vq._ema_w.detach().cpu().numpy()[k], cand[:n] * np.float32(1.0))
        assert np.array_equal(vq._ema_cluster_size.cpu().numpy()[k], np.ones(n, dtype=np.float32))
    assert total > 0


def test_eval_frozen_and_echoed_restart_nothing(mode):
    from acoustic_locating_vq_vae.vq_vae.echoed_speech_model import EchoedSpeechReconModel
    kw = dict(decay=0.9, dead_code_threshold=1.0, restart_candidates=8)
    m = small_model(1, **kw)
    vq = m._vq
    before, rng = state(vq), vq._restart_gen.get_state()
    m.eval()
    m(small_batch(0))
    m.train()
    vq.set_train_vq(False)
    m(small_batch(1))
    torch.cuda.synchronize()
    assert same(before, state(vq)) and vq.restarted_codes() == (0, 0)
    assert torch.equal(rng, vq._restart_gen.get_state())     # and no draw
    vq.set_train_vq(True)
    m(small_batch(2))
    assert not same(before, state(vq)) and vq.restarted_codes()[0] == 8

    torch.manual_seed(3)
    sp = ConvolutionalVQVAE(201, 64, 32, 2, 32, 0.25, 128, use_jitter=False, **kw)
    rir = ConvolutionalVQVAE(240, 64, 16, 2, 32, 0.25, 128, use_jitter=False, **kw)
    model = EchoedSpeechReconModel(rir, sp, 201, 64, 2, 32, False).cuda().train()
    before = state(sp._vq) + state(rir._vq)
    rngs = [q._restart_gen.get_state() for q in (sp._vq, rir._vq)]
    tr = Trainer(model, "echoed", range_check_every=0)
    assert tr.restarted_codes() == [] and "restart_rng" not in tr.state_dict()
    for s in range(3):
        tr.step(torch.randn(2, 201, 240, generator=torch.Generator().manual_seed(s)).cuda())
    torch.cuda.synchronize()
    assert same(before, state(sp._vq) + state(rir._vq))
    assert sp._vq.restarted_codes() == (0, 0) and rir._vq.restarted_codes() == (0, 0)
    assert all(torch.equal(a, q._restart_gen.get_state()) for a, q in zip(rngs, (sp._vq, rir._vq)))


def test_threshold_zero_is_the_parents_behaviour_bitwise(mode):
    a = small_model(2, decay=0.9)
    b = small_model(2, decay=0.9, dead_code_threshold=0.0, restart_candidates=8, restart_seed=9)
    assert list(a.state_dict()) == list(b.state_dict()) and not b._vq.restarts_enabled()
    for s in range(3):
        la, ra, _ = a(small_batch(s))
        lb, rb, _ = b(small_batch(s))
        assert torch.equal(la, lb) and torch.equal(ra, rb)
    assert same(state(a._vq), state(b._vq))
    ta, tb = Trainer(a, "speech", range_check_every=0), Trainer(b, "speech", range_check_every=0)
    assert ta.buffers.flat.numel() == tb.buffers.flat.numel() and ta.buffers.extra_span == tb.buffers.extra_span
    assert sorted(ta.state_dict()) == sorted(tb.state_dict()) == ["exp_avg", "exp_avg_sq", "kind", "model", "numel", "step"]
    for s in range(3):
        ta.step(small_batch(s))
        tb.step(small_batch(s))
    torch.cuda.synchronize()
    assert same(state(a._vq), state(b._vq)) and torch.equal(ta.buffers.flat, tb.buffers.flat)
    assert tb.restarted_codes() == [(0, 0)]


def test_too_few_rows_is_an_error_before_any_launch():
    vq = VectorQuantizerEMA(64, 16, 0.25, 0.9, dead_code_threshold=1.0, restart_candidates=32).cuda().train()
    before = state(vq)
    with pytest.raises(ValueError, match="rows"):
        vq.quantize(torch.randn(1, 16, 31, device="cuda"))
    torch.cuda.synchronize()
    assert same(before, state(vq))
    vq.quantize(torch.randn(1, 16, 32, device="cuda"))
    assert sorted(vq._restart_rows.tolist()) == list(range(32))


# ---------------------------------------------------------------------------------------------- the planted collapse
def planted_on_device(seed, on):
    p = R.PLANTED
    kw = dict(dead_code_threshold=p["threshold"], restart_candidates=p["R"], restart_seed=seed) if on else {}
    vq = VectorQuantizerEMA(p["K"], p["D"], 0.25, p["decay"], p["eps"], **kw).cuda().train()
    stream = R.planted_stream(seed, on)                      # the same rows as the CPU test's, seed by seed
    E0, W0 = next(stream)
    vq._embedding.weight.data.copy_(torch.from_numpy(E0).float())
    vq._ema_w.data.copy_(torch.from_numpy(W0).float())
    for x, _ in stream:                                      # (the positions are the quantiser's own draws)
        x = torch.from_numpy(x).float().cuda()
        e = vq._embedding.weight.detach().clone()
        idx = vq.quantize(x.view(1, p["N"], p["D"]))[3]
        mse = float((e[idx] - x).square().mean())
        used = int(idx.unique().numel())
    return used, mse, vq.restarted_codes()[0]


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_planted_collapse_through_the_quantiser(seed):
    used_off, mse_off, none = planted_on_device(seed, False)
    used_on, mse_on, total = planted_on_device(seed, True)
    print("seed %d: used %d -> %d, mse %.3f -> %.3f, %d restarts" % (seed, used_off, used_on, mse_off, mse_on, total))
    assert none == 0 and total > 0
    assert used_off <= 40
    assert used_on >= 56
    assert mse_on * 3 <= mse_off


# -------------------------------------------------------------------------------------------------------- the Trainer
RESTART = dict(dead_code_threshold=1.0, restart_candidates=64, restart_seed=1)


def speech_model(seed=0, **kw):
    torch.manual_seed(seed)
    return ConvolutionalVQVAE(*SPEECH, use_jitter=False, decay=DECAY, **dict(RESTART, **kw)).cuda().train()


def raw_batch(s, B=16):
    return torch.randn(B, 201, 500, generator=torch.Generator().manual_seed(1000 + s)).cuda()


@pytest.mark.parametrize("buckets", [1, 2])
def test_trainer_eager_and_graph_replay_agree_bitwise(mode, buckets):
    a, b = speech_model(), speech_model()
    ta = Trainer(a, "speech", grad_buckets=buckets, range_check_every=0)
    tb = Trainer(b, "speech", grad_buckets=buckets, range_check_every=0)
    assert ta.buffers.extra_span[1] - ta.buffers.extra_span[0] == 1024 + 1024 * 128 + 64 * 128
    before = state(a._vq)
    ta.step(raw_batch(0))
    tb.capture(raw_batch(0), warmup=1)          # one real step on the same batch, then the capture
    torch.cuda.synchronize()
    assert same(state(a._vq), state(b._vq)) and not same(before, state(a._vq))
    assert torch.equal(a._vq._restart_rows, b._vq._restart_rows)
    assert ta.restarted_codes() == tb.restarted_codes() and ta.restarted_codes()[0][0] == 64
    for s in range(1, 6):
        ta.step(raw_batch(s))
        tb.step(raw_batch(s))
        assert torch.equal(a._vq._restart_rows, b._vq._restart_rows), s      # the same stream of positions
    torch.cuda.synchronize()
    assert tb._graph is not None
    assert same(state(a._vq), state(b._vq))
    assert torch.equal(ta.buffers.flat, tb.buffers.flat)
    total, dead = ta.restarted_codes()[0]
    assert (total, dead) == tb.restarted_codes()[0] and total > 64 and dead > 0       # restarts went on happening
    # the candidates of the last step are rows of its latent, and the restarted codes sit on them
    pos = a._vq._restart_rows
    assert pos.unique().numel() == 64 and int(pos.min()) >= 0 and int(pos.max()) < 8000
    assert torch.equal(ta._ema_sinks[id(a._vq)].cand, tb._ema_sinks[id(b._vq)].cand)


def test_skip_guard_leaves_state_and_counters_untouched():
    _ops.set_compute_dtype("x3mx_hb")
    try:
        m = speech_model(4)
        tr = Trainer(m, "speech", range_check_every=0)
        tr.step(raw_batch(0))
        N.f16mx_range_flag(reset=True)
        torch.cuda.synchronize()
        before, counters = state(m._vq), tr.restarted_codes()
        assert counters[0][0] == 64
        bad = raw_batch(1)
        bad[1, 3, 5] = float("nan")
        tr.step(bad)
        torch.cuda.synchronize()
        assert float(tr.buffers.skip_slot) == 1.0
        assert same(before, state(m._vq)) and tr.restarted_codes() == counters
        tr.step(raw_batch(2))
        torch.cuda.synchronize()
        assert float(tr.buffers.skip_slot) == 0.0
        after = state(m._vq)
        assert not same(before, after) and all(bool(torch.isfinite(t).all()) for t in after)
        assert tr.restarted_codes()[0][0] > 64
        N.f16mx_range_flag(reset=True)
    finally:
        _ops.set_compute_dtype("f32")


def test_checkpoint_resumes_bitwise(mode):
    a = speech_model(5)
    ta = Trainer(a, "speech", range_check_every=0)
    for s in range(3):
        ta.step(raw_batch(s))
    sd = ta.state_dict()
    assert len(sd["restart_rng"]) == 1
    buf = io.BytesIO()
    torch.save(sd, buf)
    ta.step(raw_batch(3))
    torch.cuda.synchronize()
    b = speech_model(6, restart_seed=77)         # another init and another seed: everything must come from the checkpoint
    tb = Trainer(b, "speech", range_check_every=0)
    buf.seek(0)
    tb.load_state_dict(torch.load(buf, weights_only=True))
    tb.step(raw_batch(3))
    torch.cuda.synchronize()
    assert torch.equal(a._vq._restart_rows, b._vq._restart_rows)
    assert same(state(a._vq), state(b._vq))
    assert torch.equal(ta.buffers.flat, tb.buffers.flat)
    assert tb.restarted_codes()[0][0] > 0
    del sd["restart_rng"]
    with pytest.raises(ValueError, match="restart"):
        tb.load_state_dict(sd)


def test_two_runs_are_bitwise_identical(mode):
    runs = []
    for _ in range(2):
        torch.manual_seed(9)
        vq = VectorQuantizerEMA(1024, 128, 0.25, DECAY, EPS, **RESTART).cuda().train()
        g = torch.Generator(device="cuda")
        for s in range(3):
            vq.quantize(torch.randn(16, 128, 500, device="cuda", generator=g.manual_seed(20 + s)) * 1.5)
        m = speech_model(8)
        tr = Trainer(m, "speech", range_check_every=0)
        for s in range(2):
            tr.step(raw_batch(s))
        torch.cuda.synchronize()
        assert vq.restarted_codes()[0] == 192 and tr.restarted_codes()[0][0] == 128
        runs.append(state(vq) + state(m._vq) + [vq._restart_rows.clone(), m._vq._restart_rows.clone()])
    assert same(*runs)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _env():
    env = dict(os.environ)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("ALVQ_WIDE_MIN_TILES", None)
    return env


@pytest.mark.parametrize("run_mode,buckets", [("x3mx_hb", 2), ("f32", 1)])
def test_two_ranks_restart_the_same_codes(tmp_path, run_mode, buckets):
    """Two gloo ranks on one card: rank r offers the slots s % 2 == r from its own rows, the step's all-reduce hands both the same
    7 candidates, and both end on bitwise the same state and counters; each restarted row is a row of the slot's owner."""
    helper = os.path.join(ROOT, "tests", "helpers", "vq_restart_ddp.py")
    out = str(tmp_path / "two.pt")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), helper, run_mode, out, str(buckets), "3"]
    p = subprocess.run(cmd, env=_env(), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r0, r1 = (torch.load("%s.rank%d" % (out, r), weights_only=True) for r in (0, 1))
    for k in ("cs", "w", "e", "counters", "cs0", "w0", "e0", "counts", "sums"):
        assert torch.equal(r0[k], r1[k]), k
    assert bool((r0["cand"] == r1["cand"]).all())            # by value: -0.0 + 0.0 is +0.0
    assert r0["own"].shape == (4, 16) and r1["own"].shape == (3, 16)
    for r, d in ((0, r0), (1, r1)):
        pos = d["positions"]
        assert pos.unique().numel() == pos.numel() and int(pos.min()) >= 0 and int(pos.max()) < int(d["nrows"])
        assert bool((r0["cand"][r::2] == d["own"]).all()), r  # slot s is draw s // 2 of rank s % 2
    assert not torch.equal(r0["positions"][:3], r1["positions"])             # the ranks draw from different seeds
    total, dead = r0["counters"].tolist()
    # the last step: the codes below the threshold after the EMA update of the summed statistics, lowest first
    ucs, _, _ = E_.update_rounded(r0["cs0"].numpy(), r0["w0"].numpy(), r0["counts"].numpy(), r0["sums"].numpy(), 0.9, 1e-5)
    k = np.flatnonzero(ucs < np.float32(1.0))
    assert dead == len(k) and dead > 0 and total >= min(dead, 7)
    k = k[:7]
    assert torch.equal(r0["e"][k], r0["cand"][:len(k)])
    assert torch.equal(r0["cs"][k], torch.ones(len(k)))
