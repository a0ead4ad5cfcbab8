"""VectorQuantizerEMA on the device (csrc/kmeans.hip: alvq_vq_ema_stats_f32 / alvq_vq_ema_update_f32) against the float64
restatement tests/helpers/vq_ema_ref.py, in the default mode (x3mx_hb) and f32 -- the quantiser itself is fp32 in every mode:
the module's five consecutive training forwards, its gradient (pre-update codebook, no codebook gradient), the frozen cases,
the Trainer (eager and graph replay, one and two gradient buckets, the fp16-range skip guard, checkpoints, two gloo ranks)
and init_codebook."""
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
import vq_ema_ref as R  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402
from acoustic_locating_vq_vae import _ops  # noqa: E402
from acoustic_locating_vq_vae.train_step import Trainer  # noqa: E402
from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE  # noqa: E402
from acoustic_locating_vq_vae.vq_vae.vector_quantizer import VectorQuantizerEMA  # noqa: E402

SPEECH = (201, 1024, 128, 3, 1024, 0.25, 1024)
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
    """|dev - ref| <= rtol |ref| + 0.1 rtol max |ref[row]|: relative, with a floor at a tenth of rtol of each row's scale (an
    entry that cancels to near zero inherits the rounding of the terms it came from)."""
    d = dev.detach().double().cpu().numpy()
    r = np.asarray(ref, dtype=np.float64)
    scale = np.abs(r).max(axis=-1, keepdims=True) if r.ndim > 1 else np.abs(r).max()
    bad = np.abs(d - r) > rtol * np.abs(r) + 0.1 * rtol * scale
    assert not bad.any(), (int(bad.sum()), float(np.abs(d - r).max()))


def latent(B=16, seed=0):
    """(B, 128, 500): 500 B rows of D = 128 at the speech shape, spread over the unit-normal codebook."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(B, 128, 500, device="cuda", generator=g) * 1.5).contiguous()


def test_module_five_training_forwards_follow_the_restatement(mode):
    torch.manual_seed(0)
    vq = VectorQuantizerEMA(1024, 128, 0.25, DECAY, EPS).cuda().train()
    for step in range(5):
        z = latent(seed=step)
        cs0, w0, e0 = [t.double().cpu().numpy() for t in state(vq)]
        loss, q_st, perp, idx = vq.quantize(z)
        torch.cuda.synchronize()
        rows = z.view(-1, 128).double().cpu().numpy()
        ix = idx.cpu().numpy()
        assert rows.shape[0] == 8000
        cs, w, e = R.step(cs0, w0, rows, ix, DECAY, EPS)
        close(vq._ema_cluster_size, cs)
        close(vq._ema_w, w)
        close(vq._embedding.weight, e)
        rl, rp, q = R.forward(rows, e0, ix, 0.25)
        close(loss, rl)
        close(perp, rp)
        close(q_st.view(-1, 128), q)
    # the indices are those of the codebook the forward had: the argmin against e0 on the device
    assert torch.equal(idx, N.vq_argmin(z.view(-1, 128), torch.from_numpy(e0).float().cuda()))


def test_gradient_uses_the_pre_update_codebook(mode):
    torch.manual_seed(1)
    vq = VectorQuantizerEMA(1024, 128, 0.25, DECAY, EPS).cuda().train()
    z = latent(seed=7).requires_grad_(True)
    e_old = vq._embedding.weight.detach().clone()
    loss, q_st, _, idx = vq.quantize(z)
    g = torch.randn(q_st.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    (loss + (q_st * g).sum()).backward()
    assert vq._embedding.weight.grad is None and vq._ema_w.grad is None
    e_new = vq._embedding.weight.detach()
    assert float((e_new - e_old).abs().max()) > 1.0          # the update moved the codebook far
    rows = z.detach().view(-1, 128).double().cpu().numpy()
    ix = idx.cpu().numpy()
    ref = R.grad_rows(rows, e_old.double().cpu().numpy(), ix, 0.25, g.view(-1, 128).double().cpu().numpy())
    close(z.grad.view(-1, 128), ref)


def test_eval_and_frozen_change_nothing(mode):
    torch.manual_seed(2)
    vq = VectorQuantizerEMA(1024, 128, 0.25, DECAY, EPS).cuda()
    before = state(vq)
    vq.eval()
    out = vq(latent(seed=1))
    vq.train()
    vq.set_train_vq(False)
    vq.quantize(latent(seed=2))
    torch.cuda.synchronize()
    assert same(before, state(vq)) and out[3].shape == (8000, 1024)
    vq.set_train_vq(True)
    vq.quantize(latent(seed=3))
    assert not same(before, state(vq))


def test_echoed_model_leaves_ema_sub_codebooks_frozen(mode):
    from acoustic_locating_vq_vae.vq_vae.echoed_speech_model import EchoedSpeechReconModel
    torch.manual_seed(3)
    sp = ConvolutionalVQVAE(201, 64, 32, 2, 32, 0.25, 128, use_jitter=False, decay=DECAY)
    rir = ConvolutionalVQVAE(240, 64, 16, 2, 32, 0.25, 128, use_jitter=False, decay=DECAY)   # frames are its channels
    model = EchoedSpeechReconModel(rir, sp, 201, 64, 2, 32, False).cuda().train()
    before = state(sp._vq) + state(rir._vq)
    tr = Trainer(model, "echoed", range_check_every=0)
    for s in range(3):
        raw = torch.randn(2, 201, 240, generator=torch.Generator().manual_seed(s)).cuda()
        tr.step(raw)
    torch.cuda.synchronize()
    assert same(before, state(sp._vq) + state(rir._vq))


def speech_model(seed=0, decay=DECAY):
    torch.manual_seed(seed)
    return ConvolutionalVQVAE(*SPEECH, use_jitter=False, decay=decay).cuda().train()


def raw_batch(s, B=16):
    return torch.randn(B, 201, 500, generator=torch.Generator().manual_seed(1000 + s)).cuda()


@pytest.mark.parametrize("buckets", [1, 2])
def test_trainer_eager_and_graph_replay_agree_bitwise(mode, buckets):
    a, b = speech_model(), speech_model()
    ta = Trainer(a, "speech", grad_buckets=buckets, range_check_every=0)
    tb = Trainer(b, "speech", grad_buckets=buckets, range_check_every=0)
    before = state(a._vq)
    if mode == "f32":                           # the first step's update is the restatement's on model._latent(x)'s rows
        with torch.no_grad():
            z = a._latent(ta.preprocess(raw_batch(0))[0])
            rows = z.reshape(-1, 128)
            idx = N.vq_argmin(rows, a._vq._embedding.weight)
            rows, ix = rows.double().cpu().numpy(), idx.cpu().numpy()
        cs0, w0, _ = [t.double().cpu().numpy() for t in before]
    ta.step(raw_batch(0))
    tb.capture(raw_batch(0), warmup=1)          # one real step on the same batch, then the capture
    torch.cuda.synchronize()
    assert same(state(a._vq), state(b._vq)) and not same(before, state(a._vq))
    if mode == "f32":
        cs, w, e = R.step(cs0, w0, rows, ix, DECAY, EPS)
        close(a._vq._ema_cluster_size, cs)
        close(a._vq._ema_w, w)
        close(a._vq._embedding.weight, e)
    for s in range(1, 6):
        ta.step(raw_batch(s))
        tb.step(raw_batch(s))
    torch.cuda.synchronize()
    assert tb._graph is not None
    assert same(state(a._vq), state(b._vq))
    assert torch.equal(ta.buffers.flat, tb.buffers.flat)


def test_skip_guard_leaves_ema_state_untouched():
    _ops.set_compute_dtype("x3mx_hb")
    try:
        m = speech_model(4)
        tr = Trainer(m, "speech", range_check_every=0)
        tr.step(raw_batch(0))
        N.f16mx_range_flag(reset=True)
        torch.cuda.synchronize()
        before = state(m._vq)
        bad = raw_batch(1)
        bad[1, 3, 5] = float("nan")
        tr.step(bad)
        torch.cuda.synchronize()
        assert float(tr.buffers.skip_slot) == 1.0
        assert same(before, state(m._vq))
        tr.step(raw_batch(2))
        torch.cuda.synchronize()
        assert float(tr.buffers.skip_slot) == 0.0
        after = state(m._vq)
        assert not same(before, after) and all(bool(torch.isfinite(t).all()) for t in after)
        N.f16mx_range_flag(reset=True)
    finally:
        _ops.set_compute_dtype("f32")


def test_checkpoint_resumes_bitwise(mode):
    a = speech_model(5)
    ta = Trainer(a, "speech", range_check_every=0)
    for s in range(3):
        ta.step(raw_batch(s))
    buf = io.BytesIO()
    torch.save(ta.state_dict(), buf)
    ta.step(raw_batch(3))
    torch.cuda.synchronize()
    b = speech_model(6)                          # another init: everything must come from the checkpoint
    tb = Trainer(b, "speech", range_check_every=0)
    buf.seek(0)
    tb.load_state_dict(torch.load(buf, weights_only=True))
    tb.step(raw_batch(3))
    torch.cuda.synchronize()
    assert same(state(a._vq), state(b._vq))
    assert torch.equal(ta.buffers.flat, tb.buffers.flat)


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
def test_two_ranks_share_one_codebook(tmp_path, run_mode, buckets):
    """Two gloo ranks on one card (as tests/test_rccl_gpu.py runs tests/helpers/ddp_equiv.py): the per-code statistics are summed
    over the ranks, so both end on bitwise the same state; in f32 it is the state one process reaches on the whole batch."""
    helper = os.path.join(ROOT, "tests", "helpers", "vq_ema_ddp.py")
    two = str(tmp_path / "two.pt")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), helper, run_mode, two, str(buckets), "2"]
    p = subprocess.run(cmd, env=_env(), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r0, r1 = (torch.load("%s.rank%d" % (two, r), weights_only=True) for r in (0, 1))
    assert all(torch.equal(r0[k], r1[k]) for k in ("cs", "w", "e"))
    if run_mode == "f32":
        one = str(tmp_path / "one.pt")
        p = subprocess.run([sys.executable, helper, run_mode, one, str(buckets), "2"], env=_env(), capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        o = torch.load(one + ".rank0", weights_only=True)
        for k in ("cs", "w", "e"):
            close(r0[k], o[k].double().numpy())


def test_init_codebook_sets_the_moving_averages():
    m = speech_model(7)
    xs = [N.standardise(raw_batch(s), take_abs=True) for s in (0, 1)]      # as Trainer(kind="speech") preprocesses
    km = m.init_codebook(xs, random_state=0, max_iter=5)
    vq = m._vq
    counts = torch.bincount(km.labels_, minlength=1024).float() / 2.0
    assert torch.equal(vq._embedding.weight, km.cluster_centers_)
    assert torch.equal(vq._ema_cluster_size, counts)
    assert torch.equal(vq._ema_w, km.cluster_centers_ * counts[:, None])
    assert float(counts.sum()) == 8000.0


def test_two_runs_are_bitwise_identical(mode):
    runs = []
    for _ in range(2):
        torch.manual_seed(9)
        vq = VectorQuantizerEMA(1024, 128, 0.25, DECAY, EPS).cuda().train()
        for s in range(3):
            vq.quantize(latent(seed=20 + s))
        m = speech_model(8)
        tr = Trainer(m, "speech", range_check_every=0)
        for s in range(2):
            tr.step(raw_batch(s))
        torch.cuda.synchronize()
        runs.append(state(vq) + state(m._vq))
    assert same(*runs)


def test_shapes_outside_the_contract_raise_before_any_launch():
    z = torch.zeros(1, 4, 64, device="cuda")
    with pytest.raises(ValueError, match="16384"):
        VectorQuantizerEMA(16385, 4, 0.25, DECAY).cuda().quantize(z)
    with pytest.raises(ValueError, match="512"):
        VectorQuantizerEMA(8, 520, 0.25, DECAY).cuda().quantize(torch.zeros(1, 520, 2, device="cuda"))
    big = torch.zeros(1, 1, 1 << 24, device="cuda")
    vq = VectorQuantizerEMA(4, 1, 0.25, DECAY).cuda().train()
    with pytest.raises(ValueError, match="2\\^24"):
        vq.quantize(big)
    vq.eval()
    vq.quantize(big[:, :, :1000])                # eval mode: no statistics, no limit beyond the argmin's
