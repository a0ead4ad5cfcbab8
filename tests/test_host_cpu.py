"""Host-side logic that needs no GPU: module surface, state_dict keys, aliasing, pickling, jitter stream,
and the loud failure of the HIP path on CPU tensors."""
import io
import os
import pickle

import numpy as np
import pytest
import torch

from oracle import vqvae_oracle as O


def make(cfg=(7, 16, 4, 2, 8, 0.25, 16), **kw):
    from acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae import ConvolutionalVQVAE
    return ConvolutionalVQVAE(*cfg, **kw)


def test_state_dict_keys_and_shapes_match_reference_layout():
    m = make((201, 32, 8, 3, 16, 0.25, 64))
    sd = m.state_dict()
    expect = O.vqvae_param_shapes(201, 32, 8, 16, 64)
    for k, shape in expect.items():
        for r in range(3):
            kk = k.replace("_layers.0.", "_layers.%d." % r)
            assert kk in sd and tuple(sd[kk].shape) == shape, kk
    assert len(sd) == 17 + 2 * 2 * 2      # 17 unique + (2 stacks x 2 weights x layers 1..2) aliases
    assert len(list(m.parameters())) == 17
    # shared residual object (residual_stack.py:40-41)
    layers = m._encoder._residual_stack._layers
    assert layers[0] is layers[1] is layers[2]
    assert m._decoder._use_jitter and hasattr(m._decoder, "_jitter")
    assert not hasattr(make(use_jitter=False)._decoder, "_jitter")
    assert make(out_channels=1)._decoder._conv_trans_3.weight.shape == (16, 1, 3)
    assert m.get_embedding_dim() == 8


def test_init_distributions():
    torch.manual_seed(0)
    m = make((64, 256, 16, 2, 128, 0.25, 512))
    w = m._encoder._conv_1.weight
    assert float(w.abs().max()) <= (6.0 / (64 * 3)) ** 0.5 + 1e-6
    cb = m._vq._embedding.weight
    assert float(cb.abs().max()) <= 1.0 / 512
    k1 = m._encoder._residual_stack._layers[0]._block[3].weight     # never Kaiming-initialised (residual.py:55)
    assert float(k1.abs().max()) <= (1.0 / 128) ** 0.5 + 1e-6
    wt = m._decoder._conv_trans_3.weight                             # fan_in = Cout*k for ConvTranspose
    assert float(wt.abs().max()) <= (6.0 / (64 * 3)) ** 0.5 + 1e-6


def test_src_alias_is_same_module_object():
    import src.acoustic_locating_vq_vae.vq_vae.modules.residual as a
    import acoustic_locating_vq_vae.vq_vae.modules.residual as b
    assert a is b and a.Residual is b.Residual
    import importlib
    c = importlib.import_module("src.acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae")
    from acoustic_locating_vq_vae.vq_vae import convolutional_vq_vae as d
    assert c is d


def test_whole_module_pickle_roundtrip_keeps_aliasing():
    m = make()
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    m2 = torch.load(buf, weights_only=False)
    assert m2._encoder._residual_stack._layers[0] is m2._encoder._residual_stack._layers[1]
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    pickle.loads(pickle.dumps(m))


def test_load_reference_style_state_dict():
    m = make()
    p = O.closed_form_params(O.vqvae_param_shapes(7, 16, 4, 8, 16), codebook_scale=0.8)
    sd = {}
    for k, v in p.items():
        for r in range(2):
            sd[k.replace("_layers.0.", "_layers.%d." % r)] = v
    m.load_state_dict(sd)
    assert torch.equal(m._decoder._conv_trans_1.weight, p["_decoder._conv_trans_1.weight"])


def test_jitter_host_stream_matches_golden(golden_dir):
    from acoustic_locating_vq_vae import _ops
    g = np.load(os.path.join(golden_dir, "g5_jitter.npz"))
    for length in (13, 201, 500):
        for seed in (0, 1):
            np.random.seed(seed)
            assert np.array_equal(_ops.jitter_source_index(length, 0.25), g["L%d_s%d" % (length, seed)])


def test_forward_on_cpu_fails_loudly():
    m = make()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.randn(2, 7, 13))
    from acoustic_locating_vq_vae.vq_vae.vector_quantizer import VectorQuantizer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VectorQuantizer(16, 4, 0.25)(torch.randn(2, 4, 6))


def test_tensor_on_another_card_is_refused(monkeypatch):
    """One process per GPU: the kernels are launched on the current device's stream, so an input living on another card
    must raise instead of being handed to a kernel that runs elsewhere (stand-in tensor: this test needs no GPU)."""
    from acoustic_locating_vq_vae import _ops

    class OnCard1:
        is_cuda = True
        device = torch.device("cuda", 1)

    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    with pytest.raises(RuntimeError, match=r"set_device\(1\)"):
        _ops._need_gpu(OnCard1(), "ConvolutionalVQVAE")
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 1)
    _ops._need_gpu(OnCard1(), "ConvolutionalVQVAE")


def test_echoed_model_surface():
    from acoustic_locating_vq_vae.vq_vae.echoed_speech_model import EchoedSpeechReconModel
    rir = make((20, 16, 4, 2, 8, 0.25, 16), use_jitter=False, out_channels=1)
    sp = make((9, 16, 6, 3, 16, 0.25, 32))
    if torch.cuda.is_available():
        pytest.skip("constructor moves sub-models to the GPU; covered by the gpu tests")
    e = EchoedSpeechReconModel(rir, sp, 9, 16, 2, 16, True)
    assert e.embedding_dim == 10 and not e.rir_model._vq._train_vq and not e.speech_model._vq._train_vq
    e.set_train_encoder(True)
    assert e.flag_train_encoder
    assert e._decoder._conv_1.weight.shape == (16, 10, 3)


# The reference checkout's package layout (module names only): every __init__.py there is empty and vq_vae/location_model
# has none.  The overlay test builds a stand-in checkout of this shape, so it needs nothing outside the repository.
_REFERENCE_LAYOUT = ("src/__init__.py", "src/acoustic_locating_vq_vae/__init__.py",
                     "src/acoustic_locating_vq_vae/data_preprocessing.py", "src/acoustic_locating_vq_vae/visualization.py",
                     "src/acoustic_locating_vq_vae/rir_dataset_generator/__init__.py",
                     "src/acoustic_locating_vq_vae/rir_dataset_generator/specsdataset.py",
                     "src/acoustic_locating_vq_vae/vq_vae/__init__.py", "src/acoustic_locating_vq_vae/vq_vae/convolutional_encoder.py",
                     "src/acoustic_locating_vq_vae/vq_vae/convolutional_vq_vae.py",
                     "src/acoustic_locating_vq_vae/vq_vae/deconvolutional_decoder.py",
                     "src/acoustic_locating_vq_vae/vq_vae/echoed_speech_model.py",
                     "src/acoustic_locating_vq_vae/vq_vae/location_model/location_model.py",
                     "src/acoustic_locating_vq_vae/vq_vae/modules/__init__.py", "src/acoustic_locating_vq_vae/vq_vae/modules/jitter.py",
                     "src/acoustic_locating_vq_vae/vq_vae/modules/residual.py",
                     "src/acoustic_locating_vq_vae/vq_vae/modules/residual_stack.py",
                     "src/acoustic_locating_vq_vae/vq_vae/vector_quantizer.py")


def _stand_in_reference(root):
    """A checkout with the reference's layout: empty __init__.py files as there, every other module a stub that fails on
    import -- except visualization, which this build does not provide and which must resolve from here."""
    for rel in _REFERENCE_LAYOUT:
        path = os.path.join(root, *rel.split("/"))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            if rel.endswith("__init__.py"):
                pass
            elif rel.endswith("visualization.py"):
                fh.write("STAND_IN = True\n")
            else:
                fh.write("raise ImportError('stand-in reference module %s shadowed this build')\n" % rel)
    return root


def test_overlay_resolves_non_hot_path_modules_from_the_reference(tmp_path):
    """With the reference LATER on sys.path, every module this build provides (hot path, dataset side, location head)
    comes from this build and everything else (visualization, ...) keeps resolving from the reference."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "acoustic_locating_vq-vae_amd")
    ref = _stand_in_reference(str(tmp_path / "reference"))
    code = (
        "import acoustic_locating_vq_vae.vq_vae.convolutional_vq_vae as a;"
        "import acoustic_locating_vq_vae.vq_vae.location_model.location_model as b;"
        "import acoustic_locating_vq_vae.rir_dataset_generator.specsdataset as c;"
        "from src.acoustic_locating_vq_vae.vq_vae.modules.residual import Residual;"
        "import importlib.util as u;"
        "print(a.__file__); print(b.__file__); print(c.__file__); print(Residual.__module__);"
        "print(u.find_spec('acoustic_locating_vq_vae.visualization').origin)"
    )
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1",
               PYTHONPATH=os.pathsep.join([pkg, os.path.join(pkg, "src"), ref, os.path.join(ref, "src")]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    # hot-path modules, the dataset side and the location head (rank 4) come from this build; a module
    # this build does not provide (plotting) is found in the reference checkout
    assert lines[0].startswith(pkg) and lines[1].startswith(pkg) and lines[2].startswith(pkg)
    # the src. alias resolves to this build's module under its real name (one class identity, src/__init__.py)
    assert lines[3] == "acoustic_locating_vq_vae.vq_vae.modules.residual"
    assert lines[4].startswith(ref)


def test_package_default_mode_is_the_parity_holding_fast_mode():
    """A user who sets nothing (scripts/train_speech.py unchanged) gets x3mx_hb; ALVQ_DTYPE overrides; junk -- and the
    engines retired to internal use in round 4 -- are refused."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "acoustic_locating_vq-vae_amd")
    code = "from acoustic_locating_vq_vae import _ops; print(_ops.get_compute_dtype(), _ops.DEFAULT_DTYPE)"
    env = {k: v for k, v in os.environ.items() if k != "ALVQ_DTYPE"}
    env["PYTHONPATH"] = os.pathsep.join([pkg, os.path.join(pkg, "src")])
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.stdout.split() == ["x3mx_hb", "x3mx_hb"], out.stdout + out.stderr
    out = subprocess.run([sys.executable, "-c", code], env=dict(env, ALVQ_DTYPE="f32"), capture_output=True, text=True, timeout=300)
    assert out.stdout.split() == ["f32", "x3mx_hb"], out.stdout + out.stderr
    for junk in ("fp64", "f16mx", "bf16x3", "f16mx_hd"):
        out = subprocess.run([sys.executable, "-c", code], env=dict(env, ALVQ_DTYPE=junk), capture_output=True, text=True, timeout=300)
        assert out.returncode != 0 and "ALVQ_DTYPE" in out.stderr
    code = ("from acoustic_locating_vq_vae import _ops\n"
            "assert _ops.MODES == ('x3mx_hb', 'f16mx_hb', 'bf16x3_hb', 'f32', 'bf16')\n"
            "try:\n    _ops.set_compute_dtype('f16mx')\n    raise SystemExit(3)\nexcept ValueError:\n    pass\n"
            "_ops.set_compute_dtype('f16mx', internal=True)\nprint(_ops.get_compute_dtype())")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.split() == ["f16mx"], out.stdout + out.stderr


def test_format_and_mode_tables_say_what_the_modes_compute():
    """The arithmetic of every mode, pinned as data: which engine (forward format, gradient format) runs which role, and per
    activation format the C symbols a launch calls.  The format flags decide which trailing arguments the launch code
    appends, so each row must agree with the argument count of its own symbols -- a row paired with a neighbour's symbol is
    caught here, not on the GPU."""
    from acoustic_locating_vq_vae import _native as N
    from acoustic_locating_vq_vae import _ops
    # engine name -> (forward format, gradient format); mode -> role -> (engine name, forward, gradient)
    engines = {"f32": (None, None), "bf16": ("bf16", "bf16"), "bf16x3": ("bf16x3", "bf16x3"), "f16mx": ("f16mx", "f16mx"),
               "f16mx_hb": ("f16mx", "f16"), "bf16x3_hb": ("bf16x3", "bf16")}
    expect = {m: {None: (m,) + engines[m], "decoder": (m,) + engines[m]} for m in engines}
    expect["x3mx_hb"] = {None: ("bf16x3_hb", "bf16x3", "bf16"), "decoder": ("f16mx_hb", "f16mx", "f16")}
    expect["f16mx_hd"] = {None: ("f16mx_hb", "f16mx", "f16"), "decoder": ("f16dec", "f16", "f16")}
    assert set(expect) == set(_ops.MODES) | set(_ops.INTERNAL_MODES) and len(expect) == 8
    before = _ops.get_compute_dtype()
    try:
        for mode, roles in expect.items():
            _ops.set_compute_dtype(mode, internal=True)
            for role, (name, fwd, grad) in roles.items():
                eng = _ops._engine(role=role)
                got = (eng.name,) + tuple(f if f is None else f.name for f in (eng.fwd, eng.grad))
                assert got == (name, fwd, grad), (mode, role, got)
                assert _ops._engine(name) is eng                  # a saved node finds the engine that ran its forward
            assert _ops.has_fp16_range(mode) == (mode in ("x3mx_hb", "f16mx_hb", "f16mx", "f16mx_hd")), mode
            assert _ops.has_fp16_range() == _ops.has_fp16_range(mode)
    finally:
        _ops.set_compute_dtype(before, internal=True)
    for eng, kind in ((_ops._engine("f32"), (False, None)), (_ops._engine("bf16"), (True, N.conv1d_wgrad_bf16_multi))):
        assert (eng.can_defer, eng.wgrad_multi) == kind

    #            planes bits  scaled defer wcode wreads  operands            rows_code
    flags = {"bf16":   (1, True,  False, True,  1, (1, 2), ("bf16", "bf16x3"), 1),
             "bf16x3": (2, False, False, False, 2, (2,),   ("bf16x3",),        2),
             "f16mx":  (2, True,  True,  False, 3, (3,),   ("f16mx",),         3),
             "f16":    (1, True,  True,  True,  3, (3,),   ("f16", "f16mx"),   None)}
    symbols = {"bf16": dict(to_nlc="alvq_ncl_to_nlc_bf16", to_ncl="alvq_nlc_to_ncl_f32", relu="alvq_relu_mask_bf16",
                            pack="alvq_pack_weight_bf16", conv="alvq_conv1d_bf16", wgrad="alvq_conv1d_wgrad_bf16",
                            wgrad_multi="alvq_conv1d_wgrad_bf16_multi", wgrad_ws="alvq_conv1d_wgrad_bf16_workspace_bytes"),
               "bf16x3": dict(to_nlc="alvq_ncl_to_nlc_bf16x3", to_ncl="alvq_nlc_to_ncl_bf16x3", relu="alvq_relu_mask_bf16x3",
                              pack="alvq_pack_weight_bf16x3", conv="alvq_conv1d_bf16x3", wgrad="alvq_conv1d_wgrad_bf16x3",
                              wgrad_multi="alvq_conv1d_wgrad_bf16x3_multi",
                              wgrad_ws="alvq_conv1d_wgrad_bf16x3_workspace_bytes"),
               "f16mx": dict(to_nlc="alvq_ncl_to_nlc_f16mx", to_ncl="alvq_nlc_to_ncl_f16mx", relu="alvq_relu_mask_f16mx",
                             pack=None, conv="alvq_conv1d_f16mx", wgrad="alvq_conv1d_wgrad_f16mx",
                             wgrad_multi="alvq_conv1d_wgrad_f16mx_multi", wgrad_ws="alvq_conv1d_wgrad_f16mx_workspace_bytes"),
               "f16": dict(to_nlc="alvq_ncl_to_nlc_f16", to_ncl="alvq_nlc_to_ncl_f16", relu="alvq_relu_mask_bf16",
                           pack=None, conv="alvq_conv1d_f16", wgrad="alvq_conv1d_wgrad_f16",
                           wgrad_multi="alvq_conv1d_wgrad_f16_multi", wgrad_ws="alvq_conv1d_wgrad_bf16_workspace_bytes")}
    assert set(N._FORMATS) == set(flags)
    nargs = lambda symbol: len(N._SIGNATURES[symbol][1])
    for name, f in N._FORMATS.items():
        assert (f.name, f.planes, f.bits, f.scaled, f.defer, f.wcode, f.wreads, f.operands, f.rows_code) == (name,) + flags[name]
        for field, symbol in symbols[name].items():
            assert getattr(f, field) == symbol, (name, field)
            assert symbol is None or symbol in N.EXPORTS, symbol
        # the trailing arguments the launch code appends, against each symbol's own signature
        assert nargs(f.conv) == 17 + 2 * f.bits + f.scaled, name           # + (mask_bits, bits_out) + out_scale
        assert nargs(f.wgrad) == nargs(f.wgrad_multi) == 13 + f.scaled, name
        assert nargs(f.to_nlc) == nargs(f.to_ncl) == 6 + f.scaled, name     # + the loss scale S / 1/S
        assert nargs(f.relu) == (5 if f.relu_flat else 7), name             # (dy, t, out, n | B, C, L, stream)
        assert nargs(f.wgrad_ws) == 5 and (f.pack is None or nargs(f.pack) == 7)
        assert N._PACKERS[f.wcode] == f.pack and f.wcode in f.wreads
        # the KernelTimer families bench.py keys its roofline on (the bf16 / f16 ones ask the library which kernel it picks)
        if name in ("bf16x3", "f16mx"):
            assert f.conv_family(1, 3, 768, 4096) == "conv1d_%s_kernel<1, 3, ...>" % name
            assert f.wgrad_family(3, False) == "conv1d_wgrad_%s_kernel" % name
    assert [nargs(N._FORMATS[n].conv) for n in ("bf16", "bf16x3", "f16mx", "f16")] == [19, 17, 20, 20]
    assert [nargs(N._FORMATS[n].wgrad) for n in ("bf16", "bf16x3", "f16mx", "f16")] == [13, 13, 14, 14]

    # the operand rule: f16 accepts f16mx, bf16 accepts bf16x3, nothing else crosses
    class T:
        def __init__(self, fmt):
            self.fmt, self.planes = fmt, N._FORMATS[fmt].planes
    crossing = {(t, ref) for t in flags for ref in flags if t != ref and N._fmt_serves(T(t), T(ref))}
    assert crossing == {("f16mx", "f16"), ("bf16x3", "bf16")}
    assert all(N._fmt_serves(T(n), T(n)) for n in flags)
    with pytest.raises(ValueError):
        N._format(1, "f16mx")                                               # the door refuses a contradicting pair
    assert [N._format(p, None).name for p in (1, 2)] == ["bf16", "bf16x3"]
