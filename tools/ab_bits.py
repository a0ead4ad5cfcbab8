"""Bitwise fingerprint of the f16mx / bf16 / bf16x3 / f16 kernels' outputs on a fixed set of deterministic cases: run once per
library build (ALVQ_LIB=...), diff the JSON lines.  A kernel rewrite that claims "bit-identical" must leave every hash
unchanged.     ALVQ_LIB=$PWD/acoustic_locating_vq-vae_amd/lib/libalvq_base.so python3 tools/ab_bits.py > a.json
               python3 tools/ab_bits.py > b.json && diff a.json b.json
The modes above are the default; ``python3 tools/ab_bits.py dsp`` fingerprints the waveform front end instead (STFT power and
complex, the inverse STFT of each complex result, Griffin-Lim), in fp32 and fp64.  The ten cases reach only the tiles the default
dispatch picks: ``python3 tools/ab_bits.py tiles`` repeats the convolution entries of all four modes on two small shapes under
every forcing of the dispatch options (TILE_FORCINGS), which reaches every instantiation of every forward kernel family.
``python3 tools/ab_bits.py reduce`` fingerprints the entry points behind csrc/block_reduce.h's workgroup reductions and scans
(losses, quantiser, gradient clipping, k-means, EMA codebook, t-SNE, spectrogram statistics, speech metrics, WPE, the layout
kernels that raise the fp16 range flag) on small seeded inputs.  ``python3 tools/ab_bits.py array`` fingerprints the
microphone-array families that share csrc/array_wave.h (AuxIVA, ILRMA, cACGMM, SRP-PHAT and MUSIC, beamforming and GEV, WPE,
separation scoring, permutation alignment) on the cases of tests/helpers/size_sweep_cases.py."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "acoustic_locating_vq-vae_amd")
for p in (ROOT, PKG, os.path.join(PKG, "src")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from acoustic_locating_vq_vae import _native as N  # noqa: E402


MODES = {"f16mx": (2, 3, "f16mx"), "bf16": (1, 1, None), "bf16x3": (2, 2, None), "f16": (1, 3, "f16")}   # planes, weight code, fmt


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if isinstance(t, N.NLC):     # the defined parts only: the planes' matrices and, if valid, the sign bits (guard rows hold garbage)
            for pl in range(t.planes):
                h.update(t.matrix(pl).contiguous().view(torch.uint8).cpu().numpy().tobytes())
            if t.has_bits:
                off = (t.bits_ptr - t.storage.data_ptr())
                h.update(t.storage.view(torch.uint8)[off:off + t.rows * t.Cp // 8].cpu().numpy().tobytes())
            continue
        h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


# (B, S, n_fft, hop) per precision: the front end's own framing, and the largest n_fft of each precision at a hop of 3
DSP_CASES = {torch.float32: [(3, 1601, 400, 160), (2, 1031, 2048, 3)],
             torch.float64: [(3, 1601, 400, 160), (2, 1031, 1024, 3)]}


def dsp():
    out = {}
    for real, cases in DSP_CASES.items():
        prec = "f64" if real == torch.float64 else "f32"
        for (B, S, n_fft, hop) in cases:
            g = torch.Generator(device="cuda").manual_seed(B * 1000 + S + n_fft + hop)
            x = torch.randn(B, S, device="cuda", dtype=real, generator=g)
            spec = N.stft_complex(x, n_fft, hop)
            out["dsp:stft:%s:%s" % (prec, (B, S, n_fft, hop))] = {
                "power": digest(N.stft_power(x, n_fft, hop)), "complex": digest(torch.view_as_real(spec)),
                "istft": digest(N.istft(spec, n_fft, hop))}
        B, S, n_fft, hop = cases[0]                          # T = 11
        g = torch.Generator(device="cuda").manual_seed(B + S + n_fft + hop)
        shape = (B, n_fft // 2 + 1, 1 + S // hop)
        mag = torch.rand(shape, device="cuda", dtype=real, generator=g)
        angles = torch.view_as_complex(torch.rand(shape + (2,), device="cuda", dtype=real, generator=g))
        wave = N.griffin_lim(mag, angles, 4, 0.99, n_fft, hop, S)
        out["dsp:griffin_lim:%s:%s" % (prec, (B, S, n_fft, hop))] = {"wave": digest(wave)}
    return out


# (B, C, M, L) of tests/test_conv_tile_variants_gpu.py (its docstring says why these), each at widths 1 and 3
TILE_SHAPES = [(2, 40, 250, 300), (2, 130, 100, 300)]
# per mode the options that steer its dispatch; "wide_min_tiles" is 1 throughout
TILE_FORCINGS = {m: [dict(), dict(conv_v2=0), dict(conv_k3=0)] for m in ("bf16", "f16")}
TILE_FORCINGS.update({m: [dict(fx_narrow=n, fx_rows=r) for n in (0, 1) for r in (0, 128, 256)] for m in ("bf16x3", "f16mx")})


def tiles():
    out = {}
    for mode, (planes, wpl, fmt) in MODES.items():
        enter = (lambda t, gs=None: N.ncl_to_nlc(t, planes, fmt, gs)) if fmt else (lambda t, gs=None: N.ncl_to_nlc(t, planes))
        for (B, C, M, L) in TILE_SHAPES:
            for KW in (1, 3):
                g = torch.Generator(device="cuda").manual_seed(B * 1000 + C + M + L + KW)
                r = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
                x, w, b = r(B, C, L), r(M, C, KW) / (C * KW) ** 0.5, r(M)
                s1, s2, mk, post, dy, ds, dm = r(B, M, L), r(B, M, L), r(B, M, L), r(B, M, L), r(B, M, L), r(B, C, L), r(B, C, L)
                xn, pk, pki = enter(x), N.pack_weight(w, N.W_OIK, wpl), N.pack_weight(w, N.W_IOK, wpl)
                gs = N.grad_scale(dy) if fmt else None
                for opts in TILE_FORCINGS[mode]:
                    prev = {k: N.set_option(k, v) for k, v in dict(opts, wide_min_tiles=1).items()}
                    try:
                        res = {"relu": digest(N.conv1d_bf16(xn, pk, b, relu=True)),
                               "all": digest(*N.conv1d_bf16(xn, pk, b, enter(s1), enter(s2), enter(mk), enter(post), relu=True)),
                               "ncl": digest(N.conv1d_bf16(xn, pk, b, out_ncl=True)),
                               "dgrad_skip_mask": digest(N.conv1d_bf16(enter(dy, gs), pki, skip1=enter(ds, gs), mask=enter(dm)))}
                    finally:
                        for k, v in prev.items():
                            N.set_option(k, v)
                    tag = ",".join("%s=%d" % kv for kv in sorted(opts.items())) or "default"
                    out["tiles:%s:%s:%s" % (mode, (B, C, M, L, KW), tag)] = res
    return out


def reduce():
    from acoustic_locating_vq_vae import speech_metrics as SM
    g = torch.Generator(device="cuda").manual_seed(20261019)
    f64, i32 = torch.float64, torch.int32
    r = lambda *shape, dtype=torch.float32: torch.randn(*shape, device="cuda", dtype=dtype, generator=g)
    u = lambda *shape, dtype=torch.float32: torch.rand(*shape, device="cuda", dtype=dtype, generator=g)
    ints = lambda hi, *shape: torch.randint(0, hi, shape, device="cuda", generator=g)
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, device="cuda", dtype=dtype)
    out = {}
    out["mse"] = {str(n): digest(N.mse(r(n), r(n))) for n in (1, 257, 300001)}
    for (n, K, D) in ((777, 64, 24), (1500, 10, 23)):
        flat, book, gl = r(n, D), r(K, D), u(1) + 0.5
        idx = N.vq_argmin(flat, book)
        res = {"loss": digest(*N.vq_gather_loss(flat, book, idx, 0.25)), "loss_ema": digest(*N.vq_gather_loss(flat, book, idx, 0.25, ema=True)),
               "backward": digest(*N.vq_backward(r(n, D), gl, flat, book, idx, 0.25))}
        counts, sums, size, ema_w = z(K), z(K, D), u(K) + 0.5, r(K, D)
        N.vq_ema_stats(flat, idx, counts, sums)
        res["ema_stats"] = digest(counts, sums)
        N.vq_ema_update(counts, sums, size, ema_w, book, 0.99, 1e-5)
        res["ema_update"] = digest(size, ema_w, book)
        out["vq:%s" % ((n, K, D),)] = res
    dy, x = r(3, 20, 301), r(3, 7, 301)
    out["conv1d_wgrad_f32"] = {"dw_db": digest(*N.conv1d_wgrad(dy, x, 3, want_bias=True))}
    out["grad_scale"] = {str(n): digest(N.grad_scale(r(n) * 37.0)) for n in (5, 1031, 2 ** 20 + 3)}
    for n in (1, 65, 2 ** 20 + 3):
        sc, ws = z(N.ADAM_SCALARS), N.grad_clip_workspace("cuda")
        N.adam_advance(sc, 1e-3, 0.9, 0.999, 0.5)
        N.grad_clip(r(n), sc, 0.75, workspace=ws)
        out["grad_clip:%d" % n] = {"scalars": digest(sc), "sum": digest(ws[-1:]), "partials": digest(ws)}
    for (n, K, D) in ((1025, 5, 129), (300, 3, 5)):
        x, old = r(n, D), r(K, D)
        labels = ints(K - 1, n)                                       # cluster K - 1 is empty: the relocation runs
        new, counts, stats, flags = z(K, D), z(K, dtype=i32), z(1, dtype=f64), z(4, dtype=i32)
        N.kmeans_update(x, labels, None, old, new, counts, stats, flags, 1e-4)
        res = {"update": digest(new, counts, stats, flags), "inertia": digest(N.kmeans_inertia(x, labels, new))}
        N.kmeans_update(x, ints(K, n), labels, old, new, counts, stats, flags, 1e-4)
        res["update_full"] = digest(new, counts, stats, flags)
        res["plusplus"] = digest(*N.kmeans_plusplus(x, K, 7, u(K - 1, 4, dtype=f64)))
        out["kmeans:%s" % ((n, K, D),)] = res
    for n in (2, 257):
        P = N.tsne_code_sqdist(ints(16, n, 12).to(i32))
        beta, S = N.tsne_affinities(P, min(30.0, n / 2.0))
        Y, upd, gains, grad, stats = r(n, 2, dtype=f64) * 1e-4, z(n, 2, dtype=f64), z(n, 2, dtype=f64) + 1.0, z(n, 2, dtype=f64), z(2, dtype=f64)
        N.tsne_descend(P, Y, upd, gains, grad, stats, 5, 12.0, 0.5, 200.0)
        out["tsne:%d" % n] = {"affinities": digest(P, beta, S), "descend": digest(Y, upd, gains, grad, stats)}
    S, E = torch.view_as_complex(r(2, 5, 300, 2)), torch.view_as_complex(r(2, 5, 300, 2, dtype=f64))
    out["spec_rir_wiener"] = {"all": digest(*N.spec_rir_wiener(S, E))}
    clean = r(2, 6000, dtype=f64)
    clean[0, 2000:3000] *= 1e-4                                       # frames more than 40 dB down: dropped by the mask
    noisy = clean + 0.3 * r(2, 6000, dtype=f64)
    out["stoi"] = {"all": digest(*N.stoi(clean, noisy, *SM.stoi_band_edges()))}
    for dt, tag in ((torch.float32, "f32"), (f64, "f64")):
        a, b = r(3, 1001, dtype=dt), r(3, 1001, dtype=dt)
        p, q = u(2, 9, 300, dtype=dt), u(2, 9, 300, dtype=dt)
        out["metrics:%s" % tag] = {"si_sdr": digest(N.si_sdr(a, b)), "lsd": digest(N.lsd(p, q, 1e-10))}
    for (B, D, F, T, taps, delay) in ((2, 2, 5, 200, 8, 2), (1, 4, 2, 2000, 16, 3)):     # the row in LDS; too long for it
        for dt, tag in ((torch.float32, "c64"), (f64, "c128")):
            X = torch.view_as_complex(r(B, D, F, T, 2, dtype=dt))
            out["wpe:%s:%s" % (tag, (B, D, F, T, taps))] = {"all": digest(*N.wpe(X, taps, delay, 3, 0, 1e-10, 1e-10))}
    out["onehot_to_index"] = {"all": digest(*N.onehot_to_index(N.onehot(ints(130, 300), 130)))}
    x = r(2, 40, 300)
    x[1, 3, 5], x[0, 7, 250] = 7.0e4, float("nan")                    # raises both bits of the fp16 range flag
    N.f16mx_range_flag()
    res = {"rows_to_nlc": digest(N.rows_to_nlc(x.permute(0, 2, 1).contiguous(), 2, "f16mx")), "flag_rows": N.f16mx_range_flag()}
    res.update({"ncl_to_nlc": digest(N.ncl_to_nlc(x, 2, "f16mx")), "flag_ncl": N.f16mx_range_flag()})
    out["layout:f16mx"] = res
    return {"reduce:" + k: v for k, v in out.items()}


def array():
    """The microphone-array families behind csrc/array_wave.h, on the inputs of their own ``tests/helpers/*_ref.py`` builders:
    every case of size_sweep_cases.py (every compiled D, K, J and L) and beamform_ref.PARITY (both covariance kernels at
    every D, with the steering vectors towards their sources), in complex64 and complex128 where the family takes both; one
    WPE, one scoring and one alignment case.  Every
    hash covers the status words."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import numpy as np
    import align_ref as AR
    import beamform_ref as BR
    import cacgmm_ref as CR
    import ilrma_ref as LR
    import iva_ref as IR
    import separation_metrics_ref as MR
    import size_sweep_cases as S
    import srp_ref as SR
    import subspace_ref as UR
    import wpe_ref as WR
    from acoustic_locating_vq_vae import beamforming as BF
    from acoustic_locating_vq_vae import dereverberation as DR
    from acoustic_locating_vq_vae import localization as LOC
    from acoustic_locating_vq_vae import separation as SEP
    from acoustic_locating_vq_vae import speech_metrics as SM

    dev = lambda a: torch.tensor(np.ascontiguousarray(a)).cuda()
    def leaves(r):                                                    # the tensors of a result, its nested results included
        if torch.is_tensor(r):
            return [torch.view_as_real(r.resolve_conj()) if r.is_complex() else r]
        return [t for part in r for t in leaves(part)] if isinstance(r, tuple) else []

    flat = lambda *results: digest(*leaves(results))
    precisions = ((np.complex64, "c64"), (np.complex128, "c128"))
    out = {}
    for shape in S.IVA:
        for cdtype, tag in precisions:
            x = dev(IR.parity_case(shape).X.astype(cdtype))
            res = {model: flat(SEP.auxiva(x, shape[4], model, ref=shape[1] - 1)) for model in IR.MODELS}
            res["masks"] = flat(SEP.masks(x))
            out["auxiva:%s:%s" % (tag, shape[:4])] = res
    for shape in S.ILRMA_WALK:
        starts = [dev(a) for a in LR.parity_start(shape)]
        for cdtype, tag in precisions:
            x = dev(LR.parity_case(shape).X.astype(cdtype))
            out["ilrma:%s:%s" % (tag, shape[:5])] = {"all": flat(SEP.ilrma(x, *starts, iterations=shape[5], ref=shape[1] - 1))}
    for shape in S.CACGMM:
        c = CR.parity_case(shape)
        for cdtype, tag in precisions:
            out["cacgmm:%s:%s" % (tag, shape[:5])] = {"all": flat(SEP.cacgmm(dev(c.X.astype(cdtype)), dev(c.init), shape[5]))}
    for shape in S.SRP:
        B, D, T, G, f_lo, f_hi, n_fft = shape
        c = SR.parity_case(shape)
        mics, cand = dev(c.mics), dev(c.cand)
        for cdtype, tag in precisions:
            x = dev(c.X.astype(cdtype))
            res = {"psi": flat(LOC.cross_spectra(x, band=(f_lo, f_hi))),
                   "srp": flat(LOC.srp_phat(x, mics, cand, fs=SR.FS, n_fft=n_fft, c=SR.C, band=(f_lo, f_hi))),
                   "gcc": flat(LOC.gcc_phat(x, min(8, n_fft // 2), band=(f_lo, f_hi), n_fft=n_fft))}
            for K in UR.music_orders(D):
                res["music K=%d" % K] = flat(LOC.music(x, mics, cand, K, n_fft=n_fft, band=(f_lo, f_hi)))
            out["srp:%s:%s" % (tag, shape)] = res
    for shape in S.BEAMFORM + BR.PARITY:
        B, D, F, T, loading = shape
        c = BR.parity_case(shape)
        A, noise, speech = dev(c.A), dev(c.masks["runs"]), dev(c.masks["uniform"])
        out["steering:%s" % (shape[:4],)] = {"ref %d" % ref: flat(BF.steering_vectors(dev(c.mics), dev(c.source), F, ref=ref))
                                             for ref in sorted({0, D - 1})}
        for cdtype, tag in precisions:
            x = dev(c.X.astype(cdtype))
            cov_n, cov_s, cov = (BF.spatial_covariance(x, m) for m in (noise, speech, None))
            w = BF.weights("mvdr", cov_n.cov, A, loading=loading)
            res = {"cov": flat(cov_n, cov_s, cov), "das": flat(BF.weights("das", steering=A)), "mvdr": flat(w),
                   "souden": flat(BF.weights("souden", cov_n.cov, speech_cov=cov_s.cov, ref=D - 1, loading=loading)),
                   "apply": flat(BF.apply(x, w.w))}
            for ref in sorted({0, D - 1}):
                res["gev ref %d" % ref] = flat(BF.gev(x, noise, speech, ref=ref, loading=loading))
            out["beamform:%s:%s" % (tag, shape[:4])] = res
    B, D, F, T, taps, delay = 2, 2, 3, 200, 4, 2
    for cdtype, tag in precisions:
        x = dev(WR.case(B, D, F, T, taps, delay, 0).X.astype(cdtype))
        out["wpe:%s:%s" % (tag, (B, D, F, T, taps))] = {"all": flat(DR.wpe(x, taps, delay, 3, 0))}
    shape = S.SCORING[3]                                              # (K, J, n) = (4, 7, 257)
    c = MR.case(shape)
    for dtype, tag in ((np.float32, "f32"), (np.float64, "f64")):
        s, e = dev(c.references.astype(dtype)), dev(c.estimates.astype(dtype))
        out["scoring:%s:%s" % (tag, shape)] = {"table": flat(SM.pairwise_si_sdr(s, e)), "pit": flat(SM.pit_si_sdr(s, e)),
                                               "bss_eval": flat(SM.si_bss_eval(s, e))}
    shape = S.ALIGN[6]                                                # K = 7: a thread of the search takes more than one trip
    p = dev(AR.parity_case(shape).P)
    out["align:%s" % (shape[:4],)] = {str(n): flat(SEP.align_permutations(p, n)) for n in (1, 3)}
    return {"array:" + k: v for k, v in out.items()}


def main():
    modes = sys.argv[1:] or ["f16mx", "bf16", "bf16x3", "f16"]
    out = dsp() if "dsp" in modes else {}
    if "tiles" in modes:
        out.update(tiles())
    if "reduce" in modes:
        out.update(reduce())
    if "array" in modes:
        out.update(array())
    modes = [m for m in modes if m not in ("dsp", "tiles", "reduce", "array")]
    shapes = [(2, 7, 16, 13, 3), (3, 72, 136, 95, 1), (2, 201, 1024, 500, 3), (2, 1024, 128, 500, 3), (2, 1024, 1024, 201, 1),
              (5, 130, 130, 129, 3), (4, 1024, 1024, 500, 1), (4, 1024, 1024, 500, 3), (3, 1024, 201, 500, 3), (2, 500, 1024, 201, 3)]
    for mode in modes:
        # f16: one fp16 plane reading the H plane of f16mx-packed weights, gradients under a loss scale (the _hb backward)
        planes, wpl, fmt = MODES[mode]
        for (B, C, M, L, KW) in shapes:
            g = torch.Generator(device="cuda").manual_seed(B * 1000 + C + M + L + KW)
            x = torch.randn(B, C, L, device="cuda", generator=g)
            # small / huge magnitudes ride along: denormal fp16 halves, saturation
            x[0, 0, :4] = torch.tensor([3e-8, -2e-7, 7e4, 1e-5], device="cuda")[:min(4, L)]
            w = torch.randn(M, C, KW, device="cuda", generator=g) / (C * KW) ** 0.5
            b = torch.randn(M, device="cuda", generator=g)
            s1, s2, post = (torch.randn(B, M, L, device="cuda", generator=g) for _ in range(3))
            mk = torch.randn(B, M, L, device="cuda", generator=g)
            dy = torch.randn(B, M, L, device="cuda", generator=g)
            enter = (lambda t, gs=None: N.ncl_to_nlc(t, planes, fmt, gs)) if fmt else (lambda t, gs=None: N.ncl_to_nlc(t, planes))
            xn = enter(x)
            key = "%s:%s" % (mode, (B, C, M, L, KW))
            res = {"enter": digest(xn), "leave": digest(N.nlc_to_ncl(xn))}
            pk = N.pack_weight(w, N.W_OIK, wpl)
            pki = N.pack_weight(w, N.W_IOK, wpl)
            res["pack"] = digest(pk[0], pki[0])
            t = N.conv1d_bf16(xn, pk, b, relu=True)                                   # bias + relu (+ sign bits)
            res["relu"] = digest(t)
            y, y2 = N.conv1d_bf16(xn, pk, b, enter(s1), enter(s2), enter(mk), enter(post), relu=True)
            res["all"] = digest(y, y2)
            res["skip_relu"] = digest(N.conv1d_bf16(xn, pk, None, enter(s1), relu=True))
            res["ncl"] = digest(N.conv1d_bf16(xn, pk, b, out_ncl=True))
            gs = N.grad_scale(dy) if fmt else None
            dyn = enter(dy, gs)
            res["dgrad_maskbits"] = digest(N.conv1d_bf16(dyn, N.pack_weight(w, N.W_IOK, wpl), mask=enter(torch.randn(B, C, L, device="cuda", generator=g)) if mode == "bf16x3" else xn_relu(xn, N, mode, B, C, L, g, enter)))
            res["dgrad_skip_mask"] = digest(N.conv1d_bf16(dyn, N.pack_weight(w, N.W_IOK, wpl), skip1=enter(torch.randn(B, C, L, device="cuda", generator=g), gs), mask=enter(torch.randn(B, C, L, device="cuda", generator=g))))
            dw, db = N.conv1d_wgrad_bf16(dyn, xn, KW, N.W_OIK, want_bias=True)
            res["wgrad"] = digest(dw, db)
            res["wgrad_multi3"] = digest(N.conv1d_wgrad_bf16_multi([(dyn, xn)] * 3, KW, N.W_OIK))
            res["relu_mask"] = digest(N.relu_mask_bf16(dyn, enter(mk)))
            out[key] = res
    for k in sorted(out):
        print(json.dumps({k: out[k]}, sort_keys=True))


def xn_relu(xn, N, mode, B, C, L, g, enter):
    """A ReLU'd tensor of the input's shape that carries sign bits (the mask operand of a data-gradient launch)."""
    t = enter(torch.randn(B, C, L, device="cuda", generator=g))
    out = N.relu_mask_bf16(t, t)        # relu via mask; no sign bits here
    pk1 = N.pack_weight(torch.eye(C, device="cuda").view(C, C, 1).contiguous(), N.W_OIK, MODES[mode][1])
    return N.conv1d_bf16(out, pk1, relu=True)   # identity conv with ReLU: leaves the sign bits behind


if __name__ == "__main__":
    main()
