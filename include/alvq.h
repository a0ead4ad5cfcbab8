/*
 * alvq.h -- C ABI of libalvq.so: the MI355X (gfx950) kernels behind the VQ-VAE
 * train-step hot path of guy3540/Acoustic_Locating_VQ-VAE.
 *
 * The reference has no FFI layer: its operator API for this path is the
 * torch.nn.Module surface of src/acoustic_locating_vq_vae/vq_vae/ (SURVEY 8b), and
 * the ATen ops those modules call.  Each entry point below replaces one ATen op
 * call site (cited as file:line into /root/reference/src/acoustic_locating_vq_vae/).
 *
 * Conventions (all entry points):
 *   - plain C, no torch types; every pointer is a DEVICE pointer unless noted;
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library
 *     never allocates, frees or retains device memory;
 *   - launches are asynchronous on the caller's `stream` (a hipStream_t passed as
 *     void*); no host synchronisation inside, so calls are graph-capturable;
 *   - return 0 on success; a negative ALVQ_E* for arguments rejected before any
 *     launch; a positive value is the hipError_t of a failed launch.
 *     alvq_last_error() returns a thread-local message for the last failure;
 *   - tensors are dense row-major fp32 unless the name says otherwise
 *     ("_bf16": storage is bfloat16, accumulation is always fp32).
 */
#ifndef ALVQ_H
#define ALVQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALVQ_OK 0
#define ALVQ_EINVAL (-1)      /* bad pointer / dimension                        */
#define ALVQ_EUNSUPPORTED (-2) /* shape or flag combination not implemented      */

/* weight layouts for the conv family */
#define ALVQ_W_OIK 0 /* w[M][C][KW]: nn.Conv1d weight used forward, or ConvTranspose1d weight used for its data-grad */
#define ALVQ_W_IOK 1 /* w[C][M][KW] read flipped+transposed: nn.ConvTranspose1d forward, or nn.Conv1d data-grad       */

/* storage dtypes */
#define ALVQ_F32 0
#define ALVQ_BF16 1

const char* alvq_version(void);
const char* alvq_last_error(void);

/* Dispatch options: which kernel variant serves a launch (never what it computes).  Each starts from the environment
 * variable ALVQ_<NAME> (read once, at the first use of the library) or its default, and can be changed at run time here;
 * the launch path reads an atomic, never the environment.  Names / defaults:
 *   wide_min_tiles 192   bf16: 256 x 256-tile conv kernels only for problems with at least this many such tiles
 *   conv_v2 1, conv_k3 1 bf16: the 256 x 256 kernels at all / the shared-slab width-3 form
 *   wgrad_v3 3           bf16 weight gradient without bias: v3 kernels for width 1 (bit 0) / width 3 (bit 1)
 *   fx_rows 0            f16mx / bf16x3 conv row tile: 0 automatic, 128 or 256 forced
 *   fx_narrow 1          f16mx: 128-channel m-tile for fp32-NCL outputs of <= 128 channels; bf16x3: the 128-channel m-tiles
 *                        (outputs of <= 128 channels, problems with fewer than 192 tiles of 256 x 256)
 *   fx_epi 1             f16mx conv, f16mx output with no operand / bias alone / skip1 alone on whole 256-channel m-tiles:
 *                        the kernel compiled for that operand set (0: the general epilogue; bit-identical results)
 *   vq_reg 1             quantiser argmin, D <= 256: x rows in registers + double-buffered codebook tile (0: the
 *                        LDS-stationary kernel; bit-identical results)
 *   phat_lds 1           PHAT cross-spectra / SRP-PHAT: a bin's normalised rows / an item's psi band in LDS where they fit
 *                        (0: always re-read from global memory; bit-identical results)
 * alvq_set_option returns ALVQ_EINVAL for an unknown name; alvq_get_option returns INT64_MIN. */
int alvq_set_option(const char* name, int64_t value);
int64_t alvq_get_option(const char* name);

/* ------------------------------------------------------------------------------------------------
 * 1-D convolution, stride 1, "same" padding, KW in {1,3}:  im2col-free implicit GEMM on MFMA.
 *
 *   acc[b,m,l] = sum_c sum_t A_t[m,c] * x[b,c,l+t-(KW-1)/2]           (zero outside [0,L))
 *   A_t[m,c]   = w[m][c][t]            (ALVQ_W_OIK)
 *              = w[c][m][KW-1-t]       (ALVQ_W_IOK)
 *   v = acc (+ bias[m]) (+ skip1[b,m,l]) (+ skip2[b,m,l]);  if relu: v = max(v,0);
 *   if mask: v = mask[b,m,l] > 0 ? v : 0;   y = v;   if y2: y2 = v + post[b,m,l]
 *
 * x is (B,C,L), y/skip1/skip2/mask/post/y2 are (B,M,L), all contiguous.  Optional pointers may be NULL.
 * Replaces: nn.Conv1d forward (vq_vae/convolutional_encoder.py:17-23,40; convolutional_vq_vae.py:32-37,95;
 * deconvolutional_decoder.py:19-25,69; modules/residual.py:37-54), nn.ConvTranspose1d forward
 * (deconvolutional_decoder.py:35-59,73-77), F.relu / nn.ReLU(True) (residual.py:36,47;
 * residual_stack.py:46), the residual and encoder skip adds (residual.py:66; convolutional_encoder.py:42),
 * and -- through autograd -- the data-gradient of each of those with the ReLU-backward mask fused.
 * ---------------------------------------------------------------------------------------------- */
int alvq_conv1d_f32(const float* x, const float* w, const float* bias,
                    const float* skip1, const float* skip2, const float* mask, const float* post,
                    float* y, float* y2,
                    int B, int C, int M, int L, int KW, int w_layout, int relu, void* stream);

/* Weight gradient of the same convolution, split over the batch*length reduction:
 *   dw_t[m,c] = sum_b sum_l dy[b,m,l] * x[b,c,l+t-(KW-1)/2]
 * written as dw[m][c][t] (ALVQ_W_OIK) or dw[c][m][KW-1-t] (ALVQ_W_IOK, with dy/x roles as the caller passes them).
 * `workspace` must hold alvq_conv1d_wgrad_workspace_bytes(...) bytes; partial sums are reduced in a fixed
 * order (bitwise reproducible).  accumulate!=0 adds into dw (shared residual weights, residual_stack.py:40-41).
 * If dbias != NULL also dbias[m] (+)= sum_b sum_l dy[b,m,l].
 * Replaces: autograd's convolution_backward weight/bias grads for every call site listed above. */
int64_t alvq_conv1d_wgrad_workspace_bytes(int B, int C, int M, int L, int KW);
int alvq_conv1d_wgrad_f32(const float* dy, const float* x, float* dw, float* dbias, void* workspace,
                          int B, int C, int M, int L, int KW, int w_layout, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Vector quantiser (vq_vae/vector_quantizer.py:29-58).  x is the contiguous (B,D,L) buffer viewed as
 * (N,D) rows in memory order (no permute, :32); codebook is (K,D).
 * ---------------------------------------------------------------------------------------------- */
/* idx[n] = argmin_k fl(fl(|x_n|^2 + |e_k|^2) - 2 x_n.e_k), lowest k on ties (:34-38).
 * min_dist may be NULL.  workspace: alvq_vq_argmin_workspace_bytes(N,K) bytes.
 * Every index is in [0, K).  A row that holds a NaN or an infinity has no distance below +inf: it gets index 0 and
 * distance +inf.  A code row that holds a NaN or an infinity is never chosen by a finite row. */
int64_t alvq_vq_argmin_workspace_bytes(int64_t N, int K, int D);
int alvq_vq_argmin_f32(const float* x, const float* codebook, int64_t* idx, float* min_dist, void* workspace,
                       int64_t N, int K, int D, void* stream);

/* q_st = x + (E[idx] - x) (:43,54);  sq_partials[ALVQ_VQ_PARTIALS] = per-workgroup partial sums of
 * (E[idx]-x)^2 (fixed order, reproducible);  hist[k] += #rows with idx==k (int32[K], caller zeroes; may be NULL). */
#define ALVQ_VQ_PARTIALS 1024
int alvq_vq_gather_loss_f32(const float* x, const float* codebook, const int64_t* idx, float* q_st,
                            float* sq_partials, int32_t* hist, int64_t N, int K, int D, void* stream);

/* m = sum(sq_partials)/(N*D); loss = m + beta*m (:46-52); perplexity = exp(-sum p log(p+1e-10)), p = hist/N (:55-56).
 * out[0] = loss, out[1] = perplexity. */
int alvq_vq_finalize_f32(const float* sq_partials, const int32_t* hist, float* out, int64_t N, int K, int D,
                         float beta, void* stream);

/* The same for VectorQuantizerEMA, whose loss has no q-latent term: out[0] = beta*m, out[1] = perplexity. */
int alvq_vq_finalize_ema_f32(const float* sq_partials, const int32_t* hist, float* out, int64_t N, int K, int D,
                             float beta, void* stream);

/* Backward:  dx = g + gl*(2*beta/(N*D))*(x - E[idx]);
 * dE[k] += gl*(2/(N*D)) * sum_{n: idx_n = k} (E[k] - x_n)  (skipped when dE == NULL, i.e. _train_vq False);
 * g = grad wrt q_st (may be NULL = 0), gl = *grad_loss (device scalar, may be NULL = 1).  dE is accumulated into
 * (zero it first for a plain gradient).  No atomics: workgroups (code, row segment) gather their rows in row order
 * and sum them in a fixed pattern, partials are added in segment order, so the result is bitwise reproducible.
 * `workspace`: alvq_vq_backward_workspace_bytes(K,D) bytes, required when dE != NULL.  D % 4 == 0 and D <= 512,
 * or D <= 256. */
int64_t alvq_vq_backward_workspace_bytes(int K, int D);
int alvq_vq_backward_f32(const float* g, const float* grad_loss, const float* x, const float* codebook,
                         const int64_t* idx, float* dx, float* dE, void* workspace, int64_t N, int K, int D, float beta,
                         void* stream);

/* Dense one-hot encodings (N,K) fp32 (:39-40) -- only materialised for get_latent_representation callers. */
int alvq_onehot_f32(const int64_t* idx, float* encodings, int64_t N, int K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Jitter (vq_vae/modules/jitter.py:42-70): y[b,c,l] = x[b,c,src[l]];  backward: dx[b,c,l] = src[l]==l ? dy : 0.
 * src is an int32[L] DEVICE array produced on the host with the reference's numpy call order.
 * ---------------------------------------------------------------------------------------------- */
int alvq_jitter_gather_f32(const float* x, const int32_t* src, float* y, int64_t rows, int L, int backward, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Callers' per-step arithmetic (scripts/train_speech.py:63-64,74; train_rir.py:42-49).
 * ---------------------------------------------------------------------------------------------- */
/* y[b,c,l] = (x' - mean_c x') / (std_c x' + 1e-8), x' = |x| if take_abs else x; unbiased std over dim=1;
 * x, y are (B,C,L). */
int alvq_standardise_f32(const float* x, float* y, int B, int C, int L, int take_abs, void* stream);

/* loss[0] = mean((a-b)^2) over n elements (F.mse_loss, train_speech.py:74); workspace: ALVQ_EW_PARTIALS floats. */
#define ALVQ_EW_PARTIALS 1024
int alvq_mse_f32(const float* a, const float* b, float* loss, void* workspace, int64_t n, void* stream);
/* grad = grad_loss[0] * (2/n) * (a - b)   (grad_loss: device scalar, NULL = 1). */
int alvq_mse_backward_f32(const float* a, const float* b, const float* grad_loss, float* grad, int64_t n, void* stream);

/* out[0..n) = value (out 16-byte aligned): the flat gradient buffer's zeroing at the top of a step
 * (optimizer.zero_grad(), train_speech.py:88) as a kernel node -- a memset node recorded during stream capture
 * was observed not to be ordered before the kernel behind it on replay. */
int alvq_fill_f32(float* out, float value, int64_t n, void* stream);

/* out = a + b (elementwise), used where a gradient has two consumers. */
int alvq_add_f32(const float* a, const float* b, float* out, int64_t n, void* stream);

/* y[r] = mean over L of x[r][0..L) and its backward dx[r][l] = dy[r] / L: the optional average pooling of the latent,
 * torch.mean(z, dim=2, keepdim=True) (convolutional_vq_vae.py:96-97), with rows = B * D. */
int alvq_row_mean_f32(const float* x, float* y, int64_t rows, int L, void* stream);
int alvq_row_mean_backward_f32(const float* dy, float* dx, int64_t rows, int L, void* stream);

/* out = t > 0 ? dy : 0: ReLU backward from the saved post-ReLU activation (F.relu, residual_stack.py:46). */
int alvq_relu_mask_f32(const float* dy, const float* t, float* out, int64_t n, void* stream);

/* (B,R,C) -> (B,C,R) dense transpose (materialises permute(0,2,1), train_rir.py:45). */
int alvq_transpose_f32(const float* x, float* y, int B, int R, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Adam on a flat parameter buffer (torch.optim.Adam(lr, betas, eps, amsgrad=False), train_speech.py:154).
 * step is 1-based. grad_scale multiplies the gradient first (1/world after the all-reduce).
 * ---------------------------------------------------------------------------------------------- */
int alvq_adam_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step,
                  float lr, float beta1, float beta2, float eps, float grad_scale, void* stream);

/* Graph-replayable form: the step-dependent scalars come from device memory,
 * scalars = {lr / (1 - beta1^step), sqrt(1 - beta2^step), grad_scale}. */
/* skip (nullable, here and in alvq_adam_pack_batch / alvq_adam_segments_f32): a device float, the SKIP SLOT of the flat
 * gradient buffer.  Non-zero = this step saturated an fp16-range format on some rank (alvq_range_flag_to_slot wrote it
 * before the step's all-reduce, which sums it over the ranks): the launch leaves parameters, moments and packed images
 * bit for bit as they were -- the dynamic-loss-scaling "skip" pattern, decided on the device, no host sync. */
int alvq_adam_dev_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                      const float* scalars, float beta1, float beta2, float eps, const float* skip, void* stream);

/* Device-side step counter for the form above: scalars is EIGHT floats, {.., .., .., step, skipped, -, -, -} (both counters
 * start at 0).  Each call does step += 1 and rewrites the first three for that step, in stream order -- no host staging
 * buffer, so a host that queues steps ahead of the device cannot overwrite a step's scalars before its Adam launch reads
 * them (hyper-parameters and powers in double, as torch.optim.Adam computes them; exact step count up to 2^24).
 * prev_skip (nullable): the skip slot, still holding the PREVIOUS step's verdict (the flat gradient buffer is zeroed inside
 * the step): if non-zero that step was not applied -- step stays, skipped += 1 (a GradScaler-skipped step does not advance
 * torch.optim.Adam's step count either).  With prev_skip the call also folds the range flag's bits into its sticky word, so
 * the step about to run sees only its own. */
int alvq_adam_advance_f32(float* scalars, double lr, double beta1, double beta2, double grad_scale,
                          const float* prev_skip, void* stream);

/* *slot = 1.0f if the fp16-range formats' flag holds any bit raised since the step's guarded alvq_adam_advance_f32, else
 * 0.0f.  The last launch of a step's backward; slot is element 0 of the flat gradient buffer. */
int alvq_range_flag_to_slot(float* slot, void* stream);

/* alvq_adam_advance_f32 with a learning-rate schedule: same counters, same skip rule, but scalars[0] is derived from the rate
 * of the step t about to be applied (1-based, the APPLIED-step counter: a skipped step does not advance the schedule, a
 * replayed graph needs no host value, a resumed run lands on the same rate):
 *   t <= warmup_steps:                  lr_t = lr * t / warmup_steps                                   (linear warm-up)
 *   else, total_steps > warmup_steps:   lr_t = lr_min + (lr - lr_min) * (1 + cos(pi * p)) / 2,
 *                                       p = min(1, (t - warmup_steps) / (total_steps - warmup_steps))  (cosine annealing)
 *   else (total_steps == 0):            lr_t = lr.
 * All in double.  warmup_steps >= 0; total_steps == 0 or > warmup_steps; lr_min >= 0. */
int alvq_adam_advance_sched_f32(float* scalars, double lr, double beta1, double beta2, double grad_scale,
                                const float* prev_skip, void* stream, int64_t warmup_steps, int64_t total_steps, double lr_min);

/* Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) as an update of the scalars above; slots 5-7
 * are {norm, coef, clipped steps}.  Call it between alvq_adam_advance*_f32 (which sets scalars[2] = grad_scale) and the Adam
 * launches (which read it).  grad: n floats (4-byte aligned; 16-byte aligned buffers are read with 16-byte loads -- the
 * result does not depend on the alignment).  Two launches:
 *   1. a FIXED grid of workgroups writes partial sums of grad^2 accumulated in float64 (squares of fp32 values are exact in
 *      float64 and cannot overflow it);
 *   2. one workgroup adds the partials in index order: S, and
 *        norm = sqrt(S) * scalars[2]      -- the buffer is the sum over the ranks, scalars[2] = 1/world: the mean gradient's
 *        coef = min(1, max_norm / (norm + 1e-6))          -- an infinite norm gives 0, NaN stays NaN, as in torch
 *        scalars[5] = norm;  scalars[6] = coef;  scalars[2] *= (float)coef;  scalars[7] += 1 if coef < 1.
 * No atomics and no arrival counter: the result is a function of the buffer's contents alone, bit for bit.
 * max_norm > 0; +inf measures the norm and never clips (coef is exactly 1, scalars[2] keeps its bits).
 * skip (nullable): the skip slot; non-zero = only scalars[5] is written and scalars[6] = 1.
 * workspace: alvq_grad_clip_workspace_bytes(n) bytes, 8-byte aligned; on return its double at index
 * (bytes / 8 - 1) holds S. */
int64_t alvq_grad_clip_workspace_bytes(int64_t n);
int alvq_grad_clip_f32(const float* grad, int64_t n, float* scalars, double max_norm, void* workspace, const float* skip,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * STFT power spectrogram (scripts/genereate_dataset.py:90-91,37,39,47-49; torchaudio Spectrogram semantics:
 * center=True reflect pad, periodic Hann(n_fft), one-sided, window-normalised, |.|^2).
 * wave (B,S) -> power (B, n_fft/2+1, 1+S/hop).
 * ---------------------------------------------------------------------------------------------- */
int alvq_stft_power_f32(const float* wave, float* power, int B, int S, int n_fft, int hop, void* stream);
/* float64 form: the reference's echoed signal is float64 (scipy convolve output, genereate_dataset.py:38-39). */
int alvq_stft_power_f64(const double* wave, double* power, int B, int S, int n_fft, int hop, void* stream);

/* The same transform keeping the phase: spec (B, n_fft/2+1, T) complex, stored as interleaved (re, im) pairs of the
 * waveform's precision, divided by sqrt(sum(window^2)) (power=None, normalized=True). */
int alvq_stft_complex_f32(const float* wave, float* spec, int B, int S, int n_fft, int hop, void* stream);
int alvq_stft_complex_f64(const double* wave, double* spec, int B, int S, int n_fft, int hop, void* stream);

/* scipy.signal.convolve(wave, h, mode="same") in float64 for a float32 waveform (B,S) and float64 impulse responses
 * (genereate_dataset.py:38): out[b][i] = sum_j h[b][j] * wave[b][i + (Nh-1)/2 - j].  h_batch_stride: elements between
 * consecutive impulse responses (0: one response shared by the batch).  Nh <= S. */
int alvq_fir_same_f64(const float* wave, const double* h, double* out, int B, int S, int Nh, int h_batch_stride, void* stream);

/* Dataset-generator arithmetic on the two complex STFTs (genereate_dataset.py:41-49), per batch item:
 *   r = S / (E + 1e-8);  rir_pow = |r / max|r||^2;  wiener[f] = |sum_t E conj(S) / (sum_t S conj(S) + 1e-8)|^2;
 *   speech_pow = |S|^2 (fp32);  echoed_pow = |E|^2 (fp64).
 * speech_spec: complex64 (B,F,T) interleaved; echoed_spec: complex128 (B,F,T) interleaved; workspace: B*F doubles.
 * All sums and the max run in a fixed order. */
int alvq_spec_rir_wiener_f64(const float* speech_spec, const double* echoed_spec, float* speech_pow, double* echoed_pow,
                             double* rir_pow, double* wiener, double* workspace, int B, int F, int T, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Inverse STFT, the exact inverse of alvq_stft_complex_* (torchaudio InverseSpectrogram(n_fft, hop, center=True, pad=0,
 * normalized=True) semantics): spec (B, n_fft/2+1, T) interleaved (re, im) as alvq_stft_complex_* writes it -> wave (B, length).
 * One-sided inverse DFT (the imaginary parts of the DC and Nyquist bins are ignored, as irfft), times sqrt(sum(w^2)) and the
 * periodic Hann window w, overlap-added and divided by the overlap-added w^2, n_fft/2 trimmed at the start; samples past
 * n_fft/2 + hop*(T-1) are 0 (torch.istft's zero-padding of an explicit length).  length = hop*(T-1) is the default framing.
 * workspace: B*T*n_fft elements of the spectrum's precision.  Even n_fft >= 4, up to 2048 (f32) / 1024 (f64).  The NOLA
 * condition (overlap-added w^2 > 1e-11 over the output) is checked on the host: ALVQ_EINVAL with no launch if it fails.
 * Fixed-order sums throughout: bitwise reproducible.
 * ---------------------------------------------------------------------------------------------- */
int alvq_istft_f32(const float* spec, float* wave, float* workspace, int B, int T, int n_fft, int hop, int length, void* stream);
int alvq_istft_f64(const double* spec, double* wave, double* workspace, int B, int T, int n_fft, int hop, int length,
                   void* stream);

/* Griffin-Lim phase reconstruction (torchaudio.functional.griffinlim, the fast variant with momentum) of a magnitude
 * spectrogram mag (B, n_fft/2+1, T) normalised as alvq_stft_complex_* (|spec|), from the complex start phases angles (same
 * shape, interleaved; used as given, not normalised, as torchaudio does):
 *   tprev = 0; repeat n_iter: inverse = istft(mag * angles); rebuilt = STFT(inverse) (unnormalised);
 *              a = rebuilt - momentum/(1+momentum) * tprev; angles = a / (|a| + 1e-16); tprev = rebuilt
 *   wave = istft(mag * angles)                                                          (istft: alvq_istft_*)
 * -> wave (B, length).  n_iter >= 0, 0 <= momentum < 1; with n_iter > 0, 1 + length/hop == T and length > n_fft/2.
 * One call enqueues 3*n_iter + 2 launches on stream, with no host sync: a linear chain, capturable in a single-stream graph.
 * workspace: alvq_griffin_lim_workspace_bytes(B, T, n_fft, sizeof(element)) =
 *   (4*B*(n_fft/2+1)*T + B*T*n_fft) * elem_bytes   (two complex spectra + the inverse's frames); -1 for bad arguments. */
int64_t alvq_griffin_lim_workspace_bytes(int B, int T, int n_fft, int elem_bytes);
int alvq_griffin_lim_f32(const float* mag, const float* angles, float* wave, void* workspace, int B, int T, int n_fft, int hop,
                         int length, int n_iter, double momentum, void* stream);
int alvq_griffin_lim_f64(const double* mag, const double* angles, double* wave, void* workspace, int B, int T, int n_fft, int hop,
                         int length, int n_iter, double momentum, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Room impulse responses by the image-source method (Allen & Berkley 1979 as Habets' RIR generator states it, i.e.
 * rir_generator.generate with an omnidirectional receiver), float64.  src, rcv: device (B,3) source and receiver positions
 * (m); h: device (B, nsample).  Shared: the room Lx x Ly x Lz (m), the six wall reflection coefficients beta6_host (host array:
 * x0, x1, y0, y1, z0, z1; |beta| <= 1, negative allowed), sound speed c (m/s), sample rate fs, order (-1 = every reflection
 * order) and hp_filter (1 = the generator's 100 Hz high-pass, lfilter([1, A1, R1], [1, -B1, -B2]) per response).
 * With cTs = c/fs, Tw = 2*round(0.004*fs) and n_a = ceil(nsample / (2*L_a/cTs)), every image (m_a in [-n_a, n_a], q, j, k in
 * {0,1}) within the order whose distance d (in samples) has floor(d) < nsample adds
 *   refl / (4 pi d cTs) * 0.5 (1 + cos(2 pi (t-d)/Tw)) * sinc(pi (t-d))   at t = floor(d) - Tw/2 + 1 + n, n in [0, Tw).
 * A 2-D room is beta[4] = beta[5] = 0.  Fs up to 128 kHz (Tw <= 1024); nsample <= 2^24.  A source on the receiver gives an
 * infinite gain (callers reject it).  No atomics: each output sample is summed in one fixed image order that depends on the
 * item's own geometry only, so a response is bitwise the same in any batch.  One or two launches, no host sync, no workspace.
 * ---------------------------------------------------------------------------------------------- */
int alvq_rir_f64(const double* src, const double* rcv, double* h, int B, int nsample, double Lx, double Ly, double Lz,
                 const double* beta6_host, double c, double fs, int order, int hp_filter, void* stream);
/* The same with a room and six reflection coefficients per item: room device (B,3) (m), beta device (B,6).  Each item's image
 * ranges are computed on the device with the expression above, so row b is bitwise alvq_rir_f64 called with room[b] and
 * beta[b] alone.  status: device (B,) int, written for every item: 0, or bit 1 = some |beta[b]| > 1 (or NaN), bit 2 = a room
 * side not a positive finite length, or an image range above 4096; such an item's response is left zero (its taps are not
 * summed).  The caller reads status when it can sync.  One or two launches, no host sync, no workspace. */
int alvq_rir_rooms_f64(const double* src, const double* rcv, const double* room, const double* beta, double* h, int* status, int B,
                       int nsample, double c, double fs, int order, int hp_filter, void* stream);

/* ------------------------------------------------------------------------------------------------
 * What reverberation an impulse response has (csrc/room_acoustics.hip): Schroeder's backward integration and least-squares
 * line fits to the decay curve (ISO 3382).  h: device (B, n) responses, float32 ("_f32") or float64 ("_f64"); all arithmetic
 * is float64 (a float32 sample is widened first, so the _f32 result is bitwise the _f64 result on the widened rows).
 * B >= 1, 2 <= n <= 2^24.  One workgroup per response and one launch; no atomics, no workspace, no host sync.  Each response is
 * summed in one fixed order that depends on n alone: a row has the same bits in any batch and on any run.
 *
 * Energy decay curve: with T(t) = sum_{s >= t} h[s]^2,  edc_db[t] = 10 log10(T(t) / T(0)), evaluated as
 * 10 (log10 T(t) - log10 T(0)) and never above 0; -inf where T(t) = 0; the whole row NaN when T(0) is 0 or not finite.
 * edc_db: device (B, n) float64. */
int alvq_edc_f32(const float* h, double* edc_db, int B, int n, void* stream);
int alvq_edc_f64(const double* h, double* edc_db, int B, int n, void* stream);

/* Room-acoustic parameters.  out: device (B, 7) float64, columns t30, t20, edt (s), c50, c80 (dB), d50, drr (dB); onset and
 * status: device (B,) int32.  fs: sample rate (> 0); k50, k80, kdirect (>= 0): 50 ms, 80 ms and 2.5 ms in samples -- the
 * caller rounds them (floor(ms * 1e-3 * fs + 0.5)), the kernel has no rounding rule of its own.
 *   E(a, b) = sum_{a <= t < b} h[t]^2, a and b clipped to [0, n], taken as the difference T(a) - T(b) of tail energies.
 *   n0      = the first index of max |h[t]| (a NaN counts as the largest value), written to onset.  Everything is measured
 *             from n0.
 *   L(t)    = 10 log10(E(t, n) / E(n0, n)) for t >= n0, the decay level (evaluated as for edc_db; L(n0) = 0 exactly).
 *   A decay time over (hi, lo) dB is -60 / slope, the slope (dB/s) of the least-squares line of L(t) against (t - n0) / fs over
 *   all t >= n0 with lo <= L(t) <= hi:  t30 over (-5, -35), t20 over (-5, -25), edt over (0, -10).
 *   c50 = 10 log10(E(n0, n0 + k50) / E(n0 + k50, n)), c80 likewise with k80;  d50 = E(n0, n0 + k50) / E(n0, n);
 *   drr = 10 log10(E(n0 - kdirect, n0 + kdirect + 1) / E(n0 + kdirect + 1, n)).
 * status bits: 1 = T(0) is 0 or not finite (all seven outputs NaN, no other bit); 2 = a decay range held fewer than two
 * samples (that output NaN); 4 = a late or reverberant energy was 0 (that ratio +inf).  The caller reads status when it can
 * sync. */
int alvq_room_acoustics_f32(const float* h, double* out, int* onset, int* status, int B, int n, double fs, int k50, int k80,
                            int kdirect, void* stream);
int alvq_room_acoustics_f64(const double* h, double* out, int* onset, int* status, int B, int n, double fs, int k50, int k80,
                            int kdirect, void* stream);

/* ------------------------------------------------------------------------------------------------
 * What a listener gets from speech (csrc/speech_metrics.hip): rational resampling, STOI, SI-SDR and the log-spectral distance.
 * Rows are device (B, n), float32 ("_f32") or float64 ("_f64"); all arithmetic and every output is float64 (a float32 sample
 * is widened first).  1 <= B <= 65535, 2 <= n <= 2^24 (the resampler takes n >= 1).  No atomics, no host sync; every sum runs
 * in one order that depends on the row's sizes alone: a row has the same bits in any batch and on any run.
 *
 * Rational resampling with the semantics of scipy.signal.resample_poly(x, up, down) along the rows.  up and down are coprime,
 * 1 <= up, down <= 512; h: device (2 half + 1) float64 taps, designed by the caller: with R = max(up, down) and half = 10 R,
 * h[k] = sinc((k - half) / R) / R * kaiser(beta = 5)[k], normalised to sum 1 and multiplied by up.
 *   y[m] = sum_j x[j] h[m down - j up + half]  over the j with 0 <= j < n and 0 <= m down - j up + half <= 2 half, j rising,
 * for 0 <= m < n_out = ceil(n up / down).  y: device (B, n_out) float64.  One launch, no workspace. */
int alvq_resample_poly_f32(const float* x, const double* h, double* y, int B, int n, int up, int down, int half, void* stream);
int alvq_resample_poly_f64(const double* x, const double* h, double* y, int B, int n, int up, int down, int half, void* stream);

/* Short-time objective intelligibility (Taal, Hendriks, Heusdens, Jensen 2011) of degraded against clean, both device (B, n)
 * float64 sampled at 10 kHz.  value: device (B,) float64; kept_frames, status: device (B,) int32.
 *   W[i]    = 0.5 - 0.5 cos(2 pi (i + 1) / 257), i = 0..255.  Frames of 256 samples at hop 128 lie wholly inside the row:
 *             nf = (n - 256) / 128 + 1, frame t starts at sample 128 t.
 *   Silent frames: e_t = 20 log10(|W clean_t|_2 + eps), eps = 2^-52; frame t is kept iff e_t > max_t e_t - 40.  Both signals
 *             are rebuilt from their kept frames alone (clean's mask for both) by overlap-add of the windowed frames at hop
 *             128 in their order; M, the number kept, is written to kept_frames.
 *   Bands:    the rebuilt signals are framed the same way (M frames), windowed with W, zero-padded to 512 and transformed;
 *             X[j][m] = sqrt(sum_{lo[j] <= k < hi[j]} |DFT_m[k]|^2), 15 one-third-octave bands from 150 Hz.  band_lo_host,
 *             band_hi_host: 15 host ints each, 0 <= lo < hi <= 257, all within 256 bins of each other -- the caller finds
 *             the bins nearest the band edges, the library has no rule of its own.
 *   Segments: for every end s = 30..M and band j, x and y are the 30 envelope values before s of clean and degraded;
 *             y' = min(y |x| / (|y| + eps), (1 + 10^(15/20)) x); both lose their mean and are divided by their norm + eps;
 *             d(j, s) is their dot product.  value = the mean of d over the 15 (M - 29) pairs.
 * status: 0, or 1 = n < 256 or a frame energy of clean is not finite or all are 0 (value NaN, kept_frames 0), or
 * 2 = M < 30 (value NaN).  The caller reads it when it can sync.  Four launches.  workspace: device,
 * alvq_stoi_workspace_bytes(B, n) bytes (never 0; -1 for B or n out of range), holding the frame energies, the kept frames'
 * indices and the envelopes. */
int64_t alvq_stoi_workspace_bytes(int B, int n);
int alvq_stoi_f64(const double* clean, const double* degraded, const int* band_lo_host, const int* band_hi_host, double* value,
                  int* kept_frames, int* status, void* workspace, int B, int n, void* stream);

/* Scale-invariant signal-to-distortion ratio in dB.  With s and e the reference and estimate rows less their means and
 * a = <e, s> / <s, s>:  out[b] = 10 log10(|a s|^2 / |a s - e|^2); +inf where |a s - e|^2 is 0 (an exact multiple of the
 * reference); NaN where <s, s> is 0 or not finite.  out: device (B,) float64.  One launch, one workgroup a row. */
int alvq_si_sdr_f32(const float* reference, const float* estimate, double* out, int B, int n, void* stream);
int alvq_si_sdr_f64(const double* reference, const double* estimate, double* out, int B, int n, void* stream);

/* Log-spectral distance in dB of power spectrograms p, q: device (B, F, T), T contiguous; F, T >= 1, F T <= 2^30.
 *   out[b] = mean_t sqrt(mean_f (10 log10((p + eps) / (q + eps)))^2), eps >= 0;
 * NaN for a spectrogram pair with a negative or non-finite entry.  out: device (B,) float64.  One launch. */
int alvq_lsd_f32(const float* p, const float* q, double* out, int B, int F, int T, double eps, void* stream);
int alvq_lsd_f64(const double* p, const double* q, double* out, int B, int F, int T, double eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scores of separated sources (csrc/separation_metrics.hip): the SI-SDR of every (reference, estimate) pair, the best
 * assignment of estimates to references, and the scale-invariant SDR / SIR / SAR split (Le Roux, Wisdom, Erdogan, Hershey,
 * "SDR -- half-baked or well done?", ICASSP 2019).  references: device (B, K, n), estimates: device (B, J, n), n contiguous,
 * float32 ("_f32") or float64 ("_f64"), every sample widened on load; 1 <= K, J <= 8, 2 <= n <= 2^24, 1 <= B <= 65535.
 * Float64 arithmetic, every sum in a fixed order, no atomics, no workspace, one launch each.
 *
 * alvq_pairwise_si_sdr_*: table[b, i, j] (device (B, K, J) float64) = the SI-SDR of estimates[b, j] against references[b, i]
 * as alvq_si_sdr_* defines it, with the bits alvq_si_sdr_* gives that pair.  One workgroup per (b, i) streams the reference
 * row once per pass against all J estimates: three passes (means; <s, s> and <e_j, s>; the energies), each sum over the
 * samples t = thread, thread + 256, ... per thread, then the butterfly over the wave and the waves in order. */
int alvq_pairwise_si_sdr_f32(const float* references, const float* estimates, double* table, int B, int K, int J, int n,
                             void* stream);
int alvq_pairwise_si_sdr_f64(const double* references, const double* estimates, double* table, int B, int K, int J, int n,
                             void* stream);

/* The best assignment of J columns to K <= J rows of table (device (B, K, J) float64), by exhaustive search.  The injections
 * pi of {0..K-1} into {0..J-1} are ranked in lexicographic order of (pi(0), ..., pi(K-1)); the score of pi is
 * table[0, pi(0)] + table[1, pi(1)] + ..., k rising, starting from the first term; an injection whose score is NaN is
 * skipped.  The winner has the largest score (maximize != 0) or the smallest (maximize == 0), the lowest rank among equal
 * scores.  perm: device (B, K) int32 = pi; total: device (B,) float64 = its score; status: device (B,) int32 = 0, or 1 where
 * every injection was skipped (perm = the identity, total = NaN).  One workgroup an item: its threads stride over the ranks
 * (at most 8! = 40320), each keeps its best (score, rank), and an arg-reduction over (score, rank) under the same rule picks
 * the winner, so the result does not depend on which thread saw which rank. */
int alvq_assign_f64(const double* table, int* perm, double* total, int* status, int B, int K, int J, int maximize,
                    void* stream);

/* Scale-invariant SDR, SIR and SAR of estimates[b, perm[b, i]] against references[b, i]; perm: device (B, K) int32.  With
 * s_p the references of the item less their means, e the chosen estimate less its mean, G[p, q] = <s_p, s_q> and
 * g[p] = <s_p, e> (the sums in the order of alvq_pairwise_si_sdr_*, so G[i, i] and g[i] have the bits of its <s, s> and
 * <e, s>):  a = g[i] / G[i, i];  c solves G c = g by Gaussian elimination with partial pivoting (column j = 0 .. K - 1: the
 * pivot of the largest |.| among the rows r >= j, the lowest row winning ties; rows exchanged; row r > j loses
 * l = G[r][j] / pivot times row j; back substitution j = K - 1 .. 0);  target = a s_i;  proj = sum_p c_p s_p, p rising from
 * the first product;  interf = proj - target;  artif = e - proj.  The energies |target|^2, |target - e|^2, |interf|^2,
 * |artif|^2 and |proj|^2 are summed sample by sample in a third pass.
 *   sdr[b, i] = 10 log10(|target|^2 / |target - e|^2), with the bits of table[b, i, perm[b, i]] of alvq_pairwise_si_sdr_*;
 *   sir[b, i] = 10 log10(|target|^2 / |interf|^2);   sar[b, i] = 10 log10(|proj|^2 / |artif|^2);
 * +inf where the denominator is 0, NaN where either energy is NaN.  For K = 1, c and a are one quotient and sir = +inf.
 * sdr, sir, sar: device (B, K) float64.  status: device (B,) int32, the same in every row of the item:
 *   3  perm[b] is not an injection into 0..J-1 (checked on the device before any estimate is read): sdr, sir, sar NaN;
 *   1  else, a G[p, p] that is 0 or not finite, or a non-finite sample in an estimate perm[b] selects: sir, sar NaN;
 *   2  else, a pivot that is 0 or not finite (two identical references): sir, sar NaN;
 *   0  otherwise.  Under 1 and 2 sdr is what alvq_pairwise_si_sdr_* gives.
 * One workgroup per (b, i); each reads the item's K references and works out G and the item's status for itself. */
int alvq_si_bss_eval_f32(const float* references, const float* estimates, const int* perm, double* sdr, double* sir,
                         double* sar, int* status, int B, int K, int J, int n, void* stream);
int alvq_si_bss_eval_f64(const double* references, const double* estimates, const int* perm, double* sdr, double* sir,
                         double* sar, int* status, int B, int K, int J, int n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Weighted prediction error (WPE) dereverberation of complex spectrograms (csrc/wpe.hip; Nakatani, Yoshioka, Kinoshita,
 * Miyoshi, Juang 2010).  X, Y: device (B, D, F, T) interleaved complex, T contiguous, complex64 ("_f32") or complex128
 * ("_f64"); D microphones; X and Y must not overlap.  status: device (B, F) int32.  All arithmetic is float64 (a complex64
 * value is widened first); only Y is rounded to the input's type.  Every (b, f) bin is a problem of its own, M = D taps:
 *   x~_t in C^M  entry k D + d is x_d[t - delay - k], k = 0 .. taps - 1; 0 where t - delay - k < 0.
 *   y <- x, then `iterations` times:
 *     p_t      = the mean of |y_d[u]|^2 over d and over the frames u in [t - psd_context, t + psd_context] that exist
 *                (the window clipped to [0, T), divided by D times the frames in it)
 *     lambda_t = max(p_t, eps max_t p_t)
 *     R_ij     = sum_t x~_i[t] conj(x~_j[t]) / lambda_t,   P_id = sum_t x~_i[t] conj(x_d[t]) / lambda_t
 *     R       <- R + loading (tr R / M) I
 *     G        = R^-1 P by a Cholesky factorisation and two triangular solves
 *     y_d[t]   = x_d[t] - sum_i conj(G_id) x~_i[t]
 *   Y = the last y.
 * status: 0, or 1 = some p_t was not finite (a NaN or an infinity in the bin, or a power beyond the float64 range) or every
 * p_t was 0, or 2 = a Cholesky pivot was <= 0 or not finite (always the case where T <= delay: R = 0), in any iteration; with
 * status != 0 the bin leaves with Y = X, bit for bit.  The caller reads status when it can sync.
 * 1 <= B <= 65535, F >= 1, B F <= 2^31 - 1; 1 <= D <= 8; taps >= 1, M <= 64; 0 <= delay <= 64; 1 <= iterations <= 16;
 * 0 <= psd_context <= 64; 1 <= T <= 65535; eps, loading finite and >= 0.
 * One launch, one workgroup a bin; no atomics, no host sync; every sum runs in one order that depends on the bin's sizes alone:
 * a bin has the same bits in any batch and on any run.  workspace: device, alvq_wpe_workspace_bytes(B, D, F, T, taps) bytes --
 * 0 (the pointer may be NULL) where a bin's rows fit in the workgroup's LDS, 16 B F T otherwise; -1 for sizes out of range. */
int64_t alvq_wpe_workspace_bytes(int B, int D, int F, int T, int taps);
int alvq_wpe_f32(const float* X, float* Y, int* status, void* workspace, int B, int D, int F, int T, int taps, int delay,
                 int iterations, int psd_context, double eps, double loading, void* stream);
int alvq_wpe_f64(const double* X, double* Y, int* status, void* workspace, int B, int D, int F, int T, int taps, int delay,
                 int iterations, int psd_context, double eps, double loading, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Source localisation from a microphone array's complex spectrograms (csrc/srp_phat.hip): PHAT-weighted cross-spectra,
 * generalised cross-correlation (GCC-PHAT; Knapp, Carter 1976) and the steered response power map (SRP-PHAT; DiBiase 2000).
 * All arithmetic is float64 (a complex64 value is widened first).  No atomics, no host sync, graph-capturable; every sum
 * runs in one order that depends on sizes alone: an item has the same bits alone or in any batch and on any run, and a
 * candidate has the same bits alone or in any grid.
 *   X      device (B, D, F, T) interleaved complex, T contiguous, complex64 ("_f32") or complex128 ("_f64"); D microphones,
 *          F = n_fft / 2 + 1 bins.
 *   pairs  p = (i, j), i < j, in lexicographic order: (0,1), (0,2), ... (0,D-1), (1,2), ...;  P = D (D - 1) / 2.
 *   band   the bins f_lo .. f_hi inclusive, 0 <= f_lo <= f_hi < F.
 *   u(z)   = z / hypot(re z, im z), and 0 for z = 0: the unit phasor, taken per microphone, so no product |X_i| |X_j| is
 *          formed that could overflow or underflow.
 *   w_f    = 1 for f = 0 and for f = n_fft / 2 when n_fft is even, 2 otherwise;  W1 = sum of w_f over the band.
 *
 * PHAT cross-spectrum:
 *   psi[b, p, f] = (1 / T) sum_t u(X_i[b, f, t]) conj(u(X_j[b, f, t]))   inside the band, exactly 0 outside it.
 * psi: device (B, P, F) complex128.  status: device (B,) int32, the bits 1 and 2 of the table below.  Two launches (one
 * workgroup a (b, f) bin, then one an item for status).  The D rows of a bin are normalised once and kept in LDS where
 * 16 D T bytes fit, and normalised again at every use otherwise; both ways give the same bits (option phat_lds = 0 forces
 * the second).  A pair's sum: lane l of a wave adds t = l, l + 64, ... rising, the 64 lane sums meet in wave_sum's
 * butterfly, and the total is divided by T. */
int alvq_phat_cross_spectra_f32(const float* X, double* psi, int* status, int B, int D, int F, int T, int f_lo, int f_hi,
                                void* stream);
int alvq_phat_cross_spectra_f64(const double* X, double* psi, int* status, int B, int D, int F, int T, int f_lo, int f_hi,
                                void* stream);

/* GCC-PHAT at the integer lags l = -L .. L (F = n_fft / 2 + 1):
 *   r[b, p, L + l] = (1 / W1) sum_f w_f Re(psi[b, p, f] e^{+j 2 pi f l / n_fft})   over the band, f rising.
 * With this sign the peak lag is (arrival at i) minus (arrival at j), in samples.  The angle is reduced exactly, as
 * 2 pi ((f l) mod n_fft) / n_fft.  r: device (B, P, 2 L + 1) float64.  0 <= L <= n_fft / 2.  One launch. */
int alvq_gcc_phat_f64(const double* psi, double* r, int B, int D, int n_fft, int L, int f_lo, int f_hi, void* stream);

/* SRP-PHAT over candidate positions.  mics: device float64, D positions (x, y, z) per item, item b at mics + b mics_stride;
 * cand: G positions per item at cand + b cand_stride (strides in doubles; 0 = one array / one grid serves every item).
 *   tau_d(q)  = |q - m_d| / c
 *   S[b, g]   = (1 / (P W1)) sum_p sum_f w_f Re(psi[b, p, f] e^{+j 2 pi f (fs / n_fft) (tau_i(q_g) - tau_j(q_g))})
 * so S = 1 for perfectly coherent arrivals from q_g.  map: device (B, G) float64; best: device (B,) int32, the arg-max of
 * the item's row with the lowest index winning ties; status: device (B,) int32 bit flags:
 *   1  a non-finite spectrogram value inside the band (seen as a non-finite psi)   map row all NaN, best -1
 *   2  every psi of the item inside the band is 0 (silence)                        map row all 0,   best -1
 *   4  a non-finite microphone or candidate coordinate of the item                 map row all NaN, best -1
 * (NaN wins where bit 2 meets bit 4.)  Nothing on the host reads status: the caller does, when it can sync.
 * How it is evaluated: a thread owns a candidate.  For every bin f of the band, rising, it holds the D phasors
 * z_d = e^{j pi x}, x = (2 f (fs / n_fft)) tau_d: from sincospi at the bins f_lo + 8 n (the anchors), and at the bins between
 * from the rotation recurrence z_d <- z_d w_d, w_d = e^{j pi (2 (fs / n_fft)) tau_d}, in fused multiply-adds.  Then
 *   s_f = sum_{i = 0}^{D - 2} Re(z_i sum_{j = i + 1}^{D - 1} psi[(i, j), f] conj(z_j))      i and j rising, fused
 *         multiply-adds, the inner sum from 0
 * and S = (sum_f w_f s_f) / (P W1), f rising from 0: an order (and anchors) that depend on (D, f_lo, f_hi) alone.  The item's
 * psi[:, band] is staged in the workgroup's LDS where 16 P F_band bytes fit and read from global memory otherwise; both
 * ways give the same bits (option phat_lds = 0 forces the second).  Three launches: status, map, arg-max.
 * Limits of all four: 1 <= B <= 65535; 2 <= D <= 8; 1 <= T <= 65535; B F <= 2^31 - 1; n_fft >= 2; G >= 1,
 * B G <= 2^31 - 1; fs, c > 0 and finite; mics_stride 0 or >= 3 D, cand_stride 0 or >= 3 G. */
int alvq_srp_phat_f64(const double* psi, const double* mics, const double* cand, double* map, int* best, int* status, int B,
                      int D, int G, int64_t mics_stride, int64_t cand_stride, double fs, int n_fft, double c, int f_lo,
                      int f_hi, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Beamforming of a microphone array's complex spectrograms (csrc/beamform.hip): D channels into one.  Delay-and-sum, MVDR
 * with a steering vector (Capon 1969; MPDR where the covariance is the observed mixture's) and MVDR from two covariances
 * (Souden, Benesty, Affes 2010).  All arithmetic is float64 (a complex64 value is widened first); only Y is rounded.  No
 * atomics, no host sync, graph-capturable; every sum runs in one order that depends on the bin's sizes alone: a bin has the
 * same bits alone, in any batch and on any run.  Every (b, f) bin is a problem of its own.
 * Limits of all: 1 <= B <= 65535, F >= 1, B F <= 2^31 - 1; 1 <= D <= 8; 1 <= T <= 65535.  Every launch caps its grid at 65536
 * workgroups and strides over the bins beyond, so every size within the limits launches.
 *   X      device (B, D, F, T) interleaved complex, T contiguous, complex64 ("_f32") or complex128 ("_f64"); D microphones.
 *
 * Spatial covariance.  mask: device (B, F, T) float64 weights m_t >= 0, or NULL: every m_t = 1.
 *   Phi[b, f][i][j] = sum_t m_t x_i[t] conj(x_j[t]) / sum_t m_t
 * Phi: device (B, F, D, D) complex128.  Only i >= j is computed: the upper triangle is written as the exact conjugate of the
 * lower, and the diagonal's imaginary part is exactly +0.  status: device (B, F) int32: 0, or 1 = a non-finite value of X in
 * the bin, a negative or non-finite mask value, or sum_t m_t = 0 (not > 0); Phi of such a bin is all zeros.
 * One launch.  A wave owns a bin where T <= 1024 (four bins a workgroup), the workgroup of four waves above that.  A thread
 * adds the frames t = l, l + 64 W, l + 128 W, ... rising (W the waves a bin has, l the lane, or the thread's index where
 * W = 4).  A frame's term: y = m_t x_i (two products), then by fused multiply-adds re += y.re x_j.re, re += y.im x_j.im,
 * im += y.im x_j.re, im -= y.re x_j.im, in that order; the diagonal has the real part alone.  The lane sums meet in wave_sum's
 * butterfly and the four wave totals are added in wave order; each total is divided by the mask's sum, which is added the
 * same way. */
int alvq_spatial_covariance_f32(const float* X, const double* mask, double* Phi, int* status, int B, int D, int F, int T,
                                void* stream);
int alvq_spatial_covariance_f64(const double* X, const double* mask, double* Phi, int* status, int B, int D, int F, int T,
                                void* stream);

/* Steering vectors of a position.  mics: device float64, D positions (x, y, z), one array for every item or (mics_batched
 * != 0) one per item, (B, D, 3); src: device (B, 3) float64.  With tau_d = |q - m_d| / c for the item's position q,
 *   A[b, d, f] = exp(-j 2 pi f (fs / n_fft) (tau_d - tau_ref))
 * evaluated as cos - j sin of pi x, x = (2 f) (fs / n_fft) (tau_d - tau_ref), by sincospi.  This is the sign of a spectrogram
 * whose channel d carries S e^{-j omega r_d / c} (tests/helpers/srp_ref.py::case), so the arg-max position of
 * alvq_srp_phat_f64 steers at its source; A[b, ref, f] = 1.  A: device (B, D, F) complex128.  status: device (B,) int32,
 * bit 4 (the bit alvq_srp_phat_f64 uses) for a non-finite coordinate of the item; its A is then all NaN.
 * 2 <= n_fft <= 2^24, F <= 2^24 (F need not be n_fft / 2 + 1); fs, c > 0 and finite; 0 <= ref < D.  One launch. */
int alvq_steering_vectors_f64(const double* mics, const double* src, double* A, int* status, int B, int D, int F, double fs,
                              int n_fft, double c, int ref, int mics_batched, void* stream);

/* Beamformer weights.  Phi_n, Phi_s: device (B, F, D, D) complex128, Hermitian (of Phi_n only the lower triangle, i >= j, and
 * the real part of its diagonal are read); A: device (B, D, F) complex128; W: device (B, F, D) complex128.
 *   Phi' = Phi_n + loading (tr Phi_n / D) I                                        (WPE's loading rule)
 *   mode 0  delay-and-sum:                w = a / D.  Phi_n and Phi_s are not read (may be NULL); status is 0.
 *   mode 1  MVDR with a steering vector:  z = Phi'^-1 a by a Cholesky factorisation and two triangular solves,
 *                                         w = z / Re(a^H z).  Phi_s is not read.  With Phi_n the mixture's covariance: MPDR.
 *   mode 2  MVDR from two covariances:    G = Phi'^-1 Phi_s (D right-hand sides), w = G[:, ref] / Re tr G.  A is not read.
 * status: device (B, F) int32: 0, or 2 = a Cholesky pivot <= 0 or not finite, or the denominator (Re(a^H z), Re tr G) <= 0
 * or not finite; such a bin gets w = e_ref, which passes the reference microphone through.
 * loading finite and >= 0; 0 <= ref < D.  One launch, a wave a bin.  tr Phi_n, Re(a^H z) = sum_r Re(conj(a_r) z_r) and
 * Re tr G are added from 0 with the index rising; the factorisation and the solves take column k = 0 .. D - 1 (the back
 * substitution D - 1 .. 0) with one subtraction per column on every entry. */
int alvq_beamform_weights_f64(const double* Phi_n, const double* Phi_s, const double* A, double* W, int* status, int B, int D,
                              int F, int mode, int ref, double loading, void* stream);

/* The beamformer's output:  Y[b, f, t] = sum_d conj(W[b, f, d]) X[b, d, f, t], d rising, starting from the first product.
 * A weight of exactly 0 adds no term (its microphone may hold anything), and a weight whose imaginary part is exactly 0
 * multiplies both parts of x as a real number; for finite values neither changes the sum's value, and w = e_ref returns
 * x_ref bit for bit, a NaN included: a bin that alvq_beamform_weights_f64 refused comes back as its reference microphone.
 * Every weight 0 gives 0.  Y: device (B, F, T) of X's type; X and Y must not overlap.  One streaming launch, a thread an
 * output. */
int alvq_beamform_apply_f32(const float* X, const double* W, float* Y, int B, int D, int F, int T, void* stream);
int alvq_beamform_apply_f64(const double* X, const double* W, double* Y, int B, int D, int F, int T, void* stream);

/* The GEV (max-SNR) beamformer and the covariance-whitening steering estimate from two covariances (Warsitz, Haeb-Umbach
 * 2007; Markovich-Golan, Gannot 2015).  Phi_n, Phi_s as above (of Phi_n the lower triangle and the real part of its diagonal
 * are read, Phi_s whole).  Per bin:
 *   Phi' = Phi_n + loading (tr Phi_n / D) I = L L^H            (the factorisation of alvq_beamform_weights_f64)
 *   C    = L^-1 Phi_s L^-H: Y = L^-1 Phi_s and then L^-1 Y^H by the same forward substitution; of the result the lower
 *          triangle and the real part of the diagonal count
 *   (lambda_max, u) = the top eigenpair of C as alvq_eigh_f64 defines it (its last column, phase rule included)
 *   v = L^-H u (back substitution),  a = L u = Phi' v (k rising from the first term)
 *   RTF = a / a_ref (as a conj(a_ref) / |a_ref|^2),  W = v conj(a_ref), so that W^H RTF = 1;  gain = lambda_max, the
 *   generalised Rayleigh quotient w^H Phi_s w / w^H Phi' w at its maximum.
 * D = 1: W = RTF = 1.  W, RTF: device (B, F, D) complex128; gain: device (B, F) float64.  status: device (B, F) int32: 0, or
 * 2 = a pivot <= 0 or not finite, lambda_max <= 0 or not finite, |a_ref|^2 = 0 or not finite, or an eigensolver status other
 * than 0; such a bin gets W = RTF = e_ref and gain = 0.  Limits as above; loading finite and >= 0; 0 <= ref < D.  One launch,
 * a wave a bin. */
int alvq_beamform_gev_f64(const double* Phi_n, const double* Phi_s, double* W, double* RTF, double* gain, int* status, int B,
                          int D, int F, int ref, double loading, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Subspace methods (csrc/subspace.hip, csrc/herm_eig.h).  Float64 throughout, no atomics, no host sync, graph-capturable.
 *
 * Eigendecomposition of n_matrices complex Hermitian matrices of order D, 1 <= D <= 8.  A: device (n, D, D) complex128, of
 * which the lower triangle (i >= j) and the real part of the diagonal are read.  Cyclic Jacobi in round-robin order: with
 * m = D rounded up to even, step s = 0 .. m - 2 of a sweep pairs index m - 1 with s and every other index i with
 * (2 s - i) mod (m - 1); a pair with an index >= D is a bye; the pairs of a step are disjoint and rotate together.  With
 * nf = ||A||_F (taken as mx sqrt(sum |a / mx|^2), mx the largest |re| or |im|), u = 2^-53, the pair p < q is rotated while
 * |a_pq| > 0.5 u nf / D:  zeta = (a_qq - a_pp) / (2 |a_pq|), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (sign(0) = 1),
 * cs = 1 / sqrt(1 + t^2), sn = cs t a_pq / |a_pq|, J = [[cs, sn], [-conj(sn), cs]] on (p, q); A <- J^H A J with a_pq = 0,
 * a_pp - t |a_pq| and a_qq + t |a_pq| set outright, V <- V J from V = I.  A sweep with no rotation ends the run; at most 16
 * sweeps.  lam: device (n, D) float64, ascending (equal values in the order of their Jacobi columns); V: device (n, D, D)
 * complex128, column k the eigenvector of lam[k], each multiplied by the unit phasor that makes its component of the
 * largest re^2 + im^2 (the lowest index on ties) real and positive.  A = 0 gives lam = 0 and V = I.
 * status: device (n,) int32: 0 converged; 1 a non-finite entry was read: lam and V are NaN; 2 the 16th sweep still
 * rotated: lam and V as they stand.  One launch: a wave a matrix (lane 8 r + c holds entry (r, c) of A and of V; rows and
 * columns travel by shuffles), four matrices a workgroup, the grid capped at 65536 workgroups with waves striding over the
 * matrices beyond.  A matrix shares nothing with its neighbours: the same bits alone, in any batch and on any run.
 * 1 <= n_matrices <= 2^31 - 1. */
int alvq_eigh_f64(const double* A, double* lam, double* V, int* status, int64_t n_matrices, int D, void* stream);

/* The MUSIC null spectrum over candidate positions.  V: device (B, F, D, D) complex128 and lam: device (B, F, D) float64 as
 * alvq_eigh_f64 writes them for the (B F) spatial covariances (ascending); mics: device float64 (D, 3), or (B, D, 3) with
 * mics_batched != 0; cand: (G, 3), or (B, G, 3) with cand_batched != 0.  With
 *   tau_d(q) = |q - m_d| / c,   a_d = e^{-j 2 pi f (fs / n_fft) tau_d}   (alvq_steering_vectors_f64's sign)
 * and e_k the K last columns of V[b, f] (the K largest eigenvalues: the signal subspace),
 *   null[b, g] = mean over the counted bins f in [f_lo, f_hi] of  1 - (1 / D) sum_k |sum_d conj(e_k[d]) a_d|^2
 * which is 0 where the steering vector lies in the signal subspace.  Sums run with the index rising (d from the first term,
 * k over the columns D - K .. D - 1, f over the band); the result is not clamped.  A bin whose D eigenvalues are all 0 (a
 * silent bin) is not counted.  The phasors come from alvq_srp_phat_f64's rotation recurrence, anchors at f_lo + 8 n included.
 * null: device (B, G) float64; best: device (B,) int32, the arg-min of the item's row, the lowest index on ties;
 * status: device (B,) int32 bit flags:
 *   1  a non-finite eigenvector entry or eigenvalue inside the band      null row all NaN, best -1
 *   2  no counted bin                                                   null row all 1,   best -1
 *   4  a non-finite microphone or candidate coordinate of the item       null row all NaN, best -1
 * Three launches: status, map (a thread a candidate, tiles of 256), arg-min.  Limits: 1 <= B <= 65535, 1 <= F <= 2^24,
 * B F <= 2^31 - 1 (F need not be n_fft / 2 + 1); 2 <= D <= 8; 1 <= K <= D - 1; G >= 1, B G <= 2^31 - 1; 2 <= n_fft <= 2^24;
 * 0 <= f_lo <= f_hi < F; fs, c > 0 and finite. */
int alvq_music_f64(const double* V, const double* lam, const double* mics, const double* cand, double* null, int* best,
                   int* status, int B, int D, int F, int G, int K, double fs, int n_fft, double c, int f_lo, int f_hi,
                   int mics_batched, int cand_batched, void* stream);

/* ------------------------------------------------------------------------------------------------
 * AuxIVA blind source separation of a microphone array's complex spectrograms (csrc/iva.hip): auxiliary-function independent
 * vector analysis with iterative projection (Ono, WASPAA 2011), the determined case K = D sources, and the ratio masks of
 * its output.  It needs no geometry and no masks, starts from W = I and is deterministic.  All arithmetic is float64 (a
 * complex64 value is widened first); only Y is rounded.  No atomics, no host sync, graph-capturable; every sum runs in one
 * order that depends on sizes alone: an item has the same bits alone, in any batch and on any run.
 * Limits: 1 <= B <= 65535, F >= 1, B F <= 2^31 - 1; 1 <= D <= 8; 1 <= T <= 65535; 0 <= iterations <= 256; 0 <= ref < D; eps
 * finite and >= 0; model 0 ("laplace") or 1 ("gauss").
 *   X, Y   device (B, D, F, T) interleaved complex, T contiguous, complex64 ("_f32") or complex128 ("_f64"); they must not
 *          overlap.  X[b, d, f, t]: microphone d; Y[b, k, f, t]: source k.
 *   W      device (B, F, D, D) complex128, the demixing matrix of every bin.  Row k extracts source k:
 *          y_k[t] = sum_d W[k][d] x_d[t], d rising, the sum starting from the first product (a complex product is
 *          (a.re b.re - a.im b.im, a.re b.im + a.im b.re), each part two rounded products and one sum).
 *   W0     device (B, F, D, D) complex128 or NULL (may be W itself).  status: device (B, F) int32.
 *
 * Start.  W = I, or W0.
 * Bin status before the first iteration.  A bin that holds a non-finite value, or nothing but zeros, gets status 1.  Such a bin
 * keeps W = I (whatever W0 holds) and Y = X bit for bit, and contributes nothing to p below.
 * One iteration:
 *   1. Source activity.  p[b, k, t] = sum_f |y_k[f, t]|^2 over the item's bins whose status is not 1, f rising, as
 *      p = fma(y.im, y.im, fma(y.re, y.re, p));  r = sqrt(p).
 *   2. Weights.  model 0 (Laplace):                 phi[k, t] = 1 / max(r, eps max_t r)        (max_t r = sqrt(max_t p))
 *                model 1 (time-varying Gaussian):   phi[k, t] = F / max(p, eps max_t p)        (F: every bin of the item)
 *      Where a source's max_t p is 0 or a p of the source is not finite, phi = 1 for that source.  eps has WPE's meaning.
 *   3. Update.  For each bin of status 0, for k = 0 .. D - 1 in this order, row k replaced before row k + 1 is computed:
 *        V_k = (1 / T) sum_t phi[k, t] x_t x_t^H.  Only i >= j is computed, above the diagonal stands the exact conjugate, and
 *              the diagonal's imaginary part is exactly +0.  A frame's term c = x_i conj(x_j) is
 *              re = fma(x_i.im, x_j.im, x_i.re x_j.re), im = x_i.im x_j.re - x_i.re x_j.im (two rounded products, so that two
 *              identical microphones give exactly 0), and it enters as acc = fma(phi, c, acc), on the diagonal the real
 *              part alone.  All D matrices V_k of an iteration depend on X and phi only, not on W.
 *        M   = W V_k, entry (r, c) = sum_j W[r][j] V_k[j][c], j rising from the first product.
 *        Solve M w = e_k by Gaussian elimination with partial pivoting: in column j = 0 .. D - 1 the pivot is the entry of
 *              the largest |z|^2 = re^2 + im^2 among the rows i >= j, the lowest row winning ties; the two rows are exchanged;
 *              row r > j loses l = M[r][j] / pivot times row j (a / p is taken as a conj(p) / |p|^2).  Back substitution
 *              j = D - 1 .. 0.
 *        q   = Re(w^H V_k w) = sum_r (w_r.re u_r.re + w_r.im u_r.im), u = V_k w with c rising, both sums from their first term.
 *        w  <- w / sqrt(q), part by part; then W[k][:] <- conj(w).
 *      A pivot whose |z|^2 is 0 or not finite gives the bin status 2, and so does a q that is <= 0 or not finite.  The bin
 *      goes back to W = I and is not updated again; it goes on contributing y = x to p.
 * After `iterations` iterations, project back (the minimal distortion principle) onto microphone ref: A = W^-1 by the same
 * elimination with the D columns of I as right-hand sides; a singular W (a pivot as above) gives status 2, W = I and Y = X.
 *   Y[b, k, f, t] = A[ref][k] y_k[f, t], the image of source k at microphone ref; sum_k Y_k = x_ref up to rounding.
 * A bin of status 1 or 2 is copied from X, bit for bit.  W is the only state carried from one iteration to the next:
 * a + b iterations give the bits of b iterations started from the W of a (where no bin has left with status 2).
 *
 * Sum orders.  p: a thread owns a frame and walks f rising.  V_k: lane l of a wave adds the frames t = l, l + 64, ... rising,
 * the 64 lane sums meet in wave_sum's butterfly, and the total is divided by T: an order that depends on T alone.
 * 1 + 4 iterations + 1 launches on the stream (status and start; activity, weights, covariances, solves; projection); status
 * is read on the device.  workspace: device, alvq_auxiva_workspace_bytes(B, D, F, T) = 8 B D T rounded up to 16, plus
 * 16 B F D^3 bytes (p, then phi over it; the D matrices V_k of every bin); -1 for sizes out of range. */
int64_t alvq_auxiva_workspace_bytes(int B, int D, int F, int T);
int alvq_auxiva_f32(const float* X, const double* W0, double* W, float* Y, int* status, void* workspace, int B, int D, int F,
                    int T, int model, int iterations, int ref, double eps, void* stream);
int alvq_auxiva_f64(const double* X, const double* W0, double* W, double* Y, int* status, void* workspace, int B, int D, int F,
                    int T, int model, int iterations, int ref, double eps, void* stream);

/* Ratio masks of K separated spectrograms.  Y: device (B, K, F, T) as above, 1 <= K <= 8.
 *   M[b, k, f, t] = |Y_k|^2 / sum_j |Y_j|^2 in float64, |z|^2 = re^2 + im^2, j rising from the first term;
 *   1 / K where the sum is 0, and 0 where the sum is not finite.
 * M: device (B, K, F, T) float64.  One elementwise launch.  M[:, k] and 1 - M[:, k] are the speech and noise masks of
 * alvq_spatial_covariance_*. */
int alvq_separation_masks_f32(const float* Y, double* M, int B, int K, int F, int T, void* stream);
int alvq_separation_masks_f64(const double* Y, double* M, int B, int K, int F, int T, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ILRMA blind source separation of a microphone array's complex spectrograms (csrc/ilrma.hip): independent low-rank matrix
 * analysis (Kitamura, Ono, Sawada, Kameoka, Saruwatari, IEEE/ACM TASLP 2016), the determined case K = D sources.  The demixing
 * update is AuxIVA's iterative projection (above, and the same kernels: csrc/iva_kernels.h); the source model is not one
 * activity per frame but, per source, a non-negative matrix of rank L over (f, t),
 *   r_k[f, t] = sum_l basis[k, f, l] activations[k, l, t],
 * fitted by multiplicative updates between the demixing updates.  All arithmetic is float64 (a complex64 value is widened
 * first); only Y is rounded.  No atomics, no host sync, graph-capturable; every sum runs in one order that depends on sizes
 * alone: an item has the same bits alone, in any batch and on any run.
 * Limits: AuxIVA's for B, D, F, T, iterations and ref; 1 <= L <= 16; floor finite and > 0.
 *   X, Y, W, W0, status   as for alvq_auxiva_*.
 *   basis0, basis               device (B, D, F, L) float64 (basis0 may be basis itself).
 *   activations0, activations   device (B, D, L, T) float64 (activations0 may be activations itself).
 * Below, floor(v) = v where v > floor and v is finite, and floor otherwise (a NaN and an infinity included); it stands where
 * the literature writes max(v, floor).
 *
 * Start.  W = I, or W0; basis = basis0 and activations = activations0, copied as they are.  There is no canonical start of the
 * model: the caller owns the randomness.
 * Bin status before the first iteration.  AuxIVA's status 1; bin f of item b also gets status 1 when basis0[b, :, f, :] holds a
 * value that is not finite or not > 0, and every bin of item b gets it when activations0[b] holds such a value.  A bin of
 * status 1 keeps W = I (whatever W0 holds) and Y = X bit for bit, its rows basis[b, :, f, :] come back as they were given, on
 * whichever account the bin was refused and after any number of iterations, and it stays out of every sum over f below.
 * One iteration:
 *   1. Power.  In every bin whose status is not 1 (a bin of status 2 has W = I), y = W x as AuxIVA's activity pass takes it and
 *      P[k, f, t] = fma(y.im, y.im, y.re y.re).  s[k, f] = sum_t P; lam[k] = (sum_f s[k, f]) / (F' T) over those bins, f rising
 *      from 0.0, F' their number, the divisor the rounded product of the two; lam[k] = 1 where that is not finite or not > 0.
 *   2. Normalise, so that floor is on a known scale.  In the bins of status 0, W[k][d] <- W[k][d] / sqrt(lam[k]), part by
 *      part; in the bins whose status is not 1, P <- P / lam[k] and basis[k, f, l] <- floor(basis[k, f, l] / lam[k]).  The cost
 *      sum_{f, t, k} (P / R + log R) - 2 T sum_f log |det W_f| does not change under this step where the floor is not active.
 *   3. Basis.  In the bins whose status is not 1: R[k, f, t] = floor(sum_l basis[k, f, l] activations[k, l, t]), l rising from
 *      the first product, every product rounded; i = 1 / R; g = (P i) i;
 *        num[l] = sum_t g activations[k, l, t],  den[l] = sum_t i activations[k, l, t],  each term entering by fma;
 *        basis[k, f, l] <- floor(basis[k, f, l] sqrt(num[l] / den[l])); where the ratio is not finite, floor(basis[k, f, l]).
 *   4. Activations.  For every (k, t), R, i and g recomputed from the new basis:
 *        num[l] = sum_f g basis[k, f, l],  den[l] = sum_f i basis[k, f, l] over the bins whose status is not 1, f rising;
 *        activations[k, l, t] <- floor(activations[k, l, t] sqrt(num[l] / den[l])); where the ratio is not finite (an item
 *        without such a bin has 0 / 0), floor(activations[k, l, t]).  So no value that is not finite stays in the activations
 *        after an iteration, nor in the basis rows of a bin whose status is not 1.
 *   5. Demixing matrices.  R recomputed from the new factors.  Each bin of status 0 gets step 3 of AuxIVA to the letter with
 *      phi[k, t] replaced by 1 / R[k, f, t]: V_k, the elimination, q, the normalisation, the rows replaced in the order
 *      k = 0 .. D - 1, and the same rule for status 2.
 * After `iterations` iterations the projection onto microphone ref is AuxIVA's.  iterations = 0 returns the start -- W = I in a
 * bin of status 1 -- and its projection.  (W, basis, activations) is the only state carried from one iteration to the next:
 * a + b iterations give the bits of b iterations started from the W, basis and activations of a.
 *
 * Sum orders.  s, and num and den of step 3: lane l of a wave adds the frames t = l, l + 64, ... rising and the 64 lane sums
 * meet in wave_sum's butterfly: an order that depends on T alone.  lam, and num and den of step 4: one thread walks f rising.
 * 3 + 7 iterations + 1 launches on the stream (status and start of W, of the activations, of the basis; power, lam, basis,
 * activations, weights, covariances, solves; projection); status is read on the device.  workspace: device,
 * alvq_ilrma_workspace_bytes(B, D, L, F, T) = 8 B D F T + 16 B F D^3 + 8 B D F + 8 B D + 4 B bytes, each term rounded up to 16
 * (P, then 1 / R over it; the matrices V_k; s; lam; the items' flags); -1 for sizes out of range. */
int64_t alvq_ilrma_workspace_bytes(int B, int D, int L, int F, int T);
int alvq_ilrma_f32(const float* X, const double* W0, const double* basis0, const double* activations0, double* W, double* basis,
                   double* activations, float* Y, int* status, void* workspace, int B, int D, int L, int F, int T, int iterations,
                   int ref, double floor, void* stream);
int alvq_ilrma_f64(const double* X, const double* W0, const double* basis0, const double* activations0, double* W, double* basis,
                   double* activations, double* Y, int* status, void* workspace, int B, int D, int L, int F, int T, int iterations,
                   int ref, double floor, void* stream);

/* ------------------------------------------------------------------------------------------------
 * cACGMM spatial clustering of a microphone array's complex spectrograms (csrc/cacgmm.hip): the complex angular central
 * Gaussian mixture model (Ito, Araki, Nakatani, EUSIPCO 2016), fitted by EM.  It gives the time-frequency masks of K classes --
 * talkers and diffuse noise alike -- from D microphones, K and D independent: what the mask-driven beamformers take where AuxIVA
 * (K = D, no noise class) does not apply.  All arithmetic is float64 (a complex64 value is widened first).  No atomics, no host
 * sync, graph-capturable; every sum runs in one order that depends on sizes alone: an item has the same bits alone, in any batch
 * and on any run.  There is no frequency permutation alignment inside: the priors are shared over frequency and stand in for it
 * (alvq_align_permutations_f64 below repairs masks whose classes come out in a different order in every bin).
 * Limits: 1 <= B <= 65535, F >= 1, B F <= 2^31 - 1; 2 <= D <= 8; 1 <= K <= 8; 1 <= T <= 65535; 1 <= iterations <= 256;
 * 0 <= floor <= 1.
 *   X          device (B, D, F, T) interleaved complex, T contiguous, complex64 ("_f32") or complex128 ("_f64").
 *   init       device (B, K, F, T) float64: gamma at the start (may be masks itself).
 *   quadratic0 device (B, K, F, T) float64 or NULL: q at the start (may be quadratic itself); NULL: q = 1.
 *   masks      device (B, K, F, T) float64: gamma after the last iteration; it sums to 1 over k up to rounding.
 *   prior      device (B, K, T) float64: the priors of the last iteration.
 *   cov        device (B, F, K, D, D) complex128: the normalised class matrices of the last iteration.
 *   quadratic  device (B, K, F, T) float64: q after the last iteration.  status: device (B, F) int32.
 *
 * Start.  A bin (b, f) gets status 1 if it holds a value of X that is not finite, a frame whose n is not finite, an init value
 * that is negative or not finite, or a quadratic0 value that is not > 0 and finite.  n[f, t] = |x|^2 = sum_d (re^2 + im^2), d
 * rising from 0, each term two rounded products and their sum.  Such a bin emits masks = 1 / K, cov = I and quadratic = 1 and never
 * contributes to the priors.  gamma = init as it is (no renormalisation) and q = quadratic0, or 1.
 * The model is one of the directions z[f, t] = x / sqrt(n).  z is never formed: z z^H = x x^H / n and |v^H z|^2 = |v^H x|^2 / n.
 * A frame with n == 0 is silent: it has weight 0 in both sums of step 2, and step 3 leaves it gamma[k] = prior[k, t], q = 1.
 * (An n so small that x_i conj(x_j) underflows loses the frame's direction; scale such an input first.)
 * One iteration:
 *   1. Priors.  prior[b, k, t] = (sum_f gamma[b, k, f, t]) / F0 over the item's bins of status 0, f rising from 0.0; F0 is
 *      their number.  1 / K where F0 = 0.
 *   2. M-step.  For each bin of status 0 and each class k:
 *        sg  = sum_t gamma[t] over the frames that are not silent.
 *        S   = sum_t w[t] x_t x_t^H with w = gamma / (q n), 0 for a silent frame.  Only i >= j is computed.  A frame's term
 *              c = x_i conj(x_j) is re = fma(x_i.im, x_j.im, x_i.re x_j.re), im = x_i.im x_j.re - x_i.re x_j.im (two rounded
 *              products), and it enters as acc = fma(w, c, acc), on the diagonal the real part alone.
 *        B_k = (D S) / sg, entry by entry and part by part; above the diagonal stands the exact conjugate and the diagonal's
 *              imaginary part is +0.  Where sg is not > 0, B_k = I.
 *        B_k = V diag(lambda) V^H by the cyclic Jacobi method of alvq_eigh_f64, lambda ascending (ties in Jacobi's column order).
 *        lambda_i <- max(lambda_i, floor lambda_max);  s = sum_i lambda_i, i rising from the first;  lambda_i <- (lambda_i D) / s;
 *        logdet_k = sum_i log lambda_i, i rising from the first.
 *        cov[b, f, k][r][c] = sum_i lambda_i (V[r][i] conj(V[c][i])), i rising from the first term, the product's parts as in
 *              c above (two rounded products each): exactly Hermitian.
 *      The solver's status, or a lambda_max that is not > 0 and finite, gives the bin status 2 in the same iteration: from
 *      then on it is treated like a bin of status 1 (it has contributed to the priors of this iteration, and to no later ones).
 *   3. E-step.  For each bin of status 0 and each frame, with a_i = conj(v_i) / sqrt(lambda_i), part by part:
 *        y_i = sum_d a_i[d] x_d, d rising from the first product (a complex product is (a.re b.re - a.im b.im,
 *              a.re b.im + a.im b.re));  q_k = max((sum_i |y_i|^2) / n, 2^-1022), i rising from 0, |y|^2 = re^2 + im^2;
 *        l_k = (log prior[k, t] - logdet_k) - D log q_k;  m = max_j l_j;
 *        gamma_k = exp(l_k - m) / sum_j exp(l_j - m), j rising from 0; 1 / K where m = -inf (no class has a prior).
 *      q = q_k is stored next to gamma.  A silent frame: gamma_k = prior[k, t], q = 1.
 * After `iterations` iterations masks = gamma and quadratic = q; gamma and q are the only state carried from one iteration to
 * the next, so a + b iterations give the bits of b iterations started from the masks and quadratic of a (where no bin has left
 * with status 2).
 *
 * Sum orders.  Priors: a thread owns a frame and walks f rising.  S and sg: lane l of a wave adds the frames t = l, l + 64, ...
 * rising, the 64 lane sums meet in wave_sum's butterfly: an order that depends on T alone.
 * 1 + 4 iterations launches on the stream (status and start; priors, class matrices, decompositions, E-step); status is read
 * on the device.  workspace: device, alvq_cacgmm_workspace_bytes(B, D, K, F, T) = 16 B F K D^2 + 8 B F K + 8 B K T bytes (B_k and
 * then the matrix a of every class of every bin, their logdets, the logarithms of the priors); -1 for sizes out of range. */
int64_t alvq_cacgmm_workspace_bytes(int B, int D, int K, int F, int T);
int alvq_cacgmm_f32(const float* X, const double* init, const double* quadratic0, double* masks, double* prior, double* cov,
                    double* quadratic, int* status, void* workspace, int B, int D, int K, int F, int T, int iterations,
                    double floor, void* stream);
int alvq_cacgmm_f64(const double* X, const double* init, const double* quadratic0, double* masks, double* prior, double* cov,
                    double* quadratic, int* status, void* workspace, int B, int D, int K, int F, int T, int iterations,
                    double floor, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Frequency permutation alignment of a per-bin separation (csrc/permutation_align.hip): the first, global stage of Sawada,
 * Araki, Makino, "Underdetermined convolutive blind source separation via frequency bin-wise clustering and permutation
 * alignment" (IEEE TASLP 2011).  A separation that is right inside every bin but orders its sources differently from bin to bin
 * is repaired by the observation that source k has the same on/off pattern over time in every bin: the time profiles of the
 * classes of each bin are correlated against per-source centroids, each bin takes the permutation that correlates best, and the
 * centroids are rebuilt.  All arithmetic is float64.  No floating-point atomics, no host sync, graph-capturable; every sum runs
 * in one order that depends on sizes alone: an item has the same bits alone, in any batch, on any run and in any replay.
 * Limits: 1 <= B <= 65535, F >= 1, B F <= 2^31 - 1; 1 <= K <= 8; 2 <= T <= 65535; 1 <= iterations <= 256.
 *   profile  device (B, K, F, T) float64, T contiguous: P[b, j, f, t], the time profile of class j of bin f -- masks, powers,
 *            log-powers: any finite reals.
 *   perm0    device (B, F, K) int32 or NULL: the start; NULL: the identity.  It must not overlap perm.
 *   perm     device (B, F, K) int32: perm[b, f, k] = the class of bin f that is source k.  The only state.
 *   score    device (B, F) float64: the winner's total in the last iteration.
 *   changed  device (B,) int32: the number of bins of status 0 whose perm differs before and after the LAST iteration; 0 at a
 *            fixed point.  status: device (B, F) int32.
 *
 * Status.  A bin (b, f) with a value of P[b, :, f, :] that is not finite, or whose perm0[b, f, :] is not a permutation of
 * 0..K-1, gets status 1: perm = the identity, score = NaN; it stays out of every centroid and is never updated.  Every other
 * bin has status 0.
 * Rows.  For every row (b, j, f) of a bin of status 0: m = (sum_t P) / T;  v = sum_t (P - m)^2, each term a rounded difference
 * squared;  rn = 1 / sqrt(v) where v > 0 and finite, else 0 (a constant row carries no evidence);
 * u[j, f, t] = (P - m) rn, a rounded difference times rn.  u is never stored: (m, rn) is, 16 bytes a row.
 * One iteration (Jacobi: every bin is scored against the same centroids, so the order in which bins are visited is immaterial):
 *   1. c[b, k, t] = sum_f u[perm[b, f, k], f, t] over the item's bins of status 0, f rising, the sum starting from the first
 *      term; 0 for an item without one.
 *   2. n_k = sqrt(sum_t c^2);  c <- c / n_k where n_k > 0 and finite, else c <- 0.
 *   3. Per bin of status 0: table[k, j] = sum_t c[k, t] u[j, f, t], each term a rounded product.  The new perm[b, f, :] is the
 *      winner of alvq_assign_f64's rule on that K x K table with maximize != 0 (lexicographic rank, NaN scores skipped, the
 *      lowest rank among equal scores) and score[b, f] its total.  If every permutation was skipped the old perm stays, the
 *      score is NaN and the bin counts as unchanged.
 * perm is the only state, so a + b iterations give the perm, score and changed of b iterations started from the perm of a.
 * Nothing reads a status on the host.
 *
 * Sum orders.  Every sum over t -- of the rows, of c^2 and of the table -- is the same: thread i of a workgroup of 256 adds the
 * frames t = i, i + 256, ... rising from +0.0, then block_sum<kSequential, true> of csrc/block_reduce.h (wave_sum's butterfly,
 * the four waves in order from the first): an order that depends on T alone.  The sum over f: a thread owns a frame and walks f
 * rising, exactly as written above.
 * 1 + 3 iterations + 1 launches on the stream (status, row statistics and start; centroids, their norms, scores; changed).
 * workspace: device, alvq_align_workspace_bytes(B, K, F, T) = 16 B K F + 8 B K T + 4 B F bytes ((m, rn) of every row, the
 * centroids, a changed flag a bin); -1 for sizes out of range. */
int64_t alvq_align_workspace_bytes(int B, int K, int F, int T);
int alvq_align_permutations_f64(const double* profile, const int* perm0, int* perm, double* score, int* changed, int* status,
                                void* workspace, int B, int K, int F, int T, int iterations, void* stream);

/* out[b, k, f, t] = x[b, perm[b, f, k], f, t] for x and out device (B, K, F, T), T contiguous, of elements of elem_bytes = 4, 8
 * or 16 bytes (float32; float64 / complex64; complex128), and perm device (B, F, K) int32 as alvq_align_permutations_f64 gives
 * it: a pure copy, coalesced over t, in units of the widest of 16, 8 and 4 bytes that divides a row.  An entry of perm outside
 * 0..K-1 is not read as an index: such a bin passes through unpermuted.  out must not overlap x.  Limits as above, T >= 1. */
int alvq_permute_bins(const void* x, const int* perm, void* out, int B, int K, int F, int T, int elem_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exact t-SNE (sklearn.manifold.TSNE(method="exact", n_components=2) semantics; the contract in full: the docstring of
 * acoustic_locating_vq_vae/tsne.py).  2 <= N <= 65536 points, 1 <= L <= 4096 codes per point; every N x N matrix is
 * row-major fp32 with 64-bit element offsets.  Fixed-order sums, no atomics: bitwise reproducible.
 *
 * Code distances: d2[i][j] = 2 * (L - #{l : codes[i][l] == codes[j][l]}), the squared Euclidean distance of the one-hot
 * expansions (exact; zero diagonal).  codes: int32 (N, L). */
int alvq_tsne_code_sqdist_f32(const int32_t* codes, float* d2, int N, int L, void* stream);

/* Joint affinities, in place: P (N, N) holds distances on entry (used as given, the diagonal ignored) and the joint P on
 * return.  Per row, a binary search in fp64 for beta (from 1, <= 100 steps, |H - log(perplexity)| <= 1e-5) makes the
 * conditional P_ij = exp(-d_ij beta_i) / S_i; then P = (Pc + Pc^T) / max(sum, eps) clamped to >= eps off the diagonal
 * (eps = 2^-52), exactly symmetric, diagonal 0.  beta, S: (N) doubles out, the beta and sum of each row's last evaluation.
 * 0 < perplexity < N.  workspace: alvq_tsne_affinities_workspace_bytes(N) = (N + 1) * 8 bytes; -1 for N out of range. */
int64_t alvq_tsne_affinities_workspace_bytes(int N);
int alvq_tsne_affinities_f32(float* P, double* beta, double* S, void* workspace, int N, double perplexity, void* stream);

/* n_iter >= 1 iterations of one descent phase on the embedding Y (N, 2) fp64, in place, with the phase's state update and
 * gains (N, 2) fp64 (the caller zeroes / sets them to 1 at the start of a phase):
 *   num_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} num_ij, Q_ij = max(num_ij / Z, eps);
 *   grad_i = 4 sum_{j != i} (e P_ij - Q_ij) num_ij (y_i - y_j)             (e = exaggeration, every y of the iteration's start)
 *   gains += 0.2 where update * grad < 0, else gains *= 0.8; gains >= 0.01; grad *= gains;
 *   update = momentum * update - learning_rate * grad;  Y += update.
 * grad (N, 2) out: the gained gradient of the last iteration.  stats (2 doubles) out, of the last iteration:
 * KL = sum_{i != j} e P_ij log(max(e P_ij, eps) / Q_ij) and |grad|.  3 * n_iter + 2 launches (and, for odd n_iter, one
 * device-to-device copy) on stream, no host sync.  workspace: alvq_tsne_descend_workspace_bytes(N) = (5N + 1) * 8 bytes. */
int64_t alvq_tsne_descend_workspace_bytes(int N);
int alvq_tsne_descend_f64(const float* P, double* Y, double* update, double* gains, double* grad, double* stats, void* workspace,
                          int N, int n_iter, double exaggeration, double momentum, double learning_rate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * k-means (sklearn.cluster.KMeans(algorithm="lloyd") semantics; the contract in full: the docstring of
 * acoustic_locating_vq_vae/kmeans.py).  x (N, D) fp32 rows, centres (K, D) fp32; N < 2^30, K <= 16384, D <= 512.  The
 * assignment step is alvq_vq_argmin_f32.  Fixed-order fp64 sums, no floating-point atomics: bitwise reproducible.
 *
 * One Lloyd update from labels (int64, in [0, K)) assigned with centers_old: the rows sorted by label stably (counts,
 * exclusive scan, stable scatter), each cluster's rows summed in fp64 in row order (segments of 128 rows, in order),
 * empty clusters relocated (sklearn's _relocate_empty_clusters_dense: distances to the OLD centre of each row's label; the
 * farthest rows, distance descending and ties to the lower row, go to the empty clusters in ascending order; nothing
 * moves when the largest distance is 0), centers_new = fl32(sum * (1 / count)) (an empty cluster keeps its sum).
 * labels_old may be NULL (no previous labels).  counts (K) int32 out, may be NULL.  stats[0] = center_shift_tot =
 * sum_k |c_new - c_old|^2.  flags[0] = 1 labels unchanged since labels_old, 2 center_shift_tot <= tol, 0 otherwise;
 * flags[1] labels changed, flags[2] empty clusters before relocation, flags[3] clusters relocated.  9 launches, no host
 * sync.  workspace: alvq_kmeans_update_workspace_bytes(N, K, D) bytes (-1 out of range). */
int64_t alvq_kmeans_update_workspace_bytes(int64_t N, int K, int D);
int alvq_kmeans_update_f32(const float* x, const int64_t* labels, const int64_t* labels_old, const float* centers_old,
                           float* centers_new, int32_t* counts, double* stats, int32_t* flags, void* workspace,
                           int64_t N, int K, int D, double tol, void* stream);

/* inertia[0] = sum_n |x_n - c_{labels_n}|^2 in fp64.  workspace: alvq_kmeans_inertia_workspace_bytes(N) bytes. */
int64_t alvq_kmeans_inertia_workspace_bytes(int64_t N);
int alvq_kmeans_inertia_f32(const float* x, const int64_t* labels, const float* centers, double* inertia, void* workspace,
                            int64_t N, int K, int D, void* stream);

/* Column statistics: mean (D) = fl32 of the fp64 column means; var_mean[0] = mean over d of the fp64 column variances
 * (sum (x - mean)^2 / N).  workspace: alvq_kmeans_col_stats_workspace_bytes(N, D) bytes. */
int64_t alvq_kmeans_col_stats_workspace_bytes(int64_t N, int D);
int alvq_kmeans_col_stats_f32(const float* x, float* mean, double* var_mean, void* workspace, int64_t N, int D, void* stream);

/* y[n][d] = x[n][d] + alpha * v[d] (fp32; y may alias x). */
int alvq_kmeans_add_rows_f32(const float* x, const float* v, float* y, int64_t N, int D, float alpha, void* stream);

/* EMA codebook (VectorQuantizerEMA).  Per-code statistics of one step: counts[k] = #rows with idx == k and sums[k][:] = the
 * sum of those rows, accumulated in fp64 in row order (the Lloyd update's sort: counts, scan, stable scatter, 128-row
 * segments summed in order) and rounded once to fp32.  Every code is written (zeros for an unused one).  idx int64 in
 * [0, K); N < 2^24 (fp32 counts are exact), K <= 16384, D <= 512.  5 launches, no floating-point atomics, no host sync.
 * workspace: alvq_vq_ema_stats_workspace_bytes(N, K, D) bytes (-1 out of range). */
int64_t alvq_vq_ema_stats_workspace_bytes(int64_t N, int K, int D);
int alvq_vq_ema_stats_f32(const float* x, const int64_t* idx, float* counts, float* sums, void* workspace, int64_t N, int K,
                          int D, void* stream);

/* The EMA update, in order (fp64 arithmetic, fp32 state):  1. cs = decay*cs + (1-decay)*counts;  2. n = sum_k cs (fixed
 * order);  3. cs = (cs + eps) / (n + K*eps) * n (stored);  4. W = decay*W + (1-decay)*sums;  5. codebook = W / cs[:, None].
 * cluster_size (K), ema_w and codebook (K, D) are updated in place.  skip (nullable): a device float; non-zero leaves all
 * three untouched (the Trainer's skip slot).  0 < decay < 1, epsilon > 0.  2 launches, no host sync. */
int alvq_vq_ema_update_f32(const float* counts, const float* sums, float* cluster_size, float* ema_w, float* codebook,
                           const float* skip, int K, int D, double decay, double epsilon, void* stream);

/* Dead-code restarts of the EMA codebook (VectorQuantizerEMA(dead_code_threshold > 0)), csrc/vq_restart.hip.
 * Candidates: cand[s][:] = x[rows[s / stride]][:] for every slot s < R with s % stride == first (0 <= first < stride); the
 * other slots are not written (under data parallelism rank r of W fills the slots s % W == r and the step's all-reduce adds
 * zeros to them).  x (N, D) fp32, rows int64 with at least ceil((R - first) / stride) entries, cand (R, D) fp32.  A position
 * outside [0, N) leaves its slot zero and raises bit 1 of *status (a device int the caller reads when it can sync).
 * D <= 512, R <= 16384.  1 launch, no host sync. */
int alvq_vq_restart_gather_f32(const float* x, const int64_t* rows, float* cand, int* status, int64_t N, int D, int R, int first,
                               int stride, void* stream);

/* The restart, after alvq_vq_ema_update_f32 and on the values it stored:  1. dead = the codes k with cluster_size[k] <
 * threshold (fp32 compare), ascending;  2. n = min(#dead, R); for j < n and k = dead[j]: codebook[k] = cand[j], ema_w[k] =
 * fl32(cand[j] * threshold), cluster_size[k] = threshold;  3. counters[0] += n, counters[1] = #dead (before the cap).
 * Nothing else is written: copies and one fp32 product.  counters: device int64[2].  skip (nullable): a device float;
 * non-zero leaves everything untouched, the counters included.  K <= 16384, D <= 512, 1 <= R <= K, threshold >= 0.
 * 1 launch (one workgroup: the dead list stays in LDS), no workspace, no host sync. */
int alvq_vq_restart_dead_f32(const float* cand, float* cluster_size, float* ema_w, float* codebook, const float* skip,
                             int64_t* counters, int K, int D, int R, float threshold, void* stream);

/* Greedy k-means++ (sklearn's _kmeans_plusplus): centre 0 = x[first]; closest_dist_sq in fp64; per round c >= 1, T
 * candidates r_t = uniforms[c-1][t] * current_pot found in the blocked fp64 inclusive cumsum of closest_dist_sq (first
 * entry >= r_t, clipped to N - 1), their fp64 distances to every row, min with closest_dist_sq, the candidate of least
 * potential (lowest t on ties) kept.  uniforms (K-1, T) fp64 in [0, 1) (may be NULL for K = 1); centers (K, D) and
 * indices (K) int64 out.  3 launches a round, no host sync.  1 <= T <= 16, K <= N.
 * workspace: alvq_kmeans_plusplus_workspace_bytes(N, T) bytes. */
int64_t alvq_kmeans_plusplus_workspace_bytes(int64_t N, int T);
int alvq_kmeans_plusplus_f32(const float* x, const double* uniforms, float* centers, int64_t* indices, void* workspace,
                             int64_t N, int K, int D, int T, int64_t first, void* stream);

/* ================================================================================================
 * bf16 throughput path (BASELINE configs[1]: "batch=64 bf16").  Storage bf16, accumulation fp32.
 *
 * Activations live in the "NLC-padded" layout: a bf16 matrix act[rows][Cp] with channels contiguous,
 *   row(b,l) = 1 + b*(L+1) + l,   rows = alvq_nlc_rows(B,L) (rounded up to 128),   Cp = alvq_nlc_channels(C),
 * row 0, the row after each sample, rows past the batch and channels >= C are zero.  The caller allocates
 * alvq_nlc_guard_rows() readable rows before row 0 and after the last row; pointers passed below point at row 0.
 * ============================================================================================== */
int64_t alvq_nlc_rows(int B, int L);
int alvq_nlc_channels(int C);
int alvq_nlc_guard_rows(void);

/* Re-pack an fp32 weight into the K-contiguous bf16 image the kernels read: wp[tap][Mp128][Cp] = A_t[m][c]
 * (A_t as defined for alvq_conv1d_f32; zero padded).  wp holds alvq_packed_weight_elems(M,C,KW) bf16 values. */
int64_t alvq_packed_weight_elems(int M, int C, int KW);
int alvq_pack_weight_bf16(const float* w, void* wp, int M, int C, int KW, int w_layout, void* stream);

/* The same for n weights in one launch (a train step re-packs every conv weight, in the forward and in the
 * data-gradient layout, after each optimiser update: one launch instead of ~20).  `descs` is a HOST array; it is
 * copied into the kernel argument, so the call can be captured into a hipGraph.  planes = 1: bf16 images;
 * planes = 2: the hi + lo images of the split-bf16 path (as alvq_pack_weight_bf16x3); planes = 3: the H + Q images of
 * the f16mx path (two images of alvq_packed_weight_elems 2-byte units each, weight-class scale).
 * Every wp must be 16-byte aligned (the images are written in 16-byte runs): a descriptor whose image is not is refused
 * with ALVQ_EINVAL, naming the descriptor, before anything is launched. */
typedef struct alvq_pack_desc {
  const float* w;   /* fp32 weight, (M,C,KW) for ALVQ_W_OIK or (C,M,KW) for ALVQ_W_IOK */
  void* wp;         /* packed image(s): planes * alvq_packed_weight_elems(M,C,KW) bf16 values */
  int32_t M, C, KW, w_layout;
} alvq_pack_desc;
int alvq_pack_weights_bf16_batch(const alvq_pack_desc* descs, int n, int planes, void* stream);

/* Adam + packing in one pass (scripts/train_speech.py:154 + the re-pack above): for each conv weight (fp32, native
 * layout (dim0, dim1, KW), with its gradient and Adam moments) apply torch.optim.Adam's update -- the arithmetic of
 * alvq_adam_dev_f32, bit for bit, scalars = {lr/bias_correction1, sqrt(bias_correction2), grad_scale} on the device -- and
 * write the updated weight's packed image read as OIK (wp_oik: M = dim0, C = dim1) and / or as IOK (wp_iok: C = dim0,
 * M = dim1, taps flipped) while the new values are in registers.  Images must have been packed in full once before
 * (their padding is not rewritten).  planes as in alvq_pack_weights_bf16_batch.  descs: HOST array.
 * w, g, m, v and every non-NULL image must be 16-byte aligned (full tiles are read and written with 16-byte vectors, the
 * images in 16-byte runs): a descriptor with a pointer that is not is refused with ALVQ_EINVAL, naming the descriptor,
 * before anything is launched. */
typedef struct alvq_adam_pack_desc {
  float* w; const float* g; float* m; float* v;
  void* wp_oik; void* wp_iok;      /* either may be NULL */
  int32_t dim0, dim1, KW;
} alvq_adam_pack_desc;
int alvq_adam_pack_batch(const alvq_adam_pack_desc* descs, int n, int planes, const float* scalars,
                         float beta1, float beta2, float eps, const float* skip, void* stream);
/* alvq_adam_dev_f32 over the nseg element ranges [lo[i], hi[i]) of flat buffers, one launch (lo / hi: HOST arrays): the
 * parameters alvq_adam_pack_batch does not own (biases, the codebook). */
int alvq_adam_segments_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                           const int64_t* lo, const int64_t* hi, int nseg, const float* scalars,
                           float beta1, float beta2, float eps, const float* skip, void* stream);

/* Input boundary for a source whose CHANNEL axis is already contiguous (round 4; SURVEY 8(b) "element strides of x"):
 * x is (B, L, C) fp32 contiguous -- i.e. the model input (B, C, L) handed over as `t.permute(0, 2, 1)` of a contiguous t,
 * which is what scripts/train_rir.py:45 and scripts/train_echoed_speech.py:66 do -- and y the NLC-padded activation in format
 * fmt (1 bf16, 2 bf16x3 hi + lo planes, 3 f16mx H + Q planes): y[row(b,l)][c] = x[b][l][c], no transposition in either
 * direction.  standardise != 0 fuses train_rir.py:43-44 into the same pass: per (b, c) the mean and the UNBIASED std over l,
 * (v - mean) / (std + 1e-8), in alvq_standardise_f32's arithmetic and summation order (bit-identical to standardise ->
 * transpose -> convert); requires 2 <= L <= alvq_rows_to_nlc_max_std_rows().  take_abs applies |.| first. */
int alvq_rows_to_nlc(const float* x, void* y, int B, int C, int L, int fmt, int standardise, int take_abs, void* stream);
int alvq_rows_to_nlc_max_std_rows(void);

/* (B,C,L) fp32 -> NLC-padded bf16 (the boundary conversion for x, quantized and incoming gradients). */
int alvq_ncl_to_nlc_bf16(const float* x, void* y, int B, int C, int L, void* stream);

/* NLC-padded bf16 -> (B,C,L) fp32. */
int alvq_nlc_to_ncl_f32(const void* x, float* y, int B, int C, int L, void* stream);

/* out = t > 0 ? dy : 0 over n bf16 elements (n % 8 == 0). */
int alvq_relu_mask_bf16(const void* dy, const void* t, void* out, int64_t n, void* stream);

/* Same fused convolution as alvq_conv1d_f32 on NLC-padded bf16 operands and a packed weight.  Exactly one of
 * y (NLC bf16, row stride alvq_nlc_channels(M)) and y_ncl ((B,M,L) fp32, bias-only epilogue) is non-NULL.
 * Sign bits (both optional, NLC output only): a byte per 8 consecutive channels of a row,
 * bits[row * alvq_nlc_channels(M) / 8 + m / 8], bit (m % 8) = (value > 0); alvq_nlc_rows(B,L) * alvq_nlc_channels(M) / 8
 * bytes.  relu_bits_out receives the signs of the stored y, so that the data-gradient launch that later needs
 * "* (y > 0)" can pass them as mask_bits (instead of `mask` = the tensor itself) and read 1/16 of the bytes. */
int alvq_conv1d_bf16(const void* x, const void* wp, const float* bias, const void* skip1, const void* skip2,
                     const void* mask, const void* post, void* y, void* y2, float* y_ncl,
                     int B, int C, int M, int L, int KW, int relu, const void* mask_bits, void* relu_bits_out,
                     void* stream);

/* Weight (and bias) gradient from NLC-padded bf16 dy [rows][Mp] and x [rows][Cp]; fp32 result in the weight's
 * native layout, same contract as alvq_conv1d_wgrad_f32. */
int64_t alvq_conv1d_wgrad_bf16_workspace_bytes(int B, int C, int M, int L, int KW);
int alvq_conv1d_wgrad_bf16(const void* dy, const void* x, float* dw, float* dbias, void* workspace,
                           int B, int C, int M, int L, int KW, int w_layout, int accumulate, void* stream);

/* The same weight gradient summed over nseg (1..4) operand pairs of identical shape in ONE launch:
 * dw (+)= sum_i wgrad(dy[i], x[i]).  This is how the R uses of a shared residual weight (residual_stack.py:40-41)
 * are accumulated: one longer contraction and one split reduction instead of R.  dy / x are HOST arrays of device
 * pointers; no bias gradient (those layers have none).  Workspace: alvq_conv1d_wgrad_bf16_workspace_bytes. */
int alvq_conv1d_wgrad_bf16_multi(const void* const* dy, const void* const* x, int nseg, float* dw, void* workspace,
                                 int B, int C, int M, int L, int KW, int w_layout, int accumulate, void* stream);
/* Host-only: the number of split partials (each KW*M*C floats at the start of `workspace`) a launch over nseg segments
 * writes; never more than alvq_conv1d_wgrad_*_workspace_bytes sizes for any nseg in 1..4 (the launch re-checks it).
 * with_bias: the single-segment launch that also produces dbias.  -1 for unsupported arguments. */
int alvq_conv1d_wgrad_bf16_splits(int B, int C, int M, int L, int KW, int nseg, int with_bias);

/* Deferred, batched split reduction (bf16 / fp16 family).  With accumulate = ALVQ_WGRAD_DEFER the four weight-gradient
 * entry points of the family launch the contraction only: dw / dbias are not touched (dw may be NULL), the
 * alvq_conv1d_wgrad_bf16_splits(...) partials stay at the start of `workspace` ([split][KW][M][C] fp32) and, for the
 * single-segment launch with dbias != NULL, the bias partials ([split][pad64(M)] fp32) at
 * workspace + alvq_conv1d_wgrad_bf16_bias_offset(...).  The caller gives every deferred launch its OWN workspace and later
 * sums all of them with ONE alvq_wgrad_reduce_batch launch: per descriptor  dst (+)= scale * sum_s partial[s]  in split
 * order -- the same sums in the same order as the immediate reduction (bitwise identical), as one launch that fills the
 * chip instead of one small bandwidth-bound launch per layer.  A bias reduction is the descriptor
 * {KW = 1, M = 1, C = channels, w_layout = ALVQ_W_OIK, stride = pad64(channels)}.  descs: HOST array. */
#define ALVQ_WGRAD_DEFER 2
int64_t alvq_conv1d_wgrad_bf16_bias_offset(int B, int C, int M, int L, int KW);
typedef struct alvq_reduce_desc {
  const float* partial;   /* [splits][stride] */
  float* dst;             /* weight gradient in its native layout (w_layout), or a bias gradient */
  const float* scale;     /* device scalar multiplied into the sum (undoes a loss scale), or NULL */
  int32_t splits, KW, M, C, w_layout, accumulate;
  int64_t stride;         /* elements between consecutive partials: KW * M * C, or the padded length of bias partials */
} alvq_reduce_desc;
int alvq_wgrad_reduce_batch(const alvq_reduce_desc* descs, int n, void* stream);

/* ================================================================================================
 * Split-bf16 ("bf16x3") path: fp32-grade results on the bf16 matrix cores (gfx950 has no TF32/xf32 and its
 * exact-fp32 MFMA runs at 1/16 of the bf16 rate).  Every value is two bf16 planes, hi = bf16(v) and
 * lo = bf16(v - hi); products are hi*hi + hi*lo + lo*hi with fp32 accumulation (~1e-5 relative).
 * An NLC-padded operand's lo plane follows its hi plane (guard rows included) at +alvq_nlc_plane_bytes(B,L,C);
 * a packed weight's lo image follows its hi image at +2*alvq_packed_weight_elems(M,C,KW) bytes.  Pointers passed
 * below point at row 0 of the hi plane.  Same contracts as the bf16 entry points of the same name.
 * ============================================================================================== */
int64_t alvq_nlc_plane_bytes(int B, int L, int C);
int alvq_pack_weight_bf16x3(const float* w, void* wp, int M, int C, int KW, int w_layout, void* stream);
int alvq_ncl_to_nlc_bf16x3(const float* x, void* y, int B, int C, int L, void* stream);
int alvq_nlc_to_ncl_bf16x3(const void* x, float* y, int B, int C, int L, void* stream);
int alvq_relu_mask_bf16x3(const void* dy, const void* t, void* out, int B, int C, int L, void* stream);
int alvq_conv1d_bf16x3(const void* x, const void* wp, const float* bias, const void* skip1, const void* skip2,
                       const void* mask, const void* post, void* y, void* y2, float* y_ncl,
                       int B, int C, int M, int L, int KW, int relu, void* stream);
int64_t alvq_conv1d_wgrad_bf16x3_workspace_bytes(int B, int C, int M, int L, int KW);
int alvq_conv1d_wgrad_bf16x3(const void* dy, const void* x, float* dw, float* dbias, void* workspace,
                             int B, int C, int M, int L, int KW, int w_layout, int accumulate, void* stream);
/* dw (+)= sum_i wgrad(dy[i], x[i]) over nseg (1..4) pairs of one shape in ONE launch (the R uses of a shared residual
 * weight), as alvq_conv1d_wgrad_bf16_multi. */
int alvq_conv1d_wgrad_bf16x3_multi(const void* const* dy, const void* const* x, int nseg, float* dw, void* workspace,
                                   int B, int C, int M, int L, int KW, int w_layout, int accumulate, void* stream);
int alvq_conv1d_wgrad_bf16x3_splits(int B, int C, int M, int L, int KW, int nseg);   /* as alvq_conv1d_wgrad_bf16_splits */

/* ================================================================================================
 * "f16mx" split path: fp32-grade results at TWO matrix-pipe units per product.  Every value v is H = fp16(v) plus
 * hi8 = e4m3(v/S), lo8 = e4m3((v-H)/(S*2^-11)); a product is H*H (one fp16 MFMA) + hi8*lo8 + lo8*hi8 (one
 * block-scaled fp8 MFMA at twice the fp16 rate per K), ~1.5e-5 rms per product.  S is a power of two per tensor class
 * (activations and loss-scaled gradients 1, weights 2^-8; csrc/f16mx_common.h).  An NLC-padded operand is two planes of
 * a bf16 plane's geometry: H as [rows][Cp] fp16, then at +alvq_nlc_plane_bytes(B,L,C) Q as [rows][Cp/32][hi8 x32|lo8 x32];
 * packed weights likewise (alvq_pack_weights_bf16_batch with planes = 3).  Same contracts as the bf16x3 entry points of
 * the same name, plus device scalars that carry a loss scale in and out of a backward chain:
 *   alvq_grad_scale_f32    state[0] = S, state[1] = 1/S with S the power of two that puts amax|x| in [2^7, 2^8)
 *                          (state: 4 floats, zero-initialised by the caller once; re-armed by every call)
 *   alvq_ncl_to_nlc_f16mx  multiplies by *scale (NULL = 1) while converting; alvq_nlc_to_ncl_f16mx likewise on the way out
 *   alvq_conv1d_f16mx      y_ncl output multiplied by *out_scale (NULL = 1); mask_bits / relu_bits_out as in
 *                          alvq_conv1d_bf16 (one bit per element, [rows][Mp/8] bytes, bit = stored H > 0)
 *   alvq_conv1d_wgrad_f16mx  dw / dbias multiplied by *inv_scale (NULL = 1)
 *   alvq_f16mx_range_flag  *out (device int) = the format's sticky range flag of the current device, optionally cleared:
 *                          bit 0 = a value of magnitude >= 65504 entered the format (stored saturated: fp16 has no
 *                          larger finite value), bit 1 = a NaN entered it (set by alvq_ncl_to_nlc_f16mx: model inputs
 *                          and gradients entering a backward chain, after the loss scale); bit 2 = a value PRODUCED
 *                          inside a chain reached the limit or is a NaN (an activation above 65504, a loss-scaled gradient
 *                          that outgrew its 2^8 headroom) -- watched by the epilogues of alvq_conv1d_f16mx and
 *                          alvq_conv1d_f16.  A set flag means "this step's results are fp16-saturated somewhere".
 * ============================================================================================== */
int alvq_grad_scale_f32(const float* x, int64_t n, float* state, void* stream);
int alvq_f16mx_range_flag(int* out, int reset, void* stream);
int alvq_ncl_to_nlc_f16mx(const float* x, void* y, int B, int C, int L, const float* scale, void* stream);
int alvq_nlc_to_ncl_f16mx(const void* x, float* y, int B, int C, int L, const float* scale, void* stream);
int alvq_relu_mask_f16mx(const void* dy, const void* t, void* out, int B, int C, int L, void* stream);
int alvq_conv1d_f16mx(const void* x, const void* wp, const float* bias, const void* skip1, const void* skip2,
                      const void* mask, const void* post, void* y, void* y2, float* y_ncl,
                      int B, int C, int M, int L, int KW, int relu, const void* mask_bits, void* relu_bits_out,
                      const float* out_scale, void* stream);
int64_t alvq_conv1d_wgrad_f16mx_workspace_bytes(int B, int C, int M, int L, int KW);
int alvq_conv1d_wgrad_f16mx(const void* dy, const void* x, float* dw, float* dbias, void* workspace,
                            int B, int C, int M, int L, int KW, int w_layout, int accumulate,
                            const float* inv_scale, void* stream);
/* dw (+)= inv_scale * sum_i wgrad(dy[i], x[i]) over nseg (1..4) pairs of one shape in ONE launch (the R uses of a shared
 * residual weight), as alvq_conv1d_wgrad_bf16_multi; all segments carry the same loss scale. */
int alvq_conv1d_wgrad_f16mx_multi(const void* const* dy, const void* const* x, int nseg, float* dw, void* workspace,
                                  int B, int C, int M, int L, int KW, int w_layout, int accumulate,
                                  const float* inv_scale, void* stream);
int alvq_conv1d_wgrad_f16mx_splits(int B, int C, int M, int L, int KW, int nseg);    /* as alvq_conv1d_wgrad_bf16_splits */

/* ================================================================================================
 * fp16 element type of the 16-bit pipeline: the same kernels, layouts (NLC-padded [rows][Cp], packed weights
 * [tap][Mp][Cp], sign bits) and contracts as the "_bf16" entry points of the same name, with fp16 elements, fp16 MFMAs
 * (v_mfma_f32_16x16x32_f16 / 32x32x16_f16) and saturating conversions.  Used by the BACKWARD pass of the "f16mx_hb" mode
 * (f16mx forward: fp32-grade outputs; fp16 backward: gradients under the device-chosen loss scale of alvq_grad_scale_f32,
 * products of fp16 operands with fp32 accumulation, ~5e-4 per product): an fp16 operand may be the H plane of an f16mx
 * activation or of an f16mx packed weight (same geometry: pass the plane's pointer), a mask its sign bits.
 *   alvq_ncl_to_nlc_f16 / alvq_nlc_to_ncl_f16   multiply by *scale (NULL = 1) while converting
 *   alvq_conv1d_f16        y_ncl output multiplied by *out_scale (NULL = 1)
 *   alvq_conv1d_wgrad_f16  dw / dbias multiplied by *inv_scale (NULL = 1); workspace = alvq_conv1d_wgrad_bf16_workspace_bytes
 *   alvq_relu_mask_bf16    serves fp16 buffers unchanged (the test is "element > 0" on the int16 pattern)
 * ============================================================================================== */
int alvq_ncl_to_nlc_f16(const float* x, void* y, int B, int C, int L, const float* scale, void* stream);
int alvq_nlc_to_ncl_f16(const void* x, float* y, int B, int C, int L, const float* scale, void* stream);
int alvq_conv1d_f16(const void* x, const void* wp, const float* bias, const void* skip1, const void* skip2,
                    const void* mask, const void* post, void* y, void* y2, float* y_ncl,
                    int B, int C, int M, int L, int KW, int relu, const void* mask_bits, void* relu_bits_out,
                    const float* out_scale, void* stream);
int alvq_conv1d_wgrad_f16(const void* dy, const void* x, float* dw, float* dbias, void* workspace,
                          int B, int C, int M, int L, int KW, int w_layout, int accumulate,
                          const float* inv_scale, void* stream);
int alvq_conv1d_wgrad_f16_multi(const void* const* dy, const void* const* x, int nseg, float* dw, void* workspace,
                                int B, int C, int M, int L, int KW, int w_layout, int accumulate,
                                const float* inv_scale, void* stream);

/* ================================================================================================
 * Location head: LocationModule.fc_1 = nn.Linear(L*K, M) on the flattened one-hot codes of a
 * spectrogram (vq_vae/location_model/location_model.py:10,21; scripts/train_location.py:69-77 feeds it
 * encodings.reshape(B, 201, 1024)).  On one-hot input the dense product is an embedding bag over the indices the
 * quantiser produced: B*L*M gathered weights instead of a (B, L*K) x (L*K, M) GEMM against a 99.9 %-zero operand.
 * ============================================================================================== */
/* idx[row] = position of the single 1.0 in row `row` of encodings (rows, K); *not_onehot (device int, caller zeroes
 * it) is OR-ed with 1 if any row is not exactly one-hot (then the caller must fall back to the dense product).
 * Inverse of alvq_onehot_f32 for the value get_latent_representation returns (vector_quantizer.py:39-40,58). */
int alvq_onehot_to_index_f32(const float* encodings, int32_t* idx, int* not_onehot, int64_t rows, int K, void* stream);
/* out[i] = (int32) idx[i] for n int64 indices; a value outside [0, K) becomes -1 and ORs 1 into *bad_index (device int,
 * caller-zeroed, sticky) -- a plain narrowing cast would wrap 2^32 + 5 to 5. */
int alvq_indices_to_i32(const int64_t* idx, int32_t* out, int* bad_index, int64_t n, int K, void* stream);
/* out[b][m] = bias[m] + sum_l W[m][l*K + idx[b][l]]      W: (M, L*K) row-major (nn.Linear.weight), idx: (B, L),
 * out: (B, M); sums in a fixed order.  Replaces F.linear at location_model.py:21 for one-hot x.  B*L <= 16384 per call
 * (callers chunk over B).  An index outside [0, K) contributes nothing and ORs 1 into *bad_index (optional device int,
 * sticky, caller-zeroed): no out-of-bounds access; the caller raises, as torch's embedding_bag does. */
int alvq_embedding_bag_fwd_f32(const float* W, const float* bias, const int32_t* idx, float* out,
                               int B, int L, int K, int M, int* bad_index, void* stream);
/* dW[m][l*K + idx[b][l]] += dz[b][m] for every (b, l) -- the caller zero-fills dW (M, L*K) first (alvq_fill_f32) --
 * and dbias[m] (+)= sum_b dz[b][m].  One wave owns a weight row: no atomics, fixed order.  Out-of-range indices are
 * skipped and flagged as in the forward. */
int alvq_embedding_bag_bwd_f32(const float* dz, const int32_t* idx, float* dW, float* dbias,
                               int B, int L, int K, int M, int accumulate_bias, int* bad_index, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALVQ_H */
