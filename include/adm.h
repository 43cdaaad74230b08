/* adm.h — C-ABI of the MI355X-native audio-diffusion hot path (libadm_hip.so).
 *
 * The reference (teticio/audio-diffusion) is pure Python: its hot path sits behind a duck-typed
 * component API (`AudioDiffusionPipeline(vqvae, unet, mel, scheduler)`,
 * audiodiffusion/pipeline_audio_diffusion.py:53-61), not behind an FFI. This header is the boundary a
 * maintainer binds with ctypes to replace the calls cited per function.
 *
 * Conventions: every function returns 0 on success, non-zero on error (message via
 * adm_last_error()); nothing throws across the ABI; the CALLER owns every I/O buffer (device
 * pointers, fp32 NCHW contiguous unless stated); the library owns only opaque handles;
 * `stream` is a hipStream_t passed as void* (NULL = default stream). One handle = one device = one stream
 * at a time (the reference pipeline is not re-entrant either).
 */
#ifndef ADM_H
#define ADM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int adm_version(void);
const char* adm_last_error(void);
/* 1 if built for the device (hipcc, gfx950), 0 for the CPU-emulation test build. */
int adm_is_device_build(void);
/* Always 0 since round 6 (kept for ABI stability): rounds 1-5 had -DADM_EXPERIMENTS builds carrying superseded Winograd kernel generations
 * ("conv_wino" = 1 / 2 / 3) and ablation / cycle-accounting instantiations; they were retired with that code. */
int adm_has_experiments(void);
/* Runtime options (process-wide; a training net re-learns which weight images it reads after any change):
 * "conv_wino" = 0 (direct MFMA kernel only) | 4 (default: the Winograd kernels wherever they tile the layer; they have their own filter image,
 *   so set the mode BEFORE weights are packed) | -1 (back to the default / ADM_CONV_WINO environment variable); 1 / 2 / 3 (earlier kernel
 *   generations, retired in round 6) are an error;
 * "wino5" = 1 (default, round 5) layers with 128 | Cout whose 128-cout workgroup tiles fill the chip run on conv_wino5_kernel (every input patch
 *   transformed once per 128 output channels; all eight waves are MFMA waves and share the staging work, placed between their MFMA groups) |
 *   0 conv_wino4_kernel everywhere (same filter image, bit-identical results) | bit 1 (2): conv_wino5_kernel for every layer with 128 | Cout,
 *   however few tiles (tests) | bit 3 (8): the two halves of the workgroup run MFMA block and staging block in antiphase instead (the first
 *   schedule built; same results, same speed) | -1 (ADM_WINO5);
 * "wino6" = 1 (default, round 5) 3x3 stride-1 convolutions with 128 | Cout, 32 | Cin, 16 | H, 16 | W on planes of at least 64x64 pixels whose
 *   16x16x128 tiles give one sample at least 32 workgroups run on conv_wino6_kernel: Winograd F(4x4,3x3), 1.78x fewer MFMAs than F(2x2,3x3) at
 *   0.6-1.7e-5 of max|out| per layer (F(2x2): 0.7-1.5e-6; the per-layer bar is 1e-4; profiles/r05_accuracy.md). The choice depends on the layer
 *   only (the two transforms are not bit-identical) | 0 F(2x2,3x3) kernels everywhere | 2 every layer the kernel tiles (tests) | n >= 16: planes
 *   of at least n x n pixels (256: the latency setting — single-sample sampling at 256x256 is 18 % faster with it than with the default, a B = 32
 *   forward 10 % slower; 128: in between) | -1 (ADM_WINO6);
 * "single_sample" = 0 (default) | 1: the partition rules for models that are sampled ONE spectrogram at a time (where a layer's tiles cannot
 *   fill 256 CUs and its time is a serial chain per workgroup). (a) conv_wino4_kernel: layers whose 64-cout x 8x16-pixel tiles give one sample
 *   fewer than 256 workgroups (planes of 16x16 .. 64x64 pixels) and that conv_wino6_kernel does not take split their input channels over
 *   2 / 4 / 8 workgroups per tile (every part a multiple of 32 channels); the partial sums are added in order by a finish launch (which also
 *   leaves the GroupNorm partial sums the unsplit kernel's epilogue would). (b) the split-K 3x3 kernel of the <= 8x8-pixel planes takes 16
 *   parts instead of 4 / 8. The partitions depend on the LAYER only, never on the batch — a sample's bits do not depend on its batch — so with
 *   the rule on a model pays the slab traffic at every batch size: it is a per-model opt-in (adm_unet_set_option; AudioDiffusion selects it).
 *   Results differ from the default rules' in the last bits (another fp32 summation order) | -1 (ADM_SINGLE_SAMPLE);
 * "wino_pair": accepted and ignored since round 6 (conv_wino4_kernel keeps one cadence: one workgroup barrier per two chunks);
 * "wgrad_max_split" = n caps the split-K factor of adm_conv2d_wgrad (0 = heuristic; tests use it to put several pixel tiles on
 *   one workgroup);
 * "wgrad_path" = 0 (default) | 1 | 2 | 3 keeps adm_conv2d_wgrad off its eight-wave / software-pipelined / prefetch kernels (tests reach every
 *   kernel with it; see adm_last_wgrad_variant below);
 * "conv_bf16" = 1 runs eligible 3x3 stride-1 convolutions (forward, data gradient and weight gradient) on 16-bit MFMA operands
 *   with fp32 accumulation (`--mixed_precision bf16`, scripts/train_unet.py:391-401), 2 = additionally the eligible 1x1 convolutions
 *   and stride-2 data gradients, 0 = fp32 everywhere (default), -1 = back to the ADM_CONV_BF16 environment variable;
 *   3 (round 4; what `enable_training(mixed_precision=...)` selects) = 2, with the 3x3 stride-1 convolutions of all three passes on
 *   blocked 16-bit operand images (adm_blocked_apply / adm_conv2d_bf16_blocked / adm_conv2d_wgrad_bf16_blocked below);
 * "conv_op16_f16" = 1 makes those kernels' operand format IEEE binary16 instead of bf16 (`--mixed_precision fp16`);
 * "blk_direct_dy" = 1 (default; level 3, read when a training plan is made) the backward of a GroupNorm whose input is read by nothing
 *   else writes the producing convolution's dy image directly | 0 fp32 dx tensor + image pass (bit-identical results) | -1 ADM_BLK_DIRECT_DY.
 * "gn_fuse_finish" = 1 (default) a split-K convolution (output planes of <= 8x8 pixels) whose output a GroupNorm reads next leaves
 *   that GroupNorm's scale / shift from its finish pass (one launch instead of finish + statistics; the tensor is bit-identical) |
 *   0 separate launches | -1 ADM_GN_FUSE_FINISH.
 * "side_overlap" = 1 (default) inference plans launch the 1x1 convolutions whose inputs are ready a few ops early (the resnets' conv_shortcut)
 *   on a second stream beside those ops (scheduling only: bit-identical results; adm_plan_op.hoist_from shows where) | 0 every op in list
 *   order on the caller's stream | -1 ADM_SIDE_OVERLAP. Every net re-plans on its next call (a UNet's captured loop is re-captured).
 * The dispatch epoch moves only when a value really changes; set options BEFORE adm_unet_refresh_weights / the next train step.
 * adm_version() = 120 (test aids adm_last_conv_detail, adm_conv2d_gn_finish); 119 (test aid adm_mel_last_variant); 108 (option "wgrad_path", test aids adm_last_wgrad_variant, adm_wgrad_reduce); 107 (test aids adm_time_embedding, adm_temb_proj); 106 (adm_last_attention_variant); 105 (option "side_overlap"; adm_plan_op, adm_unet_plan_ops, adm_vae_plan_ops); 104 since round 6 (adm_conv_args.single_sample, option "single_sample"; 103: adm_conv_args.wino6_rule, adm_unet_set_option, adm_release_stream); 102 since round 5 (Winograd filter buffers hold two images: adm_winograd_packed_floats); 101 since round 4 (adm_slerp_grid takes DOUBLE weights since round 3; blocked-image entry points). */
int adm_set_option(const char* name, int value);
/* Per-(device, stream) scratch the library keeps for a stream (the split-K slab buffer of the small-plane convolutions, >= 1 MiB, at most
 * 1024 streams per device): give it back BEFORE destroying a stream that has run library calls. Drains the stream first (a captured graph of
 * that stream holds the buffer's address: destroy or stop replaying such graphs before). No-op for a stream the library holds nothing for. */
int adm_release_stream(void* stream);
/* Kernel variant the last adm_conv2d on this thread dispatched to (see adm_op_profile.variant; 4311 = Winograd). */
int adm_last_conv_variant(void);
/* Test aid (adm_version() >= 120; tests assert the forward launchers' rules with it): what the last adm_conv2d on this thread chose, for the
 * fp32 implicit-GEMM kernels (variants 1xx / 3xx / 21xx / 23xx) and the small-channel kernels (1001 / 1002). Fills out[0 .. n - 1] (slots
 * beyond ADM_CONV_DETAIL_SLOTS read 0) and returns the variant. After a launch of another family (Winograd, 16-bit operands) only slot 0 is
 * known and the others read 0; a call that returns an error before it launches may leave a partial record.
 *   [0] variant (= adm_last_conv_variant)
 *   [1] cout tile of the MFMA kernel that ran (32 / 64 / 128; the split-K instantiations choose their own). Small-channel family: the kernel,
 *       1 conv_small_cin_kernel | 2 conv_small_cin_wide_kernel | 3 conv_small_cout_wide_kernel | 4 conv_small_cout_kernel
 *   [2] parts of the K (input channel) split, 1 = unsplit
 *   [3] finish kernel of a split launch: 0 none | 1 ksplit_finish_kernel (four pixels per thread) | 2 ksplit_finish1_kernel | 3 the
 *       GroupNorm-fused finish (ksplit_finish_gn_kernel)
 *   [4] tap mask of the split generic kernel (bit ty * 3 + tx; 0x1ff everywhere else)
 *   [5] [6] pixel tile TW, TH (small-channel family: the pixels one workgroup covers, as a row x column shape)   [7] images per tile NI
 *   [8] 1 = the register-pipelined instantiation of the split generic kernel (ADM_KSP_PIPE)
 *   [9] cout parts of conv_small_cin_wide_kernel's grid (1 elsewhere) */
#define ADM_CONV_DETAIL_SLOTS 10
int adm_last_conv_detail(int* out, int n);
/* Kernel family the last attention entry point on this thread launched (adm_version() >= 106; tests assert the dispatch rules with it):
 * family * 100 + head_dim, families 1 = one pass, whole head in LDS (attention_kernel) | 2 = four lanes per query (attention_split4_kernel,
 * "single_sample") | 3 = key blocks, online softmax on the vector ALUs (attention_blocked_kernel) | 4 = flash form on the f32 MFMAs
 * (attention_mfma_kernel) | 5 = adm_cross_attention | 6 = adm_attention_backward (head resident in LDS) | 7 = adm_attention_backward_blocked |
 * 8 = adm_cross_attention_backward. E.g. 108 = attention_kernel<8>, 432 = attention_mfma_kernel<32>. 0 before the first launch; a call that
 * returns an error before launching (an LDS slab that does not fit, an unsupported head_dim) leaves the value as it was. The executors'
 * attention ops (adm_unet_forward, adm_unet_forward_backward) go through the same launchers and report the same way. */
int adm_last_attention_variant(void);

/* Test aids (adm_version() >= 107): the two launches of the timestep-embedding path at shapes of the caller's choice (the executors run
 * them at their model's shapes only).
 *   adm_time_embedding: emb (B, dim_emb) = linear_2(silu(linear_1(sinusoid(t)))) with sinusoid = [cos | sin](t[b] * freqs[i]) when flip, else
 *     [sin | cos]; t (B) and freqs (half_dim) on the device, dim_in = 2 * half_dim, w1 (dim_emb, dim_in), w2 (dim_emb, dim_emb).
 *     NULL or written: save_sinus (B, dim_in) the input of linear_1, save_z (B, dim_emb) its pre-activation output, emb_act (B, dim_emb) =
 *     silu(emb).
 *   adm_temb_proj: out (B, R) = bias + silu(emb) W^T with w (R, K) the stacked time_emb_proj matrices, emb (B, K); emb_is_activated != 0:
 *     `emb` already holds silu(emb) (adm_time_embedding's emb_act). K <= 1536 when B >= 8. */
int adm_time_embedding(const float* t_dev, const float* freqs, int half_dim, int flip, const float* w1, const float* b1, const float* w2,
                       const float* b2, int dim_in, int dim_emb, float* emb, int B, float* save_sinus, float* save_z, float* emb_act,
                       void* stream);
int adm_temb_proj(const float* emb, const float* w, const float* bias, float* out, int B, int K, int R, int emb_is_activated,
                  void* stream);

/* ---------------------------------------------------------------- scheduler epilogue (rows S2,S3,P4,P5)
 * One fused elementwise kernel replacing DDIMScheduler.step / DDPMScheduler.step
 * (pipeline_audio_diffusion.py:165-179), the mask overwrite (:181-185) and, on the last step, the
 * dequantisation (images/2+0.5).clamp(0,1)*255 -> round-half-even -> uint8 (:192-194).
 *   x0   = clamp((x - sqrt_beta*eps) / sqrt_alpha, -clip, clip)        (clip < 0: no clamp)
 *   prev = k_x0*x0 + k_x*x + k_eps*eps + k_noise*noise
 * DDIM: k_x0=sqrt(a_prev), k_x=0, k_eps=sqrt(1-a_prev-std^2), k_noise=std (eta>0).
 * DDPM: k_x0=sqrt(a_prev)*cur_beta/beta_t, k_x=sqrt(cur_alpha)*beta_prev/beta_t, k_eps=0, k_noise=sqrt(var) (t>0).
 * The host computes the scalars in the same fp32 arithmetic diffusers uses. */
typedef struct adm_sched_coef {
  float sqrt_beta, sqrt_alpha, clip, k_x0, k_x, k_eps, k_noise, timestep;
} adm_sched_coef;

/* coef_table: device array of adm_sched_coef; entry used = step_dev ? *step_dev : step.
 * noise: NULL or (B,C,H,W). mask: NULL or (B,n_steps,H,W) (requires C==1); columns [0,mask_start) and
 * [W-mask_end,W) of `out` are overwritten with mask[:,step]. u8_out: NULL or (B,H*W*C) uint8 image of `out`.
 * out may alias x. */
int adm_sched_step(const float* x, const float* eps, const float* noise, float* out, uint8_t* u8_out,
                   const adm_sched_coef* coef_table, const int* step_dev, int step,
                   const float* mask, int n_mask_steps, int mask_start, int mask_end,
                   int B, int C, int H, int W, void* stream);

/* The same epilogue for a second-order multistep data-prediction solver (DPM-Solver++ 2M; adm_version() >= 109). The update is
 * linear in (x, x0 of this step, x0 of the previous step), so adm_sched_coef keeps its eight fields and the one extra per-step
 * coefficient travels beside it in k_hist_table (device, one float per row of coef_table):
 *   m0   = clamp((x - sqrt_beta*eps) / sqrt_alpha, -clip, clip)
 *   prev = k_x0*m0 + k_x*x + k_hist*hist + k_noise*noise;   hist = m0
 * hist: (B,C,H,W) device buffer, read only where k_hist != 0 (it may be uninitialised on the first step of a run) and always
 * written with m0, before the mask overwrite. Everything else as adm_sched_step; out may alias x. */
int adm_sched_multistep(const float* x, const float* eps, const float* noise, float* out, uint8_t* u8_out,
                        const adm_sched_coef* coef_table, const float* k_hist_table, float* hist,
                        const int* step_dev, int step,
                        const float* mask, int n_mask_steps, int mask_start, int mask_end,
                        int B, int C, int H, int W, void* stream);

/* Dynamic thresholding of the x0 prediction (Saharia et al. 2022, "Imagen" §2.3; diffusers' `thresholding`; adm_version() >= 110).
 * Per sample b, with x0 = (x - sqrt_beta*eps) / sqrt_alpha as adm_sched_step computes it and n = C*H*W:
 *   q_b = fma(w, b - a, a) if w < 0.5 else fma(-(b - a), 1 - w, b),  a, b = the order statistics of rank lo, hi of the ascending |x0_b|
 *         (b - a and 1 - w rounded on their own, the multiply-add fused: torch's CPU lerp)
 *   s_b = clamp(q_b, 1, max_value);   scale_out[b] = s_b   (B floats, device)
 * which is torch.quantile(|x0_b|, ratio) (linear interpolation) to the bit when the caller computes, in float32,
 *   rank = float32(ratio) * float32(n - 1), lo = floor(rank), hi = ceil(rank), w = rank - lo        (0 <= lo <= hi <= n - 1, hi - lo <= 1).
 * One workgroup per sample, an exact MSB-first radix select over LDS histograms of the bit pattern of |x0| (integer counts only: a sample's
 * result does not depend on the batch it sits in); x0 is recomputed from x and eps in every pass, nothing is kept in global memory, so the
 * call needs no scratch. Non-finite x0 is out of contract for the value returned (NaN patterns order last); the call stays in bounds. */
int adm_sched_threshold(const float* x, const float* eps, const adm_sched_coef* coef_table, const int* step_dev, int step,
                        int lo, int hi, float w, float max_value, float* scale_out, int B, int C, int H, int W, void* stream);
/* adm_sched_step with x0 = clamp(x0, -s_b, s_b) / s_b in place of the `clip` clamp (the row's clip field is ignored): runs
 * adm_sched_threshold into `scale` (B floats, device, caller-owned: it holds s_b afterwards) and then the step kernel on the same stream, so
 * the selection has read x before an `out` that aliases x is written. With max_value == 1 every s_b is 1 and the result is bit-identical to
 * adm_sched_step with clip = 1. */
int adm_sched_step_thresholded(const float* x, const float* eps, const float* noise, float* out, uint8_t* u8_out,
                               const adm_sched_coef* coef_table, const int* step_dev, int step,
                               const float* mask, int n_mask_steps, int mask_start, int mask_end,
                               int B, int C, int H, int W, void* stream,
                               int lo, int hi, float w, float max_value, float* scale);

/* Models that predict the clean sample or the velocity instead of the noise (diffusers' prediction_type "sample" / "v_prediction", Salimans &
 * Ho 2022; adm_version() >= 111). `prediction`: 0 epsilon, 1 sample, 2 v_prediction; `eps` is then the model output o, and with
 * sa = sqrt_alpha, sb = sqrt_beta of the row
 *   epsilon       x0 = (x - sb*o) / sa     e = o
 *   sample        x0 = o                   e = (x - sa*x0) / sb
 *   v_prediction  x0 = sa*x - sb*o         e = sa*o + sb*x
 * e is formed from x0 BEFORE the clamp or the threshold; everything after is adm_sched_step's:
 *   x0 = clamp(x0) (static or dynamic),  prev = k_x0*x0 + k_x*x + k_eps*e + k_noise*noise,  mask overwrite, u8.
 * The same eight adm_sched_coef fields serve the three types. On a zero-terminal-SNR row (sa = 0, sb = 1) the two new forms stay finite:
 * x0 = -o, e = x (v_prediction) and x0 = o, e = x (sample); the epsilon form divides by zero there.
 * adm_sched_threshold_pred: adm_sched_threshold with |x0| of the given type (for `sample` that is |o|, at any sa).
 * adm_sched_step_pred: scale == NULL: adm_sched_step (the row's static clip; lo, hi, w, max_value are ignored); otherwise
 * adm_sched_step_thresholded. With prediction == 0 both run the kernels of the entry points they are named after, bit for bit. */
int adm_sched_threshold_pred(const float* x, const float* eps, const adm_sched_coef* coef_table, const int* step_dev, int step,
                             int lo, int hi, float w, float max_value, float* scale_out, int B, int C, int H, int W, void* stream,
                             int prediction);
int adm_sched_step_pred(const float* x, const float* eps, const float* noise, float* out, uint8_t* u8_out,
                        const adm_sched_coef* coef_table, const int* step_dev, int step,
                        const float* mask, int n_mask_steps, int mask_start, int mask_end,
                        int B, int C, int H, int W, void* stream,
                        int lo, int hi, float w, float max_value, float* scale, int prediction);

/* Classifier-free guidance (Ho & Salimans 2022; adm_version() >= 112). The model ran twice on the same x: eps_cond with the encoding,
 * eps_uncond with the null encoding; the step and the selection use
 *   o = eps_uncond + guidance_scale * (eps_cond - eps_uncond)      (three separately rounded fp32 operations, as diffusers' torch expression)
 * wherever the entry points above use `eps`: in x0, in e and in the multistep history. One more operand in the same kernels: 16 B/elem where
 * the unguided step moves 12 (+4 with noise, +8 with the history); each selection pass reads 12 B/elem instead of 8. eps_cond == eps_uncond
 * (the same pointer, or equal values) gives the unguided result bit for bit at any finite scale. `prediction` as adm_sched_step_pred.
 * adm_sched_threshold_guided: adm_sched_threshold_pred on |x0| of o.
 * adm_sched_step_guided: hist != NULL: adm_sched_multistep (needs k_hist_table, prediction == 0 and scale == NULL); otherwise scale != NULL:
 * adm_sched_step_thresholded; otherwise adm_sched_step (lo, hi, w, max_value ignored; k_hist_table ignored when hist == NULL).
 * out may alias x; it must not alias eps_cond or eps_uncond's other samples (each lane reads its own elements before it writes them, so
 * out == eps_cond or out == eps_uncond is in contract for the plain and multistep steps; the thresholded step's selection reads whole
 * samples first, on the same stream, and is safe as well). A non-finite guidance_scale is refused; scale <= 1 is computed as asked
 * (callers that follow diffusers' rule skip guidance there: u + 1*(c - u) is not c in floating point). */
int adm_sched_threshold_guided(const float* x, const float* eps_cond, const float* eps_uncond, float guidance_scale,
                               const adm_sched_coef* coef_table, const int* step_dev, int step,
                               int lo, int hi, float w, float max_value, float* scale_out, int B, int C, int H, int W, void* stream,
                               int prediction);
int adm_sched_step_guided(const float* x, const float* eps_cond, const float* eps_uncond, float guidance_scale, const float* noise,
                          float* out, uint8_t* u8_out, const adm_sched_coef* coef_table, const float* k_hist_table, float* hist,
                          const int* step_dev, int step,
                          const float* mask, int n_mask_steps, int mask_start, int mask_end,
                          int B, int C, int H, int W, void* stream,
                          int lo, int hi, float w, float max_value, float* scale, int prediction);

/* Noise drawn on the device, inside the kernel that consumes it (adm_version() >= 113).
 *
 * "adm noise stream 1": a normal is a pure function of (seed, global sample row, integer timestep, element, stream id). It is its own
 * definition; it does not reproduce torch.randn on any device.
 *   generator  Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as 1, 2, 3"): multipliers 0xD2511F53, 0xCD9E8D57, key
 *              increments 0x9E3779B9, 0xBB67AE85; key = (seed & 0xffffffff, seed >> 32) of a uint64 seed.
 *   counter    (q, row, t, stream):  q = element index / 4, element index = c*H*W + y*W + x inside the sample (the index of the float4);
 *              row = row_offset + b, the GLOBAL sample row;  t = the row's adm_sched_coef.timestep converted to an integer (not the loop's
 *              step index);  stream = 0 step noise, 1 initial latent (t = 0), 2 and 3 reserved (VAE posterior, training noise; not built).
 *   normals    the four outputs r0..r3 give the normals of elements 4q .. 4q+3:  (z0, z1) = BM(r0, r1), (z2, z3) = BM(r2, r3) with
 *              BM(a, b): u1 = ((a >> 8) + 1) * 2^-24 in (0, 1], u2 = (b >> 8) * 2^-24 in [0, 1) (both exact in fp32),
 *                        R = sqrt(-2 ln u1),  result (R cos 2 pi u2, R sin 2 pi u2).   |z| <= sqrt(48 ln 2) < 5.77: always finite.
 * Within one build of the library every kernel that draws from the stream gives the same bits (one device helper); two builds (gfx950, the
 * CPU emulation) agree to the accuracy of their logf / sinf / cosf, not bit for bit. So a sample's bits depend on neither its batch, its
 * shard, a chunking of the steps nor the step a run starts at.
 *
 * adm_randn: out (B, per_sample) device floats = the normals of rows row_offset .. row_offset + B - 1 at (t, noise_stream); what the step
 * kernel draws for the same counters, materialised. per_sample % 4 == 0, row_offset >= 0, row_offset + B within 32 bits, t in [0, 2^31),
 * noise_stream 0 or 1.
 * adm_sched_step_philox: adm_sched_step_guided's step (scale == NULL: the static clip; otherwise thresholded) with the noise of a row with
 * k_noise != 0 drawn in the kernel from (seed, row_offset + b, timestep of the row, element) of stream 0 instead of read from a buffer:
 * 12 B/elem where the buffer costs 16 (guided: 16 instead of 20). eps_uncond == NULL: unguided (guidance_scale is ignored). A row with
 * k_noise == 0 draws nothing and equals the step without noise. There is no multistep form: that step has no noise rows. */
int adm_randn(float* out, int B, long per_sample, uint64_t seed, int row_offset, int t, int noise_stream, void* stream);
int adm_sched_step_philox(const float* x, const float* eps_cond, const float* eps_uncond, float guidance_scale,
                          float* out, uint8_t* u8_out, const adm_sched_coef* coef_table,
                          const int* step_dev, int step,
                          const float* mask, int n_mask_steps, int mask_start, int mask_end,
                          int B, int C, int H, int W, void* stream,
                          int lo, int hi, float w, float max_value, float* scale, int prediction,
                          uint64_t seed, int row_offset);

/* The scheduler step as ONE entry point (adm_version() >= 114). Every combination above, and each one a later version adds, is a
 * value of this struct: new scheduler features add fields at its end and bump adm_version(), as adm_conv_args does, and add no symbol.
 * Zero-initialise it and set what the call uses.
 *
 * FROZEN: adm_sched_step, adm_sched_multistep, adm_sched_threshold, adm_sched_step_thresholded, adm_sched_threshold_pred,
 * adm_sched_step_pred, adm_sched_threshold_guided, adm_sched_step_guided and adm_sched_step_philox keep their signatures and their
 * results for existing callers; each fills this struct and calls adm_sched_step_ex / adm_sched_threshold_ex. None of them will grow. */
typedef struct adm_sched_step_args {
  const float* x;            /* (B,C,H,W) */
  const float* eps;          /* the model output (the conditional one under guidance) */
  const float* eps_uncond;   /* NULL: unguided, guidance_scale is ignored; otherwise the unconditional output and a finite scale */
  float guidance_scale;
  const float* noise;        /* NULL or (B,C,H,W); must be NULL with noise_source 1 */
  float* out;                /* may alias x */
  uint8_t* u8_out;           /* NULL or (B,H*W*C) */
  const adm_sched_coef* coef_table;
  const float* k_hist_table; /* mode 2: one float per row of coef_table */
  float* hist;               /* mode 2: (B,C,H,W), see adm_sched_multistep */
  const int* step_dev;       /* row used = step_dev ? *step_dev : step */
  int step;
  const float* mask;         /* NULL or (B,n_mask_steps,H,W); needs C == 1 */
  int n_mask_steps, mask_start, mask_end;
  int B, C, H, W;            /* W % 4 == 0 */
  int mode;                  /* 0 plain (the row's static clip), 1 thresholded (needs scale), 2 multistep (needs k_hist_table and hist;
                                prediction 0, noise_source 0 and scale == NULL: that step is epsilon only, has no noise rows and no
                                thresholded form) */
  int prediction;            /* 0 epsilon, 1 sample, 2 v_prediction */
  int lo, hi;                /* mode 1, and adm_sched_threshold_ex: the ranks, weight and maximum of adm_sched_threshold */
  float w, max_value;
  float* scale;              /* mode 1, and adm_sched_threshold_ex: (B,) device, receives s_b */
  int noise_source;          /* 0: `noise` (or none); 1: "adm noise stream 1", stream 0, drawn in the kernel from (seed, row_offset + b) */
  uint64_t seed;
  int row_offset;            /* noise_source 1: >= 0 and row_offset + B within 32 bits */
  float guidance_rescale;    /* adm_version() >= 115. 0: off; otherwise phi in (0, 1], and needs eps_uncond and rescale ("guidance rescale" below) */
  float* rescale;            /* (B,) device, caller-owned: receives r_b, as scale receives s_b */
  const struct adm_unipc_coef* unipc_table;   /* adm_version() >= 116 ("UniPC" below). NULL: the steps above. Otherwise the UniPC step: one
                                row per row of coef_table; `hist` is then the TWO-slot history (2,B,C,H,W) and k_hist_table is ignored;
                                mode 0 (x0 as predicted) or 1 (thresholded, needs scale), mode 2 is refused; noise must be NULL and
                                noise_source 0 (each refused by name) */
  float* last;               /* the UniPC step: (B,C,H,W) device, the corrected sample of the previous row; read where c_t != 0, always written */
  const float* known;        /* adm_version() >= 118 ("Region in-painting" below). (Bk,C,H,W) device, Bk = B (known_batched != 0) or 1 */
  const float* known_noise;  /* (B,C,H,W) device */
  const uint8_t* keep;       /* NULL: off, and the other five fields are ignored. Otherwise (Bm,H,W) device bytes, Bm = B (keep_batched
                                != 0) or 1; non-zero: the element is overwritten. Needs known, known_noise and known_table, and mask == NULL
                                (each refused by name) */
  const float* known_table;  /* device, two floats (ka, kb) per row of coef_table */
  int known_batched, keep_batched;
} adm_sched_step_args;
int adm_sched_step_ex(const adm_sched_step_args* a, void* stream);
/* The selection alone (adm_sched_threshold and its _pred / _guided forms): reads x, eps, eps_uncond, guidance_scale, coef_table, step_dev,
 * step, B, C, H, W, prediction, lo, hi, w, max_value, guidance_rescale of the same struct and writes scale (and, with guidance_rescale != 0,
 * rescale first); the other fields are ignored. */
int adm_sched_threshold_ex(const adm_sched_step_args* a, void* stream);

/* Guidance rescale (adm_version() >= 115): Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4;
 * diffusers' `rescale_noise_cfg` / `guidance_rescale` [3P-recall: restated from memory, diffusers is not consulted]. THE definition; the
 * kernels (csrc/k_sched.hip) and the documents refer to it. Per sample b, with c the conditional model output, u the unconditional one, g
 * the guidance scale, phi the fp32 guidance_rescale and n = C*H*W elements:
 *   o      = u + g*(c - u)                                   unchanged: three separately rounded fp32 operations
 *   std_c  = fp32( sqrt( sum((c - mean c)^2) / (n - 1) ) )   unbiased, as torch.std; the sums are accumulated in fp64, over
 *   std_o  = fp32( sqrt( sum((o - mean o)^2) / (n - 1) ) )   d = v - v[first element of the sample] (S2 - S1*S1/n), in a fixed order
 *   r_b    = std_c / std_o                                   one fp32 division
 *            r_b = 1 when std_o == 0 or either standard deviation is not finite (n == 1 included).
 *            Deliberate deviation: diffusers yields NaN there. A sample whose c and u are constant is left as guidance made it.
 *   o'     = phi*(o*r_b) + (1 - phi)*o                       three products and one sum, each rounded on its own; 1 - phi formed in fp32
 * o' stands wherever o stood: in x0, in e, in the multistep history and in the key of the thresholding selection. The rescale acts on the
 * model output whatever it predicts (epsilon, sample or v). r_b is a function of sample b's c and u alone: it depends on neither the batch
 * nor the order of execution (no floating-point atomics, no scratch that outlives a launch). With guidance_rescale != 0 the step entry
 * points enqueue, on the one stream: the statistics kernel (8 B/elem read, writes rescale), the selection (mode 1), the step.
 * guidance_rescale == 0 is the path of version 114, bit for bit, and the statistics kernel is not launched. Refused: a guidance_rescale
 * outside [0, 1] or not finite; guidance_rescale != 0 with eps_uncond == NULL (encoding_uncond == NULL for the loop); guidance_rescale != 0
 * with rescale == NULL (adm_sched_step_ex, adm_sched_threshold_ex; the loop's buffer is the handle's). */

/* UniPC (adm_version() >= 116): Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion
 * Models"; config names follow diffusers' `UniPCMultistepScheduler` [3P-recall: restated from memory, diffusers is not consulted, so the
 * arithmetic is unpinned like the multistep solver's; tests/test_unipc.py anchors it independently]. THE definition; the kernel
 * (csrc/k_unipc.hip), the scheduler (schedulers.py `unipc_rows`) and the documents refer to it. Data-prediction form, orders 1 and 2.
 *
 * Levels i = 0..N, float64 (alpha_i, sigma_i, lambda_i = ln alpha_i - ln sigma_i): level i < N is the i-th timestep of the schedule, level N
 * is sigma = 0 (lambda = +inf) or the sigma of timestep 0. A zero-SNR first level has alpha = 0, lambda = -inf.
 * Data prediction m_i: the x0 prediction at row i from the sample x the model was evaluated on: x0 of the row's prediction type (the
 *   table under adm_sched_step_pred) of o, o the guided / rescaled output under guidance; thresholded (mode 1): clamp(x0, -s_b, s_b) / s_b with
 *   s_b of adm_sched_threshold. There is no static clip (coef_table's clip is -1 and is not read).
 * B(h), for h > 0 with hh = -h, phi = expm1(hh):  solver_type bh2: B = phi;  bh1: B = hh.
 * Corrector vector b(h, K): g = phi/hh - 1, f = 1; for k = 1..K: b_k = g*f/B, f <- f*(k+1), g <- g/hh - 1/f.
 * Orders, for a run that starts at row r: predictor order p_i = min(solver_order, i - r + 1, N - i if lower_order_final); row i > r has a
 *   corrector unless i - 1 is in disable_corrector, of order q_i = p_(i-1). A level with lambda = -inf is never used as history: the order
 *   that would need it is lowered by one.
 * Corrector (re-does the move i-1 -> i now that m_i is known), h = lambda_i - lambda_(i-1), r1 = (lambda_(i-2) - lambda_(i-1)) / h:
 *   q = 1: rho = [0.5];  q = 2: rho solves [[1, 1], [r1, 1]] rho = b(h, 2)
 *   x_c = (sigma_i/sigma_(i-1)) x_last - alpha_i phi m_(i-1) - alpha_i B ( [q = 2] rho_1 (m_(i-2) - m_(i-1)) / r1 + rho_last (m_i - m_(i-1)) )
 *   x_last: the corrected sample of row i-1 (the model input itself on row r). Without a corrector x_c = x.
 *   h = +inf (level i-1 at zero SNR): phi = B = -1 and q = 1.
 * Predictor (moves i -> i+1 from x_c), h = lambda_(i+1) - lambda_i, r1' = (lambda_(i-1) - lambda_i) / h:
 *   x' = (sigma_(i+1)/sigma_i) x_c - alpha_(i+1) phi m_i - [p = 2] alpha_(i+1) B 0.5 (m_(i-1) - m_i) / r1'
 *   lambda_(i+1) = +inf: x' = m_i, written out (the k_x*x_c product is not formed);  lambda_i = -inf: phi = B = -1, x' = sigma_(i+1) x_c + alpha_(i+1) m_i.
 * Both stages are linear in (x_last, m_(i-1), m_(i-2), m_i, x_c), so a row is the adm_sched_coef of coef_table — sqrt_alpha, sqrt_beta of
 * level i, k_x = sigma_(i+1)/sigma_i, k_x0 = the coefficient of m_i in x', clip = -1, k_eps = k_noise = 0, timestep — and one adm_unipc_coef:
 *   x_c = c_x*x_last + c_t*m_i + c_m1*m_(i-1) + c_m2*m_(i-2)       applied iff c_t != 0 (otherwise x_c = x and x_last is not read)
 *   x'  = k_x0*m_i + k_x*x_c + p_m1*m_(i-1)                         k_x*x_c formed iff k_x != 0
 * all computed in float64 on the host and rounded to fp32 once. m_(i-1) is read only where c_m1 != 0 || p_m1 != 0, m_(i-2) only where
 * c_m2 != 0: the first row of a run (c_t = c_m1 = c_m2 = p_m1 = 0) finds last and both history slots uninitialised.
 * State: last (B,C,H,W) receives x_c on every row; hist (2,B,C,H,W): row s (the index into the tables) reads m_(i-2) from slot s & 1 and
 * then writes m_i there, and reads m_(i-1) from slot (s - 1) & 1. The mask overwrite goes on `out` only. out may alias x.
 * Traffic of a full row: 20 B/elem read + 12 B/elem written, +4 read under guidance. */
typedef struct adm_unipc_coef {
  float c_x, c_m1, c_m2, c_t, p_m1;
} adm_unipc_coef;

/* Region in-painting (adm_version() >= 118): part of the sample is pinned to a known image under an arbitrary keep mask, the noised known
 * image being formed inside the step kernel instead of being staged per step. THE definition; the kernels (csrc/k_sched.hip "KNOWN",
 * csrc/k_sched_common.h sched_known4) and the documents refer to it.
 * Operands (adm_sched_step_args; adm_sample_loop_args has the same with a host table):
 *   known        (Bk,C,H,W) fp32, Bk = B or 1 (known_batched 0: the one image serves every sample)   the known image, in model space
 *   known_noise  (B,C,H,W)  fp32                                                                     one fixed draw for all steps
 *   keep         (Bm,H,W)   bytes, Bm = B or 1 (keep_batched 0: the one mask serves every sample)    no channel axis: broadcast over C
 *   known_table  two floats (ka, kb) per row of coef_table (the loop: known_coef_host, n_steps x 2 host floats)
 *   keep must be 4-byte aligned, known and known_noise 16-byte aligned; W % 4 == 0 as everywhere.
 * Arithmetic, on row s, after the step has formed out (and after the multistep history / the UniPC state, which are the solver's own and
 * never overwritten, have been written), before the store and the u8 pack: for every element e of sample b with
 *   keep[b or 0][e mod H*W] != 0:    out = fma(ka, known[b or 0][e], kb * known_noise[b][e]),    (ka, kb) = known_table[s]
 * the product kb * noise rounded to fp32 on its own, then one fused multiply-add: adm_add_noise's expression, bit for bit (with
 * ka = sqrt(alphas_cumprod[t]), kb = sqrt(1 - alphas_cumprod[t]) it IS add_noise(known, noise, t)). Elements with keep == 0 are the
 * step's, bit for bit; keep == NULL is the path of version 117, bit for bit.
 * The two levels a caller can put into the table (the Python API's `known_level`):
 *   "current"   row i carries the level of its own timestep t_i, the level the sample had BEFORE the step: the reference's mask rule,
 *               equal to the staged `mask` path bit for bit; the kept region of the result still carries the noise of the last timestep.
 *   "previous"  row i carries the level of t_(i+1), the level the sample has AFTER the step, and the last row (1, 0): the kept region
 *               of the result is the known image exactly (fma(1, known, 0 * noise) = known for finite noise).
 * Traffic: +1 B/elem for the keep word (one 32-bit load per float4), +8 B/elem where kept. Nothing has a step axis.
 * Windowed sampling: the three tensors have the wide shape (window_total_w for W) and the overwrite acts on the wide sample.
 * Refused, each naming the field: keep without known or known_noise; keep without known_table (known_coef_host); keep with mask. */

/* Windowed sampling (adm_version() >= 117): one wide sample denoised jointly through overlapping model-sized windows, the model outputs
 * averaged where windows overlap and ONE scheduler step made on the wide sample (the fusion of Bar-Tal et al. 2023, "MultiDiffusion",
 * applied to the model output before the step). THE definition; the kernels (csrc/k_window.hip), the loop (csrc/unet_exec.hip) and the
 * documents refer to it.
 * Shapes: the model's sample is (C,H,W); the wide sample is (C,H,Wt) (Wt = total_w; the Python API's `frames`); stride s.
 *   Required: W % 4 == 0, s % 4 == 0, Wt % 4 == 0 and 0 < s <= W <= Wt.
 * Placement:
 *   open     (wrap = 0)  requires (Wt - W) % s == 0;  nW = (Wt - W)/s + 1 windows;  window w covers columns [w*s, w*s + W)
 *   circular (wrap = 1)  requires Wt % s == 0;        nW = Wt/s windows;            window w covers columns (w*s + j) mod Wt, j in [0, W)
 *   With W <= Wt no window covers a column twice. On the circle the time axis has no edge: the seam is a column like any other.
 * Gather:  windows[(b*nW + w), c, y, j] = x[b, c, y, col(w, j)].  A copy, bit-exact. Rows are sample-major: the nW windows of sample b
 *   are contiguous.
 * Blend:   mean[b, c, y, col] = (o_w0 + o_w1 + ...) / float(count)  over the windows that cover col, in ASCENDING window index; the sum
 *   starts from the first window's value (not from zero), every addition is rounded to fp32 on its own, and there is one IEEE division
 *   by the integer cover count converted to float. A column covered once gives o itself. No atomics: the result depends on neither the
 *   launch geometry nor a replay.
 * Step:    one scheduler step of the existing kind on the wide tensors, (x, mean) -> x' at shape (B,C,H,Wt). Everything that is per
 *   sample is per WIDE sample: the thresholding statistic is over n = C*H*Wt; the guidance-rescale factor is per wide sample; the
 *   device-noise counter is (float4 index inside the wide sample, row_offset + b, timestep); the multistep and UniPC state has the wide
 *   shape. Under guidance both forwards run on the same gathered windows and both outputs are blended before u + g*(c - u).
 * Where the step is not affine in the model output (the clip clamp, thresholding) "average the model outputs, then step once" IS the
 * definition; it is not the same as "step each window, then average".
 * Both entry points refuse, by the name of the argument (total_w, stride or wrap), every placement rule above; null pointers, B <= 0 and
 * a B*nW past int are refused too. Traffic: gather 8 B per window element; blend 4 B read per window element + 4 B written per wide one. */
int adm_window_gather(const float* x, float* windows, int B, int C, int H, int total_w, int W, int stride, int wrap, void* stream);
int adm_window_blend(const float* windows, float* out, int B, int C, int H, int total_w, int W, int stride, int wrap, void* stream);

/* Tiled codec (adm_version() >= 121): the cross-fade that joins the windows of a tensor that went through a model window by window AFTER
 * sampling (AutoencoderKL.decode_tiled / encode_tiled: the VAE's mid-block attention is global, so it only ever sees windows of the width
 * it was trained at). THE definition. The blend's plain mean is the right fusion of model outputs inside a step; a decoder's image is
 * distorted towards ITS OWN edges by the zero padding of its stacked 3x3 convolutions, so here a window's weight falls off towards every
 * edge that has a neighbour. Layout, placement rules and refusals are those of "Windowed sampling" above: windows (B*nW,C,H,W),
 * sample-major, as adm_window_gather writes them; out (B,C,H,Wt).
 * Weights: r = W - s, the overlap of neighbouring windows. Window w, local column j, integer weight m_w(j):
 *   r == 0: m = 1.   Otherwise m = min(a, b) with
 *   a = min(2j + 1, 2r)           if the window has a left neighbour,  else 2r
 *   b = min(2(W - 1 - j) + 1, 2r) if it has a right neighbour,         else 2r
 *   open: window 0 has no left neighbour and window nW-1 no right one. circular: every window has both, except that nW == 1 has neither.
 *   m is an integer in [1, 2r], exact in fp32. With s == W/2 the weights over a column sum to the constant 2r (the linear cross-fade of
 *   two windows); with a cover above 2 it is not constant in general (the open placement Wt = 24, W = 16, s = 4 gives 24..31), hence the
 *   normalisation.
 * Output: out[b,c,y,col] = (float(m_w0)*o_w0 + float(m_w1)*o_w1 + ...) / float(m_w0 + m_w1 + ...) over the windows that cover col, in the
 *   blend's order (ascending index: the windows that reach col without wrapping, then the wrapping ones); the sum starts from the first
 *   product; every product and every addition is rounded to fp32 on its own (no contraction); the weights are summed as integers; one
 *   IEEE division. A column covered by ONE window is that window's value, copied ((m*o)/m is not o in fp32). No atomics, no table: the
 *   result depends on neither the launch geometry nor a replay.
 * u8_out: NULL, or (B,C,H,Wt) bytes: what adm_dequant_u8 gives for `out`, element for element, written from the value just computed.
 * Traffic: 4 B read per window element + 4 B (+ 1 B with u8_out) written per wide element. */
int adm_window_crossfade(const float* windows, float* out, uint8_t* u8_out /* may be NULL */, int B, int C, int H, int total_w, int W,
                         int stride, int wrap, void* stream);

/* scheduler.add_noise (rows S4,P3,T3): out[b][n][p] = sa[b*cb+n*cn]*x0[b*x0_bstride+p] + sb[..]*noise[b*P+p];
 * sa/sb are device arrays (sqrt(acp[t]), sqrt(1-acp[t])). */
int adm_add_noise(const float* x0, long x0_bstride, const float* noise, const float* sa, const float* sb,
                  int cb, int cn, float* out, int B, int N, long P, void* stream);

/* Training prologue of a v_prediction model (adm_version() >= 111): per sample b over P elements, with sa, sb device arrays of B floats,
 *   noisy_out[b][p]    = sa[b]*x0[b][p] + sb[b]*noise[b][p]      (bit-identical to adm_add_noise with cb = 1, cn = 0, N = 1)
 *   velocity_out[b][p] = sa[b]*noise[b][p] - sb[b]*x0[b][p]      (the regression target; diffusers' get_velocity)
 * One read of x0 and noise, two writes. P % 4 == 0. */
int adm_noise_and_velocity(const float* x0, const float* noise, const float* sa, const float* sb, float* noisy_out,
                           float* velocity_out, int B, long P, void* stream);

/* (x/2+0.5).clamp(0,1)*255 round-half-even -> u8 (pipeline_audio_diffusion.py:192-194). */
int adm_dequant_u8(const float* x, uint8_t* out, long n, void* stream);
/* AudioDiffusionPipeline.slerp (pipeline_audio_diffusion.py:244-258) for a whole grid of interpolation weights at once:
 * out (n_alpha, n) = sin((1-alpha) theta) x0 / sin(theta) + sin(alpha theta) x1 / sin(theta), theta the angle between x0 and
 * x1 (n floats each); alphas_dev: device double[n_alpha] (the reference evaluates sin((1 - alpha) * theta) on Python doubles); scratch3: device double[3]. */
int adm_slerp_grid(const float* x0, const float* x1, long n, const double* alphas_dev, int n_alpha, float* out,
                   double* scratch3, void* stream);

/* ---------------------------------------------------------------- op-level entry points (parity tests)
 * GroupNorm statistics over a (virtually concatenated) NCHW input: writes per-(n,c) scale/shift with
 *   scale = rstd*gamma[c], shift = beta[c] - mean*scale   (torch.nn.GroupNorm, biased variance). */
int adm_groupnorm_stats(const float* x1, int C1, const float* x2, int C2, int N, int HW, int groups, float eps,
                        const float* gamma, const float* beta, float* scale, float* shift, void* stream);

/* Fused 2-D convolution (rows U2-U5,U7,U8): implicit GEMM on v_mfma_f32_32x32x2_f32.
 *   in  = concat(x1[C1], x2[C2]) (x2 may be NULL), optional nearest x2 upsample (up=1) or zero-insertion x2 (up=2,
 *         the transposed stride-2 conv of the backward pass) of the input,
 *   optional per-(n,c) affine (gn_scale/gn_shift from adm_groupnorm_stats) and SiLU (act=1) applied on load,
 *   out = conv(in, w, stride, pad) + bias[co] + chan_add[n][co] (NULL ok) + residual[n][co][y][x] (NULL ok).
 * wpacked: weights repacked by adm_pack_conv_weight to [Cin][ks*ks][Cout]. H,W are the *source* dims of x1/x2.
 * pad_lo is the top/left zero padding (1 for ks=3 "same"; 0 with stride 2 gives diffusers' (0,1,0,1) pad). */
typedef struct adm_conv_args {
  const float* x1; int C1;
  const float* x2; int C2;
  int N, H, W;
  int up, stride, ks, pad_lo;
  const float* gn_scale; const float* gn_shift; int act;
  const float* wpacked; const float* bias; int Cout;
  const float* chan_add; int chan_add_stride;
  const float* residual;
  float* out;
  /* optional (0 = default): batch strides in elements of x1/x2 when they are channel slices of wider tensors, and
   * of `wpacked` when every sample has its own weights (activation x activation products, e.g. Q K^T). */
  long x1_bstride, x2_bstride, w_bstride;
  /* optional: the same 3x3 weights pre-transformed by adm_pack_winograd_weight ([Cin][16][Cout]); when present and the
   * shape is eligible (stride 1, output >= 8x16) the Winograd F(2x2,3x3) kernel may be used (ADM_CONV_WINO=1). */
  const float* wino_packed;
  /* optional: the same 3x3 weights as bf16 MFMA operands (adm_pack_bf16_weight: [tap][Cin/8][Cout][8] bf16); used when
   * option "conv_bf16" is on and the shape is eligible (stride 1, output a multiple of 16x16, Cout % 128 == 0). */
  const void* bf16_packed;
  /* optional: GroupNorm statistics of the OUTPUT, produced by the convolution's own epilogue instead of a separate read
   * pass: per (sample, output channel, pixel tile) the fp64 pair (sum, sum of squares) of the final output values,
   * stats_out[((n * Cout + c) * stats_tiles + tile) * 2 + {0, 1}]. stats_tiles must equal adm_conv_stats_tiles(args) (> 0
   * only for the kernels that can do it: the Winograd v4 kernel and the conv_in class kernel (Cin <= 4, W % 4 == 0));
   * adm_groupnorm_finalize turns them into scale / shift. */
  double* stats_out; int stats_tiles;
  /* optional (0 = the process-wide "wino6" option decides): this call's own F(4x4) layer rule, same values as the option (1 default rule,
   * 2 every layer the kernel tiles, n >= 16 planes of at least n x n pixels). A model handle carries one (adm_unet_set_option), so that a
   * single-sample front end can run the latency rule on ITS model without touching other models in the process. Since adm_version() 103. */
  int wino6_rule;
  /* optional (0 = the process-wide "single_sample" option decides; 1 on; -1 off): this call's (its model's) single-sample partition rules —
   * see the option. Since adm_version() 104. */
  int single_sample;
} adm_conv_args;
/* number of statistic tiles per (sample, channel) the kernel chosen for these arguments would emit, 0 = it cannot. */
int adm_conv_stats_tiles(const adm_conv_args* a);
/* GroupNorm scale / shift (as adm_groupnorm_stats) from the per-tile partial sums of one tensor or of a virtual concat
 * (x1 | x2) whose parts were produced by different convolutions (stats2 NULL / C2 0: one part); HW = pixels per channel. */
int adm_groupnorm_finalize(const double* stats1, int C1, int tiles1, const double* stats2, int C2, int tiles2, int N, int HW,
                           int groups, float eps, const float* gamma, const float* beta, float* scale, float* shift,
                           void* stream);
int adm_conv2d(const adm_conv_args* a, void* stream);
/* Test aid (adm_version() >= 120): adm_conv2d announced the way the executors announce a convolution whose output a GroupNorm (gamma, beta:
 * Cout floats; groups; eps) reads next. Where a launcher honours the announcement and option "gn_fuse_finish" is on, the launch's finish
 * pass leaves that GroupNorm's scale / shift (N x Cout floats each, as adm_groupnorm_stats) and *taken = 1; otherwise the call is adm_conv2d,
 * scale / shift are not written and *taken = 0. `out` is bit-identical either way. The launchers that honour it: the split-K launches of the
 * fp32 implicit-GEMM kernels on planes of at most 8x8 pixels (with "conv_wino" = 0 and "conv_bf16" = 0 the only ones) and, where they run,
 * the split Winograd launch of the single-sample rule and the blocked 16-bit route: *taken reports whichever of them took it. */
int adm_conv2d_gn_finish(const adm_conv_args* a, const float* gamma, const float* beta, int groups, float eps, float* scale, float* shift,
                         int* taken, void* stream);
/* (Cout,Cin,ks,ks) -> [Cin][ks*ks][Cout]; both device pointers. */
int adm_pack_conv_weight(const float* w, float* wpacked, int Cout, int Cin, int ks, void* stream);
/* Backward-data form: (Cout,Cin,ks,ks) -> [Cout][ks*ks][Cin] (channel-transposed, spatially flipped). Feeding it to
 * adm_conv2d with x1 = dy (Cout channels) yields d(input): stride-1 convs directly; stride-2 convs with up = 2
 * (zero-insertion); nearest-upsampled convs give the gradient at the upsampled resolution (then adm_sumpool2x2). */
int adm_pack_conv_weight_T(const float* w, float* wpT, int Cout, int Cin, int ks, void* stream);
/* Number of floats a Winograd filter buffer (wu: transposed = 0, wuT: transposed = 1) must hold: the F(2x2,3x3) image (16 per filter) and,
 * where the channel counts allow conv_wino6_kernel (128 | output channels, 32 | input channels of the packed convolution), the F(4x4,3x3)
 * image (36 per filter) behind it. adm_version() >= 102. */
long adm_winograd_packed_floats(int Cout, int Cin, int transposed);
/* (Cout,Cin,3,3) -> Winograd-domain weights U = G g G^T into a buffer of adm_winograd_packed_floats(Cout, Cin, 0) floats (kernel-specific
 * layouts: [Cin][16][Cout], or the MFMA-fragment images of conv_wino4/5/6_kernel); both device pointers. */
int adm_pack_winograd_weight(const float* w, float* wu, int Cout, int Cin, void* stream);
/* ... of the data-gradient convolution (input channels = Cout, output channels = Cin, taps flipped): [Cout][16][Cin].
 * Pass it as `wino_packed` together with adm_pack_conv_weight_T's packing to run the backward-data pass of a 3x3
 * stride-1 Conv2d (what torch autograd does for scripts/train_unet.py:262 `accelerator.backward(loss)`). */
int adm_pack_winograd_weight_T(const float* w, float* wuT, int Cout, int Cin, void* stream);
/* (Cout,Cin,3,3) fp32 -> bf16 (round-to-nearest-even) MFMA operand layout [tap][Cin/8][Cout][8]; transposed != 0 packs
 * the data-gradient filters instead ([flipped tap][Cout/8][Cin][8]). 2 bytes per weight; both device pointers. */
int adm_pack_bf16_weight(const float* w, void* wb, int Cout, int Cin, int transposed, void* stream);
/* the same for (Cout,Cin,ks,ks), ks = 3 or 1 (1x1: [Cin/8][Cout][8]; used when option "conv_bf16" = 2 also puts the
 * 1x1 convolutions on bf16 operands — opt-in, see k_conv1x1_bf16.hip). */
int adm_pack_bf16_weight_ks(const float* w, void* wb, int Cout, int Cin, int ks, int transposed, void* stream);
void adm_conv_out_dims(int H, int W, int up, int stride, int ks, int pad_lo, int* Ho, int* Wo);

/* Self-attention core (row U6): qkv is (N, 3*C, T) with channels [q | k | v], head h = channels
 * [h*d, (h+1)*d); out (N, C, T) = softmax(q^T k * d^-0.5) v per head, fp32 softmax. */
int adm_attention(const float* qkv, float* out, int N, int C, int T, int head_dim, void* stream);

/* Transformer2DModel pieces of UNet2DConditionModel (scripts/train_unet.py:139-159; diffusers transformer_2d.py /
 * attention.py), all on (N, C, T) activations:
 *   adm_layernorm_nct: LayerNorm over the channel axis for every token (norm1/2/3 of BasicTransformerBlock).
 *   adm_geglu: (N, 2*C4, T) = [h | gate] -> (N, C4, T) = h * gelu(gate) (exact erf GELU).
 *   adm_cross_attention: tokens attend to the encoding ctx (N, S, Dc) through to_k / to_v weights (C, Dc), q given.
 *   adm_attention_blocked: adm_attention with the keys in blocks of `key_block` (0 = 64 KiB of K+V) and an online
 *   softmax; adm_attention switches to it by itself when a head's K/V exceed 64 KiB.
 *   Round 5: for head_dim 16 / 32 / 64 and T % 128 == 0 (T % 256 for head_dim <= 32) — the Transformer2DModel blocks of the conditional UNet —
 *   adm_attention runs the flash form on the f32 matrix pipe (attention_mfma_kernel: both products on v_mfma_f32_16x16x4_f32, online softmax;
 *   the choice depends on the layer's shape only). */
int adm_layernorm_nct(const float* x, const float* gamma, const float* beta, float* y, int N, int C, long T, float eps,
                      void* stream);
int adm_geglu(const float* in, float* out, int N, int C4, long T, void* stream);
int adm_cross_attention(const float* q, const float* ctx, const float* Wk, const float* Wv, float* out, int N, int C, int T,
                        int S, int Dc, int head_dim, void* stream);
int adm_attention_blocked(const float* qkv, float* out, int N, int C, int T, int head_dim, int key_block, void* stream);
/* 1 if adm_attention runs this shape on the f32 matrix pipe (attention_mfma_kernel), 0 if on the VALU kernels. */
int adm_attention_mfma_eligible(int C, int T, int head_dim);
/* Backward passes of the three (training of the conditional UNet, scripts/train_unet.py:254-259 with --encodings):
 *   adm_layernorm_nct_backward: dx (accumulate != 0: +=), dgamma += , dbeta += ; stats: 2*N*T floats of scratch.
 *   adm_geglu_backward: d(in) (N, 2*C4, T) from dy (N, C4, T).
 *   adm_cross_attention_backward: dq (N, C, T); dWk, dWv (C, Dc) += (atomics). The encoding receives no gradient. */
int adm_layernorm_nct_backward(const float* x, const float* dy, const float* gamma, float* dx, int accumulate, float* stats,
                               float* dgamma, float* dbeta, int N, int C, long T, float eps, void* stream);
int adm_geglu_backward(const float* in, const float* dy, float* din, int N, int C4, long T, void* stream);
/* adm_attention_backward for any token count: keys / queries in LDS blocks of `block` (0 = 64 KiB), probabilities
 * recomputed; stats: 3 * N * (C / head_dim) * T floats of scratch. */
int adm_attention_backward_blocked(const float* qkv, const float* dout, float* dqkv, float* stats, int N, int C, int T,
                                   int head_dim, int block, void* stream);
int adm_cross_attention_backward(const float* q, const float* ctx, const float* Wk, const float* Wv, const float* dy,
                                 float* dq, float* dWk, float* dWv, int N, int C, int T, int S, int Dc, int head_dim,
                                 void* stream);

/* AudioEncoder (audiodiffusion/audio_encoder.py:62-84; produces the `encoding` of the conditional models), eval mode:
 *   adm_sepconv_block: ConvBlock = depthwise 3x3 (no bias, dw (Ci,1,3,3)) -> pointwise 1x1 (pw (Co,Ci), pb) ->
 *     LeakyReLU(slope) -> BatchNorm2d folded to bn_scale/bn_shift -> MaxPool 2x2; x (N,Ci,H,W) -> y (N,Co,H/2,W/2);
 *     tmp: N*Ci*H*W floats of scratch.
 *   adm_dense_act: y (N,J) = post(b + W x), W (J,K); leaky != 0 applies LeakyReLU(slope), post_scale/shift (NULL ok) a
 *     folded BatchNorm1d; hwc_C > 0 reads x (N, hwc_C, K/hwc_C) as if flattened in NHWC order (DenseBlock, :55). */
int adm_sepconv_block(const float* x, const float* dw, const float* pw, const float* pb, const float* bn_scale,
                      const float* bn_shift, float slope, float* tmp, float* y, int N, int Ci, int Co, int H, int W,
                      void* stream);
int adm_dense_act(const float* x, const float* W, const float* b, const float* post_scale, const float* post_shift,
                  float slope, int leaky, float* y, int N, int K, int J, int hwc_C, void* stream);

/* ---------------------------------------------------------------- UNet2DModel executor (rows U1-U8)
 * Replaces `self.unet(images, t)["sample"]` (pipeline_audio_diffusion.py:163,237; train_unet.py:257). */
typedef struct adm_unet adm_unet_t;
typedef struct adm_unet_config {
  int in_channels, out_channels, layers_per_block, n_blocks;
  int block_out_channels[8];
  int down_attn[8]; /* 1 = AttnDownBlock2D, 2 = CrossAttnDownBlock2D (UNet2DConditionModel) */
  int up_attn[8];   /* 1 = AttnUpBlock2D,   2 = CrossAttnUpBlock2D */
  int attention_head_dim, norm_num_groups; /* conditional model: attention_head_dim is the NUMBER of heads (diffusers 0.24) */
  float norm_eps;
  int flip_sin_to_cos;
  float freq_shift;
  int sample_h, sample_w;
  /* > 0: UNet2DConditionModel (scripts/train_unet.py:139-159): width of the encoding; the mid block is then
   * UNetMidBlock2DCrossAttn and adm_unet_set_encoding must be called before a forward / sample loop. */
  int cross_attention_dim;
} adm_unet_config;

int adm_unet_create(const adm_unet_config* cfg, adm_unet_t** out);
/* Per-MODEL options (adm_version() >= 103; "single_sample" >= 104: 0 = follow the process-wide option, 1 = on, -1 = off for this model —
 * AudioDiffusion sets 1: one 256x256 sample per call 6.6 -> 4.2 ms per step, profiles/r06_single_sample.md). "wino6": this model's F(4x4) layer rule — 0 = follow the process-wide option (default), 1 / 2 /
 * n >= 16 as adm_set_option("wino6", .). `audiodiffusion.AudioDiffusion` (the reference's single-sample facade, audiodiffusion/__init__.py:58-68:
 * batch_size is forced to 1) sets 256 on its own model: planes whose 16x16x128 tiles fill the chip with ONE sample keep F(4x4), the
 * levels below run the 64-cout F(2x2) kernel, whose smaller tiles are 4x as many workgroups (256x256, one sample: 6.8 instead of 8.3 ms per
 * step). The rule stays a function of the layer and the model — never of the batch — so rows of one model's batches remain bit-identical to
 * single-sample runs of THAT model. Re-plans the model (drops a captured loop). */
int adm_unet_set_option(adm_unet_t* h, const char* name, int value);
void adm_unet_destroy(adm_unet_t* h);
/* Upload one parameter by its diffusers state-dict key (host pointer, fp32, `numel` elements).
 * Deprecated attention names (query/key/value/proj_attn, audiodiffusion/utils.py:41-54) are accepted. */
int adm_unet_set_param(adm_unet_t* h, const char* key, const float* host_data, size_t numel);
/* Conditional model: encoder_hidden_states for the following forwards / sample loops — device pointer (B, seq_len,
 * cross_attention_dim) fp32, owned by the caller and kept alive until replaced
 * (`self.unet(images, t, encoding)`, pipeline_audio_diffusion.py:160-161). */
int adm_unet_set_encoding(adm_unet_t* h, const float* encoding_dev, int seq_len);
/* Number of parameters still missing after the set_param calls (0 = ready); names via adm_last_error(). */
int adm_unet_missing_params(adm_unet_t* h);
/* eps = unet(x, t): x,out (B,Cin,H,W)/(B,Cout,H,W) device; timesteps: B floats on the HOST (or 1 broadcast). */
int adm_unet_forward(adm_unet_t* h, const float* x, const float* timesteps_host, int n_timesteps, float* out,
                     int B, void* stream);
size_t adm_unet_workspace_bytes(adm_unet_t* h);
/* Measurement aid (bench.py roofline leg): one eager forward with a HIP-event pair around every launch on `stream`.
 * kind: 0 GroupNorm stats, 1 MFMA conv, 2 attention core, 3 direct small-channel conv, 4 time-embedding projection.
 * variant (MFMA conv): ks*100 + stride*10 + cout_tile/32, +2000 for the software-pipelined kernel
 * (conv_mfma_pf_kernel); 1001/1002 = direct small-Cin / small-Cout kernels. flops/bytes are ALGORITHMIC. */
typedef struct adm_op_profile { int kind, variant; float ms; double flops, bytes; } adm_op_profile;
int adm_unet_profile(adm_unet_t* h, const float* x, float timestep, float* out, int B, adm_op_profile* recs, int cap,
                     int* n_out, void* stream);
/* Test aid (adm_version() >= 105): the inference plan of a net at batch B, one record per op in list order — what each op reads and writes and
 * where the side-stream overlap ("side_overlap") launches it. Plans the net at B first if it is not planned (outside any capture, exactly as a
 * forward would; a UNet's captured loop is dropped then). Byte ranges come from the arguments the launches are made with (adm_conv_args for
 * convolutions, including the statistics epilogue and the GroupNorm scale / shift a split-K finish pass may leave); they may over-approximate
 * (a channel slice reports the span of every sample's slice) and never under-approximate the plan's own memory. The network input and output
 * and the per-stream split-K slab are not plan memory: the first two appear by tensor id only, the slab not at all (each stream has its own).
 * n_out receives the op count; at most cap records are written. */
#define ADM_PLAN_GN_LOAD 1        /* convolution: GroupNorm affine on its load path */
#define ADM_PLAN_ACT 2            /* convolution: SiLU on its load path */
#define ADM_PLAN_STATS 4          /* convolution: GroupNorm partial sums from its epilogue (stats_out) */
#define ADM_PLAN_PER_SAMPLE_W 8   /* convolution: weights taken from an activation tensor */
#define ADM_PLAN_GN_FUSE 16       /* convolution: offered the scale / shift of GroupNorm op gn_fuse (its split-K finish pass may write them) */
#define ADM_PLAN_MAX_T 4
#define ADM_PLAN_MAX_R 12
typedef struct adm_plan_range { uint64_t lo, hi; } adm_plan_range;   /* device bytes [lo, hi) */
typedef struct adm_plan_op {
  int kind;        /* 0 GroupNorm statistics, 1 convolution, 2 attention core, 3 channel softmax (in place), 4 transpose, 5 LayerNorm, 6 GEGLU,
                    * 7 cross-attention */
  int hoist_from;  /* -1: in place; i >= 0: launched on the side stream in front of op i and joined at its own position */
  int ks, stride, up, flags, gn_fuse;             /* convolutions (gn_fuse: the GroupNorm op offered, -1 none) */
  int n_tread, n_twrite;
  int tread[ADM_PLAN_MAX_T], twrite[ADM_PLAN_MAX_T];   /* activation tensor ids */
  int n_read, n_write;
  adm_plan_range read[ADM_PLAN_MAX_R], write[ADM_PLAN_MAX_R];
} adm_plan_op;
int adm_unet_plan_ops(adm_unet_t* h, int B, adm_plan_op* recs, int cap, int* n_out);

/* ---- training (rows T4,T5; scripts/train_unet.py:257-259): the master parameters live in ONE caller-owned flat fp32
 * device buffer (so the fused optimizer kernel can update them in a single launch); call order:
 *   create -> adm_unet_bind_param for every key -> adm_unet_enable_training -> adm_unet_forward_backward ...
 *   -> (optimizer step on the flat buffer) -> adm_unet_refresh_weights -> next step. */
int adm_unet_bind_param(adm_unet_t* h, const char* key, float* dev_ptr);
int adm_unet_enable_training(adm_unet_t* h, const float* params_base, long numel);
int adm_unet_refresh_weights(adm_unet_t* h, void* stream);
/* loss_dev[0] = mean((unet(x,t) - target)^2); grads_base (flat, same offsets as the parameter buffer) = d loss/d params.
 * Every activation is kept for the reverse pass; GroupNorm/SiLU are recomputed in the weight-gradient load path. */
int adm_unet_forward_backward(adm_unet_t* h, const float* x, const float* timesteps_host, int n_timesteps,
                              const float* target, float* loss_dev, float* grads_base, int B, void* stream);
/* `--mixed_precision fp16`: the factor the loss gradient is multiplied with before the reverse pass (GradScaler's scale;
 * 1 = off). The gradients adm_unet_forward_backward writes then carry it: un-scale with adm_grad_norm_clip_scaled. */
int adm_unet_set_loss_scale(adm_unet_t* h, float scale);
/* Data-parallel overlap (DistributedDataParallel's bucketed all-reduce running under autograd, train_unet.py:259): cut the
 * flat gradient buffer into n_buckets ranges [bounds[b], bounds[b+1]) (elements, ascending, n_buckets + 1 values);
 * fn(user, b) is called on the calling thread during adm_unet_forward_backward as soon as the last kernel writing into
 * bucket b has been ENQUEUED on the stream — queue the bucket's all-reduce behind it (RCCL orders after the stream) while
 * the rest of the reverse pass runs. Buckets holding a parameter the pass never touches do not fire: reduce those after
 * the call returns. n_buckets = 0 removes the hook. */
typedef void (*adm_bucket_fn)(void* user, int bucket);
int adm_unet_set_grad_bucket_hook(adm_unet_t* h, int n_buckets, const long* bounds, adm_bucket_fn fn, void* user);

/* ---------------------------------------------------------------- whole denoising loop (row P4; hipGraph)
 * Runs n_steps x {UNet forward, scheduler epilogue, mask} on `x` in place and (optionally) the final u8 image.
 * coef_host: n_steps adm_sched_coef (host) including .timestep; step_noise: NULL or device
 * (n_steps,B,C,H,W) noise consumed where k_noise != 0. With use_graph=1 one step is captured into a hipGraph
 * and replayed n_steps times (step-dependent scalars come from a device table indexed by a device counter).
 *
 * What keys the captured step (every loop entry point below refers to this paragraph). A handle holds ONE captured step, keyed by everything its launches were given:
 * the addresses of the caller's tensors (x, step_noise, mask, u8_out, encoding_uncond, known, known_noise, keep), B, n_steps, mask_start,
 * mask_end, mode, prediction, the stream, the encoding set on the handle, the addresses of the handle's device tables, and the values of
 * the features that are ON: lo, hi and the bits of w and max_value in mode 1; the bits of guidance_scale and guidance_rescale with
 * encoding_uncond; window_stride and window_wrap with window_total_w; the two batched flags with keep. A loop whose key equals the stored
 * one replays the stored graph, so the following all replay: new CONTENTS at the same addresses (x, the noise, the mask, the encodings, the
 * known-region tensors), new values in any *_host table of the same n_steps, another seed or row_offset, and any value in a field of a
 * feature that is off. Any other difference captures again and replaces the stored step, so one handle may alternate between any two
 * loops; a new plan (another B, adm_unet_set_option) forgets the step as well. use_graph=0 neither uses nor changes it. */
int adm_sample_loop(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, int n_steps,
                    const float* step_noise, const float* mask, int mask_start, int mask_end,
                    uint8_t* u8_out, int use_graph, void* stream);
/* adm_sample_loop with the multistep epilogue (adm_sched_multistep; adm_version() >= 109). k_hist_host: n_steps floats (host),
 * k_hist_host[0] must be 0 (the first row of a run is first order: the history buffer, which the handle owns and allocates with its
 * plan, holds nothing of this run yet). coef_host[i].timestep feeds the time embedding as in adm_sample_loop. */
int adm_sample_loop_multistep(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, const float* k_hist_host,
                              int n_steps, const float* step_noise, const float* mask, int mask_start, int mask_end,
                              uint8_t* u8_out, int use_graph, void* stream);
/* adm_sample_loop with the dynamically thresholded epilogue (adm_sched_step_thresholded; adm_version() >= 110): every step runs the
 * selection and then the thresholded step kernel between the forward and the step counter's increment, inside the captured graph. lo, hi, w
 * as in adm_sched_threshold for n = in_channels * sample_h * sample_w; the per-sample scale buffer belongs to the handle's plan. */
int adm_sample_loop_thresholded(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, int n_steps,
                                const float* step_noise, const float* mask, int mask_start, int mask_end,
                                uint8_t* u8_out, int use_graph, void* stream, int lo, int hi, float w, float max_value);
/* adm_sample_loop / adm_sample_loop_thresholded for a model of the given `prediction` (0 epsilon, 1 sample, 2 v_prediction; adm_sched_step_pred;
 * adm_version() >= 111). thresholded == 0: the static clamp, and lo, hi, w, max_value are ignored. One handle may alternate between types
 * ("what keys the captured step" above). */
int adm_sample_loop_pred(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, int n_steps,
                         const float* step_noise, const float* mask, int mask_start, int mask_end,
                         uint8_t* u8_out, int use_graph, void* stream, int lo, int hi, float w, float max_value,
                         int thresholded, int prediction);
/* The sampling loops with classifier-free guidance (adm_sched_step_guided; adm_version() >= 112). The handle must be conditional and have
 * an encoding set (adm_unet_set_encoding): that is the conditional branch. encoding_uncond_dev: device, the shape of the set encoding
 * (B, seq_len, cross_attention_dim), the unconditional branch (zeros for a model trained with dropped encodings). Every step runs TWO forwards of
 * batch B on the same plan, the second with the encoding pointer swapped and into a second output buffer that the handle allocates with its
 * plan on the first guided call at a batch size, then one guided step kernel; all inside the one captured step. A sample's bits do not
 * depend on its batch, and encoding_uncond_dev equal to the set encoding gives the unguided loop's bits. k_hist_host != NULL: the multistep
 * loop (k_hist_host[0] == 0, prediction == 0, thresholded == 0); otherwise as adm_sample_loop_pred. The handle's encoding is unchanged on
 * return. */
int adm_sample_loop_guided(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, const float* k_hist_host, int n_steps,
                           const float* step_noise, const float* mask, int mask_start, int mask_end,
                           uint8_t* u8_out, int use_graph, void* stream, int lo, int hi, float w, float max_value,
                           int thresholded, int prediction, const float* encoding_uncond_dev, float guidance_scale);
/* adm_sample_loop_pred / adm_sample_loop_guided with the step noise drawn inside the step kernel (adm_sched_step_philox; adm_version() >=
 * 113): no noise tensor, whatever n_steps. row_offset: the global row of x[0] (a shard's first row). encoding_uncond_dev == NULL: unguided,
 * and the model may be unconditional; otherwise as adm_sample_loop_guided. The handle owns a 16-byte device block {seed_lo, seed_hi,
 * row_offset, stream id} that the step kernel reads through a pointer, as it reads the step index; this call rewrites it with a
 * stream-ordered copy before the first step, outside the captured step: another seed or another row_offset replays the same graph (the block's
 * address is stable for the life of the handle). Every coef_host[i].timestep must be in [0, 2^31). */
int adm_sample_loop_philox(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, int n_steps,
                           const float* mask, int mask_start, int mask_end,
                           uint8_t* u8_out, int use_graph, void* stream, int lo, int hi, float w, float max_value,
                           int thresholded, int prediction, const float* encoding_uncond_dev, float guidance_scale,
                           uint64_t seed, int row_offset);
/* The sampling loop as ONE entry point (adm_version() >= 114); the struct grows as adm_sched_step_args does, and no loop symbol is added.
 * FROZEN: adm_sample_loop, adm_sample_loop_multistep, adm_sample_loop_thresholded, adm_sample_loop_pred, adm_sample_loop_guided and
 * adm_sample_loop_philox keep their signatures and results; each fills this struct and calls adm_sample_loop_ex.
 * mode, prediction, lo, hi, w, max_value, guidance_scale, noise_source, seed, row_offset: as adm_sched_step_args (the scale, history and
 * second output buffers are the handle's). k_hist_host: mode 2, n_steps host floats, k_hist_host[0] == 0. encoding_uncond: NULL, or the
 * device encoding of the unconditional branch (adm_sample_loop_guided). step_noise: NULL with noise_source 1. */
typedef struct adm_sample_loop_args {
  float* x;
  int B;
  const adm_sched_coef* coef_host;
  const float* k_hist_host;
  int n_steps;
  const float* step_noise;
  const float* mask;
  int mask_start, mask_end;
  uint8_t* u8_out;
  int use_graph;
  int mode, prediction;
  int lo, hi;
  float w, max_value;
  const float* encoding_uncond;
  float guidance_scale;
  int noise_source;
  uint64_t seed;
  int row_offset;
  float guidance_rescale;    /* adm_version() >= 115: "guidance rescale" above; 0: off; otherwise needs encoding_uncond */
  const adm_unipc_coef* unipc_host;   /* adm_version() >= 116: NULL, or n_steps host rows: the UniPC loop ("UniPC" above; mode 0 or 1, any
                                prediction, step_noise NULL and noise_source 0). Row 0 must have c_t == 0 && p_m1 == 0 (a run starts
                                without state). The handle owns `last` and the two history slots */
  int window_total_w, window_stride, window_wrap;   /* adm_version() >= 117: "Windowed sampling" above. window_total_w == 0: off, and the
                                other two are ignored. Otherwise x and u8_out are (B,C,sample_h,window_total_w), step_noise is
                                (n_steps,B,C,sample_h,window_total_w), B counts WIDE samples, the handle is planned at batch B*nW (its
                                encodings have B*nW rows, sample-major) and one captured step is: gather into a handle-owned window
                                buffer, the forward(s) at batch B*nW, one blend per forward output into handle-owned wide buffers, the
                                step at W = window_total_w, the counter's increment. One handle may alternate windowed and ordinary
                                loops. Refused by name: mask != NULL, and every placement rule (window_total_w, window_stride,
                                window_wrap) */
  const float* known;        /* adm_version() >= 118: "Region in-painting" above, as adm_sched_step_args; with window_total_w the three */
  const float* known_noise;  /* tensors have the wide shape. One handle may alternate loops with and without it. known_coef_host: */
  const uint8_t* keep;       /* n_steps x 2 HOST floats (ka, kb), row i beside coef_host[i]. keep == NULL: off, and the other five are */
  const float* known_coef_host;   /* ignored. Refused by name as in adm_sched_step_ex */
  int known_batched, keep_batched;
} adm_sample_loop_args;
int adm_sample_loop_ex(adm_unet_t* h, const adm_sample_loop_args* a, void* stream);
/* DDIM inversion (row P6, pipeline_audio_diffusion.py:228-240; the other prediction types, the conditional model and the windowed loop:
 * adm_version() >= 123). x is the sample at level s, o the model output, t the target level and c the level of the timestep the model was
 * given; sa = sqrt(alphas_cumprod), sb = sqrt(1 - alphas_cumprod):
 *   e  = o (epsilon)     e = (x - sa_c*o) / sb_c (sample)     e = sa_c*o + sb_c*x (v_prediction)       -- the table of adm_sched_step_pred
 *   x' = ((x - sb_s*e) * (1/sa_s)) * sa_t + sb_t*e
 * What the eight adm_sched_coef fields mean in an inversion row:
 *   sqrt_beta = sb_s    sqrt_alpha = 1/sa_s (NOT sa_s)    k_x0 = sa_t    k_eps = sb_t    timestep = the timestep the model is given
 *   k_x = sa_c          k_noise = sb_c                    clip: not read (the schedulers write -1)
 * An epsilon row reads neither k_x nor k_noise (the schedulers leave both 0 there, as before version 123). The reference's rule gives
 * the model the TARGET timestep (c = t); the textbook rule gives it the sample's own (c = s, DDIMScheduler.encode_rows(level="matched")).
 * On a zero-SNR row (sa_c = 0, sb_c = 1) the two new forms give e = x and stay finite; a sample row with sb_c = 0 is out of contract, as
 * in adm_sched_step_pred. A first row with sa_s = 1, sb_s = 0 (final_alpha_cumprod = 1) leaves x0 = x exactly.
 * adm_encode_step: ONE step on n elements (n % 4 == 0), in place; row = step_dev ? *step_dev : step; prediction 0, 1, 2 as above. */
int adm_encode_step(float* x, const float* model_out, const adm_sched_coef* coef_table, const int* step_dev, int step, int prediction,
                    long n, void* stream);
/* The inversion loop (adm_version() >= 123): per step the forward at coef_host[i].timestep, then adm_encode_step. It takes the struct of
 * adm_sample_loop_ex and honours x, B, coef_host, n_steps, use_graph, prediction and window_total_w / window_stride / window_wrap (the
 * windowed step is the sampling loop's: gather, ONE forward at batch B*nW, blend, the inversion step at the wide shape). Every other
 * field must be NULL / 0 and is refused by its name otherwise (mode included: adm_sample_loop_ex in turn has no inversion mode). A
 * conditional handle reads its encoding (adm_unet_set_encoding; B*nW rows, sample-major, when windowed); there is no guided inversion.
 * The captured step is keyed as the sampling loop's: new table values at the same n_steps replay, another prediction or window
 * placement captures again, and one handle may alternate inversion and sampling loops.
 * FROZEN: adm_encode_loop keeps its signature and results (epsilon, unconditional or not, the model's width); it fills the struct and
 * calls adm_encode_loop_ex. */
int adm_encode_loop_ex(adm_unet_t* h, const adm_sample_loop_args* a, void* stream);
int adm_encode_loop(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, int n_steps, int use_graph,
                    void* stream);
/* Test aid (adm_version() >= 122): how many times this handle has captured a step since it was created (0 for NULL). The emulation build
 * has no graphs and runs every step eagerly; it keeps the key and counts at the same point, so "what keys the captured step" above is
 * checked on both builds (tests/test_loop_graph_key.py). */
int adm_unet_loop_captures(adm_unet_t* h);

/* ---------------------------------------------------------------- AutoencoderKL executor (rows V1-V3, config 4)
 * Replaces `vqvae.encode(x).latent_dist.sample(generator)` (pipeline_audio_diffusion.py:144; train_unet.py:104,233)
 * and `vqvae.decode(z)["sample"]` (pipeline_audio_diffusion.py:190). Architecture per audiodiffusion/utils.py:132-153:
 * Down/UpDecoderBlock2D stacks, GroupNorm eps 1e-6, single-head mid-block attention. */
typedef struct adm_vae adm_vae_t;
typedef struct adm_vae_config {
  int in_channels, out_channels, latent_channels, layers_per_block, n_blocks;
  int block_out_channels[8];
  int norm_num_groups;
  int sample_h, sample_w;
} adm_vae_config;
int adm_vae_create(const adm_vae_config* cfg, adm_vae_t** out);
void adm_vae_destroy(adm_vae_t* h);
int adm_vae_set_param(adm_vae_t* h, const char* key, const float* host_data, size_t numel);
int adm_vae_latent_dims(adm_vae_t* h, int* lat_h, int* lat_w);
/* z_out (B,Cz,h,w) = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * out_scale, noise (B,Cz,h,w) or NULL (= mode);
 * moments_out: NULL or (B,2*Cz,h,w) receives quant_conv(encoder(x)). out_scale carries the reference's 0.18215. */
int adm_vae_encode(adm_vae_t* h, const float* x, const float* noise, float out_scale, float* z_out, float* moments_out,
                   int B, void* stream);
/* out (B,Cout,H,W) = decoder(post_quant_conv(in_scale * z)); in_scale carries the reference's 1/0.18215. */
int adm_vae_decode(adm_vae_t* h, const float* z, float in_scale, float* out, int B, void* stream);
/* The tail of adm_vae_encode as a launch of its own (adm_version() >= 121; the same kernel, not a second formula): z_out (B,Cz,n) from
 * moments (B,2*Cz,n) = [mean | logvar] that the caller holds, e.g. the cross-faded moments of a tiled encode; noise (B,Cz,n) or NULL (mode). */
int adm_vae_sample_moments(const float* moments, const float* noise, float out_scale, float* z_out, int B, int Cz, long n, void* stream);
/* The plan report of adm_unet_plan_ops for the encoder (which = 0, quant_conv included) or the decoder (1, post_quant_conv included). */
int adm_vae_plan_ops(adm_vae_t* h, int which, int B, adm_plan_op* recs, int cap, int* n_out);

/* ---------------------------------------------------------------- training-step optimizer side (rows T4,T6,T7,T9)
 * scripts/train_unet.py:258-267 over FLAT fp32 buffers (all parameters / grads / moments / EMA shadow contiguous).
 * Nothing here synchronises with the host: scalars (loss, norm, clip factor) stay on the device. */
/* F.mse_loss (:258): loss_out[0] = mean((pred-target)^2); grad_out (NULL ok) = 2(pred-target)/n; scratch: double[1]. */
int adm_mse_loss(const float* pred, const float* target, long n, float* loss_out, float* grad_out, double* scratch,
                 void* stream);
/* clip_grad_norm_ (:261-262): norm_clip_out = {||g||_2, min(1, max_norm/(||g||_2+1e-6))}; scratch: double[1]. */
int adm_grad_norm_clip(const float* grads, long n, float max_norm, float* norm_clip_out, double* scratch, void* stream);
/* the same on loss-scaled gradients (`--mixed_precision fp16`: GradScaler.unscale_ + clip_grad_norm_ in one pass):
 * norm_clip_out = {||g||_2 * inv_scale, min(1, max_norm/(norm + 1e-6)) * inv_scale}; inf / nan gradients give a non-finite
 * norm, on which the caller skips the optimizer step and backs the scale off. */
int adm_grad_norm_clip_scaled(const float* grads, long n, float max_norm, float inv_scale, float* norm_clip_out, double* scratch,
                              void* stream);
/* torch.optim.AdamW step (:263; lr/betas/wd/eps :166-172) fused with the clip factor (device scalar, NULL = 1) and
 * diffusers EMAModel.step (:265-266; ema == NULL skips): shadow -= (1-ema_decay)*(shadow-param). step is 1-based. */
int adm_adamw_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, long n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int step, const float* clip_coef_dev,
                       float ema_decay, void* stream);
/* the remaining optimizer-side passes over a flat buffer, one launch each: op 0: y += x (accelerator.accumulate micro-step
 * sum, :252); 1: y = x*a (mean of the accumulated micro-gradients); 2: y /= a (DDP's 1/world, :259); 3: y -= a*(y-x)
 * (EMAModel.step on its own, a = 1-decay, :265-266). Buffers 16-byte aligned. */
int adm_flat_op(float* y, const float* x, long n, int op, float a, void* stream);

/* ---------------------------------------------------------------- backward ops of the training step (rows T5/T8)
 * What `accelerator.backward(loss)` (scripts/train_unet.py:259-262) asks torch autograd to run for the ops of
 * UNet2DModel; adm_unet_forward_backward chains them natively, these entry points expose each op for parity tests and
 * for a host that wants to drive the backward pass itself. All pointers are device pointers. */
/* adm_groupnorm_stats that also keeps (N, groups, 2) {mean, rstd} for the backward pass (mean_rstd may be NULL). */
int adm_groupnorm_stats_ex(const float* x1, int C1, const float* x2, int C2, int N, int HW, int groups, float eps,
                           const float* gamma, const float* beta, float* scale, float* shift, float* mean_rstd,
                           void* stream);
/* Backward of GroupNorm(+SiLU) applied on a conv's load path: da = gradient w.r.t. the activated tensor (virtual concat
 * of x1|x2); writes/accumulates dx1, dx2 (acc1/acc2 != 0: add) and ACCUMULATES dgamma, dbeta. s12_scratch: N*groups*2. */
int adm_groupnorm_backward(const float* x1, int C1, const float* x2, int C2, const float* da, int N, int HW, int groups,
                           const float* mean_rstd, const float* gamma, const float* beta, int act, float* s12_scratch,
                           float* dgamma, float* dbeta, float* dx1, int acc1, float* dx2, int acc2, void* stream);
/* Conv2d weight gradient dW (Cout,Cin,ks,ks) of the fused convolution described by `a` (same load-path fusions) for the
 * output gradient dy; split-K partial slabs live in `workspace` (adm_conv_wgrad_workspace floats). */
long adm_conv_wgrad_workspace(const adm_conv_args* a);
int adm_conv2d_wgrad(const adm_conv_args* a, const float* dy, float* dW, int accumulate, float* workspace, void* stream);
/* Test aids (adm_version() >= 108).
 * adm_last_wgrad_variant: what the last adm_conv2d_wgrad on this thread launched (returns `kernel`; `out` NULL or filled). The executors'
 * weight gradients go through the same launcher and report the same way. All zero before the first launch; a call that fails before it
 * launches leaves the values as they were.
 *   kernel: 310 / 320 / 110 = generic conv_wgrad_kernel<3,1> / <3,2> / <1,1> | 1300 / 1301 = conv_wgrad_pf_kernel<3,false> / <3,true> and
 *     1100 / 1101 = <1,false> / <1,true> (register prefetch; the last digit is the tile-invariant fast path) | 2304 = conv_wgrad_sp_kernel
 *     (four waves, LDS double buffer) | 2308 = conv_wgrad_sp8_kernel (eight waves) | 5316 / 5116 = the bf16-operand routes of option
 *     "conv_bf16" (3x3 / 1x1; tiles_per_block is then the fp32 launcher's figure, not theirs);
 *   reduce: 1 = wgrad_reduce_kernel, 9 = wgrad_reduce9_kernel (adm_wgrad_reduce sets this field too);
 *   split, tiles_per_block: the number of partial-sum slabs that were reduced and the pixel tiles per workgroup
 *     (tiles_per_block = ceil(n_ptiles / split0), split = ceil(n_ptiles / tiles_per_block), split0 = min(ceil(768 / (cout tiles x channel
 *     chunks)), "wgrad_max_split", n_ptiles)).
 * Option "wgrad_path" (adm_set_option) = 0 (default): the launcher's heuristic, where the developer switches ADM_WGRAD_SP8=0 / ADM_WGRAD_SP=0 /
 *   ADM_WGRAD_PF=0 of the environment still mean what 1 / 2 / 3 mean here | 1 no eight-wave kernel | 2 no software-pipelined kernels (the
 *   prefetch kernels take their shapes) | 3 generic kernels only. Any other value is an error and is not recorded.
 * adm_wgrad_reduce: the launcher's second launch alone: dW (=|+=) sum over k < split of workspace[k][0:numel], slabs in [tap][cout*cin] order,
 *   dW in (cout, cin, tap) order; taps == 9 runs wgrad_reduce9_kernel, anything else wgrad_reduce_kernel. numel % taps == 0. */
typedef struct adm_wgrad_variant { int kernel, reduce, split, tiles_per_block; } adm_wgrad_variant;
int adm_last_wgrad_variant(adm_wgrad_variant* out);
int adm_wgrad_reduce(const float* workspace, int split, long numel, float* dW, int accumulate, int taps, void* stream);
/* ---- blocked 16-bit operand images (option "conv_bf16" = 3; `--mixed_precision bf16`, scripts/train_unet.py:391-401) ----
 * A blocked image is  img[n][C/8][H+2][W+2] x 16 B : one 16-byte unit = 8 consecutive channels of one pixel as bf16 (or IEEE
 * binary16 under option "conv_op16_f16"), with a one-pixel halo that must be ZERO (zero the buffer once after allocating it:
 * adm_blocked_apply writes the interior only).  adm_blocked_image_bytes gives its size.
 *   adm_blocked_apply: img = round16(act(scale[n][c] * concat(x1, x2)[n][c] + shift[n][c])), scale / shift as produced by
 *     adm_groupnorm_stats (both NULL: identity), act != 0: SiLU — the activated conv input, written ONCE per layer; with
 *     scale = NULL, act = 0 on dy it is the operand image of the backward kernels.  C1, C2 multiples of 8, W of 4.
 *     sum_nc (N, nc_stride): NULL or receives the per-(n, c) sums of the fp32 INPUT; sum_c (C): NULL or ACCUMULATES the per-c
 *     sums (the time-embedding-bias and bias gradients when the input is dy, as adm_chan_sums); both need sum_scratch
 *     (adm_blocked_sums_scratch floats: one partial per workgroup, added in a fixed order).
 *   adm_conv2d_bf16_blocked: out (N,Cout,H,W) fp32 = conv3x3(img, stride 1, pad 1) + bias[co] + chan_add[n][co] + residual
 *     (each NULL ok), filters `wb` from adm_pack_bf16_weight (transposed = 1 and img = image of dy: the data gradient).
 *     Cin % 16 == 0, Cin >= 32, Cout % 128 == 0, H % 8 == 0, W % 32 == 0 (adm_conv2d_bf16_blocked_eligible) — or W == 16 / W == 8 with
 *     Cin >= 64 and N % 2 / N % 4 == 0: two / four images side by side in one 32-column tile, K split over workgroups and finished in
 *     slab order through the library's per-(device, stream) scratch (no stats_out, no stride-2 variant; up = 1 at W == 16 only).
 *   adm_conv2d_wgrad_bf16_blocked: dW (Cout,Cin,3,3) (+)= sum over pixels of dy x activated input, both as blocked images;
 *     Cin % 64 == 0, Cout % 128 == 0, H % 4 == 0, W % 32 == 0 (or W == 16 / 8 with N % 2 / N % 4 == 0, as above); workspace:
 *     adm_conv_wgrad_blocked_workspace floats (0 = shape not eligible for this N).
 *     stats_out: NULL or (N, Cout, (H/8)*(W/32), 2) fp64 — per 8x32-pixel tile the (sum, sum of squares) of the final output
 *     values, the input adm_groupnorm_finalize needs (as adm_conv_args.stats_out).
 *   up = 1 (both): the convolution of Upsample2D — H, W are the OUTPUT dims and the input image is the half-resolution tensor
 *     (N, Cin, H/2, W/2); the nearest x2 is folded into the patch addresses.
 *   Stride 2 (Downsample2D.conv) = every other pixel of the stride-1 "same" convolution o of the same image: adm_conv2d_bf16_blocked
 *     with up = 2 for pad (0, 1, 0, 1) + 3x3 stride 2 without padding (AutoencoderKL encoder; out(y, x) = o(2y + 1, 2x + 1)) or up = 3
 *     for 3x3 stride 2 padding 1 (UNet2DModel; out(y, x) = o(2y, 2x)) — H, W are the INPUT dims, out is (N, Cout, H/2, W/2), bias only.
 *     Its backward passes take the ZERO-INSERTED image of dy: adm_blocked_apply(zero_insert = 1 / 2 for up = 2 / 3) on dy
 *     (N, Cout, H/2, W/2) writes an image of (H, W) pixels (adm_blocked_image_bytes(N, Cout, H, W), zeroed once) with dy(y, x) on pixel
 *     (2y + 1, 2x + 1) / (2y, 2x); the data gradient is then the plain stride-1 call with the transposed filters, the weight gradient
 *     the plain call with the input's image. */
size_t adm_blocked_image_bytes(int N, int C, int H, int W);
long adm_blocked_sums_scratch(int N, int C, int H, int W);
int adm_blocked_apply(const float* x1, int C1, const float* x2, int C2, int N, int H, int W, const float* scale,
                      const float* shift, int act, int zero_insert, void* img, float* sum_scratch, float* sum_nc, int nc_stride,
                      float* sum_c, void* stream);
int adm_conv2d_bf16_blocked_eligible(int Cin, int Cout, int H, int W);
int adm_conv2d_bf16_blocked(const void* img, int Cin, int N, int H, int W, const void* wb, int Cout, const float* bias,
                            const float* chan_add, int chan_add_stride, const float* residual, float* out, int up,
                            double* stats_out, void* stream);
int adm_conv2d_wgrad_bf16_blocked_eligible(int Cin, int Cout, int H, int W);
long adm_conv_wgrad_blocked_workspace(int Cin, int Cout, int N, int H, int W);
int adm_conv2d_wgrad_bf16_blocked(const void* x_img, int Cin, const void* dy_img, int Cout, int N, int H, int W, float* dW,
                                  int accumulate, float* workspace, int up, void* stream);
/* gradient of the nearest-x2 upsample folded into a conv: out (planes,H/2,W/2) (+)= 2x2 sums of in (planes,H,W). */
int adm_sumpool2x2(const float* in, float* out, int H, int W, long planes, int accumulate, void* stream);
/* dst[n][0:per_sample] (+)= src[n][0:per_sample] with independent batch strides (gradient fan-in of channel slices). */
int adm_accumulate(float* dst, long dst_bs, const float* src, long src_bs, long per_sample, int N, int accumulate,
                   void* stream);
/* per-(n,c) sums of dy over HW into out_nc (time-embedding bias gradient, NULL ok) and per-c sums into out_c (bias
 * gradient, accumulated, NULL ok). */
int adm_chan_sums(const float* dy, int N, int C, int HW, float* out_nc, int nc_stride, int nc_accumulate, float* out_c,
                  void* stream);
/* backward of adm_attention: dqkv (N,3C,T) from dout (N,C,T) and the saved qkv. */
int adm_attention_backward(const float* qkv, const float* dout, float* dqkv, int N, int C, int T, int head_dim,
                           void* stream);
/* Linear Y = act(X) W^T + b: dW (J,K) += dY^T act(X), db += colsum(dY), dX = (dY W) * act'(X); x_silu: act = SiLU. */
int adm_linear_backward(const float* dY, int ldy, const float* X, const float* W, int B, int J, int K, int x_silu,
                        float* dW, float* db, float* dX, void* stream);
/* conv_in (Cin <= 4) weight gradient and conv_out (Cout <= 4) weight + data gradient (the direct small-channel kernels). Both ADD to
 * what dW holds (fp32 atomics over the samples): zero it, or pass the gradient to accumulate onto; da is written; da or dW may be NULL. */
int adm_conv_small_cin_wgrad(const float* x, int Cin, int N, int H, int W, const float* dy, int Cout, float* dW,
                             void* stream);
int adm_conv_small_cout_backward(const float* x, int Cin, int N, int H, int W, const float* gn_scale,
                                 const float* gn_shift, int act, const float* w, const float* dy, int Cout, float* da,
                                 float* dW, void* stream);

/* ---------------------------------------------------------------- Mel codec (rows M3-M8)
 * Replaces Mel.audio_slice_to_image (audiodiffusion/mel.py:135-151: librosa melspectrogram + power_to_db + u8) and
 * Mel.image_to_audio (mel.py:153-168: db_to_power + mel_to_stft NNLS + Griffin-Lim), batched over slices/images.
 * The constant tables of a configuration are computed by the host binding exactly as librosa/scipy do:
 * window (n_fft fp64, periodic Hann), twiddle (n_fft/2 complex fp64 exp(-2 pi i q/n)), the Slaney filterbank as CSR
 * (fb_start/fb_count per mel row, fb_w32/fb_w64 taps) and CSC (fbt_off/fbt_idx/fbt_w64), pinv (n_bins x n_mels fp64),
 * wss (window sum-square envelope, fp32, trimmed to hop*(x_res-1)), nnls_cols (librosa.util.nnls column blocking). */
typedef struct adm_mel adm_mel_t;
typedef struct adm_mel_config { int x_res, y_res, sample_rate, n_fft, hop_length, top_db, n_iter; } adm_mel_config;
int adm_mel_create(const adm_mel_config* cfg, const double* window, const double* twiddle, const int* fb_start,
                   const int* fb_count, const float* fb_w32, const double* fb_w64, int nnz, const int* fbt_off,
                   const int* fbt_idx, const double* fbt_w64, const double* pinv, const float* wss, int nnls_cols,
                   adm_mel_t** out);
void adm_mel_destroy(adm_mel_t* h);
/* audio: device, B slices of n_samples fp32 (is_f64=0) or fp64 (=1), slice_stride elements apart;
 * image_out: device (B, y_res, 1 + n_samples/hop) uint8. */
int adm_mel_forward(adm_mel_t* h, const void* audio, int is_f64, int B, long slice_stride, int n_samples,
                    uint8_t* image_out, void* stream);
/* the mel power spectrogram before the dB conversion (librosa.feature.melspectrogram, audiodiffusion/mel.py:140-147):
 * melspec_out: device (B, y_res, 1 + n_samples/hop) in the audio's precision (fp32 or fp64). */
int adm_mel_forward_power(adm_mel_t* h, const void* audio, int is_f64, int B, long slice_stride, int n_samples,
                          void* melspec_out, void* stream);
/* images: device (B, y_res, n_frames) uint8; init_phase: device (B, n_bins, n_frames) fp64 in [0,1) (Griffin-Lim start
 * phase / 2 pi); audio_out: device (B, hop*(n_frames-1)) fp32; stft_mag_out: NULL or device (B, n_frames, n_bins) fp64;
 * pg_max_host: NULL or receives max |projected gradient| of the NNLS solution returned (librosa's rule: <= 1e-5). */
int adm_mel_inverse(adm_mel_t* h, const uint8_t* images, const double* init_phase, int B, int n_frames,
                    float* audio_out, double* stft_mag_out, float* pg_max_host, void* stream);
/* librosa.util.nnls behind mel_to_stft (audiodiffusion/mel.py:165): column blocks whose start point fails L-BFGS-B's rule
 * (max |projected gradient| > pgtol = 1e-5) are solved on the device (projected accelerated gradient, step 1/lipschitz,
 * lipschitz = lambda_max(A A^T) of the fp64 filterbank, at most max_iter iterations per column); blocks that satisfy it are
 * returned as they are, as scipy does (nit = 0). Without this call adm_mel_inverse returns the start point everywhere. */
int adm_mel_set_nnls_solver(adm_mel_t* h, double lipschitz, int max_iter);
/* after an adm_mel_inverse with pg_max_host != NULL (which then holds the projected gradient of the RETURNED point):
 * the start point's max |projected gradient| and the largest iteration count any column needed. */
int adm_mel_last_nnls(adm_mel_t* h, float* pg_start, int* iterations);
/* Test aid (adm_version() >= 119; tests assert the forward launcher's rules with it): what the last adm_mel_forward /
 * adm_mel_forward_power on this thread launched, engine * 100 + element size * 10 + waves per SIMD. Engine 1 = radix-2 in LDS, one frame
 * per workgroup of four waves (mel_stft_power_kernel, any n_fft) | 2 = wave per frame, radix 16 (mel_stft2048_kernel, n_fft = 2048 unless
 * ADM_MEL_FAST=0); element size 4 = fp32 audio, 8 = fp64; waves per SIMD 1 or 2 (engine 2: 2 unless ADM_MEL_OCC=1 or the eight-wave LDS
 * image exceeds 160 KiB). E.g. 141 = mel_stft_power_kernel<float>, 282 = mel_stft2048_kernel<double, 2>. 0 before the first launch; a
 * call that returns an error before launching leaves the value as it was. */
int adm_mel_last_variant(void);

#ifdef __cplusplus
}
#endif
#endif /* ADM_H */
