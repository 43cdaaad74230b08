// unet_exec.hip — native UNet2DModel executor + whole-loop sampler behind the C-ABI (include/adm.h).
//
// Replaces `self.unet(images, t)["sample"]` and the Python denoising loop of
// audiodiffusion/pipeline_audio_diffusion.py:159-185. Design (MI355X-first):
//  * the layer graph is built ONCE from the diffusers config into a flat op list (GroupNorm-stats, fused conv,
//    attention core) — ~190 kernel launches per forward instead of ~300 eager ops, no concat / upsample /
//    residual / activation kernels at all (they are folded into the conv load path and epilogue);
//  * weights are uploaded by diffusers state-dict key, then repacked once ([Cin][tap][Cout]; q|k|v stacked;
//    all time_emb_proj matrices stacked) so every hot load is a coalesced float4 row;
//  * activations live in one arena planned by liveness (skip connections stay resident until consumed);
//  * one denoising step {temb, UNet, scheduler epilogue, step++} is captured into a hipGraph and replayed
//    n_steps times; step-dependent scalars (timestep, scheduler coefficients, noise/mask slices) are read on the
//    device from a coefficient table indexed by a device-side step counter, so one graph serves every step.
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "net_exec.h"

namespace adm {
// One step of a loop, described: everything its launches depend on that can differ between two loop calls on the same plan. enqueue_step
// launches from this and sees nothing else of the call, and run_loop replays the stored graph exactly when two of these are the same bytes;
// so what reaches a kernel argument is in the comparison by construction. describe_step fills it, a feature that is off as zeros. Per-plan
// buffers are not here: when one moves, free_plan forgets the stored step. Floats are held as their bits and there is no padding.
struct StepDesc {
  float* x; const float* step_noise; const float* mask; uint8_t* u8_out;   // the caller's tensors
  const float* encoding_uncond;                                             // guided
  const float *known, *known_noise; const uint8_t* keep;                    // in-painting
  // the handle's: the coefficient table and, where the step reads them, the multistep / UniPC / known-region tables and the noise-stream
  // block (a table that is set selects its step: unipc the UniPC step, noise_blk the noise drawn on the device); the encoding
  const adm_sched_coef* coef; const float* khist; const adm_unipc_coef* unipc; const float* known_tab; const uint32_t* noise_blk;
  const float* ctx;
  hipStream_t stream;
  int32_t B, n_steps, mask_start, mask_end, mode, prediction, ctx_S;
  int32_t lo, hi; uint32_t w, max_value;                 // SCHED_THRESH
  uint32_t guidance_scale, guidance_rescale;             // guided
  int32_t window_total_w, window_stride, window_wrap;    // windowed
  int32_t known_batched, keep_batched;                   // in-painting
};
static_assert(std::has_unique_object_representations_v<StepDesc>, "StepDesc is compared as bytes: no padding, no float members");
}  // namespace adm

extern "C" int adm_mse_loss(const float* pred, const float* target, long n, float* loss_out, float* grad_out,
                            double* scratch, void* stream);

using namespace adm;

struct adm_unet {
  adm_unet_config cfg;
  ParamStore ps;
  Net net;
  std::vector<void*> owned;  // device allocations freed on destroy
  bool finalized = false;
  int temb_dim = 0, temb_rows = 0;
  float *freqs = nullptr, *temb_w = nullptr, *temb_b = nullptr;
  // per-batch plan
  int planned_B = 0;
  std::vector<void*> extra;  // per-batch buffers besides the net arena
  PackItem* temb_items = nullptr; int n_temb_items = 0;   // restack_temb's device table
  float *emb = nullptr, *emb_act = nullptr, *temb_all = nullptr, *t_dev = nullptr, *eps_buf = nullptr;
  float* hist_buf = nullptr;     // x0 of the previous step (multistep scheduler loop); same size as eps_buf
  float* scale_buf = nullptr;    // per-sample dynamic threshold of the thresholded loop (B floats)
  float* rescale_buf = nullptr;  // per-sample guidance-rescale factor r_b of the rescaled guided loop (B floats)
  // Per-plan buffers allocated by the first loop that needs them at this batch size (run_loop) and released with the plan's other extras;
  // free_plan resets the struct by value, so a buffer added here cannot be left dangling.
  struct LazyBufs {
    float* eps_uncond = nullptr;   // the unconditional forward's output of a guided loop; same size as eps_buf
    float* unipc = nullptr;        // the UniPC loop's state: the two history slots, then `last` (three times eps_buf's size)
    // the windowed loop (include/adm.h "Windowed sampling"): the gathered windows (the forwards' input) and the blended model outputs of
    // the wide shape (the step's eps / eps_uncond). Each of eps_buf's size — nW*W >= Wt, so a wide tensor fits where the windows do
    float *win = nullptr, *wide_eps = nullptr, *wide_uncond = nullptr;
  } lazy;
  // per-step device tables beside coef_dev, each grown by upload_rows: the multistep history coefficient, the UniPC loop's adm_unipc_coef,
  // the (ka, kb) of the known-region overwrite (include/adm.h "Region in-painting")
  adm_sched_coef* coef_dev = nullptr;
  float* khist_dev = nullptr;
  adm_unipc_coef* unipc_dev = nullptr;
  float* known_dev = nullptr;
  int coef_cap = 0, khist_cap = 0, unipc_cap = 0, known_cap = 0;
  int* step_dev = nullptr;
  // the noise-stream block of adm_sample_loop_philox: {seed_lo, seed_hi, row_offset, stream id}. Allocated once and never moved (its address
  // is part of the captured step's description); rewritten from noise_blk_host by a stream-ordered copy before every run.
  uint32_t* noise_blk_dev = nullptr;
  uint32_t noise_blk_host[4] = {0, 0, 0, 0};
  // training
  bool training = false;
  int warm_B = 0;         // batch size at which an uncaptured forward has already run (see run_loop)
  int bf16_level = 0;     // mixed-precision level of THIS model (option conv_bf16 as it stood at adm_unet_enable_training)
  int op16_f16 = 0;       // ... and the operand format of its 16-bit kernels (option conv_op16_f16: fp16 instead of bf16)
  float loss_scale = 1.f; // fp16 loss scaling (adm_unet_set_loss_scale)
  long params_numel = 0;
  float *dtemb_all = nullptr, *demb = nullptr, *dz = nullptr, *save_sinus = nullptr, *save_z = nullptr;
  double* scratch_d = nullptr;
  adm::StepDesc captured{};   // the step the last use_graph loop captured (all zeros: none; a step has an x); the emulator keeps it too
  int captures = 0;           // adm_unet_loop_captures
#if !defined(ADM_EMU)
  hipStream_t own_stream = nullptr;
  hipGraphExec_t gexec = nullptr;    // `captured` as an executable graph, replayed on captured.stream
#endif
};

namespace adm {

// Enumerates parameters exactly as diffusers' UNet2DModel.__init__ does for this config.
static void declare_all(adm_unet* h) {
  const adm_unet_config& c = h->cfg;
  ParamStore& ps = h->ps;
  const int nb = c.n_blocks, L = c.layers_per_block;
  const int* boc = c.block_out_channels;
  const int temb = boc[0] * 4;
  h->temb_dim = temb;
  ps.declare_conv("conv_in", boc[0], c.in_channels, 3);
  ps.declare_lin("time_embedding.linear_1", temb, boc[0]);
  ps.declare_lin("time_embedding.linear_2", temb, temb);
  int out = boc[0];
  for (int i = 0; i < nb; ++i) {
    const int cin = out;
    out = boc[i];
    const std::string bp = "down_blocks." + std::to_string(i);
    for (int j = 0; j < L; ++j) {
      ps.declare_resnet(bp + ".resnets." + std::to_string(j), j == 0 ? cin : out, out, temb);
      if (c.down_attn[i] == 2) ps.declare_transformer(bp + ".attentions." + std::to_string(j), out, c.cross_attention_dim);
      else if (c.down_attn[i]) ps.declare_attn(bp + ".attentions." + std::to_string(j), out);
    }
    if (i != nb - 1) ps.declare_conv(bp + ".downsamplers.0.conv", out, out, 3);
  }
  const int mid = boc[nb - 1];
  ps.declare_resnet("mid_block.resnets.0", mid, mid, temb);
  if (c.cross_attention_dim > 0) ps.declare_transformer("mid_block.attentions.0", mid, c.cross_attention_dim);
  else ps.declare_attn("mid_block.attentions.0", mid);
  ps.declare_resnet("mid_block.resnets.1", mid, mid, temb);
  out = boc[nb - 1];
  for (int i = 0; i < nb; ++i) {
    const int prev = out;
    out = boc[nb - 1 - i];
    const int cin = boc[nb - 1 - (i + 1 < nb - 1 ? i + 1 : nb - 1)];
    const std::string bp = "up_blocks." + std::to_string(i);
    for (int j = 0; j < L + 1; ++j) {
      const int skip = (j == L) ? cin : out;
      const int rin = (j == 0) ? prev : out;
      ps.declare_resnet(bp + ".resnets." + std::to_string(j), rin + skip, out, temb);
      if (c.up_attn[i] == 2) ps.declare_transformer(bp + ".attentions." + std::to_string(j), out, c.cross_attention_dim);
      else if (c.up_attn[i]) ps.declare_attn(bp + ".attentions." + std::to_string(j), out);
    }
    if (i != nb - 1) ps.declare_conv(bp + ".upsamplers.0.conv", out, out, 3);
  }
  ps.declare_gn("conv_norm_out", boc[0]);
  ps.declare_conv("conv_out", c.out_channels, boc[0], 3);
}

static int dalloc(adm_unet* h, void** p, size_t bytes) {
  ADM_TRY(dmalloc(p, bytes));
  h->owned.push_back(*p);
  return 0;
}

static float* P(adm_unet* h, const std::string& k) { return h->ps.P(k); }

// stacked copy of all time_emb_proj matrices (re-done after every optimizer step in training)
// the 32 time_emb_proj matrices (+ biases) stacked row-wise: ONE batched copy launch over a device table built once (the
// parameter pointers are stable: master parameters never move after finalize) instead of 64 copies per optimizer step
static int restack_temb(adm_unet* h, hipStream_t st) {
  if (h->temb_items == nullptr) {
    std::vector<PackItem> items;
    int off = 0;
    for (auto& r : h->net.temb_rows) {
      items.push_back(PackItem{P(h, r.first + ".weight"), h->temb_w + (size_t)off * h->temb_dim, 0, 0, 0, r.second * h->temb_dim});
      items.push_back(PackItem{P(h, r.first + ".bias"), h->temb_b + off, 0, 0, 0, r.second});
      off += r.second;
    }
    h->n_temb_items = (int)items.size();
    if (items.empty()) return 0;
    ADM_TRY(h->net.dalloc((void**)&h->temb_items, sizeof(PackItem) * items.size()));
    ADM_TRY(copy_h2d(h->temb_items, items.data(), sizeof(PackItem) * items.size(), st));
    ADM_TRY(stream_sync(st));
  }
  return launch_copy_batch(h->temb_items, h->n_temb_items, st);
}

// The conv dispatchers read the process-wide option conv_bf16; a model's own level is put in force only while one of ITS
// training entry points runs (and while its weights are packed), and every inference entry point runs at level 0 — so the
// sampling path stays fp32 even through a training handle, and one model's setting never leaks into another's.
struct Bf16Scope {
  int prev, prev_fmt;
  explicit Bf16Scope(int level, int f16 = 0) : prev(conv_bf16_mode()), prev_fmt(conv_op16_f16() ? 1 : 0) {
    set_conv_bf16(level);
    set_conv_op16_f16(f16);
  }
  ~Bf16Scope() { set_conv_bf16(prev); set_conv_op16_f16(prev_fmt); }
};

// Inference through a training handle: packings refreshed in full first (begin_inference), training's usage masks restored after.
struct InferenceScope {
  Net* n; std::vector<unsigned> saved; int rc;
  InferenceScope(Net* net, hipStream_t st) : n(net) { rc = n->begin_inference(st, &saved); }
  ~InferenceScope() { if (rc == 0) n->end_inference(saved); }
};

static int finalize(adm_unet* h) {
  Bf16Scope pack_scope(h->training ? h->bf16_level : 0, h->training ? h->op16_f16 : 0);
  if (h->finalized) return 0;
  std::string missing;
  const int nmiss = h->ps.missing(&missing);
  ADM_REQUIRE(nmiss == 0, "unet: " + std::to_string(nmiss) + " parameters not set: " + missing);
  const adm_unet_config& c = h->cfg;
  const int nb = c.n_blocks, L = c.layers_per_block;
  const int* boc = c.block_out_channels;
  Net& b = h->net;
  b.ps = &h->ps;
  b.groups = c.norm_num_groups;
  b.eps = c.norm_eps;
  b.training = h->training;
  b.ctx_D = c.cross_attention_dim;      // (adm_unet_set_encoding sets the same; the plan report sizes the to_k / to_v weights with it)
  int rc = 0;
  b.t_in = b.new_tensor(c.in_channels, c.sample_h, c.sample_w, true);
  const ConvW* w;
  ADM_TRY(b.make_conv("conv_in", boc[0], c.in_channels, 3, &w));
  int x = b.conv_op(b.t_in, -1, w, -1, 0, 0, 1, 1, -1, -1);
  std::vector<int> skips{x};
  int out = boc[0];
  const int hd = c.attention_head_dim > 0 ? c.attention_head_dim : 0;
  for (int i = 0; i < nb; ++i) {
    const int cin = out;
    out = boc[i];
    const std::string bp = "down_blocks." + std::to_string(i);
    for (int j = 0; j < L; ++j) {
      x = b.resnet(bp + ".resnets." + std::to_string(j), x, -1, j == 0 ? cin : out, out, true, &rc);
      ADM_TRY(rc);
      if (c.down_attn[i] == 2) { x = b.transformer(bp + ".attentions." + std::to_string(j), x, out, hd, c.cross_attention_dim, &rc); ADM_TRY(rc); }
      else if (c.down_attn[i]) { x = b.attention(bp + ".attentions." + std::to_string(j), x, out, hd ? hd : out, &rc); ADM_TRY(rc); }
      skips.push_back(x);
    }
    if (i != nb - 1) {
      ADM_TRY(b.make_conv(bp + ".downsamplers.0.conv", out, out, 3, &w));
      x = b.conv_op(x, -1, w, -1, 0, 0, 2, 1, -1, -1);
      skips.push_back(x);
    }
  }
  const int mid = boc[nb - 1];
  x = b.resnet("mid_block.resnets.0", x, -1, mid, mid, true, &rc); ADM_TRY(rc);
  if (c.cross_attention_dim > 0) x = b.transformer("mid_block.attentions.0", x, mid, hd, c.cross_attention_dim, &rc);
  else x = b.attention("mid_block.attentions.0", x, mid, hd ? hd : mid, &rc);
  ADM_TRY(rc);
  x = b.resnet("mid_block.resnets.1", x, -1, mid, mid, true, &rc); ADM_TRY(rc);
  out = boc[nb - 1];
  for (int i = 0; i < nb; ++i) {
    const int prev = out;
    out = boc[nb - 1 - i];
    const int cin = boc[nb - 1 - (i + 1 < nb - 1 ? i + 1 : nb - 1)];
    const std::string bp = "up_blocks." + std::to_string(i);
    for (int j = 0; j < L + 1; ++j) {
      const int skip = (j == L) ? cin : out;
      const int rin = (j == 0) ? prev : out;
      const int s = skips.back();
      skips.pop_back();
      ADM_REQUIRE(b.tensors[s].C == skip, "unet: skip channel mismatch at " + bp);
      x = b.resnet(bp + ".resnets." + std::to_string(j), x, s, rin + skip, out, true, &rc);
      ADM_TRY(rc);
      if (c.up_attn[i] == 2) { x = b.transformer(bp + ".attentions." + std::to_string(j), x, out, hd, c.cross_attention_dim, &rc); ADM_TRY(rc); }
      else if (c.up_attn[i]) { x = b.attention(bp + ".attentions." + std::to_string(j), x, out, hd ? hd : out, &rc); ADM_TRY(rc); }
    }
    if (i != nb - 1) {
      ADM_TRY(b.make_conv(bp + ".upsamplers.0.conv", out, out, 3, &w));
      x = b.conv_op(x, -1, w, -1, 0, 1, 1, 1, -1, -1);
    }
  }
  const int g = b.gn_op(x, -1, b.make_gn("conv_norm_out", boc[0]));
  ADM_TRY(b.make_conv("conv_out", c.out_channels, boc[0], 3, &w));
  b.t_out = b.new_tensor(c.out_channels, c.sample_h, c.sample_w, true);
  b.conv_op(x, -1, w, g, 1, 0, 1, 1, -1, -1, b.t_out);
  // stacked time_emb_proj
  int R = 0;
  for (auto& r : b.temb_rows) R += r.second;
  h->temb_rows = R;
  ADM_TRY(dalloc(h, (void**)&h->temb_w, sizeof(float) * (size_t)R * h->temb_dim));
  ADM_TRY(dalloc(h, (void**)&h->temb_b, sizeof(float) * (size_t)R));
  ADM_TRY(restack_temb(h, nullptr));
  // sinusoid frequencies: exp(-ln(10000) * i / (half - freq_shift)) in fp32, as diffusers computes them
  const int half = boc[0] / 2;
  std::vector<float> fr(half);
  for (int i = 0; i < half; ++i) {
    float e = -logf(10000.0f) * (float)i;
    e = e / ((float)half - c.freq_shift);
    fr[i] = expf(e);
  }
  ADM_TRY(dalloc(h, (void**)&h->freqs, sizeof(float) * half));
  ADM_TRY(copy_h2d(h->freqs, fr.data(), sizeof(float) * half, nullptr));
  ADM_TRY(stream_sync(nullptr));
  b.finish_liveness();
  h->finalized = true;
  return 0;
}

static void free_plan(adm_unet* h) {
  h->net.free_plan();
  for (void* p : h->extra) dfree(p);
  h->extra.clear();
  h->planned_B = 0;
  h->lazy = {};
  h->warm_B = 0;       // the next capture is preceded by an uncaptured forward again (another kernel's one-time set-up)
#if !defined(ADM_EMU)
  if (h->gexec) {                     // (a replay may still be in flight: drain the stream it ran on before the executable graph goes)
    (void)stream_sync(h->captured.stream);
    (void)hipGraphExecDestroy(h->gexec);
    h->gexec = nullptr;
  }
#endif
  h->captured = {};
}

static int extra_alloc(adm_unet* h, void** p, size_t bytes) {
  ADM_TRY(dmalloc(p, bytes));
  h->extra.push_back(*p);
  return 0;
}

// A member of adm_unet::LazyBufs: allocated with the plan by the first loop that needs it.
static int ensure(adm_unet* h, float** p, size_t elems) { return *p ? 0 : extra_alloc(h, (void**)p, sizeof(float) * elems); }

static int plan(adm_unet* h, int B) {
  // (re-planned as well when adm_set_option has moved since: a layer may have changed kernel, and the partial-sum buffers of the
  //  GroupNorm statistics follow the kernels — free_plan also drops the captured graph, which holds the old kernels)
  if (h->planned_B == B && h->net.plan_current(B)) return 0;
  free_plan(h);
  ADM_TRY(h->net.plan(B));
  ADM_TRY(extra_alloc(h, (void**)&h->emb, sizeof(float) * (size_t)B * h->temb_dim));
  ADM_TRY(extra_alloc(h, (void**)&h->emb_act, sizeof(float) * (size_t)B * h->temb_dim));
  ADM_TRY(extra_alloc(h, (void**)&h->temb_all, sizeof(float) * (size_t)B * h->temb_rows));
  ADM_TRY(extra_alloc(h, (void**)&h->t_dev, sizeof(float) * (size_t)B));
  ADM_TRY(extra_alloc(h, (void**)&h->eps_buf,
                      sizeof(float) * (size_t)B * h->cfg.out_channels * h->cfg.sample_h * h->cfg.sample_w));
  ADM_TRY(extra_alloc(h, (void**)&h->hist_buf,
                      sizeof(float) * (size_t)B * h->cfg.out_channels * h->cfg.sample_h * h->cfg.sample_w));
  ADM_TRY(extra_alloc(h, (void**)&h->scale_buf, sizeof(float) * (size_t)B));
  ADM_TRY(extra_alloc(h, (void**)&h->rescale_buf, sizeof(float) * (size_t)B));
  ADM_TRY(extra_alloc(h, (void**)&h->step_dev, sizeof(int)));
  if (h->training) {
    ADM_TRY(extra_alloc(h, (void**)&h->dtemb_all, sizeof(float) * (size_t)B * h->temb_rows));
    ADM_TRY(extra_alloc(h, (void**)&h->demb, sizeof(float) * (size_t)B * h->temb_dim));
    ADM_TRY(extra_alloc(h, (void**)&h->dz, sizeof(float) * (size_t)B * h->temb_dim));
    ADM_TRY(extra_alloc(h, (void**)&h->save_sinus, sizeof(float) * (size_t)B * h->cfg.block_out_channels[0]));
    ADM_TRY(extra_alloc(h, (void**)&h->save_z, sizeof(float) * (size_t)B * h->temb_dim));
    ADM_TRY(extra_alloc(h, (void**)&h->scratch_d, sizeof(double)));
  }
  h->planned_B = B;
  return 0;
}

// Enqueue one UNet forward. Timestep source: t_dev (B floats) when table == nullptr, else table[*step_dev].
static int run_forward(adm_unet* h, const float* x, float* out, int B, const adm_sched_coef* table, hipStream_t st,
                       OpTimer* tm = nullptr) {
  const adm_unet_config& c = h->cfg;
  const int dim_in = c.block_out_channels[0];
  ADM_TRY(launch_time_embedding(table ? nullptr : h->t_dev, 1, table, h->step_dev, h->freqs, dim_in / 2,
                                c.flip_sin_to_cos, P(h, "time_embedding.linear_1.weight"),
                                P(h, "time_embedding.linear_1.bias"), P(h, "time_embedding.linear_2.weight"),
                                P(h, "time_embedding.linear_2.bias"), dim_in, h->temb_dim, h->emb, B, st,
                                h->training ? h->save_sinus : nullptr, h->training ? h->save_z : nullptr, h->emb_act));
  if (tm) { tm->st = st; tm->begin(); }
  ADM_TRY(launch_temb_proj(h->emb_act, h->temb_w, h->temb_b, h->temb_all, B, h->temb_dim, h->temb_rows, st, 1));
  if (tm) tm->end(4, 0, 2.0 * B * h->temb_dim * h->temb_rows, 4.0 * h->temb_dim * h->temb_rows);
  return h->net.run(x, out, B, h->temb_all, h->temb_rows, st, tm);
}

// One of the handle's per-step device tables: grown to n rows when it is smaller (it then moves, and a captured step that read it is
// captured again), then filled from the host rows in stream order.
template <class T>
static int upload_rows(adm_unet* h, T** dev, int* cap, const T* host, size_t row_bytes, int n, hipStream_t st) {
  if (*cap < n) {
    ADM_TRY(dalloc(h, (void**)dev, row_bytes * (size_t)n));
    *cap = n;
  }
  return copy_h2d(*dev, host, row_bytes * (size_t)n, st);
}

// adm_sample_loop_args::mode inside this file: the SCHED_* mode of the step that follows the forward, or the DDIM inversion step
// (adm_encode_loop_ex sets it; adm_sample_loop_ex refuses it)
enum { LOOP_ENCODE = -1 };
using LoopArgs = adm_sample_loop_args;
// LoopArgs::encoding_uncond and guidance_scale: classifier-free guidance (the unconditional encoding, device, of the shape of the handle's).
// LoopArgs::seed and row_offset (noise_source 1, "adm noise stream 1": the seed and the global row of x[0]) reach the kernel through the
// handle's device block, never as kernel arguments: neither is in the StepDesc.

// The noise-stream block, written in stream order before the first step and outside the captured step.
static int ensure_noise_block(adm_unet* h, const LoopArgs& a, hipStream_t st) {
  if (h->noise_blk_dev == nullptr) ADM_TRY(dalloc(h, (void**)&h->noise_blk_dev, sizeof(h->noise_blk_host)));
  h->noise_blk_host[0] = (uint32_t)(a.seed & 0xffffffffull); h->noise_blk_host[1] = (uint32_t)(a.seed >> 32);
  h->noise_blk_host[2] = (uint32_t)a.row_offset; h->noise_blk_host[3] = 0;   // stream 0: step noise
  return copy_h2d(h->noise_blk_dev, h->noise_blk_host, sizeof(h->noise_blk_host), st);
}

// The windowed loop (LoopArgs::window_total_w != 0; include/adm.h "Windowed sampling"): windows per wide sample. adm_sample_loop_ex has
// checked the placement, so the count is the definition's quotient.
template <class A>   // LoopArgs (before there is a plan) or StepDesc
static int loop_windows(const adm_unet* h, const A& a) {
  if (a.window_total_w == 0) return 1;
  return a.window_wrap ? a.window_total_w / a.window_stride : (a.window_total_w - h->cfg.sample_w) / a.window_stride + 1;
}

static uint32_t f32_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static float bits_f32(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

// The step of loop `a` run on stream `run`, after plan(), the lazy buffers and the table uploads (any of which may move what this reads
// from the handle). Normalised: the fields of a feature that is off stay zero, whatever the caller left in them, because the launchers do
// not read them then (launch_sched_threshold is reached in SCHED_THRESH only; guidance and the rescale need eps_uncond; the window fields
// are read under window_total_w != 0 and the known-region fields under keep != NULL; k_hist_table is read by the multistep kernels only).
static StepDesc describe_step(const adm_unet* h, const LoopArgs& a, hipStream_t run) {
  StepDesc d{};
  d.x = a.x; d.step_noise = a.step_noise; d.mask = a.mask; d.u8_out = a.u8_out;
  d.B = a.B; d.n_steps = a.n_steps; d.mask_start = a.mask_start; d.mask_end = a.mask_end; d.mode = a.mode; d.prediction = a.prediction;
  d.coef = h->coef_dev; d.ctx = h->net.ctx; d.ctx_S = h->net.ctx_S; d.stream = run;
  if (a.mode == SCHED_THRESH) { d.lo = a.lo; d.hi = a.hi; d.w = f32_bits(a.w); d.max_value = f32_bits(a.max_value); }
  if (a.mode == SCHED_MULTISTEP) d.khist = h->khist_dev;
  if (a.unipc_host != nullptr) d.unipc = h->unipc_dev;
  if (a.noise_source == 1) d.noise_blk = h->noise_blk_dev;
  if (a.encoding_uncond != nullptr) {
    d.encoding_uncond = a.encoding_uncond; d.guidance_scale = f32_bits(a.guidance_scale); d.guidance_rescale = f32_bits(a.guidance_rescale);
  }
  if (a.window_total_w != 0) { d.window_total_w = a.window_total_w; d.window_stride = a.window_stride; d.window_wrap = a.window_wrap; }
  if (a.keep != nullptr) {
    d.known = a.known; d.known_noise = a.known_noise; d.keep = a.keep; d.known_tab = h->known_dev;
    d.known_batched = a.known_batched != 0; d.keep_batched = a.keep_batched != 0;
  }
  return d;
}

static int gather_windows(adm_unet* h, const StepDesc& d) {
  const adm_unet_config& c = h->cfg;
  return launch_window_gather(d.x, h->lazy.win, d.B, c.in_channels, c.sample_h, d.window_total_w, c.sample_w, d.window_stride,
                              d.window_wrap, d.stream);
}

// One denoising step on d.stream; every step-dependent scalar is read on the device through *step_dev.
static int enqueue_step(adm_unet* h, const StepDesc& d, int step) {
  const adm_unet_config& c = h->cfg;
  const hipStream_t st = d.stream;
  const bool guided = d.encoding_uncond != nullptr;
  // windowed: gather, the forward(s) on the windows as ONE batch of B*nW, one blend per model output, then the step on the wide tensors
  const bool windowed = d.window_total_w != 0;
  const int FB = d.B * loop_windows(h, d);                      // the forwards' batch
  const int Wx = windowed ? d.window_total_w : c.sample_w;      // the width of x, and of everything the step touches
  const float* fx = d.x;
  if (windowed) {
    ADM_TRY(gather_windows(h, d));
    fx = h->lazy.win;
  }
  ADM_TRY(run_forward(h, fx, h->eps_buf, FB, d.coef, st));
  if (guided) {
    // The unconditional branch: a second forward of batch B on the SAME plan (its side-stream hoists included), with the encoding pointer
    // swapped. Nothing derived from the encoding outlives a forward (the cross-attention kernel projects K and V from net.ctx inside every
    // launch), so the swap is all it takes; both forwards run in stream order, the second after the first has joined its side launches.
    const float* ctx_cond = h->net.ctx;
    h->net.ctx = d.encoding_uncond;
    const int rc = run_forward(h, fx, h->lazy.eps_uncond, FB, d.coef, st);
    h->net.ctx = ctx_cond;
    ADM_TRY(rc);
  }
  const float *eps = h->eps_buf, *eps_uncond = h->lazy.eps_uncond;
  if (windowed) {
    ADM_TRY(launch_window_blend(eps, h->lazy.wide_eps, d.B, c.out_channels, c.sample_h, Wx, c.sample_w, d.window_stride, d.window_wrap, st));
    eps = h->lazy.wide_eps;
    if (guided) {
      ADM_TRY(launch_window_blend(eps_uncond, h->lazy.wide_uncond, d.B, c.out_channels, c.sample_h, Wx, c.sample_w, d.window_stride,
                                  d.window_wrap, st));
      eps_uncond = h->lazy.wide_uncond;
    }
  }
  const long n = (long)d.B * c.in_channels * c.sample_h * Wx;
  if (d.mode == LOOP_ENCODE) {
    ADM_TRY(launch_encode_step(d.x, eps, d.coef, h->step_dev, step, d.prediction, n, st));
  } else {
    SchedStepParams p{d.x, eps, d.step_noise, d.x, d.u8_out, d.coef, h->step_dev, step, d.mask, d.n_steps, d.mask_start,
                      d.mask_end, d.B, c.in_channels, c.sample_h, Wx};
    p.noise_step_stride = n; p.u8_step = d.n_steps - 1;
    p.scale = h->scale_buf; p.hist = h->hist_buf; p.k_hist_table = d.khist;
    if (d.mode == SCHED_THRESH) { p.lo = d.lo; p.hi = d.hi; p.w = bits_f32(d.w); p.max_value = bits_f32(d.max_value); }
    if (guided) {
      p.eps_uncond = eps_uncond; p.guidance = bits_f32(d.guidance_scale);
      p.guidance_rescale = bits_f32(d.guidance_rescale); p.rescale = h->rescale_buf;   // (0: off, the buffer is not touched)
    }
    if (d.noise_blk != nullptr) { p.philox = 1; p.nblock = d.noise_blk; }
    if (d.keep != nullptr) {   // the known-region overwrite: three caller tensors of x's shape (wide when windowed) and the handle's table
      p.known = d.known; p.known_noise = d.known_noise; p.keep = d.keep; p.known_table = d.known_tab;
      p.known_batched = d.known_batched; p.keep_batched = d.keep_batched;
    }
    if (d.unipc != nullptr) {   // the UniPC step: two history slots, then last, in the handle's one buffer
      p.unipc_table = d.unipc; p.hist = h->lazy.unipc; p.last = h->lazy.unipc + 2 * n;
      ADM_TRY(launch_unipc_step(p, d.mode, st, d.prediction));
    } else {
      ADM_TRY(launch_sched_step(p, d.mode, st, d.prediction));
    }
  }
  ADM_TRY(launch_step_advance(h->step_dev, st));
  return 0;
}

static int run_loop(adm_unet* h, const LoopArgs& a, hipStream_t st) {
  ADM_REQUIRE(h->cfg.in_channels == h->cfg.out_channels, "sample_loop: in/out channels differ");
  // the plan's batch: the forwards' (B*nW windows with window_total_w != 0). Every per-plan buffer below is sized by it, and the wide
  // sample's state (history, UniPC state, per-sample factors) lives in the same buffers: nW*W >= Wt and PB >= B
  const int PB = a.B * loop_windows(h, a);
  const size_t plan_elems = (size_t)PB * h->cfg.out_channels * h->cfg.sample_h * h->cfg.sample_w;
  const bool guided = a.encoding_uncond != nullptr, windowed = a.window_total_w != 0;
  if (windowed)
    ADM_REQUIRE((size_t)a.B * h->cfg.out_channels * h->cfg.sample_h * a.window_total_w <= plan_elems,
                "sample_loop: the wide sample does not fit the buffers of the windows' plan (window_total_w > nW * sample_w)");
  ADM_TRY(plan(h, PB));
  if (guided) ADM_TRY(ensure(h, &h->lazy.eps_uncond, plan_elems));
  if (a.unipc_host != nullptr) ADM_TRY(ensure(h, &h->lazy.unipc, 3 * plan_elems));
  if (windowed) {
    ADM_TRY(ensure(h, &h->lazy.win, plan_elems));
    ADM_TRY(ensure(h, &h->lazy.wide_eps, plan_elems));
  }
  if (windowed && guided) ADM_TRY(ensure(h, &h->lazy.wide_uncond, plan_elems));
  hipStream_t run = st;
#if !defined(ADM_EMU)
  hipEvent_t ev = nullptr;
  if (a.use_graph && st == nullptr) {  // the legacy default stream cannot be captured: hop onto an owned stream
    if (!h->own_stream) ADM_HIP_OK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    run = h->own_stream;
    ADM_HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ADM_HIP_OK(hipEventRecord(ev, st));
    ADM_HIP_OK(hipStreamWaitEvent(run, ev, 0));
  }
#endif
  ADM_TRY(upload_rows(h, &h->coef_dev, &h->coef_cap, a.coef_host, sizeof(adm_sched_coef), a.n_steps, run));
  ADM_TRY(dmemset(h->step_dev, 0, sizeof(int), run));
  if (a.mode == SCHED_MULTISTEP) ADM_TRY(upload_rows(h, &h->khist_dev, &h->khist_cap, a.k_hist_host, sizeof(float), a.n_steps, run));
  if (a.unipc_host != nullptr) ADM_TRY(upload_rows(h, &h->unipc_dev, &h->unipc_cap, a.unipc_host, sizeof(adm_unipc_coef), a.n_steps, run));
  if (a.noise_source == 1) ADM_TRY(ensure_noise_block(h, a, run));
  if (a.keep != nullptr) ADM_TRY(upload_rows(h, &h->known_dev, &h->known_cap, a.known_coef_host, 2 * sizeof(float), a.n_steps, run));
  const StepDesc d = describe_step(h, a, run);
  if (a.use_graph && memcmp(&d, &h->captured, sizeof d) != 0) {   // nothing captured yet (all zeros), or another step: capture this one
#if !defined(ADM_EMU)
    if (h->gexec) {
      // the previous loop's replays may still be running (a caller that samples again without a host synchronisation in between — 50
      // single-step calls in tests/test_pipeline.py): destroying an executable graph under its own replays made that test die with SIGSEGV
      // inside this call — 4 of 11 runs of test_full_size.py + test_pipeline.py without the drain, 0 of 12 with it.
      // Re-capture is the rare path; a drain costs nothing there.
      static const int drain = [] { const char* e = getenv("ADM_GRAPH_DRAIN"); return e ? atoi(e) : 1; }();   // (0: tools/graph_churn_probe.py's A/B)
      if (drain) (void)stream_sync(h->captured.stream);
      (void)hipGraphExecDestroy(h->gexec);
      h->gexec = nullptr;
      h->captured = {};   // (no graph, no stored step: a failure below leaves the handle with neither)
    }
    if (h->warm_B != PB) {
      // One UNCAPTURED forward (into eps_buf; the sample is not touched) before the first capture at this batch size:
      // the launchers' one-time work — constant buffers (hipMalloc + null-stream copy), hipFuncSetAttribute for the
      // >64 KiB LDS kernels, device-attribute queries — is not legal inside a stream capture.
      // Windowed: x holds B wide samples, fewer elements than the PB windows the forward reads: it reads the gathered windows.
      if (windowed) ADM_TRY(gather_windows(h, d));
      ADM_TRY(run_forward(h, windowed ? h->lazy.win : d.x, h->eps_buf, PB, d.coef, run));
      h->warm_B = PB;
    }
    hipGraph_t graph = nullptr;
    ADM_HIP_OK(hipStreamBeginCapture(run, hipStreamCaptureModeThreadLocal));
    int rc = enqueue_step(h, d, 0);
    hipError_t e = hipStreamEndCapture(run, &graph);
    if (rc != 0) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    ADM_HIP_OK(e);
    ADM_HIP_OK(hipGraphInstantiate(&h->gexec, graph, nullptr, nullptr, 0));
    ADM_HIP_OK(hipGraphDestroy(graph));
#endif
    h->captured = d;   // (the emulator has no graphs: it remembers and counts the step at the same point, and runs its steps eagerly)
    ++h->captures;
  }
#if !defined(ADM_EMU)
  if (a.use_graph) {
    for (int s = 0; s < a.n_steps; ++s) ADM_HIP_OK(hipGraphLaunch(h->gexec, run));
  } else
#endif
  {
    for (int s = 0; s < a.n_steps; ++s) ADM_TRY(enqueue_step(h, d, s));
  }
#if !defined(ADM_EMU)
  if (ev) {
    ADM_HIP_OK(hipEventRecord(ev, run));
    ADM_HIP_OK(hipStreamWaitEvent(st, ev, 0));
    ADM_HIP_OK(hipEventDestroy(ev));
  }
#endif
  return 0;
}

// What every loop entry point does after its own argument checks.
static int run_loop_fp32(adm_unet* h, const LoopArgs& a, void* stream) {
  Bf16Scope fp32(0);
  ADM_TRY(finalize(h));
  InferenceScope inf(&h->net, (hipStream_t)stream);
  ADM_TRY(inf.rc);
  return run_loop(h, a, (hipStream_t)stream);
}

}  // namespace adm

extern "C" {

int adm_unet_create(const adm_unet_config* cfg, adm_unet_t** out) {
  ADM_REQUIRE(cfg && out, "unet_create: null argument");
  ADM_REQUIRE(cfg->n_blocks >= 1 && cfg->n_blocks <= 8, "unet_create: n_blocks out of range");
  ADM_REQUIRE(cfg->norm_num_groups > 0 && cfg->layers_per_block >= 1, "unet_create: bad config");
  ADM_REQUIRE(cfg->cross_attention_dim >= 0, "unet_create: cross_attention_dim < 0");
  for (int i = 0; i < cfg->n_blocks; ++i)
    ADM_REQUIRE((cfg->down_attn[i] != 2 && cfg->up_attn[i] != 2) || cfg->cross_attention_dim > 0,
                "unet_create: CrossAttn blocks need cross_attention_dim > 0");
  if (cfg->cross_attention_dim > 0) {
    ADM_REQUIRE(cfg->attention_head_dim > 0, "unet_create: conditional model needs attention_head_dim (= number of heads)");
    for (int i = 0; i < cfg->n_blocks; ++i)
      ADM_REQUIRE(cfg->block_out_channels[i] % cfg->attention_head_dim == 0, "unet_create: channels not divisible by the head count");
  }
  for (int i = 0; i < cfg->n_blocks; ++i)
    ADM_REQUIRE(cfg->block_out_channels[i] % cfg->norm_num_groups == 0 && cfg->block_out_channels[i] % 32 == 0,
                "unet_create: block_out_channels must be multiples of 32 and of norm_num_groups");
  adm_unet* h = new adm_unet();
  h->cfg = *cfg;
  declare_all(h);
  *out = h;
  return 0;
}

void adm_unet_destroy(adm_unet_t* h) {
  if (!h) return;
  free_plan(h);
  h->net.destroy();
  h->ps.free_all();
  for (void* p : h->owned) dfree(p);
#if !defined(ADM_EMU)
  if (h->own_stream) { conv_ksplit_release(h->own_stream); (void)hipStreamDestroy(h->own_stream); }
#endif
  delete h;
}

int adm_unet_set_option(adm_unet_t* h, const char* name, int value) {
  ADM_REQUIRE(h && name, "unet_set_option: null argument");
  const std::string nm(name);
  ADM_REQUIRE(nm == "wino6" || nm == "single_sample", "unet_set_option: the per-model options are: wino6, single_sample");
  if (nm == "single_sample") {
    ADM_REQUIRE(value >= -1 && value <= 1, "unet_set_option: single_sample takes 0 (follow the process-wide option), 1 (on) or -1 (off)");
    if (h->net.single_sample != value) {
      h->net.single_sample = value;
      free_plan(h);
    }
    return 0;
  }
  ADM_REQUIRE(value == 0 || value == 1 || value == 2 || (value >= 16 && value <= 65536),
              "unet_set_option: wino6 takes 0 (follow the process-wide option), 1 (default layer rule), 2 (every layer the kernel tiles) or a plane-size floor n >= 16");
  if (h->net.wino6_rule != value) {
    h->net.wino6_rule = value;
    free_plan(h);                     // the statistic-tile counts and a captured loop follow the kernels: plan again on the next call
  }
  return 0;
}

int adm_unet_set_param(adm_unet_t* h, const char* key, const float* host_data, size_t numel) {
  ADM_REQUIRE(h && key && host_data, "unet_set_param: null argument");
  ADM_REQUIRE(!h->finalized, "unet_set_param: model already finalized (first forward ran)");
  return h->ps.set(key, host_data, numel);
}

int adm_unet_missing_params(adm_unet_t* h) {
  std::string names;
  const int n = h->ps.missing(&names);
  if (n) set_error("missing: " + names);
  return n;
}

int adm_unet_forward(adm_unet_t* h, const float* x, const float* timesteps_host, int n_timesteps, float* out, int B,
                     void* stream) {
  ADM_REQUIRE(h && x && out && timesteps_host, "unet_forward: null argument");
  ADM_REQUIRE(n_timesteps == 1 || n_timesteps == B, "unet_forward: need 1 or B timesteps");
  hipStream_t st = (hipStream_t)stream;
  ADM_TRY(finalize(h));
  ADM_TRY(plan(h, B));
  std::vector<float> t(B);
  for (int i = 0; i < B; ++i) t[i] = timesteps_host[n_timesteps == 1 ? 0 : i];
  ADM_TRY(copy_h2d(h->t_dev, t.data(), sizeof(float) * B, st));
  ADM_TRY(stream_sync(st));  // t is a stack/vector buffer: make the copy complete before returning
  Bf16Scope fp32(0);
  InferenceScope inf(&h->net, st);
  ADM_TRY(inf.rc);
  return run_forward(h, x, out, B, nullptr, st);
}

int adm_unet_set_encoding(adm_unet_t* h, const float* encoding_dev, int seq_len) {
  ADM_REQUIRE(h, "unet_set_encoding: null handle");
  ADM_REQUIRE(h->cfg.cross_attention_dim > 0, "unet_set_encoding: this model has no cross-attention (UNet2DModel)");
  ADM_REQUIRE((encoding_dev != nullptr) == (seq_len > 0), "unet_set_encoding: pointer and seq_len must both be given (or both cleared)");
  h->net.ctx = encoding_dev; h->net.ctx_S = seq_len; h->net.ctx_D = h->cfg.cross_attention_dim;
  return 0;
}

int adm_unet_bind_param(adm_unet_t* h, const char* key, float* dev_ptr) {
  ADM_REQUIRE(h && key && dev_ptr, "unet_bind_param: null argument");
  ADM_REQUIRE(!h->finalized, "unet_bind_param: model already finalized");
  return h->ps.bind(key, dev_ptr);
}

int adm_unet_enable_training(adm_unet_t* h, const float* params_base, long numel) {
  ADM_REQUIRE(h && params_base && numel > 0, "unet_enable_training: bad argument");
  ADM_REQUIRE(!h->finalized, "unet_enable_training: must be called before the first forward");
  for (auto& kv : h->ps.params)
    ADM_REQUIRE(kv.second.set && kv.second.dev >= params_base && kv.second.dev + kv.second.numel <= params_base + numel,
                "unet_enable_training: parameter " + kv.first + " is not bound inside the flat buffer");
  h->training = true;
  h->bf16_level = conv_bf16_mode();
  h->op16_f16 = conv_op16_f16() ? 1 : 0;
  h->params_numel = numel;
  h->net.params_base = params_base;
  return 0;
}

int adm_unet_set_loss_scale(adm_unet_t* h, float scale) {
  ADM_REQUIRE(h && scale > 0.f, "unet_set_loss_scale: bad argument");
  h->loss_scale = scale;
  return 0;
}

int adm_unet_refresh_weights(adm_unet_t* h, void* stream) {
  ADM_REQUIRE(h && h->finalized, "unet_refresh_weights: model not finalized");
  Bf16Scope own(h->bf16_level, h->op16_f16);
  ADM_TRY(h->net.refresh_weights((hipStream_t)stream));
  return restack_temb(h, (hipStream_t)stream);
}

// One training forward + backward (scripts/train_unet.py:257-259 without the optimizer): loss_dev[0] = mse(unet(x, t),
// target); grads_base (flat, same offsets as the parameter buffer) receives d loss / d parameters.
int adm_unet_forward_backward(adm_unet_t* h, const float* x, const float* timesteps_host, int n_timesteps,
                              const float* target, float* loss_dev, float* grads_base, int B, void* stream) {
  ADM_REQUIRE(h && x && timesteps_host && target && loss_dev && grads_base, "unet_forward_backward: null argument");
  ADM_REQUIRE(h->training, "unet_forward_backward: call adm_unet_enable_training first");
  ADM_REQUIRE(n_timesteps == 1 || n_timesteps == B, "unet_forward_backward: need 1 or B timesteps");
  hipStream_t st = (hipStream_t)stream;
  Bf16Scope own(h->bf16_level, h->op16_f16);
  ADM_TRY(finalize(h));
  // `drop_last=False` (train_unet.py:181): the partial last batch of an epoch runs INSIDE the full batch's plan (every buffer
  // is sized per sample and the split-K workspace shrinks with B) instead of re-planning twice per epoch
  if (!(h->planned_B > 0 && B <= h->planned_B)) ADM_TRY(plan(h, B));
  ADM_TRY(h->net.begin_training_batch(B, st));
  std::vector<float> t(B);
  for (int i = 0; i < B; ++i) t[i] = timesteps_host[n_timesteps == 1 ? 0 : i];
  ADM_TRY(copy_h2d(h->t_dev, t.data(), sizeof(float) * B, st));
  ADM_TRY(stream_sync(st));
  ADM_TRY(run_forward(h, x, h->eps_buf, B, nullptr, st));
  Net& net = h->net;
  const adm_unet_config& c = h->cfg;
  const long n_out = (long)B * c.out_channels * c.sample_h * c.sample_w;
  ADM_TRY(adm_mse_loss(h->eps_buf, target, n_out, loss_dev, net.tensors[net.t_out].grad, h->scratch_d, st));
  if (h->loss_scale != 1.f)   // fp16 loss scaling: every gradient of the reverse pass carries the factor
    ADM_TRY(adm_flat_op(net.tensors[net.t_out].grad, net.tensors[net.t_out].grad, n_out, 1, h->loss_scale, st));
  net.grads_base = grads_base;
  net.bucket_reset();
  ADM_TRY(dmemset(grads_base, 0, sizeof(float) * (size_t)h->params_numel, st));
  ADM_TRY(net.run_backward(B, h->dtemb_all, h->temb_rows, st));
  // ---- time-embedding path: time_emb_proj (per resnet), then the 2-layer MLP ---------------------------------
  const int K = h->temb_dim, R = h->temb_rows, dim_in = c.block_out_channels[0];
  int off = 0;
  for (auto& r : net.temb_rows) {
    ADM_TRY(launch_linear_bwd(h->dtemb_all + off, R, h->emb, nullptr, B, r.second, K, 1,
                              net.grad_of(P(h, r.first + ".weight")), net.grad_of(P(h, r.first + ".bias")), nullptr, st));
    net.mark_ready(P(h, r.first + ".weight"), (size_t)r.second * K);
    net.mark_ready(P(h, r.first + ".bias"), (size_t)r.second);
    off += r.second;
  }
  ADM_TRY(launch_linear_bwd(h->dtemb_all, R, h->emb, h->temb_w, B, R, K, 1, nullptr, nullptr, h->demb, st));
  ADM_TRY(launch_linear_bwd(h->demb, K, h->save_z, P(h, "time_embedding.linear_2.weight"), B, K, K, 1,
                            net.grad_of(P(h, "time_embedding.linear_2.weight")),
                            net.grad_of(P(h, "time_embedding.linear_2.bias")), h->dz, st));
  ADM_TRY(launch_linear_bwd(h->dz, K, h->save_sinus, nullptr, B, K, dim_in, 0,
                            net.grad_of(P(h, "time_embedding.linear_1.weight")),
                            net.grad_of(P(h, "time_embedding.linear_1.bias")), nullptr, st));
  net.mark_ready(P(h, "time_embedding.linear_2.weight"), (size_t)K * K);
  net.mark_ready(P(h, "time_embedding.linear_2.bias"), (size_t)K);
  net.mark_ready(P(h, "time_embedding.linear_1.weight"), (size_t)K * dim_in);
  net.mark_ready(P(h, "time_embedding.linear_1.bias"), (size_t)K);
  return 0;
}

// Data-parallel overlap (scripts/train_unet.py:259: DDP all-reduces gradient buckets while autograd is still running):
// fn(user, b) fires on the calling thread, during adm_unet_forward_backward, right after the last kernel writing into
// bucket b = [bounds[b], bounds[b+1]) of the flat gradient buffer has been enqueued. n_buckets = 0 removes the hook.
int adm_unet_set_grad_bucket_hook(adm_unet_t* h, int n_buckets, const long* bounds, adm_bucket_fn fn, void* user) {
  ADM_REQUIRE(h, "unet_set_grad_bucket_hook: null handle");
  ADM_REQUIRE(n_buckets == 0 || h->training, "unet_set_grad_bucket_hook: call adm_unet_enable_training first");
  if (n_buckets > 0) ADM_TRY(finalize(h));   // the op list (and its parameter table) must exist to count a bucket's writers
  return h->net.set_bucket_hook(n_buckets, bounds, fn, user);
}

size_t adm_unet_workspace_bytes(adm_unet_t* h) { return h ? h->net.arena_bytes : 0; }

int adm_unet_profile(adm_unet_t* h, const float* x, float timestep, float* out, int B, adm_op_profile* recs, int cap,
                     int* n_out, void* stream) {
  ADM_REQUIRE(h && x && out && recs && n_out, "unet_profile: null argument");
  hipStream_t st = (hipStream_t)stream;
  ADM_TRY(finalize(h));
  ADM_TRY(plan(h, B));
  std::vector<float> t(B, timestep);
  ADM_TRY(copy_h2d(h->t_dev, t.data(), sizeof(float) * B, st));
  ADM_TRY(stream_sync(st));
  std::vector<adm_op_profile> v;
  OpTimer tm;
  tm.recs = &v;
  Bf16Scope fp32(0);
  InferenceScope inf(&h->net, st);
  ADM_TRY(inf.rc);
  ADM_TRY(run_forward(h, x, out, B, nullptr, st, &tm));
  *n_out = (int)v.size();
  for (int i = 0; i < (int)v.size() && i < cap; ++i) recs[i] = v[i];
  return 0;
}

int adm_unet_plan_ops(adm_unet_t* h, int B, adm_plan_op* recs, int cap, int* n_out) {
  ADM_REQUIRE(h && B > 0 && (recs || cap == 0) && n_out, "unet_plan_ops: bad argument");
  ADM_TRY(finalize(h));
  ADM_TRY(plan(h, B));
  return h->net.plan_report(h->temb_all, h->temb_rows, recs, cap, n_out);
}

// The sampling loop: all argument checks are here.
int adm_sample_loop_ex(adm_unet_t* h, const adm_sample_loop_args* a, void* stream) {
  ADM_REQUIRE(h && a && a->x && a->coef_host && a->n_steps > 0, "sample_loop: bad argument");
  ADM_REQUIRE(a->mode >= SCHED_PLAIN && a->mode <= SCHED_MULTISTEP, "sample_loop: mode must be 0 (plain), 1 (thresholded) or 2 (multistep)");
  ADM_REQUIRE(a->noise_source == 0 || a->noise_source == 1, "sample_loop: noise_source must be 0 (step_noise, or none) or 1 (adm noise stream 1)");
  if (a->encoding_uncond != nullptr) {   // guided; NULL: unguided, and the model may be unconditional
    ADM_REQUIRE(h->cfg.cross_attention_dim > 0, "sample_loop: this model has no cross-attention (UNet2DModel): nothing to guide");
    ADM_REQUIRE(h->net.ctx != nullptr && h->net.ctx_S > 0, "sample_loop: no encoding set (adm_unet_set_encoding)");
    ADM_REQUIRE(std::isfinite(a->guidance_scale), "sample_loop: the guidance scale must be finite");
  }
  ADM_REQUIRE(std::isfinite(a->guidance_rescale) && a->guidance_rescale >= 0.f && a->guidance_rescale <= 1.f,
              "sample_loop: guidance_rescale must be in [0, 1]");
  ADM_REQUIRE(a->guidance_rescale == 0.f || a->encoding_uncond != nullptr,
              "sample_loop: guidance_rescale needs encoding_uncond (it rescales the guided output)");
  ADM_REQUIRE(a->prediction >= PRED_EPSILON && a->prediction <= PRED_V, "sample_loop: prediction must be 0 (epsilon), 1 (sample) or 2 (v_prediction)");
  if (a->unipc_host != nullptr) {
    ADM_REQUIRE(a->mode != SCHED_MULTISTEP, "sample_loop: with unipc_host, mode must be 0 (x0 as predicted) or 1 (thresholded); 2 (the multistep step) is another step");
    ADM_REQUIRE(a->step_noise == nullptr, "sample_loop: step_noise must be NULL with unipc_host (the UniPC step has no noise rows)");
    ADM_REQUIRE(a->noise_source == 0, "sample_loop: noise_source must be 0 with unipc_host (the UniPC step has no noise rows)");
    ADM_REQUIRE(a->unipc_host[0].c_t == 0.f && a->unipc_host[0].p_m1 == 0.f,
                "sample_loop: the first row of a UniPC run has no corrector and a first-order predictor (unipc_host[0].c_t == 0 and p_m1 == 0)");
  }
  if (a->mode == SCHED_MULTISTEP) {
    ADM_REQUIRE(a->k_hist_host != nullptr, "sample_loop: the multistep loop needs k_hist_host");
    ADM_REQUIRE(a->prediction == PRED_EPSILON, "sample_loop: the multistep loop is epsilon only and not thresholded");
    ADM_REQUIRE(a->noise_source == 0, "sample_loop: the multistep step has no noise rows");
    ADM_REQUIRE(a->k_hist_host[0] == 0.f, "sample_loop: the first row of a run must be first order (k_hist[0] == 0)");
  }
  if (a->noise_source == 1) {
    ADM_REQUIRE(a->B > 0, "sample_loop: bad argument");
    ADM_REQUIRE(a->step_noise == nullptr, "sample_loop: a noise buffer and the noise stream exclude each other");
    ADM_REQUIRE(a->row_offset >= 0, "sample_loop: row_offset must be >= 0");
    ADM_REQUIRE((uint64_t)a->row_offset + (uint64_t)a->B <= 0xffffffffull, "sample_loop: row_offset + B must fit in 32 bits");
    ADM_REQUIRE(((long)h->cfg.in_channels * h->cfg.sample_h * h->cfg.sample_w) % 4 == 0, "sample_loop: C*H*W must be a multiple of 4");
    for (int i = 0; i < a->n_steps; ++i)   // the counter's third word is the row's timestep as an integer
      ADM_REQUIRE(a->coef_host[i].timestep >= 0.f && a->coef_host[i].timestep < 2147483648.f, "sample_loop: every timestep must be in [0, 2^31)");
  }
  if (a->keep != nullptr) {   // the known-region overwrite (include/adm.h "Region in-painting"); NULL: off, the other five fields are ignored
    ADM_REQUIRE(a->known != nullptr && a->known_noise != nullptr, "sample_loop: keep needs known and known_noise");
    ADM_REQUIRE(a->known_coef_host != nullptr, "sample_loop: keep needs known_coef_host (n_steps x 2 host floats)");
    ADM_REQUIRE(a->mask == nullptr, "sample_loop: keep and mask exclude each other (the known-region overwrite replaces the staged mask)");
  }
  if (a->window_total_w != 0) {   // windowed (include/adm.h "Windowed sampling"); 0: off, and window_stride / window_wrap are ignored
    ADM_REQUIRE(a->B > 0, "sample_loop: bad argument");
    ADM_REQUIRE(a->mask == nullptr, "sample_loop: mask must be NULL with window_total_w (the mask's layout assumes the model's width)");
    int nW = 0;
    ADM_TRY(window_count("sample_loop", "window_", a->window_total_w, h->cfg.sample_w, a->window_stride, a->window_wrap, &nW));
    ADM_REQUIRE((long)a->B * nW <= 2147483647L, "sample_loop: B times the number of windows (window_total_w, window_stride) must fit in an int");
  }
  return run_loop_fp32(h, *a, stream);
}

// ---- the frozen positional entry points (include/adm.h): a struct fill and one call each
static adm_sample_loop_args loop_args(float* x, int B, const adm_sched_coef* coef_host, int n_steps, const float* step_noise, const float* mask,
                                      int mask_start, int mask_end, uint8_t* u8_out, int use_graph) {
  adm_sample_loop_args a{};
  a.x = x; a.B = B; a.coef_host = coef_host; a.n_steps = n_steps; a.step_noise = step_noise; a.mask = mask; a.mask_start = mask_start;
  a.mask_end = mask_end; a.u8_out = u8_out; a.use_graph = use_graph;
  return a;
}
// thresholded == 0: the static clamp, and lo, hi, w, max_value are ignored
static void loop_args_threshold(adm_sample_loop_args& a, int thresholded, int lo, int hi, float w, float max_value) {
  if (!thresholded) return;
  a.mode = SCHED_THRESH; a.lo = lo; a.hi = hi; a.w = w; a.max_value = max_value;
}

int adm_sample_loop(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, int n_steps,
                    const float* step_noise, const float* mask, int mask_start, int mask_end, uint8_t* u8_out,
                    int use_graph, void* stream) {
  const adm_sample_loop_args a = loop_args(x, B, coef_host, n_steps, step_noise, mask, mask_start, mask_end, u8_out, use_graph);
  return adm_sample_loop_ex(h, &a, stream);
}

int adm_sample_loop_multistep(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, const float* k_hist_host,
                              int n_steps, const float* step_noise, const float* mask, int mask_start, int mask_end,
                              uint8_t* u8_out, int use_graph, void* stream) {
  adm_sample_loop_args a = loop_args(x, B, coef_host, n_steps, step_noise, mask, mask_start, mask_end, u8_out, use_graph);
  a.mode = SCHED_MULTISTEP; a.k_hist_host = k_hist_host;
  return adm_sample_loop_ex(h, &a, stream);
}

int adm_sample_loop_thresholded(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, int n_steps,
                                const float* step_noise, const float* mask, int mask_start, int mask_end, uint8_t* u8_out,
                                int use_graph, void* stream, int lo, int hi, float w, float max_value) {
  adm_sample_loop_args a = loop_args(x, B, coef_host, n_steps, step_noise, mask, mask_start, mask_end, u8_out, use_graph);
  loop_args_threshold(a, 1, lo, hi, w, max_value);
  return adm_sample_loop_ex(h, &a, stream);
}

int adm_sample_loop_pred(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, int n_steps, const float* step_noise,
                         const float* mask, int mask_start, int mask_end, uint8_t* u8_out, int use_graph, void* stream, int lo,
                         int hi, float w, float max_value, int thresholded, int prediction) {
  adm_sample_loop_args a = loop_args(x, B, coef_host, n_steps, step_noise, mask, mask_start, mask_end, u8_out, use_graph);
  loop_args_threshold(a, thresholded, lo, hi, w, max_value);
  a.prediction = prediction;
  return adm_sample_loop_ex(h, &a, stream);
}

int adm_sample_loop_guided(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, const float* k_hist_host, int n_steps,
                           const float* step_noise, const float* mask, int mask_start, int mask_end, uint8_t* u8_out, int use_graph,
                           void* stream, int lo, int hi, float w, float max_value, int thresholded, int prediction,
                           const float* encoding_uncond_dev, float guidance_scale) {
  ADM_REQUIRE(encoding_uncond_dev != nullptr, "sample_loop_guided: bad argument");   // (NULL means "unguided" to the struct)
  // (`thresholded` together with k_hist_host: the struct has one mode and cannot say it)
  ADM_REQUIRE(k_hist_host == nullptr || !thresholded, "sample_loop_guided: the multistep loop is epsilon only and not thresholded");
  adm_sample_loop_args a = loop_args(x, B, coef_host, n_steps, step_noise, mask, mask_start, mask_end, u8_out, use_graph);
  loop_args_threshold(a, thresholded, lo, hi, w, max_value);
  if (k_hist_host != nullptr) { a.mode = SCHED_MULTISTEP; a.k_hist_host = k_hist_host; }
  a.prediction = prediction; a.encoding_uncond = encoding_uncond_dev; a.guidance_scale = guidance_scale;
  return adm_sample_loop_ex(h, &a, stream);
}

int adm_sample_loop_philox(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, int n_steps, const float* mask, int mask_start,
                           int mask_end, uint8_t* u8_out, int use_graph, void* stream, int lo, int hi, float w, float max_value,
                           int thresholded, int prediction, const float* encoding_uncond_dev, float guidance_scale, uint64_t seed,
                           int row_offset) {
  adm_sample_loop_args a = loop_args(x, B, coef_host, n_steps, nullptr, mask, mask_start, mask_end, u8_out, use_graph);
  loop_args_threshold(a, thresholded, lo, hi, w, max_value);
  a.prediction = prediction; a.encoding_uncond = encoding_uncond_dev; a.guidance_scale = guidance_scale;
  a.noise_source = 1; a.seed = seed; a.row_offset = row_offset;
  return adm_sample_loop_ex(h, &a, stream);
}

int adm_unet_loop_captures(adm_unet_t* h) { return h ? h->captures : 0; }

// The inversion loop: all argument checks are here. The fields it honours are x, B, coef_host, n_steps, use_graph, prediction and the three
// window fields; every other one is a feature of the sampling step that the inversion step does not have, and is refused by its name.
int adm_encode_loop_ex(adm_unet_t* h, const adm_sample_loop_args* a, void* stream) {
  ADM_REQUIRE(h && a && a->x && a->coef_host && a->n_steps > 0 && a->B > 0, "encode_loop: bad argument");
  ADM_REQUIRE(a->mode == SCHED_PLAIN, "encode_loop: mode must be 0 (the inversion step is not thresholded and not multistep)");
  ADM_REQUIRE(a->prediction >= PRED_EPSILON && a->prediction <= PRED_V, "encode_loop: prediction must be 0 (epsilon), 1 (sample) or 2 (v_prediction)");
  ADM_REQUIRE(a->k_hist_host == nullptr, "encode_loop: k_hist_host must be NULL (inversion is a DDIM procedure)");
  ADM_REQUIRE(a->unipc_host == nullptr, "encode_loop: unipc_host must be NULL (inversion is a DDIM procedure)");
  ADM_REQUIRE(a->step_noise == nullptr, "encode_loop: step_noise must be NULL (inversion is deterministic)");
  ADM_REQUIRE(a->noise_source == 0, "encode_loop: noise_source must be 0 (inversion is deterministic)");
  ADM_REQUIRE(a->seed == 0, "encode_loop: seed must be 0 (inversion is deterministic)");
  ADM_REQUIRE(a->row_offset == 0, "encode_loop: row_offset must be 0 (inversion is deterministic)");
  ADM_REQUIRE(a->mask == nullptr, "encode_loop: mask must be NULL");
  ADM_REQUIRE(a->mask_start == 0, "encode_loop: mask_start must be 0");
  ADM_REQUIRE(a->mask_end == 0, "encode_loop: mask_end must be 0");
  ADM_REQUIRE(a->u8_out == nullptr, "encode_loop: u8_out must be NULL (the result is noise, not an image)");
  ADM_REQUIRE(a->lo == 0, "encode_loop: lo must be 0 (the inversion step is not thresholded)");
  ADM_REQUIRE(a->hi == 0, "encode_loop: hi must be 0 (the inversion step is not thresholded)");
  ADM_REQUIRE(a->w == 0.f, "encode_loop: w must be 0 (the inversion step is not thresholded)");
  ADM_REQUIRE(a->max_value == 0.f, "encode_loop: max_value must be 0 (the inversion step is not thresholded)");
  ADM_REQUIRE(a->encoding_uncond == nullptr, "encode_loop: encoding_uncond must be NULL (guided inversion is not offered)");
  ADM_REQUIRE(a->guidance_scale == 0.f, "encode_loop: guidance_scale must be 0 (guided inversion is not offered)");
  ADM_REQUIRE(a->guidance_rescale == 0.f, "encode_loop: guidance_rescale must be 0 (guided inversion is not offered)");
  ADM_REQUIRE(a->keep == nullptr, "encode_loop: keep must be NULL (inversion has no known region)");
  ADM_REQUIRE(a->known == nullptr, "encode_loop: known must be NULL (inversion has no known region)");
  ADM_REQUIRE(a->known_noise == nullptr, "encode_loop: known_noise must be NULL (inversion has no known region)");
  ADM_REQUIRE(a->known_coef_host == nullptr, "encode_loop: known_coef_host must be NULL (inversion has no known region)");
  ADM_REQUIRE(a->known_batched == 0, "encode_loop: known_batched must be 0 (inversion has no known region)");
  ADM_REQUIRE(a->keep_batched == 0, "encode_loop: keep_batched must be 0 (inversion has no known region)");
  adm_sample_loop_args e = *a;
  if (a->window_total_w != 0) {   // windowed (include/adm.h "Windowed sampling"); 0: off, and window_stride / window_wrap are ignored
    int nW = 0;
    ADM_TRY(window_count("encode_loop", "window_", a->window_total_w, h->cfg.sample_w, a->window_stride, a->window_wrap, &nW));
    ADM_REQUIRE((long)a->B * nW <= 2147483647L, "encode_loop: B times the number of windows (window_total_w, window_stride) must fit in an int");
  } else {
    e.window_stride = e.window_wrap = 0;
  }
  ADM_REQUIRE(((long)a->B * h->cfg.in_channels * h->cfg.sample_h * (a->window_total_w != 0 ? a->window_total_w : h->cfg.sample_w)) % 4 == 0,
              "encode_loop: B*C*H*W must be a multiple of 4");
  e.mode = LOOP_ENCODE;
  return run_loop_fp32(h, e, stream);
}

// FROZEN: a struct fill and one call
int adm_encode_loop(adm_unet_t* h, float* x, int B, const adm_sched_coef* coef_host, int n_steps, int use_graph,
                    void* stream) {
  const adm_sample_loop_args a = loop_args(x, B, coef_host, n_steps, nullptr, nullptr, 0, 0, nullptr, use_graph);
  return adm_encode_loop_ex(h, &a, stream);
}

}  // extern "C"
