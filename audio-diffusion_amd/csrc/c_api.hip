// c_api.hip — error state + op-level C-ABI entry points (include/adm.h). The UNet executor and the
// sampling loop export their own entry points from unet_exec.hip.
#include <map>
#include <mutex>

#include "adm_kernels.h"

namespace adm {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error() { return g_err.c_str(); }
}  // namespace adm

using namespace adm;

// ADM_SEGV_BACKTRACE=1: a SIGSEGV / SIGABRT inside the process prints the NATIVE stack (backtrace_symbols_fd) before the default action — Python's
// faulthandler stops at the ctypes call. Diagnostic only; nothing is installed without the variable.
#if !defined(ADM_EMU)
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
namespace {
void adm_segv_handler(int sig) {
  void* frames[64];
  const int n = backtrace(frames, 64);
  const char msg[] = "\n[adm] fatal signal, native stack:\n";
  (void)!write(2, msg, sizeof(msg) - 1);
  backtrace_symbols_fd(frames, n, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}
struct AdmSegvInstall {
  AdmSegvInstall() {
    const char* e = getenv("ADM_SEGV_BACKTRACE");
    if (e && atoi(e)) { signal(SIGSEGV, adm_segv_handler); signal(SIGABRT, adm_segv_handler); signal(SIGBUS, adm_segv_handler); }
  }
} g_adm_segv_install;
}  // namespace
#endif

extern "C" {

int adm_version(void) { return 123; }   // 123: adm_encode_step / adm_encode_loop_ex (DDIM inversion for the three prediction types, conditional models and the windowed loop; an inversion row carries the conversion pair (sa_c, sb_c) in k_x / k_noise; adm_encode_loop is frozen and calls adm_encode_loop_ex); 122: test aid adm_unet_loop_captures (how often a handle has captured a step of the sampling loop); 121: adm_window_crossfade (the weighted join of a tiled codec's windows, csrc/k_window.hip) and adm_vae_sample_moments (adm_vae_encode's sampling tail as a launch of its own): AutoencoderKL.decode_tiled / encode_tiled, windowed sampling with a vqvae; 120: test aids adm_conv2d_gn_finish (a convolution announced as the executors announce it when a GroupNorm reads its output) and adm_last_conv_detail (what the fp32 implicit-GEMM / small-channel launchers chose: cout tile, split, finish kernel, tap mask, pixel tile); 119: test aid adm_mel_last_variant; 118: adm_sched_step_args.known / .known_noise / .keep / .known_table / .known_batched / .keep_batched, adm_sample_loop_args the same with .known_coef_host (region in-painting: the known-region overwrite under an arbitrary keep mask inside the step kernels, csrc/k_sched_common.h sched_known4; no new symbol); 117: adm_window_gather / adm_window_blend, adm_sample_loop_args.window_total_w / .window_stride / .window_wrap (windowed sampling: wide and circular spectrograms through overlapping model-sized windows in the captured loop, csrc/k_window.hip; no new loop symbol); 116: adm_unipc_coef, adm_sched_step_args.unipc_table / .last, adm_sample_loop_args.unipc_host (the UniPC predictor-corrector step and loop, csrc/k_unipc.hip; no new symbol); 115: adm_sched_step_args.guidance_rescale / .rescale, adm_sample_loop_args.guidance_rescale (rescaled classifier-free guidance; no new symbol); 114: adm_sched_step_args / adm_sample_loop_args and adm_sched_step_ex / adm_sched_threshold_ex / adm_sample_loop_ex (one struct-argument entry point per family; the positional ones are frozen); 113: adm_randn / adm_sched_step_philox / adm_sample_loop_philox (noise drawn in the step kernel: "adm noise stream 1"); 112: adm_sched_threshold_guided / adm_sched_step_guided / adm_sample_loop_guided (classifier-free guidance); 111: adm_sched_step_pred / adm_sched_threshold_pred / adm_sample_loop_pred / adm_noise_and_velocity (sample and v_prediction models); 110: adm_sched_threshold / adm_sched_step_thresholded / adm_sample_loop_thresholded (dynamic thresholding of x0); 109: adm_sched_multistep / adm_sample_loop_multistep (second-order multistep scheduler step and loop); 108: option "wgrad_path", test aids adm_last_wgrad_variant / adm_wgrad_reduce; 107: test aids adm_time_embedding / adm_temb_proj; 106: adm_last_attention_variant; 105: option "side_overlap", adm_unet_plan_ops / adm_vae_plan_ops (adm_plan_op)
//   // 104 (round 6): adm_conv_args.single_sample, option "single_sample"; 103 (round 6): adm_conv_args.wino6_rule, adm_unet_set_option, adm_release_stream
//   // 102 (round 5): Winograd buffers hold two images (adm_winograd_packed_floats)
//   // 101 (round 4): adm_slerp_grid takes double weights (round 3), blocked-image entry points
const char* adm_last_error(void) { return adm::last_error(); }
int adm_set_option(const char* name, int value) {
  ADM_REQUIRE(name, "set_option: null name");
  const std::string nm(name);
  static const char* known[] = {"conv_wino", "wino_pair", "wino5", "wino6", "single_sample", "wgrad_max_split", "wgrad_path", "conv_bf16", "conv_op16_f16", "blk_direct_dy", "gn_fuse_finish", "side_overlap"};
  bool ok = false;
  for (const char* k : known) ok |= nm == k;
  if (!ok) ADM_FAIL(std::string("set_option: unknown option ") + name);
  // the dispatch epoch (training nets re-learn which weight images they read: a full re-pack) moves only when a value really
  // changes — a model that sets the options it already runs under (every enable_training does) leaves other nets alone
  if (nm == "conv_wino")   // validate BEFORE the value is recorded: a rejected value must neither move the epoch nor be remembered
    ADM_REQUIRE(adm::winograd_mode_available(value), "set_option: conv_wino takes -1 (environment), 0 (direct MFMA kernel only) or 4 (Winograd kernels: "
                "the default); modes 1-3 were earlier kernel generations, retired in round 6");
  if (nm == "wino6")
    ADM_REQUIRE(value == -1 || value == 0 || value == 1 || value == 2 || (value >= 16 && value <= 65536),
                "set_option: wino6 takes -1 (environment), 0 (off), 1 (default layer rule), 2 (every layer the kernel tiles) or a plane-size floor n >= 16");
  if (nm == "single_sample") ADM_REQUIRE(value >= -1 && value <= 1, "set_option: single_sample takes -1 (environment), 0 (off) or 1 (on)");
  if (nm == "side_overlap") ADM_REQUIRE(value >= -1 && value <= 1, "set_option: side_overlap takes -1 (environment), 0 (off) or 1 (on)");
  if (nm == "wgrad_path")
    ADM_REQUIRE(value >= 0 && value <= 3, "set_option: wgrad_path takes 0 (heuristic), 1 (no eight-wave kernel), 2 (no software-pipelined kernels) or "
                "3 (generic kernels only)");
  static std::mutex mu;
  static std::map<std::string, int> last;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = last.find(nm);
    const bool same = it != last.end() && it->second == value;
    last[nm] = value;
    if (!same) adm::bump_dispatch_epoch();
  }
  if (nm == "conv_wino") { adm::set_winograd_mode(value); return 0; }
  if (nm == "wino5") { adm::set_winograd_v5(value); return 0; }
  if (nm == "wino6") { adm::set_winograd_v6(value); return 0; }
  if (nm == "single_sample") { adm::set_single_sample(value); return 0; }
  if (nm == "wino_pair") { adm::set_winograd_pair(value); return 0; }
  if (nm == "wgrad_max_split") { adm::set_wgrad_max_split(value); return 0; }
  if (nm == "wgrad_path") { adm::set_wgrad_path(value); return 0; }
  if (nm == "conv_bf16") { adm::set_conv_bf16(value); return 0; }
  if (nm == "conv_op16_f16") { adm::set_conv_op16_f16(value); return 0; }
  if (nm == "gn_fuse_finish") { adm::set_gn_fuse_finish(value); return 0; }
  if (nm == "side_overlap") { adm::set_side_overlap(value); return 0; }
  adm::set_blk_direct_dy(value);
  return 0;
}
int adm_last_conv_variant(void) { return adm::last_conv_variant(); }
int adm_last_conv_detail(int* out, int n) {
  const adm::ConvDetail d = adm::last_conv_detail();
  const int v = adm::last_conv_variant();
  const bool fresh = d.variant == v && v != 0;       // (a Winograd / bf16 launch since: only the variant is known)
  const int slots[ADM_CONV_DETAIL_SLOTS] = {v, d.bm, d.split, d.finish, d.tap_mask, d.TW, d.TH, d.NI, d.kpf, d.zparts};
  for (int i = 0; out != nullptr && i < n; ++i) out[i] = i >= ADM_CONV_DETAIL_SLOTS ? 0 : ((i == 0 || fresh) ? slots[i] : 0);
  return v;
}
int adm_last_attention_variant(void) { return adm::last_attention_variant(); }
int adm_release_stream(void* stream) { adm::conv_ksplit_release((hipStream_t)stream); return 0; }
int adm_has_experiments(void) { return 0; }   // (kept for ABI stability: the experiments builds were retired in round 6)
int adm_is_device_build(void) {
#if defined(ADM_EMU)
  return 0;
#else
  return 1;
#endif
}

// The scheduler step and the selection: all validation that is not about the shape (k_sched.hip's launchers have that) is here.
int adm_sched_step_ex(const adm_sched_step_args* a, void* stream) {
  ADM_REQUIRE(a != nullptr, "sched_step: null argument struct");
  ADM_REQUIRE(a->x && a->eps && a->out && a->coef_table, "sched_step: null argument");
  ADM_REQUIRE(a->noise_source == 0 || a->noise_source == 1, "sched_step: noise_source must be 0 (the noise buffer, or none) or 1 (adm noise stream 1)");
  SchedStepParams p{a->x, a->eps, a->noise, a->out, a->u8_out, a->coef_table, a->step_dev, a->step, a->mask, a->n_mask_steps,
                    a->mask_start, a->mask_end, a->B, a->C, a->H, a->W};
  p.eps_uncond = a->eps_uncond; p.guidance = a->guidance_scale;
  p.guidance_rescale = a->guidance_rescale; p.rescale = a->rescale;   // (0: off; checked by k_sched.hip's launchers, before any launch)
  if (a->keep != nullptr) {   // the known-region overwrite ("Region in-painting"); refused here, by field, before any launch
    ADM_REQUIRE(a->known != nullptr && a->known_noise != nullptr, "sched_step: keep needs known and known_noise");
    ADM_REQUIRE(a->known_table != nullptr, "sched_step: keep needs known_table (two floats per row of coef_table)");
    ADM_REQUIRE(a->mask == nullptr, "sched_step: keep and mask exclude each other (the known-region overwrite replaces the staged mask)");
    p.known = a->known; p.known_noise = a->known_noise; p.keep = a->keep; p.known_table = a->known_table;
    p.known_batched = a->known_batched != 0; p.keep_batched = a->keep_batched != 0;
  }
  if (a->mode == SCHED_THRESH) {
    ADM_REQUIRE(a->scale != nullptr, "sched_step: the thresholded step needs scale");
    p.lo = a->lo; p.hi = a->hi; p.w = a->w; p.max_value = a->max_value; p.scale = a->scale;
  }
  if (a->unipc_table != nullptr) {   // the UniPC step (k_unipc.hip): its own kernel and launcher; hist is the two-slot history
    ADM_REQUIRE(a->mode != SCHED_MULTISTEP, "sched_step: with unipc_table, mode must be 0 (x0 as predicted) or 1 (thresholded); 2 (the multistep step) is another step");
    ADM_REQUIRE(a->noise == nullptr, "sched_step: noise must be NULL with unipc_table (the UniPC step has no noise rows)");
    ADM_REQUIRE(a->noise_source == 0, "sched_step: noise_source must be 0 with unipc_table (the UniPC step has no noise rows)");
    ADM_REQUIRE(a->hist != nullptr && a->last != nullptr, "sched_step: the UniPC step needs last and the two-slot hist");
    p.unipc_table = a->unipc_table; p.last = a->last; p.hist = a->hist;
    return launch_unipc_step(p, a->mode, (hipStream_t)stream, a->prediction);
  }
  if (a->mode == SCHED_MULTISTEP) {
    ADM_REQUIRE(a->k_hist_table && a->hist, "sched_step: the multistep step needs k_hist_table and hist");
    ADM_REQUIRE(a->scale == nullptr, "sched_step: the multistep step is epsilon only and not thresholded");
    p.hist = a->hist; p.k_hist_table = a->k_hist_table;
  }
  if (a->noise_source == 1) {
    ADM_REQUIRE(a->B > 0 && a->C > 0 && a->H > 0 && a->W > 0, "sched_step: bad shape");
    ADM_REQUIRE(a->row_offset >= 0, "sched_step: row_offset must be >= 0");
    ADM_REQUIRE((uint64_t)a->row_offset + (uint64_t)a->B <= 0xffffffffull, "sched_step: row_offset + B must fit in 32 bits");
    p.philox = 1;
    p.nvals[0] = (uint32_t)(a->seed & 0xffffffffull); p.nvals[1] = (uint32_t)(a->seed >> 32); p.nvals[2] = (uint32_t)a->row_offset; p.nvals[3] = 0;
  }
  return launch_sched_step(p, a->mode, (hipStream_t)stream, a->prediction);
}

int adm_sched_threshold_ex(const adm_sched_step_args* a, void* stream) {
  ADM_REQUIRE(a != nullptr, "sched_threshold: null argument struct");
  ADM_REQUIRE(a->x && a->eps && a->coef_table && a->scale, "sched_threshold: null argument");
  SchedStepParams p{a->x, a->eps, nullptr, nullptr, nullptr, a->coef_table, a->step_dev, a->step, nullptr, 0, 0, 0, a->B, a->C, a->H, a->W};
  p.eps_uncond = a->eps_uncond; p.guidance = a->guidance_scale;
  p.guidance_rescale = a->guidance_rescale; p.rescale = a->rescale;   // (0: off; checked by k_sched.hip's launchers, before any launch)
  p.lo = a->lo; p.hi = a->hi; p.w = a->w; p.max_value = a->max_value; p.scale = a->scale;
  return launch_sched_threshold(p, (hipStream_t)stream, a->prediction);
}

// ---- the frozen positional entry points (include/adm.h): a struct fill and one call each
static adm_sched_step_args sched_args(const float* x, const float* eps, const float* noise, float* out, uint8_t* u8_out,
                                      const adm_sched_coef* coef_table, const int* step_dev, int step, const float* mask, int n_mask_steps,
                                      int mask_start, int mask_end, int B, int C, int H, int W) {
  adm_sched_step_args a{};
  a.x = x; a.eps = eps; a.noise = noise; a.out = out; a.u8_out = u8_out; a.coef_table = coef_table; a.step_dev = step_dev; a.step = step;
  a.mask = mask; a.n_mask_steps = n_mask_steps; a.mask_start = mask_start; a.mask_end = mask_end; a.B = B; a.C = C; a.H = H; a.W = W;
  return a;
}
// scale == NULL: the static clip (mode 0; lo, hi, w, max_value are ignored); otherwise the thresholded step
static void sched_args_threshold(adm_sched_step_args& a, int lo, int hi, float w, float max_value, float* scale) {
  if (scale == nullptr) return;
  a.mode = SCHED_THRESH; a.lo = lo; a.hi = hi; a.w = w; a.max_value = max_value; a.scale = scale;
}
static adm_sched_step_args threshold_args(const float* x, const float* eps, const adm_sched_coef* coef_table, const int* step_dev, int step,
                                          int lo, int hi, float w, float max_value, float* scale_out, int B, int C, int H, int W) {
  adm_sched_step_args a = sched_args(x, eps, nullptr, nullptr, nullptr, coef_table, step_dev, step, nullptr, 0, 0, 0, B, C, H, W);
  a.lo = lo; a.hi = hi; a.w = w; a.max_value = max_value; a.scale = scale_out;
  return a;
}

int adm_sched_step(const float* x, const float* eps, const float* noise, float* out, uint8_t* u8_out,
                   const adm_sched_coef* coef_table, const int* step_dev, int step, const float* mask,
                   int n_mask_steps, int mask_start, int mask_end, int B, int C, int H, int W, void* stream) {
  const adm_sched_step_args a = sched_args(x, eps, noise, out, u8_out, coef_table, step_dev, step, mask, n_mask_steps, mask_start, mask_end, B, C, H, W);
  return adm_sched_step_ex(&a, stream);
}

int adm_sched_multistep(const float* x, const float* eps, const float* noise, float* out, uint8_t* u8_out,
                        const adm_sched_coef* coef_table, const float* k_hist_table, float* hist, const int* step_dev,
                        int step, const float* mask, int n_mask_steps, int mask_start, int mask_end, int B, int C, int H,
                        int W, void* stream) {
  adm_sched_step_args a = sched_args(x, eps, noise, out, u8_out, coef_table, step_dev, step, mask, n_mask_steps, mask_start, mask_end, B, C, H, W);
  a.mode = SCHED_MULTISTEP; a.k_hist_table = k_hist_table; a.hist = hist;
  return adm_sched_step_ex(&a, stream);
}

int adm_sched_threshold(const float* x, const float* eps, const adm_sched_coef* coef_table, const int* step_dev, int step, int lo,
                        int hi, float w, float max_value, float* scale_out, int B, int C, int H, int W, void* stream) {
  const adm_sched_step_args a = threshold_args(x, eps, coef_table, step_dev, step, lo, hi, w, max_value, scale_out, B, C, H, W);
  return adm_sched_threshold_ex(&a, stream);
}

int adm_sched_step_thresholded(const float* x, const float* eps, const float* noise, float* out, uint8_t* u8_out,
                               const adm_sched_coef* coef_table, const int* step_dev, int step, const float* mask,
                               int n_mask_steps, int mask_start, int mask_end, int B, int C, int H, int W, void* stream, int lo,
                               int hi, float w, float max_value, float* scale) {
  adm_sched_step_args a = sched_args(x, eps, noise, out, u8_out, coef_table, step_dev, step, mask, n_mask_steps, mask_start, mask_end, B, C, H, W);
  a.mode = SCHED_THRESH;   // (not sched_args_threshold: a null scale is refused here, not read as "the static clip")
  a.lo = lo; a.hi = hi; a.w = w; a.max_value = max_value; a.scale = scale;
  return adm_sched_step_ex(&a, stream);
}

int adm_sched_threshold_pred(const float* x, const float* eps, const adm_sched_coef* coef_table, const int* step_dev, int step, int lo,
                             int hi, float w, float max_value, float* scale_out, int B, int C, int H, int W, void* stream,
                             int prediction) {
  adm_sched_step_args a = threshold_args(x, eps, coef_table, step_dev, step, lo, hi, w, max_value, scale_out, B, C, H, W);
  a.prediction = prediction;
  return adm_sched_threshold_ex(&a, stream);
}

int adm_sched_step_pred(const float* x, const float* eps, const float* noise, float* out, uint8_t* u8_out,
                        const adm_sched_coef* coef_table, const int* step_dev, int step, const float* mask, int n_mask_steps,
                        int mask_start, int mask_end, int B, int C, int H, int W, void* stream, int lo, int hi, float w,
                        float max_value, float* scale, int prediction) {
  adm_sched_step_args a = sched_args(x, eps, noise, out, u8_out, coef_table, step_dev, step, mask, n_mask_steps, mask_start, mask_end, B, C, H, W);
  sched_args_threshold(a, lo, hi, w, max_value, scale);
  a.prediction = prediction;
  return adm_sched_step_ex(&a, stream);
}

int adm_sched_threshold_guided(const float* x, const float* eps_cond, const float* eps_uncond, float guidance_scale,
                               const adm_sched_coef* coef_table, const int* step_dev, int step, int lo, int hi, float w, float max_value,
                               float* scale_out, int B, int C, int H, int W, void* stream, int prediction) {
  ADM_REQUIRE(eps_uncond != nullptr, "sched_threshold_guided: null argument");   // (NULL means "unguided" to the struct)
  adm_sched_step_args a = threshold_args(x, eps_cond, coef_table, step_dev, step, lo, hi, w, max_value, scale_out, B, C, H, W);
  a.prediction = prediction; a.eps_uncond = eps_uncond; a.guidance_scale = guidance_scale;
  return adm_sched_threshold_ex(&a, stream);
}

int adm_sched_step_guided(const float* x, const float* eps_cond, const float* eps_uncond, float guidance_scale, const float* noise,
                          float* out, uint8_t* u8_out, const adm_sched_coef* coef_table, const float* k_hist_table, float* hist,
                          const int* step_dev, int step, const float* mask, int n_mask_steps, int mask_start, int mask_end, int B, int C,
                          int H, int W, void* stream, int lo, int hi, float w, float max_value, float* scale, int prediction) {
  ADM_REQUIRE(eps_uncond != nullptr, "sched_step_guided: null argument");   // (NULL means "unguided" to the struct)
  adm_sched_step_args a = sched_args(x, eps_cond, noise, out, u8_out, coef_table, step_dev, step, mask, n_mask_steps, mask_start, mask_end, B, C, H, W);
  a.eps_uncond = eps_uncond; a.guidance_scale = guidance_scale; a.prediction = prediction;
  if (hist != nullptr) {   // the multistep step; with a scale as well it is refused as "not thresholded"
    a.mode = SCHED_MULTISTEP; a.k_hist_table = k_hist_table; a.hist = hist; a.scale = scale;
  } else {
    sched_args_threshold(a, lo, hi, w, max_value, scale);
  }
  return adm_sched_step_ex(&a, stream);
}

int adm_randn(float* out, int B, long per_sample, uint64_t seed, int row_offset, int t, int noise_stream, void* stream) {
  return launch_randn(out, B, per_sample, seed, row_offset, t, noise_stream, (hipStream_t)stream);
}

int adm_sched_step_philox(const float* x, const float* eps_cond, const float* eps_uncond, float guidance_scale, float* out, uint8_t* u8_out,
                          const adm_sched_coef* coef_table, const int* step_dev, int step, const float* mask, int n_mask_steps,
                          int mask_start, int mask_end, int B, int C, int H, int W, void* stream, int lo, int hi, float w, float max_value,
                          float* scale, int prediction, uint64_t seed, int row_offset) {
  adm_sched_step_args a = sched_args(x, eps_cond, nullptr, out, u8_out, coef_table, step_dev, step, mask, n_mask_steps, mask_start, mask_end, B, C, H, W);
  a.eps_uncond = eps_uncond; a.guidance_scale = guidance_scale; a.prediction = prediction;
  sched_args_threshold(a, lo, hi, w, max_value, scale);
  a.noise_source = 1; a.seed = seed; a.row_offset = row_offset;
  return adm_sched_step_ex(&a, stream);
}

int adm_encode_step(float* x, const float* model_out, const adm_sched_coef* coef_table, const int* step_dev, int step, int prediction,
                    long n, void* stream) {
  ADM_REQUIRE(x && model_out && coef_table, "encode_step: null argument");
  return launch_encode_step(x, model_out, coef_table, step_dev, step, prediction, n, (hipStream_t)stream);
}

int adm_add_noise(const float* x0, long x0_bstride, const float* noise, const float* sa, const float* sb, int cb,
                  int cn, float* out, int B, int N, long P, void* stream) {
  ADM_REQUIRE(x0 && noise && sa && sb && out, "add_noise: null argument");
  return launch_add_noise(x0, x0_bstride, noise, sa, sb, cb, cn, out, B, N, P, (hipStream_t)stream);
}

int adm_dequant_u8(const float* x, uint8_t* out, long n, void* stream) {
  ADM_REQUIRE(x && out, "dequant: null argument");
  return launch_dequant(x, out, n, (hipStream_t)stream);
}

int adm_slerp_grid(const float* x0, const float* x1, long n, const double* alphas_dev, int n_alpha, float* out,
                   double* scratch3, void* stream) {
  ADM_REQUIRE(x0 && x1 && alphas_dev && out && scratch3 && n > 0 && n_alpha > 0, "slerp_grid: bad argument");
  return launch_slerp_grid(x0, x1, n, alphas_dev, n_alpha, out, scratch3, (hipStream_t)stream);
}

int adm_groupnorm_stats(const float* x1, int C1, const float* x2, int C2, int N, int HW, int groups, float eps,
                        const float* gamma, const float* beta, float* scale, float* shift, void* stream) {
  ADM_REQUIRE(x1 && gamma && beta && scale && shift, "groupnorm_stats: null argument");
  return launch_groupnorm_stats(x1, C1, x2, C2, N, HW, groups, eps, gamma, beta, scale, shift, (hipStream_t)stream);
}

// Test aids (adm_version() >= 107): the two launches of the timestep-embedding path, which the executors call with their own shapes only.
int adm_time_embedding(const float* t_dev, const float* freqs, int half_dim, int flip, const float* w1, const float* b1, const float* w2,
                       const float* b2, int dim_in, int dim_emb, float* emb, int B, float* save_sinus, float* save_z, float* emb_act,
                       void* stream) {
  ADM_REQUIRE(t_dev && freqs && w1 && b1 && w2 && b2 && emb, "time_embedding: null argument");
  ADM_REQUIRE(B > 0 && half_dim > 0 && dim_in == 2 * half_dim && dim_emb > 0, "time_embedding: dim_in = 2 * half_dim, B and dim_emb positive");
  return launch_time_embedding(t_dev, 1, nullptr, nullptr, freqs, half_dim, flip, w1, b1, w2, b2, dim_in, dim_emb, emb, B,
                               (hipStream_t)stream, save_sinus, save_z, emb_act);
}

int adm_temb_proj(const float* emb, const float* w, const float* bias, float* out, int B, int K, int R, int emb_is_activated,
                  void* stream) {
  ADM_REQUIRE(emb && w && bias && out, "temb_proj: null argument");
  ADM_REQUIRE(B > 0 && K > 0 && R > 0, "temb_proj: B, K and R positive");
  return launch_temb_proj(emb, w, bias, out, B, K, R, (hipStream_t)stream, emb_is_activated ? 1 : 0);
}

int adm_conv_stats_tiles(const adm_conv_args* a) { return a ? conv_stats_tiles(*a) : 0; }

int adm_groupnorm_finalize(const double* stats1, int C1, int tiles1, const double* stats2, int C2, int tiles2, int N, int HW,
                           int groups, float eps, const float* gamma, const float* beta, float* scale, float* shift,
                           void* stream) {
  ADM_REQUIRE(stats1 && gamma && beta && scale && shift, "groupnorm_finalize: null argument");
  return launch_groupnorm_finalize(stats1, C1, tiles1, stats2, C2, tiles2, N, HW, groups, eps, gamma, beta, scale, shift,
                                   (hipStream_t)stream);
}

int adm_conv2d(const adm_conv_args* a, void* stream) {
  ADM_REQUIRE(a && a->x1 && a->wpacked && a->out, "conv2d: null argument");
  return launch_conv2d(*a, (hipStream_t)stream);
}
// Test aid (adm_version() >= 120): adm_conv2d announced to the launchers the way the executors announce it when a GroupNorm reads `out` next.
int adm_conv2d_gn_finish(const adm_conv_args* a, const float* gamma, const float* beta, int groups, float eps, float* scale, float* shift,
                         int* taken, void* stream) {
  ADM_REQUIRE(a && a->x1 && a->wpacked && a->out && gamma && beta && scale && shift && groups > 0, "conv2d_gn_finish: null argument");
  const GnFuse f = {gamma, beta, eps, groups, scale, shift, nullptr};
  conv_gn_fuse_request(&f);
  const int rc = launch_conv2d(*a, (hipStream_t)stream);
  if (taken != nullptr) *taken = conv_gn_fuse_taken() ? 1 : 0;
  conv_gn_fuse_request(nullptr);
  return rc;
}

int adm_pack_conv_weight(const float* w, float* wpacked, int Cout, int Cin, int ks, void* stream) {
  ADM_REQUIRE(w && wpacked, "pack_conv_weight: null argument");
  return launch_pack_conv_weight(w, wpacked, Cout, Cin, ks, (hipStream_t)stream);
}

int adm_pack_conv_weight_T(const float* w, float* wpT, int Cout, int Cin, int ks, void* stream) {
  ADM_REQUIRE(w && wpT, "pack_conv_weight_T: null argument");
  return launch_pack_conv_weight_T(w, wpT, Cout, Cin, ks, (hipStream_t)stream);
}

long adm_winograd_packed_floats(int Cout, int Cin, int transposed) { return winograd_packed_floats(Cout, Cin, transposed); }
int adm_pack_winograd_weight(const float* w, float* wu, int Cout, int Cin, void* stream) {
  ADM_REQUIRE(w && wu, "pack_winograd_weight: null argument");
  return launch_pack_winograd_weight(w, wu, Cout, Cin, (hipStream_t)stream);
}

int adm_pack_winograd_weight_T(const float* w, float* wuT, int Cout, int Cin, void* stream) {
  ADM_REQUIRE(w && wuT, "pack_winograd_weight_T: null argument");
  return launch_pack_winograd_weight_T(w, wuT, Cout, Cin, (hipStream_t)stream);
}

int adm_pack_bf16_weight(const float* w, void* wb, int Cout, int Cin, int transposed, void* stream) {
  ADM_REQUIRE(w && wb, "pack_bf16_weight: null argument");
  return launch_pack_bf16_weight(w, wb, Cout, Cin, transposed, (hipStream_t)stream);
}

int adm_pack_bf16_weight_ks(const float* w, void* wb, int Cout, int Cin, int ks, int transposed, void* stream) {
  ADM_REQUIRE(w && wb, "pack_bf16_weight: null argument");
  return launch_pack_bf16_weight(w, wb, Cout, Cin, transposed, (hipStream_t)stream, ks);
}

void adm_conv_out_dims(int H, int W, int up, int stride, int ks, int pad_lo, int* Ho, int* Wo) {
  conv_out_dims(H, W, up, stride, ks, pad_lo, Ho, Wo);
}

int adm_attention(const float* qkv, float* out, int N, int C, int T, int head_dim, void* stream) {
  ADM_REQUIRE(qkv && out, "attention: null argument");
  return launch_attention(qkv, out, N, C, T, head_dim, (hipStream_t)stream);
}

int adm_layernorm_nct(const float* x, const float* gamma, const float* beta, float* y, int N, int C, long T, float eps,
                      void* stream) {
  ADM_REQUIRE(x && gamma && beta && y, "layernorm_nct: null argument");
  return launch_layernorm_nct(x, gamma, beta, y, N, C, T, eps, (hipStream_t)stream);
}
int adm_geglu(const float* in, float* out, int N, int C4, long T, void* stream) {
  ADM_REQUIRE(in && out, "geglu: null argument");
  return launch_geglu(in, out, N, C4, T, (hipStream_t)stream);
}
int adm_cross_attention(const float* q, const float* ctx, const float* Wk, const float* Wv, float* out, int N, int C, int T,
                        int S, int Dc, int head_dim, void* stream) {
  ADM_REQUIRE(q && ctx && Wk && Wv && out, "cross_attention: null argument");
  return launch_cross_attention(q, ctx, Wk, Wv, out, N, C, T, S, Dc, head_dim, (hipStream_t)stream);
}
int adm_attention_mfma_eligible(int C, int T, int head_dim) { return attention_mfma_eligible(C, T, head_dim) ? 1 : 0; }
int adm_attention_blocked(const float* qkv, float* out, int N, int C, int T, int head_dim, int key_block, void* stream) {
  ADM_REQUIRE(qkv && out, "attention_blocked: null argument");
  return launch_attention_blocked(qkv, out, N, C, T, head_dim, key_block, (hipStream_t)stream);
}

int adm_layernorm_nct_backward(const float* x, const float* dy, const float* gamma, float* dx, int accumulate, float* stats,
                               float* dgamma, float* dbeta, int N, int C, long T, float eps, void* stream) {
  ADM_REQUIRE(x && dy && gamma && dx && stats && dgamma && dbeta, "layernorm_nct_backward: null argument");
  return launch_layernorm_nct_bwd(x, dy, gamma, dx, accumulate, stats, dgamma, dbeta, N, C, T, eps, (hipStream_t)stream);
}
int adm_geglu_backward(const float* in, const float* dy, float* din, int N, int C4, long T, void* stream) {
  ADM_REQUIRE(in && dy && din, "geglu_backward: null argument");
  return launch_geglu_bwd(in, dy, din, N, C4, T, (hipStream_t)stream);
}
int adm_cross_attention_backward(const float* q, const float* ctx, const float* Wk, const float* Wv, const float* dy,
                                 float* dq, float* dWk, float* dWv, int N, int C, int T, int S, int Dc, int head_dim,
                                 void* stream) {
  ADM_REQUIRE(q && ctx && Wk && Wv && dy && dq && dWk && dWv, "cross_attention_backward: null argument");
  return launch_cross_attention_bwd(q, ctx, Wk, Wv, dy, dq, dWk, dWv, N, C, T, S, Dc, head_dim, (hipStream_t)stream);
}
int adm_attention_backward_blocked(const float* qkv, const float* dout, float* dqkv, float* stats, int N, int C, int T,
                                   int head_dim, int block, void* stream) {
  ADM_REQUIRE(qkv && dout && dqkv && stats, "attention_backward_blocked: null argument");
  return launch_attention_bwd_blocked(qkv, dout, dqkv, stats, N, C, T, head_dim, block, (hipStream_t)stream);
}
int adm_sepconv_block(const float* x, const float* dw, const float* pw, const float* pb, const float* bn_scale,
                      const float* bn_shift, float slope, float* tmp, float* y, int N, int Ci, int Co, int H, int W,
                      void* stream) {
  ADM_REQUIRE(x && dw && pw && pb && bn_scale && bn_shift && tmp && y, "sepconv_block: null argument");
  return launch_sepconv_block(x, dw, pw, pb, bn_scale, bn_shift, slope, tmp, y, N, Ci, Co, H, W, (hipStream_t)stream);
}
int adm_dense_act(const float* x, const float* W, const float* b, const float* post_scale, const float* post_shift,
                  float slope, int leaky, float* y, int N, int K, int J, int hwc_C, void* stream) {
  ADM_REQUIRE(x && W && b && y && ((post_scale == nullptr) == (post_shift == nullptr)), "dense_act: bad argument");
  return launch_dense_act(x, W, b, post_scale, post_shift, slope, leaky, y, N, K, J, hwc_C, (hipStream_t)stream);
}

}  // extern "C"
