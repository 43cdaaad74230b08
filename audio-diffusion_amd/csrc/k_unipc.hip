// k_unipc.hip — the fused UniPC predictor-corrector step (include/adm.h "UniPC" has THE definition; Zhao et al. 2023).
// One kernel per denoising step, unipc_step_kernel<PRED, THRESH, GUIDED>, 12 instantiations: per element
//   o   = the model output (GUIDED: sched_guided of the two outputs, sched_rescaled of that with p.guidance_rescale != 0)
//   m   = sched_x0<PRED>(x, o), THRESH: clamped to the sample's dynamic threshold s_b and divided by it (no static clip)
//   x_c = x, or with a corrector (u.c_t != 0):  u.c_x*last + u.c_t*m  (+ u.c_m1*m1) (+ u.c_m2*m2)
//   x'  = c.k_x0*m  (+ c.k_x*x_c where c.k_x != 0)  (+ u.p_m1*m1)
// with c the row's adm_sched_coef, u its adm_unipc_coef, m1 / m2 the data predictions of the two previous rows and `last` the corrected
// sample of the previous row. Both stages are linear, so the host folds every order, solver type and special level into the nine scalars.
// What is read follows the scalars and nothing else, because the first row of a run finds last and both history slots uninitialised
// (0 * NaN must not reach the output): last only where c_t != 0, m1 only where c_m1 != 0 || p_m1 != 0, m2 only where c_m2 != 0, and the
// k_x*x_c product is not formed on a row that ends at sigma = 0 (k_x == 0, x' = m). All four conditions are uniform over the grid.
// State: last = x_c is written in place (each lane reads then rewrites its own elements), hist is (2,B,C,H,W): row s reads m2 from slot
// s & 1 and then writes m into that same slot, and reads m1 from slot (s - 1) & 1; no history is ever copied. The mask overwrite and the
// known-region overwrite (p.keep != nullptr; k_sched.hip "KNOWN") go on `out` alone (the state is the solver's own), then the u8 pack; both are k_sched_common.h's, as are the model-output helpers, so the
// bits of m are those of the other step kernels and of the selection (sched_threshold_kernel, launched in front for THRESH).
// One float4 per lane per iteration, grid-stride, 256 lanes, the grid of sched_step_kernel. Algorithmic traffic on a full row (corrector
// of order 2): 20 B/elem read (x, o, last, m1, m2) + 12 B/elem written (out, last, m), +4 read when guided; the first row of a run
// reads 8 and writes 12. HBM-bound like the other steps: about 32/20 of the multistep step's time at size, launch-bound at 64 x 64.
// The guidance terms keep their separately rounded operations (sched_guided / sched_rescaled under `fp contract(off)`); the two linear
// stages are plain products and sums that the compiler may contract, as the other step bodies do.
#include "k_sched_common.h"
#include <cmath>

namespace adm {

template <int PRED, bool THRESH, bool GUIDED>
__device__ __forceinline__ void unipc_step_body(const SchedStepParams& p, const long first, const long stride) {
  const int s = p.step_dev ? *p.step_dev : p.step;
  const adm_sched_coef c = p.table[s];
  const adm_unipc_coef u = p.unipc_table[s];
  const bool corrected = u.c_t != 0.f;
  const bool use_m1 = u.c_m1 != 0.f || u.p_m1 != 0.f;
  const bool use_m2 = u.c_m2 != 0.f;
  const bool use_xc = c.k_x != 0.f;
  const bool rescaled = GUIDED && p.guidance_rescale != 0.f;
  const long n4s = p.per_sample >> 2;   // float4 per sample
  float4* hist_w = reinterpret_cast<float4*>(p.hist) + (long)(s & 1) * p.n4;              // m2 before the write, m after it
  const float4* hist_1 = reinterpret_cast<const float4*>(p.hist) + (long)((s & 1) ^ 1) * p.n4;   // m1 (slot (s - 1) & 1)
  unsigned char* u8 = p.u8_step >= 0 && s != p.u8_step ? nullptr : p.u8;
  const bool known = p.keep != nullptr;   // the known-region overwrite (k_sched.hip "KNOWN"): a kernel argument, uniform over the grid
  const float ka = known ? p.known_table[2 * s] : 0.f, kb = known ? p.known_table[2 * s + 1] : 0.f;
  for (long i = first; i < p.n4; i += stride) {
    const float4 xv = reinterpret_cast<const float4*>(p.x)[i];
    float4 ev = reinterpret_cast<const float4*>(p.eps)[i];
    long row = 0;   // the float4's sample (W % 4 == 0: a float4 never straddles two samples)
    if (rescaled || THRESH) row = i / n4s;
    if (GUIDED) {
      const float4 uv = reinterpret_cast<const float4*>(p.eps_uncond)[i];
      ev = sched_guided4(uv, ev, p.guidance);
      if (rescaled) ev = sched_rescaled4(ev, p.rescale[row], p.guidance_rescale);
    }
    float4 lv = make_float4(0.f, 0.f, 0.f, 0.f), h1 = lv, h2 = lv;
    if (corrected) lv = reinterpret_cast<const float4*>(p.last)[i];
    if (use_m1) h1 = hist_1[i];
    if (use_m2) h2 = hist_w[i];
    float th = 0.f;
    if (THRESH) th = p.scale[row];
    float4 mv, cv;   // this row's data prediction and corrected sample: the next rows' state
    auto one = [&](float x, float o, float xl, float m1, float m2, float& m, float& xc) {
      float x0 = sched_x0<PRED>(x, o, c);
      if (THRESH) x0 = fminf(fmaxf(x0, -th), th) / th;
      xc = x;
      if (corrected) {
        xc = u.c_x * xl + u.c_t * x0;
        if (use_m1) xc = xc + u.c_m1 * m1;
        if (use_m2) xc = xc + u.c_m2 * m2;
      }
      // (the expression of the multistep step, so that a row without a corrector contracts as that step's does)
      float prev = use_xc ? c.k_x0 * x0 + c.k_x * xc : c.k_x0 * x0;
      if (use_m1) prev = prev + u.p_m1 * m1;
      m = x0;
      return prev;
    };
    float r[4] = {one(xv.x, ev.x, lv.x, h1.x, h2.x, mv.x, cv.x), one(xv.y, ev.y, lv.y, h1.y, h2.y, mv.y, cv.y),
                  one(xv.z, ev.z, lv.z, h1.z, h2.z, mv.z, cv.z), one(xv.w, ev.w, lv.w, h1.w, h2.w, mv.w, cv.w)};
    hist_w[i] = mv;
    reinterpret_cast<float4*>(p.last)[i] = cv;
    if (p.mask != nullptr) sched_mask4(p, s, i, r);
    if (known) sched_known4(p, ka, kb, i, r);
    reinterpret_cast<float4*>(p.out)[i] = make_float4(r[0], r[1], r[2], r[3]);
    if (u8 != nullptr) reinterpret_cast<unsigned*>(u8)[i] = pack_u8x4(r[0], r[1], r[2], r[3]);
  }
}

template <int PRED, bool THRESH, bool GUIDED>
__global__ void __launch_bounds__(256) unipc_step_kernel(const SchedStepParams p) {
  unipc_step_body<PRED, THRESH, GUIDED>(p, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}

using UnipcKernel = void (*)(const SchedStepParams);
constexpr int unipc_slot(int pred, bool thresh, bool guided) { return (pred * 2 + thresh) * 2 + guided; }
static constexpr UnipcKernel kUnipcKernels[12] = {
    unipc_step_kernel<0, false, false>, unipc_step_kernel<0, false, true>, unipc_step_kernel<0, true, false>, unipc_step_kernel<0, true, true>,
    unipc_step_kernel<1, false, false>, unipc_step_kernel<1, false, true>, unipc_step_kernel<1, true, false>, unipc_step_kernel<1, true, true>,
    unipc_step_kernel<2, false, false>, unipc_step_kernel<2, false, true>, unipc_step_kernel<2, true, false>, unipc_step_kernel<2, true, true>};
static_assert(unipc_slot(PRED_V, true, true) == 11 && unipc_slot(PRED_SAMPLE, false, true) == 5, "slot function and table agree");

// THRESH: selection, then the step on the same stream: the selection has read x before an `out` that aliases x is written.
// guidance_rescale != 0: the statistics first (inside launch_sched_threshold for THRESH), so statistics, selection, step.
int launch_unipc_step(const SchedStepParams& in, int mode, hipStream_t st, int pred) {
  ADM_REQUIRE(mode == SCHED_PLAIN || mode == SCHED_THRESH,
              "sched_step: with unipc_table, mode must be 0 (x0 as predicted) or 1 (thresholded); 2 (the multistep step) is another step");
  ADM_REQUIRE(pred >= PRED_EPSILON && pred <= PRED_V, "sched_step: prediction must be 0 (epsilon), 1 (sample) or 2 (v_prediction)");
  SchedStepParams p = in;
  p.per_sample = (long)p.C * p.H * p.W;
  p.n4 = p.per_sample * p.B / 4;
  p.mask_bstride = (long)p.n_mask_steps * p.per_sample;
  const bool guided = p.eps_uncond != nullptr;
  ADM_REQUIRE(p.unipc_table != nullptr && p.last != nullptr && p.hist != nullptr,
              "sched_step: the UniPC step needs unipc_table, last and the two-slot hist");
  ADM_REQUIRE(p.noise == nullptr, "sched_step: noise must be NULL with unipc_table (the UniPC step has no noise rows)");
  ADM_REQUIRE(p.philox == 0, "sched_step: noise_source must be 0 with unipc_table (the UniPC step has no noise rows)");
  ADM_REQUIRE(p.B > 0 && p.per_sample > 0 && p.W % 4 == 0, "sched_step: W must be a multiple of 4");
  ADM_REQUIRE(p.mask == nullptr || p.C == 1, "sched_step: mask path requires C == 1 (as in the reference)");
  ADM_TRY(sched_known_prepare(p));
  if (guided) ADM_REQUIRE(std::isfinite(p.guidance), "sched_step: the guidance scale must be finite");
  if (mode == SCHED_THRESH) {
    ADM_REQUIRE(p.scale != nullptr, "sched_step: the thresholded step needs scale");
    ADM_TRY(launch_sched_threshold(p, st, pred, "sched_step"));
  } else {
    ADM_TRY(launch_guidance_stats(p, st, "sched_step"));
  }
  const UnipcKernel kernel = kUnipcKernels[unipc_slot(pred, mode == SCHED_THRESH, guided)];
  ADM_LAUNCH(kernel, dim3(ew_grid(p.n4)), dim3(256), 0, st, p);
  return ADM_CHECK_LAUNCH();
}

}  // namespace adm
