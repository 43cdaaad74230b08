// k_sched_common.h — the small device helpers that every scheduler step kernel shares (k_sched.hip, k_unipc.hip): the x0 and noise
// predictions of the three model types, the guided and rescaled model output, the mask overwrite, the known-region overwrite (with
// add_noise's one expression, noisy_of), the u8 quantiser / packer and the launch geometry. ONE definition each, so that two translation units see the same bits.
#pragma once
#include "adm_kernels.h"

namespace adm {

// the x0 prediction: ONE helper for the step kernels and the selection, so that both see the same bits. o is the model output:
//   PRED_EPSILON  x0 = (x - sb*o) / sa      PRED_SAMPLE  x0 = o      PRED_V  x0 = sa*x - sb*o
// The v form is written as one product and one fused multiply-add, so that its bits depend on no contraction setting and on no
// inlining context (two products and a difference can be contracted two ways). At the zero-SNR row (sa = 0, sb = 1) it is -o exactly.
template <int PRED>
__device__ __forceinline__ float sched_x0(float x, float o, const adm_sched_coef& c) {
  if (PRED == PRED_SAMPLE) return o;
  if (PRED == PRED_V) return fmaf(c.sqrt_alpha, x, -__fmul_rn(c.sqrt_beta, o));
  return (x - c.sqrt_beta * o) / c.sqrt_alpha;
}

// the noise prediction that k_eps multiplies, from the x0 of sched_x0 BEFORE its clamp or threshold (diffusers does the same):
//   PRED_EPSILON  e = o      PRED_SAMPLE  e = (x - sa*x0) / sb      PRED_V  e = sa*o + sb*x
// At sa = 0, sb = 1 both new forms give e = x exactly. The sample form divides by sb: a row with sb = 0 (alphas_cumprod == 1, which only
// trained betas that start with zeros can make) is out of contract here and refused by the schedulers on the host.
template <int PRED>
__device__ __forceinline__ float sched_eps(float x, float o, float x0, const adm_sched_coef& c) {
  if (PRED == PRED_SAMPLE) return fmaf(-c.sqrt_alpha, x0, x) / c.sqrt_beta;
  if (PRED == PRED_V) return fmaf(c.sqrt_alpha, o, __fmul_rn(c.sqrt_beta, x));
  return o;
}

// classifier-free guidance: diffusers' `uncond + scale * (cond - uncond)` with its three separate roundings. ONE helper for the step
// body and the selection's key, so that both see the same bits. Plain operators under `fp contract(off)`, not __fadd_rn / __fmul_rn: hipcc's
// headers define those as `x + y` / `x * y` compiled under the default contraction, and once inlined the product and the sum fuse into
// fma(g, c - u, u), one rounding fewer than torch's. u == c gives u at any finite g.
__device__ __forceinline__ float sched_guided(float u, float c, float g) {
#pragma clang fp contract(off)
  const float d = c - u;
  const float gd = g * d;
  return u + gd;
}

// guidance rescale (include/adm.h): o' = phi*(o*r) + (1 - phi)*o with r the sample's std(c) / std(o) from guidance_stats_kernel. Three
// products and one sum, each rounded on its own, and 1 - phi formed in fp32: plain operators under `fp contract(off)` for sched_guided's
// reason. ONE helper for the step body and the selection's key, so that both see the same bits.
__device__ __forceinline__ float sched_rescaled(float o, float r, float phi) {
#pragma clang fp contract(off)
  const float om = 1.f - phi;
  const float a = o * r;
  const float b = phi * a;
  const float k = om * o;
  return b + k;
}
__device__ __forceinline__ float4 sched_guided4(const float4& u, const float4& c, float g) {
  return make_float4(sched_guided(u.x, c.x, g), sched_guided(u.y, c.y, g), sched_guided(u.z, c.z, g), sched_guided(u.w, c.w, g));
}
__device__ __forceinline__ float4 sched_rescaled4(const float4& o, float r, float phi) {
  return make_float4(sched_rescaled(o.x, r, phi), sched_rescaled(o.y, r, phi), sched_rescaled(o.z, r, phi), sched_rescaled(o.w, r, phi));
}

__device__ __forceinline__ unsigned char quant_u8(float v) {
  float q = fminf(fmaxf(v * 0.5f + 0.5f, 0.f), 1.f) * 255.f;
  return (unsigned char)rintf(q);  // round-half-even == numpy .round() (pipeline:194)
}

__device__ __forceinline__ unsigned pack_u8x4(float a, float b, float c, float d) {
  return (unsigned)quant_u8(a) | ((unsigned)quant_u8(b) << 8) | ((unsigned)quant_u8(c) << 16) | ((unsigned)quant_u8(d) << 24);
}

// The mask overwrite of the float4 r of `out` at float4 index i on row s: columns [0, mask_start) and [W - mask_end, W) take
// mask[b][s] (C == 1: the element index inside the sample is row*W + col). W % 4 == 0: a float4 never straddles two image rows.
__device__ __forceinline__ void sched_mask4(const SchedStepParams& p, int s, long i, float (&r)[4]) {
  const long e0 = i * 4;
  const long b = e0 / p.per_sample;
  const long q = e0 - b * p.per_sample;  // C == 1: q = row*W + col
  const int col0 = (int)(q % p.W);
  const float* mrow = p.mask + b * p.mask_bstride + (long)s * p.per_sample + q;
  ADM_UNROLL
  for (int k = 0; k < 4; ++k) {
    const int col = col0 + k;
    if (col < p.mask_start || col >= p.W - p.mask_end) r[k] = mrow[k];
  }
}

// sa*x0 + sb*noise: ONE expression for add_noise_kernel, noise_and_velocity_kernel (whose `noisy` must equal add_noise's bit for bit) and
// the known-region overwrite (sched_known4). Written out as what add_noise_kernel compiled to for gfx950 under the default contraction
// when it read `a * x + s * n`: the product s*n rounded on its own, then ONE fused multiply-add of a, x and that product (v_pk_mul_f32,
// v_pk_fma_f32). The product stands under `fp contract(off)` and feeds nothing but the fmaf, so the bits depend on no contraction setting
// and on no inlining context.
__device__ __forceinline__ float noisy_of(float a, float x, float s, float n) {
#pragma clang fp contract(off)
  const float sn = s * n;
  return fmaf(a, x, sn);
}

// The known-region overwrite (include/adm.h "Region in-painting") of the float4 r of `out` at float4 index i: every element whose keep
// byte is non-zero becomes noisy_of(ka, known, kb, known_noise), (ka, kb) the row's pair of known_table. keep is (Bm,H,W) bytes without a
// channel axis: the element index inside the sample, modulo H*W. One 32-bit word of keep per float4 (W % 4 == 0: a float4 never
// straddles an image row, a channel or a sample), and the two float4 loads only where that word is non-zero: +1 B/elem everywhere,
// +8 B/elem where kept.
__device__ __forceinline__ void sched_known4(const SchedStepParams& p, float ka, float kb, long i, float (&r)[4]) {
  const long e0 = i * 4;
  const long b = e0 / p.per_sample;
  const long q = e0 - b * p.per_sample;
  const unsigned kw = *reinterpret_cast<const unsigned*>(p.keep + b * p.keep_bstride + q % p.plane);
  if (kw == 0u) return;
  const float4 kv = *reinterpret_cast<const float4*>(p.known + b * p.known_bstride + q);
  const float4 nv = reinterpret_cast<const float4*>(p.known_noise)[i];
  if (kw & 0x000000ffu) r[0] = noisy_of(ka, kv.x, kb, nv.x);
  if (kw & 0x0000ff00u) r[1] = noisy_of(ka, kv.y, kb, nv.y);
  if (kw & 0x00ff0000u) r[2] = noisy_of(ka, kv.z, kb, nv.z);
  if (kw & 0xff000000u) r[3] = noisy_of(ka, kv.w, kb, nv.w);
}

// The known-region operands of a step (both launchers, after per_sample is derived): the refusals, each by the name of its field, and
// the two batch strides. keep == NULL: nothing to check, the other five fields are ignored.
static inline int sched_known_prepare(SchedStepParams& p) {
  if (p.keep == nullptr) return 0;
  ADM_REQUIRE(p.known != nullptr && p.known_noise != nullptr, "sched_step: keep needs known and known_noise");
  ADM_REQUIRE(p.known_table != nullptr, "sched_step: keep needs known_table (two floats per row of coef_table)");
  ADM_REQUIRE(p.mask == nullptr, "sched_step: keep and mask exclude each other (the known-region overwrite replaces the staged mask)");
  ADM_REQUIRE(p.B > 0 && p.per_sample > 0 && p.W % 4 == 0, "sched_step: W must be a multiple of 4");
  ADM_REQUIRE(((uintptr_t)p.keep & 3u) == 0 && ((uintptr_t)p.known & 15u) == 0 && ((uintptr_t)p.known_noise & 15u) == 0,
              "sched_step: keep must be 4-byte aligned, known and known_noise 16-byte aligned");
  p.plane = (long)p.H * p.W;
  p.known_bstride = p.known_batched ? p.per_sample : 0;
  p.keep_bstride = p.keep_batched ? p.plane : 0;
  return 0;
}

static inline int ew_grid(long n4) {
  long g = (n4 + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));  // cap + grid-stride (guide §6 G11)
}

}  // namespace adm
