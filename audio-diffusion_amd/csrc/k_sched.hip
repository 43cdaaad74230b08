// k_sched.hip — fused scheduler epilogue, add_noise and u8 dequantisation (HBM-bound elementwise).
// Replaces DDIMScheduler.step / DDPMScheduler.step + mask overwrite + final dequant
// (reference: audiodiffusion/pipeline_audio_diffusion.py:165-185,192-194; SURVEY.md §8(a) S2-S4,P4,P5).
// One float4 per lane per iteration, grid-stride; algorithmic bytes: 12 B/elem (x, eps in; out), +4 with a noise BUFFER, +0 with noise
// drawn in the kernel (the noise stream below): a noisy step moves 12 B/elem instead of 16 (guided: 16 instead of 20).
// ONE step kernel, sched_step_kernel<MODE, PRED, GUIDED, PHILOX>: the loop, the noise slice, the mask overwrite and the u8 pack are shared,
// and each template parameter changes a handful of lines of sched_step_body:
//   MODE    SCHED_PLAIN      DDIM / DDPM with the row's static clamp.
//           SCHED_MULTISTEP  the second-order multistep solver (DPM-Solver++ 2M): the update is linear in (x, x0 of this step, x0 of the
//                            previous step), so it adds one per-step coefficient k_hist and one per-element history buffer that the same
//                            lane reads and rewrites in place: +8 B/elem over SCHED_PLAIN (one history read, one write), 20 B/elem in all.
//           SCHED_THRESH     sched_threshold_kernel first: dynamic thresholding (Imagen §2.3) of x0 in place of the static clamp. The
//                            per-sample percentile of |x0| is an exact order statistic: one workgroup per sample, MSB-first radix select
//                            (11 + 10 + 10 bits) over an LDS histogram of the bit pattern of |x0|; x0 is recomputed from x and eps in every
//                            pass (8 B/elem per pass, 3 passes + 1 when the two ranks straddle two distinct values: 24-32 B/elem,
//                            L2-resident), nothing but the B scales goes to global memory.
//   PRED    what the model predicts (PRED_EPSILON / PRED_SAMPLE / PRED_V), also a parameter of the selection's key. Same traffic: it only
//           changes the few flops that turn (x, model output) into (x0, eps).
//   GUIDED  classifier-free guidance, also a parameter of the selection's key: p.eps is the conditional model output c, p.eps_uncond the
//           unconditional one u, and o = sched_guided(u, c, g) stands wherever the model output stood. One more float4 load per lane:
//           16 B/elem where the unguided step moves 12 (+4 with a noise buffer, +8 with the multistep history); every pass of the
//           selection reads 12 B/elem instead of 8.
//   PHILOX  the noise source. Noise has three: none, a buffer (p.noise), and "adm noise stream 1" (include/adm.h): Philox4x32-10 keyed by
//           the seed and counted by (float4 index inside the sample, global sample row, timestep, stream id), turned into four normals by
//           two Box-Muller pairs, drawn by the lane that consumes them. noise_stream_normals is the ONE helper for randn_fill_kernel (the
//           initial latent, and what tests materialise) and for the step body. A template parameter, not a runtime branch: the
//           instantiations without it compile without a line of the generator. In the captured loop the key, the row offset and the
//           stream id are read from a 16-byte device block (p.nblock), as the step index is read from *step_dev, so a new seed or shard
//           offset replays the same graph; the eager entry point passes them by value (p.nvals).
//   RESCALE guidance rescale (Lin et al. 2023 §3.4; the arithmetic is defined in include/adm.h), NOT a template parameter: a runtime branch
//           inside the GUIDED instantiations on p.guidance_rescale != 0, a kernel argument and so uniform over the whole grid (no
//           divergence: a scalar compare and branch per float4). o' = sched_rescaled(o, r_b, phi) stands wherever o stood, in the step body
//           and in the selection's key, through that ONE helper. Why not a third value of GUIDED: it would double the 13 guided step and
//           the 3 guided selection instantiations for four flops per element in kernels that are bound by their 16 - 32 B/elem of traffic,
//           and the branch leaves the arithmetic of the unrescaled path untouched: sched_guided's three operations carry no contraction
//           flag, so what follows them fuses (or not) exactly as before whether o arrives directly or through the branch. With the
//           rescale on, the step reads 4 B more per SAMPLE (r_b), nothing more per element.
//           r_b comes from guidance_stats_kernel, launched before the selection and the step on the same stream: 8 B/elem read (c and u,
//           both just written by conv_out and L2 / Infinity-Cache resident), B floats written. One workgroup of 1024 lanes per sample,
//           as sched_threshold_kernel and with its trick of loads issued before use (two float4 pairs per lane, 64 KiB in flight per
//           workgroup): at 256 x 256 a sample is 512 KiB over the two buffers, 16 float4 pairs per lane, eight turns of the loop, ONE
//           sweep where the selection makes three or four of 12 B/elem. B workgroups leave most of the chip idle at B = 1, but a split
//           over several workgroups would need a second pass or a consumer that sums partials, for a sweep that is latency bound either
//           way and far shorter than the two forwards it follows (measured, profiles/guidance_rescale.md: 5.0 us at 64 x 64, B = 1, where
//           the selection beside it takes 10.3, and 9.2 us against 52.1 at 256 x 256, B = 16). The sums are fp64,
//           combined in a fixed order (lane, wave butterfly, LDS, one lane): no atomics and no global scratch, so r_b depends on neither
//           the batch, the order of execution nor earlier replays of a captured graph.
//   KNOWN   the known-region overwrite (region in-painting; the arithmetic is defined in include/adm.h), NOT a template parameter: a
//           runtime branch on p.keep != nullptr, a kernel argument and so uniform over the whole grid, for RESCALE's reason and as the
//           existing p.mask != nullptr: a template parameter would double the 26 step and the 12 UniPC instantiations for one load and
//           one compare per float4. After the history is written and before the store and the u8 pack, where the staged mask stands,
//           every element whose keep byte is non-zero becomes noisy_of(ka, known, kb, known_noise) with (ka, kb) = p.known_table[s]:
//           add_noise formed by the lane that writes the element, under an arbitrary (H,W) keep mask broadcast over the channels, at
//           any channel count and width, from three buffers whose size does not depend on the number of steps. sched_known4 and
//           noisy_of (k_sched_common.h) are the ONE definition for this file, k_unipc.hip and add_noise_kernel. Bytes: +1 B/elem
//           everywhere for the keep word (one 32-bit load per float4), +8 B/elem where kept (known and known_noise, loaded only where
//           the keep word is non-zero); with keep == nullptr nothing is read and the arithmetic above is untouched.
// 26 step instantiations are built: plain and thresholded for the three prediction types, guided or not, with the stream or not (24), and
// the multistep step for epsilon, guided or not (it has no noise rows); the 13 guided ones carry the rescaled form. The launchers look the
// kernel up in a table filled at compile time (kStepKernels by (mode, pred, guided, philox), kThresholdKernels by (pred, guided)); a
// combination that is not built is an empty slot and is refused.
// The small device helpers (sched_x0, sched_eps, sched_guided*, sched_rescaled*, the two overwrites, the u8 quantiser / packer) and the
// launch geometry live in k_sched_common.h: the UniPC step (k_unipc.hip, its own kernel template and launcher) shares them bit for bit.
#include "k_sched_common.h"
#include <array>
#include <cmath>
#include <utility>

namespace adm {

// ---- "adm noise stream 1" (include/adm.h) -----------------------------------------------------------------------------------------
// The high half of a 32 x 32 product, in plain C++ (the compiler picks v_mul_hi_u32; the emulator multiplies in 64 bits).
__device__ __forceinline__ uint32_t noise_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// Box-Muller on two 32-bit words: u1 = ((a >> 8) + 1) * 2^-24 in (0, 1], u2 = (b >> 8) * 2^-24 in [0, 1), both exact in fp32;
// (z0, z1) = sqrt(-2 ln u1) * (cos 2 pi u2, sin 2 pi u2). |z| <= sqrt(48 ln 2) < 5.77. Products only, each feeding a function or another
// product, under `fp contract(off)`: there is nothing to fuse, so the bits depend on no contraction setting and on no inlining context.
__device__ __forceinline__ void noise_box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
#pragma clang fp contract(off)
  const float u1 = (float)((a >> 8) + 1u) * 5.9604644775390625e-8f;
  const float u2 = (float)(b >> 8) * 5.9604644775390625e-8f;
  const float m = -2.f * logf(u1);
  const float r = sqrtf(m);
  const float th = 6.283185307179586f * u2;
  const float cs = cosf(th), sn = sinf(th);
  z0 = r * cs;
  z1 = r * sn;
}

// The four normals of elements 4q .. 4q+3 of global sample row `row` at integer timestep `t` of stream `sid`: Philox4x32-10 (Salmon et al.
// 2011) with key (k0, k1) = (seed & 0xffffffff, seed >> 32) on the counter (q, row, t, sid); (z0, z1) = BM(r0, r1), (z2, z3) = BM(r2, r3).
__device__ __forceinline__ float4 noise_stream_normals(uint32_t k0, uint32_t k1, uint32_t q, uint32_t row, uint32_t t, uint32_t sid) {
  uint32_t c0 = q, c1 = row, c2 = t, c3 = sid;
  ADM_UNROLL
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = noise_mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = noise_mulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  float4 z;
  noise_box_muller(c0, c1, z.x, z.y);
  noise_box_muller(c2, c3, z.z, z.w);
  return z;
}

// x0 of this step, then prev: the three modes differ in these lines only, and on purpose (an unconditional `+ k * 0` turns -0.0 into +0.0):
//   SCHED_PLAIN      x0 clamped to the row's c.clip (when >= 0);   prev = k_x0*x0 + k_x*x, += k_eps*eps, += k_noise*noise (noise 0 if unused)
//   SCHED_THRESH     x0 = clamp(x0, -s, s) / s with the sample's dynamic threshold s = scale[b] (c.clip is ignored); prev as SCHED_PLAIN
//   SCHED_MULTISTEP  m0 = x0 clamped as SCHED_PLAIN, m1 = x0 of the previous step from `hist`;
//                    prev = k_x0*m0 + k_x*x, += k_hist*m1 only where k_hist != 0, += k_noise*noise only where noise is used;
//                    hist = m0 (always, and before the mask: the history is the model's x0).
//                    hist is read ONLY where k_hist != 0: the first row of a run has k_hist == 0 and finds the buffer uninitialised
//                    (0 * NaN must not reach the output). Each lane reads and rewrites its own elements of hist.
// PRED: what p.eps holds (the model output o); e below is sched_eps of it, the model output itself for PRED_EPSILON.
// GUIDED: p.eps is the conditional output and o = sched_guided(p.eps_uncond, p.eps, p.guidance): in x0, in e and so in the history m0.
//   With p.guidance_rescale != 0 (uniform over the grid) o is replaced by sched_rescaled(o, p.rescale[b], p.guidance_rescale).
// PHILOX: the noise of a row with k_noise != 0 is noise_stream_normals of (q, row) = (i % (per_sample/4), row offset + i / (per_sample/4))
// at the row's integer timestep, and p.noise is not read; a row with k_noise == 0 draws nothing (the branch is uniform over the grid).
// out may alias x.
// first, stride: the lane's first float4 and the grid's stride, which the kernel works out itself (a launch-geometry builtin is only
// folded against the kernel's launch bounds where the kernel reads it).
template <int MODE, int PRED, bool GUIDED, bool PHILOX>
__device__ __forceinline__ void sched_step_body(const SchedStepParams& p, const long first, const long stride) {
  const int s = p.step_dev ? *p.step_dev : p.step;
  const adm_sched_coef c = p.table[s];
  const float k_hist = MODE == SCHED_MULTISTEP ? p.k_hist_table[s] : 0.f;
  const bool use_hist = k_hist != 0.f;
  const bool use_noise = (PHILOX || p.noise != nullptr) && c.k_noise != 0.f;
  uint32_t nk0 = 0, nk1 = 0, nrow0 = 0, nsid = 0, nt = 0;
  const long n4s = p.per_sample >> 2;   // float4 per sample
  const bool rescaled = GUIDED && p.guidance_rescale != 0.f;
  if (PHILOX) {
    nk0 = p.nblock ? p.nblock[0] : p.nvals[0]; nk1 = p.nblock ? p.nblock[1] : p.nvals[1];
    nrow0 = p.nblock ? p.nblock[2] : p.nvals[2]; nsid = p.nblock ? p.nblock[3] : p.nvals[3];
    nt = (uint32_t)(int)c.timestep;
  }
  const float* noise = p.noise + (long)s * p.noise_step_stride;  // per-step slice of a (n_steps,B,C,H,W) noise tensor (0: single step)
  unsigned char* u8 = p.u8_step >= 0 && s != p.u8_step ? nullptr : p.u8;
  const bool known = p.keep != nullptr;   // KNOWN (a kernel argument: uniform over the grid)
  const float ka = known ? p.known_table[2 * s] : 0.f, kb = known ? p.known_table[2 * s + 1] : 0.f;
  for (long i = first; i < p.n4; i += stride) {
    const float4 xv = reinterpret_cast<const float4*>(p.x)[i];
    float4 ev = reinterpret_cast<const float4*>(p.eps)[i];
    long row = 0;   // the float4's sample: one division, shared by the rescale factor and the noise stream's counter
    if (rescaled || (PHILOX && use_noise)) row = i / n4s;
    if (GUIDED) {
      const float4 uv = reinterpret_cast<const float4*>(p.eps_uncond)[i];
      ev = sched_guided4(uv, ev, p.guidance);
      if (rescaled) ev = sched_rescaled4(ev, p.rescale[row], p.guidance_rescale);   // W % 4 == 0: a float4 never straddles two samples
    }
    float4 nv = make_float4(0.f, 0.f, 0.f, 0.f), hv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (PHILOX) {
      if (use_noise) {
        nv = noise_stream_normals(nk0, nk1, (uint32_t)(i - row * n4s), nrow0 + (uint32_t)row, nt, nsid);
      }
    } else if (use_noise) nv = reinterpret_cast<const float4*>(noise)[i];
    if (use_hist) hv = reinterpret_cast<const float4*>(p.hist)[i];
    float th = 0.f;
    if (MODE == SCHED_THRESH) th = p.scale[(i * 4) / p.per_sample];  // W % 4 == 0: a float4 never straddles two samples
    float4 mv;  // x0 of this step, clamped: the next step's history
    auto one = [&](float x, float o, float nz, float h, float& m0) {
      float x0 = sched_x0<PRED>(x, o, c);
      const float e = sched_eps<PRED>(x, o, x0, c);
      if (MODE == SCHED_THRESH) x0 = fminf(fmaxf(x0, -th), th) / th;
      else if (c.clip >= 0.f) x0 = fminf(fmaxf(x0, -c.clip), c.clip);
      float prev = c.k_x0 * x0 + c.k_x * x;
      if (MODE == SCHED_MULTISTEP) {
        if (use_hist) prev = prev + k_hist * h;
        if (use_noise) prev = prev + c.k_noise * nz;
      } else {
        prev = prev + c.k_eps * e;
        prev = prev + c.k_noise * nz;
      }
      m0 = x0;
      return prev;
    };
    float r[4] = {one(xv.x, ev.x, nv.x, hv.x, mv.x), one(xv.y, ev.y, nv.y, hv.y, mv.y), one(xv.z, ev.z, nv.z, hv.z, mv.z),
                  one(xv.w, ev.w, nv.w, hv.w, mv.w)};
    if (MODE == SCHED_MULTISTEP) reinterpret_cast<float4*>(p.hist)[i] = mv;
    if (p.mask != nullptr) sched_mask4(p, s, i, r);
    if (known) sched_known4(p, ka, kb, i, r);
    reinterpret_cast<float4*>(p.out)[i] = make_float4(r[0], r[1], r[2], r[3]);
    if (u8 != nullptr) reinterpret_cast<unsigned*>(u8)[i] = pack_u8x4(r[0], r[1], r[2], r[3]);
  }
}

template <int MODE, int PRED, bool GUIDED, bool PHILOX>
__global__ void __launch_bounds__(256) sched_step_kernel(const SchedStepParams p) {
  static_assert(MODE != SCHED_MULTISTEP || PRED == PRED_EPSILON, "the multistep step is epsilon only");
  static_assert(MODE != SCHED_MULTISTEP || !PHILOX, "the multistep step has no noise rows");
  sched_step_body<MODE, PRED, GUIDED, PHILOX>(p, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}

// (B, per_sample) normals of the stream at one (t, stream id): out[b][4q .. 4q+3] = noise_stream_normals(q, row_offset + b). One float4 per lane.
__global__ void __launch_bounds__(256) randn_fill_kernel(float* __restrict__ out, long n4, long n4s, uint32_t k0, uint32_t k1,
                                                         uint32_t row0, uint32_t t, uint32_t sid) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const long row = i / n4s;
    reinterpret_cast<float4*>(out)[i] = noise_stream_normals(k0, k1, (uint32_t)(i - row * n4s), row0 + (uint32_t)row, t, sid);
  }
}

// ---- dynamic threshold: exact per-sample order statistics of |x0| ---------------------------------------------------------------------
// Key = bit pattern of |x0| (non-negative floats order as unsigned integers; -0.0 becomes 0; NaN patterns order last). Three passes select
// the key of rank lo digit by digit, most significant first: each pass histograms, in LDS, one digit of the keys that match the digits
// found so far, and wave 0 locates the bin that holds the rank. After the last pass the bin is the run of elements equal to a = v[lo]; if
// rank hi still falls inside that run b = a, otherwise b is the smallest key above a (one more sweep). Integer counts only, one workgroup
// per sample and no global scratch: nothing to reset between replays, and a sample's result cannot depend on its batch.
constexpr int kThreshThreads = 1024, kThreshBins = 2048;

template <int PRED>
__device__ __forceinline__ unsigned thresh_key(float x, float e, const adm_sched_coef& c) {
  return __float_as_uint(sched_x0<PRED>(x, e, c)) & 0x7fffffffu;
}

__device__ __forceinline__ float thresh_bits_to_float(unsigned u) {
  float f;
  __builtin_memcpy(&f, &u, sizeof(f));
  return f;
}

// One sweep of a sample: f(key) for the key of every element. Four float4 pairs (GUIDED: triples) per lane are loaded before any is used:
// with one workgroup per sample (a single CU when B = 1) the sweep is bound by load latency, not by bandwidth.
// GUIDED: up is the unconditional output and the key is |x0| of sched_guided(up, ep, g), the step body's own combination; with phi != 0
// (uniform over the workgroup) of sched_rescaled(that, r, phi), r the sample's rescale factor.
template <int PRED, bool GUIDED, class F>
__device__ __forceinline__ void thresh_sweep(const float4* __restrict__ xp, const float4* __restrict__ ep, const float4* __restrict__ up,
                                             float g, float r, float phi, int n4, int tid, const adm_sched_coef& c, F f) {
  for (int i0 = tid; i0 < n4; i0 += 4 * kThreshThreads) {
    float4 xv[4], ev[4], uv[4];
    ADM_UNROLL
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * kThreshThreads;
      if (i < n4) {
        xv[u] = xp[i]; ev[u] = ep[i];
        if (GUIDED) uv[u] = up[i];
      }
    }
    ADM_UNROLL
    for (int u = 0; u < 4; ++u) {
      if (i0 + u * kThreshThreads < n4) {
        if (GUIDED) {
          ev[u] = sched_guided4(uv[u], ev[u], g);
          if (phi != 0.f) ev[u] = sched_rescaled4(ev[u], r, phi);
        }
        f(thresh_key<PRED>(xv[u].x, ev[u].x, c)); f(thresh_key<PRED>(xv[u].y, ev[u].y, c));
        f(thresh_key<PRED>(xv[u].z, ev[u].z, c)); f(thresh_key<PRED>(xv[u].w, ev[u].w, c));
      }
    }
  }
}

// Wave 0, all 64 lanes: the bin of hist[0..nbins) that holds rank k of the counted keys -> sel = {bin, rank inside the bin, bin count}.
__device__ __forceinline__ void thresh_find_bin(const unsigned* hist, int nbins, unsigned k, unsigned* sel) {
  const int lane = threadIdx.x & 63, per = nbins >> 6;
  unsigned sum = 0;
  for (int j = 0; j < per; ++j) sum += hist[lane * per + j];
  unsigned inc = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned t = __shfl(inc, (lane - d) & 63, 64);
    if (lane >= d) inc += t;
  }
  const unsigned exc = inc - sum;
  if (k >= exc && k < inc) {  // exactly one lane (the caller keeps k below the number of counted keys)
    unsigned r = k - exc;
    for (int j = 0; j < per; ++j) {
      const unsigned cnt = hist[lane * per + j];
      if (r < cnt) { sel[0] = (unsigned)(lane * per + j); sel[1] = r; sel[2] = cnt; break; }
      r -= cnt;
    }
  }
}

template <int PRED, bool GUIDED>
__device__ __forceinline__ void sched_threshold_body(
    const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ eps_uncond, float guidance,
    const float* __restrict__ rescale, float phi, const adm_sched_coef* __restrict__ table,
    const int* __restrict__ step_dev, int step, long per_sample, unsigned lo, unsigned hi, float w, float max_value,
    float* __restrict__ scale) {
  __shared__ unsigned hist[kThreshBins];
  __shared__ unsigned sel[3];
  const adm_sched_coef c = table[step_dev ? *step_dev : step];
  const float4* xp = reinterpret_cast<const float4*>(x + (long)blockIdx.x * per_sample);
  const float4* ep = reinterpret_cast<const float4*>(eps + (long)blockIdx.x * per_sample);
  const float4* uq = GUIDED ? reinterpret_cast<const float4*>(eps_uncond + (long)blockIdx.x * per_sample) : nullptr;
  const int n4 = (int)(per_sample >> 2);
  const int tid = threadIdx.x;
  if (!GUIDED) phi = 0.f;
  const float rs = phi != 0.f ? rescale[blockIdx.x] : 1.f;
  if (tid < 3) sel[tid] = 0;
  unsigned prefix = 0, k = lo, run = 0;
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);   // digits: bits 30..20, 19..10, 9..0
    const int nbins = pass == 0 ? kThreshBins : 1024;
    const int up = pass == 0 ? 31 : shift + 10;                // the digits above this one are fixed by `prefix`
    for (int j = tid; j < nbins; j += kThreshThreads) hist[j] = 0;
    __syncthreads();
    thresh_sweep<PRED, GUIDED>(xp, ep, uq, guidance, rs, phi, n4, tid, c, [&](unsigned key) {
      if ((key >> up) == (prefix >> up)) atomicAdd(&hist[(key >> shift) & (unsigned)(nbins - 1)], 1u);
    });
    __syncthreads();
    if (tid < 64) thresh_find_bin(hist, nbins, k, sel);
    __syncthreads();
    prefix |= sel[0] << shift;
    k = sel[1];
    run = sel[2];
  }
  // prefix = key of a = v[lo]; k = position of rank lo inside the run of `run` elements equal to a
  unsigned key_b = prefix;
  if (hi > lo && k + 1 >= run) {  // (uniform over the workgroup) rank hi lies past the run: b = the smallest key above a
    if (tid == 0) hist[0] = 0;
    __syncthreads();
    unsigned m = 0xffffffffu;
    thresh_sweep<PRED, GUIDED>(xp, ep, uq, guidance, rs, phi, n4, tid, c, [&](unsigned key) {
      if (key > prefix && key < m) m = key;
    });
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned t = __shfl_xor(m, d, 64);
      m = t < m ? t : m;
    }
    if ((tid & 63) == 0) atomicMax(&hist[0], ~m);   // min as the max of the complement: integer, order-independent
    __syncthreads();
    if (hist[0] != 0) key_b = ~hist[0];             // (0: no key above a, which hi <= n - 1 excludes; b stays a)
  }
  if (tid == 0) {
    // torch.quantile's linear interpolation is torch's CPU lerp, whose multiply-add is FUSED (one rounding; measured: 20000 of 20000
    // random (a, b, w) agree with the fused form, 92 % with separately rounded operations). The difference and 1 - w are rounded on
    // their own; fmaf is written out so that the result depends on no contraction setting.
    const float a = thresh_bits_to_float(prefix), b = thresh_bits_to_float(key_b);
    const float d = __fadd_rn(b, -a);
    const float q = w < 0.5f ? fmaf(w, d, a) : fmaf(-d, __fadd_rn(1.f, -w), b);
    scale[blockIdx.x] = fminf(fmaxf(q, 1.f), max_value);
  }
}

// One signature for the six instantiations; the unguided ones ignore eps_uncond, guidance, rescale and phi, as the body does.
template <int PRED, bool GUIDED>
__global__ void __launch_bounds__(kThreshThreads) sched_threshold_kernel(
    const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ eps_uncond, float guidance,
    const float* __restrict__ rescale, float phi, const adm_sched_coef* __restrict__ table, const int* __restrict__ step_dev, int step,
    long per_sample, unsigned lo, unsigned hi, float w, float max_value, float* __restrict__ scale) {
  sched_threshold_body<PRED, GUIDED>(x, eps, eps_uncond, guidance, rescale, phi, table, step_dev, step, per_sample, lo, hi, w, max_value,
                                     scale);
}

// ---- guidance rescale: the per-sample factor r_b = std(c_b) / std(o_b) (include/adm.h) ---------------------------------------------------
// One workgroup per sample. Both standard deviations come from one sweep of fp64 sums of d and d*d, d = v - v[first element of the sample]:
// the shift by the sample's own first element makes a constant sample give 0 exactly (every d is 0) and takes the mean out of the
// cancellation in S2 - S1*S1/n, and it depends on the sample alone. d is exact in fp64 unless the two exponents lie more than 29 binades
// apart, and then off by 2^-53 relative. The eight partial sums are combined in a fixed order: the lane's own elements in index order,
// a __shfl_xor butterfly over the wave, one LDS slot per wave, and lane 0 adding the 16 slots in wave order. No atomics, no global scratch.
constexpr int kStatsThreads = 1024, kStatsLoads = 2;   // float4 pairs (c, u) in flight per lane: 64 KiB per workgroup

__global__ void __launch_bounds__(kStatsThreads) guidance_stats_kernel(const float* __restrict__ eps, const float* __restrict__ eps_uncond,
                                                                       float g, long per_sample, float* __restrict__ rescale) {
  __shared__ double red[4][kStatsThreads / 64];
  const float4* cp = reinterpret_cast<const float4*>(eps + (long)blockIdx.x * per_sample);
  const float4* up = reinterpret_cast<const float4*>(eps_uncond + (long)blockIdx.x * per_sample);
  const int n4 = (int)(per_sample >> 2);
  const int tid = threadIdx.x;
  const float c0 = eps[(long)blockIdx.x * per_sample];
  const float o0 = sched_guided(eps_uncond[(long)blockIdx.x * per_sample], c0, g);
  double s[4] = {0.0, 0.0, 0.0, 0.0};   // sum dc, sum dc^2, sum do, sum do^2
  auto add = [&](float c, float u) {
    const double dc = (double)c - (double)c0, dv = (double)sched_guided(u, c, g) - (double)o0;
    s[0] += dc; s[1] += dc * dc; s[2] += dv; s[3] += dv * dv;
  };
  for (int i0 = tid; i0 < n4; i0 += kStatsLoads * kStatsThreads) {
    float4 cv[kStatsLoads], uv[kStatsLoads];
    ADM_UNROLL
    for (int k = 0; k < kStatsLoads; ++k) {
      const int i = i0 + k * kStatsThreads;
      if (i < n4) { cv[k] = cp[i]; uv[k] = up[i]; }
    }
    ADM_UNROLL
    for (int k = 0; k < kStatsLoads; ++k) {
      if (i0 + k * kStatsThreads < n4) {
        add(cv[k].x, uv[k].x); add(cv[k].y, uv[k].y); add(cv[k].z, uv[k].z); add(cv[k].w, uv[k].w);
      }
    }
  }
  ADM_UNROLL
  for (int j = 0; j < 4; ++j)
    for (int m = 32; m >= 1; m >>= 1) s[j] += __shfl_xor(s[j], m, 64);
  if ((tid & 63) == 0) {
    ADM_UNROLL
    for (int j = 0; j < 4; ++j) red[j][tid >> 6] = s[j];
  }
  __syncthreads();
  if (tid == 0) {
    double t[4];
    ADM_UNROLL
    for (int j = 0; j < 4; ++j) {
      t[j] = red[j][0];
      for (int wv = 1; wv < kStatsThreads / 64; ++wv) t[j] += red[j][wv];
    }
    const double n = (double)per_sample;
    const double var_c = (t[1] - t[0] * t[0] / n) / (n - 1.0), var_o = (t[3] - t[2] * t[2] / n) / (n - 1.0);   // unbiased, as torch.std
    const float std_c = (float)sqrt(var_c > 0.0 ? var_c : (var_c == var_c ? 0.0 : var_c));   // (a rounding below zero is zero; NaN stays)
    const float std_o = (float)sqrt(var_o > 0.0 ? var_o : (var_o == var_o ? 0.0 : var_o));
    const bool ok = std_o != 0.f && std_c - std_c == 0.f && std_o - std_o == 0.f;   // x - x == 0: x is finite
    rescale[blockIdx.x] = ok ? __fdiv_rn(std_c, std_o) : 1.f;
  }
}

__global__ void step_advance_kernel(int* step_dev) { *step_dev += 1; }

// DDIM inversion update (pipeline_audio_diffusion.py:238-240), in place, for the three prediction types (include/adm.h "DDIM inversion"
// names the fields of a row). PRED changes one line: e, the noise prediction, is sched_eps of the model output at the level the model
// was given, (sa_c, sb_c) = (k_x, k_noise) of the row; the epsilon instantiation reads neither and keeps the reference's two expressions
// and their rounding order. 12 B/elem: x and the model output in, x out.
template <int PRED>
__global__ void __launch_bounds__(256) encode_step_kernel(float* x, const float* __restrict__ eps,
                                                          const adm_sched_coef* __restrict__ table,
                                                          const int* __restrict__ step_dev, int step, long n4) {
  const adm_sched_coef c = table[step_dev ? *step_dev : step];
  adm_sched_coef cc = c;   // the row as sched_eps reads it: the conversion pair where a sampling row has (sa, sb)
  cc.sqrt_alpha = c.k_x; cc.sqrt_beta = c.k_noise;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 xv = reinterpret_cast<const float4*>(x)[i];
    const float4 ev = reinterpret_cast<const float4*>(eps)[i];
    float* xs = reinterpret_cast<float*>(&xv);
    const float* es = reinterpret_cast<const float*>(&ev);
    ADM_UNROLL
    for (int k = 0; k < 4; ++k) {
      const float e = sched_eps<PRED>(xs[k], es[k], es[k], cc);   // (a sample model's output is its x0)
      float s = (xs[k] - c.sqrt_beta * e) * c.sqrt_alpha;
      xs[k] = s * c.k_x0 + c.k_eps * e;
    }
    reinterpret_cast<float4*>(x)[i] = xv;
  }
}

// (sa*x0 + sb*noise is noisy_of, k_sched_common.h: ONE expression for the two kernels below and the known-region overwrite of the step)
__global__ void __launch_bounds__(256) add_noise_kernel(const float* __restrict__ x0, long x0_bstride,
                                                        const float* __restrict__ noise,
                                                        const float* __restrict__ sa, const float* __restrict__ sb,
                                                        int cb, int cn, float* __restrict__ out, int N, long P4) {
  const int b = blockIdx.z, n = blockIdx.y;
  const float a = sa[b * cb + n * cn], s = sb[b * cb + n * cn];
  const float4* xp = reinterpret_cast<const float4*>(x0 + (long)b * x0_bstride);
  const float4* np = reinterpret_cast<const float4*>(noise) + (long)b * P4;
  float4* op = reinterpret_cast<float4*>(out) + ((long)b * N + n) * P4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < P4; i += (long)gridDim.x * blockDim.x) {
    const float4 xv = xp[i], nv = np[i];
    op[i] = make_float4(noisy_of(a, xv.x, s, nv.x), noisy_of(a, xv.y, s, nv.y), noisy_of(a, xv.z, s, nv.z), noisy_of(a, xv.w, s, nv.w));
  }
}

// Training prologue of a v-model: per sample b, noisy = sa[b]*x0 + sb[b]*noise (add_noise's per-sample form) and the regression target
// velocity = sa[b]*noise - sb[b]*x0, from one read of x0 and noise: 16 B/elem where two add_noise passes would move 24.
__global__ void __launch_bounds__(256) noise_and_velocity_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                                 const float* __restrict__ sa, const float* __restrict__ sb,
                                                                 float* __restrict__ noisy, float* __restrict__ velocity, long P4) {
  const int b = blockIdx.y;
  const float a = sa[b], s = sb[b];
  const float4* xp = reinterpret_cast<const float4*>(x0) + (long)b * P4;
  const float4* np = reinterpret_cast<const float4*>(noise) + (long)b * P4;
  float4* yp = reinterpret_cast<float4*>(noisy) + (long)b * P4;
  float4* vp = reinterpret_cast<float4*>(velocity) + (long)b * P4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < P4; i += (long)gridDim.x * blockDim.x) {
    const float4 xv = xp[i], nv = np[i];
    yp[i] = make_float4(noisy_of(a, xv.x, s, nv.x), noisy_of(a, xv.y, s, nv.y), noisy_of(a, xv.z, s, nv.z), noisy_of(a, xv.w, s, nv.w));
    vp[i] = make_float4(a * nv.x - s * xv.x, a * nv.y - s * xv.y, a * nv.z - s * xv.z, a * nv.w - s * xv.w);
  }
}

__global__ void __launch_bounds__(256) dequant_kernel(const float* __restrict__ x, unsigned char* __restrict__ out,
                                                      long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    reinterpret_cast<unsigned*>(out)[i] = pack_u8x4(v.x, v.y, v.z, v.w);
  }
}

// The kernel tables. A slot is a kernel's address, or nullptr for a combination that is not built: the helper keeps those from being
// instantiated (their static_asserts would fire).
using StepKernel = void (*)(const SchedStepParams);
using ThresholdKernel = void (*)(const float*, const float*, const float*, float, const float*, float, const adm_sched_coef*, const int*,
                                 int, long, unsigned, unsigned, float, float, float*);

template <int MODE, int PRED, bool GUIDED, bool PHILOX>
constexpr StepKernel step_kernel_or_null() {
  if constexpr (MODE == SCHED_MULTISTEP && (PRED != PRED_EPSILON || PHILOX)) return nullptr;
  else return sched_step_kernel<MODE, PRED, GUIDED, PHILOX>;
}

constexpr int step_slot(int mode, int pred, bool guided, bool philox) { return ((mode * 3 + pred) * 2 + guided) * 2 + philox; }
constexpr int threshold_slot(int pred, bool guided) { return pred * 2 + guided; }

template <size_t... I>
constexpr std::array<StepKernel, sizeof...(I)> step_kernel_table(std::index_sequence<I...>) {
  return {{step_kernel_or_null<I / 12, I / 4 % 3, (I / 2 % 2) != 0, (I % 2) != 0>()...}};
}
template <size_t... I>
constexpr std::array<ThresholdKernel, sizeof...(I)> threshold_kernel_table(std::index_sequence<I...>) {
  return {{sched_threshold_kernel<I / 2, (I % 2) != 0>...}};
}
static constexpr auto kStepKernels = step_kernel_table(std::make_index_sequence<3 * 3 * 2 * 2>{});
static constexpr auto kThresholdKernels = threshold_kernel_table(std::make_index_sequence<3 * 2>{});
static_assert(step_slot(SCHED_MULTISTEP, PRED_V, true, true) == 35 && threshold_slot(PRED_V, true) == 5, "slot functions and tables agree");

// guidance rescale on (p.guidance_rescale != 0): writes the B factors r_b to p.rescale; before the selection and the step, on their stream
int launch_guidance_stats(const SchedStepParams& p, hipStream_t st, const char* who) {
  const long per_sample = (long)p.C * p.H * p.W;
  ADM_REQUIRE(std::isfinite(p.guidance_rescale) && p.guidance_rescale >= 0.f && p.guidance_rescale <= 1.f,
              std::string(who) + ": guidance_rescale must be in [0, 1]");
  if (p.guidance_rescale == 0.f) return 0;
  ADM_REQUIRE(p.eps_uncond != nullptr, std::string(who) + ": guidance_rescale needs eps_uncond (it rescales the guided output)");
  ADM_REQUIRE(p.rescale != nullptr, std::string(who) + ": guidance_rescale needs the rescale buffer");
  ADM_REQUIRE(std::isfinite(p.guidance), std::string(who) + ": the guidance scale must be finite");
  ADM_REQUIRE(p.B > 0 && p.W % 4 == 0, std::string(who) + ": W must be a multiple of 4");
  ADM_REQUIRE(per_sample > 0 && per_sample < (1L << 31), std::string(who) + ": C*H*W must be below 2^31");
  ADM_LAUNCH(guidance_stats_kernel, dim3(p.B), dim3(kStatsThreads), 0, st, p.eps, p.eps_uncond, p.guidance, per_sample, p.rescale);
  return ADM_CHECK_LAUNCH();
}

// reads p's x, eps, eps_uncond, guidance, guidance_rescale, table, step_dev, step, the ranks and the shape; writes the B thresholds to
// p.scale (and, with guidance_rescale != 0, the B factors to p.rescale first)
int launch_sched_threshold(const SchedStepParams& p, hipStream_t st, int pred, const char* who) {
  const long per_sample = (long)p.C * p.H * p.W;
  const bool guided = p.eps_uncond != nullptr;
  ADM_REQUIRE(p.B > 0 && p.W % 4 == 0, "sched_threshold: W must be a multiple of 4");
  ADM_REQUIRE(per_sample > 0 && per_sample < (1L << 31), "sched_threshold: C*H*W must be below 2^31");
  ADM_REQUIRE(p.lo >= 0 && p.hi >= p.lo && p.hi - p.lo <= 1 && p.hi < per_sample,
              "sched_threshold: need 0 <= lo <= hi <= C*H*W - 1 and hi - lo <= 1");
  ADM_REQUIRE(p.w >= 0.f && p.w < 1.f, "sched_threshold: the interpolation weight must be in [0, 1)");
  ADM_REQUIRE(p.max_value >= 1.f, "sched_threshold: max_value must be >= 1");
  ADM_REQUIRE(pred >= PRED_EPSILON && pred <= PRED_V, "sched_threshold: prediction must be 0 (epsilon), 1 (sample) or 2 (v_prediction)");
  if (guided) ADM_REQUIRE(std::isfinite(p.guidance), "sched_threshold: the guidance scale must be finite");
  ADM_TRY(launch_guidance_stats(p, st, who));   // (its refusals carry the entry point's name: the thresholded step passes its own)
  const ThresholdKernel kernel = kThresholdKernels[threshold_slot(pred, guided)];
  ADM_LAUNCH(kernel, dim3(p.B), dim3(kThreshThreads), 0, st, p.x, p.eps, p.eps_uncond, p.guidance, p.rescale, p.guidance_rescale, p.table,
             p.step_dev, p.step, per_sample, (unsigned)p.lo, (unsigned)p.hi, p.w, p.max_value, p.scale);
  return ADM_CHECK_LAUNCH();
}

int launch_randn(float* out, int B, long per_sample, uint64_t seed, int row_offset, int t, int noise_stream, hipStream_t st) {
  ADM_REQUIRE(out != nullptr && B > 0, "randn: null output or B <= 0");
  ADM_REQUIRE(per_sample > 0 && per_sample % 4 == 0, "randn: per_sample must be a positive multiple of 4");
  ADM_REQUIRE(per_sample / 4 <= 0xffffffffL, "randn: per_sample / 4 must fit in 32 bits (the counter's first word)");
  ADM_REQUIRE(row_offset >= 0, "randn: row_offset must be >= 0");
  ADM_REQUIRE((uint64_t)row_offset + (uint64_t)B <= 0xffffffffull, "randn: row_offset + B must fit in 32 bits");
  ADM_REQUIRE(t >= 0, "randn: the timestep must be in [0, 2^31)");
  ADM_REQUIRE(noise_stream == 0 || noise_stream == 1, "randn: noise_stream must be 0 (step noise) or 1 (initial latent); 2 and 3 are reserved");
  const long n4s = per_sample / 4, n4 = n4s * B;
  ADM_LAUNCH(randn_fill_kernel, dim3(ew_grid(n4)), dim3(256), 0, st, out, n4, n4s, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32),
             (uint32_t)row_offset, (uint32_t)t, (uint32_t)noise_stream);
  return ADM_CHECK_LAUNCH();
}

// SCHED_THRESH: selection, then the step on the same stream: the selection has read x before an `out` that aliases x is written.
// guidance_rescale != 0: the statistics first (inside launch_sched_threshold for SCHED_THRESH), so statistics, selection, step.
int launch_sched_step(const SchedStepParams& in, int mode, hipStream_t st, int pred) {
  ADM_REQUIRE(mode >= SCHED_PLAIN && mode <= SCHED_MULTISTEP, "sched_step: mode must be 0 (plain), 1 (thresholded) or 2 (multistep)");
  ADM_REQUIRE(pred >= PRED_EPSILON && pred <= PRED_V, "sched_step: prediction must be 0 (epsilon), 1 (sample) or 2 (v_prediction)");
  SchedStepParams p = in;
  p.per_sample = (long)p.C * p.H * p.W;
  p.n4 = p.per_sample * p.B / 4;
  p.mask_bstride = (long)p.n_mask_steps * p.per_sample;
  const bool guided = p.eps_uncond != nullptr, philox = p.philox != 0;
  ADM_REQUIRE(p.W % 4 == 0, "sched_step: W must be a multiple of 4");
  ADM_REQUIRE(p.mask == nullptr || p.C == 1, "sched_step: mask path requires C == 1 (as in the reference)");
  ADM_TRY(sched_known_prepare(p));
  if (guided) ADM_REQUIRE(std::isfinite(p.guidance), "sched_step: the guidance scale must be finite");
  if (philox) {   // noise drawn in the kernel: the key, row offset and stream id from *p.nblock, or from p.nvals when it is null
    ADM_REQUIRE(p.noise == nullptr, "sched_step: a noise buffer and the noise stream exclude each other");
    ADM_REQUIRE(p.B > 0 && p.per_sample > 0 && p.per_sample % 4 == 0, "sched_step: C*H*W must be a positive multiple of 4");
    ADM_REQUIRE(p.per_sample / 4 <= 0xffffffffL, "sched_step: C*H*W / 4 must fit in 32 bits (the counter's first word)");
  }
  const StepKernel kernel = kStepKernels[step_slot(mode, pred, guided, philox)];
  if (kernel == nullptr) {   // the two reasons a multistep combination is not built
    ADM_REQUIRE(pred == PRED_EPSILON, "sched_step: prediction must be 0 (the multistep step is epsilon only)");
    ADM_FAIL("sched_step: the multistep step has no noise rows");
  }
  if (mode == SCHED_THRESH) ADM_TRY(launch_sched_threshold(p, st, pred, "sched_step"));
  else ADM_TRY(launch_guidance_stats(p, st, "sched_step"));
  ADM_LAUNCH(kernel, dim3(ew_grid(p.n4)), dim3(256), 0, st, p);
  return ADM_CHECK_LAUNCH();
}

int launch_step_advance(int* step_dev, hipStream_t st) {
  ADM_LAUNCH(step_advance_kernel, dim3(1), dim3(1), 0, st, step_dev);
  return ADM_CHECK_LAUNCH();
}

int launch_encode_step(float* x, const float* eps, const adm_sched_coef* table, const int* step_dev, int step, int pred, long n,
                       hipStream_t st) {
  ADM_REQUIRE(n > 0 && n % 4 == 0, "encode_step: size must be a positive multiple of 4");
  ADM_REQUIRE(pred >= PRED_EPSILON && pred <= PRED_V, "encode_step: prediction must be 0 (epsilon), 1 (sample) or 2 (v_prediction)");
  ADM_REQUIRE(step_dev != nullptr || step >= 0, "encode_step: step must be >= 0 (or step_dev given)");
  using EncodeKernel = void (*)(float*, const float*, const adm_sched_coef*, const int*, int, long);
  static constexpr EncodeKernel kEncodeKernels[3] = {encode_step_kernel<PRED_EPSILON>, encode_step_kernel<PRED_SAMPLE>,
                                                     encode_step_kernel<PRED_V>};
  const EncodeKernel kernel = kEncodeKernels[pred];
  ADM_LAUNCH(kernel, dim3(ew_grid(n / 4)), dim3(256), 0, st, x, eps, table, step_dev, step, n / 4);
  return ADM_CHECK_LAUNCH();
}

int launch_add_noise(const float* x0, long x0_bstride, const float* noise, const float* sa, const float* sb, int cb,
                     int cn, float* out, int B, int N, long P, hipStream_t st) {
  ADM_REQUIRE(P % 4 == 0 && x0_bstride % 4 == 0, "add_noise: sizes must be multiples of 4");
  long g = (P / 4 + 255) / 256;
  if (g > 256) g = 256;
  ADM_LAUNCH(add_noise_kernel, dim3((unsigned)g, N, B), dim3(256), 0, st, x0, x0_bstride, noise, sa, sb, cb, cn, out, N,
             P / 4);
  return ADM_CHECK_LAUNCH();
}

int launch_noise_and_velocity(const float* x0, const float* noise, const float* sa, const float* sb, float* noisy, float* velocity,
                              int B, long P, hipStream_t st) {
  ADM_REQUIRE(B > 0 && B <= 65535 && P > 0 && P % 4 == 0, "noise_and_velocity: need 0 < B <= 65535 and P a positive multiple of 4");
  long g = (P / 4 + 255) / 256;
  if (g > 256) g = 256;
  ADM_LAUNCH(noise_and_velocity_kernel, dim3((unsigned)g, B), dim3(256), 0, st, x0, noise, sa, sb, noisy, velocity, P / 4);
  return ADM_CHECK_LAUNCH();
}

// ---- spherical interpolation grid (pipeline_audio_diffusion.py:244-258, batched over alphas) -------------------------------------
// theta = acos(<x0, x1> / |x0| / |x1|);  out[a] = sin((1 - alpha_a) theta) x0 / sin(theta) + sin(alpha_a theta) x1 / sin(theta)
// The three reductions accumulate in fp64 (torch: fp32); the blend repeats torch's float32 operation order exactly: python
// double scalars are cast to float32, then (s0 * x0) / sin(theta) + (s1 * x1) / sin(theta) with IEEE multiplies / divisions.
__global__ void __launch_bounds__(256) slerp_reduce_kernel(const float* __restrict__ x0, const float* __restrict__ x1, long n,
                                                           double* __restrict__ acc3) {
  __shared__ double red[3][4];
  double d = 0.0, a = 0.0, b = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const double u = x0[i], v = x1[i];
    d += u * v; a += u * u; b += v * v;
  }
  for (int m = 32; m >= 1; m >>= 1) { d += __shfl_xor(d, m, 64); a += __shfl_xor(a, m, 64); b += __shfl_xor(b, m, 64); }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = d; red[1][wave] = a; red[2][wave] = b; }
  __syncthreads();
  if (threadIdx.x < 3) atomicAdd(acc3 + threadIdx.x, red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]);
}

__global__ void __launch_bounds__(256) slerp_blend_kernel(const float* __restrict__ x0, const float* __restrict__ x1, long n,
                                                          const double* __restrict__ acc3, const double* __restrict__ alphas,
                                                          int n_alpha, float* __restrict__ out) {
  // torch: dot / norm / norm on float32 0-d tensors, then math.acos of the float32 quotient
  const float dotf = (float)acc3[0], n0 = (float)sqrt(acc3[1]), n1 = (float)sqrt(acc3[2]);
  const double theta = acos((double)((dotf / n0) / n1));
  const float st = (float)sin(theta);
  const int a = blockIdx.y;
  const double al = alphas[a];   // a double, as the reference's Python float: s0, s1 are rounded to float32 once
  const float s0 = (float)sin((1.0 - al) * theta), s1 = (float)sin(al * theta);
  float* o = out + (long)a * n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    o[i] = __fadd_rn(__fdiv_rn(__fmul_rn(s0, x0[i]), st), __fdiv_rn(__fmul_rn(s1, x1[i]), st));
}

int launch_slerp_grid(const float* x0, const float* x1, long n, const double* alphas_dev, int n_alpha, float* out,
                      double* scratch3, hipStream_t st) {
  ADM_TRY(dmemset(scratch3, 0, 3 * sizeof(double), st));
  ADM_LAUNCH(slerp_reduce_kernel, dim3(ew_grid(n)), dim3(256), 0, st, x0, x1, n, scratch3);
  ADM_LAUNCH(slerp_blend_kernel, dim3(ew_grid(n), n_alpha), dim3(256), 0, st, x0, x1, n, (const double*)scratch3, alphas_dev,
             n_alpha, out);
  return ADM_CHECK_LAUNCH();
}

int launch_dequant(const float* x, uint8_t* out, long n, hipStream_t st) {
  ADM_REQUIRE(n % 4 == 0, "dequant: size must be a multiple of 4");
  ADM_LAUNCH(dequant_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, st, x, out, n / 4);
  return ADM_CHECK_LAUNCH();
}

}  // namespace adm
