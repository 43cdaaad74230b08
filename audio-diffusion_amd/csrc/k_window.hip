// k_window.hip — windowed sampling (include/adm.h "Windowed sampling" has THE definition): the two copies that let a wide sample
// (B,C,H,Wt) go through a model of width W <= Wt as overlapping windows, and the cross-fade that joins the windows of a tiled codec.
//   window_gather_kernel     windows[(b*nW + w), c, y, j] = x[b, c, y, col(w, j)]                    a copy, bit-exact
//   window_blend_kernel      mean[b, c, y, col] = (o_w0 + o_w1 + ...) / float(count)                 over the windows that cover col
//   window_crossfade_kernel  out[b, c, y, col] = (m_w0*o_w0 + m_w1*o_w1 + ...) / float(m_w0 + ...)   the same windows in the same order, each
//                            weighted by an integer ramp m_w(j) that falls to 1 at an edge that has a neighbour ("Tiled codec" in adm.h)
// col(w, j) = w*s + j (open) or (w*s + j) mod Wt (circular). W, s and Wt are multiples of 4, so a float4 never straddles a window
// edge or the circle's seam: one float4 per lane per iteration, grid-stride, 256 lanes, the grid of the step kernels (ew_grid).
// The blend visits the covering windows in ascending index: first the windows that reach `col` without wrapping, w in
// [max(0, (col - W)/s + 1), min(col/s, nW - 1)], then (circular only) the windows whose tail wraps over the seam onto it,
// w in [(col + Wt - W)/s + 1, nW - 1]; the two ranges are disjoint because W <= Wt. The sum starts from the first window's value and
// every addition is an fp32 addition of its own (there is no product to contract with); one IEEE division by the cover count.
// No atomics, no scratch: the result depends on neither the launch geometry nor a replay.
// The cross-fade has the blend's form and order; its weights are computed from the index (no table), every product and every sum is
// rounded to fp32 on its own (plain operators under `fp contract(off)`), one IEEE division by the integer weight sum, and a column that ONE
// window covers is that window's value, copied ((m*o)/m is not o in fp32). With u8_out it also writes dequant_kernel's bytes of the value
// the lane has just computed, four to a 32-bit store.
// Traffic: gather 8 B per window element; blend and cross-fade 4 B read per window element + 4 B written per wide element (+ 1 B with
// u8_out). HBM-bound, tiny next to a forward. The blend is deliberately NOT fused into the step kernels: with `mean` written as a wide tensor every step instantiation,
// the UniPC step, the selection and the statistics kernel run on the wide shape as they are.
#include "k_sched_common.h"

namespace adm {

struct WindowGeom {
  int C, H, Wt, W, s, wrap, nW;
  long n4;   // float4 of the kernel's own index space (gather: the windows; blend: the wide tensor)
};

__global__ void __launch_bounds__(256) window_gather_kernel(const float* __restrict__ x, float* __restrict__ windows, const WindowGeom g) {
  const long stride = (long)gridDim.x * blockDim.x;
  const int w4 = g.W >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n4; i += stride) {
    const int j = (int)(i % w4) << 2;
    long r = i / w4;                       // ((b*nW + w)*C + c)*H + y
    const int y = (int)(r % g.H); r /= g.H;
    const int c = (int)(r % g.C); r /= g.C;
    const int w = (int)(r % g.nW);
    const long b = r / g.nW;
    int col = w * g.s + j;                 // < 2*Wt: w*s < Wt in either placement, j < W <= Wt
    if (g.wrap && col >= g.Wt) col -= g.Wt;
    const long src = ((b * g.C + c) * g.H + y) * g.Wt + col;
    reinterpret_cast<float4*>(windows)[i] = *reinterpret_cast<const float4*>(x + src);
  }
}

__global__ void __launch_bounds__(256) window_blend_kernel(const float* __restrict__ windows, float* __restrict__ out, const WindowGeom g) {
  const long stride = (long)gridDim.x * blockDim.x;
  const int t4 = g.Wt >> 2;
  const long plane = (long)g.H * g.W;      // one channel of one window
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n4; i += stride) {
    const int col = (int)(i % t4) << 2;
    long r = i / t4;                       // (b*C + c)*H + y
    const int y = (int)(r % g.H); r /= g.H;
    const int c = (int)(r % g.C);
    const long b = r / g.C;
    // element (c, y, 0) of window 0 of sample b; window w is w*C*plane further on
    const float* base = windows + ((b * g.nW * g.C + c) * g.H + y) * (long)g.W;
    const long wstep = (long)g.C * plane;
    const int lo = col >= g.W ? (col - g.W) / g.s + 1 : 0;
    int hi = col / g.s;
    if (hi > g.nW - 1) hi = g.nW - 1;
    float4 acc = *reinterpret_cast<const float4*>(base + lo * wstep + (col - lo * g.s));
    int count = 1;
    for (int w = lo + 1; w <= hi; ++w, ++count) {
      const float4 v = *reinterpret_cast<const float4*>(base + w * wstep + (col - w * g.s));
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    if (g.wrap) {
      for (int w = (col + g.Wt - g.W) / g.s + 1; w < g.nW; ++w, ++count) {
        const float4 v = *reinterpret_cast<const float4*>(base + w * wstep + (col + g.Wt - w * g.s));
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
    const float n = (float)count;          // (a column covered once: o / 1.0f is o itself)
    reinterpret_cast<float4*>(out)[i] = make_float4(__fdiv_rn(acc.x, n), __fdiv_rn(acc.y, n), __fdiv_rn(acc.z, n), __fdiv_rn(acc.w, n));
  }
}

// The integer weight of local column j of a window (include/adm.h "Tiled codec"): r = W - s is the overlap of neighbouring windows; the
// ramp 1, 3, 5, ... is capped at 2r and exists only towards an edge that has a neighbour.
__device__ __forceinline__ int crossfade_weight(int j, int W, int r, bool left, bool right) {
  if (r == 0) return 1;
  const int cap = 2 * r, up = 2 * j + 1, down = 2 * (W - 1 - j) + 1;
  const int a = left && up < cap ? up : cap;
  const int b = right && down < cap ? down : cap;
  return a < b ? a : b;
}

// One covering window's float4 v (local columns j..j+3) into the running weighted sum; the first window's products START the sum.
// Plain operators under `fp contract(off)`, for sched_guided's reason: hipcc's __fmul_rn / __fadd_rn are inline x * y and x + y, which
// the default contraction fuses into one fma once they are inlined side by side.
__device__ __forceinline__ void crossfade_visit(const float4& v, int j, int W, int r, bool left, bool right, bool first, float (&acc)[4],
                                                int (&den)[4]) {
#pragma clang fp contract(off)
  const float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int m = crossfade_weight(j + e, W, r, left, right);
    const float p = (float)m * o[e];
    acc[e] = first ? p : acc[e] + p;
    den[e] = first ? m : den[e] + m;
  }
}

__global__ void __launch_bounds__(256) window_crossfade_kernel(const float* __restrict__ windows, float* __restrict__ out,
                                                               unsigned char* __restrict__ u8_out, const WindowGeom g) {
  const long stride = (long)gridDim.x * blockDim.x;
  const int t4 = g.Wt >> 2;
  const long plane = (long)g.H * g.W;      // one channel of one window
  const int r = g.W - g.s;
  const bool ring = g.wrap && g.nW > 1;    // on the circle every window has both neighbours, unless it is alone
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n4; i += stride) {
    const int col = (int)(i % t4) << 2;
    long q = i / t4;                       // (b*C + c)*H + y
    const int y = (int)(q % g.H); q /= g.H;
    const int c = (int)(q % g.C);
    const long b = q / g.C;
    const float* base = windows + ((b * g.nW * g.C + c) * g.H + y) * (long)g.W;   // as window_blend_kernel
    const long wstep = (long)g.C * plane;
    const int lo = col >= g.W ? (col - g.W) / g.s + 1 : 0;
    int hi = col / g.s;
    if (hi > g.nW - 1) hi = g.nW - 1;
    const float4 v0 = *reinterpret_cast<const float4*>(base + lo * wstep + (col - lo * g.s));
    float acc[4];
    int den[4], count = 1;
    crossfade_visit(v0, col - lo * g.s, g.W, r, ring || lo > 0, ring || (!g.wrap && lo < g.nW - 1), true, acc, den);
    for (int w = lo + 1; w <= hi; ++w, ++count) {
      const float4 v = *reinterpret_cast<const float4*>(base + w * wstep + (col - w * g.s));
      crossfade_visit(v, col - w * g.s, g.W, r, true, ring || (!g.wrap && w < g.nW - 1), false, acc, den);   // (w > lo >= 0: a left neighbour)
    }
    if (g.wrap) {
      for (int w = (col + g.Wt - g.W) / g.s + 1; w < g.nW; ++w, ++count) {
        const float4 v = *reinterpret_cast<const float4*>(base + w * wstep + (col + g.Wt - w * g.s));
        crossfade_visit(v, col + g.Wt - w * g.s, g.W, r, ring, ring, false, acc, den);
      }
    }
    const float4 res = count == 1 ? v0   // a column covered once: the window's value, copied
                                  : make_float4(__fdiv_rn(acc[0], (float)den[0]), __fdiv_rn(acc[1], (float)den[1]),
                                                __fdiv_rn(acc[2], (float)den[2]), __fdiv_rn(acc[3], (float)den[3]));
    reinterpret_cast<float4*>(out)[i] = res;
    if (u8_out) reinterpret_cast<unsigned*>(u8_out)[i] = pack_u8x4(res.x, res.y, res.z, res.w);
  }
}

// The placement rules of the definition, each refused by the name of its argument (`pre` + total_w / stride / wrap: the loop's fields
// carry the prefix "window_"). -> the number of windows per wide sample.
int window_count(const char* who, const char* pre, int total_w, int W, int stride, int wrap, int* nW) {
  const std::string f = std::string(who) + ": ", p(pre);
  ADM_REQUIRE(wrap == 0 || wrap == 1, f + p + "wrap must be 0 (open) or 1 (circular)");
  ADM_REQUIRE(W > 0 && W % 4 == 0, f + "the window width W must be a positive multiple of 4");
  ADM_REQUIRE(stride > 0 && stride % 4 == 0, f + p + "stride must be a positive multiple of 4");
  ADM_REQUIRE(stride <= W, f + p + "stride must not exceed the window width W (every column is covered)");
  ADM_REQUIRE(total_w > 0 && total_w % 4 == 0, f + p + "total_w must be a positive multiple of 4");
  ADM_REQUIRE(total_w >= W, f + p + "total_w must be at least the window width W");
  if (wrap) {
    ADM_REQUIRE(total_w % stride == 0, f + p + "total_w must be a multiple of " + p + "stride when " + p + "wrap == 1");
    *nW = total_w / stride;
  } else {
    ADM_REQUIRE((total_w - W) % stride == 0, f + p + "total_w - W must be a multiple of " + p + "stride when " + p + "wrap == 0");
    *nW = (total_w - W) / stride + 1;
  }
  return 0;
}

static int window_geom(const char* who, const void* a, const void* b, int B, int C, int H, int total_w, int W, int stride, int wrap, WindowGeom* g) {
  ADM_REQUIRE(a != nullptr && b != nullptr, std::string(who) + ": null argument");
  ADM_REQUIRE(B > 0 && C > 0 && H > 0, std::string(who) + ": B, C and H must be positive");
  int nW = 0;
  ADM_TRY(window_count(who, "", total_w, W, stride, wrap, &nW));
  ADM_REQUIRE((long)B * nW <= 2147483647L, std::string(who) + ": B times the number of windows must fit in an int");
  *g = WindowGeom{C, H, total_w, W, stride, wrap, nW, 0};
  return 0;
}

int launch_window_gather(const float* x, float* windows, int B, int C, int H, int total_w, int W, int stride, int wrap, hipStream_t st) {
  WindowGeom g;
  ADM_TRY(window_geom("window_gather", x, windows, B, C, H, total_w, W, stride, wrap, &g));
  g.n4 = (long)B * g.nW * C * H * (W >> 2);
  ADM_LAUNCH(window_gather_kernel, dim3(ew_grid(g.n4)), dim3(256), 0, st, x, windows, g);
  return ADM_CHECK_LAUNCH();
}

int launch_window_blend(const float* windows, float* out, int B, int C, int H, int total_w, int W, int stride, int wrap, hipStream_t st) {
  WindowGeom g;
  ADM_TRY(window_geom("window_blend", windows, out, B, C, H, total_w, W, stride, wrap, &g));
  g.n4 = (long)B * C * H * (total_w >> 2);
  ADM_LAUNCH(window_blend_kernel, dim3(ew_grid(g.n4)), dim3(256), 0, st, windows, out, g);
  return ADM_CHECK_LAUNCH();
}

int launch_window_crossfade(const float* windows, float* out, uint8_t* u8_out, int B, int C, int H, int total_w, int W, int stride, int wrap,
                            hipStream_t st) {
  WindowGeom g;
  ADM_TRY(window_geom("window_crossfade", windows, out, B, C, H, total_w, W, stride, wrap, &g));
  g.n4 = (long)B * C * H * (total_w >> 2);
  ADM_LAUNCH(window_crossfade_kernel, dim3(ew_grid(g.n4)), dim3(256), 0, st, windows, out, u8_out, g);
  return ADM_CHECK_LAUNCH();
}

}  // namespace adm

extern "C" {

int adm_window_gather(const float* x, float* windows, int B, int C, int H, int total_w, int W, int stride, int wrap, void* stream) {
  return adm::launch_window_gather(x, windows, B, C, H, total_w, W, stride, wrap, (hipStream_t)stream);
}

int adm_window_blend(const float* windows, float* out, int B, int C, int H, int total_w, int W, int stride, int wrap, void* stream) {
  return adm::launch_window_blend(windows, out, B, C, H, total_w, W, stride, wrap, (hipStream_t)stream);
}

int adm_window_crossfade(const float* windows, float* out, uint8_t* u8_out, int B, int C, int H, int total_w, int W, int stride, int wrap,
                         void* stream) {
  return adm::launch_window_crossfade(windows, out, u8_out, B, C, H, total_w, W, stride, wrap, (hipStream_t)stream);
}

}  // extern "C"
