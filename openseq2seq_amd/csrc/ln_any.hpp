// LayerNorm rows of any width D % 8 == 0, 8 <= D <= 4096, next to the D = 512 / 1024 instantiations of
// transformer.hip ("layernorm_L2", kL1 = false) and transformer_norm.hip ("layernorm_L1", kL1 = true): one wave
// per row with a RUNTIME loop over the row's 16-byte pieces. A row (at most 8 KB) is read again from the cache for
// every pass instead of being held in a register array a runtime index would demote to scratch. Same results,
// saved statistics and [num_parts, 2, D] partial layout as the fixed-width kernels. Not tuned.
#pragma once
#include "os2s_common.hpp"

namespace os2s {

constexpr int kLnAnyMaxD = 4096;
static inline bool ln_any_width_ok(int D) { return D >= 8 && D <= kLnAnyMaxD && D % 8 == 0; }

__device__ __forceinline__ void ln_unpack8(const u32x4& t, float (&f)[8]) {
#pragma unroll
  for (int w = 0; w < 4; ++w) { f[2 * w] = bflo(t[w]); f[2 * w + 1] = bfhi(t[w]); }
}
__device__ __forceinline__ u32x4 ln_pack8(const float (&f)[8]) {
  u32x4 o;
#pragma unroll
  for (int w = 0; w < 4; ++w) o[w] = pack2bf(f[2 * w], f[2 * w + 1]);
  return o;
}

// L2: saves mean and rstd = rsqrt(var + eps); L1: mean and r = 1 / (mean|x - mean| + eps)
template <bool kL1>
__global__ __launch_bounds__(256) void layernorm_any_fwd_kernel(
    const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, long long N, int D, bf16_t* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ r_out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int D8 = D >> 3;
  const bf16_t* xr = x + row * D;
  const float fD = (float)D;      // divisions, not a reciprocal: 1 / D is inexact when D is no power of two, and a
  float s = 0.f;                  // constant row must come out with mean == x exactly (L1: mean|x - mean| = 0)
  for (int c = lane; c < D8; c += 64) {
    float v[8];
    ln_unpack8(*reinterpret_cast<const u32x4*>(xr + c * 8), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[e];
  }
  const float mean = wave_sum(s) / fD;
  float q = 0.f;
  for (int c = lane; c < D8; c += 64) {
    float v[8];
    ln_unpack8(*reinterpret_cast<const u32x4*>(xr + c * 8), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float d = v[e] - mean; q += kL1 ? fabsf(d) : d * d; }
  }
  q = wave_sum(q) / fD;
  const float r = kL1 ? 1.f / (q + eps) : rsqrtf(q + eps);
  for (int c = lane; c < D8; c += 64) {
    float v[8], o8[8];
    ln_unpack8(*reinterpret_cast<const u32x4*>(xr + c * 8), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = (v[e] - mean) * r * gamma[c * 8 + e] + beta[c * 8 + e];
    *reinterpret_cast<u32x4*>(y + row * D + c * 8) = ln_pack8(o8);
  }
  if (lane == 0) {
    if (mean_out) mean_out[row] = mean;
    if (r_out) r_out[row] = r;
  }
}

// One workgroup per block of rows_per_block rows (the num_parts of the fixed-width kernels). First the
// parameter-gradient partials, one column per thread over the block's rows in a fixed order:
//   partial[blk][0][c] = sum dy, partial[blk][1][c] = sum dy * (x - mean) * r;
// then one wave per row: dx = dres + (the formulas of layernorm_bwd_kernel / layernorm_l1_bwd_kernel).
template <bool kL1>
__global__ __launch_bounds__(512) void layernorm_any_bwd_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rsave,
    const bf16_t* __restrict__ dres, long long N, int D, int rows_per_block, bf16_t* __restrict__ dx,
    float* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long left = N - r0;
  const int n = (int)(left < rows_per_block ? left : rows_per_block);
  for (int c = threadIdx.x; c < D; c += 512) {
    float sb = 0.f, sg = 0.f;
    for (int i = 0; i < n; ++i) {
      const float d = bf2f(dy[(r0 + i) * D + c]);
      sb += d;
      sg += d * ((bf2f(x[(r0 + i) * D + c]) - mean[r0 + i]) * rsave[r0 + i]);
    }
    partial[((long long)blockIdx.x * 2) * D + c] = sb;
    partial[((long long)blockIdx.x * 2 + 1) * D + c] = sg;
  }
  const int D8 = D >> 3;
  const float invD = 1.f / (float)D;
  for (int i = wid; i < n; i += 8) {
    const long long ro = (r0 + i) * D;
    const float mu = mean[r0 + i], rs = rsave[r0 + i];
    // L2: s1 = sum g, s2 = sum g * xhat;  L1: s1 = sum g, s2 = sum g * c, s3 = sum sign(c)   (g = gamma * dy)
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int c = lane; c < D8; c += 64) {
      float dv[8], xv[8];
      ln_unpack8(*reinterpret_cast<const u32x4*>(dy + ro + c * 8), dv);
      ln_unpack8(*reinterpret_cast<const u32x4*>(x + ro + c * 8), xv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = gamma[c * 8 + e] * dv[e];
        const float cc = xv[e] - mu;
        s1 += g;
        s2 += g * (kL1 ? cc : cc * rs);
        if (kL1) s3 += cc > 0.f ? 1.f : (cc < 0.f ? -1.f : 0.f);
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (kL1) s3 = wave_sum(s3);
    const float k = rs * rs * invD * s2;                 // L1
    const float mdc = (rs * s1 - k * s3) * invD;         // L1
    for (int c = lane; c < D8; c += 64) {
      float dv[8], xv[8], rv[8], o8[8];
      ln_unpack8(*reinterpret_cast<const u32x4*>(dy + ro + c * 8), dv);
      ln_unpack8(*reinterpret_cast<const u32x4*>(x + ro + c * 8), xv);
      u32x4 t = {0u, 0u, 0u, 0u};
      if (dres) t = *reinterpret_cast<const u32x4*>(dres + ro + c * 8);
      ln_unpack8(t, rv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = gamma[c * 8 + e] * dv[e];
        const float cc = xv[e] - mu;
        if (kL1) {
          const float sgn = cc > 0.f ? 1.f : (cc < 0.f ? -1.f : 0.f);
          o8[e] = g * rs - k * sgn - mdc + rv[e];
        } else {
          o8[e] = rs * (g - s1 * invD - cc * rs * (s2 * invD)) + rv[e];
        }
      }
      *reinterpret_cast<u32x4*>(dx + ro + c * 8) = ln_pack8(o8);
    }
  }
}

}  // namespace os2s
