// The other two normalisations of the Transformer's PrePostProcessingWrapper / output_normalization
// (parts/transformer/common.py:11-106, norm_params "type"), on PACKED token-major bf16 [N, D] tensors:
//   * LayerNormalization "layernorm_L1" (common.py:69-80): per row c = x - mean(x), a = mean(|c|),
//     y = c / (a + eps) * scale + bias. The reference's fp16 saturate_cast has no counterpart: activations
//     here are bf16, whose range is fp32's, so the cast back cannot overflow.
//     Forward / backward follow layernorm_fwd_kernel / layernorm_bwd_kernel of transformer.hip (one wave per
//     row; the backward shares their row prefetch, ln_rows.hpp, adds the residual-branch gradient and writes
//     [nparts, 2, D] parameter-gradient partials).
//   * Transformer_BatchNorm (common.py:11-38) over the tokens of the packed batch: statistics come from
//     os2s_bn_stats + os2s_bn_finalize (batchnorm.hip, TF fused-BN conventions), the kernels here are the
//     affine apply and the two backward passes (one reduction, one apply that adds the residual gradient).
#include "os2s_common.hpp"
#include "ln_rows.hpp"
#include "ln_any.hpp"

namespace os2s {

// ---------------------------------------------------------------------------
// layernorm_L1: one wave per row
// ---------------------------------------------------------------------------
// saves mean and r = 1 / (mean|x - mean| + eps) per row; both reductions run on the row held in registers
template <int VPL>  // 16-byte vectors per lane: D = 64 * 8 * VPL
__global__ __launch_bounds__(256) void layernorm_l1_fwd_kernel(
    const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, long long N, bf16_t* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ r_out) {
  constexpr int D = 64 * 8 * VPL;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  float v[VPL][8];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < VPL; ++u) {
    const u32x4 t = *reinterpret_cast<const u32x4*>(x + row * D + (u * 64 + lane) * 8);
    v[u][0] = bflo(t[0]); v[u][1] = bfhi(t[0]); v[u][2] = bflo(t[1]); v[u][3] = bfhi(t[1]);
    v[u][4] = bflo(t[2]); v[u][5] = bfhi(t[2]); v[u][6] = bflo(t[3]); v[u][7] = bfhi(t[3]);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[u][e];
  }
  const float mean = wave_sum(s) * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < VPL; ++u)
#pragma unroll
    for (int e = 0; e < 8; ++e) q += fabsf(v[u][e] - mean);
  const float r = 1.f / (wave_sum(q) * (1.f / D) + eps);
#pragma unroll
  for (int u = 0; u < VPL; ++u) {
    const int c0 = (u * 64 + lane) * 8;
    float o8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = (v[u][e] - mean) * r * gamma[c0 + e] + beta[c0 + e];
    u32x4 o;
    o[0] = pack2bf(o8[0], o8[1]); o[1] = pack2bf(o8[2], o8[3]);
    o[2] = pack2bf(o8[4], o8[5]); o[3] = pack2bf(o8[6], o8[7]);
    *reinterpret_cast<u32x4*>(y + row * D + c0) = o;
  }
  if (lane == 0) {
    if (mean_out) mean_out[row] = mean;
    if (r_out) r_out[row] = r;
  }
}

// With g = dy * scale, c = x - mean, s = sign(c) (0 at 0), r = 1 / (a + eps), a = mean|c|:
//   dc = g r - (r^2 / D) sum(g c) s,   dx = dc - mean(dc) + dres,
// and mean(dc) = (r sum(g) - (r^2 / D) sum(g c) sum(s)) / D: the three sums are ONE reduction step per row.
// Per-block partial sums of dbias = sum dy, dscale = sum dy * c r -> partial[blk][2][D].
constexpr int kL1Waves = 8;
static const int kL1RowsPerBlock = 32;

template <int VPL>
__global__ __launch_bounds__(64 * kL1Waves) void layernorm_l1_bwd_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rinv,
    const bf16_t* __restrict__ dres, long long N, int rows_per_block, bf16_t* __restrict__ dx,
    float* __restrict__ partial) {
  constexpr int D = 64 * 8 * VPL;
  constexpr int kOob = 0x7fffffff;
  __shared__ float red[kL1Waves][D];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float gb[VPL][8], gg[VPL][8], gm[VPL][8];
#pragma unroll
  for (int u = 0; u < VPL; ++u) {
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + (u * 64 + lane) * 8);
    const f32x4 g1 = *reinterpret_cast<const f32x4*>(gamma + (u * 64 + lane) * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { gm[u][e] = g0[e]; gm[u][4 + e] = g1[e]; }
#pragma unroll
    for (int e = 0; e < 8; ++e) { gb[u][e] = 0.f; gg[u][e] = 0.f; }
  }
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long left = N - r0;
  const int n = (int)(left < rows_per_block ? left : rows_per_block);
  const __amdgpu_buffer_rsrc_t dyr = ln_rows_rsrc(dy, r0, n, D);
  const __amdgpu_buffer_rsrc_t xr = ln_rows_rsrc(x, r0, n, D);
  const __amdgpu_buffer_rsrc_t drr = ln_rows_rsrc(dres, r0, n, D);
  const __amdgpu_buffer_rsrc_t dxr = ln_rows_rsrc(dx, r0, n, D);
  auto fetch = [&](int i, LnRow<VPL>& R) {
    const bool in = i < n;
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
      const int off = in ? i * (D * 2) + (u * 64 + lane) * 16 : kOob;
      R.a[u] = __builtin_amdgcn_raw_buffer_load_b128(dyr, off, 0, 0);
      R.t[u] = __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0);
      R.r[u] = __builtin_amdgcn_raw_buffer_load_b128(drr, off, 0, 0);
    }
    const long long gr = r0 + (in ? i : 0);
    R.mu = mean[gr];
    R.rs = rinv[gr];
  };
  auto process = [&](int i, const LnRow<VPL>& cur) {
    const float mu = cur.mu, rs = cur.rs;
    float gv[VPL][8], cv[VPL][8];
    float sg = 0.f, sgc = 0.f, ss = 0.f;
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
      const u32x4 a = cur.a[u], t = cur.t[u];
      float dyv[8];
      dyv[0] = bflo(a[0]); dyv[1] = bfhi(a[0]); dyv[2] = bflo(a[1]); dyv[3] = bfhi(a[1]);
      dyv[4] = bflo(a[2]); dyv[5] = bfhi(a[2]); dyv[6] = bflo(a[3]); dyv[7] = bfhi(a[3]);
      cv[u][0] = bflo(t[0]); cv[u][1] = bfhi(t[0]); cv[u][2] = bflo(t[1]); cv[u][3] = bfhi(t[1]);
      cv[u][4] = bflo(t[2]); cv[u][5] = bfhi(t[2]); cv[u][6] = bflo(t[3]); cv[u][7] = bfhi(t[3]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float c = cv[u][e] - mu;
        cv[u][e] = c;
        gb[u][e] += dyv[e];
        gg[u][e] += dyv[e] * (c * rs);
        const float g = gm[u][e] * dyv[e];
        gv[u][e] = g;
        sg += g;
        sgc += g * c;
        ss += c > 0.f ? 1.f : (c < 0.f ? -1.f : 0.f);
      }
    }
    sg = wave_sum_dpp(sg);
    sgc = wave_sum_dpp(sgc);
    ss = wave_sum_dpp(ss);
    const float k = rs * rs * (1.f / D) * sgc;
    const float mdc = (rs * sg - k * ss) * (1.f / D);
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
      float o8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float c = cv[u][e];
        const float s = c > 0.f ? 1.f : (c < 0.f ? -1.f : 0.f);
        o8[e] = gv[u][e] * rs - k * s - mdc;
      }
      const u32x4 t = cur.r[u];            // zeros without a residual gradient
      o8[0] += bflo(t[0]); o8[1] += bfhi(t[0]); o8[2] += bflo(t[1]); o8[3] += bfhi(t[1]);
      o8[4] += bflo(t[2]); o8[5] += bfhi(t[2]); o8[6] += bflo(t[3]); o8[7] += bfhi(t[3]);
      u32x4 o;
      o[0] = pack2bf(o8[0], o8[1]); o[1] = pack2bf(o8[2], o8[3]);
      o[2] = pack2bf(o8[4], o8[5]); o[3] = pack2bf(o8[6], o8[7]);
      __builtin_amdgcn_raw_buffer_store_b128(o, dxr, i * (D * 2) + (u * 64 + lane) * 16, 0, 0);
    }
  };
  // two row buffers used alternately, the next row's loads issued before this row is reduced
  // (the scheme of layernorm_bwd_kernel)
  LnRow<VPL> ra, rb;
  fetch(wid, ra);
  for (int i = wid; i < n; i += 2 * kL1Waves) {
    fetch(i + kL1Waves, rb);
    __builtin_amdgcn_sched_barrier(0);
    process(i, ra);
    if (i + kL1Waves >= n) break;
    fetch(i + 2 * kL1Waves, ra);
    __builtin_amdgcn_sched_barrier(0);
    process(i + kL1Waves, rb);
  }
  // block reduce the parameter-gradient partials over the waves (fixed order)
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < VPL; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        red[wid][(u * 64 + lane) * 8 + e] = pass == 0 ? gb[u][e] : gg[u][e];
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += 64 * kL1Waves) {
      float acc = 0.f;
#pragma unroll
      for (int w = 0; w < kL1Waves; ++w) acc += red[w][c];
      partial[((long long)blockIdx.x * 2 + pass) * D + c] = acc;
    }
  }
}

// ---------------------------------------------------------------------------
// token BatchNorm over [N, D] rows
// ---------------------------------------------------------------------------
// y = x * scale + shift (scale / shift per column: os2s_bn_finalize's, from batch or moving statistics)
__global__ __launch_bounds__(256) void token_bn_apply_kernel(
    const bf16_t* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
    long long n8, int D8, bf16_t* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    const int c0 = (int)(i % D8) * 8;
    const u32x4 t = reinterpret_cast<const u32x4*>(x)[i];
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(scale + c0), a1 = *reinterpret_cast<const f32x4*>(scale + c0 + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(shift + c0), b1 = *reinterpret_cast<const f32x4*>(shift + c0 + 4);
    u32x4 o;
    o[0] = pack2bf(bflo(t[0]) * a0[0] + b0[0], bfhi(t[0]) * a0[1] + b0[1]);
    o[1] = pack2bf(bflo(t[1]) * a0[2] + b0[2], bfhi(t[1]) * a0[3] + b0[3]);
    o[2] = pack2bf(bflo(t[2]) * a1[0] + b1[0], bfhi(t[2]) * a1[1] + b1[1]);
    o[3] = pack2bf(bflo(t[3]) * a1[2] + b1[2], bfhi(t[3]) * a1[3] + b1[3]);
    reinterpret_cast<u32x4*>(y)[i] = o;
  }
}

// backward reduction: partial[blk][2][D] = {sum dy, sum dy * xhat} over the block's rows, xhat = (x - mean) rstd.
// Thread -> 8-column group g = tid % D8, row lane rl = tid / D8 (D8 = D / 8 divides 256); four rows of loads in
// flight per thread, then the row lanes are summed through LDS in a fixed order.
static const int kTokBnRowsPerBlock = 64;

__global__ __launch_bounds__(256) void token_bn_bwd_reduce_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, long long N, int D, int rows_per_block, float* __restrict__ partial) {
  __shared__ float red[2][256 * 8];
  const int D8 = D >> 3;
  const int RL = 256 / D8;
  const int g = threadIdx.x % D8, rl = threadIdx.x / D8;
  const int c0 = g * 8;
  float mu[8], rs[8], sd[8], sx[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { mu[e] = mean[c0 + e]; rs[e] = rstd[c0 + e]; sd[e] = 0.f; sx[e] = 0.f; }
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = min(N, r0 + rows_per_block);
  auto acc = [&](const u32x4 a, const u32x4 t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d0 = bflo(a[e]), d1 = bfhi(a[e]);
      sd[2 * e] += d0; sx[2 * e] += d0 * (bflo(t[e]) - mu[2 * e]) * rs[2 * e];
      sd[2 * e + 1] += d1; sx[2 * e + 1] += d1 * (bfhi(t[e]) - mu[2 * e + 1]) * rs[2 * e + 1];
    }
  };
  long long r = r0 + rl;
  for (; r + 3LL * RL < r1; r += 4LL * RL) {
    u32x4 a[4], t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = *reinterpret_cast<const u32x4*>(dy + (r + (long long)u * RL) * D + c0);
      t[u] = *reinterpret_cast<const u32x4*>(x + (r + (long long)u * RL) * D + c0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc(a[u], t[u]);
  }
  for (; r < r1; r += RL)
    acc(*reinterpret_cast<const u32x4*>(dy + r * D + c0), *reinterpret_cast<const u32x4*>(x + r * D + c0));
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[0][threadIdx.x * 8 + e] = sd[e];
    red[1][threadIdx.x * 8 + e] = sx[e];
  }
  __syncthreads();
  if (rl != 0) return;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float s0 = 0.f, s1 = 0.f;
    for (int l = 0; l < RL; ++l) {
      s0 += red[0][(l * D8 + g) * 8 + e];
      s1 += red[1][(l * D8 + g) * 8 + e];
    }
    partial[((long long)blockIdx.x * 2) * D + c0 + e] = s0;
    partial[((long long)blockIdx.x * 2 + 1) * D + c0 + e] = s1;
  }
}

// eight consecutive fp32 per-column values (c0 a multiple of 8: 32-byte aligned in a torch allocation)
__device__ __forceinline__ void load8(const float* p, float* v) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}

// backward apply: dx = gamma * rstd * (dy - c1 - xhat * c2) + dres (gamma NULL = 1, dres NULL = 0)
__global__ __launch_bounds__(256) void token_bn_bwd_apply_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ c1,
    const float* __restrict__ c2, const bf16_t* __restrict__ dres, long long n8, int D8,
    bf16_t* __restrict__ dx) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    const int c0 = (int)(i % D8) * 8;
    const u32x4 a = reinterpret_cast<const u32x4*>(dy)[i];
    const u32x4 t = reinterpret_cast<const u32x4*>(x)[i];
    u32x4 rr = {0u, 0u, 0u, 0u};
    if (dres) rr = reinterpret_cast<const u32x4*>(dres)[i];
    float mu[8], rs[8], k1[8], k2[8], gm[8];
    load8(mean + c0, mu);
    load8(rstd + c0, rs);
    load8(c1 + c0, k1);
    load8(c2 + c0, k2);
    if (gamma) load8(gamma + c0, gm);
    float o8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = (e & 1) ? bfhi(a[e >> 1]) : bflo(a[e >> 1]);
      const float xv = (e & 1) ? bfhi(t[e >> 1]) : bflo(t[e >> 1]);
      const float rv = (e & 1) ? bfhi(rr[e >> 1]) : bflo(rr[e >> 1]);
      const float xh = (xv - mu[e]) * rs[e];
      const float gr = (gamma ? gm[e] : 1.f) * rs[e];
      o8[e] = gr * (d - k1[e] - xh * k2[e]) + rv;
    }
    u32x4 o;
    o[0] = pack2bf(o8[0], o8[1]); o[1] = pack2bf(o8[2], o8[3]);
    o[2] = pack2bf(o8[4], o8[5]); o[3] = pack2bf(o8[6], o8[7]);
    reinterpret_cast<u32x4*>(dx)[i] = o;
  }
}

static int tn_blocks(long long work) {
  long long b = (work + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (int)b;
}

static bool tok_bn_width_ok(int D) { return D >= 8 && D % 8 == 0 && D / 8 <= 256 && 256 % (D / 8) == 0; }

}  // namespace os2s

using namespace os2s;

extern "C" int os2s_layernorm_l1_fwd(os2s_stream_t stream, const uint16_t* x, const float* gamma,
                                     const float* beta, float eps, long long N, int D, uint16_t* y,
                                     float* mean, float* rinv) {
  OS2S_REQUIRE(x && gamma && beta && y && N >= 0);
  if (N == 0) return OS2S_OK;
  dim3 grid(ceil_div(N, 4));
  if (D == 1024) {
    OS2S_LAUNCH(layernorm_l1_fwd_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, x, gamma, beta, eps,
                N, y, mean, rinv);
  } else if (D == 512) {
    OS2S_LAUNCH(layernorm_l1_fwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, gamma, beta, eps,
                N, y, mean, rinv);
  } else if (ln_any_width_ok(D)) {      // every other width: the row kernel with a runtime column loop
    OS2S_LAUNCH(layernorm_any_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, gamma, beta, eps,
                N, D, y, mean, rinv);
  } else {
    return OS2S_ERR_UNSUPPORTED;
  }
  return OS2S_OK;
}

extern "C" int os2s_layernorm_l1_bwd_num_parts(long long N) { return ceil_div(N, kL1RowsPerBlock); }

extern "C" int os2s_layernorm_l1_bwd(os2s_stream_t stream, const uint16_t* dy, const uint16_t* x,
                                     const float* gamma, const float* mean, const float* rinv,
                                     const uint16_t* dres, long long N, int D, uint16_t* dx,
                                     float* partial) {
  OS2S_REQUIRE(dy && x && gamma && mean && rinv && dx && partial && N >= 0);
  if (N == 0) return OS2S_OK;
  dim3 grid(ceil_div(N, kL1RowsPerBlock));
  if (D == 1024) {
    OS2S_LAUNCH(layernorm_l1_bwd_kernel<2>, grid, dim3(64 * kL1Waves), 0, (hipStream_t)stream, dy, x, gamma, mean,
                rinv, dres, N, kL1RowsPerBlock, dx, partial);
  } else if (D == 512) {
    OS2S_LAUNCH(layernorm_l1_bwd_kernel<1>, grid, dim3(64 * kL1Waves), 0, (hipStream_t)stream, dy, x, gamma, mean,
                rinv, dres, N, kL1RowsPerBlock, dx, partial);
  } else if (ln_any_width_ok(D)) {
    OS2S_LAUNCH(layernorm_any_bwd_kernel<true>, grid, dim3(512), 0, (hipStream_t)stream, dy, x, gamma, mean,
                rinv, dres, N, D, kL1RowsPerBlock, dx, partial);
  } else {
    return OS2S_ERR_UNSUPPORTED;
  }
  return OS2S_OK;
}

extern "C" int os2s_token_bn_apply(os2s_stream_t stream, const uint16_t* x, const float* scale,
                                   const float* shift, long long N, int D, uint16_t* y) {
  OS2S_REQUIRE(x && scale && shift && y && N >= 0 && D >= 8 && D % 8 == 0);
  if (N == 0) return OS2S_OK;
  const long long n8 = N * (D / 8);
  OS2S_LAUNCH(token_bn_apply_kernel, dim3(tn_blocks(n8)), dim3(256), 0, (hipStream_t)stream, x, scale, shift,
              n8, D / 8, y);
  return OS2S_OK;
}

extern "C" int os2s_token_bn_bwd_num_parts(long long N) {
  return N < 1 ? 1 : (int)ceil_div(N, kTokBnRowsPerBlock);
}

extern "C" int os2s_token_bn_bwd_reduce(os2s_stream_t stream, const uint16_t* dy, const uint16_t* x,
                                        const float* mean, const float* rstd, long long N, int D,
                                        float* partial) {
  OS2S_REQUIRE(dy && x && mean && rstd && partial && N >= 1);
  if (!tok_bn_width_ok(D)) return OS2S_ERR_UNSUPPORTED;
  OS2S_LAUNCH(token_bn_bwd_reduce_kernel, dim3(ceil_div(N, kTokBnRowsPerBlock)), dim3(256), 0,
              (hipStream_t)stream, dy, x, mean, rstd, N, D, kTokBnRowsPerBlock, partial);
  return OS2S_OK;
}

extern "C" int os2s_token_bn_bwd_apply(os2s_stream_t stream, const uint16_t* dy, const uint16_t* x,
                                       const float* gamma, const float* mean, const float* rstd,
                                       const float* c1, const float* c2, const uint16_t* dres,
                                       long long N, int D, uint16_t* dx) {
  OS2S_REQUIRE(dy && x && mean && rstd && c1 && c2 && dx && N >= 0 && D >= 8 && D % 8 == 0);
  if (N == 0) return OS2S_OK;
  const long long n8 = N * (D / 8);
  OS2S_LAUNCH(token_bn_bwd_apply_kernel, dim3(tn_blocks(n8)), dim3(256), 0, (hipStream_t)stream, dy, x, gamma,
              mean, rstd, c1, c2, dres, n8, D / 8, dx);
  return OS2S_OK;
}
