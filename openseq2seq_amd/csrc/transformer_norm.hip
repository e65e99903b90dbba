// The "batch_norm" normalisation of the Transformer's PrePostProcessingWrapper / output_normalization
// (parts/transformer/common.py:11-106, norm_params "type"; the two LayerNorm kinds: layernorm.hip), on PACKED
// token-major bf16 [N, D] tensors: Transformer_BatchNorm (common.py:11-38) over the tokens of the packed batch.
// Statistics come from os2s_bn_stats + os2s_bn_finalize (batchnorm.hip, TF fused-BN conventions), the kernels here
// are the affine apply and the two backward passes (one reduction, one apply that adds the residual gradient).
#include "os2s_common.hpp"

namespace os2s {

// ---------------------------------------------------------------------------
// token BatchNorm over [N, D] rows
// ---------------------------------------------------------------------------
// y = x * scale + shift (scale / shift per column: os2s_bn_finalize's, from batch or moving statistics)
__global__ __launch_bounds__(256) void token_bn_apply_kernel(
    const bf16_t* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
    long long n8, int D8, bf16_t* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    const int c0 = (int)(i % D8) * 8;
    float v[8], a[8], b[8];
    unpack8(reinterpret_cast<const u32x4*>(x)[i], v);
    load8(scale + c0, a);
    load8(shift + c0, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = v[e] * a[e] + b[e];
    reinterpret_cast<u32x4*>(y)[i] = pack8(v);
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
    float d[8], xv[8];
    unpack8(a, d);
    unpack8(t, xv);
#pragma unroll
    for (int e = 0; e < 8; ++e) { sd[e] += d[e]; sx[e] += d[e] * (xv[e] - mu[e]) * rs[e]; }
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
    float d[8], xv[8], rv[8], o8[8];
    unpack8(a, d);
    unpack8(t, xv);
    unpack8(rr, rv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = (xv[e] - mu[e]) * rs[e];
      const float gr = (gamma ? gm[e] : 1.f) * rs[e];
      o8[e] = gr * (d[e] - k1[e] - xh * k2[e]) + rv[e];
    }
    reinterpret_cast<u32x4*>(dx)[i] = pack8(o8);
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
