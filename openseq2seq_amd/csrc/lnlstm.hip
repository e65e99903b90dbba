// LayerNorm-LSTM recurrence (AWD-style LSTM language model), forward and backward-through-time, gfx950.
//
// Reference cell: parts/rnns/weight_drop.py:140-166, WeightDropLayerNormBasicLSTMCell with layer_norm=True (no
// bias), gate order i, j, f, o, tf.contrib.layers.layer_norm over the H units of one sample (biased variance,
// epsilon 1e-12) on each gate pre-activation and on the new cell state, recurrent dropout on the candidate:
//   a_g  = gx_g[b,t] + h_{t-1} Wh_g^T
//   n_g  = LN(a_g; gamma_g, beta_g)
//   cand = tanh(n_j) * m / keep
//   c~   = c_{t-1} * s(n_f + forget_bias) + s(n_i) * cand
//   c_t  = LN(c~; gamma_s, beta_s)              (the NORMALISED state is carried)
//   h_t  = tanh(c_t) * s(n_o)
//
// Structure. csrc/rnn.hip splits the hidden units of a step over workgroups (8 units each); a LayerNorm over all
// H units is an all-to-all seam between them, so a step is TWO launches, cut at that seam:
//   1. product: the split-K recurrent product of rnn_tile.hpp, exactly the tile of rnn_step_fwd_kernel<4>, with
//      an epilogue that only adds gx and stores the raw pre-activations [B, 4H] in fp32 (a bf16 round in front
//      of a LayerNorm would be amplified by 1 / sigma);
//   2. cell: one WAVE per sample. Lane l owns the 8-unit chunks l, l + 64, ... (NCH of them: 1 up to H = 512,
//      2 up to 1024, 4 up to 2048), all four gates of them in registers; five pairs of wave reductions (mean, then
//      the centred variance, never E[x^2] - mean^2), everything else lane-local.
// The backward mirrors it: dh = dgx[s + 1] . Wh as the product launch (ROWS = 8 or 32 as in rnn.hip), then a
// per-sample cell backward with the five LayerNorm backward reduction pairs. The gamma / beta gradients
// accumulate over t in a per-sample fp32 buffer that only that sample's wave touches and are summed over B in
// a fixed order at the end: no atomics, bit-identical on a rerun.
// Saved for the backward: xhat [B,T,4H] bf16 (the normalised pre-activations, before gamma / beta), s_hat
// [B,T,H] fp32 (the normalised c~: c_t = gamma_s s_hat + beta_s), rstd [B,T,5] fp32. The mask is recomputed.
#include "os2s_common.hpp"
#include "rnn_tile.hpp"

namespace os2s {

constexpr int kLnWaves = 8;
constexpr float kLnEps = 1e-12f;

__device__ __forceinline__ void ld8(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}
__device__ __forceinline__ void st8(float* p, const float (&v)[8]) {
  const f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
  *reinterpret_cast<f32x4*>(p) = a;
  *reinterpret_cast<f32x4*>(p + 4) = b;
}
__device__ __forceinline__ void ld8bf(const bf16_t* p, float (&v)[8]) {
  const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[2 * e] = bflo(q[e]); v[2 * e + 1] = bfhi(q[e]); }
}
__device__ __forceinline__ void st8bf(bf16_t* p, const float (&v)[8]) {
  u32x4 q;
#pragma unroll
  for (int e = 0; e < 4; ++e) q[e] = pack2bf(v[2 * e], v[2 * e + 1]);
  *reinterpret_cast<u32x4*>(p) = q;
}

// ---------------------------------------------------------------------------------------------- forward
struct LnInitArgs {
  const float* h0; const float* c0;   // [B,H] or null (zero)
  float* h32; float* c32; bf16_t* h16;
  long long n;
};
__global__ __launch_bounds__(256) void lnlstm_init_kernel(LnInitArgs p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const float h = p.h0 ? p.h0[i] : 0.f;
  p.h32[i] = h;
  p.h16[i] = f2bf(h);
  p.c32[i] = p.c0 ? p.c0[i] : 0.f;
}

struct LnProdFwdArgs {
  const bf16_t* gx;     // [B,T,4H]
  const bf16_t* wh;     // [4H,H]
  const bf16_t* h16;    // [B,H]
  float* pre;           // [B,4H] raw pre-activations of this step
  const int32_t* lens;
  int B, T, H, step;
};
// the tile of rnn_step_fwd_kernel<4>: 8 units x 4 gates x 32 samples per workgroup, split-K over 8 waves
__global__ __launch_bounds__(64 * kLnWaves) void lnlstm_prod_fwd_kernel(LnProdFwdArgs p) {
  __shared__ float red[kLnWaves * 16 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int j0 = blockIdx.x * 8, b0 = blockIdx.y * 32;
  const int H = p.H;
  const int eb = b0 + l31, ej = j0 + (wave & 3) + 4 * lhi;
  const bool evalid = wave < 4 && eb < p.B && ej < H;
  bool act = false;
  float pre[4] = {0.f, 0.f, 0.f, 0.f};
  if (evalid) {
    const int len = p.lens ? min(max(p.lens[eb], 0), p.T) : p.T;
    act = p.step < len;
    if (act) {
      const long long row = (long long)eb * p.T + p.step;
#pragma unroll
      for (int g = 0; g < 4; ++g) pre[g] = bf2f(p.gx[row * (4 * H) + (long long)g * H + ej]);
    }
  }
  f32x16 accw;
#pragma unroll
  for (int e = 0; e < 16; ++e) accw[e] = 0.f;
  {
    const int g = l31 >> 3, uu = min(j0 + (l31 & 7), H - 1);
    const bf16_t* wrow = p.wh + ((long long)g * H + uu) * H;
    const int brow = b0 + l31;
    const bf16_t* irow = brow < p.B ? p.h16 + (long long)brow * H : nullptr;
    tile_gemm_prefetch<kLnWaves, 8>(wrow, irow, H, accw, p.wh);
  }
  float acc[4];
  tile_reduce_units<kLnWaves>(accw, red, acc);
  if (!act) return;
#pragma unroll
  for (int g = 0; g < 4; ++g) p.pre[(long long)eb * (4 * H) + (long long)g * H + ej] = pre[g] + acc[g];
}

struct LnCellFwdArgs {
  const float* pre;     // [B,4H]
  const float* ln;      // [10,H]: gamma_i, beta_i, gamma_j, beta_j, gamma_f, beta_f, gamma_o, beta_o, gamma_s, beta_s
  float* h32; float* c32; bf16_t* h16;   // [B,H] state
  bf16_t* y; long long ldy;
  bf16_t* xhat;         // [B,T,4H] or null
  float* shat;          // [B,T,H] or null
  float* rstd;          // [B,T,5] or null
  const int32_t* lens;
  int B, T, H, step;
  float forget_bias, keep;
  unsigned long long seed;
};

// One wave per sample; lane l owns chunks l + 64 c (c < NCH) of 8 consecutive units.
template <int NCH>
__global__ __launch_bounds__(64) void lnlstm_cell_fwd_kernel(LnCellFwdArgs p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int H = p.H, nchunk = H >> 3;
  const int len = p.lens ? min(max(p.lens[b], 0), p.T) : p.T;
  if (p.step >= len) return;       // wave-uniform: past the end the state passes through, y stays zero
  const long long row = (long long)b * p.T + p.step;
  const float invH = 1.f / (float)H;
  float a[4][NCH][8];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = lane + 64 * c;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (ch < nchunk) ld8(p.pre + (long long)b * (4 * H) + (long long)g * H + ch * 8, a[g][c]);
      else {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[g][c][e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) s[g] += a[g][c][e];
    }
  }
  float mean[4], rs[5], q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < 4; ++g) mean[g] = wave_sum(s[g]) * invH;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const bool v = lane + 64 * c < nchunk;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a[g][c][e] = v ? a[g][c][e] - mean[g] : 0.f;
        q[g] += a[g][c][e] * a[g][c][e];
      }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) rs[g] = 1.f / sqrtf(wave_sum(q[g]) * invH + kLnEps);
  // gates and the un-normalised new state c~ (kept in a[1], the candidate's registers)
  const float inv_keep = 1.f / p.keep;
  float ssum = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = lane + 64 * c;
    if (ch < nchunk) {
      float n[4][8], gm[8], bt[8], cprev[8];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        ld8(p.ln + (long long)(2 * g) * H + ch * 8, gm);
        ld8(p.ln + (long long)(2 * g + 1) * H + ch * 8, bt);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          a[g][c][e] *= rs[g];
          n[g][e] = gm[e] * a[g][c][e] + bt[e];
        }
        if (p.xhat) st8bf(p.xhat + row * (4 * H) + (long long)g * H + ch * 8, a[g][c]);
      }
      ld8(p.c32 + (long long)b * H + ch * 8, cprev);
      const uint32_t bits = p.keep < 1.f ? dropout_bits8(p.seed, (unsigned long long)(row * H + ch * 8) >> 3, p.keep)
                                         : 0xffu;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float cand = ((bits >> e) & 1u) ? tanhf(n[1][e]) * inv_keep : 0.f;
        const float ct = cprev[e] * sigmoidf_(n[2][e] + p.forget_bias) + sigmoidf_(n[0][e]) * cand;
        a[1][c][e] = ct;
        a[3][c][e] = sigmoidf_(n[3][e]);     // the output gate
        ssum += ct;
      }
    }
  }
  const float smean = wave_sum(ssum) * invH;
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const bool v = lane + 64 * c < nchunk;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      a[1][c][e] = v ? a[1][c][e] - smean : 0.f;
      sq += a[1][c][e] * a[1][c][e];
    }
  }
  rs[4] = 1.f / sqrtf(wave_sum(sq) * invH + kLnEps);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = lane + 64 * c;
    if (ch < nchunk) {
      float gm[8], bt[8], cn[8], hn[8];
      ld8(p.ln + (long long)8 * H + ch * 8, gm);
      ld8(p.ln + (long long)9 * H + ch * 8, bt);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a[1][c][e] *= rs[4];
        cn[e] = gm[e] * a[1][c][e] + bt[e];
        hn[e] = tanhf(cn[e]) * a[3][c][e];
      }
      if (p.shat) st8(p.shat + row * H + ch * 8, a[1][c]);
      st8(p.c32 + (long long)b * H + ch * 8, cn);
      st8(p.h32 + (long long)b * H + ch * 8, hn);
      st8bf(p.h16 + (long long)b * H + ch * 8, hn);
      st8bf(p.y + row * p.ldy + ch * 8, hn);
    }
  }
  if (p.rstd && lane == 0) {
#pragma unroll
    for (int g = 0; g < 5; ++g) p.rstd[row * 5 + g] = rs[g];
  }
}

// ---------------------------------------------------------------------------------------------- backward
struct LnProdBwdArgs {
  const bf16_t* whT;    // [H,4H]
  const bf16_t* dg;     // dgx rows of step s + 1: sample b at dg + b * ldg (zero rows past a length)
  long long ldg;
  float* dhp;           // [B,H] fp32: dgx[s + 1] . Wh
  int B, H;
};
// ROWS hidden units x 32 samples per workgroup, the reduction (4H) split over 8 waves; ROWS as in rnn.hip
template <int ROWS>
__global__ __launch_bounds__(64 * kLnWaves) void lnlstm_prod_bwd_kernel(LnProdBwdArgs p) {
  __shared__ float red[kLnWaves * (ROWS == 8 ? 4 : 16) * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int j0 = blockIdx.x * ROWS, b0 = blockIdx.y * 32;
  const int H = p.H, GH = 4 * p.H;
  const int b = b0 + l31, j = j0 + 8 * wave + 4 * lhi;
  const bool evalid = wave < ROWS / 8 && b < p.B && j < H;
  f32x16 accw;
#pragma unroll
  for (int e = 0; e < 16; ++e) accw[e] = 0.f;
  const bf16_t* wrow = (l31 < ROWS && j0 + l31 < H) ? p.whT + (long long)(j0 + l31) * GH : nullptr;
  const bf16_t* irow = b < p.B ? p.dg + (long long)b * p.ldg : nullptr;
  tile_gemm_prefetch<kLnWaves, 16>(wrow, irow, GH, accw, p.whT);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (ROWS == 8) tile_reduce_rows8<kLnWaves>(accw, red, acc);
  else tile_reduce_rows<kLnWaves>(accw, red, acc);
  if (!evalid) return;
  const f32x4 o = {acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<f32x4*>(p.dhp + (long long)b * H + j) = o;
}

struct LnCellBwdArgs {
  const bf16_t* dy; long long lddy;   // null: no gradient on y (zero)
  const float* dhp;     // [B,H] or null at the last step (nothing follows it)
  const bf16_t* xhat;   // [B,T,4H]
  const float* shat;    // [B,T,H]
  const float* rstd;    // [B,T,5]
  const float* c0;      // [B,H] or null
  const float* ln;      // [10,H]
  float* dcc;           // [B,H] gradient carried to c_{t-1}
  float* pgrad;         // [B,10,H] per-sample parameter gradients, rows as ln
  bf16_t* dgx;          // [B,T,4H]
  const int32_t* lens;
  int B, T, H, step;
  float forget_bias, keep;
  unsigned long long seed;
  const float* dhT;     // [B,H] or null: the gradient of the final h, entering at the sample's last live step (ST)
};

// ST: the instance for a call without dy or with dhT (os2s_lnlstm_layer_bwd_state). ST = false is the code of the
// plain backward: no test in front of the dy load, which would put one more memory round trip on every step of the
// language model's chain of dependent launches (0.9 us per launch at H = 896). The two instances contract their
// multiply-adds differently, so a state call that needs neither (dy given, no dhT) runs the plain one: its result is
// os2s_lnlstm_layer_bwd's bit for bit.
template <int NCH, bool ST>
__global__ __launch_bounds__(64) void lnlstm_cell_bwd_kernel(LnCellBwdArgs p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int H = p.H, nchunk = H >> 3;
  const int len = p.lens ? min(max(p.lens[b], 0), p.T) : p.T;
  if (p.step >= len) return;       // wave-uniform; dgx of the row is zero already, the carries stay
  const int t = p.step;
  const long long row = (long long)b * p.T + t;
  const float invH = 1.f / (float)H;
  const float inv_keep = 1.f / p.keep;
  float rs[5];
#pragma unroll
  for (int g = 0; g < 5; ++g) rs[g] = p.rstd[row * 5 + g];
  float xh[4][NCH][8], dx[4][NCH][8];   // xhat_g and gamma_g * d n_g
  float sh[NCH][8], ds[NCH][8];
  float r1 = 0.f, r2 = 0.f;
  // pass 1: activations, dh -> d c_t -> the state LayerNorm's two sums
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = lane + 64 * c;
    if (ch < nchunk) {
      float gm[8], bt[8], dyv[8], dh[8], dcarry[8], pg[8];
      float* pgb = p.pgrad + (long long)b * (10 * H) + ch * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) dh[e] = dyv[e] = 0.f;
      if (!ST || p.dy) ld8bf(p.dy + row * p.lddy + ch * 8, dyv);
      if (p.dhp) ld8(p.dhp + (long long)b * H + ch * 8, dh);
#pragma unroll
      for (int e = 0; e < 8; ++e) dh[e] += dyv[e];
      if (ST && p.dhT && t == len - 1) {    // wave-uniform. dhp of this step is zero for the sample (dgx[t + 1] is a dead row)
        float dT[8];
        ld8(p.dhT + (long long)b * H + ch * 8, dT);
#pragma unroll
        for (int e = 0; e < 8; ++e) dh[e] += dT[e];
      }
      ld8(p.dcc + (long long)b * H + ch * 8, dcarry);
      ld8(p.shat + row * H + ch * 8, sh[c]);
      ld8(p.ln + (long long)8 * H + ch * 8, gm);
      ld8(p.ln + (long long)9 * H + ch * 8, bt);
      // the output gate: n_o, o; xhat_o stays in xh[3], dx[3] = d n_o for now
      float go[8], bo[8];
      ld8bf(p.xhat + row * (4 * H) + (long long)3 * H + ch * 8, xh[3][c]);
      ld8(p.ln + (long long)6 * H + ch * 8, go);
      ld8(p.ln + (long long)7 * H + ch * 8, bo);
      float dgam[8], dbet[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float og = sigmoidf_(go[e] * xh[3][c][e] + bo[e]);
        const float tc = tanhf(gm[e] * sh[c][e] + bt[e]);
        dx[3][c][e] = dh[e] * tc * og * (1.f - og);
        const float dc = dh[e] * og * (1.f - tc * tc) + dcarry[e];
        dgam[e] = dc * sh[c][e];
        dbet[e] = dc;
        ds[c][e] = dc * gm[e];
        r1 += ds[c][e];
        r2 += ds[c][e] * sh[c][e];
      }
      ld8(pgb + (long long)8 * H, pg);
#pragma unroll
      for (int e = 0; e < 8; ++e) pg[e] += dgam[e];
      st8(pgb + (long long)8 * H, pg);
      ld8(pgb + (long long)9 * H, pg);
#pragma unroll
      for (int e = 0; e < 8; ++e) pg[e] += dbet[e];
      st8(pgb + (long long)9 * H, pg);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) { sh[c][e] = 0.f; ds[c][e] = 0.f; }
    }
  }
  const float m1 = wave_sum(r1) * invH, m2 = wave_sum(r2) * invH;
  // pass 2: d c~ -> the gates' d n_g, parameter gradients, the eight sums of the gate LayerNorms
  float g1[4] = {0.f, 0.f, 0.f, 0.f}, g2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = lane + 64 * c;
    if (ch < nchunk) {
      float gm[4][8], bt[8], cprev[8], pg[8];
      float* pgb = p.pgrad + (long long)b * (10 * H) + ch * 8;
      if (t > 0) {
        float gs[8], bs[8];
        ld8(p.shat + (row - 1) * H + ch * 8, cprev);
        ld8(p.ln + (long long)8 * H + ch * 8, gs);
        ld8(p.ln + (long long)9 * H + ch * 8, bs);
#pragma unroll
        for (int e = 0; e < 8; ++e) cprev[e] = gs[e] * cprev[e] + bs[e];
      } else if (p.c0) {
        ld8(p.c0 + (long long)b * H + ch * 8, cprev);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) cprev[e] = 0.f;
      }
      float n[3][8];
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        ld8bf(p.xhat + row * (4 * H) + (long long)g * H + ch * 8, xh[g][c]);
        ld8(p.ln + (long long)(2 * g) * H + ch * 8, gm[g]);
        ld8(p.ln + (long long)(2 * g + 1) * H + ch * 8, bt);
#pragma unroll
        for (int e = 0; e < 8; ++e) n[g][e] = gm[g][e] * xh[g][c][e] + bt[e];
      }
      ld8(p.ln + (long long)6 * H + ch * 8, gm[3]);
      const uint32_t bits = p.keep < 1.f ? dropout_bits8(p.seed, (unsigned long long)(row * H + ch * 8) >> 3, p.keep)
                                         : 0xffu;
      float dn[4][8], dcn[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float dct = rs[4] * (ds[c][e] - m1 - sh[c][e] * m2);
        const float ig = sigmoidf_(n[0][e]), tj = tanhf(n[1][e]), f = sigmoidf_(n[2][e] + p.forget_bias);
        const float mk = ((bits >> e) & 1u) ? inv_keep : 0.f;
        dn[0][e] = dct * tj * mk * ig * (1.f - ig);
        dn[1][e] = dct * ig * mk * (1.f - tj * tj);
        dn[2][e] = dct * cprev[e] * f * (1.f - f);
        dn[3][e] = dx[3][c][e];
        dcn[e] = dct * f;
      }
      st8(p.dcc + (long long)b * H + ch * 8, dcn);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        ld8(pgb + (long long)(2 * g) * H, pg);
#pragma unroll
        for (int e = 0; e < 8; ++e) pg[e] += dn[g][e] * xh[g][c][e];
        st8(pgb + (long long)(2 * g) * H, pg);
        ld8(pgb + (long long)(2 * g + 1) * H, pg);
#pragma unroll
        for (int e = 0; e < 8; ++e) pg[e] += dn[g][e];
        st8(pgb + (long long)(2 * g + 1) * H, pg);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          dx[g][c][e] = dn[g][e] * gm[g][e];
          g1[g] += dx[g][c][e];
          g2[g] += dx[g][c][e] * xh[g][c][e];
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    g1[g] = wave_sum(g1[g]) * invH;
    g2[g] = wave_sum(g2[g]) * invH;
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = lane + 64 * c;
    if (ch < nchunk) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float da[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) da[e] = rs[g] * (dx[g][c][e] - g1[g] - xh[g][c][e] * g2[g]);
        st8bf(p.dgx + row * (4 * H) + (long long)g * H + ch * 8, da);
      }
    }
  }
}

// dln[k][j] = sum over b, in order, of pgrad[b][k][j]
__global__ __launch_bounds__(256) void lnlstm_param_sum_kernel(const float* pgrad, float* dln, int B, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += pgrad[(long long)b * n + i];
  dln[i] = s;
}

// ---------------------------------------------------------------------------------------------- embedding
// tf.nn.embedding_lookup of a table whose ELEMENTS were dropped (encoders/lm_encoders.py:264: tf.nn.dropout on the
// [V,E] matrix, not on the looked-up rows): out[n, c] = table[id, c] * m[id, c] / keep, the mask indexed by
// (token id, column), so two occurrences of a token share one mask. DET: one thread per 8-column chunk walks the
// tokens in order (no atomics), as embed_bwd_det_kernel does.
__global__ __launch_bounds__(256) void embed_wdrop_fwd_kernel(const int32_t* __restrict__ ids,
                                                              const bf16_t* __restrict__ table, int V, int D,
                                                              long long N, float keep, unsigned long long seed,
                                                              bf16_t* __restrict__ out) {
  const int D8 = D >> 3;
  const float ik = 1.f / keep;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N * D8; i += (long long)gridDim.x * 256) {
    const long long n = i / D8;
    const int c0 = (int)(i - n * D8) * 8;
    const int id = min(max(ids[n], 0), V - 1);
    float v[8];
    ld8bf(table + (long long)id * D + c0, v);
    if (keep < 1.f) {
      const uint32_t bits = dropout_bits8(seed, (unsigned long long)((long long)id * D + c0) >> 3, keep);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = ((bits >> e) & 1u) ? v[e] * ik : 0.f;
    }
    st8bf(out + n * D + c0, v);
  }
}

template <bool DET>
__global__ __launch_bounds__(256) void embed_wdrop_bwd_kernel(const int32_t* __restrict__ ids,
                                                              const bf16_t* __restrict__ dout, int V, int D,
                                                              long long N, float keep, unsigned long long seed,
                                                              float* __restrict__ dtable) {
  const int D8 = D >> 3;
  const float ik = 1.f / keep;
  const long long first = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long count = DET ? (first < D8 ? N : 0) : N * D8;
  for (long long k = DET ? 0 : first; k < count; k += DET ? 1 : (long long)gridDim.x * 256) {
    const long long n = DET ? k : k / D8;
    const int c0 = (int)(DET ? first : k - n * D8) * 8;
    const int id = min(max(ids[n], 0), V - 1);
    float g[8];
    ld8bf(dout + n * D + c0, g);
    const uint32_t bits = keep < 1.f ? dropout_bits8(seed, (unsigned long long)((long long)id * D + c0) >> 3, keep)
                                     : 0xffu;
    float* const row = dtable + (long long)id * D + c0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = ((bits >> e) & 1u) ? g[e] * (keep < 1.f ? ik : 1.f) : 0.f;
      if (x == 0.f) continue;
      if (DET) row[e] += x;
      else __hip_atomic_fetch_add(row + e, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace os2s

using namespace os2s;

static bool lnlstm_shape_ok(int B, int T, int H) { return B >= 1 && T >= 1 && H >= 8 && H <= 2048 && H % 8 == 0; }
static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// h16 [B,H] bf16 + pre [B,4H] + h32 [B,H] + c32 [B,H] fp32
extern "C" size_t os2s_lnlstm_fwd_workspace_bytes(int B, int H) {
  const size_t bh = (size_t)B * H;
  return align256(bh * 2) + align256(bh * 16) + 2 * align256(bh * 4);
}

extern "C" int os2s_lnlstm_layer_fwd(os2s_stream_t stream_, const uint16_t* gx, const uint16_t* wh, const float* ln,
                                     const int32_t* lens, int B, int T, int H, float forget_bias, float keep_prob,
                                     unsigned long long seed, const float* h0, const float* c0, uint16_t* y,
                                     long long ldy, uint16_t* xhat, float* s_hat, float* rstd, float* hT, float* cT,
                                     void* workspace, size_t workspace_bytes) {
  OS2S_REQUIRE(gx && wh && ln && y && workspace && B >= 1 && T >= 1 && H >= 1);
  OS2S_REQUIRE(keep_prob > 0.f && keep_prob <= 1.f);
  if (!lnlstm_shape_ok(B, T, H)) return OS2S_ERR_UNSUPPORTED;
  OS2S_REQUIRE(ldy >= H && ldy % 8 == 0);
  if (workspace_bytes < os2s_lnlstm_fwd_workspace_bytes(B, H)) return OS2S_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t bh = (size_t)B * H;
  char* ws = (char*)workspace;
  bf16_t* h16 = (bf16_t*)ws; ws += align256(bh * 2);
  float* pre = (float*)ws; ws += align256(bh * 16);
  float* h32 = (float*)ws; ws += align256(bh * 4);
  float* c32 = (float*)ws;
  if (lens && hipMemset2DAsync(y, (size_t)ldy * 2, 0, (size_t)H * 2, (size_t)B * T, stream) != hipSuccess)
    return OS2S_ERR_LAUNCH;
  LnInitArgs ia;
  ia.h0 = h0; ia.c0 = c0; ia.h32 = h32; ia.c32 = c32; ia.h16 = h16; ia.n = (long long)bh;
  OS2S_LAUNCH(lnlstm_init_kernel, dim3(ceil_div((long long)bh, 256)), dim3(256), 0, stream, ia);
  LnProdFwdArgs pa;
  pa.gx = (const bf16_t*)gx; pa.wh = (const bf16_t*)wh; pa.h16 = h16; pa.pre = pre; pa.lens = lens;
  pa.B = B; pa.T = T; pa.H = H;
  LnCellFwdArgs ca;
  ca.pre = pre; ca.ln = ln; ca.h32 = h32; ca.c32 = c32; ca.h16 = h16; ca.y = (bf16_t*)y; ca.ldy = ldy;
  ca.xhat = (bf16_t*)xhat; ca.shat = s_hat; ca.rstd = rstd; ca.lens = lens;
  ca.B = B; ca.T = T; ca.H = H; ca.forget_bias = forget_bias; ca.keep = keep_prob; ca.seed = seed;
  const dim3 pgrid(H / 8, ceil_div(B, 32));
  for (int s = 0; s < T; ++s) {
    pa.step = ca.step = s;
    OS2S_LAUNCH(lnlstm_prod_fwd_kernel, pgrid, dim3(64 * kLnWaves), 0, stream, pa);
    if (H <= 512) { OS2S_LAUNCH(lnlstm_cell_fwd_kernel<1>, dim3(B), dim3(64), 0, stream, ca); }
    else if (H <= 1024) { OS2S_LAUNCH(lnlstm_cell_fwd_kernel<2>, dim3(B), dim3(64), 0, stream, ca); }
    else { OS2S_LAUNCH(lnlstm_cell_fwd_kernel<4>, dim3(B), dim3(64), 0, stream, ca); }
  }
  if (hT && hipMemcpyAsync(hT, h32, bh * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess) return OS2S_ERR_LAUNCH;
  if (cT && hipMemcpyAsync(cT, c32, bh * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess) return OS2S_ERR_LAUNCH;
  return OS2S_OK;
}

// dhp [B,H] + dcc [B,H] + pgrad [B,10,H] fp32
extern "C" size_t os2s_lnlstm_bwd_workspace_bytes(int B, int H) {
  const size_t bh = (size_t)B * H;
  return 2 * align256(bh * 4) + align256(bh * 40);
}

// Both backward entries; state: the call of os2s_lnlstm_layer_bwd_state, where dy may be null; dhT / dcT [B,H] fp32 or null: the gradients of the forward's hT / cT.
// cT[b] is the carried (normalised) state after the sample's last live step, so dcT is the initial value of the dcc
// carry, which the dead steps before it leave alone; hT[b] is that step's h, so the cell kernel adds dhT there.
static int lnlstm_layer_bwd_impl(os2s_stream_t stream_, const uint16_t* whT, const float* ln, const int32_t* lens,
                                 const uint16_t* dy, long long lddy, bool state, const float* dhT,
                                 const float* dcT, const uint16_t* xhat, const float* s_hat, const float* rstd,
                                 const float* c0, int B, int T, int H, float forget_bias, float keep_prob,
                                 unsigned long long seed, uint16_t* dgx, float* dln, void* workspace,
                                 size_t workspace_bytes) {
  OS2S_REQUIRE(state || (dy && !dhT && !dcT));
  const bool st = !dy || dhT;       // dcT alone is the carry's initial value: no kernel support needed
  OS2S_REQUIRE(whT && ln && xhat && s_hat && rstd && dgx && dln && workspace && B >= 1 && T >= 1 && H >= 1);
  OS2S_REQUIRE(keep_prob > 0.f && keep_prob <= 1.f);
  if (!lnlstm_shape_ok(B, T, H)) return OS2S_ERR_UNSUPPORTED;
  OS2S_REQUIRE(!dy || (lddy >= H && lddy % 8 == 0));
  const size_t need = os2s_lnlstm_bwd_workspace_bytes(B, H);
  if (workspace_bytes < need) return OS2S_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t bh = (size_t)B * H;
  char* ws = (char*)workspace;
  float* dhp = (float*)ws; ws += align256(bh * 4);
  float* dcc = (float*)ws; ws += align256(bh * 4);
  float* pgrad = (float*)ws;
  if (hipMemsetAsync(workspace, 0, need, stream) != hipSuccess) return OS2S_ERR_LAUNCH;
  if (dcT && hipMemcpyAsync(dcc, dcT, bh * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess) return OS2S_ERR_LAUNCH;
  // gate gradients of frames past the sequence ends are zero (and are what the step before a sample's last reads)
  if (hipMemsetAsync(dgx, 0, (size_t)B * T * 4 * H * 2, stream) != hipSuccess) return OS2S_ERR_LAUNCH;
  LnProdBwdArgs pa;
  pa.whT = (const bf16_t*)whT; pa.ldg = (long long)T * 4 * H; pa.dhp = dhp; pa.B = B; pa.H = H;
  LnCellBwdArgs ca;
  ca.dy = (const bf16_t*)dy; ca.lddy = lddy; ca.dhT = dhT; ca.xhat = (const bf16_t*)xhat; ca.shat = s_hat; ca.rstd = rstd;
  ca.c0 = c0; ca.ln = ln; ca.dcc = dcc; ca.pgrad = pgrad; ca.dgx = (bf16_t*)dgx; ca.lens = lens;
  ca.B = B; ca.T = T; ca.H = H; ca.forget_bias = forget_bias; ca.keep = keep_prob; ca.seed = seed;
  const bool rows8 = ceil_div(H, 32) * ceil_div(B, 32) < 128;
  const dim3 pgrid(ceil_div(H, rows8 ? 8 : 32), ceil_div(B, 32));
  for (int s = T - 1; s >= 0; --s) {
    ca.step = s;
    ca.dhp = nullptr;
    if (s < T - 1) {
      pa.dg = (const bf16_t*)dgx + (long long)(s + 1) * 4 * H;
      ca.dhp = dhp;
      if (rows8) { OS2S_LAUNCH(lnlstm_prod_bwd_kernel<8>, pgrid, dim3(64 * kLnWaves), 0, stream, pa); }
      else { OS2S_LAUNCH(lnlstm_prod_bwd_kernel<32>, pgrid, dim3(64 * kLnWaves), 0, stream, pa); }
    }
    if (st) {
      if (H <= 512) { OS2S_LAUNCH((lnlstm_cell_bwd_kernel<1, true>), dim3(B), dim3(64), 0, stream, ca); }
      else if (H <= 1024) { OS2S_LAUNCH((lnlstm_cell_bwd_kernel<2, true>), dim3(B), dim3(64), 0, stream, ca); }
      else { OS2S_LAUNCH((lnlstm_cell_bwd_kernel<4, true>), dim3(B), dim3(64), 0, stream, ca); }
    } else {
      if (H <= 512) { OS2S_LAUNCH((lnlstm_cell_bwd_kernel<1, false>), dim3(B), dim3(64), 0, stream, ca); }
      else if (H <= 1024) { OS2S_LAUNCH((lnlstm_cell_bwd_kernel<2, false>), dim3(B), dim3(64), 0, stream, ca); }
      else { OS2S_LAUNCH((lnlstm_cell_bwd_kernel<4, false>), dim3(B), dim3(64), 0, stream, ca); }
    }
  }
  OS2S_LAUNCH(lnlstm_param_sum_kernel, dim3(ceil_div(10 * H, 256)), dim3(256), 0, stream, (const float*)pgrad, dln, B,
              10 * H);
  return OS2S_OK;
}

extern "C" int os2s_lnlstm_layer_bwd(os2s_stream_t stream, const uint16_t* whT, const float* ln, const int32_t* lens,
                                     const uint16_t* dy, long long lddy, const uint16_t* xhat, const float* s_hat,
                                     const float* rstd, const float* c0, int B, int T, int H, float forget_bias,
                                     float keep_prob, unsigned long long seed, uint16_t* dgx, float* dln,
                                     void* workspace, size_t workspace_bytes) {
  return lnlstm_layer_bwd_impl(stream, whT, ln, lens, dy, lddy, false, nullptr, nullptr, xhat, s_hat, rstd, c0, B, T, H,
                               forget_bias, keep_prob, seed, dgx, dln, workspace, workspace_bytes);
}

extern "C" int os2s_lnlstm_layer_bwd_state(os2s_stream_t stream, const uint16_t* whT, const float* ln,
                                           const int32_t* lens, const uint16_t* dy, long long lddy, const float* dhT,
                                           const float* dcT, const uint16_t* xhat, const float* s_hat,
                                           const float* rstd, const float* c0, int B, int T, int H, float forget_bias,
                                           float keep_prob, unsigned long long seed, uint16_t* dgx, float* dln,
                                           void* workspace, size_t workspace_bytes) {
  return lnlstm_layer_bwd_impl(stream, whT, ln, lens, dy, lddy, true, dhT, dcT, xhat, s_hat, rstd, c0, B, T, H, forget_bias,
                               keep_prob, seed, dgx, dln, workspace, workspace_bytes);
}

extern "C" int os2s_embed_wdrop_fwd(os2s_stream_t stream, const int32_t* ids, const uint16_t* table, int V, int D,
                                    long long N, float keep_prob, unsigned long long seed, uint16_t* out) {
  OS2S_REQUIRE(ids && table && out && V >= 1 && D >= 8 && D % 8 == 0 && N >= 0);
  OS2S_REQUIRE(keep_prob > 0.f && keep_prob <= 1.f);
  if (N == 0) return OS2S_OK;
  const long long blocks = (N * (D / 8) + 255) / 256;
  OS2S_LAUNCH(embed_wdrop_fwd_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
              (hipStream_t)stream, ids, (const bf16_t*)table, V, D, N, keep_prob, seed, (bf16_t*)out);
  return OS2S_OK;
}

extern "C" int os2s_embed_wdrop_bwd(os2s_stream_t stream, const int32_t* ids, const uint16_t* dout, int V, int D,
                                    long long N, float keep_prob, unsigned long long seed, float* dtable) {
  OS2S_REQUIRE(ids && dout && dtable && V >= 1 && D >= 8 && D % 8 == 0 && N >= 0);
  OS2S_REQUIRE(keep_prob > 0.f && keep_prob <= 1.f);
  if (N == 0) return OS2S_OK;
  if (os2s_deterministic()) {
    OS2S_LAUNCH(embed_wdrop_bwd_kernel<true>, dim3(ceil_div(D / 8, 256)), dim3(256), 0, (hipStream_t)stream, ids,
                (const bf16_t*)dout, V, D, N, keep_prob, seed, dtable);
    return OS2S_OK;
  }
  const long long blocks = (N * (D / 8) + 255) / 256;
  OS2S_LAUNCH(embed_wdrop_bwd_kernel<false>, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
              (hipStream_t)stream, ids, (const bf16_t*)dout, V, D, N, keep_prob, seed, dtable);
  return OS2S_OK;
}
