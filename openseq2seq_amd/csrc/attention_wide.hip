// Dense cross-attention with one head as wide as the hidden state (Centaur's decoder -> encoder attention,
// attention_heads = 1, hidden_size = 512): Attention.call, mode "loung"
// (parts/transformer/attention_layer.py:104-220), restated for the dense padded layout.
//
//   q [B, Tq, H*D], k / v [B, S, H*D] bf16, head h owns channels [h*D, (h+1)*D); key_bias [B, S] fp32;
//   logits = scale * q k^T (fp32) + bias; p = softmax over the S keys (fp32, WRITTEN: it is the model's alignment
//   and what the backward reads); o = dropout(p) v.
//   bias = key_bias, or with `positions` max(key_bias + window mask, -1e9) (:166-187), the window mask of query t
//   being 0 for keys in [w, w + window), w = max(positions[b, h, t] - back_step, 0), and -1e9 elsewhere: an ADDITIVE
//   fp32 bias, so a row whose window lies wholly past the real keys degenerates to the reference's near-uniform row
//   and never to NaN. The reference applies the window only when its logits are fp32 (:154-187); ours always are,
//   so the window applies whenever it is configured.
//
// What differs from attention.hip: that family stops at a head dim of 128, works on the packed variable-length
// layout and never materialises the probabilities. Here the head dim goes to 512, the batch is dense (Centaur's
// BatchNorm statistics and convolutions see the padding, so packing would buy nothing) and p is an output.
//
// Tiling. A workgroup of 4 waves owns 64 query rows of one (b, h); a wave owns 16 of them. All products are
// v_mfma_f32_16x16x32_bf16.
//   1. strip = x y^T (forward: q k^T, backward: dO v^T): the wave keeps its 16 x D x-fragments in registers
//      (D / 32 fragments) and walks the 16-key tiles, y-fragments straight from global memory (a lane's 8 reduction
//      elements are 16 contiguous bytes of a row), the next tile's loads in flight under this tile's MFMAs. The
//      64 x S fp32 strip stays in LDS.
//   2. row pass, one wave per row (two rows, one per 32-lane half, when S <= 256), a lane per 8 consecutive keys:
//      forward = bias, softmax, p out, argmax, dropout; backward = dS = p o (dPd - delta). The bf16 operand of
//      step 3 is written IN PLACE over the head of the same strip row (the whole row is in registers by then).
//      Rows past Tq are skipped.
//   3. out^T = z^T img^T (forward: o = Pd v, backward: dq = scale dS k) in column chunks of min(D, 128), so the
//      accumulator is 32 VGPRs per lane at any D. z is staged 32 keys at a time into a row-major LDS image (two
//      images taking turns, the tiles of the next four steps in flight in registers: a workgroup is one latency
//      chain, and at Centaur's shapes a launch is one workgroup per CU) and consumed through ds_read_b64_tr_b16; the
//      transposed orientation leaves a lane 4 consecutive channels of one query (8-byte stores).
// LDS = 64 (Sp + 4) * 4 + 2 * 32 (DC + 4) * 2 bytes, Sp = S rounded up to 32: 65 KB at S = 184, 146 KB at the limit
// S = 512 (64 KB and more: through the large-LDS launch path).
//
// Backward, no atomics, bitwise reproducible: launch 1 (the kernel above with kBwd) owns dq per 64-query tile and
// leaves dS (bf16, unscaled) in a [B, H, Tq, S] workspace; launch 2 owns dk and dv per (64-key tile, column chunk)
// and walks the queries 32 at a time: dv^T = dO^T Pd, dk^T = scale q^T dS, Pd rebuilt from p and the mask.
// The bias and the window take no gradient.
//
// Rounding points (everything else fp32): q, k, v, dO are bf16 inputs; Pd = p o m / keep is rounded to bf16 for
// P.V and for dV; dS is rounded to bf16 for dQ and dK (scale is applied to the fp32 sums); o, dq, dk, dv are bf16.
//
// Dropout mask: element ((b*H + h)*Tq + t)*S + key of the generator behind os2s_dropout_mask.
#include <type_traits>

#include "os2s_common.hpp"

namespace os2s {
namespace {

constexpr int kWideRows = 64;       // query rows of a workgroup
constexpr int kWideMaxS = 512;      // a lane of the row pass owns 8 keys
constexpr int kWideKc = 32;         // keys (forward / dq) or queries (dk, dv) staged per step
constexpr int kWideRing = 4;        // z tiles in flight in step 3 (even: the two LDS images alternate)
constexpr float kNegBias = -1e9f;

struct WideArgs {
  const bf16_t *x, *y, *z;          // forward: q, k, v; backward launch 1: dO, v, k
  bf16_t* out;                      // o / dq
  float* p;                         // forward: written; backward: read
  const float* key_bias;
  const int32_t* positions;
  int32_t* argmax;
  bf16_t* ds;                       // backward: dS workspace
  int B, H, Tq, S, Sp;
  long long ldx, ldy, ldz, ldo;
  int window, back_step;
  float scale, keep_prob;
  unsigned long long seed;
};

__device__ __forceinline__ bf16x8 ld_frag(const bf16_t* p, bool ok) {
  bf16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
  if (ok) r = *reinterpret_cast<const bf16x8*>(p);
  return r;
}

// operand[m][k], m = m0 + (lane & 15), k = 8 (lane >> 4) + 0..7, from a row-major LDS image [k][m] of `ld`
// elements per row (ld * 2 a multiple of 8): two transposed 4 x 16 block reads per 16-lane group
__device__ __forceinline__ bf16x8 frag_col(const bf16_t* img, int ld, int m0, int lane) {
  const int i16 = lane & 15;
  const bf16_t* a = img + (8 * (lane >> 4) + (i16 >> 2)) * ld + m0 + (i16 & 3) * 4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)a);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(a + 4 * ld));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// 8 bf16 into an image row whose start is only 8-byte aligned
__device__ __forceinline__ void st_img8(bf16_t* dst, const u32x4& v) {
  u32x2 a = {v[0], v[1]}, b = {v[2], v[3]};
  *reinterpret_cast<u32x2*>(dst) = a;
  *reinterpret_cast<u32x2*>(dst + 4) = b;
}

// the keep bits of the 8 elements that start at element index e0 (a multiple of 8)
__device__ __forceinline__ uint32_t wide_keep8(unsigned long long seed, long long e0, uint32_t thr) {
  const unsigned long long z0 = (unsigned long long)(e0 >> 2) * kDropGolden + seed;
  return dropout_bits4_z(z0, thr) | (dropout_bits4_z(z0 + kDropGolden, thr) << 4);
}

// Row reductions of FULLY ACTIVE waves (the DPP steps of wave_sum_dpp / wave_max_dpp): over the wave, or with `half`
// over each 32-lane half, whose result sits in lanes 31 and 63 after the row_bcast:15 step.
__device__ __forceinline__ float wide_row_sum(float x, bool half, int lane) {
  x += dpp_mov<0xB1, 0xf>(0.f, x);
  x += dpp_mov<0x4E, 0xf>(0.f, x);
  x += dpp_mov<0x124, 0xf>(0.f, x);
  x += dpp_mov<0x128, 0xf>(0.f, x);
  x += dpp_mov<0x142, 0xa>(0.f, x);
  const float lo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 31));
  const float hi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
  return half ? (lane < 32 ? lo : hi) : lo + hi;
}
__device__ __forceinline__ float wide_row_max(float x, bool half, int lane) {
  const float ninf = -__builtin_inff();
  x = fmaxf(x, dpp_mov<0xB1, 0xf>(ninf, x));
  x = fmaxf(x, dpp_mov<0x4E, 0xf>(ninf, x));
  x = fmaxf(x, dpp_mov<0x124, 0xf>(ninf, x));
  x = fmaxf(x, dpp_mov<0x128, 0xf>(ninf, x));
  x = fmaxf(x, dpp_mov<0x142, 0xa>(ninf, x));
  const float lo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 31));
  const float hi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
  return half ? (lane < 32 ? lo : hi) : fmaxf(lo, hi);
}

template <int D, bool kBwd>
__global__ __launch_bounds__(256) void attn_wide_kernel(const WideArgs a) {
  constexpr int DC = D < 128 ? D : 128, NT = DC / 16, ZLD = DC + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int sld = a.Sp + 4;                                   // strip row, in floats
  float* strip = reinterpret_cast<float*>(smem);
  bf16_t* zimg = reinterpret_cast<bf16_t*>(smem + (size_t)kWideRows * sld * 4);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y, t0 = blockIdx.x * kWideRows;
  const int l15 = lane & 15, lg = lane >> 4;
  const int S = a.S, Tq = a.Tq;
  const bf16_t* xb = a.x + ((long long)b * Tq + t0) * a.ldx + h * D;
  const bf16_t* yb = a.y + (long long)b * S * a.ldy + h * D;
  const bf16_t* zb = a.z + (long long)b * S * a.ldz + h * D;
  const long long bh = (long long)b * a.H + h;

  // ---- 1. strip = x y^T
  {
    bf16x8 xf[D / 32];
    const int xr = w * 16 + l15;
    const bool xok = t0 + xr < Tq;
#pragma unroll
    for (int i = 0; i < D / 32; ++i) xf[i] = ld_frag(xb + (long long)xr * a.ldx + i * 32 + 8 * lg, xok);
    const int ntn = (S + 15) >> 4;
    bf16x8 yf[D / 32], yn[D / 32];                            // this key tile's fragments and the next one's
    const bf16_t* yr = yb + (long long)l15 * a.ldy + 8 * lg;
#pragma unroll
    for (int i = 0; i < D / 32; ++i) yf[i] = ld_frag(yr + i * 32, l15 < S);
    for (int nt = 0; nt < ntn; ++nt) {
      const int key = nt * 16 + l15;
      const bool nok = key + 16 < S;                          // also false past the last tile
#pragma unroll
      for (int i = 0; i < D / 32; ++i) yn[i] = ld_frag(yr + ((long long)(nt + 1) * 16) * a.ldy + i * 32, nok);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < D / 32; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[i], yf[i], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) strip[(w * 16 + lg * 4 + r) * sld + key] = acc[r];
#pragma unroll
      for (int i = 0; i < D / 32; ++i) yf[i] = yn[i];
    }
  }
  __syncthreads();

  // ---- 2. row pass: lane owns keys c0 .. c0 + 7 of one row at a time. S <= 256 (every LJSpeech line): a row fits
  // half a wave, so the wave takes two rows at a time, the reductions staying inside the 32-lane halves
  {
    const bool two = S <= 256;
    const int c0 = (two ? lane & 31 : lane) * 8, sub = two ? lane >> 5 : 0, nrr = two ? 8 : 16;
    const bool cv = c0 < S;
    const bool drop = a.keep_prob < 1.f;
    const uint32_t thr = (uint32_t)(a.keep_prob * 65536.0f);
    const float ik = 1.f / a.keep_prob;
    float kb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) kb[e] = 0.f;
    if (!kBwd && cv) load8(a.key_bias + (long long)b * S + c0, kb);
    for (int rr = 0; rr < nrr; ++rr) {
      const int row = w * 16 + (two ? 2 * rr + sub : rr), t = t0 + row;
      const bool tv = t < Tq;
      const long long e0 = (bh * Tq + t) * S + c0;
      if (t0 + w * 16 + (two ? 2 * rr : rr) >= Tq) {          // no live row in this round (wave-uniform): zeros
        const u32x4 zero = {0u, 0u, 0u, 0u};
        if (c0 < a.Sp) *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(strip + row * sld) + c0 * 2) = zero;
        continue;
      }
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
      if (cv) load8(strip + row * sld + c0, v);
      uint32_t keep = 0xffu;
      if (drop && cv && tv) keep = wide_keep8(a.seed, e0, thr);
      float w8[8];                                           // what goes into the step-3 image
      if (!kBwd) {
        int wlo = 0, whi = 0x7fffffff;
        const bool win = a.positions != nullptr;
        if (win) {
          const int pos = a.positions[bh * Tq + (tv ? t : Tq - 1)];
          wlo = pos - a.back_step > 0 ? pos - a.back_step : 0;
          whi = wlo + a.window;
        }
        float mx = -__builtin_inff();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float bias = kb[e];
          if (win) bias = fmaxf(bias + ((c0 + e >= wlo && c0 + e < whi) ? 0.f : kNegBias), kNegBias);
          v[e] = cv ? a.scale * v[e] + bias : -__builtin_inff();
          mx = fmaxf(mx, v[e]);
        }
        mx = wide_row_max(mx, two, lane);
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[e] = cv ? __expf(v[e] - mx) : 0.f; sum += v[e]; }
        sum = wide_row_sum(sum, two, lane);
        const float inv = 1.f / sum;
        float bv = -1.f;
        int bi = 0x7fffffff;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] *= inv;
          if (cv && v[e] > bv) { bv = v[e]; bi = c0 + e; }
          w8[e] = ((keep >> e) & 1u) ? (drop ? v[e] * ik : v[e]) : 0.f;
        }
        if (a.argmax != nullptr) {
          for (int o = two ? 16 : 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
          }
          if (c0 == 0 && tv) a.argmax[bh * Tq + t] = bi;
        }
        if (cv && tv) {
          f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
          *reinterpret_cast<f32x4*>(a.p + e0) = lo;
          *reinterpret_cast<f32x4*>(a.p + e0 + 4) = hi;
        }
      } else {
        float pv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) pv[e] = 0.f;
        if (cv && tv) load8(a.p + e0, pv);
        float delta = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = ((keep >> e) & 1u) ? (drop ? v[e] * ik : v[e]) : 0.f;      // dPd o m / keep
          delta += pv[e] * v[e];
        }
        delta = wide_row_sum(delta, two, lane);
#pragma unroll
        for (int e = 0; e < 8; ++e) w8[e] = pv[e] * (v[e] - delta);
      }
      const u32x4 packed = pack8(w8);
      if (kBwd && cv && tv) *reinterpret_cast<u32x4*>(a.ds + e0) = packed;
      // in place: every lane's floats of this row are in registers (LDS serves a wave's accesses in order)
      if (c0 < a.Sp) *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(strip + row * sld) + c0 * 2) = packed;
    }
  }

  // ---- 3. out^T[d][q] = sum_key z[key][d] img[q][key], a column chunk of DC at a time. One step = 32 keys of one
  // chunk. The z tiles of the next kWideRing steps are on their way to registers while this one's MFMAs run, and the
  // two LDS images take turns, so a step has one barrier (a wave that overwrites an image has passed the barrier of
  // the step in between, which every wave reaches only after its reads of that image)
  const float mul = kBwd ? a.scale : 1.f;
  const int qr = w * 16 + l15;
  const bf16_t* prow = reinterpret_cast<const bf16_t*>(strip + qr * sld) + 8 * lg;
  constexpr int NU = (kWideKc * DC / 8 + 255) / 256;          // 16-byte pieces of a z tile per thread
  const int nkc = a.Sp / kWideKc, nsteps = (D / DC) * nkc;
  bf16x8 stage[kWideRing][NU];                                // tiles on their way: a step is far shorter than a load
  auto fetch = [&](int step, bf16x8 (&st)[NU]) {
    const int dc = step / nkc, kc = step % nkc;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int u = tid + i * 256, r = u / (DC / 8), c8 = u % (DC / 8), key = kc * kWideKc + r;
      st[i] = ld_frag(zb + (long long)key * a.ldz + dc * DC + c8 * 8,
                      step < nsteps && u < kWideKc * DC / 8 && key < S);
    }
  };
#pragma unroll
  for (int j = 0; j < kWideRing; ++j) fetch(j, stage[j]);
  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int step0 = 0; step0 < nsteps; step0 += kWideRing) {
#pragma unroll
    for (int j = 0; j < kWideRing; ++j) {                     // static ring slot j, static image j & 1
      const int step = step0 + j;
      if (step >= nsteps) break;
      bf16_t* img = zimg + (j & 1) * (kWideKc * ZLD);
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        const int u = tid + i * 256, r = u / (DC / 8), c8 = u % (DC / 8);
        if (u < kWideKc * DC / 8) st_img8(img + r * ZLD + c8 * 8, __builtin_bit_cast(u32x4, stage[j][i]));
      }
      __syncthreads();                                       // step 0: the row pass is done as well
      fetch(step + kWideRing, stage[j]);
      const int dc = step / nkc, kc = step % nkc;
      const bf16x8 pf = *reinterpret_cast<const bf16x8*>(prow + kc * kWideKc);
#pragma unroll
      for (int n = 0; n < NT; ++n)
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_col(img, ZLD, n * 16, lane), pf, acc[n], 0, 0, 0);
      if (kc == nkc - 1) {
        if (t0 + qr < Tq) {
          bf16_t* orow = a.out + ((long long)b * Tq + t0 + qr) * a.ldo + h * D + dc * DC + lg * 4;
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            u32x2 o2 = {pack2bf(acc[n][0] * mul, acc[n][1] * mul), pack2bf(acc[n][2] * mul, acc[n][3] * mul)};
            *reinterpret_cast<u32x2*>(orow + n * 16) = o2;
          }
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
}

struct WideKvArgs {
  const bf16_t *q, *d_o, *ds;
  const float* p;
  bf16_t *dk, *dv;
  int B, H, Tq, S;
  long long ldq, lddo, lddk, lddv;
  float scale, keep_prob;
  unsigned long long seed;
};

// dv^T[d][key] = sum_q dO[q][d] Pd[q][key], dk^T[d][key] = scale sum_q q[q][d] dS[q][key]: one workgroup per
// (64-key tile, column chunk of DC, head, batch), a wave per 16 keys, 32 queries per step
template <int D>
__global__ __launch_bounds__(256) void attn_wide_dkv_kernel(const WideKvArgs a) {
  constexpr int DC = D < 128 ? D : 128, NT = DC / 16, ZLD = DC + 4, PLD = 64 + 4, NDC = D / DC;
  constexpr int kSet = 2 * kWideKc * PLD + 2 * kWideKc * ZLD;      // pd, dS, dO, q images of one step
  constexpr int NU = (kWideKc * DC / 8 + 255) / 256;
  __shared__ __attribute__((aligned(16))) bf16_t imgs[2 * kSet];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kt = blockIdx.x / NDC, dc = blockIdx.x % NDC, h = blockIdx.y, b = blockIdx.z;
  const int S = a.S, Tq = a.Tq, l15 = lane & 15, lg = lane >> 4;
  const long long bh = (long long)b * a.H + h;
  const bf16_t* qb = a.q + (long long)b * Tq * a.ldq + h * D + dc * DC;
  const bf16_t* dob = a.d_o + (long long)b * Tq * a.lddo + h * D + dc * DC;
  const bool drop = a.keep_prob < 1.f;
  const uint32_t thr = (uint32_t)(a.keep_prob * 65536.0f);
  const float ik = 1.f / a.keep_prob;
  const int pr = tid >> 3, pc = (tid & 7) * 8, pkey = kt * 64 + pc;     // this thread's piece of the p / dS images

  // the next step's pieces travel to registers under this step's MFMAs; the two image sets take turns (one barrier
  // a step, as in attn_wide_kernel)
  float pv[8];
  bf16x8 dsr, dor[NU], qrr[NU];
  auto fetch = [&](int q0) {
    const int t = q0 + pr;
    const bool ok = t < Tq && pkey < S;
    const long long e0 = (bh * Tq + t) * S + pkey;
#pragma unroll
    for (int e = 0; e < 8; ++e) pv[e] = 0.f;
    if (ok) load8(a.p + e0, pv);
    dsr = ld_frag(a.ds + e0, ok);
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int u = tid + i * 256, r = u / (DC / 8), c8 = u % (DC / 8), tt = q0 + r;
      const bool uok = u < kWideKc * DC / 8 && tt < Tq;
      dor[i] = ld_frag(dob + (long long)tt * a.lddo + c8 * 8, uok);
      qrr[i] = ld_frag(qb + (long long)tt * a.ldq + c8 * 8, uok);
    }
  };
  fetch(0);
  f32x4 dv[NT], dk[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) { dv[n] = f32x4{0.f, 0.f, 0.f, 0.f}; dk[n] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  int set = 0;
  for (int q0 = 0; q0 < Tq; q0 += kWideKc, set ^= 1) {
    bf16_t* pd_img = imgs + set * kSet;
    bf16_t* ds_img = pd_img + kWideKc * PLD;
    bf16_t* do_img = ds_img + kWideKc * PLD;
    bf16_t* q_img = do_img + kWideKc * ZLD;
    if (drop && q0 + pr < Tq && pkey < S) {
      const uint32_t keep = wide_keep8(a.seed, (bh * Tq + q0 + pr) * S + pkey, thr);
#pragma unroll
      for (int e = 0; e < 8; ++e) pv[e] = ((keep >> e) & 1u) ? pv[e] * ik : 0.f;
    }
    st_img8(pd_img + pr * PLD + pc, pack8(pv));
    st_img8(ds_img + pr * PLD + pc, __builtin_bit_cast(u32x4, dsr));
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int u = tid + i * 256, r = u / (DC / 8), c8 = u % (DC / 8);
      if (u < kWideKc * DC / 8) {
        st_img8(do_img + r * ZLD + c8 * 8, __builtin_bit_cast(u32x4, dor[i]));
        st_img8(q_img + r * ZLD + c8 * 8, __builtin_bit_cast(u32x4, qrr[i]));
      }
    }
    __syncthreads();
    if (q0 + kWideKc < Tq) fetch(q0 + kWideKc);
    const bf16x8 fpd = frag_col(pd_img, PLD, w * 16, lane), fds = frag_col(ds_img, PLD, w * 16, lane);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      dv[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_col(do_img, ZLD, n * 16, lane), fpd, dv[n], 0, 0, 0);
      dk[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_col(q_img, ZLD, n * 16, lane), fds, dk[n], 0, 0, 0);
    }
  }
  const int key = kt * 64 + w * 16 + l15;
  if (key < S) {
    bf16_t* vrow = a.dv + ((long long)b * S + key) * a.lddv + h * D + dc * DC + lg * 4;
    bf16_t* krow = a.dk + ((long long)b * S + key) * a.lddk + h * D + dc * DC + lg * 4;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      u32x2 v2 = {pack2bf(dv[n][0], dv[n][1]), pack2bf(dv[n][2], dv[n][3])};
      u32x2 k2 = {pack2bf(dk[n][0] * a.scale, dk[n][1] * a.scale), pack2bf(dk[n][2] * a.scale, dk[n][3] * a.scale)};
      *reinterpret_cast<u32x2*>(vrow + n * 16) = v2;
      *reinterpret_cast<u32x2*>(krow + n * 16) = k2;
    }
  }
}

template <typename F>
int wide_dispatch(int D, F&& f) {
  switch (D) {
    case 32: return f(std::integral_constant<int, 32>());
    case 64: return f(std::integral_constant<int, 64>());
    case 128: return f(std::integral_constant<int, 128>());
    case 256: return f(std::integral_constant<int, 256>());
    case 512: return f(std::integral_constant<int, 512>());
  }
  return OS2S_ERR_UNSUPPORTED;
}

bool wide_ld_ok(long long ld, int H, int D) { return ld % 8 == 0 && ld >= (long long)H * D && ld < (1LL << 22); }
bool wide_al_ok(const void* p) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int D, bool kBwd>
int wide_launch(hipStream_t stream, const WideArgs& a) {
  constexpr int DC = D < 128 ? D : 128;
  const size_t lds = (size_t)kWideRows * (a.Sp + 4) * 4 + 2 * (size_t)kWideKc * (DC + 4) * 2;
  OS2S_LAUNCH_LDS((attn_wide_kernel<D, kBwd>), dim3(ceil_div(a.Tq, kWideRows), a.H, a.B), dim3(256), lds, stream, a);
  return OS2S_OK;
}

int wide_shape_check(int B, int H, int D, int Tq, int S, float keep_prob) {
  OS2S_REQUIRE(B >= 1 && H >= 1 && Tq >= 1 && S >= 1 && B < 65536 && H < 65536);
  OS2S_REQUIRE(keep_prob > 0.f && keep_prob <= 1.f);
  OS2S_REQUIRE((long long)Tq * S < (1LL << 40));
  if (D != 32 && D != 64 && D != 128 && D != 256 && D != 512) return OS2S_ERR_UNSUPPORTED;
  if (S > kWideMaxS || S % 8 != 0) return OS2S_ERR_UNSUPPORTED;
  return OS2S_OK;
}

}  // namespace
}  // namespace os2s

using namespace os2s;

extern "C" int os2s_attention_wide_fwd(os2s_stream_t stream, const uint16_t* q, const uint16_t* k,
                                       const uint16_t* v, const float* key_bias, const int32_t* positions,
                                       uint16_t* o, float* p, int32_t* argmax, int B, int H, int D, int Tq,
                                       int S, long long ldq, long long ldk, long long ldv, long long ldo,
                                       int window, int back_step, float scale, float keep_prob,
                                       unsigned long long seed) {
  const int rc = wide_shape_check(B, H, D, Tq, S, keep_prob);
  if (rc != OS2S_OK) return rc;
  OS2S_REQUIRE(wide_al_ok(q) && wide_al_ok(k) && wide_al_ok(v) && wide_al_ok(o) && wide_al_ok(p) && wide_al_ok(key_bias));
  OS2S_REQUIRE(wide_ld_ok(ldq, H, D) && wide_ld_ok(ldk, H, D) && wide_ld_ok(ldv, H, D) && wide_ld_ok(ldo, H, D));
  if (positions != nullptr) OS2S_REQUIRE(window >= 1 && back_step >= 0);
  WideArgs a{};
  a.x = q; a.y = k; a.z = v; a.out = o; a.p = p; a.key_bias = key_bias;
  a.positions = positions; a.argmax = argmax; a.ds = nullptr;
  a.B = B; a.H = H; a.Tq = Tq; a.S = S; a.Sp = (S + kWideKc - 1) / kWideKc * kWideKc;
  a.ldx = ldq; a.ldy = ldk; a.ldz = ldv; a.ldo = ldo;
  a.window = window; a.back_step = back_step; a.scale = scale; a.keep_prob = keep_prob; a.seed = seed;
  return wide_dispatch(D, [&](auto d) -> int { return wide_launch<decltype(d)::value, false>((hipStream_t)stream, a); });
}

extern "C" int os2s_attention_wide_bwd(os2s_stream_t stream, const uint16_t* q, const uint16_t* k,
                                       const uint16_t* v, const uint16_t* d_o, const float* p, uint16_t* ds,
                                       uint16_t* dq, uint16_t* dk, uint16_t* dv, int B, int H, int D, int Tq,
                                       int S, long long ldq, long long ldk, long long ldv, long long lddo,
                                       long long lddq, long long lddk, long long lddv, float scale,
                                       float keep_prob, unsigned long long seed) {
  const int rc = wide_shape_check(B, H, D, Tq, S, keep_prob);
  if (rc != OS2S_OK) return rc;
  OS2S_REQUIRE(wide_al_ok(q) && wide_al_ok(k) && wide_al_ok(v) && wide_al_ok(d_o) && wide_al_ok(p) && wide_al_ok(ds));
  OS2S_REQUIRE(wide_al_ok(dq) && wide_al_ok(dk) && wide_al_ok(dv));
  OS2S_REQUIRE(wide_ld_ok(ldq, H, D) && wide_ld_ok(ldk, H, D) && wide_ld_ok(ldv, H, D) && wide_ld_ok(lddo, H, D));
  OS2S_REQUIRE(wide_ld_ok(lddq, H, D) && wide_ld_ok(lddk, H, D) && wide_ld_ok(lddv, H, D));
  WideArgs a{};
  a.x = d_o; a.y = v; a.z = k; a.out = dq; a.p = const_cast<float*>(p); a.key_bias = nullptr;
  a.positions = nullptr; a.argmax = nullptr; a.ds = ds;
  a.B = B; a.H = H; a.Tq = Tq; a.S = S; a.Sp = (S + kWideKc - 1) / kWideKc * kWideKc;
  a.ldx = lddo; a.ldy = ldv; a.ldz = ldk; a.ldo = lddq;
  a.window = 0; a.back_step = 0; a.scale = scale; a.keep_prob = keep_prob; a.seed = seed;
  int r2 = wide_dispatch(D, [&](auto d) -> int { return wide_launch<decltype(d)::value, true>((hipStream_t)stream, a); });
  if (r2 != OS2S_OK) return r2;
  WideKvArgs kv{q, d_o, ds, p, dk, dv, B, H, Tq, S, ldq, lddo, lddk, lddv, scale, keep_prob, seed};
  return wide_dispatch(D, [&](auto d) -> int {
    constexpr int DD = decltype(d)::value, NDC = DD / (DD < 128 ? DD : 128);
    OS2S_LAUNCH((attn_wide_dkv_kernel<DD>), dim3(ceil_div(S, 64) * NDC, H, B), dim3(256), 0, (hipStream_t)stream, kv);
    return OS2S_OK;
  });
}
