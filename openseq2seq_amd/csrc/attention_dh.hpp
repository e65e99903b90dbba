// The attention kernels of attention.hip for head dims 8, 16, 32 and 128 (included by attention.hip after the
// tuned dh = 64 kernels, whose LDS images, lane maps and dropout indexing these share). The multi-tile forward
// WITH dropout has no tuned twin and is this family's at dh = 64 too. Same contract: packed
// token-major q / k / v with arbitrary row strides, lse [Nq, H] fp32, fp32 accumulation and softmax, the
// dropout mask indexed ((b*H + h)*64 + q)*64 + key whatever the head dim.
//
// A head is handled as ceil(DH / 64) LDS images of 64 channels (the images of attention.hip, unchanged):
//   * DH < 64: the channels past DH belong to the NEIGHBOURING head in memory, so every load of them is
//     replaced by zeros (a 16-byte piece is wholly inside or wholly outside a head: DH % 8 == 0) and every store
//     of them is dropped; reduction steps and 32-row result blocks past DH are not computed. At DH = 8 the upper
//     half (lanes 32-63) of the one 16-deep score step is zero.
//   * DH = 128: two images per operand, eight score steps, four 32-row result blocks.
// These kernels are not tuned: the loads sit in the loops that use them and the compiler schedules them.
#pragma once

namespace os2s {

template <int DH>
struct HeadDim {
  static_assert(DH == 8 || DH == 16 || DH == 32 || DH == 64 || DH == 128,
                "head dims next to the tuned 64, and 64 itself for the kernels that have no tuned twin");
  static constexpr int kImgs = (DH + 63) / 64;      // 64-channel LDS images per [64 rows][DH] operand
  static constexpr int kSteps = (DH + 15) / 16;     // 16-deep MFMA steps of a reduction over the channels
  static constexpr int kDBlocks = (DH + 31) / 32;   // 32-row blocks of a [d][*] result
};

// head_rsrc for a head of DH channels: rows >= `rows` are out of range (zeros). Channels past DH of an earlier
// row are NOT out of range — the callers mask them.
template <int DH>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t head_rsrc_dh(const bf16_t* base, long long ld, int rows) {
  const unsigned long long a = (unsigned long long)base;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  const int bytes = __builtin_amdgcn_readfirstlane(rows > 0 ? (int)((long long)(rows - 1) * ld * 2 + DH * 2) : 0);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, bytes, 0x00020000);
}
// MFMA operand piece: channels kk*16 + lhi*8 .. +7 (voff already holds the lhi*16 bytes). Only DH = 8 has a
// piece past the head inside a live step: the upper half of step 0.
template <int DH>
__device__ __forceinline__ bf16x8 load8_dh(__amdgpu_buffer_rsrc_t rs, int voff, int soff, int lhi) {
  const bf16x8 v = load8(rs, voff, soff);
  if (DH == 8 && lhi) return zero8();
  return v;
}
template <int DH>
__device__ __forceinline__ bf16x8 frag_global_dh(const bf16_t* base, long long ld, int row, int nvalid, int kofs) {
  if (row >= nvalid || kofs >= DH) return zero8();
  return *reinterpret_cast<const bf16x8*>(base + (long long)row * ld + kofs);
}
// stage_tr for the kImgs images of one operand (8 KB apart); pieces past the head or the length are zeros
template <int DH>
__device__ __forceinline__ void stage_tr_dh(char* buf, const bf16_t* base, long long ld, int nvalid, int lane) {
#pragma unroll
  for (int hh = 0; hh < HeadDim<DH>::kImgs; ++hh)
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int piece = it * 64 + lane;
      const int row = piece >> 3, p8 = piece & 7;
      const int ch = hh * 64 + p8 * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row < nvalid && ch < DH) v = *reinterpret_cast<const u32x4*>(base + (long long)row * ld + ch);
      *reinterpret_cast<u32x4*>(buf + hh * 8192 + tr_off(row, p8 * 8)) = v;
    }
}
// store_dT_quad for result block db of kDBlocks: the 8-row pieces past DH are dropped
template <int DH>
__device__ __forceinline__ void store_dT_quad_dh(const f32x16& d, int db, int j, bf16_t* out, long long ld,
                                                 int nvalid, float mul, int lane) {
  const int n = j * 32 + (lane & 31);
#pragma unroll
  for (int gp = 0; gp < 2; ++gp) {
    const u32x4 v = rows8(d, 2 * gp, mul);
    const int d0 = db * 32 + 8 * (2 * gp + (lane >> 5));
    if (n < nvalid && d0 < DH) *reinterpret_cast<u32x4*>(out + (long long)n * ld + d0) = v;
  }
}

// ---------------------------------------------------------------------------
// forward, Lq, Lk <= 64: attn_fwd_kernel's structure (one wave per (batch, head), P in registers, V^T in LDS)
// ---------------------------------------------------------------------------
template <int DH, bool kDrop>
__global__ __launch_bounds__(kFwdWaves * 64) void attn_fwd_dh_kernel(AttnArgs p) {
  using HD = HeadDim<DH>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  const int bh = blockIdx.x * kFwdWaves + wid;      // B * H < 2^30 (checked by the host side)
  if (bh >= p.B * p.H) return;
  const int b = bh / p.H, h = bh - b * p.H;
  const int q0 = p.cu_q[b], k0 = p.cu_k[b];
  const int Lq = min(p.cu_q[b + 1] - q0, kL), Lk = min(p.cu_k[b + 1] - k0, kL);
  if (Lq <= 0) return;
  char* const vt = smem + wid * (HD::kImgs * 8192);   // V[key][d]   (tr images)
  const int nj = Lq > 32 ? 2 : 1, ni = Lk > 32 ? 2 : 1;
  const bool causal = p.causal != 0;
  const __amdgpu_buffer_rsrc_t qrs = head_rsrc_dh<DH>(p.q + (long long)q0 * p.ldq + h * DH, p.ldq, Lq);
  const __amdgpu_buffer_rsrc_t krs = head_rsrc_dh<DH>(p.k + (long long)k0 * p.ldk + h * DH, p.ldk, Lk);
  const __amdgpu_buffer_rsrc_t vrs = head_rsrc_dh<DH>(p.v + (long long)k0 * p.ldv + h * DH, p.ldv, Lk);
  // ---- V image(s): the rows the P.V reduction touches (zeros past Lk and past the head) ------------
  const int Lk16 = (Lk + 15) & ~15;
#pragma unroll
  for (int hh = 0; hh < HD::kImgs; ++hh)
#pragma unroll
    for (int it = 0; it < 8; ++it)
      if (it * 8 < Lk16) {
        const int ch = hh * 64 + (lane & 7) * 8;
        u32x4 t = {0u, 0u, 0u, 0u};
        if (ch < DH)
          t = __builtin_amdgcn_raw_buffer_load_b128(vrs, (lane >> 3) * (int)p.ldv * 2 + ch * 2,
                                                    it * 8 * (int)p.ldv * 2, 0);
        *reinterpret_cast<u32x4*>(vt + hh * 8192 + tr_off(it * 8 + (lane >> 3), (lane & 7) * 8)) = t;
      }
  // ---- S^T[key][q] per live 32 x 32 block -----------------------------------------------------
  f32x16 s[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) s[i][j][e] = 0.f;
  {
    const int kv = l31 * (int)p.ldk * 2 + lhi * 16, qv = l31 * (int)p.ldq * 2 + lhi * 16;
    const int ks = 32 * (int)p.ldk * 2, qs = 32 * (int)p.ldq * 2;
#pragma unroll
    for (int kk = 0; kk < HD::kSteps; ++kk) {
      bf16x8 ka[2], qb[2];
      ka[0] = load8_dh<DH>(krs, kv + kk * 32, 0, lhi);
      qb[0] = load8_dh<DH>(qrs, qv + kk * 32, 0, lhi);
      ka[1] = load8_dh<DH>(krs, kv + kk * 32, ks, lhi);      // past the length: zeros, no memory access
      qb[1] = load8_dh<DH>(qrs, qv + kk * 32, qs, lhi);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (i < ni && j < nj && !(causal && i > j))
            s[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[i], qb[j], s[i][j], 0, 0, 0);
    }
  }
  // ---- softmax over keys (rows) for each query column; P stays in registers as the B operand ------
  const float sc2 = p.scale * 1.4426950408889634f;
  const uint32_t thr = (uint32_t)(p.keep_prob * 65536.0f);
  const unsigned long long zlane =
      (unsigned long long)((long long)bh * (kL * kL / 4) + l31 * (kL / 4) + lhi) * kDropGolden + p.seed;
  bf16x8 pmb[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) pmb[j][kk] = zero8();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j >= nj) continue;
    const int q = j * 32 + l31;
    const int lim = min(Lk, causal ? q + 1 : kL) - 4 * lhi;
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i >= ni || (causal && i > j)) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = (i * 32 + (r & 3) + 8 * (r >> 2)) < lim ? s[i][j][r] * sc2 : -INFINITY;
        s[i][j][r] = v;
        m = fmaxf(m, v);
      }
    }
    m = half_max(m);
    const float msafe = m == -INFINITY ? 0.f : m;
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i >= ni || (causal && i > j)) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(s[i][j][r] - msafe);
        s[i][j][r] = e;
        l += e;
      }
    }
    l = half_sum(l);
    if (lhi == 0 && q < Lq && p.lse)
      p.lse[(long long)(q0 + q) * p.H + h] = (msafe + __log2f(l)) * 0.6931471805599453f;
    float mul = l > 0.f ? 1.f / l : 0.f;
    if (kDrop) mul *= 1.f / p.keep_prob;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i >= ni || (causal && i > j)) continue;
      uint32_t pk[4][2];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint32_t keep = 0xfu;
        if (kDrop) keep = dropout_bits4_z(zlane + attn_drop_step(j * (32 * kL / 4) + i * 8 + 2 * g), thr);
        float w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = ((keep >> e) & 1u) ? s[i][j][4 * g + e] * mul : 0.f;
        pk[g][0] = pack2bf(w[0], w[1]);
        pk[g][1] = pack2bf(w[2], w[3]);
      }
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        u32x4 t;
        t[0] = pk[2 * k2][0]; t[1] = pk[2 * k2][1]; t[2] = pk[2 * k2 + 1][0]; t[3] = pk[2 * k2 + 1][1];
        pmb[j][2 * i + k2] = __builtin_bit_cast(bf16x8, t);
      }
    }
  }
  __builtin_amdgcn_wave_barrier();        // the V^T images are this wave's own: LDS ops of a wave are in order
  // ---- O^T[d][q] = sum_key V^T[d][key] * PM^T[key][q], one 32-row d block at a time ---------------
  bf16_t* ob = p.o + (long long)q0 * p.ldo + h * DH;
#pragma unroll
  for (int db = 0; db < HD::kDBlocks; ++db) {
    f32x16 o[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[j][e] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (kk * 16 >= Lk) continue;
      const bf16x8 a = frag_tr_acc(vt + (db >> 1) * 8192, db & 1, kk, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j >= nj || (causal && (kk >> 1) > j)) continue;
        o[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pmb[j][kk], o[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (j < nj) store_dT_quad_dh<DH>(o[j], db, j, ob, p.ldo, Lq, 1.f, lane);
  }
}

// ---------------------------------------------------------------------------
// forward for sequences longer than one tile: attn_fwd_long_kernel's structure (online softmax over the
// key tiles, P through an LDS image). kDrop (training; at every head dim, 64 included): the running sum is of the
// UNDROPPED probabilities, so lse is what the forward without dropout stores; the mask, element
// ((b*H + h)*Lp + q)*Lp + key (long_drop_z), zeroes P on its way into the image and 1 / keep goes into the final
// normalisation.
// ---------------------------------------------------------------------------
// z of dropout_bits4_z for the four keys key4 * 4 .. + 3 of query q, both counted from the start of the sequence;
// Lp = max_len rounded up to 64 (at Lp = 64: the index of the one-tile kernels)
__device__ __forceinline__ unsigned long long long_drop_z(long long bh, int Lp, int q, int key4,
                                                          unsigned long long seed) {
  return (unsigned long long)((bh * Lp + q) * (long long)(Lp >> 2) + key4) * kDropGolden + seed;
}

template <int DH, bool kDrop>
__global__ __launch_bounds__(kFwdWaves * 64) void attn_fwd_long_dh_kernel(AttnArgs p, int q_tiles, int Lp) {
  using HD = HeadDim<DH>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const long long work = (long long)blockIdx.x * kFwdWaves + wid;
  if (work >= (long long)p.B * p.H * q_tiles) return;       // waves are independent (own LDS slice)
  const long long bh = work / q_tiles;
  const int qt = (int)(work - bh * q_tiles);
  const int b = (int)(bh / p.H), h = (int)(bh - (long long)b * p.H);
  const int q0 = p.cu_q[b], k0 = p.cu_k[b];
  const int Lq_tot = p.cu_q[b + 1] - q0, Lk_tot = p.cu_k[b + 1] - k0;
  const int qs = qt * kL;
  if (qs >= Lq_tot) return;
  const int Lq = min(Lq_tot - qs, kL);
  char* pm = smem + wid * ((1 + HD::kImgs) * 8192);   // P[q][key]  (kc image)
  char* vt = pm + 8192;                               // V[key][d]  (tr images)
  const bf16_t* qb = p.q + (long long)(q0 + qs) * p.ldq + h * DH;
  const uint32_t thr = (uint32_t)(p.keep_prob * 65536.0f);
  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
  f32x16 o[HD::kDBlocks][2];
#pragma unroll
  for (int i = 0; i < HD::kDBlocks; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[i][j][e] = 0.f;
  const int nkt = p.causal ? min(qt + 1, (Lk_tot + kL - 1) / kL) : (Lk_tot + kL - 1) / kL;
  for (int kt = 0; kt < nkt; ++kt) {
    const int ks = kt * kL;
    const int Lk = min(Lk_tot - ks, kL);
    const bf16_t* kb = p.k + (long long)(k0 + ks) * p.ldk + h * DH;
    const bf16_t* vb = p.v + (long long)(k0 + ks) * p.ldv + h * DH;
    f32x16 s[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) s[i][j][e] = 0.f;
#pragma unroll
    for (int kk = 0; kk < HD::kSteps; ++kk) {
      bf16x8 a[2], bq[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = frag_global_dh<DH>(kb, p.ldk, i * 32 + l31, Lk, kk * 16 + lhi * 8);
#pragma unroll
      for (int j = 0; j < 2; ++j) bq[j] = frag_global_dh<DH>(qb, p.ldq, j * 32 + l31, Lq, kk * 16 + lhi * 8);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          s[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], bq[j], s[i][j], 0, 0, 0);
    }
    stage_tr_dh<DH>(vt, vb, p.ldv, Lk, lane);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = j * 32 + l31;
      float mt = -INFINITY;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = key_of(i, r, lhi);
          const bool ok = key < Lk && !(p.causal && ks + key > qs + q);
          const float v = ok ? s[i][j][r] * p.scale : -INFINITY;
          s[i][j][r] = v;
          mt = fmaxf(mt, v);
        }
      mt = fmaxf(mt, xhalf(mt));
      const float mn = fmaxf(m_run[j], mt);
      const float msafe = mn == -INFINITY ? 0.f : mn;
      const float corr = m_run[j] == -INFINITY ? 0.f : __expf(m_run[j] - msafe);
      float lsum = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = __expf(s[i][j][r] - msafe);      // exp(-inf) = 0 for masked keys
          s[i][j][r] = e;
          lsum += e;
        }
      lsum += xhalf(lsum);
      l_run[j] = l_run[j] * corr + lsum;
      m_run[j] = mn;
#pragma unroll
      for (int i = 0; i < HD::kDBlocks; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[i][j][e] *= corr;
      // keys ks + 4*lhi + (i*32 + 8g) .. + 3 of query qs + q: draw (ks >> 2) + lhi + i*8 + 2g
      const unsigned long long zq = kDrop ? long_drop_z(bh, Lp, qs + q, (ks >> 2) + lhi, p.seed) : 0ull;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int key0 = i * 32 + 8 * g + 4 * lhi;
          uint32_t keep = 0xfu;
          if (kDrop) keep = dropout_bits4_z(zq + attn_drop_step(i * 8 + 2 * g), thr);
          float w[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) w[e] = ((keep >> e) & 1u) ? s[i][j][4 * g + e] : 0.f;
          u32x2 pk;
          pk[0] = pack2bf(w[0], w[1]);
          pk[1] = pack2bf(w[2], w[3]);
          *reinterpret_cast<u32x2*>(pm + kc_off(q, key0)) = pk;
        }
    }
    __builtin_amdgcn_wave_barrier();      // LDS ops of one wave complete in order
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      bf16x8 bq[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bq[j] = frag_kc(pm, j * 32 + l31, kk * 2 + lhi);
#pragma unroll
      for (int i = 0; i < HD::kDBlocks; ++i) {
        const bf16x8 a = frag_tr(vt + (i >> 1) * 8192, i & 1, kk, lane);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          o[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bq[j], o[i][j], 0, 0, 0);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  bf16_t* ob = p.o + (long long)(q0 + qs) * p.ldo + h * DH;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int q = j * 32 + l31;
    if (q < Lq) {
      const float inv = l_run[j] > 0.f ? (kDrop ? 1.f / p.keep_prob : 1.f) / l_run[j] : 0.f;
      if (lhi == 0 && p.lse)
        p.lse[(long long)(q0 + qs + q) * p.H + h] = (m_run[j] == -INFINITY ? 0.f : m_run[j]) + __logf(l_run[j]);
#pragma unroll
      for (int i = 0; i < HD::kDBlocks; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d0 = i * 32 + 8 * g + 4 * lhi;
          if (d0 >= DH) continue;           // a 4-channel piece is inside or outside the head: DH % 8 == 0
          u32x2 pk;
          pk[0] = pack2bf(o[i][j][4 * g] * inv, o[i][j][4 * g + 1] * inv);
          pk[1] = pack2bf(o[i][j][4 * g + 2] * inv, o[i][j][4 * g + 3] * inv);
          *reinterpret_cast<u32x2*>(ob + (long long)q * p.ldo + d0) = pk;
        }
    }
  }
}

// ---------------------------------------------------------------------------
// backward: attn_bwd_kernel's structure (four waves per (batch, head); wave (wi, wj) owns block (key wi,
// query wj) of S / P / dS). In the gradient products wave (wi, wj) takes the d blocks wi, wi + 2, ...: with
// DH <= 32 there is one d block and the waves wi = 1 only help with S, at DH = 128 every wave takes two.
// LDS: dO, K, Q as kImgs images each, then PM and dS, each as TWO bf16 images hi + lo (hi = bf16(x), lo =
// bf16(x - hi)) that the gradient products multiply one after the other. With a single bf16 image the rounding
// of P (2^-9 relative) is summed over the queries of a key: for a sentence of 2 keys and 33 queries that is 2.3e-3
// * |dO| * sqrt(33) per element of dV, half of the 3e-2-of-the-tensor-rms bound the gradients are held to, and an
// element in the tail of that error misses it; dS into dK likewise. The split leaves the output rounding only.
// ---------------------------------------------------------------------------
template <int DH>
constexpr int attn_bwd_dh_lds() { return (3 * HeadDim<DH>::kImgs + 4) * 8192; }

// four consecutive values of row `off` as hi + lo bf16 pieces into the two images
__device__ __forceinline__ void store4_split(char* hi_img, char* lo_img, int off, const float (&w)[4]) {
  u32x2 hi, lo;
  hi[0] = pack2bf(w[0], w[1]);
  hi[1] = pack2bf(w[2], w[3]);
  lo[0] = pack2bf(w[0] - bflo(hi[0]), w[1] - bfhi(hi[0]));
  lo[1] = pack2bf(w[2] - bflo(hi[1]), w[3] - bfhi(hi[1]));
  *reinterpret_cast<u32x2*>(hi_img + off) = hi;
  *reinterpret_cast<u32x2*>(lo_img + off) = lo;
}

template <int DH, bool kDrop>
__global__ __launch_bounds__(kBwdThreads) void attn_bwd_dh_kernel(AttnArgs p) {
  using HD = HeadDim<DH>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wid >> 1, wj = wid & 1;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int bh = blockIdx.x;             // B * H < 2^31 (checked by the host side)
  const int b = bh / p.H, h = bh - b * p.H;
  const int q0 = p.cu_q[b], k0 = p.cu_k[b];
  const int Lq = min(p.cu_q[b + 1] - q0, kL), Lk = min(p.cu_k[b + 1] - k0, kL);
  const bool causal = p.causal != 0;
  char* const do_img = smem;                              // dO[q][d]   tr images (rows = q)
  char* const k_img = smem + HD::kImgs * 8192;            // K[key][d]  tr images (rows = key)
  char* const q_img = smem + 2 * HD::kImgs * 8192;        // Q[q][d]    tr images (rows = q)
  char* const pm = smem + 3 * HD::kImgs * 8192;           // PM[q][key] tr images hi, lo (rows = q)
  char* const pm_lo = pm + 8192;
  char* const ds = pm + 16384;                            // dS[q][key] tr images hi, lo (rows = q); also read row-wise
  char* const ds_lo = ds + 8192;
  float* const dbuf = reinterpret_cast<float*>(ds);       // [2][64] partial deltas, before dS is written
  const int ldq = (int)p.ldq, ldk = (int)p.ldk, ldv = (int)p.ldv, lddo = (int)p.lddo;
  const __amdgpu_buffer_rsrc_t qrs = head_rsrc_dh<DH>(p.q + (long long)q0 * p.ldq + h * DH, p.ldq, Lq);
  const __amdgpu_buffer_rsrc_t krs = head_rsrc_dh<DH>(p.k + (long long)k0 * p.ldk + h * DH, p.ldk, Lk);
  const __amdgpu_buffer_rsrc_t vrs = head_rsrc_dh<DH>(p.v + (long long)k0 * p.ldv + h * DH, p.ldv, Lk);
  const __amdgpu_buffer_rsrc_t dors = head_rsrc_dh<DH>(p.d_o + (long long)q0 * p.lddo + h * DH, p.lddo, Lq);
  const int nbq = Lq > 32 ? 2 : 1, nbk = Lk > 32 ? 2 : 1;
  const bool live1 = wi * 32 < Lk && wj * 32 < Lq && !(causal && wi > wj);
  const int q = wj * 32 + l31;

  // ---- the transpose-read images: 32-row blocks that hold a live row (zeros past the length / the head) ----
  {
    const int srow = tid >> 3;
#pragma unroll
    for (int hh = 0; hh < HD::kImgs; ++hh) {
      const int ch = hh * 64 + (tid & 7) * 8;
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int o = hh * 8192 + tr_off(it * 32 + srow, (tid & 7) * 8);
        u32x4 tdo = {0u, 0u, 0u, 0u}, tq = tdo, tk = tdo;
        if (ch < DH) {
          if (it < nbq) {
            tdo = __builtin_amdgcn_raw_buffer_load_b128(dors, srow * lddo * 2 + ch * 2, it * 32 * lddo * 2, 0);
            tq = __builtin_amdgcn_raw_buffer_load_b128(qrs, srow * ldq * 2 + ch * 2, it * 32 * ldq * 2, 0);
          }
          if (it < nbk) tk = __builtin_amdgcn_raw_buffer_load_b128(krs, srow * ldk * 2 + ch * 2, it * 32 * ldk * 2, 0);
        }
        if (it < nbq) {
          *reinterpret_cast<u32x4*>(do_img + o) = tdo;
          *reinterpret_cast<u32x4*>(q_img + o) = tq;
        }
        if (it < nbk) *reinterpret_cast<u32x4*>(k_img + o) = tk;
      }
    }
  }
  // ---- S^T[key][q] = K Q^T and dPM^T[key][q] = V dO^T, this wave's block; P, M, the partial
  //      delta = sum over this wave's 32 keys of P * M * dPM; PM[q][key] to LDS -----------------------
  f32x16 s, dp;
  float delta = 0.f;
  if (live1) {
    const float lse2 = q < Lq ? p.lse[(long long)(q0 + q) * p.H + h] * 1.4426950408889634f : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
    const int kv = l31 * ldk * 2 + lhi * 16, qv = l31 * ldq * 2 + lhi * 16;
    const int vv = l31 * ldv * 2 + lhi * 16, dv_ = l31 * lddo * 2 + lhi * 16;
#pragma unroll
    for (int kk = 0; kk < HD::kSteps; ++kk) {
      const bf16x8 fk = load8_dh<DH>(krs, kv + kk * 32, wi * 32 * ldk * 2, lhi);
      const bf16x8 fq = load8_dh<DH>(qrs, qv + kk * 32, wj * 32 * ldq * 2, lhi);
      const bf16x8 fv = load8_dh<DH>(vrs, vv + kk * 32, wi * 32 * ldv * 2, lhi);
      const bf16x8 fdo = load8_dh<DH>(dors, dv_ + kk * 32, wj * 32 * lddo * 2, lhi);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fk, fq, s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fv, fdo, dp, 0, 0, 0);
    }
    const float ik = 1.f / p.keep_prob, sc2 = p.scale * 1.4426950408889634f;
    const uint32_t thr = (uint32_t)(p.keep_prob * 65536.0f);
    const unsigned long long zlane =
        (unsigned long long)((long long)bh * (kL * kL / 4) + q * (kL / 4) + wi * 8 + lhi) * kDropGolden + p.seed;
    // register 4g + e is key wi*32 + 8g + e + 4*lhi: live <=> 8g + e < lim
    const int lim = q < Lq ? min(Lk, causal ? q + 1 : kL) - 4 * lhi - wi * 32 : 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint32_t keep = 0xfu;
      if (kDrop) keep = dropout_bits4_z(zlane + attn_drop_step(2 * g), thr);
      float pmv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        const float pv = (8 * g + e) < lim ? __builtin_amdgcn_exp2f(s[r] * sc2 - lse2) : 0.f;
        const float mk = kDrop ? (((keep >> e) & 1u) ? ik : 0.f) : 1.f;
        s[r] = pv;                  // P
        dp[r] *= mk;                // dP = dPM * M
        delta += pv * dp[r];
        pmv[e] = pv * mk;
      }
      store4_split(pm, pm_lo, tr_off(q, wi * 32 + 8 * g + 4 * lhi), pmv);
    }
    delta = half_sum(delta);
  }
  if (lhi == 0) dbuf[wi * 64 + q] = delta;       // 0 from a dead block
  __syncthreads();
  delta += dbuf[(wi ^ 1) * 64 + q];      // the other 32 keys of this query (wave (1 - wi, wj))
  __syncthreads();                        // dbuf is overwritten by the dS image next
  if (live1) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = s[4 * g + e] * (dp[4 * g + e] - delta);   // dS (w.r.t. the scaled logits)
      store4_split(ds, ds_lo, tr_off(q, wi * 32 + 8 * g + 4 * lhi), w);
    }
  }
  __syncthreads();
  // ---- the three gradient products, d block db of this wave, key / query block wj ---------------------
  const bool krows = wj * 32 < Lk, qrows = wj * 32 < Lq;
#pragma unroll
  for (int db = wi; db < HD::kDBlocks; db += 2) {
    const int io = (db >> 1) * 8192, mt = db & 1;
    f32x16 dv, dq, dk;
#pragma unroll
    for (int e = 0; e < 16; ++e) { dv[e] = 0.f; dq[e] = 0.f; dk[e] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (krows && kk * 16 < Lq && !(causal && wj > (kk >> 1))) {       // block (key wj, query kk/2)
        // dV^T[d][key] = sum_q dO[q][d] PM[q][key], dK^T[d][key] = scale * sum_q Q[q][d] dS[q][key]
        const bf16x8 fdo = frag_tr(do_img + io, mt, kk, lane), fq = frag_tr(q_img + io, mt, kk, lane);
        dv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fdo, frag_tr(pm, wj, kk, lane), dv, 0, 0, 0);
        dv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fdo, frag_tr(pm_lo, wj, kk, lane), dv, 0, 0, 0);
        dk = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fq, frag_tr(ds, wj, kk, lane), dk, 0, 0, 0);
        dk = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fq, frag_tr(ds_lo, wj, kk, lane), dk, 0, 0, 0);
      }
      if (qrows && kk * 16 < Lk && !(causal && (kk >> 1) > wj)) {       // block (key kk/2, query wj)
        // dQ^T[d][q] = scale * sum_key K[key][d] dS[q][key]: B operand = 8 consecutive keys of row q
        const int ro = tr_off(wj * 32 + l31, kk * 16 + lhi * 8);
        const bf16x8 fk = frag_tr(k_img + io, mt, kk, lane);
        dq = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fk, *reinterpret_cast<const bf16x8*>(ds + ro), dq, 0, 0, 0);
        dq = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fk, *reinterpret_cast<const bf16x8*>(ds_lo + ro), dq, 0, 0, 0);
      }
    }
    if (krows) {
      store_dT_quad_dh<DH>(dv, db, wj, p.dv + (long long)k0 * p.lddv + h * DH, p.lddv, Lk, 1.f, lane);
      store_dT_quad_dh<DH>(dk, db, wj, p.dk + (long long)k0 * p.lddk + h * DH, p.lddk, Lk, p.scale, lane);
    }
    if (qrows) store_dT_quad_dh<DH>(dq, db, wj, p.dq + (long long)q0 * p.lddq + h * DH, p.lddq, Lq, p.scale, lane);
  }
}

}  // namespace os2s

// ---- host side -------------------------------------------------------------------------------------
namespace os2s {

template <int DH>
static int attn_fwd_dh_launch(hipStream_t st, const AttnArgs& a, int max_len) {
  using HD = HeadDim<DH>;
  const int B = a.B, H = a.H;
  if (max_len > kL) {      // multi-tile forward; DH = 64 comes here with dropout only
    const size_t smem = (size_t)kFwdWaves * (1 + HD::kImgs) * 8192;       // 64 KB, 96 KB at DH = 128
    const int q_tiles = (max_len + kL - 1) / kL;
    const dim3 grid(ceil_div((long long)B * H * q_tiles, kFwdWaves)), block(kFwdWaves * 64);
    if (a.keep_prob < 1.f) {
      OS2S_LAUNCH_LDS((attn_fwd_long_dh_kernel<DH, true>), grid, block, smem, st, a, q_tiles, q_tiles * kL);
    } else {
      OS2S_LAUNCH_LDS((attn_fwd_long_dh_kernel<DH, false>), grid, block, smem, st, a, q_tiles, q_tiles * kL);
    }
    return OS2S_OK;
  }
  const size_t smem = (size_t)kFwdWaves * HD::kImgs * 8192;               // 32 KB, 64 KB at DH = 128
  const dim3 grid(ceil_div((long long)B * H, kFwdWaves)), block(kFwdWaves * 64);
  if (a.keep_prob < 1.f) {
    OS2S_LAUNCH_LDS((attn_fwd_dh_kernel<DH, true>), grid, block, smem, st, a);
  } else {
    OS2S_LAUNCH_LDS((attn_fwd_dh_kernel<DH, false>), grid, block, smem, st, a);
  }
  return OS2S_OK;
}

template <int DH>
static int attn_bwd_dh_launch(hipStream_t st, const AttnArgs& a) {
  const size_t smem = (size_t)attn_bwd_dh_lds<DH>();                      // 56 KB, 80 KB at DH = 128
  const dim3 grid((unsigned)((long long)a.B * a.H)), block(kBwdThreads);
  if (a.keep_prob < 1.f) {
    OS2S_LAUNCH_LDS((attn_bwd_dh_kernel<DH, true>), grid, block, smem, st, a);
  } else {
    OS2S_LAUNCH_LDS((attn_bwd_dh_kernel<DH, false>), grid, block, smem, st, a);
  }
  return OS2S_OK;
}

// the head dims next to 64; the caller has checked dh with attn_dh_ok
static int attn_fwd_dh(hipStream_t st, const AttnArgs& a, int dh, int max_len) {
  switch (dh) {
    case 8: return attn_fwd_dh_launch<8>(st, a, max_len);
    case 16: return attn_fwd_dh_launch<16>(st, a, max_len);
    case 32: return attn_fwd_dh_launch<32>(st, a, max_len);
    case 64: return attn_fwd_dh_launch<64>(st, a, max_len);      // max_len > 64 with dropout only (attention.hip)
    case 128: return attn_fwd_dh_launch<128>(st, a, max_len);
  }
  return OS2S_ERR_UNSUPPORTED;
}
static int attn_bwd_dh(hipStream_t st, const AttnArgs& a, int dh) {
  switch (dh) {
    case 8: return attn_bwd_dh_launch<8>(st, a);
    case 16: return attn_bwd_dh_launch<16>(st, a);
    case 32: return attn_bwd_dh_launch<32>(st, a);
    case 128: return attn_bwd_dh_launch<128>(st, a);
  }
  return OS2S_ERR_UNSUPPORTED;
}

}  // namespace os2s
