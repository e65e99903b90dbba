// The attention BACKWARD for sequences longer than one 64-token tile (included by attention.hip after its kernels,
// on top of its helpers: HeadDim, head_rsrc, load8, load_piece, frag_tr, long_drop_z, store_dT_quad; launched by
// os2s_attention_bwd_long there), templated on the head dim like them. Same contract as the rest of attention.hip:
// packed token-major q / k / v with arbitrary row strides, lse [Nq, H] fp32 of the undropped scaled logits, fp32
// softmax, bf16 I/O. Calls with max_len <= 64 never come here. The forward it belongs to is
// attn_fwd_long_kernel<DH, kDrop>.
//
// Dropout mask (long_drop_z, shared with that forward): element ((b*H + h)*Lp + q)*Lp + key of the generator behind
// os2s_dropout_mask, q and key counted from the start of the sequence, Lp = max_len rounded up to 64, 64-bit
// arithmetic. At Lp = 64 that is the index of the one-tile kernels. Four consecutive keys share one draw
// (dropout_bits4_z), as there.
//
// Backward: P is recomputed per 64 x 64 tile from (q, k, lse); with Pd = P o m / keep
//   dV = Pd^T dO, dPd = dO V^T, delta_q = sum_d dO[q,d] O[q,d] = sum_key P (dPd o m / keep),
//   dS = P o (dPd o m / keep - delta),
//   dQ = scale dS K, dK = scale dS^T Q.
// Two launches, no float atomics, no workgroup waits for another: every output element has ONE owner that sums
// its tiles in a fixed order, so the result is bitwise the same from run to run.
//   1. attn_bwd_long_dq_kernel: one workgroup per (batch, head, 64-query tile) sweeps the key tiles TWICE and owns
//      dQ. The first sweep obtains delta_q = sum_key P (dPd o m / keep) in fp32 (the same number as rowsum(dO o O)
//      with an unrounded O) and writes it to the [Nq, H] fp32 workspace; the second forms dS and dQ.
//   2. attn_bwd_long_dkv_kernel: one workgroup per (batch, head, 64-key tile) sweeps the query tiles, reads delta
//      from the workspace, and owns dK and dV.
// Why delta is not rowsum(dO o O) from the forward's bf16 O, which would save the first sweep: where a query
// attends to few keys (a source of 1 or 2 tokens, the first rows under the causal mask) dPd o m / keep and delta
// nearly cancel, and the 2^-9 rounding of O does not. The gradients are held to 3e-2 of their rms, like those of
// the one-tile kernels (which sum P dPd in fp32 too); a float64 model of the variant with a rounded O put elements
// of dQ and dK off by 0.13 of the rms (causal, dropout) and 0.7 (a one-token source), and the variant itself, on
// the device, missed that bound against the oracle and against the one-tile kernels on the same sentences.
// All three sweeps recompute S and dPd, the price of not summing across workgroups. Under the causal mask the
// tiles wholly above the diagonal are not visited (wave-uniform loop bounds); the diagonal tile and the key / query
// tails of the last tiles are masked per element. A workgroup is four waves; wave (wi, wj) owns the 32 x 32 block
// (key block wi, query block wj) of S / P / dS, as in attn_bwd_kernel, and in the gradient products the d blocks
// wi, wi + 2 of key / query block wj. P o m and dS are rounded to bf16 ONCE, into LDS images the gradient products
// read.
// LDS per workgroup: dQ kernel (kImgs + 1) * 8 KB + 512 B (K image(s), dS, delta halves) = 16.5 / 24.5 KB; dK/dV
// kernel (2 * kImgs + 2) * 8 KB (dO, Q images, Pd, dS) = 32 / 48 KB, kImgs = 2 at dh = 128 and 1 otherwise.
// Tile base addresses are 64-bit; offsets inside a tile are 32-bit (row strides < 2^22 elements).
#pragma once

namespace os2s {

constexpr int kAttnLongMaxLen = 65536;      // B * H * Lp * Lp stays below 2^62 with B * H < 2^30

// d blocks one wave of the backward owns (wi, wi + 2, ...)
template <int DH>
constexpr int long_own() { return (HeadDim<DH>::kDBlocks + 1) / 2; }

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// What the two backward kernels know about their (batch, head)
struct LongSeq {
  int b, h, q0, k0, Lq_tot, Lk_tot;
  long long bh;
};
__device__ __forceinline__ LongSeq long_seq(const AttnArgs& p, long long bh) {
  LongSeq s;
  s.bh = bh;
  s.b = (int)(bh / p.H);
  s.h = (int)(bh - (long long)s.b * p.H);
  s.q0 = p.cu_q[s.b];
  s.k0 = p.cu_k[s.b];
  s.Lq_tot = p.cu_q[s.b + 1] - s.q0;
  s.Lk_tot = p.cu_k[s.b + 1] - s.k0;
  return s;
}

// the MFMA operand pieces of one 32-row block of a [rows][DH] tile: row l31 of the block at byte offset `soff`
template <int DH>
__device__ __forceinline__ void long_frags(__amdgpu_buffer_rsrc_t rs, int ld, int soff, int lane,
                                           bf16x8 (&f)[HeadDim<DH>::kSteps]) {
  const int voff = (lane & 31) * ld * 2 + (lane >> 5) * 16;
#pragma unroll
  for (int kk = 0; kk < HeadDim<DH>::kSteps; ++kk) f[kk] = load8<DH>(rs, voff + kk * 32, soff, lane >> 5);
}

// a [64 rows][DH] tile into kImgs transpose-read images, by the whole workgroup (zeros past `rs`'s rows / the head)
template <int DH>
__device__ __forceinline__ void long_stage(char* img, __amdgpu_buffer_rsrc_t rs, int ld, int tid) {
  const int srow = tid >> 3;
#pragma unroll
  for (int hh = 0; hh < HeadDim<DH>::kImgs; ++hh) {
    const int ch = hh * 64 + (tid & 7) * 8;
#pragma unroll
    for (int it = 0; it < 2; ++it)
      *reinterpret_cast<u32x4*>(img + hh * 8192 + tr_off(it * 32 + srow, (tid & 7) * 8)) =
          load_piece<DH>(rs, srow * ld * 2 + ch * 2, it * 32 * ld * 2, ch);
  }
}

// Block (key block wi, query block wj) of the tile (keys ks .., queries qs ..): S^T = K Q^T and dPd^T = V dO^T on
// the MFMA, then per element P (pv), Pd = P o m / keep (pd) and dPd o m / keep (dpm); the callers form delta =
// sum_key pv * dpm and dS = pv * (dpm - delta). Register 4g + e of a lane is key wi*32 + 8g + e + 4*lhi of query
// wj*32 + l31. lse2 = lse * log2(e) of the lane's query. Lq, Lk: live rows of the tile. (attn_bwd_kernel spells
// this block out for one tile, writing PM as it goes: called with qs = ks = 0, Lp = 64 this function cost its
// dropout instance at head dim 64 32 more registers and a wave per SIMD, and its delta sum lost its FMAs, which
// is another rounding: profiles/attention_unified.md.)
template <int DH, bool kDrop>
__device__ __forceinline__ void long_bwd_block(const AttnArgs& p, const LongSeq& sq, int Lp,
                                               const bf16x8 (&fk)[HeadDim<DH>::kSteps],
                                               const bf16x8 (&fq)[HeadDim<DH>::kSteps],
                                               const bf16x8 (&fv)[HeadDim<DH>::kSteps],
                                               const bf16x8 (&fdo)[HeadDim<DH>::kSteps], int wi, int wj, int lane,
                                               int qs, int ks, int Lq, int Lk, float lse2, float (&pv)[16],
                                               float (&pd)[16], float (&dpm)[16]) {
  const int l31 = lane & 31, lhi = lane >> 5;
  f32x16 s, dp;
#pragma unroll
  for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
  for (int kk = 0; kk < HeadDim<DH>::kSteps; ++kk) {
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fk[kk], fq[kk], s, 0, 0, 0);
    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fv[kk], fdo[kk], dp, 0, 0, 0);
  }
  const int q = wj * 32 + l31;
  const float ik = 1.f / p.keep_prob, sc2 = p.scale * 1.4426950408889634f;
  const uint32_t thr = (uint32_t)(p.keep_prob * 65536.0f);
  const unsigned long long zlane = long_drop_z(sq.bh, Lp, qs + q, ((ks + wi * 32) >> 2) + lhi, p.seed);
  // live <=> 8g + e < lim: inside the tile's keys and, with the causal band, key <= query
  const int lim = q < Lq ? min(Lk, p.causal ? qs + q - ks + 1 : kL) - 4 * lhi - wi * 32 : 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    uint32_t keep = 0xfu;
    if (kDrop) keep = dropout_bits4_z(zlane + attn_drop_step(2 * g), thr);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 4 * g + e;
      const float mk = kDrop ? (((keep >> e) & 1u) ? ik : 0.f) : 1.f;
      pv[r] = (8 * g + e) < lim ? __builtin_amdgcn_exp2f(s[r] * sc2 - lse2) : 0.f;
      pd[r] = pv[r] * mk;
      dpm[r] = dp[r] * mk;
    }
  }
}

// 16 values of a lane (accumulator order) as bf16 into a transpose-read image with rows = query
__device__ __forceinline__ void long_store_img(char* img, int q, int key0, const float (&w)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    u32x2 pk;
    pk[0] = pack2bf(w[4 * g], w[4 * g + 1]);
    pk[1] = pack2bf(w[4 * g + 2], w[4 * g + 3]);
    *reinterpret_cast<u32x2*>(img + tr_off(q, key0 + 8 * g)) = pk;
  }
}

template <int DH>
constexpr int attn_bwd_long_dq_lds() { return (HeadDim<DH>::kImgs + 1) * 8192 + 512; }
template <int DH>
constexpr int attn_bwd_long_dkv_lds() { return (2 * HeadDim<DH>::kImgs + 2) * 8192; }

// launch 1: one workgroup per (batch, head, 64-query tile); delta over the key tiles, then dQ over them again
template <int DH, bool kDrop>
__global__ __launch_bounds__(kBwdThreads) void attn_bwd_long_dq_kernel(AttnArgs p, float* delta_ws, int tiles,
                                                                        int Lp) {
  using LD = HeadDim<DH>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wid >> 1, wj = wid & 1;
  const int l31 = lane & 31, lhi = lane >> 5;
  const long long bh = blockIdx.x / tiles;            // grid = B * H * tiles < 2^31 (checked by the host side)
  const int qt = (int)(blockIdx.x - bh * tiles);
  const LongSeq sq = long_seq(p, bh);
  const int qs = qt * kL;
  if (qs >= sq.Lq_tot) return;                        // the whole workgroup
  const int Lq = min(sq.Lq_tot - qs, kL);
  char* const k_img = smem;                                         // K[key][d]   tr images (rows = key)
  char* const ds_img = smem + LD::kImgs * 8192;                     // dS[q][key]  tr image, read row-wise
  float* const dl = reinterpret_cast<float*>(ds_img + 8192);        // [2][64] delta over the keys of waves wi = 0, 1
  const int ldq = (int)p.ldq, ldk = (int)p.ldk, ldv = (int)p.ldv, lddo = (int)p.lddo;
  const long long qrow = (long long)(sq.q0 + qs);
  const int hc = sq.h * DH;
  const __amdgpu_buffer_rsrc_t qrs = head_rsrc<DH>(p.q + qrow * p.ldq + hc, p.ldq, Lq);
  const __amdgpu_buffer_rsrc_t dors = head_rsrc<DH>(p.d_o + qrow * p.lddo + hc, p.lddo, Lq);
  bf16x8 fq[LD::kSteps], fdo[LD::kSteps];
  long_frags<DH>(qrs, ldq, wj * 32 * ldq * 2, lane, fq);
  long_frags<DH>(dors, lddo, wj * 32 * lddo * 2, lane, fdo);
  const int q = wj * 32 + l31;
  const float lse2 = q < Lq ? p.lse[(qrow + q) * p.H + sq.h] * 1.4426950408889634f : 0.f;
  const int k_tiles = (sq.Lk_tot + kL - 1) / kL;
  const int nkt = p.causal ? min(qt + 1, k_tiles) : k_tiles;
  // ---- first sweep: delta[q] = sum_key P * (dPd o m / keep), fp32; this wave's 32 keys of every tile ----------
  float delta = 0.f;
  for (int kt = 0; kt < nkt; ++kt) {
    const int ks = kt * kL;
    const int Lk = min(sq.Lk_tot - ks, kL);
    const long long krow = (long long)(sq.k0 + ks);
    const __amdgpu_buffer_rsrc_t krs = head_rsrc<DH>(p.k + krow * p.ldk + hc, p.ldk, Lk);
    const __amdgpu_buffer_rsrc_t vrs = head_rsrc<DH>(p.v + krow * p.ldv + hc, p.ldv, Lk);
    bf16x8 fk[LD::kSteps], fv[LD::kSteps];
    long_frags<DH>(krs, ldk, wi * 32 * ldk * 2, lane, fk);
    long_frags<DH>(vrs, ldv, wi * 32 * ldv * 2, lane, fv);
    float pv[16], pd[16], dpm[16];
    long_bwd_block<DH, kDrop>(p, sq, Lp, fk, fq, fv, fdo, wi, wj, lane, qs, ks, Lq, Lk, lse2, pv, pd, dpm);
#pragma unroll
    for (int r = 0; r < 16; ++r) delta += pv[r] * dpm[r];
  }
  delta = half_sum(delta);
  if (lhi == 0) dl[wi * 64 + q] = delta;
  __syncthreads();
  delta = dl[q] + dl[64 + q];      // the same order in both waves of a query block
  if (wi == 0 && lhi == 0 && q < Lq) delta_ws[(qrow + q) * p.H + sq.h] = delta;
  // ---- second sweep: dS, dQ ------------------------------------------------------------------------------
  f32x16 dq[long_own<DH>()];
#pragma unroll
  for (int n = 0; n < long_own<DH>(); ++n)
#pragma unroll
    for (int e = 0; e < 16; ++e) dq[n][e] = 0.f;
  for (int kt = 0; kt < nkt; ++kt) {
    const int ks = kt * kL;
    const int Lk = min(sq.Lk_tot - ks, kL);
    const long long krow = (long long)(sq.k0 + ks);
    const __amdgpu_buffer_rsrc_t krs = head_rsrc<DH>(p.k + krow * p.ldk + hc, p.ldk, Lk);
    const __amdgpu_buffer_rsrc_t vrs = head_rsrc<DH>(p.v + krow * p.ldv + hc, p.ldv, Lk);
    bf16x8 fk[LD::kSteps], fv[LD::kSteps];
    long_frags<DH>(krs, ldk, wi * 32 * ldk * 2, lane, fk);
    long_frags<DH>(vrs, ldv, wi * 32 * ldv * 2, lane, fv);
    long_stage<DH>(k_img, krs, ldk, tid);
    float pv[16], pd[16], dpm[16], ds[16];
    long_bwd_block<DH, kDrop>(p, sq, Lp, fk, fq, fv, fdo, wi, wj, lane, qs, ks, Lq, Lk, lse2, pv, pd, dpm);
#pragma unroll
    for (int r = 0; r < 16; ++r) ds[r] = pv[r] * (dpm[r] - delta);
    long_store_img(ds_img, q, wi * 32 + 4 * lhi, ds);
    __syncthreads();
    // dQ^T[d][q] += sum_key K[key][d] dS[q][key]: B operand = 8 consecutive keys of row q
#pragma unroll
    for (int n = 0; n < long_own<DH>(); ++n) {
      const int db = wi + 2 * n;
      if (db >= LD::kDBlocks) continue;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        if (kk * 16 >= Lk) continue;
        const bf16x8 dsrow = *reinterpret_cast<const bf16x8*>(ds_img + tr_off(q, kk * 16 + lhi * 8));
        dq[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(k_img + (db >> 1) * 8192, db & 1, kk, lane), dsrow,
                                                        dq[n], 0, 0, 0);
      }
    }
    __syncthreads();      // the images are rewritten by the next key tile
  }
  if (wj * 32 < Lq) {
#pragma unroll
    for (int n = 0; n < long_own<DH>(); ++n) {
      const int db = wi + 2 * n;
      if (db < LD::kDBlocks)
        store_dT_quad<DH>(dq[n], db, wj, p.dq + qrow * p.lddq + hc, p.lddq, Lq, p.scale, lane);
    }
  }
}

// launch 2: one workgroup per (batch, head, 64-key tile); dK and dV over the query tiles
template <int DH, bool kDrop>
__global__ __launch_bounds__(kBwdThreads) void attn_bwd_long_dkv_kernel(AttnArgs p, const float* delta_ws,
                                                                         int tiles, int Lp) {
  using LD = HeadDim<DH>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wid >> 1, wj = wid & 1;
  const int l31 = lane & 31, lhi = lane >> 5;
  const long long bh = blockIdx.x / tiles;            // grid = B * H * tiles < 2^31 (checked by the host side)
  const int kt = (int)(blockIdx.x - bh * tiles);
  const LongSeq sq = long_seq(p, bh);
  const int ks = kt * kL;
  if (ks >= sq.Lk_tot) return;                        // the whole workgroup
  const int Lk = min(sq.Lk_tot - ks, kL);
  char* const do_img = smem;                                        // dO[q][d]    tr images (rows = q)
  char* const q_img = smem + LD::kImgs * 8192;                      // Q[q][d]     tr images (rows = q)
  char* const pd_img = smem + 2 * LD::kImgs * 8192;                 // Pd[q][key]  tr image  (rows = q)
  char* const ds_img = pd_img + 8192;                               // dS[q][key]  tr image  (rows = q)
  const int ldq = (int)p.ldq, ldk = (int)p.ldk, ldv = (int)p.ldv, lddo = (int)p.lddo;
  const long long krow = (long long)(sq.k0 + ks);
  const int hc = sq.h * DH;
  const __amdgpu_buffer_rsrc_t krs = head_rsrc<DH>(p.k + krow * p.ldk + hc, p.ldk, Lk);
  const __amdgpu_buffer_rsrc_t vrs = head_rsrc<DH>(p.v + krow * p.ldv + hc, p.ldv, Lk);
  bf16x8 fk[LD::kSteps], fv[LD::kSteps];
  long_frags<DH>(krs, ldk, wi * 32 * ldk * 2, lane, fk);
  long_frags<DH>(vrs, ldv, wi * 32 * ldv * 2, lane, fv);
  f32x16 dv[long_own<DH>()], dk[long_own<DH>()];
#pragma unroll
  for (int n = 0; n < long_own<DH>(); ++n)
#pragma unroll
    for (int e = 0; e < 16; ++e) { dv[n][e] = 0.f; dk[n][e] = 0.f; }
  const int q_tiles = (sq.Lq_tot + kL - 1) / kL;
  // causal: the query tiles before this key tile see none of its keys
  for (int qt = p.causal ? kt : 0; qt < q_tiles; ++qt) {
    const int qs = qt * kL;
    const int Lq = min(sq.Lq_tot - qs, kL);
    const long long qrow = (long long)(sq.q0 + qs);
    const __amdgpu_buffer_rsrc_t qrs = head_rsrc<DH>(p.q + qrow * p.ldq + hc, p.ldq, Lq);
    const __amdgpu_buffer_rsrc_t dors = head_rsrc<DH>(p.d_o + qrow * p.lddo + hc, p.lddo, Lq);
    bf16x8 fq[LD::kSteps], fdo[LD::kSteps];
    long_frags<DH>(qrs, ldq, wj * 32 * ldq * 2, lane, fq);
    long_frags<DH>(dors, lddo, wj * 32 * lddo * 2, lane, fdo);
    long_stage<DH>(do_img, dors, lddo, tid);
    long_stage<DH>(q_img, qrs, ldq, tid);
    const int q = wj * 32 + l31;
    float lse2 = 0.f, delta = 0.f;
    if (q < Lq) {
      lse2 = p.lse[(qrow + q) * p.H + sq.h] * 1.4426950408889634f;
      delta = delta_ws[(qrow + q) * p.H + sq.h];
    }
    float pv[16], pd[16], dpm[16], ds[16];
    long_bwd_block<DH, kDrop>(p, sq, Lp, fk, fq, fv, fdo, wi, wj, lane, qs, ks, Lq, Lk, lse2, pv, pd, dpm);
#pragma unroll
    for (int r = 0; r < 16; ++r) ds[r] = pv[r] * (dpm[r] - delta);
    long_store_img(pd_img, q, wi * 32 + 4 * lhi, pd);
    long_store_img(ds_img, q, wi * 32 + 4 * lhi, ds);
    __syncthreads();
    // dV^T[d][key] += sum_q dO[q][d] Pd[q][key], dK^T[d][key] += sum_q Q[q][d] dS[q][key]: all four operands by
    // transpose reads (rows = q)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (kk * 16 >= Lq) continue;
      const bf16x8 fpd = frag_tr(pd_img, wj, kk, lane), fds = frag_tr(ds_img, wj, kk, lane);
#pragma unroll
      for (int n = 0; n < long_own<DH>(); ++n) {
        const int db = wi + 2 * n;
        if (db >= LD::kDBlocks) continue;
        const int io = (db >> 1) * 8192, mt = db & 1;
        dv[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(do_img + io, mt, kk, lane), fpd, dv[n], 0, 0, 0);
        dk[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(q_img + io, mt, kk, lane), fds, dk[n], 0, 0, 0);
      }
    }
    __syncthreads();      // the images are rewritten by the next query tile
  }
  if (wj * 32 < Lk) {
#pragma unroll
    for (int n = 0; n < long_own<DH>(); ++n) {
      const int db = wi + 2 * n;
      if (db >= LD::kDBlocks) continue;
      store_dT_quad<DH>(dv[n], db, wj, p.dv + krow * p.lddv + hc, p.lddv, Lk, 1.f, lane);
      store_dT_quad<DH>(dk[n], db, wj, p.dk + krow * p.lddk + hc, p.lddk, Lk, p.scale, lane);
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------
// the bounds of multi-tile training (forward with dropout, backward): max_len, and grids of one workgroup per
// (batch, head, tile)
static int attn_long_check(int B, int H, int max_len) {
  if (max_len > kAttnLongMaxLen) return OS2S_ERR_INVALID_ARG;
  const long long tiles = (max_len + kL - 1) / kL;
  if ((long long)B * H * tiles >= (1ll << 31)) return OS2S_ERR_INVALID_ARG;
  return OS2S_OK;
}

}  // namespace os2s
