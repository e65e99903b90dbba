// MXFP8 inference residual block end in ONE launch on the block-scaled matrix instruction of gfx950, hand-written:
//
//   y[b, t, co] = act( sum_{k, ci} deq(xq)[b, t + k dil - padL, ci] * deq(wq)[k, co, ci]
//                    + sum_{r < R} sum_ci deq(sq_r)[b, t, ci] * deq(vq_r)[co, ci]  +  ch_shift[co] )
//   y[b, t, :]  = 0 for t >= out_len[b]
//
// conv_bn_res_bn_actv of the speech encoders in eval / infer mode (open_seq2seq/parts/cnns/conv_blocks.py:61-168):
// the main tf.layers.conv1d, one 1x1 tf.layers.conv1d per residual input, a tf.layers.batch_normalization
// (training=False) behind each, their sum and activation_fn. A BatchNorm on moving statistics is a per-channel affine
// map: its scale goes into the ROWS of its branch's weights on the host before they are quantised, the shifts add up
// to one vector. What is left is one accumulation — the K taps of the main convolution plus one tap per residual
// source — and the epilogue of conv1d_mx.hip without its scale. No branch tensor, no raw y, no sum pass.
//
// ---- operands ------------------------------------------------------------------------------------------------
// xq / x_scale / wq / w_scale: as os2s_conv1d_fwd_mx (conv1d_mx.hip). Source r: sq_r [B, Tout, C_r] e4m3 with the
// scale words of os2s_mx_quantize_rows of its [B*Tout, C_r] view; vq_r [Cout, C_r] and the words of that view. The
// sources come as a table of up to 16 os2s_mx_res_src_t, copied into the kernel arguments.
//
// ---- tile and step sequence ------------------------------------------------------------------------------------
// The tile of conv1d_mx_kernel: 256 output rows of ONE sample x 256 output channels, 8 waves as 2 x 4, wave tile
// 128 x 64 = 4 x 2 accumulator blocks of v_mfma_scale_f32_32x32x64_f8f6f4 (fragments, scale routing, patch:
// mx_common.hpp). The reduction is ONE flattened step sequence walked by a cursor (operand, channel tile, tap):
//   operand -1, the main convolution: (channel tile of 128, tap) steps in exactly conv1d_mx_kernel's order — with
//     R = 0 the accumulators, and so the output, have that kernel's bits;
//   operand r = 0 .. R-1, the residual sources in table order: one step per channel tile of C_r, one tap.
// Each step is 2 MFMA steps of 64 channels (1 in an operand's last channel tile when C % 128 == 64). The loop body
// does not know which kind of step it runs: an operand is a record (A base / rows / live rows / first slab row /
// slab height / taps, W base, the two scale bases, C) built from the arguments by one function, and a residual
// source is the record of a one-tap convolution with no padding whose input has Tout rows.
//   slab: per (operand, channel tile) ONE slab of A rows x 128 bytes. Main: 256 + (K-1) dil rows from input row
//     t0 - padL, tap k reads at slab row offset k dil. Residual: 256 rows from row t0, no halo, read at offset 0.
//     Staged by buffer-load-to-LDS, 8 rows per instruction, double-buffered across SLABS: the step that opens a slab
//     issues the next one (the next main channel tile, the first tile of source 0, the next tile of a source, the
//     first tile of the next source — one cursor), so a residual step stages the next residual slab while it computes.
//   W: per step 256 x 128 bytes (main: tap k's rows n0 .. of wq; residual: rows n0 .. of vq_r), double-buffered
//     across steps.
//   zeros from the descriptor: as conv1d_mx.hip. A source's descriptor starts at the sample and ends at row
//     out_len[b]: rows past it read as 0 (they only feed output rows the mask zeroes). A residual slab has no row in
//     front of the sample, the main slab's left padding goes to an offset behind the end. W descriptors run from
//     column n0 to the end of the operand's weights: a column past Cout reads the next tap (main) or 0.
//   LDS map (bytes): [0, 40 K) slab 0, [40 K, 80 K) slab 1, [80 K, 112 K) W 0, [112 K, 144 K) W 1 = 144 KB of 160;
//     a residual slab fills the first 32 KB of its buffer. The 8 epilogue patches (8.5 KB each) reuse [0, 68 K).
//   swizzle: 16-byte slot q of slab row s sits at slot q ^ ((s >> 1) & 7), keyed on the slab row. conv1d_mx.hip
//     shows that the 16 lanes of a ds_read_b128 phase — 16 consecutive slab rows s0 .. s0 + 15 at one logical slot —
//     hit 16 different 16-byte chunks of the 256-byte bank line for EVERY s0, even or odd. A residual step reads at
//     tap offset 0: s0 = 32 im + 16 j is a multiple of 16, the even case: 8 row pairs, 8 different keys, both
//     parities. Conflict-free with nothing added; W tiles use the same rule on their own rows as there.
//   loop: wait for (this step's W, its slab if it opens one), barrier, issue the next step's W DMA and six scale
//     words (and, when this step opens a slab, the next slab), then 2 x (6 fragments + 8 MFMAs). ONE barrier a step.
//   A tile that starts at or past out_len[b] writes zeros and does no matrix work.
//   epilogue: accumulators -> this wave's LDS patch -> 8 columns per lane: + ch_shift, ReLU, length mask, one
//     16-byte store of bf16 (two of fp32).
//
// ---- resources (hipcc of ROCm 7, -O3, gfx950; -Rpass-analysis=kernel-resource-usage) --------------------------
// conv1d_block_end_mx_kernel: 207 VGPRs (128 of them the accumulators; conv1d_mx_kernel: 206), no AGPRs, 80 SGPRs,
// no scratch, no spills, 144 KB dynamic LDS, occupancy 2 waves / SIMD = one workgroup of 8 waves per CU, as
// conv1d_mx_kernel. The operand records and both cursors stay in SGPRs.
#include <type_traits>

#include "mx_common.hpp"

namespace os2s {

constexpr int kMxMaxSources = 16;

struct MxBlockEndArgs {
  const uint8_t* x; const uint32_t* x_scale; const uint8_t* w; const uint32_t* w_scale;
  void* y; const int32_t* in_len; const int32_t* out_len; const float* ch_shift;
  long long y_stride_b, y_stride_t;
  int B, Tin, Cin, Cout, K, dil, padL, Tout, act, out_f32, MT, NT, U, R, nsteps, nslabs;
  os2s_mx_res_src_t src[kMxMaxSources];
};

constexpr int kMxEndMaxHalo = 64;                                    // (K - 1) dil, as conv1d_mx.hip
constexpr int kMxEndSlab = (kMxTile + kMxEndMaxHalo) * kMxKTile;     // 40 KB
constexpr size_t kMxEndLds = 2 * kMxEndSlab + 2 * kMxOperand;        // 144 KB
constexpr int kMxEndBehind = (int)0x80000000u;                       // an offset behind the end of every descriptor

// One operand pair of the reduction as the step loop sees it (all wave-uniform): the main convolution, or a residual
// source as a one-tap convolution without padding.
struct MxEndOperand {
  const uint8_t* a; const uint32_t* a_scale; const uint8_t* w; const uint32_t* w_scale;
  int C;        // channels = bytes per row of a and w
  int rows;     // rows of a per sample (Tin / Tout)
  int live;     // rows of this sample the descriptor covers
  int r0;       // the row of a under slab row 0
  int nslab;    // DMA instructions of one slab, 8 rows each
  int taps;     // K / 1
};

struct MxEndCursor { int op, ct, k; };                               // op -1: the main convolution

__device__ __forceinline__ void mx_end_store8(const MxBlockEndArgs& p, int b, int t, int col, const float (&v)[8]) {
  const long long o = (long long)b * p.y_stride_b + (long long)t * p.y_stride_t + col;
  if (p.out_f32) {
    float* const dst = reinterpret_cast<float*>(p.y) + o;
    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
  } else {
    *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(p.y) + o) = pack8(v);
  }
}

__global__ __launch_bounds__(512, 1) void conv1d_block_end_mx_kernel(MxBlockEndArgs p) {
  constexpr int MI = 4, NI = 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 2, wn = wid & 3;
  // the workgroup order of conv1d_mx_kernel: column tiles of one row tile behind one XCD's L2, row tiles round the XCDs
  const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int jm = j / p.NT, n_idx = j - jm * p.NT;
  const int m_blk = jm * 8 + xcd;
  if (m_blk >= p.B * p.MT) return;
  const int b = m_blk / p.MT;
  const int t0 = (m_blk - b * p.MT) * kMxTile, n0 = n_idx * kMxTile;
  const int lin = p.in_len ? min(max(p.in_len[b], 0), p.Tin) : p.Tin;
  const int lout = p.out_len ? min(max(p.out_len[b], 0), p.Tout) : p.Tout;

  if (t0 >= lout) {       // the whole tile lies past the sample's end: zeros, no matrix work
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int u = tid; u < kMxTile * 32; u += 512) {
      const int t = t0 + (u >> 5), col = n0 + (u & 31) * 8;
      if (t < p.Tout && col < p.Cout) mx_end_store8(p, b, t, col, z);
    }
    return;
  }

  auto operand = [&](int op) {
    MxEndOperand o;
    if (op < 0) {
      o.a = p.x; o.a_scale = p.x_scale; o.w = p.w; o.w_scale = p.w_scale;
      o.C = p.Cin; o.rows = p.Tin; o.live = lin; o.r0 = t0 - p.padL; o.taps = p.K;
      o.nslab = (kMxTile + (p.K - 1) * p.dil + 7) >> 3;
    } else {
      const os2s_mx_res_src_t& s = p.src[op];
      o.a = s.sq; o.a_scale = reinterpret_cast<const uint32_t*>(s.s_scale);
      o.w = s.vq; o.w_scale = reinterpret_cast<const uint32_t*>(s.v_scale);
      o.C = s.C; o.rows = p.Tout; o.live = lout; o.r0 = t0; o.taps = 1;
      o.nslab = kMxTile >> 3;
    }
    return o;
  };
  auto tiles = [&](int op) { return ((op < 0 ? p.Cin : p.src[op].C) + kMxKTile - 1) / kMxKTile; };
  // the channel tile after (op, ct): the operand's next one, or the first of the next operand
  auto next_tile = [&](int& op, int& ct) {
    if (++ct == tiles(op)) { ++op; ct = 0; }
  };

  // a: this sample of the operand, ending with its last live row
  auto stage_slab = [&](const MxEndOperand& o, int ct, int buf) {
    const __amdgpu_buffer_rsrc_t ars = mx_rsrc(o.a + (long long)b * o.rows * o.C, (long long)o.live * o.C);
    char* const s = smem + buf * kMxEndSlab;
#pragma unroll
    for (int pi = 0; pi < 5; ++pi) {
      const int i = pi * 8 + wid;                    // instruction i covers slab rows 8 i .. 8 i + 7
      if (i < o.nslab) {
        const int row = i * 8 + (lane >> 3), slot = (lane & 7) ^ ((row >> 1) & 7);
        const int off = (o.r0 + row) * o.C + slot * 16 + ct * kMxKTile;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ars, (__attribute__((address_space(3))) void*)(s + i * 1024), 16,
                                                 o.r0 + row < 0 ? kMxEndBehind : off, 0, 0, 0);
      }
    }
  };
  // w: columns n0 .. of the operand's first tap up to the end of its last tap
  int wrow[4], wslot[4];
#pragma unroll
  for (int pi = 0; pi < 4; ++pi) {
    wrow[pi] = (pi * 8 + wid) * 8 + (lane >> 3);
    wslot[pi] = ((lane & 7) ^ ((wrow[pi] >> 1) & 7)) * 16;
  }
  auto stage_w = [&](const MxEndOperand& o, int ct, int k, int buf) {
    const __amdgpu_buffer_rsrc_t wrs =
        mx_rsrc(o.w + (long long)n0 * o.C, ((long long)o.taps * p.Cout - n0) * o.C);
    char* const s = smem + 2 * kMxEndSlab + buf * kMxOperand;
    const int base = k * p.Cout * o.C + ct * kMxKTile;
#pragma unroll
    for (int pi = 0; pi < 4; ++pi)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(s + (pi * 8 + wid) * 1024),
                                               16, wrow[pi] * o.C + wslot[pi] + base, 0, 0, 0);
  };
  // scale words of one step: rows of the wave's 4 row blocks under tap k, columns of its 2 column blocks
  const int wcol0 = n0 + wn * 64 + l31;
  auto load_scales = [&](const MxEndOperand& o, int ct, int k, uint32_t (&sa)[MI], uint32_t (&sw)[NI]) {
    const uint32_t* const xs = o.a_scale + ((long long)ct * p.B + b) * o.rows;
    const uint32_t* const ws = o.w_scale + ((long long)ct * o.taps + k) * p.Cout;
    const int arow0 = o.r0 + wm * 128 + l31 + k * p.dil;
#pragma unroll
    for (int im = 0; im < MI; ++im)      // a row outside [0, rows) is all zeros: any scale will do
      sa[im] = xs[min(max(arow0 + im * 32, 0), o.rows - 1)];
#pragma unroll
    for (int in = 0; in < NI; ++in) sw[in] = ws[min(wcol0 + in * 32, p.Cout - 1)];
  };

  f32x16 acc[NI][MI];
#pragma unroll
  for (int in = 0; in < NI; ++in)
#pragma unroll
    for (int im = 0; im < MI; ++im)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[in][im][e] = 0.f;

  // W fragment offsets inside the operand tile: MFMA step ks, the lane's piece h of scale block h (as the GEMM)
  int foff[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      foff[ks][h] = l31 * kMxKTile + (((ks * 4 + h * 2 + lhi) ^ ((l31 >> 1) & 7)) << 4);
  const int abase = wm * 128 * kMxKTile, wbase = 2 * kMxEndSlab + wn * 64 * kMxKTile;

  const int sh = lhi * 8;
  uint32_t sa_n[MI], sw_n[NI];
  MxEndCursor cur = {-1, 0, 0};
  int slab = 0;                          // the slab the current step reads lives in buffer slab & 1
  int sn_op = -1, sn_ct = 0;             // the slab after it
  {
    const MxEndOperand o = operand(-1);
    stage_slab(o, 0, 0);
    stage_w(o, 0, 0, 0);
    load_scales(o, 0, 0, sa_n, sw_n);
    next_tile(sn_op, sn_ct);
  }
  for (int it = 0; it < p.nsteps; ++it) {
    uint32_t sa[MI], sw[NI];
#pragma unroll
    for (int im = 0; im < MI; ++im) sa[im] = sa_n[im] >> sh;
#pragma unroll
    for (int in = 0; in < NI; ++in) sw[in] = sw_n[in] >> sh;
    // this step's W (and slab) have landed — this wave's share, the barrier makes it everybody's — and nobody
    // reads the other W stage (last read in step it - 1) or the other slab buffer (last read in slab - 1, whose last
    // step is at most it - 1)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    mx_barrier();
    MxEndCursor nx = cur;
    if (cur.op < 0 && cur.k + 1 < p.K) {
      ++nx.k;
    } else {
      nx.k = 0;
      next_tile(nx.op, nx.ct);
    }
    if (it + 1 < p.nsteps) {
      const MxEndOperand o = operand(nx.op);
      stage_w(o, nx.ct, nx.k, (it + 1) & 1);
      load_scales(o, nx.ct, nx.k, sa_n, sw_n);
    }
    if (cur.k == 0 && slab + 1 < p.nslabs) {         // this step opened a slab: the next one goes out under it
      stage_slab(operand(sn_op), sn_ct, (slab + 1) & 1);
      next_tile(sn_op, sn_ct);
    }
    const int C = cur.op < 0 ? p.Cin : p.src[cur.op].C;
    const bool one_step = (C & (kMxKTile - 1)) != 0 && cur.ct == (C >> 7);     // the operand's 64-channel tail
    const char* const sl = smem + (slab & 1) * kMxEndSlab + abase;
    const char* const sw_lds = smem + wbase + (it & 1) * kMxOperand;
    // A fragment offsets of this tap: slab row l31 + k dil of the 32-row block, the swizzle keyed on that row (the
    // block bases are multiples of 32); a residual step has k = 0
    const int srow = l31 + cur.k * p.dil, key = (srow >> 1) & 7;
    int aoff[2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int h = 0; h < 2; ++h) aoff[ks][h] = srow * kMxKTile + (((ks * 4 + h * 2 + lhi) ^ key) << 4);
    auto mfma_step = [&](auto KS) {
      constexpr int ks = decltype(KS)::value;
      i32x8 wf[NI], af[MI];
#pragma unroll
      for (int in = 0; in < NI; ++in) wf[in] = mx_frag(sw_lds + in * 32 * kMxKTile, foff[ks][0], foff[ks][1]);
#pragma unroll
      for (int im = 0; im < MI; ++im) af[im] = mx_frag(sl + im * 32 * kMxKTile, aoff[ks][0], aoff[ks][1]);
#pragma unroll
      for (int im = 0; im < MI; ++im)
#pragma unroll
        for (int in = 0; in < NI; ++in)
          acc[in][im] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[in], af[im], acc[in][im], 0, 0, ks * 2,
                                                                        (int)sw[in], ks * 2, (int)sa[im]);
    };
    mfma_step(std::integral_constant<int, 0>{});
    if (!one_step) mfma_step(std::integral_constant<int, 1>{});
    if (nx.k == 0) ++slab;
    cur = nx;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- epilogue (the accumulator layout: mx_acc_to_patch) ----
  float* const patch = reinterpret_cast<float*>(smem + wid * kMxPatch);
  const int rr = lane >> 3, c8 = (lane & 7) * 8;
  const int col = n0 + wn * 64 + c8;
  float cb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) cb[e] = 0.f;
  if (p.ch_shift && col < p.Cout) load8(p.ch_shift + col, cb);
#pragma unroll
  for (int im = 0; im < MI; ++im) {
#pragma unroll
    for (int in = 0; in < NI; ++in) mx_acc_to_patch(patch, acc[in][im], in, l31, lhi);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int pr = ps * 8 + rr;
      const int t = t0 + wm * 128 + im * 32 + pr;
      float v[8];
      load8(patch + pr * kMxPatchStride + c8, v);
      if (t < p.Tout && col < p.Cout) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = v[e] + cb[e];
          if (p.act == 1) v[e] = fmaxf(v[e], 0.f);
          if (t >= lout) v[e] = 0.f;
        }
        mx_end_store8(p, b, t, col, v);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace os2s

extern "C" int os2s_conv1d_block_end_fwd_mx(os2s_stream_t stream, const uint8_t* xq, const uint8_t* x_scale,
                                            const uint8_t* wq, const uint8_t* w_scale, const os2s_mx_res_src_t* src,
                                            int R, void* y, const int32_t* in_len, const int32_t* out_len,
                                            const float* ch_shift, int B, int Tin, int Cin, int Cout, int K, int dil,
                                            int padL, int Tout, long long y_stride_b, long long y_stride_t,
                                            int out_f32, int act, int variant) {
  using namespace os2s;
  OS2S_REQUIRE(xq && x_scale && wq && w_scale && y && variant == -1);
  OS2S_REQUIRE(B >= 1 && Tin >= 1 && Tout >= 1 && K >= 1 && dil >= 1 && Cin >= 1 && Cout >= 1);
  OS2S_REQUIRE(R >= 0 && (R == 0 || src));
  if (Cin < 64 || Cin % 64 != 0 || Cout % 8 != 0) return OS2S_ERR_UNSUPPORTED;
  if ((long long)(K - 1) * dil > kMxEndMaxHalo) return OS2S_ERR_UNSUPPORTED;
  if (act != 0 && act != 1) return OS2S_ERR_UNSUPPORTED;
  if (R > kMxMaxSources) return OS2S_ERR_UNSUPPORTED;
  const int halo = (K - 1) * dil;
  OS2S_REQUIRE(padL >= 0 && padL <= halo);
  OS2S_REQUIRE(y_stride_t >= Cout && y_stride_t % 8 == 0 && y_stride_b % 8 == 0);
  OS2S_REQUIRE(((uintptr_t)xq | (uintptr_t)wq | (uintptr_t)y | (uintptr_t)ch_shift) % 16 == 0);
  OS2S_REQUIRE(((uintptr_t)x_scale | (uintptr_t)w_scale | (uintptr_t)in_len | (uintptr_t)out_len) % 4 == 0);
  // 32-bit byte offsets: inside a sample for the slab (rows -padL .. Tout + 8 + halo), inside the weights for W
  const long long span = (long long)(Tin > Tout ? Tin : Tout) + kMxTile + halo + 8;
  if (span * Cin >= (1ll << 31) || ((long long)K * Cout + kMxTile) * Cin >= (1ll << 31)) return OS2S_ERR_UNSUPPORTED;
  MxBlockEndArgs p;
  p.nslabs = ceil_div(Cin, kMxKTile);
  p.nsteps = p.nslabs * K;
  for (int r = 0; r < R; ++r) {
    const os2s_mx_res_src_t& s = src[r];
    OS2S_REQUIRE(s.sq && s.s_scale && s.vq && s.v_scale);
    OS2S_REQUIRE(((uintptr_t)s.sq | (uintptr_t)s.vq) % 16 == 0 && ((uintptr_t)s.s_scale | (uintptr_t)s.v_scale) % 4 == 0);
    if (s.C < 64 || s.C % 64 != 0) return OS2S_ERR_UNSUPPORTED;
    if (((long long)Tout + kMxTile + 8) * s.C >= (1ll << 31) || ((long long)Cout + kMxTile) * s.C >= (1ll << 31))
      return OS2S_ERR_UNSUPPORTED;
    p.src[r] = s;
    p.nslabs += ceil_div(s.C, kMxKTile);
    p.nsteps += ceil_div(s.C, kMxKTile);
  }
  for (int r = R; r < kMxMaxSources; ++r) p.src[r] = os2s_mx_res_src_t{nullptr, nullptr, nullptr, nullptr, 0};
  p.x = xq; p.x_scale = reinterpret_cast<const uint32_t*>(x_scale);
  p.w = wq; p.w_scale = reinterpret_cast<const uint32_t*>(w_scale);
  p.y = y; p.in_len = in_len; p.out_len = out_len; p.ch_shift = ch_shift;
  p.y_stride_b = y_stride_b; p.y_stride_t = y_stride_t;
  p.B = B; p.Tin = Tin; p.Cin = Cin; p.Cout = Cout; p.K = K; p.dil = dil; p.padL = padL; p.Tout = Tout;
  p.act = act; p.out_f32 = out_f32; p.R = R;
  p.MT = ceil_div(Tout, kMxTile);
  p.NT = ceil_div(Cout, kMxTile);
  const long long U = ((long long)B * p.MT + 7) / 8 * 8 * p.NT;      // row tiles rounded up to the 8 XCDs
  if (U >= (1ll << 31)) return OS2S_ERR_UNSUPPORTED;
  p.U = (int)U;
  OS2S_LAUNCH_LDS(conv1d_block_end_mx_kernel, dim3(p.U), dim3(512), kMxEndLds, (hipStream_t)stream, p);
  return OS2S_OK;
}
