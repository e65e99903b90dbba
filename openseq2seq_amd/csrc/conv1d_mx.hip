// MXFP8 inference conv1d (stride 1) on the block-scaled matrix instruction of gfx950, hand-written:
//
//   y[b, t, co] = act(ch_scale[co] * sum_{k, ci} deq(xq)[b, t + k dil - padL, ci] * deq(wq)[k, co, ci] + ch_shift[co])
//   y[b, t, :]  = 0 for t >= out_len[b]
//
// tf.layers.conv1d(use_bias=False) + tf.layers.batch_normalization(training=False) + activation_fn of the speech
// encoders in eval / infer mode (open_seq2seq/parts/cnns/conv_blocks.py:195-232): the BatchNorm of an eval pass is a
// per-channel affine map and sits in the epilogue, so the raw convolution output never reaches memory.
//
// ---- operands (format and scale layout: the head of gemm_mx.hip; no new quantiser) ---------------------------
// xq [B, Tin, Cin] e4m3 and x_scale [ceil(Cin/128)][B*Tin] words: os2s_mx_quantize_rows of the [B*Tin, Cin] view of
// the activation. wq [K, Cout, Cin] and w_scale [ceil(Cin/128)][K*Cout]: the same of the [K*Cout, Cin] view of the
// weights: scale blocks run along Cin, per tap. The activation is quantised ONCE along the channels and every tap
// reuses the bytes and the scale words: the A-side scale word of output row t under tap k is the word of INPUT
// row t + k dil - padL.
//
// ---- tile --------------------------------------------------------------------------------------------------
// 256 output rows of ONE sample x 256 output channels, 8 waves as 2 x 4, wave tile 128 x 64 = 4 x 2 accumulator
// blocks of v_mfma_scale_f32_32x32x64_f8f6f4: the tile, scale routing and epilogue patch of gemm_nt_mx_kernel. The
// reduction runs over the flattened (channel tile of 128, tap) loop, 2 MFMA steps each (1 in the last channel tile
// when Cin % 128 == 64).
//   slab: per channel tile ONE slab of S = 256 + (K-1) dil input rows x 128 bytes (rows t0 - padL ..) serves all K
//     taps: tap k reads its A fragments at slab row offset k dil. The A side of the global and DMA traffic is 1/K
//     of an im2col GEMM's. Staged by buffer-load-to-LDS, 8 rows per instruction, ceil(S/8) <= 40 instructions over
//     the 8 waves, double-buffered across channel tiles (the next slab is issued under tap 0 of this one).
//   W: per (channel tile, tap) 256 x 128 bytes, double-buffered across the flattened loop, as in the GEMM.
//   LDS: 2 x 40 KB slab + 2 x 32 KB W = 144 KB ((K-1) dil <= 64); the 8 epilogue patches reuse the first 68 KB.
//   zeros from the descriptor: the slab's buffer descriptor starts at the sample and ends at row in_len[b]. A row
//     at or past the length lies behind its end and reads as 0 with no test. A row of the left padding has a
//     negative offset; as an unsigned number that is behind the end too, but its last 16 bytes (offset -16) end
//     exactly at the wrap of 32-bit arithmetic, so such a lane is sent to offset 2^31 instead (one select per DMA
//     instruction, 5 a wave per channel tile): no byte in front of the sample is ever addressed. The scale word of
//     such rows is loaded from a clamped row: any finite scale times zero elements is zero. W has one descriptor
//     for all taps, from column n0 to the end of the last tap: a column past Cout reads the next tap's rows (or 0
//     in the last tap) into accumulator columns that are never stored.
//   swizzle: 16-byte slot q of slab row s is stored at slot q ^ ((s >> 1) & 7), keyed on the SLAB row, applied on
//     the global side of the DMA. A ds_read_b128 phase is 16 lanes = 16 consecutive slab rows s0 .. s0 + 15 reading
//     the same logical slot; two rows of 128 bytes fill one 256-byte line of the 64 banks, so the 16-byte chunk a
//     lane hits is 8 (s & 1) + (q ^ ((s >> 1) & 7)). s0 = 32 im + k dil is even for an even tap offset: 8 row
//     pairs, 8 different keys, both parities: 16 different chunks. For an ODD offset the 16 rows touch nine row
//     pairs, and the first and the ninth (s0 >> 1 and s0 >> 1 + 8) share a key. But the first pair contributes only
//     its odd row and the ninth only its even row: chunks 8 + (q ^ key) and (q ^ key), different halves of the line.
//     The seven pairs between have the seven other keys. Sixteen different chunks again: the swizzle of gemm_mx.hip
//     is conflict-free for every tap offset, nothing else was needed.
//   loop: wait for (W of this step, slab if the channel tile starts), barrier, issue the W DMA and the six scale
//     words of the next step (and the next slab under tap 0), then 2 x (6 fragments + 8 MFMAs). One barrier a step.
//   A tile that starts at or past out_len[b] only writes zeros. Rows at or past out_len[b] of a live tile are
//     zeroed in the epilogue; rows at or past Tout and columns at or past Cout are not stored.
//   epilogue: accumulators -> this wave's LDS patch -> 8 columns per lane: fp32 ch_scale / ch_shift, ReLU, length
//     mask, one 16-byte store of bf16 (two of fp32).
#include <type_traits>

#include "mx_common.hpp"

namespace os2s {

struct MxConvArgs {
  const uint8_t* x; const uint32_t* x_scale; const uint8_t* w; const uint32_t* w_scale;
  void* y; const int32_t* in_len; const int32_t* out_len; const float* ch_scale; const float* ch_shift;
  long long y_stride_b, y_stride_t;
  int B, Tin, Cin, Cout, K, dil, padL, Tout, act, out_f32, MT, NT, U;
};

constexpr int kMxConvMaxHalo = 64;                                   // (K - 1) dil
constexpr int kMxSlab = (kMxTile + kMxConvMaxHalo) * kMxKTile;       // 40 KB: 40 DMA instructions of 1 KB
constexpr size_t kMxConvLds = 2 * kMxSlab + 2 * kMxOperand;          // 144 KB
constexpr int kMxBehind = (int)0x80000000u;                          // an offset behind the end of every descriptor

// eight outputs of one row: bf16 as one 16-byte store, fp32 as two
__device__ __forceinline__ void mx_conv_store8(const MxConvArgs& p, int b, int t, int col, const float (&v)[8]) {
  const long long o = (long long)b * p.y_stride_b + (long long)t * p.y_stride_t + col;
  if (p.out_f32) {
    float* const dst = reinterpret_cast<float*>(p.y) + o;
    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
  } else {
    *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(p.y) + o) = pack8(v);
  }
}

__global__ __launch_bounds__(512, 1) void conv1d_mx_kernel(MxConvArgs p) {
  constexpr int MI = 4, NI = 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 2, wn = wid & 3;
  // Workgroup blockIdx.x runs on XCD blockIdx.x & 7. The column tiles of one row tile stay behind one XCD's L2
  // (they share the slab); consecutive ROW tiles — the tiles of one sample — go round the 8 XCDs, so the live
  // tiles of a ragged batch spread evenly over them. (Measured against the GEMM's contiguous rank range per XCD at
  // the Jasper shapes: no difference beyond the spread; kept because it is the simpler index arithmetic.)
  const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int jm = j / p.NT, n_idx = j - jm * p.NT;
  const int m_blk = jm * 8 + xcd;
  if (m_blk >= p.B * p.MT) return;                   // the grid is rounded up to 8 row tiles
  const int b = m_blk / p.MT;
  const int t0 = (m_blk - b * p.MT) * kMxTile, n0 = n_idx * kMxTile;
  const int lin = p.in_len ? min(max(p.in_len[b], 0), p.Tin) : p.Tin;
  const int lout = p.out_len ? min(max(p.out_len[b], 0), p.Tout) : p.Tout;

  if (t0 >= lout) {       // the whole tile lies past the sample's end: zeros, no matrix work
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int u = tid; u < kMxTile * 32; u += 512) {
      const int t = t0 + (u >> 5), col = n0 + (u & 31) * 8;
      if (t < p.Tout && col < p.Cout) mx_conv_store8(p, b, t, col, z);
    }
    return;
  }

  const int halo = (p.K - 1) * p.dil;
  const int nslab = (kMxTile + halo + 7) >> 3;       // DMA instructions of one slab, 8 rows each
  const int r0 = t0 - p.padL;                        // the input row of slab row 0
  // x: this sample, ending with row lin - 1. w: columns n0 .. of tap 0 up to the end of the last tap
  const __amdgpu_buffer_rsrc_t xrs = mx_rsrc(p.x + (long long)b * p.Tin * p.Cin, (long long)lin * p.Cin);
  const __amdgpu_buffer_rsrc_t wrs =
      mx_rsrc(p.w + (long long)n0 * p.Cin, ((long long)p.K * p.Cout - n0) * p.Cin);
  auto stage_slab = [&](int ct, int buf) {
    char* const s = smem + buf * kMxSlab;
#pragma unroll
    for (int pi = 0; pi < 5; ++pi) {
      const int i = pi * 8 + wid;                    // instruction i covers slab rows 8 i .. 8 i + 7
      if (i < nslab) {
        const int row = i * 8 + (lane >> 3), slot = (lane & 7) ^ ((row >> 1) & 7);
        const int off = (r0 + row) * p.Cin + slot * 16 + ct * kMxKTile;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(s + i * 1024), 16,
                                                 r0 + row < 0 ? kMxBehind : off, 0, 0, 0);
      }
    }
  };
  int wv[4];
#pragma unroll
  for (int pi = 0; pi < 4; ++pi) {
    const int row = (pi * 8 + wid) * 8 + (lane >> 3), slot = (lane & 7) ^ ((row >> 1) & 7);
    wv[pi] = row * p.Cin + slot * 16;
  }
  const int tap_bytes = p.Cout * p.Cin;
  auto stage_w = [&](int ct, int k, int buf) {
    char* const s = smem + 2 * kMxSlab + buf * kMxOperand;
    const int o = k * tap_bytes + ct * kMxKTile;
#pragma unroll
    for (int pi = 0; pi < 4; ++pi)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          wrs, (__attribute__((address_space(3))) void*)(s + (pi * 8 + wid) * 1024), 16, wv[pi] + o, 0, 0, 0);
  };
  // scale words of one step: input rows of the wave's 4 row blocks under tap k, columns of its 2 column blocks
  const int arow0 = r0 + wm * 128 + l31, wcol0 = n0 + wn * 64 + l31;
  auto load_scales = [&](int ct, int k, uint32_t (&sa)[MI], uint32_t (&sw)[NI]) {
    const uint32_t* const xs = p.x_scale + ((long long)ct * p.B + b) * p.Tin;
    const uint32_t* const ws = p.w_scale + ((long long)ct * p.K + k) * p.Cout;
#pragma unroll
    for (int im = 0; im < MI; ++im)      // a row outside [0, Tin) is all zeros: any scale will do
      sa[im] = xs[min(max(arow0 + im * 32 + k * p.dil, 0), p.Tin - 1)];
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
  const int abase = wm * 128 * kMxKTile, wbase = 2 * kMxSlab + wn * 64 * kMxKTile;

  const int nct = (p.Cin + kMxKTile - 1) / kMxKTile;
  const int nsteps = nct * p.K;
  const bool half_tail = (p.Cin & (kMxKTile - 1)) != 0;
  const int sh = lhi * 8;
  uint32_t sa_n[MI], sw_n[NI];
  stage_slab(0, 0);
  stage_w(0, 0, 0);
  load_scales(0, 0, sa_n, sw_n);
  int ct = 0, k = 0;
  for (int it = 0; it < nsteps; ++it) {
    uint32_t sa[MI], sw[NI];
#pragma unroll
    for (int im = 0; im < MI; ++im) sa[im] = sa_n[im] >> sh;
#pragma unroll
    for (int in = 0; in < NI; ++in) sw[in] = sw_n[in] >> sh;
    // this step's W (and slab) have landed — this wave's share, the barrier makes it everybody's — and nobody
    // reads the other W stage (last read in step it - 1) or the other slab (last read in channel tile ct - 1)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    mx_barrier();
    int kn = k + 1, ctn = ct;
    if (kn == p.K) { kn = 0; ++ctn; }
    if (it + 1 < nsteps) {
      stage_w(ctn, kn, (it + 1) & 1);
      load_scales(ctn, kn, sa_n, sw_n);
    }
    if (k == 0 && ct + 1 < nct) stage_slab(ct + 1, (ct + 1) & 1);
    const char* const sl = smem + (ct & 1) * kMxSlab + abase;
    const char* const sw_lds = smem + wbase + (it & 1) * kMxOperand;
    // A fragment offsets of this tap: slab row l31 + k dil of the 32-row block, the swizzle keyed on that row (the
    // block bases are multiples of 32)
    const int srow = l31 + k * p.dil, key = (srow >> 1) & 7;
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
    if (!(half_tail && ct == nct - 1)) mfma_step(std::integral_constant<int, 1>{});
    k = kn;
    ct = ctn;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- epilogue (the accumulator layout: mx_acc_to_patch) ----
  float* const patch = reinterpret_cast<float*>(smem + wid * kMxPatch);
  const int rr = lane >> 3, c8 = (lane & 7) * 8;
  const int col = n0 + wn * 64 + c8;
  float cs[8], cb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { cs[e] = 1.f; cb[e] = 0.f; }
  if (p.ch_scale && col < p.Cout) load8(p.ch_scale + col, cs);
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
          v[e] = v[e] * cs[e] + cb[e];
          if (p.act == 1) v[e] = fmaxf(v[e], 0.f);
          if (t >= lout) v[e] = 0.f;
        }
        mx_conv_store8(p, b, t, col, v);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace os2s

extern "C" int os2s_conv1d_fwd_mx(os2s_stream_t stream, const uint8_t* xq, const uint8_t* x_scale, const uint8_t* wq,
                                  const uint8_t* w_scale, void* y, const int32_t* in_len, const int32_t* out_len,
                                  const float* ch_scale, const float* ch_shift, int B, int Tin, int Cin, int Cout,
                                  int K, int dil, int padL, int Tout, long long y_stride_b, long long y_stride_t,
                                  int out_f32, int act) {
  using namespace os2s;
  OS2S_REQUIRE(xq && x_scale && wq && w_scale && y);
  OS2S_REQUIRE(B >= 1 && Tin >= 1 && Tout >= 1 && K >= 1 && dil >= 1 && Cin >= 1 && Cout >= 1);
  if (Cin < 64 || Cin % 64 != 0 || Cout % 8 != 0) return OS2S_ERR_UNSUPPORTED;
  if ((long long)(K - 1) * dil > kMxConvMaxHalo) return OS2S_ERR_UNSUPPORTED;
  if (act != 0 && act != 1) return OS2S_ERR_UNSUPPORTED;
  const int halo = (K - 1) * dil;
  OS2S_REQUIRE(padL >= 0 && padL <= halo);
  OS2S_REQUIRE(y_stride_t >= Cout && y_stride_t % 8 == 0 && y_stride_b % 8 == 0);
  OS2S_REQUIRE(((uintptr_t)xq | (uintptr_t)wq | (uintptr_t)y | (uintptr_t)ch_scale | (uintptr_t)ch_shift) % 16 == 0);
  OS2S_REQUIRE(((uintptr_t)x_scale | (uintptr_t)w_scale | (uintptr_t)in_len | (uintptr_t)out_len) % 4 == 0);
  // 32-bit byte offsets: inside a sample for the slab (rows -padL .. Tout + 8 + halo), inside wq for W
  const long long span = (long long)(Tin > Tout ? Tin : Tout) + kMxTile + halo + 8;
  if (span * Cin >= (1ll << 31) || ((long long)K * Cout + kMxTile) * Cin >= (1ll << 31)) return OS2S_ERR_UNSUPPORTED;
  MxConvArgs p;
  p.x = xq; p.x_scale = reinterpret_cast<const uint32_t*>(x_scale);
  p.w = wq; p.w_scale = reinterpret_cast<const uint32_t*>(w_scale);
  p.y = y; p.in_len = in_len; p.out_len = out_len; p.ch_scale = ch_scale; p.ch_shift = ch_shift;
  p.y_stride_b = y_stride_b; p.y_stride_t = y_stride_t;
  p.B = B; p.Tin = Tin; p.Cin = Cin; p.Cout = Cout; p.K = K; p.dil = dil; p.padL = padL; p.Tout = Tout;
  p.act = act; p.out_f32 = out_f32;
  p.MT = ceil_div(Tout, kMxTile);
  p.NT = ceil_div(Cout, kMxTile);
  const long long U = ((long long)B * p.MT + 7) / 8 * 8 * p.NT;      // row tiles rounded up to the 8 XCDs
  if (U >= (1ll << 31)) return OS2S_ERR_UNSUPPORTED;
  p.U = (int)U;
  OS2S_LAUNCH_LDS(conv1d_mx_kernel, dim3(p.U), dim3(512), kMxConvLds, (hipStream_t)stream, p);
  return OS2S_OK;
}
