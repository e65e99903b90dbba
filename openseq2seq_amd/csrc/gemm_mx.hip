// MXFP8 inference GEMM on the block-scaled matrix instruction of gfx950, hand-written:
//
//   out[M,N] (bf16 or fp32) = act(deq(a)[M,K] . deq(w)[N,K]^T + bias) + residual
//
// Both operands are OCP MX: e4m3 elements, one E8M0 scale (a power of two, biased by 127) per 32 consecutive
// elements along K. The forward-only tf.layers.Dense calls of the Transformer in eval / infer mode
// (open_seq2seq/parts/transformer/attention_layer.py:54-62,125-127,219, ffn_layer.py:51-85, the logits matmul of
// embedding_layer.py:90-105). The e4m3 bytes and the scale bytes go to v_mfma_scale_f32_32x32x64_f8f6f4 as they
// are: nothing is widened to bf16 and nothing is rescaled in the loop.
//
// ---- format (mx_quantize_rows_kernel) ----------------------------------------------------------------------
// block of 32 with largest magnitude amax: e = floor(log2(amax)) - 8 (8 = the largest e4m3 exponent), scale byte
// = clamp(e + 127, 0, 254), element = RNE_e4m3(clamp(x * 2^-e, -448, 448)); an all-zero block: byte 0, zeros.
// amax is a bf16 value: floor(log2) is its exponent field, the byte is max(field - 8, 0).
//
// ---- scale layout ------------------------------------------------------------------------------------------
// scale[ceil(K/128)][rows] of 32-bit words: word (kt, r) holds the four scale bytes of row r for the K blocks
// 4 kt .. 4 kt + 3 (byte b = block 4 kt + b; blocks past K / 32 hold 0). That is one K tile of the GEMM per word:
// the 32 lanes of a half wave own 32 consecutive rows of a tile, so their scale operand of a whole K tile is ONE
// coalesced 128-byte load. In the 32x32x64 instruction lane l holds row l % 32; as the hardware reads its 32
// bytes, the first 16 are elements 16 (l / 32) .. + 15 of the 64-deep step (scale block 0) and the second 16 are
// elements 32 + 16 (l / 32) .. + 15 (scale block 1); the scale of (row, block b) is taken from lane row + 32 b, as
// one byte of a register chosen by op_sel. The two halves of a wave need different bytes under the same op_sel,
// so the upper half shifts its word down by one byte once per tile: op_sel 0 is then block 2 ks + (l / 32) of
// MFMA step ks = 0 and op_sel 2 that of ks = 1.
//
// ---- tile --------------------------------------------------------------------------------------------------
// 256 x 256 outputs, 8 waves as 2 (rows) x 4 (columns), wave tile 128 x 64 = 4 x 2 accumulator blocks of
// 32x32 (128 registers), K tile 128: a tile row is 128 bytes, two MFMA steps of 64. 32x32x64 and not 16x16x128:
// it needs half the fragment bytes per FLOP (a 32-row fragment feeds 32 columns) and the LDS read port, not the
// matrix core, is what a tile of 8-bit operands runs into first. Transformer-big eval has M = 16 384: N = 1024
// is 256 tiles, one per CU; the narrow-M tiles of the decode steps are gemm_skinny_mx.hip.
//   LDS: two stages x (A 32 KB + W 32 KB) = 128 KB, filled by buffer-load-to-LDS, 16 bytes per lane: one
//     instruction writes 8 rows x 128 bytes, 8 per wave per K tile. A lane's fragment is 32 bytes of a row = the
//     two 16-byte slots 4 ks + l / 32 and 4 ks + 2 + l / 32. Slots are stored at (slot ^ ((row >> 1) & 7)): the
//     16 lanes of one ds_read_b128 phase cover 8 row pairs, each pair fills one 256-byte line of the 64 banks, and
//     the xor puts the 8 pairs on 8 different slots — no bank conflict.
//     The swizzle is applied on the global side of the DMA (the LDS side of a DMA is lane-linear).
//   loop (double-buffered): wait for tile t, barrier, issue the DMA of tile t + 1 into the other stage and load
//     its six scale words, then 2 x (6 fragments + 8 MFMAs) of tile t. One barrier per K tile.
//   K % 128 == 64: the last tile runs one MFMA step (its second half holds whatever follows the row).
//   Rows past M and columns past N are outside the buffer descriptors and read as zeros (their lanes load the scale word of the last real row).
//   epilogue: per 32-row block, accumulators -> this wave's LDS patch (row stride 68 floats) -> 8 columns per
//     lane: bias, ReLU, residual, one 16-byte store of bf16 (two of fp32).
#include <type_traits>

#include "mx_common.hpp"

namespace os2s {

// ------------------------------------------------------------------------------------------------------------
// Quantiser: 16 lanes own one (row, K tile) unit of 128 elements, 4 lanes a block of 32, 8 elements a lane.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mx_quantize_rows_kernel(const bf16_t* __restrict__ x, long long ldx, int rows,
                                                             int K, uint8_t* __restrict__ q,
                                                             uint32_t* __restrict__ scale) {
  const int KT = (K + 127) >> 7;
  const int lane = threadIdx.x & 63, sub = lane & 15;
  const long long u = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4;
  const int r = (int)(u / KT), kt = (int)(u - (long long)r * KT);
  const int k = kt * 128 + sub * 8;
  const bool live = r < rows && k < K;        // K % 64 == 0: the last unit of a row may be half empty
  u32x4 v = {0u, 0u, 0u, 0u};
  if (live) v = *reinterpret_cast<const u32x4*>(x + (long long)r * ldx + k);
  int byte;
  const u32x2 o = mx_quantize8(v, byte);
  if (live) *reinterpret_cast<u32x2*>(q + (long long)r * K + k) = o;
  const uint32_t word = mx_scale_word(byte, lane);   // the unit's four scale bytes as one word
  if (sub == 0 && r < rows) scale[(long long)kt * rows + r] = word;
}

// ------------------------------------------------------------------------------------------------------------
// GEMM
// ------------------------------------------------------------------------------------------------------------
struct MxGemmArgs {
  const uint8_t* a; const uint32_t* a_scale; const uint8_t* w; const uint32_t* w_scale;
  void* out; const float* bias; const bf16_t* residual;
  long long lda, ldc;
  int M, N, K, act, out_f32, NT, U;
};

constexpr int kMxStage = 2 * kMxOperand;                // A + W
constexpr size_t kMxLds = 2 * kMxStage;                 // 128 KB (the 8 epilogue patches reuse 68 KB of it)

__global__ __launch_bounds__(512, 1) void gemm_nt_mx_kernel(MxGemmArgs p) {
  constexpr int MI = 4, NI = 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 2, wn = wid & 3;
  // consecutive ranks = the column tiles of one row block, behind one XCD's L2 (a contiguous rank range per XCD)
  int rank;
  {
    const int q8 = p.U >> 3, r8 = p.U & 7, x = blockIdx.x & 7;
    rank = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + (blockIdx.x >> 3);
  }
  const int m_blk = rank / p.NT, n_idx = rank - m_blk * p.NT;
  const int m0 = m_blk * kMxTile, n0 = n_idx * kMxTile;

  // the descriptors end with the last real byte: a row past M / N, and whatever follows the last row, reads as 0
  const __amdgpu_buffer_rsrc_t ars =
      mx_rsrc(p.a + (long long)m0 * p.lda, (long long)(p.M - m0 - 1) * p.lda + p.K);
  const __amdgpu_buffer_rsrc_t wrs =
      mx_rsrc(p.w + (long long)n0 * p.K, (long long)(p.N - n0) * p.K);
  // this wave's DMA instructions: 4 of the 32 of each operand tile; instruction i covers tile rows 8 i .. 8 i + 7
  int av[4], wv[4];
#pragma unroll
  for (int pi = 0; pi < 4; ++pi) {
    const int row = (pi * 8 + wid) * 8 + (lane >> 3), slot = (lane & 7) ^ ((row >> 1) & 7);
    av[pi] = row * (int)p.lda + slot * 16;
    wv[pi] = row * p.K + slot * 16;
  }
  auto stage = [&](int kt, int buf) {
    char* const s = smem + buf * kMxStage;
#pragma unroll
    for (int pi = 0; pi < 4; ++pi) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          ars, (__attribute__((address_space(3))) void*)(s + (pi * 8 + wid) * 1024), 16, av[pi] + kt * kMxKTile, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          wrs, (__attribute__((address_space(3))) void*)(s + kMxOperand + (pi * 8 + wid) * 1024), 16,
          wv[pi] + kt * kMxKTile, 0, 0, 0);
    }
  };
  // scale words of one K tile: rows of the wave's 4 row blocks, columns of its 2 column blocks
  const int arow0 = m0 + wm * 128 + l31, wrow0 = n0 + wn * 64 + l31;
  auto load_scales = [&](int kt, uint32_t (&sa)[MI], uint32_t (&sw)[NI]) {
#pragma unroll
    for (int im = 0; im < MI; ++im) {
      const int r = min(arow0 + im * 32, p.M - 1);      // a row past M is all zeros: any scale will do
      sa[im] = p.a_scale[(long long)kt * p.M + r];
    }
#pragma unroll
    for (int in = 0; in < NI; ++in) {
      const int r = min(wrow0 + in * 32, p.N - 1);
      sw[in] = p.w_scale[(long long)kt * p.N + r];
    }
  };

  f32x16 acc[NI][MI];
#pragma unroll
  for (int in = 0; in < NI; ++in)
#pragma unroll
    for (int im = 0; im < MI; ++im)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[in][im][e] = 0.f;

  // fragment offsets inside an operand tile: MFMA step ks, the lane's piece h of scale block h
  int foff[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      foff[ks][h] = l31 * kMxKTile + (((ks * 4 + h * 2 + lhi) ^ ((l31 >> 1) & 7)) << 4);
  const int abase = wm * 128 * kMxKTile, wbase = kMxOperand + wn * 64 * kMxKTile;
  auto frag = [&](const char* s, int ks) { return mx_frag(s, foff[ks][0], foff[ks][1]); };

  const int nkt = (p.K + kMxKTile - 1) / kMxKTile;
  const bool half_tail = (p.K & (kMxKTile - 1)) != 0;
  const int sh = lhi * 8;
  uint32_t sa_n[MI], sw_n[NI];
  stage(0, 0);
  load_scales(0, sa_n, sw_n);
  for (int t = 0; t < nkt; ++t) {
    uint32_t sa[MI], sw[NI];
#pragma unroll
    for (int im = 0; im < MI; ++im) sa[im] = sa_n[im] >> sh;
#pragma unroll
    for (int in = 0; in < NI; ++in) sw[in] = sw_n[in] >> sh;
    // tile t has landed (this wave's share; the barrier makes it everybody's) and nobody reads the other stage
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    mx_barrier();
    if (t + 1 < nkt) {
      stage(t + 1, (t + 1) & 1);
      load_scales(t + 1, sa_n, sw_n);
    }
    const char* const s = smem + (t & 1) * kMxStage;
    auto mfma_step = [&](auto KS) {
      constexpr int ks = decltype(KS)::value;
      i32x8 wf[NI], af[MI];
#pragma unroll
      for (int in = 0; in < NI; ++in) wf[in] = frag(s + wbase + in * 32 * kMxKTile, ks);
#pragma unroll
      for (int im = 0; im < MI; ++im) af[im] = frag(s + abase + im * 32 * kMxKTile, ks);
#pragma unroll
      for (int im = 0; im < MI; ++im)
#pragma unroll
        for (int in = 0; in < NI; ++in)
          acc[in][im] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[in], af[im], acc[in][im], 0, 0, ks * 2,
                                                                        (int)sw[in], ks * 2, (int)sa[im]);
    };
    mfma_step(std::integral_constant<int, 0>{});
    if (!(half_tail && t == nkt - 1)) mfma_step(std::integral_constant<int, 1>{});
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- epilogue: D[i][j], i = output column (W row) = 8 (e / 4) + 4 (lane / 32) + e % 4, j = output row = lane % 32
  float* const patch = reinterpret_cast<float*>(smem + wid * kMxPatch);
  const int rr = lane >> 3, c8 = (lane & 7) * 8;
  const int col = n0 + wn * 64 + c8;
  float bv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bv[e] = 0.f;
  if (p.bias && col < p.N) load8(p.bias + col, bv);
#pragma unroll
  for (int im = 0; im < MI; ++im) {
#pragma unroll
    for (int in = 0; in < NI; ++in) mx_acc_to_patch(patch, acc[in][im], in, l31, lhi);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int pr = ps * 8 + rr;
      const int row = m0 + wm * 128 + im * 32 + pr;
      float v[8];
      load8(patch + pr * kMxPatchStride + c8, v);
      if (row < p.M && col < p.N) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] += bv[e];
          if (p.act == 1) v[e] = fmaxf(v[e], 0.f);
        }
        const long long o = (long long)row * p.ldc + col;
        if (p.residual) {
          float rv[8];
          unpack8(*reinterpret_cast<const u32x4*>(p.residual + o), rv);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += rv[e];
        }
        if (p.out_f32) {
          float* const dst = reinterpret_cast<float*>(p.out) + o;
          *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
          *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else {
          *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(p.out) + o) = pack8(v);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace os2s

extern "C" int os2s_mx_quantize_rows(os2s_stream_t stream, const uint16_t* x, long long ldx, int rows, int K,
                                     uint8_t* q, uint8_t* scale) {
  using namespace os2s;
  OS2S_REQUIRE(x && q && scale && rows >= 1);
  if (K < 64 || K % 64 != 0) return OS2S_ERR_UNSUPPORTED;
  OS2S_REQUIRE(ldx >= K && ldx % 8 == 0);
  OS2S_REQUIRE(((uintptr_t)x | (uintptr_t)q) % 16 == 0 && (uintptr_t)scale % 4 == 0);
  const long long units = (long long)rows * ceil_div(K, 128);
  if (units >= (1ll << 27)) return OS2S_ERR_UNSUPPORTED;
  OS2S_LAUNCH(mx_quantize_rows_kernel, dim3(ceil_div(units, 16)), dim3(256), 0, (hipStream_t)stream, x, ldx, rows, K,
              q, reinterpret_cast<uint32_t*>(scale));
  return OS2S_OK;
}

extern "C" int os2s_gemm_nt_mx(os2s_stream_t stream, const uint8_t* a, long long lda, const uint8_t* a_scale,
                               const uint8_t* w, const uint8_t* w_scale, void* out, long long ldc, int M, int N,
                               int K, const float* bias, int act, const uint16_t* residual, int out_f32) {
  using namespace os2s;
  OS2S_REQUIRE(a && a_scale && w && w_scale && out);
  if (M < 1 || N < 8 || N % 8 != 0 || K < 64 || K % 64 != 0) return OS2S_ERR_UNSUPPORTED;
  if (act != 0 && act != 1) return OS2S_ERR_UNSUPPORTED;
  OS2S_REQUIRE(lda >= K && lda % 16 == 0 && ldc >= N && ldc % 8 == 0);
  OS2S_REQUIRE(((uintptr_t)a | (uintptr_t)w | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)residual) % 16 == 0);
  OS2S_REQUIRE(((uintptr_t)a_scale | (uintptr_t)w_scale) % 4 == 0);
  // 32-bit byte offsets inside a 256-row tile; scale words indexed below 2^31
  if ((lda + 1) * 256 >= (1ll << 31) || ((long long)K + 1) * 256 >= (1ll << 31)) return OS2S_ERR_UNSUPPORTED;
  MxGemmArgs p;
  p.a = a; p.a_scale = reinterpret_cast<const uint32_t*>(a_scale);
  p.w = w; p.w_scale = reinterpret_cast<const uint32_t*>(w_scale);
  p.out = out; p.bias = bias; p.residual = residual;
  p.lda = lda; p.ldc = ldc; p.M = M; p.N = N; p.K = K; p.act = act; p.out_f32 = out_f32;
  p.NT = ceil_div(N, kMxTile);
  const long long U = (long long)ceil_div(M, kMxTile) * p.NT;
  if (U >= (1ll << 31)) return OS2S_ERR_UNSUPPORTED;
  p.U = (int)U;
  OS2S_LAUNCH_LDS(gemm_nt_mx_kernel, dim3(p.U), dim3(512), kMxLds, (hipStream_t)stream, p);
  return OS2S_OK;
}
