// MXFP8 skinny GEMM for the incremental decoding step, gfx950, hand-written:
//
//   y[M,N] (bf16) = act(deq(mx(x))[M,K] . deq(w_q)[N,K]^T + bias) (+ residual)
//
// The tf.layers.Dense calls under TransformerDecoder._get_symbols_to_logits_fn
// (open_seq2seq/decoders/transformer_decoder.py:232-285) with M = batch * beam rows, behind the 'mxfp8_decode'
// parameter of TransformerDecoder. The bf16 kernels of gemm_skinny.hip are bound by the bytes the L2 delivers to the
// workgroups (tile re-reads), not by FLOPs; here the weights are the cached MXFP8 copies (one byte per element,
// os2s_mx_quantize_rows), one 64-deep v_mfma_scale_f32_32x32x64_f8f6f4 replaces four 16-deep bf16 MFMAs, and the
// LDS that held a chunk of bf16 holds twice the K.
//
// ---- the activation is quantised in the kernel ---------------------------------------------------------------
// x stays bf16 in memory; every workgroup quantises the X rows it stages on their way into LDS, under the format
// rule at the head of gemm_mx.hip and with the very code of mx_quantize_rows_kernel (mx_common.hpp): one 16-byte
// load per lane = 8 elements, 4 lanes a block of 32, amax by DPP over the quad, v_cvt_pk_fp8_f32 after the clamp,
// one 8-byte ds_write into the swizzled slot, and the four scale bytes of a (row, K tile) as one word of a small
// LDS table. No quantiser launch, no e4m3 copy of x in memory. The work is redundant across the N tiles of a row
// block and cheap: at most 64 x 4096 elements over 512 threads in the tiles the decode shapes take.
//
// ---- tile family ---------------------------------------------------------------------------------------------
// MxSkCfg<TN, TM, WN, WM, CT>: a workgroup owns TN x TM sub-tiles of 32 (n) x 32 (m) outputs and stages K in
// chunks of CT K tiles of 128 elements; its 8 waves are (group of WN x WM sub-tiles, K-share): kGroups groups,
// kSplit = 8 / kGroups waves per group, which take the chunk's 64-deep MFMA steps round robin. K-shares are summed
// through LDS in fp32 in wave order (bitwise reproducible), then the epilogue of gemm_skinny_lds_kernel.
//   LDS stage = W [CT][32 TN rows][128 B] + X [CT][32 TM rows][128 B] + X scale words [CT][32 TM], two stages.
//   W: 16-byte buffer-load-to-LDS, one instruction = 8 rows x 128 bytes; 16-byte slots are stored at
//     slot ^ ((row >> 1) & 7) (conflict-free ds_read_b128, as gemm_nt_mx_kernel), the swizzle applied on the global
//     side since the LDS side of a DMA is lane-linear. Rows past N lie outside the descriptor and read as zeros.
//   X: through registers (load of chunk c + 1 issued before the MFMAs of chunk c, quantised and written after them).
//   fragments and scales: the lane mapping measured for gemm_mx.hip — lane l holds row l % 32, its first 16 bytes
//     are elements 16 (l / 32) .. + 15 of the step and its second 16 bytes elements 32 + 16 (l / 32) .. + 15; the
//     scale of block b comes from lanes 32 b .. 32 b + 31. A step is half h of a K tile: every lane shifts the
//     tile's scale word down by 16 h + 8 (l / 32) bits and op_sel stays 0. The W scale words of a sub-tile for one
//     K tile are one coalesced 128-byte load, issued one chunk ahead.
//   loop: one barrier per chunk. K % 128 == 64: the steps past K / 64 are skipped.
#include "mx_common.hpp"

namespace os2s {

struct SkinnyMxArgs {
  const bf16_t* x; long long ldx;                   // [M, K] bf16
  const uint8_t* w; const uint32_t* w_scale;        // e4m3 [N, K], scale words [ceil(K / 128)][N]
  const float* bias;                                // [N] or null
  const bf16_t* res; long long ldr;                 // [M, N] or null
  bf16_t* y; long long ldy;
  int M, N, K, relu;
};

template <int TN, int TM, int WN, int WM, int CT>
struct MxSkCfg {
  static constexpr int kWRows = 32 * TN, kXRows = 32 * TM;
  static constexpr int kWTile = kWRows * 128, kXTile = kXRows * 128;      // bytes of one K tile of an operand
  static constexpr int kW = CT * kWTile, kX = CT * kXTile, kXs = CT * kXRows * 4;
  static constexpr int kStage = kW + kX + kXs;
  static constexpr int kGroups = (TN / WN) * (TM / WM);                   // wave groups = output sub-blocks
  static constexpr int kSplit = 8 / kGroups;                              // waves sharing one sub-block
  static constexpr int kSteps = 2 * CT;                                   // MFMA steps of a chunk
  static constexpr int kSpw = kSteps / kSplit;                            // ... per wave
  static constexpr int kDma = CT * 4 * TN / 8;                            // W DMA instructions per wave per chunk
  static constexpr int kPieces = TM * CT;                                 // 16-byte X loads per thread per chunk
  static constexpr int kRed = (kSplit - 1) * kGroups * 4096;
  static constexpr int kSmem = 2 * kStage > kRed ? 2 * kStage : kRed;
  static_assert(kGroups * kSplit == 8 && kSpw * kSplit == kSteps && kDma * 8 == CT * 4 * TN, "8 waves");
  static_assert(kSplit == 1 || (WN == 1 && WM == 1), "K-split variants hold one sub-tile per wave");
};

// One W DMA instruction (64 lanes x 16 bytes, LDS side lane-linear from `dst`) and one scaled MFMA step with the
// scale bytes in byte 0 of sw / sx. Plain functions on purpose: inside a template the host pass drops these builtins
// without a diagnostic and emits no kernel stub (an undefined symbol at load time).
__device__ __forceinline__ void mx_dma16(__amdgpu_buffer_rsrc_t rs, char* dst, int voffset) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, voffset, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mx_mfma64(const i32x8& wf, const i32x8& xf, const f32x16& acc, uint32_t sw,
                                            uint32_t sx) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf, xf, acc, 0, 0, 0, (int)sw, 0, (int)sx);
}

template <int TN, int TM, int WN, int WM, int CT>
__global__ __launch_bounds__(512) void gemm_skinny_mx_kernel(SkinnyMxArgs p) {
  using C = MxSkCfg<TN, TM, WN, WM, CT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * C::kWRows, m0 = blockIdx.y * C::kXRows;
  const int sub = wave % C::kGroups, ks = C::kSplit == 1 ? 0 : wave / C::kGroups;
  const int tn = (sub % (TN / WN)) * WN, tm = (sub / (TN / WN)) * WM;     // first sub-tile of this wave
  const int nsteps = p.K >> 6, nchunks = (nsteps + C::kSteps - 1) / C::kSteps;

  // ---- W: this wave's DMA instructions; instruction i covers rows 8 (i % 4 TN) .. + 7 of K tile i / (4 TN)
  const __amdgpu_buffer_rsrc_t wrs = mx_rsrc(p.w + (long long)n0 * p.K, (long long)(p.N - n0) * p.K);
  int wv[C::kDma];
#pragma unroll
  for (int pi = 0; pi < C::kDma; ++pi) {
    const int i = pi * 8 + wave, kt = i / (4 * TN);
    const int row = (i % (4 * TN)) * 8 + (lane >> 3), slot = (lane & 7) ^ ((row >> 1) & 7);
    wv[pi] = row * p.K + kt * 128 + slot * 16;
  }
  auto stage_w = [&](int c, int buf) {
#pragma unroll
    for (int pi = 0; pi < C::kDma; ++pi) {
      const int i = pi * 8 + wave, kt = i / (4 * TN);
      if ((c * CT + kt) * 128 < p.K)
        mx_dma16(wrs, smem + buf * C::kStage + kt * C::kWTile + (i % (4 * TN)) * 1024, wv[pi] + c * CT * 128);
    }
  };
  // ---- X: piece j of a thread = 8 elements of (row, K tile); 16 consecutive lanes own one (row, K tile) unit
  const int col16 = tid & 15;
  const bf16_t* xsrc[C::kPieces];
  int xk[C::kPieces], xdst[C::kPieces], xsdst[C::kPieces];
  bool xok[C::kPieces];
#pragma unroll
  for (int j = 0; j < C::kPieces; ++j) {
    const int rk = (j * 512 + tid) >> 4, kt = rk % CT, row = rk / CT;
    xok[j] = m0 + row < p.M;
    xsrc[j] = p.x + (long long)min(m0 + row, p.M - 1) * p.ldx;
    xk[j] = kt * 128 + col16 * 8;
    xdst[j] = C::kW + kt * C::kXTile + row * 128 + (((col16 >> 1) ^ ((row >> 1) & 7)) << 4) + (col16 & 1) * 8;
    xsdst[j] = C::kW + C::kX + (kt * C::kXRows + row) * 4;
  }
  u32x4 st[C::kPieces];
  auto load_x = [&](int c) {
#pragma unroll
    for (int j = 0; j < C::kPieces; ++j) {
      const int k = c * CT * 128 + xk[j];
      const u32x4 v = *reinterpret_cast<const u32x4*>(xsrc[j] + min(k, p.K - 8));
      const u32x4 z = {0u, 0u, 0u, 0u};
      st[j] = (xok[j] && k < p.K) ? v : z;
    }
  };
  auto store_x = [&](int buf) {
    char* const s = smem + buf * C::kStage;
#pragma unroll
    for (int j = 0; j < C::kPieces; ++j) {
      int byte;
      const u32x2 o = mx_quantize8(st[j], byte);
      *reinterpret_cast<u32x2*>(s + xdst[j]) = o;
      const uint32_t word = mx_scale_word(byte, lane);
      if (col16 == 0) *reinterpret_cast<uint32_t*>(s + xsdst[j]) = word;
    }
  };
  // ---- W scale words of this wave's steps of one chunk (a step past K loads nothing and is never used)
  const int wrow0 = n0 + tn * 32 + l31;
  auto load_wscales = [&](int c, uint32_t (&sw)[C::kSpw][WN]) {
#pragma unroll
    for (int i = 0; i < C::kSpw; ++i) {
      const int gs = c * C::kSteps + ks + i * C::kSplit;
#pragma unroll
      for (int in = 0; in < WN; ++in) {
        const int r = min(wrow0 + in * 32, p.N - 1);      // a row past N is all zeros: any scale will do
        sw[i][in] = gs < nsteps ? p.w_scale[(long long)(gs >> 1) * p.N + r] : 0u;
      }
    }
  };

  f32x16 acc[WN][WM];
#pragma unroll
  for (int i = 0; i < WN; ++i)
#pragma unroll
    for (int j = 0; j < WM; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // fragment offsets inside a 32-row sub-tile of one K tile: half h of the tile, the lane's piece q of scale block q
  int foff[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int q = 0; q < 2; ++q) foff[h][q] = l31 * 128 + (((h * 4 + q * 2 + lhi) ^ ((l31 >> 1) & 7)) << 4);
  auto frag = [&](const char* s, int h) {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(s + (h ? foff[1][0] : foff[0][0]));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(s + (h ? foff[1][1] : foff[0][1]));
    i32x8 f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[e] = (int)lo[e]; f[4 + e] = (int)hi[e]; }
    return f;
  };

  uint32_t sw_n[C::kSpw][WN];
  stage_w(0, 0);
  load_x(0);
  load_wscales(0, sw_n);
  store_x(0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  mx_barrier();
  for (int c = 0; c < nchunks; ++c) {
    uint32_t sw[C::kSpw][WN];
#pragma unroll
    for (int i = 0; i < C::kSpw; ++i)
#pragma unroll
      for (int in = 0; in < WN; ++in) sw[i][in] = sw_n[i][in];
    if (c + 1 < nchunks) {      // nobody reads the other stage: everyone passed the barrier that ended chunk c - 1
      stage_w(c + 1, (c + 1) & 1);
      load_x(c + 1);
      load_wscales(c + 1, sw_n);
    }
    const char* const s = smem + (c & 1) * C::kStage;
#pragma unroll
    for (int i = 0; i < C::kSpw; ++i) {
      const int sidx = ks + i * C::kSplit;                 // step of the chunk: half h of its K tile kt
      if (c * C::kSteps + sidx < nsteps) {
        const int kt = sidx >> 1, h = sidx & 1, sh = h * 16 + lhi * 8;
        i32x8 wf[WN], xf[WM];
        uint32_t sx[WM];
#pragma unroll
        for (int in = 0; in < WN; ++in) wf[in] = frag(s + kt * C::kWTile + (tn + in) * 4096, h);
#pragma unroll
        for (int im = 0; im < WM; ++im) {
          xf[im] = frag(s + C::kW + kt * C::kXTile + (tm + im) * 4096, h);
          sx[im] = *reinterpret_cast<const uint32_t*>(s + C::kW + C::kX + (kt * C::kXRows + (tm + im) * 32 + l31) * 4) >> sh;
        }
#pragma unroll
        for (int im = 0; im < WM; ++im)
#pragma unroll
          for (int in = 0; in < WN; ++in)
            acc[in][im] = mx_mfma64(wf[in], xf[im], acc[in][im], sw[i][in] >> sh, sx[im]);
      }
    }
    if (c + 1 < nchunks) store_x((c + 1) & 1);
    // chunk c + 1 has landed (this wave's share; the barrier makes it everybody's) and chunk c has been read
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    mx_barrier();
  }
  // ---- combine the K-shares in wave order, epilogue (D[i][j]: i = output column, j = output row = lane % 32) ----
  if constexpr (C::kSplit > 1) {
    float* red = reinterpret_cast<float*>(smem);      // [kSplit-1][groups][16][64]
    if (ks > 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(((ks - 1) * C::kGroups + sub) * 16 + r) * 64 + lane] = acc[0][0][r];
    }
    __syncthreads();
    if (ks > 0) return;
#pragma unroll
    for (int q = 0; q < C::kSplit - 1; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][0][r] += red[((q * C::kGroups + sub) * 16 + r) * 64 + lane];
  }
#pragma unroll
  for (int j = 0; j < WM; ++j) {
    const int m = m0 + (tm + j) * 32 + l31;
    if (m >= p.M) continue;
#pragma unroll
    for (int i = 0; i < WN; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + (tn + i) * 32 + 8 * g + 4 * lhi;
        if (n >= p.N) continue;
        float out[4] = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
        if (p.bias) {
          const f32x4 bb = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) out[e] += bb[e];
        }
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) out[e] = fmaxf(out[e], 0.f);
        }
        if (p.res) {
          const u32x2 r = *reinterpret_cast<const u32x2*>(p.res + (long long)m * p.ldr + n);
          out[0] += bflo(r[0]); out[1] += bfhi(r[0]); out[2] += bflo(r[1]); out[3] += bfhi(r[1]);
        }
        u32x2 o;
        o[0] = pack2bf(out[0], out[1]);
        o[1] = pack2bf(out[2], out[3]);
        *reinterpret_cast<u32x2*>(p.y + (long long)m * p.ldy + n) = o;
      }
  }
}


}  // namespace os2s

using namespace os2s;

#define OS2S_SKINNY_MX_CASE(V, TN, TM, WN, WM, CT)                                                             \
  case V:                                                                                                    \
    OS2S_LAUNCH_LDS((gemm_skinny_mx_kernel<TN, TM, WN, WM, CT>), dim3(ceil_div(N, 32 * TN), ceil_div(M, 32 * TM)), \
                    dim3(512), (MxSkCfg<TN, TM, WN, WM, CT>::kSmem), s, a);                                  \
    return OS2S_OK

extern "C" int os2s_gemm_skinny_mx(os2s_stream_t stream, const uint16_t* x, long long ldx, const uint8_t* w_q,
                                   const uint8_t* w_scale, const float* bias, const uint16_t* residual,
                                   long long ldr, int M, int N, int K, int relu, uint16_t* y, long long ldy,
                                   int tile) {
  OS2S_REQUIRE(x && w_q && w_scale && y);
  if (M < 1 || N < 8 || N % 8 != 0 || K < 64 || K % 64 != 0) return OS2S_ERR_UNSUPPORTED;
  if ((relu != 0 && relu != 1) || tile < -1 || tile > 4) return OS2S_ERR_UNSUPPORTED;
  OS2S_REQUIRE(ldx >= K && ldx % 8 == 0 && ldy >= N && ldy % 4 == 0 && (!residual || (ldr >= N && ldr % 4 == 0)));
  OS2S_REQUIRE(((uintptr_t)x | (uintptr_t)w_q | (uintptr_t)bias) % 16 == 0 && (uintptr_t)w_scale % 4 == 0);
  OS2S_REQUIRE(((uintptr_t)y | (uintptr_t)residual) % 8 == 0);
  // 32-bit byte offsets inside a 256-row W tile; grid.y
  if (((long long)K + 1) * 256 >= (1ll << 31) || M > 65535 * 32) return OS2S_ERR_UNSUPPORTED;
  SkinnyMxArgs a;
  a.x = x; a.ldx = ldx; a.w = w_q; a.w_scale = reinterpret_cast<const uint32_t*>(w_scale); a.bias = bias;
  a.res = residual; a.ldr = ldr; a.y = y; a.ldy = ldy; a.M = M; a.N = N; a.K = K; a.relu = relu;
  // by shape: the widest tile that still makes 192 workgroups (delivered bytes = X bytes * N / tile n + W bytes *
  // M / tile m) — the fastest MX tile at each measured decode shape (profiles/mxfp8_decode_first_measurements.md:
  // workgroup count beats traffic); tile >= 0 (tests, tools) names one: (m x n) 0 = 32x32, 1 = 64x64, 2 = 64x128, 3 = 128x256,
  // 4 = 256x256. Deliberately an argument and not a process-wide option: a forced tile cannot outlive its call.
  auto wgs = [&](int tm, int tn) { return (long long)ceil_div(M, tm) * ceil_div(N, tn); };
  int variant = 0;
  if (wgs(64, 64) >= 192) variant = 1;
  if (wgs(64, 128) >= 192) variant = 2;
  if (M > 64 && wgs(128, 256) >= 192) variant = 3;
  if (M > 128 && wgs(256, 256) >= 192) variant = 4;
  if (tile >= 0) variant = tile;
  const hipStream_t s = (hipStream_t)stream;
  switch (variant) {
    OS2S_SKINNY_MX_CASE(0, 1, 1, 1, 1, 4);
    OS2S_SKINNY_MX_CASE(1, 2, 2, 1, 1, 2);
    OS2S_SKINNY_MX_CASE(2, 4, 2, 1, 1, 2);
    OS2S_SKINNY_MX_CASE(3, 8, 4, 2, 2, 1);
    OS2S_SKINNY_MX_CASE(4, 8, 8, 2, 4, 1);
  }
  return OS2S_ERR_UNSUPPORTED;
}
