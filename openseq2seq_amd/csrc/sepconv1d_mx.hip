// MXFP8 inference separable conv1d (stride 1, dilation 1) in ONE launch, gfx950, hand-written:
//
//   z[b, t, ci] = bf16(sum_k x[b, t + k - padL, ci] * d[k, ci])        rows outside [0, in_len[b]) read as 0; fp32 sum
//   zq, zs      = the format rule of os2s_mx_quantize_rows (head of gemm_mx.hip) applied to z along ci
//   y[b, t, co] = act(ch_scale[co] * sum_ci deq(zq, zs)[b, t, ci] * deq(wq, ws)[co, ci] + ch_shift[co])
//   y[b, t, :]  = 0 for t >= out_len[b]
//
// tf.layers.separable_conv1d(use_bias=False) + tf.layers.batch_normalization(training=False) + activation_fn of the
// "sep_conv1d" layers (open_seq2seq/parts/cnns/conv_blocks.py:11-16, the QuartzNet configs) in eval / infer mode.
// Depthwise FIR, MX quantiser, block-scaled pointwise GEMM and the BatchNorm / ReLU / mask epilogue: the depthwise
// output never reaches memory, there is no quantiser launch and no BatchNorm pass. z is rounded to bf16 before the
// quantiser on purpose: mx_quantize8 is used as it is and the result equals the unfused chain (depthwise ->
// os2s_mx_quantize_rows -> os2s_conv1d_fwd_mx with K = 1) up to the fp32 summation order of the two stages.
//
// ---- operands ------------------------------------------------------------------------------------------------
// x [B, Tin, Cin] bf16, NOT quantised (the depthwise half runs on bf16 data as os2s_depthwise_conv1d_fwd does);
// d [K, Cin] fp32 (the depthwise master); wq [Cout, Cin] e4m3 / w_scale [ceil(Cin/128)][Cout] words:
// os2s_mx_quantize_rows of the pointwise kernel.
//
// ---- split: the pointwise A operand is stationary in LDS -----------------------------------------------------
// A workgroup (512 threads, 8 waves, 1 per CU) owns 128 output rows of ONE sample and ALL of Cout, so the depthwise
// half is computed once per output row (a 256 x 256 tiling would redo it per column tile). Grid = B x ceil(Tout/128);
// workgroup i runs on XCD i & 7, so the consecutive row tiles of a sample go round the 8 XCDs (as
// conv1d_mx_kernel). A tile that starts at or past out_len[b] only stores zeros.
//
// Phase 1 builds zq [ceil(Cin/128)][128 rows][128 B] (<= 64 KB) and the A-side scale bytes [ceil(Cin/128)][128][4]
// (<= 2 KB) in LDS, per group of 64 channels:
//   slab: input rows t0 - padL .. t0 + 127 + (K-1) - padL x 64 channels (128 B a row), buffer-load-to-LDS, 8 rows
//     per instruction, <= 28 instructions over the 8 waves, double-buffered across groups. The descriptor starts at
//     the sample and ends at row in_len[b]: rows past the length read as 0; a row of the left padding is sent to
//     offset 2^31, behind the end of every descriptor (conv1d_mx.hip, "zeros from the descriptor").
//   taps: d[:, group] as fp32 [K][64] in LDS, loaded to registers one group ahead.
//   FIR: thread = (channel pair, run of 8 consecutive rows): a register window of 8 rows, per tap ONE new row
//     (ds_read_b32: two bf16) and one tap pair (ds_read_b64) for 16 fp32 FMAs, taps in ascending order. The unit is
//     built without packed fp32 arithmetic, as the other MX units: the FMAs are v_fma_f32.
//   transpose: a wave owns 16 rows x 64 channels. After a barrier (everybody is through with the slab) it writes its
//     z as bf16 into its own 2 KB of the slab just read and reads it back as "8 consecutive channels per lane, 4
//     lanes per 32-block", the arrangement mx_quantize8 expects.
//   store: the 8 e4m3 bytes at the swizzled slot of the zq tile (16-byte slot q of row r at q ^ ((r >> 1) & 7), the
//     key of gemm_mx.hip), so phase 2 reads its A fragments with mx_frag unchanged; the scale byte into the table.
// Phase 2 loops over Cout in chunks of 256 columns: W tiles of 256 columns x 128 bytes by DMA, double-buffered over
//   the flattened (chunk, channel tile) loop as in gemm_nt_mx_kernel; waves as 2 x 4, wave tile 64 x 64 = 2 x 2
//   accumulator blocks of v_mfma_scale_f32_32x32x64_f8f6f4 (64 fp32 a lane); one MFMA step in the last channel tile
//   when Cin % 128 == 64. One barrier a step.
//   epilogue (after the last channel tile of a chunk): accumulator block -> the wave's 32 x 32 fp32 patch (4 KB,
//     16-byte chunks swizzled with the same row key) -> 8 columns per lane: ch_scale / ch_shift, ReLU, length mask,
//     one 16-byte store of bf16 (two of fp32). The 8 patches lie in the W stage that was read LAST; the next chunk's
//     first W tile is already on its way into the other stage. Columns at or past Cout (zeros from W's descriptor)
//     and rows at or past Tout are not stored.
//   LDS: zq 16 KB per channel tile + scale bytes 512 B per channel tile + one region shared by phase 1 (2 slabs of
//     ceil((127 + K) / 8) KB + K x 256 B of taps) and phase 2 (2 x 32 KB of W / the patches): never live together.
//     Cin 512: 130 KB up to K = 64, 137 KB at K = 75, 146 KB at K = 96; sized per launch.
//
//
// ---- resources and what bounds it ------------------------------------------------------------------------------
// hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage: 145 VGPRs, 0 AGPRs, 106 SGPRs, scratch 0, no VGPR spill;
// LDS 80.5 KB (Cin 64) .. 146 KB (Cin 512, K 96), dynamic, through OS2S_LAUNCH_LDS.
// Measured on an MI355X (profiles/mxfp8_sepconv_first_measurements.md, B = 32, T = 808 ragged): the launch takes
// 25.6 / 26.8 / 35.3 us at (Cin, Cout, K) = (256, 256, 33) / (256, 256, 39) / (256, 512, 51) and 60.7 / 68.7 / 77.3 us
// at (512, 512, 51 / 63 / 75); the same launch with a one-tap depthwise kernel takes 15.4 / 15.4 / 20.3 and 30 us.
// The difference is what phase 1 spends on K taps instead of one — the tap loop's FMAs and LDS reads, the K - 1 more
// slab rows staged per group and the tap table: 40 - 43 % of the launch at Cin 256, 50 - 61 % at Cin 512 (0.6 us a
// tap). That is an upper bound on the FIR's arithmetic, not a measurement of it. PHASE 1 BOUNDS THE KERNEL at the
// Cin 512 shapes (it is the larger part and the only part that grows with K), and the fused launch loses there to the
// bf16 chain, whose depthwise half runs on the matrix pipe. These are timings of v_fma_f32: the unit is built without
// packed fp32 arithmetic (build.py says why), which doubles the FIR's FMA instructions against v_pk_fma_f32. A packed
// build was not timed; if the whole difference were FMA issue it would save at most half of it (15 - 24 us at Cin
// 512): in that best case the Cin 512 chains would come to 0.83 - 0.90 x the bf16 chain instead of 1.09 - 1.30 x.
// So the rule that keeps Cin 512 on bf16 is a statement about this build.
// What remains at K = 1 is far above phase 2's matrix work: with one workgroup per CU the DMA waits of both phases
// are exposed; which phase holds most of that is not established.
// Follow-up: the Toeplitz-band depthwise on v_mfma_f32_16x16x32_bf16 (depthwise_mfma_fwd_kernel's hi + lo tap pair)
// inside phase 1, which needs no packed fp32 arithmetic. That is variant 1, below.
//
// ---- variant 1 (os2s_sepconv1d_fwd_mx_variant): phase 1 on the matrix pipe --------------------------------------
// Same workgroup, same zq / zs, same phase 2; what is above is variant 0. For one (sample, channel) the depthwise
// sum is a Toeplitz-band product (header of depthwise_mfma_fwd_kernel), here on v_mfma_f32_16x16x32_bf16:
//     z[16 s + i] = sum_p T[i][p] X[p][s],   T[i][p] = d[p - i],   X[p][s] = x[t0 - padL + 16 s + p]
// M = position i in a 16-step segment, N = segment s (a 128-row tile is 8 segments: columns 8 .. 15 repeat 0 .. 7, the
// same addresses, and serve the store below), K = window position p in J = ceil((16 + K - 1) / 32) steps of 32. The
// fp32 taps enter as a bf16 hi + lo pair, two MFMAs a step: the fp32-tap sum of the FIR up to fp32 rounding. J is a
// template parameter (1 .. 4): with a run-time J every step is a basic block that waits for its own reads.
// Split: groups of 64 channels, wave w owns the 8 consecutive channels 8 w .. 8 w + 7 of the group — one 16-byte slot
//   of a row — and all 128 rows: 8 J x 2 MFMAs a group, 32 fp32 accumulators a lane.
// In: thread = (4 window positions, 8 channels): four 16-byte row loads (rows outside [0, in_len) and positions past
//   128 + K - 1 masked to zero; a dead row's address is clamped, there is no branch), one group ahead in registers,
//   transposed to eight 8-byte writes, one per channel PLANE (time-contiguous, 112 + 32 J positions). The LDS DMA
//   cannot transpose. Taps: lane = (tap mod 8, channel) reads 32-byte runs of d, one group ahead, and writes hi / lo
//   into the wave's own zero-padded tables [8 channels][hi, lo][32 J + 24], tap k at element 16 + k.
// Fragments: B = one aligned ds_read_b128 of the plane at position 16 s + 32 j + 8 (lane / 16). A = 8 taps from
//   element 16 + 32 j + 8 (lane / 16) - i, 2-byte aligned: five aligned words and v_alignbit by 0 or 16 bits (a
//   lane-private unaligned ds_read_b128 costs ~100 cycles, see depthwise_mfma_fwd_kernel). The reads of channel i + 1
//   are issued before the MFMAs of channel i (two register sets, sched_barrier).
// Out: acc[i][e] is channel 8 w + i at row 16 s + 4 (lane / 16) + e: a lane packs its 8 channels of a row to bf16 in
//   registers, one ds_write_b128 into the row-major bounce tile [128 rows][128 B] (columns 0 .. 7 rows e = 0, 1,
//   columns 8 .. 15 e = 2, 3); after a barrier "8 consecutive channels per lane, 4 lanes per 32-block" is a
//   ds_read_b128, then mx_quantize8 and the zq / zs stores of variant 0. Two barriers a group.
// LDS: zq + zs as above (66 KB at Cin 512) + one region shared with phase 2: planes 64 x 288 B (J = 1) or 64 x 544 B
//   + bounce 16 KB + tables 64 x 2 x (32 J + 24) x 2 B: 48 KB (J = 1) .. 88 KB (J = 4); 154 KB at Cin 512, K 96.
// Bank conflicts: plane writes — 32 lanes = 4 positions-of-4 (8 B apart) x 8 planes whose stride is 32 B mod 256 B:
//   256 distinct bytes, that is why a plane is 288 or 544 B long; plane reads — a wave reads ONE plane, 16 lanes of a
//   16-byte quarter read chunks 2 s + const, columns 8 .. 15 the addresses of 0 .. 7 (broadcast): no conflict; tap
//   reads — ONE table, the wave's words span 20 consecutive ones, equal addresses broadcast: none; bounce — slot w of
//   row r lies at w ^ (r >> 4): the 8 lanes of a 128-byte write beat have 8 different s, so 8 different slots; the read
//   back takes whole rows.
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), J = 1 / 2 / 3 / 4: 144 / 164 / 198 / 241
//   VGPRs, 0 AGPRs, 74 / 76 / 83 / 91 SGPRs, scratch 0, no VGPR spill (variant 0 is unchanged: 145 VGPRs).
// Measured (profiles/mxfp8_sepconv_mfma_first_measurements.md, same batch): the chain with this launch takes 22.1 /
//   22.0 / 31.1 us at (256, 256, 33) / (256, 256, 39) / (256, 512, 51) and 49.6 / 49.8 / 49.7 us at (512, 512, 51 / 63 /
//   75): 0.65 - 0.84 x variant 0, 0.87 - 0.90 x the bf16 chain at Cin 512. K moves it only through J; with one tap it
//   takes 18.2 / 23.2 / 34.3 us, 1 - 2 us more than variant 0 with one tap. So a window step more (its MFMAs,
//   fragment reads, 32 more plane positions and table elements) costs about 4 us at Cin 256 and 7.6 us at Cin 512 —
//   J = 2 at K 33 / 39, J = 3 at K 51 .. 75 — and the larger part of the launch now is what is left at K = 1 (staging, quantiser, phase
//   2), as §"resources" above says of variant 0; which part of that is largest is not established.
#include <type_traits>

#include "mx_common.hpp"

namespace os2s {

struct MxSepArgs {
  const bf16_t* x; const float* d; const uint8_t* w; const uint32_t* w_scale;
  void* y; const int32_t* in_len; const int32_t* out_len; const float* ch_scale; const float* ch_shift;
  long long y_stride_b, y_stride_t;
  int B, Tin, Cin, Cout, K, padL, Tout, act, out_f32, MT;
  int slab;      // bytes of one staging slab: ceil((127 + K) / 8) KB
};

constexpr int kSepRows = 128;                         // output rows of a workgroup
constexpr int kSepZTile = kSepRows * kMxKTile;        // bytes of zq per channel tile of 128
constexpr int kSepMaxK = 96, kSepMaxCin = 512;
constexpr int kSepTapRegs = kSepMaxK * 64 / 512;      // taps of one group per thread
constexpr int kSepBehind = (int)0x80000000u;          // an offset behind the end of every descriptor

__host__ __device__ constexpr int sep_slab_bytes(int K) { return (kSepRows + K - 1 + 7) / 8 * 1024; }

// eight outputs of one row: bf16 as one 16-byte store, fp32 as two
__device__ __forceinline__ void sep_store8(const MxSepArgs& p, int b, int t, int col, const float (&v)[8]) {
  const long long o = (long long)b * p.y_stride_b + (long long)t * p.y_stride_t + col;
  if (p.out_f32) {
    float* const dst = reinterpret_cast<float*>(p.y) + o;
    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
  } else {
    *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(p.y) + o) = pack8(v);
  }
}

__device__ __forceinline__ void sep_row(const char* ptr, float (&dst)[2]) {
  const uint32_t v = *reinterpret_cast<const uint32_t*>(ptr);
  dst[0] = bflo(v);
  dst[1] = bfhi(v);
}

// ---- variant 1: phase 1 as a Toeplitz-band product (geometry: the head of this file) ----
constexpr int kSmCh = 64;                             // channels of a group: 8 consecutive ones per wave
constexpr int kSmOff = 16;                            // table element of tap 0
constexpr int kSmBounce = kSepRows * kSmCh * 2;       // z of one group, bf16, row-major
__host__ __device__ constexpr int sm_steps(int K) { return (16 + K - 1 + 31) / 32; }        // window steps of 32
__host__ __device__ constexpr int sm_rows(int K) { return 112 + 32 * sm_steps(K); }         // time steps of a plane
__host__ __device__ constexpr int sm_plane_bytes(int K) { return sm_steps(K) == 1 ? 288 : 544; }   // % 256 == 32
__host__ __device__ constexpr int sm_table(int K) { return 32 * sm_steps(K) + 24; }         // elements of a tap table
__host__ __device__ constexpr int sm_phase1_bytes(int K) {
  return kSmCh * sm_plane_bytes(K) + kSmBounce + kSmCh * 2 * sm_table(K) * 2;
}

template <int J>   // J = sm_steps(K): a constant, so that the fragment reads of a group's 8 J steps can be issued ahead of its MFMAs
__device__ __forceinline__ void sep_phase1_mfma(const MxSepArgs& p, int b, int t0, int lin, char* zq, char* zs,
                                                char* sh) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int pb = J == 1 ? 288 : 544, wt = 32 * J + 24;           // sm_plane_bytes, sm_table
  const int ng = p.Cin >> 6;
  char* const planes = sh;                             // [64 planes][pb]: channel 8 w + i of the group is plane 8 i + w
  char* const bounce = sh + kSmCh * pb;                // [128 rows][8 slots of 16 B], slot w of row r at w ^ (r >> 4)
  bf16_t* const tabs = reinterpret_cast<bf16_t*>(bounce + kSmBounce) + wid * 16 * wt;   // this wave's [8][hi, lo][wt]

  // staging item: plane positions 4 p4 .. 4 p4 + 3 (input rows t0 - padL + ...) x the 8 channels of wave cg. Rows
  // outside [0, in_len) and positions past the tile's window (they meet zero taps only) are zeros, not loads
  // (a dead row loads row 0 or Tin - 1 and is masked where it is used, a group later: no branch around the loads
  // and nothing that waits for them before the MFMAs of the group in between)
  const int cg = tid & 7, p4 = tid >> 3, live = kSepRows + p.K - 1;
  const bf16_t* xb[4];
  uint32_t xm[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int r = p4 * 4 + u, tin = t0 - p.padL + r;
    xb[u] = p.x + ((long long)b * p.Tin + min(max(tin, 0), p.Tin - 1)) * p.Cin + cg * 8;
    xm[u] = (r < live && tin >= 0 && tin < lin) ? 0xffffffffu : 0u;
  }
  u32x4 xr[4];
  auto load_rows = [&](int g) {
#pragma unroll
    for (int u = 0; u < 4; ++u) xr[u] = *reinterpret_cast<const u32x4*>(xb[u] + g * kSmCh);
  };
  // taps of the wave's 8 channels: lane = (tap k mod 8, channel), 32-byte runs of d
  constexpr int kTapRegs = 4 * J - 1;                 // K <= 32 J - 15: taps k < 32 J - 8, zeros from K on
  const int tk = lane >> 3, ti = lane & 7;
  float tp[kTapRegs];
  auto load_taps = [&](int g) {
#pragma unroll
    for (int r = 0; r < kTapRegs; ++r) {
      const int k = r * 8 + tk;
      tp[r] = p.d[(long long)min(k, p.K - 1) * p.Cin + g * kSmCh + wid * 8 + ti];       // masked at the table
    }
  };
  // the tables are zero outside [kSmOff, kSmOff + K), and K is the same for every group
  for (int i = lane; i < 2 * wt; i += 64) reinterpret_cast<u32x4*>(tabs)[i] = u32x4{0u, 0u, 0u, 0u};
  asm volatile("" ::: "memory");
  load_rows(0);
  load_taps(0);

  const int n = lane & 15, kg = lane >> 4, seg = n & 7, up = n >> 3;   // columns 8 .. 15 repeat segments 0 .. 7
  const int e0 = kSmOff + 8 * kg - n;                  // table element of A[i = n][p = 8 kg] of step 0: 1 .. 40
  const uint32_t shb = (e0 & 1) ? 16u : 0u;
  for (int g = 0; g < ng; ++g) {
    // nobody reads the planes of group g - 1 any more (barrier B below); the tables are the wave's own
    if (p4 * 4 < 112 + 32 * J) {                        // sm_rows
      char* const dst = planes + cg * pb + p4 * 8;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // channel 2k (low halves) and 2k + 1 (high halves) of the wave's eight
        u32x2 lo, hi;
        const uint32_t x0 = xr[0][k] & xm[0], x1 = xr[1][k] & xm[1], x2 = xr[2][k] & xm[2], x3 = xr[3][k] & xm[3];
        lo[0] = (x0 & 0xffffu) | (x1 << 16);
        lo[1] = (x2 & 0xffffu) | (x3 << 16);
        hi[0] = (x0 >> 16) | (x1 & 0xffff0000u);
        hi[1] = (x2 >> 16) | (x3 & 0xffff0000u);
        *reinterpret_cast<u32x2*>(dst + (2 * k) * 8 * pb) = lo;
        *reinterpret_cast<u32x2*>(dst + (2 * k + 1) * 8 * pb) = hi;
      }
    }
#pragma unroll
    for (int r = 0; r < kTapRegs; ++r) {
      const int k = r * 8 + tk;
      const float w = k < p.K ? tp[r] : 0.f;
      const bf16_t h = f2bf(w);
      tabs[(2 * ti) * wt + kSmOff + k] = h;
      tabs[(2 * ti + 1) * wt + kSmOff + k] = f2bf(w - bf2f(h));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    mx_barrier();                                      // A: the planes of group g are everybody's
    if (g + 1 < ng) {
      load_rows(g + 1);
      load_taps(g + 1);
    }
    // D[i][n] = sum_p T[i][p] X[p][n]: T[i][p] = tap p - i, X[p][n] = plane position 16 seg + p
    // The fragments of channel i + 1 are read while channel i multiplies (two register sets, the scheduler held to
    // that order): left to itself the compiler waits for each step's reads right in front of its two MFMAs.
    // B fragment: one aligned 16-byte read of the plane. A fragment: it starts at a 2-byte-aligned element, so five
    // aligned words and a funnel shift by 0 or 16 bits (depthwise_mfma_fwd_kernel says why it is no unaligned read)
    f32x4 acc[8];
    bf16x8 fb[2][J];
    uint32_t fh[2][J][5], fl[2][J][5];
    auto read_frags = [&](int i, int s) {
      const char* const pl = planes + (i * 8 + wid) * pb + (2 * seg + kg) * 16;
      const uint32_t* const th = reinterpret_cast<const uint32_t*>(tabs + (2 * i) * wt) + (e0 >> 1);
      const uint32_t* const tl = th + (wt >> 1);
#pragma unroll
      for (int j = 0; j < J; ++j) {
        fb[s][j] = *reinterpret_cast<const bf16x8*>(pl + j * 64);
#pragma unroll
        for (int k = 0; k < 5; ++k) { fh[s][j][k] = th[16 * j + k]; fl[s][j][k] = tl[16 * j + k]; }
      }
    };
    read_frags(0, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i + 1 < 8) read_frags(i + 1, (i + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
      acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < J; ++j) {
        u32x4 ah, al;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          ah[k] = __builtin_amdgcn_alignbit(fh[i & 1][j][k + 1], fh[i & 1][j][k], shb);
          al[k] = __builtin_amdgcn_alignbit(fl[i & 1][j][k + 1], fl[i & 1][j][k], shb);
        }
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah), fb[i & 1][j], acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, al), fb[i & 1][j], acc[i], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // acc[i][e]: channel 8 w + i at row 16 seg + 4 kg + e. Eight channels of a row are one 16-byte slot; the lanes of
    // the repeated columns store e = 2, 3, the others e = 0, 1
#pragma unroll
    for (int ee = 0; ee < 2; ++ee) {
      u32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        o[k] = pack2bf(up ? acc[2 * k][2 + ee] : acc[2 * k][ee], up ? acc[2 * k + 1][2 + ee] : acc[2 * k + 1][ee]);
      const int row = 16 * seg + 4 * kg + 2 * up + ee;
      *reinterpret_cast<u32x4*>(bounce + row * 128 + ((wid ^ seg) << 4)) = o;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    mx_barrier();                                      // B: everybody is through with the planes; z of the group is there
    const int q = tid & 7, ct = g >> 1;                // 8 channels 8 q .. of the group; quad = one block of 32
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = h * 64 + (tid >> 3);
      const u32x4 v = *reinterpret_cast<const u32x4*>(bounce + row * 128 + ((q ^ (row >> 4)) << 4));
      int byte;
      const u32x2 o = mx_quantize8(v, byte);
      const int slot = (g & 1) * 4 + (q >> 1);
      *reinterpret_cast<u32x2*>(zq + ct * kSepZTile + row * kMxKTile + ((slot ^ ((row >> 1) & 7)) << 4) +
                                (q & 1) * 8) = o;
      if ((q & 3) == 0) zs[(ct * kSepRows + row) * 4 + (g & 1) * 2 + (q >> 2)] = (char)byte;
    }
  }
}

// V: phase 1. 0 = the register-window FIR (variant 0); 1 .. 4 = the Toeplitz-band product on the matrix pipe (variant
// 1) with V = sm_steps(K) window steps.
template <int V>
__global__ __launch_bounds__(512, 1) void sepconv1d_mx_kernel(MxSepArgs p) {
  constexpr int MI = 2, NI = 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 2, wn = wid & 3;
  const int b = blockIdx.x / p.MT, t0 = (blockIdx.x - b * p.MT) * kSepRows;
  const int lin = p.in_len ? min(max(p.in_len[b], 0), p.Tin) : p.Tin;
  const int lout = p.out_len ? min(max(p.out_len[b], 0), p.Tout) : p.Tout;

  if (t0 >= lout) {       // the whole tile lies past the sample's end: zeros, no depthwise or matrix work
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int c8n = p.Cout >> 3;
    for (int u = tid; u < kSepRows * c8n; u += 512) {
      const int r = u / c8n, t = t0 + r;
      if (t < p.Tout) sep_store8(p, b, t, (u - r * c8n) * 8, z);
    }
    return;
  }

  const int nct = (p.Cin + kMxKTile - 1) / kMxKTile, ng = p.Cin >> 6;
  char* const zq = smem;                               // [nct][128 rows][128 B], swizzled
  char* const zs = smem + nct * kSepZTile;             // [nct][128 rows][4] scale bytes = one word per (tile, row)
  char* const sh = zs + nct * (kSepRows * 4);          // the shared region

  // ================= phase 1: depthwise FIR -> bf16 -> MX quantiser -> zq / zs =================
  if constexpr (V >= 1) {
    sep_phase1_mfma<V>(p, b, t0, lin, zq, zs, sh);
  } else {
    const int nsl = p.slab >> 10;                      // DMA instructions of one slab, 8 rows each
    const int r0 = t0 - p.padL;                        // the input row of slab row 0
    const int row_bytes = p.Cin * 2;
    const __amdgpu_buffer_rsrc_t xrs = mx_rsrc(reinterpret_cast<const uint8_t*>(p.x + (long long)b * p.Tin * p.Cin),
                                               (long long)lin * row_bytes);
    auto stage_slab = [&](int g, int buf) {
      char* const s = sh + buf * p.slab;
#pragma unroll
      for (int pi = 0; pi < 4; ++pi) {
        const int i = pi * 8 + wid;                    // instruction i covers slab rows 8 i .. 8 i + 7
        if (i < nsl) {
          const int row = i * 8 + (lane >> 3);
          const int off = (r0 + row) * row_bytes + g * 128 + (lane & 7) * 16;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(s + i * 1024), 16,
                                                   r0 + row < 0 ? kSepBehind : off, 0, 0, 0);
        }
      }
    };
    float* const taps = reinterpret_cast<float*>(sh + 2 * p.slab);      // [K][64]
    float tp[kSepTapRegs];
    auto load_taps = [&](int g) {
#pragma unroll
      for (int i = 0; i < kSepTapRegs; ++i) {
        const int idx = i * 512 + tid, k = idx >> 6;
        tp[i] = k < p.K ? p.d[(long long)k * p.Cin + g * 64 + (idx & 63)] : 0.f;
      }
    };
    const int pr = tid & 31, run = tid >> 5;           // channel pair of the group, run of 8 rows (wave: 2 runs)
    stage_slab(0, 0);
    load_taps(0);
    for (int g = 0; g < ng; ++g) {
      // nobody reads the taps of group g - 1 any more (barrier C below)
#pragma unroll
      for (int i = 0; i < kSepTapRegs; ++i) {
        const int idx = i * 512 + tid;
        if ((idx >> 6) < p.K) taps[idx] = tp[i];
      }
      // slab g has landed — this wave's share, the barrier makes it everybody's — and the other slab buffer (slab
      // and transpose patches of group g - 1) is read by nobody
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      mx_barrier();
      if (g + 1 < ng) {
        stage_slab(g + 1, (g + 1) & 1);
        load_taps(g + 1);
      }
      char* const slab = sh + (g & 1) * p.slab;
      const char* const xr = slab + run * 8 * 128 + pr * 4;
      const float* const wr = taps + pr * 2;
      float a[8][2], xw[8][2];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j][0] = a[j][1] = 0.f;
#pragma unroll
      for (int sl = 0; sl < 7; ++sl) sep_row(xr + sl * 128, xw[sl]);
      // window slot of output j at tap k = kb + kk is (j + kk) & 7 — static after unrolling
      for (int kb = 0; kb < p.K; kb += 8) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          const int k = kb + kk;
          if (k < p.K) {
            sep_row(xr + (k + 7) * 128, xw[(7 + kk) & 7]);
            const f32x2 w = *reinterpret_cast<const f32x2*>(wr + k * 64);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              a[j][0] = __builtin_fmaf(xw[(j + kk) & 7][0], w[0], a[j][0]);
              a[j][1] = __builtin_fmaf(xw[(j + kk) & 7][1], w[1], a[j][1]);
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      mx_barrier();                                    // C: everybody is through with slab g and the taps
      char* const zt = slab + wid * 2048;              // this wave's 16 rows x 64 channels of bf16
#pragma unroll
      for (int j = 0; j < 8; ++j)
        *reinterpret_cast<uint32_t*>(zt + ((run & 1) * 8 + j) * 128 + pr * 4) = pack2bf(a[j][0], a[j][1]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      const int q = lane & 7, ct = g >> 1;             // 8 channels 8 q .. of the group; quad = one block of 32
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int lr = h * 8 + (lane >> 3), row = wid * 16 + lr;
        const u32x4 v = *reinterpret_cast<const u32x4*>(zt + lr * 128 + q * 16);
        int byte;
        const u32x2 o = mx_quantize8(v, byte);
        const int slot = (g & 1) * 4 + (q >> 1);
        *reinterpret_cast<u32x2*>(zq + ct * kSepZTile + row * kMxKTile + ((slot ^ ((row >> 1) & 7)) << 4) +
                                  (q & 1) * 8) = o;
        if ((q & 3) == 0) zs[(ct * kSepRows + row) * 4 + (g & 1) * 2 + (q >> 2)] = (char)byte;
      }
    }
  }
  // zq and zs are complete and the shared region is free once every wave is here
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  mx_barrier();

  // ================= phase 2: y = epilogue(zq . wq^T), 256 columns at a time =================
  int wv[4];
#pragma unroll
  for (int pi = 0; pi < 4; ++pi) {
    const int row = (pi * 8 + wid) * 8 + (lane >> 3), slot = (lane & 7) ^ ((row >> 1) & 7);
    wv[pi] = row * p.Cin + slot * 16;
  }
  // W of chunk c: columns 256 c .. up to Cout; a column past Cout lies behind the descriptor's end and reads as 0
  auto stage_w = [&](int c, int ct, int buf) {
    const __amdgpu_buffer_rsrc_t wrs =
        mx_rsrc(p.w + (long long)c * kMxTile * p.Cin, (long long)(p.Cout - c * kMxTile) * p.Cin);
    char* const s = sh + buf * kMxOperand;
#pragma unroll
    for (int pi = 0; pi < 4; ++pi)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          wrs, (__attribute__((address_space(3))) void*)(s + (pi * 8 + wid) * 1024), 16, wv[pi] + ct * kMxKTile, 0,
          0, 0);
  };
  auto load_wscales = [&](int c, int ct, uint32_t (&sw)[NI]) {
#pragma unroll
    for (int in = 0; in < NI; ++in)      // a column past Cout is all zeros: any scale will do
      sw[in] = p.w_scale[(long long)ct * p.Cout + min(c * kMxTile + wn * 64 + in * 32 + l31, p.Cout - 1)];
  };

  f32x16 acc[NI][MI];
#pragma unroll
  for (int in = 0; in < NI; ++in)
#pragma unroll
    for (int im = 0; im < MI; ++im)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[in][im][e] = 0.f;

  // fragment offsets inside a 32-row block of a 128-byte-wide tile: MFMA step ks, the lane's piece h of scale block h
  int foff[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      foff[ks][h] = l31 * kMxKTile + (((ks * 4 + h * 2 + lhi) ^ ((l31 >> 1) & 7)) << 4);
  const int abase = wm * 64 * kMxKTile, wbase = wn * 64 * kMxKTile;

  const int nch = (p.Cout + kMxTile - 1) / kMxTile, nsteps = nch * nct;
  const bool half_tail = (p.Cin & (kMxKTile - 1)) != 0;
  const int shb = lhi * 8;
  const int rr = lane >> 2, c8 = (lane & 3) * 8;       // epilogue: patch row of a 16-row pass, first of 8 columns
  uint32_t sw_n[NI];
  stage_w(0, 0, 0);
  load_wscales(0, 0, sw_n);
  int c = 0, ct = 0;
  for (int it = 0; it < nsteps; ++it) {
    uint32_t sw[NI], sa[MI];
#pragma unroll
    for (int in = 0; in < NI; ++in) sw[in] = sw_n[in] >> shb;
    // this step's W has landed and nobody reads the other stage (W of step it - 1, or the patches of the chunk
    // that ended there)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    mx_barrier();
    int ctn = ct + 1, cn = c;
    if (ctn == nct) { ctn = 0; ++cn; }
    if (it + 1 < nsteps) {
      stage_w(cn, ctn, (it + 1) & 1);
      load_wscales(cn, ctn, sw_n);
    }
#pragma unroll
    for (int im = 0; im < MI; ++im)
      sa[im] = *reinterpret_cast<const uint32_t*>(zs + (ct * kSepRows + wm * 64 + im * 32 + l31) * 4) >> shb;
    const char* const za = zq + ct * kSepZTile + abase;
    const char* const sw_lds = sh + (it & 1) * kMxOperand + wbase;
    auto mfma_step = [&](auto KS) {
      constexpr int ks = decltype(KS)::value;
      i32x8 wf[NI], af[MI];
#pragma unroll
      for (int in = 0; in < NI; ++in) wf[in] = mx_frag(sw_lds + in * 32 * kMxKTile, foff[ks][0], foff[ks][1]);
#pragma unroll
      for (int im = 0; im < MI; ++im) af[im] = mx_frag(za + im * 32 * kMxKTile, foff[ks][0], foff[ks][1]);
#pragma unroll
      for (int im = 0; im < MI; ++im)
#pragma unroll
        for (int in = 0; in < NI; ++in)
          acc[in][im] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[in], af[im], acc[in][im], 0, 0, ks * 2,
                                                                        (int)sw[in], ks * 2, (int)sa[im]);
    };
    mfma_step(std::integral_constant<int, 0>{});
    if (!(half_tail && ct == nct - 1)) mfma_step(std::integral_constant<int, 1>{});

    if (ct == nct - 1) {
      // ---- epilogue of chunk c. D[i][j]: i = output column = 8 (e / 4) + 4 (lane / 32) + e % 4, j = output row =
      // lane % 32. The patches take the W stage just read, once every wave is through with it.
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      mx_barrier();
      char* const patch = sh + (it & 1) * kMxOperand + wid * 4096;
#pragma unroll
      for (int in = 0; in < NI; ++in) {
        const int col = c * kMxTile + wn * 64 + in * 32 + c8;
        float cs[8], cb[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { cs[e] = 1.f; cb[e] = 0.f; }
        if (p.ch_scale && col < p.Cout) load8(p.ch_scale + col, cs);
        if (p.ch_shift && col < p.Cout) load8(p.ch_shift + col, cb);
#pragma unroll
        for (int im = 0; im < MI; ++im) {
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const f32x4 v = {acc[in][im][4 * qq], acc[in][im][4 * qq + 1], acc[in][im][4 * qq + 2],
                             acc[in][im][4 * qq + 3]};
            *reinterpret_cast<f32x4*>(patch + l31 * 128 + (((2 * qq + lhi) ^ ((l31 >> 1) & 7)) << 4)) = v;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[in][im][4 * qq + e] = 0.f;
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int ps = 0; ps < 2; ++ps) {
            const int prow = ps * 16 + rr, key = (prow >> 1) & 7;
            const int t = t0 + wm * 64 + im * 32 + prow;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(patch + prow * 128 + (((lane & 3) * 2 ^ key) << 4));
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(patch + prow * 128 + ((((lane & 3) * 2 + 1) ^ key) << 4));
            if (t < p.Tout && col < p.Cout) {
              float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                v[e] = v[e] * cs[e] + cb[e];
                if (p.act == 1) v[e] = fmaxf(v[e], 0.f);
                if (t >= lout) v[e] = 0.f;
              }
              sep_store8(p, b, t, col, v);
            }
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
    c = cn;
    ct = ctn;
  }
}

// variant -1: the choice by shape. Variant 1 where it measured faster than variant 0
// (profiles/mxfp8_sepconv_mfma_first_measurements.md); 384 is the midpoint of the measured widths 256 and 512, a
// convention.
static int sep_variant_by_shape(int Cin) { return Cin >= 384 ? 1 : 0; }

static int sepconv1d_mx_launch(os2s_stream_t stream, const uint16_t* x, const float* d, const uint8_t* wq,
                               const uint8_t* w_scale, void* y, const int32_t* in_len, const int32_t* out_len,
                               const float* ch_scale, const float* ch_shift, int B, int Tin, int Cin, int Cout, int K,
                               int stride, int dil, int padL, int Tout, long long y_stride_b, long long y_stride_t,
                               int out_f32, int act, int variant) {
  OS2S_REQUIRE(variant >= -1 && variant <= 1);
  OS2S_REQUIRE(x && d && wq && w_scale && y);
  OS2S_REQUIRE(B >= 1 && Tin >= 1 && Tout >= 1 && K >= 1 && stride >= 1 && dil >= 1 && Cin >= 1 && Cout >= 1);
  if (stride != 1 || dil != 1 || K > kSepMaxK) return OS2S_ERR_UNSUPPORTED;
  if (Cin < 64 || Cin % 64 != 0 || Cin > kSepMaxCin || Cout % 8 != 0) return OS2S_ERR_UNSUPPORTED;
  if (act != 0 && act != 1) return OS2S_ERR_UNSUPPORTED;
  OS2S_REQUIRE(padL >= 0 && padL <= K - 1);
  OS2S_REQUIRE(y_stride_t >= Cout && y_stride_t % 8 == 0 && y_stride_b % 8 == 0);
  OS2S_REQUIRE(((uintptr_t)x | (uintptr_t)wq | (uintptr_t)y | (uintptr_t)ch_scale | (uintptr_t)ch_shift) % 16 == 0);
  OS2S_REQUIRE(((uintptr_t)d | (uintptr_t)w_scale | (uintptr_t)in_len | (uintptr_t)out_len) % 4 == 0);
  // 32-bit byte offsets: inside a sample for the slab (rows -padL .. Tout + 127 + K + 8), inside wq for W
  const long long span = (long long)(Tin > Tout ? Tin : Tout) + kSepRows + K + 8;
  if (span * Cin * 2 >= (1ll << 31) || ((long long)Cout + kMxTile) * Cin >= (1ll << 31)) return OS2S_ERR_UNSUPPORTED;
  MxSepArgs p;
  p.x = x; p.d = d; p.w = wq; p.w_scale = reinterpret_cast<const uint32_t*>(w_scale);
  p.y = y; p.in_len = in_len; p.out_len = out_len; p.ch_scale = ch_scale; p.ch_shift = ch_shift;
  p.y_stride_b = y_stride_b; p.y_stride_t = y_stride_t;
  p.B = B; p.Tin = Tin; p.Cin = Cin; p.Cout = Cout; p.K = K; p.padL = padL; p.Tout = Tout;
  p.act = act; p.out_f32 = out_f32;
  p.MT = ceil_div(Tout, kSepRows);
  p.slab = sep_slab_bytes(K);
  if ((long long)B * p.MT >= (1ll << 31)) return OS2S_ERR_UNSUPPORTED;
  const int nct = ceil_div(Cin, kMxKTile);
  if (variant < 0) variant = sep_variant_by_shape(Cin);
  const int phase1 = variant == 1 ? sm_phase1_bytes(K) : 2 * p.slab + K * 64 * 4, phase2 = 2 * kMxOperand;
  const size_t lds = (size_t)nct * (kSepZTile + kSepRows * 4) + (size_t)(phase1 > phase2 ? phase1 : phase2);
  const int J = sm_steps(K);
  if (variant == 1 && J == 1) {
    OS2S_LAUNCH_LDS(sepconv1d_mx_kernel<1>, dim3(B * p.MT), dim3(512), lds, (hipStream_t)stream, p);
  } else if (variant == 1 && J == 2) {
    OS2S_LAUNCH_LDS(sepconv1d_mx_kernel<2>, dim3(B * p.MT), dim3(512), lds, (hipStream_t)stream, p);
  } else if (variant == 1 && J == 3) {
    OS2S_LAUNCH_LDS(sepconv1d_mx_kernel<3>, dim3(B * p.MT), dim3(512), lds, (hipStream_t)stream, p);
  } else if (variant == 1) {
    OS2S_LAUNCH_LDS(sepconv1d_mx_kernel<4>, dim3(B * p.MT), dim3(512), lds, (hipStream_t)stream, p);
  } else {
    OS2S_LAUNCH_LDS(sepconv1d_mx_kernel<0>, dim3(B * p.MT), dim3(512), lds, (hipStream_t)stream, p);
  }
  return OS2S_OK;
}

}  // namespace os2s

extern "C" int os2s_sepconv1d_fwd_mx(os2s_stream_t stream, const uint16_t* x, const float* d, const uint8_t* wq,
                                     const uint8_t* w_scale, void* y, const int32_t* in_len, const int32_t* out_len,
                                     const float* ch_scale, const float* ch_shift, int B, int Tin, int Cin, int Cout,
                                     int K, int stride, int dil, int padL, int Tout, long long y_stride_b,
                                     long long y_stride_t, int out_f32, int act) {
  return os2s::sepconv1d_mx_launch(stream, x, d, wq, w_scale, y, in_len, out_len, ch_scale, ch_shift, B, Tin, Cin,
                                   Cout, K, stride, dil, padL, Tout, y_stride_b, y_stride_t, out_f32, act, 0);
}

extern "C" int os2s_sepconv1d_fwd_mx_variant(os2s_stream_t stream, const uint16_t* x, const float* d,
                                             const uint8_t* wq, const uint8_t* w_scale, void* y,
                                             const int32_t* in_len, const int32_t* out_len, const float* ch_scale,
                                             const float* ch_shift, int B, int Tin, int Cin, int Cout, int K,
                                             int stride, int dil, int padL, int Tout, long long y_stride_b,
                                             long long y_stride_t, int out_f32, int act, int variant) {
  return os2s::sepconv1d_mx_launch(stream, x, d, wq, w_scale, y, in_len, out_len, ch_scale, ch_shift, B, Tin, Cin,
                                   Cout, K, stride, dil, padL, Tout, y_stride_b, y_stride_t, out_f32, act, variant);
}
