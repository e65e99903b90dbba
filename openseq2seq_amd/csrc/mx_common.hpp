// Device helpers shared by the MXFP8 kernels (gemm_mx.hip, gemm_skinny_mx.hip, conv1d_mx.hip): the quantisation of
// eight elements under the format rule at the head of gemm_mx.hip, the buffer descriptor of the LDS DMA, the
// barrier, and the fragment read / epilogue patch of the 256 x 256 tile.
#pragma once
#include "os2s_common.hpp"

namespace os2s {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// Eight bf16 of one lane -> eight e4m3 bytes and the scale byte of their block of 32. The four lanes of an aligned
// quad hold one block (8 consecutive elements each); every lane of the quad returns the same `byte`.
__device__ __forceinline__ u32x2 mx_quantize8(const u32x4& v, int& byte) {
  // largest magnitude as an integer: bf16 without its sign orders like its value
  int m = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int lo = (int)(v[e] & 0x7fffu), hi = (int)((v[e] >> 16) & 0x7fffu);
    m = max(m, max(lo, hi));
  }
  m = max(m, __builtin_amdgcn_update_dpp(0, m, 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
  m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
  byte = max((m >> 7) - 8, 0);                                            // exponent field - 8, clamped at 0
  const float mult = __builtin_bit_cast(float, (uint32_t)(254 - byte) << 23);   // 2^-(byte - 127)
  u32x2 o;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float a0 = fminf(fmaxf(bflo(v[2 * h]) * mult, -448.f), 448.f);
    const float a1 = fminf(fmaxf(bfhi(v[2 * h]) * mult, -448.f), 448.f);
    const float a2 = fminf(fmaxf(bflo(v[2 * h + 1]) * mult, -448.f), 448.f);
    const float a3 = fminf(fmaxf(bfhi(v[2 * h + 1]) * mult, -448.f), 448.f);
    int pk = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, 0, false);
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(a2, a3, pk, true);
    o[h] = (uint32_t)pk;
  }
  return o;
}

// The four scale bytes of a (row, 128-element K tile) unit held by 16 consecutive lanes (aligned at 16), gathered
// from the first lane of each quad, as the word of the scale layout.
__device__ __forceinline__ uint32_t mx_scale_word(int byte, int lane) {
  const int g0 = lane & 48;
  return (uint32_t)__shfl(byte, g0, 64) | ((uint32_t)__shfl(byte, g0 + 4, 64) << 8) |
         ((uint32_t)__shfl(byte, g0 + 8, 64) << 16) | ((uint32_t)__shfl(byte, g0 + 12, 64) << 24);
}

__device__ __forceinline__ void mx_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// ---- the 256 x 256 tile of gemm_mx.hip and conv1d_mx.hip (layout and swizzle: the head of gemm_mx.hip) ----
constexpr int kMxTile = 256, kMxKTile = 128;
constexpr int kMxOperand = kMxTile * kMxKTile;          // bytes of one operand tile
constexpr int kMxPatchStride = 68;                      // floats per row of a wave's epilogue patch
constexpr int kMxPatch = 32 * kMxPatchStride * 4;       // bytes

// A lane's 32-byte fragment of one MFMA step: its two 16-byte pieces (scale block 0, scale block 1) at the byte
// offsets off0 / off1 of a 32-row block in LDS.
__device__ __forceinline__ i32x8 mx_frag(const char* s, int off0, int off1) {
  const u32x4 lo = *reinterpret_cast<const u32x4*>(s + off0);
  const u32x4 hi = *reinterpret_cast<const u32x4*>(s + off1);
  i32x8 f;
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[e] = (int)lo[e]; f[4 + e] = (int)hi[e]; }
  return f;
}

// One 32x32 accumulator block D[i][j] (i = output column = 8 (e / 4) + 4 (lane / 32) + e % 4, j = output row =
// lane % 32) into columns 32 in .. 32 in + 31 of this wave's epilogue patch.
__device__ __forceinline__ void mx_acc_to_patch(float* patch, const f32x16& a, int in, int l31, int lhi) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 v = {a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
    *reinterpret_cast<f32x4*>(patch + l31 * kMxPatchStride + in * 32 + q * 8 + lhi * 4) = v;
  }
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t mx_rsrc(const uint8_t* base, long long bytes) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)base);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)base >> 32));
  const long long cl = bytes < 0 ? 0 : (bytes < 0x7fffffffll ? bytes : 0x7fffffffll);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0,
                                           __builtin_amdgcn_readfirstlane((int)cl), 0x00020000);
}

}  // namespace os2s
