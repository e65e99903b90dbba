// Row-block helpers shared by the one-wave-per-row LayerNorm backward kernels (layernorm_bwd_kernel in
// transformer.hip, layernorm_l1_bwd_kernel in transformer_norm.hip): a buffer descriptor over the n rows of D bf16
// a workgroup owns, so the prefetch past the last row needs no branch (out of range: zeros, no memory request), and
// the registers of one prefetched row.
#pragma once
#include "os2s_common.hpp"

namespace os2s {

__device__ __forceinline__ __amdgpu_buffer_rsrc_t ln_rows_rsrc(const void* base, long long r0, int n, int D) {
  const unsigned long long a = (unsigned long long)base + (unsigned long long)r0 * (unsigned)D * 2ull;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  const int bytes = __builtin_amdgcn_readfirstlane(base ? n * D * 2 : 0);   // null tensor: everything is out of range
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, bytes, 0x00020000);
}

// dy, x, residual gradient (16 bytes per lane per vector) and the row's two saved statistics
template <int VPL>
struct LnRow {
  u32x4 a[VPL], t[VPL], r[VPL];
  float mu, rs;
};

}  // namespace os2s
