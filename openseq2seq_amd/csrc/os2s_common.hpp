// Shared device/host helpers for the os2s HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/os2s.h"

// hipGetLastError() is sticky per thread and also reports benign errors left
// behind by other HIP users in the process (e.g. PyTorch's event queries), so
// every launch is bracketed: clear first, then check.
#define OS2S_LAUNCH(kernel, grid, block, smem, stream, ...)              \
  do {                                                                   \
    (void)hipGetLastError();                                             \
    hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__);  \
    hipError_t e__ = hipGetLastError();                                  \
    if (e__ != hipSuccess) {                                             \
      os2s_record_hip_error((int)e__, #kernel);                          \
      return OS2S_ERR_LAUNCH;                                            \
    }                                                                    \
  } while (0)

extern "C" void os2s_record_hip_error(int hip_error, const char* where);

// THE launch form of a kernel whose dynamic LDS can reach the default limit of 64 KB: OS2S_LAUNCH, after making
// sure that this kernel has been opted in (up to the 160 KB of a gfx950 CU) on the CURRENT device; the attribute
// belongs to a (function, device) pair. One flag word per expansion site, and so per template instance, one bit
// per device: a launch of 64 KB or more costs hipGetDevice and an atomic load. A failure is recorded and returned,
// never latched: the next call tries again. Two host threads may both set the attribute; that is harmless, and
// so is the opt-in of a launch exactly at the limit. Launches below 64 KB go straight through, so a site may use
// this form whatever its size.
// OS2S_LAUNCH_LDS_MAX names the limit to opt in to, for a kernel whose static LDS leaves less than 160 KB.
#define OS2S_LAUNCH_LDS_MAX(lds_max, kernel, grid, block, smem, stream, ...)                \
  do {                                                                                      \
    if ((size_t)(smem) >= os2s::kLdsDefault) {                                              \
      static std::atomic<uint32_t> opted__{0};                                              \
      const hipError_t a__ = os2s::lds_opt_in(opted__, (const void*)kernel, (int)(lds_max)); \
      if (a__ != hipSuccess) {                                                              \
        os2s_record_hip_error((int)a__, #kernel);                                           \
        return OS2S_ERR_LAUNCH;                                                             \
      }                                                                                     \
    }                                                                                       \
    OS2S_LAUNCH(kernel, grid, block, smem, stream, __VA_ARGS__);                            \
  } while (0)
#define OS2S_LAUNCH_LDS(kernel, grid, block, smem, stream, ...) \
  OS2S_LAUNCH_LDS_MAX(os2s::kLdsMax, kernel, grid, block, smem, stream, __VA_ARGS__)

#define OS2S_REQUIRE(cond) \
  do {                     \
    if (!(cond)) return OS2S_ERR_INVALID_ARG; \
  } while (0)

namespace os2s {

// Named test / measurement options behind the ONE entry point os2s_set_option (os2s_api.hip). A translation
// unit registers its knobs next to the state they set: `static OptionReg r("conv1d.variant", &g_conv_variant);`
// (host-side only; the registry lives behind a function-local static so the order in which the translation
// units are initialised does not matter). A knob is the file-scope variable the launch path reads, registered by
// address (a setter / getter pair only where setting has a side effect); os2s_get_option returns it. A
// registration may name an environment variable: it is read ONCE, at registration (static initialisation, when the
// library is loaded), and stored as os2s_set_option would: atoi of the text, or `parse` of it. That is the
// library's only getenv. Options are changed BETWEEN passes: a forward and its backward, and a workspace-size query
// and the call that uses the workspace, have to see the same values.
typedef void (*OptionSetter)(double value);
typedef double (*OptionGetter)();
typedef int (*OptionParser)(const char* text);
struct OptionReg {
  OptionReg(const char* name, int* var, const char* env = nullptr, OptionParser parse = nullptr);
  OptionReg(const char* name, float* var);
  OptionReg(const char* name, OptionSetter set, OptionGetter get);
};
// debug time-stamp buffers of instrumented kernels (os2s_set_debug_stamps): fn(stamps, mode)
typedef void (*StampSetter)(void* stamps, int mode);
struct StampReg { StampReg(const char* name, StampSetter fn); };

constexpr int kWave = 64;

// ---- per-device host state (device indices 0 .. 31 are cached; beyond that the runtime is asked every time) ----
constexpr size_t kLdsDefault = 64 * 1024;   // LDS a kernel may use without an opt-in (static + dynamic)
constexpr int kLdsMax = 160 * 1024;         // LDS of a gfx950 CU

// Behind OS2S_LAUNCH_LDS: `opted` has bit d set once `fn` may use `lds_max` bytes of dynamic LDS on device d.
inline hipError_t lds_opt_in(std::atomic<uint32_t>& opted, const void* fn, int lds_max) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) dev = -1;
  if (dev >= 0 && ((opted.load(std::memory_order_acquire) >> dev) & 1u)) return hipSuccess;
  const hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
  if (rc == hipSuccess && dev >= 0) opted.fetch_or(1u << dev, std::memory_order_release);
  return rc;
}

// CUs of the current device; `unknown` (256: an MI355X) when the runtime cannot be asked.
inline int device_cus(int unknown = 256) {
  static std::atomic<int> cus[32];   // zero-initialised: 0 = not asked yet
  int dev = -1, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return unknown;
  if (dev < 32 && (n = cus[dev].load(std::memory_order_relaxed)) > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return unknown;
  if (dev < 32) cus[dev].store(n, std::memory_order_relaxed);
  return n;
}

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

typedef uint16_t bf16_t;  // raw storage type used across the C ABI

// round-to-nearest-even fp32 -> bf16 (NaN stays a quiet NaN): the gfx950 conversion instruction
// v_cvt_pk_bf16_f32, two values per instruction. (The integer formulation — add 0x7fff + lsb, NaN
// test per value — is ~12 VALU instructions and two exec-mask branches per value; it was 2000 of
// the instructions of a 256 x 256 convolution epilogue.)
typedef __bf16 hw_bf16x2 __attribute__((ext_vector_type(2)));
typedef float hw_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) {
  const hw_f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, hw_bf16x2));
}
__device__ __forceinline__ bf16_t f2bf(float f) { return (bf16_t)(pack2bf(f, 0.f) & 0xffffu); }
__device__ __forceinline__ float bf2f(bf16_t h) {
  return __builtin_bit_cast(float, ((uint32_t)h) << 16);
}
__device__ __forceinline__ float bflo(uint32_t p) {
  return __builtin_bit_cast(float, p << 16);
}
__device__ __forceinline__ float bfhi(uint32_t p) {
  return __builtin_bit_cast(float, p & 0xffff0000u);
}
// eight bf16 of one 16-byte vector <-> eight floats
__device__ __forceinline__ void unpack8(const u32x4& t, float (&f)[8]) {
#pragma unroll
  for (int w = 0; w < 4; ++w) { f[2 * w] = bflo(t[w]); f[2 * w + 1] = bfhi(t[w]); }
}
__device__ __forceinline__ u32x4 pack8(const float (&f)[8]) {
  u32x4 o;
#pragma unroll
  for (int w = 0; w < 4; ++w) o[w] = pack2bf(f[2 * w], f[2 * w + 1]);
  return o;
}
// eight consecutive fp32 per-column values (c0 a multiple of 8: 32-byte aligned in a torch allocation)
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// DPP-based wave64 reductions for FULLY ACTIVE waves (checked against the shuffle versions by
// tools/probe_dpp.hip): six VALU DPP moves instead of six ds_bpermute round trips through
// the LDS crossbar (~10x lower latency — it matters in the sequential decoder kernels). The
// result is wave-uniform (read from lane 63).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_mov(float old, float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(x), CTRL,
                                                    ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum_dpp(float x) {
  x += dpp_mov<0xB1, 0xf>(0.f, x);    // quad_perm [1,0,3,2]
  x += dpp_mov<0x4E, 0xf>(0.f, x);    // quad_perm [2,3,0,1]
  x += dpp_mov<0x124, 0xf>(0.f, x);   // row_ror:4
  x += dpp_mov<0x128, 0xf>(0.f, x);   // row_ror:8
  x += dpp_mov<0x142, 0xa>(0.f, x);   // row_bcast:15 into rows 1, 3
  x += dpp_mov<0x143, 0xc>(0.f, x);   // row_bcast:31 into rows 2, 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
__device__ __forceinline__ float wave_max_dpp(float x) {
  const float ninf = -__builtin_inff();
  x = fmaxf(x, dpp_mov<0xB1, 0xf>(ninf, x));
  x = fmaxf(x, dpp_mov<0x4E, 0xf>(ninf, x));
  x = fmaxf(x, dpp_mov<0x124, 0xf>(ninf, x));
  x = fmaxf(x, dpp_mov<0x128, 0xf>(ninf, x));
  x = fmaxf(x, dpp_mov<0x142, 0xa>(ninf, x));
  x = fmaxf(x, dpp_mov<0x143, 0xc>(ninf, x));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

// Counter-based RNG (philox-like mixing, cheap): deterministic per (seed, idx).
__device__ __forceinline__ uint32_t hash_u32(uint64_t seed, uint64_t idx) {
  uint64_t z = idx * 0x9E3779B97F4A7C15ull + seed;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (uint32_t)(z >> 32);
}

// 256 B of zeros: LDS-DMA source for padding rows / masked frames (one copy per
// translation unit; device code is not linked across TUs).
static __device__ __attribute__((aligned(256))) uint32_t g_zero_page[64];

// 4 keep/drop decisions (elements idx4*4 .. idx4*4 + 3) from the mixing state
// z0 = idx4 * kDropGolden + seed: one 64-bit mix -> four 16-bit uniforms, keep iff u16 < thr
// (thr = keep * 65536). Callers that walk idx4 in constant steps add step * kDropGolden to z0
// instead of redoing the first multiply.
constexpr unsigned long long kDropGolden = 0x9E3779B97F4A7C15ull;
__device__ __forceinline__ uint32_t dropout_bits4_z(unsigned long long z, uint32_t thr) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  uint32_t bits = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t u = (uint32_t)(z >> (16 * e)) & 0xffffu;
    bits |= (u < thr ? 1u : 0u) << e;
  }
  return bits;
}
// 8 keep/drop decisions for the 8 channels starting at element index idx8*8:
// two 64-bit mixes (idx4 = idx8*2, idx8*2 + 1) -> eight 16-bit uniforms, keep iff u16 < keep*65536.
__device__ __forceinline__ uint32_t dropout_bits8(unsigned long long seed,
                                                  unsigned long long idx8,
                                                  float keep_prob) {
  const uint32_t thr = (uint32_t)(keep_prob * 65536.0f);
  const unsigned long long z0 = (idx8 * 2) * kDropGolden + seed;
  return dropout_bits4_z(z0, thr) | (dropout_bits4_z(z0 + kDropGolden, thr) << 4);
}

static inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace os2s
