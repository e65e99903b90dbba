// Sampled softmax of the LSTM language model (tf.nn.sampled_softmax_loss at losses/sequence_loss.py:391-396): the
// log-uniform candidate sampler, the gather of the sampled rows into a compact GEMM operand, the row loss with
// accidental-hit removal, and the scatter / true-row halves of the backward. The [N, S] logits and the two compact
// gradient GEMMs run on the existing GEMM entry points; see include/os2s.h for the arithmetic.
#include <math.h>

#include "os2s_common.hpp"

namespace os2s {

constexpr int kSsThreads = 256;    // workgroup of every kernel here; the sampler draws this many tries per round
constexpr int kSsLdsHead = 264;    // words in front of the sampler's bitmap: cls[256], wsum[4], stop, 3 pad

// exclusive prefix sum of one int per thread over the 256-thread workgroup; `total` is uniform
__device__ __forceinline__ int ss_block_excl_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();   // the previous use of wsum has been read
  if (lane == 63) wsum[wid] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wid; ++w) base += wsum[w];
  total = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
  return base + inc - v;
}

// log of the expected count Q(k) = -expm1(num_tries * log1p(-p(k))), p(k) = log((k+2)/(k+1)) / log(V+1)
__device__ __forceinline__ float ss_log_q(int k, int num_tries, double inv_log_v1) {
  const double p = log1p(1.0 / ((double)k + 1.0)) * inv_log_v1;
  return (float)log(-expm1((double)num_tries * log1p(-p)));
}

// One workgroup. Try t draws hash_u32(seed, t) and maps it to the class k with bounds[k-1] <= u < bounds[k] (the last
// bound counts as 2^32): integer compares only. A round takes 256 tries: a try is NEW when its class is neither in the
// bitmap of the earlier rounds nor drawn by a lower try of the same round, so the accepted classes are the first S
// distinct ones in try order whatever the round size. At the cap the free classes fill the rest in ascending order.
__global__ __launch_bounds__(kSsThreads) void ss_sampler_kernel(
    const uint32_t* __restrict__ bounds, int V, int S, int Spad, unsigned long long seed, int max_tries,
    int32_t* ids, int32_t* __restrict__ num_tries, float* __restrict__ log_q) {
  extern __shared__ uint32_t ss_lds[];
  int* const cls = reinterpret_cast<int*>(ss_lds);
  int* const wsum = cls + kSsThreads;
  int* const stop = wsum + 4;
  uint32_t* const bitmap = ss_lds + kSsLdsHead;
  const int tid = threadIdx.x;
  const int words = (V + 31) >> 5;
  for (int i = tid; i < words; i += kSsThreads) bitmap[i] = 0u;
  if (tid == 0) *stop = max_tries;
  __syncthreads();
  int nfound = 0;   // uniform
  for (int t0 = 0; nfound < S && t0 < max_tries; t0 += kSsThreads) {
    const int t = t0 + tid;
    int k = -1;
    if (t < max_tries) {
      const uint32_t u = hash_u32(seed, (uint64_t)t);
      int lo = 0, hi = V - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u < bounds[mid]) hi = mid; else lo = mid + 1;
      }
      k = lo;
      if ((bitmap[k >> 5] >> (k & 31)) & 1u) k = -1;
    }
    cls[tid] = k;
    __syncthreads();
    bool isnew = k >= 0;
    if (isnew) {
      for (int j = 0; j < tid; ++j)
        if (cls[j] == k) { isnew = false; break; }   // the lower try owns the class
    }
    int total;
    const int slot = nfound + ss_block_excl_scan(isnew ? 1 : 0, wsum, total);
    if (isnew && slot < S) {
      ids[slot] = k;
      atomicOr(&bitmap[k >> 5], 1u << (k & 31));
      if (slot == S - 1) *stop = t + 1;
    }
    nfound += total;
    __syncthreads();
  }
  for (int w0 = 0; nfound < S && w0 < words; w0 += kSsThreads) {   // the cap was reached: fill
    const int w = w0 + tid;
    uint32_t free_bits = 0u;
    if (w < words) {
      free_bits = ~bitmap[w];
      const int rem = V - w * 32;
      if (rem < 32) free_bits &= (1u << rem) - 1u;
    }
    int total;
    int slot = nfound + ss_block_excl_scan(__popc(free_bits), wsum, total);
    while (free_bits && slot < S) {
      ids[slot++] = w * 32 + (__ffs(free_bits) - 1);
      free_bits &= free_bits - 1u;
    }
    nfound += total;
  }
  __syncthreads();
  const int nt = *stop;
  if (tid == 0) *num_tries = nt;
  const double inv_log_v1 = 1.0 / log((double)V + 1.0);
  for (int j = tid; j < Spad; j += kSsThreads) {
    if (j < S) {
      log_q[j] = ss_log_q(ids[j], nt, inv_log_v1);
    } else {
      ids[j] = -1;
      log_q[j] = 0.f;
    }
  }
}

// w_s[j] = table[ids[j]], b_s[j] = bias[ids[j]] - log_q[j]; padding rows (ids < 0) are zero
__global__ __launch_bounds__(kSsThreads) void ss_gather_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ log_q, const bf16_t* __restrict__ table,
    const float* __restrict__ bias, int V, int Spad, int D, bf16_t* __restrict__ w_s, float* __restrict__ b_s) {
  const int D8 = D >> 3;
  const long long n8 = (long long)Spad * D8;
  for (long long i = (long long)blockIdx.x * kSsThreads + threadIdx.x; i < n8;
       i += (long long)gridDim.x * kSsThreads) {
    const int j = (int)(i / D8), c = (int)(i - (long long)j * D8);
    const int id = ids[j];
    const bool valid = id >= 0 && id < V;
    u32x4 t = {0u, 0u, 0u, 0u};
    if (valid) t = *reinterpret_cast<const u32x4*>(table + (long long)id * D + c * 8);
    *reinterpret_cast<u32x4*>(w_s + (long long)j * D + c * 8) = t;
    if (c == 0) b_s[j] = valid ? (bias ? bias[id] : 0.f) - log_q[j] : 0.f;
  }
}

// One workgroup per row: the true logit, one online max / sum pass over the sampled logits, the gradient in a second.
__global__ __launch_bounds__(kSsThreads) void ss_loss_kernel(
    const bf16_t* __restrict__ x, long long ldx, const bf16_t* __restrict__ table, const float* __restrict__ bias,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ ids, const int32_t* __restrict__ num_tries,
    int V, int S, int Spad, int D, bf16_t* logits, long long ld, float grad_scale_host,
    const float* __restrict__ grad_scale_dev, int want_grad, float* __restrict__ row_loss,
    float* __restrict__ dtrue) {
  __shared__ float red_m[4], red_s[4];
  __shared__ float bc[2];
  const long long row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int label = labels[row];
  label = label < 0 ? 0 : (label > V - 1 ? V - 1 : label);
  // true[n] = x[n] . W[l] + b[l] - log Q(l)
  float acc = 0.f;
  for (int c = tid; c < (D >> 3); c += kSsThreads) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(x + row * ldx + c * 8);
    const u32x4 w = *reinterpret_cast<const u32x4*>(table + (long long)label * D + c * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += bflo(a[e]) * bflo(w[e]) + bfhi(a[e]) * bfhi(w[e]);
  }
  acc = wave_sum(acc);
  if (lane == 0) red_s[wid] = acc;
  __syncthreads();
  if (tid == 0) {
    const float dot = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    bc[0] = dot + (bias ? bias[label] : 0.f) - ss_log_q(label, *num_tries, 1.0 / log((double)V + 1.0));
  }
  __syncthreads();
  const float tl = bc[0];
  bf16_t* const lr = logits + row * ld;
  const int S8 = Spad >> 3;
  float m = tid == 0 ? tl : -INFINITY, s = tid == 0 ? 1.f : 0.f;
  for (int i = tid; i < S8; i += kSsThreads) {
    const u32x4 t = *reinterpret_cast<const u32x4*>(lr + (long long)i * 8);
    float v[8] = {bflo(t[0]), bfhi(t[0]), bflo(t[1]), bfhi(t[1]), bflo(t[2]), bfhi(t[2]), bflo(t[3]), bfhi(t[3])};
    float vm = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = i * 8 + e;
      const int id = ids[j];
      if (j >= S || id < 0 || id == label) v[e] = -INFINITY;   // padding column or accidental hit
      vm = fmaxf(vm, v[e]);
    }
    if (vm > -INFINITY) {
      const float mn = fmaxf(m, vm);
      float add = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) add += __expf(v[e] - mn);
      s = s * __expf(m - mn) + add;
      m = mn;
    }
  }
  const float wm = wave_max(m);
  s = wave_sum(m > -INFINITY ? s * __expf(m - wm) : 0.f);
  __syncthreads();
  if (lane == 0) { red_m[wid] = wm; red_s[wid] = s; }
  __syncthreads();
  if (tid == 0) {
    const float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));   // finite: the true logit is in
    float tot = 0.f;
    for (int w = 0; w < 4; ++w) tot += red_m[w] > -INFINITY ? red_s[w] * __expf(red_m[w] - M) : 0.f;
    bc[1] = M + __logf(tot);
  }
  __syncthreads();
  const float lse = bc[1];
  const float gs = grad_scale_dev ? grad_scale_host * (*grad_scale_dev) : grad_scale_host;
  if (tid == 0) {
    row_loss[row] = lse - tl;
    if (dtrue) dtrue[row] = gs * (__expf(tl - lse) - 1.f);
  }
  if (!want_grad) return;
  for (int i = tid; i < S8; i += kSsThreads) {
    const u32x4 t = *reinterpret_cast<const u32x4*>(lr + (long long)i * 8);
    const float v[8] = {bflo(t[0]), bfhi(t[0]), bflo(t[1]), bfhi(t[1]),
                        bflo(t[2]), bfhi(t[2]), bflo(t[3]), bfhi(t[3])};
    float g[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = i * 8 + e;
      const int id = ids[j];
      g[e] = (j >= S || id < 0 || id == label) ? 0.f : gs * __expf(v[e] - lse);
    }
    u32x4 o;
    o[0] = pack2bf(g[0], g[1]); o[1] = pack2bf(g[2], g[3]);
    o[2] = pack2bf(g[4], g[5]); o[3] = pack2bf(g[6], g[7]);
    *reinterpret_cast<u32x4*>(lr + (long long)i * 8) = o;
  }
}

__global__ void ss_sum_rows_kernel(const float* __restrict__ v, long long n, float mul, float* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) s += (double)v[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = (float)(red[0] * (double)mul);
}

// dtable[ids[j]] += dw_s[j], dbias[ids[j]] += db_s[j]: the sampled ids are distinct, plain adds
__global__ __launch_bounds__(kSsThreads) void ss_scatter_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ dw_s, const float* __restrict__ db_s, int V, int S,
    int D, float* __restrict__ dtable, float* __restrict__ dbias) {
  const int D4 = D >> 2;
  const long long n4 = (long long)S * D4;
  for (long long i = (long long)blockIdx.x * kSsThreads + threadIdx.x; i < n4;
       i += (long long)gridDim.x * kSsThreads) {
    const int j = (int)(i / D4), c = (int)(i - (long long)j * D4);
    const int id = ids[j];
    if (id < 0 || id >= V) continue;
    f32x4* const dst = reinterpret_cast<f32x4*>(dtable + (long long)id * D) + c;
    *dst = *dst + reinterpret_cast<const f32x4*>(dw_s + (long long)j * D)[c];
    if (c == 0 && dbias && db_s) dbias[id] += db_s[j];
  }
}

// One workgroup per row: dX[n] += dtrue[n] W[l], and whole contiguous rows of fp32 atomics into dtable[l] (labels
// repeat), one more into dbias[l].
__global__ __launch_bounds__(kSsThreads) void ss_true_bwd_kernel(
    const bf16_t* __restrict__ x, long long ldx, const bf16_t* __restrict__ table,
    const int32_t* __restrict__ labels, const float* __restrict__ dtrue, int V, int D, bf16_t* __restrict__ dx,
    long long lddx, float* __restrict__ dtable, float* __restrict__ dbias) {
  const long long row = blockIdx.x;
  int label = labels[row];
  label = label < 0 ? 0 : (label > V - 1 ? V - 1 : label);
  const float g = dtrue[row];
  if (dx) {
    for (int c = threadIdx.x; c < (D >> 3); c += kSsThreads) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(table + (long long)label * D + c * 8);
      u32x4* const dp = reinterpret_cast<u32x4*>(dx + row * lddx + c * 8);
      const u32x4 d = *dp;
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] = pack2bf(bflo(d[e]) + g * bflo(w[e]), bfhi(d[e]) + g * bfhi(w[e]));
      *dp = o;
    }
  }
  // one column per lane: every wave-wide atomic covers 256 contiguous bytes of the row
  float* const dst = dtable + (long long)label * D;
  for (int c = threadIdx.x; c < D; c += kSsThreads)
    __hip_atomic_fetch_add(dst + c, g * bf2f(x[row * ldx + c]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (threadIdx.x == 0 && dbias)
    __hip_atomic_fetch_add(dbias + label, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Deterministic mode: one thread per 8-column chunk walks the rows in order (thread D/8 owns the bias), so every
// element of dtable / dbias gets its adds from one thread in row order. The adds are the same memory-side fp32
// atomic as in default mode (one issuer per address, program order): the two modes differ in the order of the
// addends and in nothing else, whatever the rounding of that adder.
__global__ __launch_bounds__(kSsThreads) void ss_true_bwd_det_kernel(
    const bf16_t* __restrict__ x, long long ldx, const bf16_t* __restrict__ table,
    const int32_t* __restrict__ labels, const float* __restrict__ dtrue, long long N, int V, int D,
    bf16_t* __restrict__ dx, long long lddx, float* __restrict__ dtable, float* __restrict__ dbias) {
  const int D8 = D >> 3;
  const int col = blockIdx.x * kSsThreads + threadIdx.x;
  if (col > D8) return;
  for (long long row = 0; row < N; ++row) {
    int label = labels[row];
    label = label < 0 ? 0 : (label > V - 1 ? V - 1 : label);
    const float g = dtrue[row];
    if (col == D8) {
      if (dbias) __hip_atomic_fetch_add(dbias + label, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    const u32x4 a = *reinterpret_cast<const u32x4*>(x + row * ldx + col * 8);
    const u32x4 w = *reinterpret_cast<const u32x4*>(table + (long long)label * D + col * 8);
    if (dx) {
      u32x4* const dp = reinterpret_cast<u32x4*>(dx + row * lddx + col * 8);
      const u32x4 d = *dp;
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] = pack2bf(bflo(d[e]) + g * bflo(w[e]), bfhi(d[e]) + g * bfhi(w[e]));
      *dp = o;
    }
    float* const dst = dtable + (long long)label * D + col * 8;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      __hip_atomic_fetch_add(dst + 2 * e, g * bflo(a[e]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(dst + 2 * e + 1, g * bfhi(a[e]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

static inline int ss_blocks(long long work) {
  long long b = (work + kSsThreads - 1) / kSsThreads;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

}  // namespace os2s

using namespace os2s;

extern "C" int os2s_sampled_softmax_sample(os2s_stream_t stream, const uint32_t* bounds, int V, int S,
                                           unsigned long long seed, int max_tries, int32_t* ids,
                                           int32_t* num_tries, float* log_q) {
  OS2S_REQUIRE(bounds && ids && num_tries && log_q && max_tries >= 1 && max_tries <= (1 << 30));
  if (V < 2 || V > (1 << 20) || S < 1 || S > V / 2) return OS2S_ERR_UNSUPPORTED;
  const int Spad = (S + 7) / 8 * 8;
  const size_t smem = (size_t)(kSsLdsHead + (V + 31) / 32) * sizeof(uint32_t);
  OS2S_LAUNCH_LDS(ss_sampler_kernel, dim3(1), dim3(kSsThreads), smem, (hipStream_t)stream, bounds, V, S, Spad,
                  seed, max_tries, ids, num_tries, log_q);
  return OS2S_OK;
}

extern "C" int os2s_sampled_softmax_gather(os2s_stream_t stream, const int32_t* ids, const float* log_q,
                                           const uint16_t* table, const float* bias, int V, int S, int D,
                                           uint16_t* w_s, float* b_s) {
  OS2S_REQUIRE(ids && log_q && table && w_s && b_s && D >= 8 && D % 8 == 0);
  if (V < 2 || V > (1 << 20) || S < 1 || S > V / 2) return OS2S_ERR_UNSUPPORTED;
  const int Spad = (S + 7) / 8 * 8;
  OS2S_LAUNCH(ss_gather_kernel, dim3(ss_blocks((long long)Spad * (D / 8))), dim3(kSsThreads), 0,
              (hipStream_t)stream, ids, log_q, table, bias, V, Spad, D, w_s, b_s);
  return OS2S_OK;
}

extern "C" int os2s_sampled_softmax_loss(os2s_stream_t stream, const uint16_t* x, long long ldx,
                                         const uint16_t* table, const float* bias, const int32_t* labels,
                                         const int32_t* ids, const int32_t* num_tries, long long N, int V, int S,
                                         int D, uint16_t* logits, long long ld, float grad_scale,
                                         const float* grad_scale_dev, int want_grad, float* row_loss, float* loss,
                                         float* dtrue) {
  OS2S_REQUIRE(x && table && labels && ids && num_tries && logits && row_loss && N >= 1);
  OS2S_REQUIRE(D >= 8 && D % 8 == 0 && ldx >= D && ldx % 8 == 0 && ld % 8 == 0);
  OS2S_REQUIRE(!want_grad || dtrue);
  if (V < 2 || V > (1 << 20) || S < 1 || S > V / 2) return OS2S_ERR_UNSUPPORTED;
  const int Spad = (S + 7) / 8 * 8;
  OS2S_REQUIRE(ld >= Spad && N <= 0x7fffffffLL);
  OS2S_LAUNCH(ss_loss_kernel, dim3((unsigned)N), dim3(kSsThreads), 0, (hipStream_t)stream, x, ldx, table, bias,
              labels, ids, num_tries, V, S, Spad, D, logits, ld, grad_scale, grad_scale_dev, want_grad, row_loss,
              dtrue);
  if (loss) {
    OS2S_LAUNCH(ss_sum_rows_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_loss, N, grad_scale, loss);
  }
  return OS2S_OK;
}

extern "C" int os2s_sampled_softmax_scatter(os2s_stream_t stream, const int32_t* ids, const float* dw_s,
                                            const float* db_s, int V, int S, int D, float* dtable, float* dbias) {
  OS2S_REQUIRE(ids && dw_s && dtable && D >= 8 && D % 8 == 0);
  if (V < 2 || V > (1 << 20) || S < 1 || S > V / 2) return OS2S_ERR_UNSUPPORTED;
  OS2S_LAUNCH(ss_scatter_kernel, dim3(ss_blocks((long long)S * (D / 4))), dim3(kSsThreads), 0,
              (hipStream_t)stream, ids, dw_s, db_s, V, S, D, dtable, dbias);
  return OS2S_OK;
}

extern "C" int os2s_sampled_softmax_true_bwd(os2s_stream_t stream, const uint16_t* x, long long ldx,
                                             const uint16_t* table, const int32_t* labels, const float* dtrue,
                                             long long N, int V, int D, uint16_t* dx, long long lddx,
                                             float* dtable, float* dbias) {
  OS2S_REQUIRE(x && table && labels && dtrue && dtable && N >= 1 && N <= 0x7fffffffLL && V >= 2);
  OS2S_REQUIRE(D >= 8 && D % 8 == 0 && ldx >= D && ldx % 8 == 0 && (!dx || (lddx >= D && lddx % 8 == 0)));
  if (os2s_deterministic()) {
    OS2S_LAUNCH(ss_true_bwd_det_kernel, dim3(ceil_div(D / 8 + 1, kSsThreads)), dim3(kSsThreads), 0,
                (hipStream_t)stream, x, ldx, table, labels, dtrue, N, V, D, dx, lddx, dtable, dbias);
    return OS2S_OK;
  }
  OS2S_LAUNCH(ss_true_bwd_kernel, dim3((unsigned)N), dim3(kSsThreads), 0, (hipStream_t)stream, x, ldx, table,
              labels, dtrue, V, D, dx, lddx, dtable, dbias);
  return OS2S_OK;
}
