// Training-summary statistics: one multi-tensor pass over a flat fp32 buffer laid out like the optimizer's
// (tensor-aligned chunks of os2s_opt_chunk_elems() elements), for the TensorBoard summaries of
// open_seq2seq/optimizers/optimizers.py:289-330 (tf.norm and tf.summary.histogram of every variable and gradient).
//
// Per selected tensor: min, max, num, sum, sum of squares and the count of non-finite values of v = x * m (fp32
// product, then double), and optionally the counts of TensorFlow's default histogram buckets
// (tensorflow/core/lib/histogram/histogram.cc InitDefaultBucketsInner: 1e-12 * 1.1^k by repeated multiplication,
// mirrored, with 0 and +-DBL_MAX; bucket(v) = std::upper_bound of the limits).
//
// Three launches on one stream:
//   summary_table_kernel    the 774 positive limits into the workspace (a few microseconds; the table is rebuilt by
//                           every call so that calls on different streams share nothing)
//   summary_chunks_kernel   a workgroup per kGroup consecutive chunks: per-chunk, per-wave partials {min, max, num, sum,
//                           sumsq, nonfinite} as doubles, bucket counts in an LDS histogram that is added to the tensor's
//                           global counts (integer atomics) whenever the tensor changes and at the end
//   summary_tensor_kernel   a workgroup per tensor adds the tensor's partials in chunk order: 256 blocks of consecutive
//                           chunks, each summed chunk by chunk (a chunk's four waves in wave order), then the block
//                           totals in block order
// Nothing is accumulated with floating-point atomics: thread -> wave (xor tree) -> the four waves in order -> the
// chunks of a block in order -> the blocks in order is one fixed order, so the doubles are the same bits in every run.
//
// Contention: trained weights and gradients fall into a few dozen adjacent buckets and a constant tensor into one,
// where 64 LDS atomics of a wave on one address are served one after the other. Measured on Jasper's 1.33 GB buffers
// (profiles/summary_step_cost.md) that costs less than avoiding it: one LDS add per lane takes 1.01 ms on weights or
// gradients and 1.35 ms on a constant buffer; combining the lanes that share the index of the wave's first valid lane
// into ONE add of their count first (two ballots and a popcount per element row) takes 1.36 ms and 0.91 ms. The
// per-lane add is the default; OS2S_SUMMARY_COMBINE_LANES in `flags` selects the other form (same counts).
// A workgroup has no barrier per chunk: every wave leaves its own partial of its quarter of the chunk, and the next
// chunk's loads are issued before the current chunk's arithmetic.
#include <float.h>

#include "os2s_common.hpp"

namespace os2s {

constexpr int kSumChunk = 4096;        // == os2s_opt_chunk_elems() (checked by the entry point)
constexpr int kGroup = 8;              // chunks per workgroup
constexpr int kPos = 774;              // positive finite limits
constexpr int kBuckets = 2 * kPos + 3; // 1551
constexpr int kZeroBucket = kPos + 2;  // 776: first limit > 0 is limits[776] = 1e-12
constexpr int kStatFields = 6;

constexpr int kWaves = 4;              // waves of a workgroup: partials per chunk

__global__ void summary_table_kernel(double* __restrict__ pos) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double v = 1e-12;
  for (int i = 0; i < kPos; ++i) {
    pos[i] = v;
    v *= 1.1;
  }
}

// number of table entries <= a (a > 0 finite): the logf guess corrected against the table, so the index is exact
__device__ __forceinline__ int count_limits_le(const double* pos, float af) {
  const double a = (double)af;
  if (af < 1e-12f) return 0;         // (float(1e-12) < 1e-12: below the first limit, denormals included)
  // log2(1e-12) = -39.863137..., 1 / log2(1.1) = 7.272540...
  int g = (int)((__log2f(af) + 39.8631371f) * 7.2725409f) + 1;
  g = g < 0 ? 0 : (g > kPos ? kPos : g);
  while (g < kPos && pos[g] <= a) ++g;
  while (g > 0 && pos[g - 1] > a) --g;
  return g;
}

__device__ __forceinline__ int bucket_of(const double* pos, float v) {
  const float a = fabsf(v);
  if (!(a > 0.f)) return kZeroBucket;                       // +0 and -0
  if (v > 0.f) return kZeroBucket + count_limits_le(pos, a);  // limits[776 + k] = pos[k]
  // v < 0: limits[i] = -pos[774 - i] for i in 1..774; the first one > v is i = 775 - #{pos < a}
  const double ad = (double)a;
  int k = count_limits_le(pos, a);
  while (k > 0 && pos[k - 1] == ad) --k;                    // (strictly smaller; never taken for an fp32 value)
  return kZeroBucket - 1 - k;
}

template <bool HIST, bool COMBINE>
__global__ __launch_bounds__(256) void summary_chunks_kernel(
    const float* __restrict__ buf, const int32_t* __restrict__ chunk_tensor,
    const int32_t* __restrict__ tensor_chunk_begin, const long long* __restrict__ tensor_count,
    const uint8_t* __restrict__ tensor_select, float host_mult, const float* __restrict__ dev_mult,
    int mask_nonfinite, int nchunks, const double* __restrict__ pos_table, double* __restrict__ partial,
    uint32_t* __restrict__ hist) {
  __shared__ double s_pos[HIST ? kPos : 1];
  __shared__ uint32_t s_hist[HIST ? kBuckets : 1];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float m = dev_mult ? host_mult * dev_mult[0] : host_mult;
  if (HIST) {
    for (int i = tid; i < kPos; i += 256) s_pos[i] = pos_table[i];
    for (int i = tid; i < kBuckets; i += 256) s_hist[i] = 0u;
    __syncthreads();
  }
  const int c_begin = blockIdx.x * kGroup;
  const int c_end = c_begin + kGroup < nchunks ? c_begin + kGroup : nchunks;
  int hist_t = -1;                       // tensor whose counts s_hist holds (uniform)
  f32x4 x[4], nx[4];
  {
    const f32x4* p4 = reinterpret_cast<const f32x4*>(buf + (long long)c_begin * kSumChunk);
#pragma unroll
    for (int i = 0; i < 4; ++i) nx[i] = p4[i * 256 + tid];
  }
  for (int c = c_begin; c < c_end; ++c) {
    const int t = chunk_tensor[c];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = nx[i];
    if (c + 1 < c_end) {                 // the next chunk's loads are in flight during this chunk's arithmetic
      const f32x4* n4 = reinterpret_cast<const f32x4*>(buf + (long long)(c + 1) * kSumChunk);
#pragma unroll
      for (int i = 0; i < 4; ++i) nx[i] = n4[i * 256 + tid];
    }
    if (HIST && hist_t >= 0 && t != hist_t) {
      __syncthreads();
      for (int i = tid; i < kBuckets; i += 256) {
        const uint32_t n = s_hist[i];
        if (n) { atomicAdd(hist + (long long)hist_t * kBuckets + i, n); s_hist[i] = 0u; }
      }
      __syncthreads();
      hist_t = -1;
    }
    if (!tensor_select[t]) continue;
    const int c0 = tensor_chunk_begin[t], c1 = tensor_chunk_begin[t + 1];
    long long cnt = tensor_count[t];
    const long long span = (long long)(c1 - c0) * kSumChunk;
    cnt = cnt < 0 ? 0 : (cnt > span ? span : cnt);      // never past the tensor's own chunks
    const long long left = cnt - (long long)(c - c0) * kSumChunk;   // logical elements from this chunk on
    double sum = 0.0, sq = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    int num = 0, nf = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long idx = (long long)(i * 256 + tid) * 4 + e;
        bool valid = idx < left;
        float v = x[i][e] * m;
        const bool finite = (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
        if (!finite) {
          if (mask_nonfinite) {
            v = 0.f;
          } else {
            nf += valid ? 1 : 0;
            valid = false;
          }
        }
        if (valid) {
          const double d = (double)v;
          sum += d;
          sq += d * d;
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
          ++num;
        }
        if (HIST) {
          const int b = valid ? bucket_of(s_pos, v) : 0;
          if (COMBINE) {
            const unsigned long long act = __ballot(valid);
            if (act) {
              const int first = __ffsll((long long)act) - 1;
              const int lead = __builtin_amdgcn_readlane(b, first);    // (`first` is wave-uniform: no LDS permute)
              const unsigned long long same = __ballot(valid && b == lead);
              if (lane == first) atomicAdd(&s_hist[lead], (uint32_t)__popcll(same));
              else if (valid && b != lead) atomicAdd(&s_hist[b], 1u);
            }
          } else {
            if (valid) atomicAdd(&s_hist[b], 1u);
          }
        }
      }
    }
    if (HIST) hist_t = t;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o, 64);
      sq += __shfl_xor(sq, o, 64);
      mn = fminf(mn, __shfl_xor(mn, o, 64));
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      num += __shfl_xor(num, o, 64);
      nf += __shfl_xor(nf, o, 64);
    }
    if (lane == 0) {
      double* o = partial + ((long long)c * kWaves + wid) * kStatFields;
      o[0] = num ? (double)mn : DBL_MAX;
      o[1] = num ? (double)mx : -DBL_MAX;
      o[2] = (double)num; o[3] = sum; o[4] = sq; o[5] = (double)nf;
    }
  }
  if (HIST && hist_t >= 0) {
    __syncthreads();
    for (int i = tid; i < kBuckets; i += 256) {
      const uint32_t n = s_hist[i];
      if (n) atomicAdd(hist + (long long)hist_t * kBuckets + i, n);
    }
  }
}

// one workgroup per selected tensor: zero its bucket counts before the chunks add to them
__global__ __launch_bounds__(256) void summary_zero_hist_kernel(const uint8_t* __restrict__ tensor_select,
                                                                uint32_t* __restrict__ hist) {
  const int t = blockIdx.x;
  if (!tensor_select[t]) return;
  for (int i = threadIdx.x; i < kBuckets; i += 256) hist[(long long)t * kBuckets + i] = 0u;
}

// One workgroup per tensor, in two fixed stages: thread j adds up the partials of the j-th block of consecutive chunks
// IN CHUNK ORDER (the four waves of a chunk in wave order), then thread 0 adds the 256 block totals in block order.
// (One wave walking all chunks of Jasper's largest kernels one by one took longer than the pass over the data.)
__global__ __launch_bounds__(256) void summary_tensor_kernel(const double* __restrict__ partial,
                                                             const int32_t* __restrict__ tensor_chunk_begin,
                                                             const uint8_t* __restrict__ tensor_select,
                                                             double* __restrict__ stats) {
  __shared__ double s_part[256][kStatFields];
  const int t = blockIdx.x;
  if (!tensor_select[t]) return;
  const int c0 = tensor_chunk_begin[t], c1 = tensor_chunk_begin[t + 1];
  const int per = (c1 - c0 + 255) / 256;
  const int b0 = c0 + (int)threadIdx.x * per;
  const int b1 = b0 + per < c1 ? b0 + per : c1;
  double v[kStatFields] = {DBL_MAX, -DBL_MAX, 0.0, 0.0, 0.0, 0.0};
  for (int c = b0; c < b1; ++c) {
    for (int w = 0; w < kWaves; ++w) {
      const double* q = partial + ((long long)c * kWaves + w) * kStatFields;
      v[0] = fmin(v[0], q[0]); v[1] = fmax(v[1], q[1]);
#pragma unroll
      for (int k = 2; k < kStatFields; ++k) v[k] += q[k];
    }
  }
#pragma unroll
  for (int k = 0; k < kStatFields; ++k) s_part[threadIdx.x][k] = v[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nblocks = per > 0 ? (c1 - c0 + per - 1) / per : 0;
    for (int j = 1; j < nblocks; ++j) {
      v[0] = fmin(v[0], s_part[j][0]); v[1] = fmax(v[1], s_part[j][1]);
#pragma unroll
      for (int k = 2; k < kStatFields; ++k) v[k] += s_part[j][k];
    }
    double* o = stats + (long long)t * kStatFields;
#pragma unroll
    for (int k = 0; k < kStatFields; ++k) o[k] = v[k];
  }
}

// One thread: the multipliers of the gradient summaries. out[0] = 1 / (loss_scale * world_size); out[1] = out[0] *
// clip * min(1 / norm, 1 / clip) with norm = sqrt(sum of the selected tensors' sum_squares) — NaN as soon as one of
// them holds a non-finite value, as tf.global_norm would be — or out[0] when clip <= 0 or stats is NULL.
__global__ void summary_grad_mult_kernel(const float* __restrict__ loss_scale, int world_size, float clip,
                                         const double* __restrict__ stats, const uint8_t* __restrict__ tensor_select,
                                         int ntensors, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float scale = loss_scale ? loss_scale[0] : 1.f;
  const float inv = 1.f / (scale * (float)world_size);
  float f = 1.f;
  if (clip > 0.f && stats) {
    double s = 0.0, bad = 0.0;
    for (int t = 0; t < ntensors; ++t) {
      if (tensor_select && !tensor_select[t]) continue;
      s += stats[(long long)t * kStatFields + 4];
      bad += stats[(long long)t * kStatFields + 5];
    }
    const float norm = bad > 0.0 ? __builtin_nanf("") : (float)sqrt(s);
    f = clip * fminf(1.f / norm, 1.f / clip);
    if (!(norm == norm)) f = norm;        // (fminf drops a NaN)
  }
  out[0] = inv;
  out[1] = inv * f;
}

}  // namespace os2s

using namespace os2s;

extern "C" int os2s_summary_num_buckets(void) { return kBuckets; }

extern "C" size_t os2s_summary_stats_workspace_bytes(int nchunks) {
  if (nchunks < 0) return 0;
  return ((size_t)kPos + 2 + (size_t)nchunks * kWaves * kStatFields) * sizeof(double);
}

extern "C" int os2s_summary_stats(os2s_stream_t stream_, const float* buf, int nchunks, int ntensors,
                                  const int32_t* chunk_tensor, const int32_t* tensor_chunk_begin,
                                  const long long* tensor_count, long long max_count, const uint8_t* tensor_select,
                                  float host_mult, const float* dev_mult, int flags, double* stats,
                                  uint32_t* hist, void* workspace, size_t workspace_bytes) {
  OS2S_REQUIRE(buf && chunk_tensor && tensor_chunk_begin && tensor_count && tensor_select && stats && workspace);
  OS2S_REQUIRE(nchunks >= 1 && ntensors >= 1 && max_count >= 0);
  OS2S_REQUIRE((flags & ~(OS2S_SUMMARY_MASK_NONFINITE | OS2S_SUMMARY_COMBINE_LANES)) == 0);
  const int mask_nonfinite = (flags & OS2S_SUMMARY_MASK_NONFINITE) ? 1 : 0;
  OS2S_REQUIRE(os2s_opt_chunk_elems() == kSumChunk);
  OS2S_REQUIRE(workspace_bytes >= os2s_summary_stats_workspace_bytes(nchunks));
  OS2S_REQUIRE((reinterpret_cast<uintptr_t>(buf) % 16) == 0 && (reinterpret_cast<uintptr_t>(workspace) % 8) == 0);
  // bucket counts are 32-bit
  if (hist) OS2S_REQUIRE(max_count < (1ll << 32));
  hipStream_t stream = (hipStream_t)stream_;
  double* pos = (double*)workspace;
  double* partial = pos + kPos + 2;
  const int nblocks = (nchunks + kGroup - 1) / kGroup;
  if (hist) {
    OS2S_LAUNCH(summary_table_kernel, dim3(1), dim3(64), 0, stream, pos);
    OS2S_LAUNCH(summary_zero_hist_kernel, dim3(ntensors), dim3(256), 0, stream, tensor_select, hist);
    if (flags & OS2S_SUMMARY_COMBINE_LANES)
      OS2S_LAUNCH((summary_chunks_kernel<true, true>), dim3(nblocks), dim3(256), 0, stream, buf, chunk_tensor,
                  tensor_chunk_begin, tensor_count, tensor_select, host_mult, dev_mult, mask_nonfinite, nchunks,
                  (const double*)pos, partial, hist);
    else
      OS2S_LAUNCH((summary_chunks_kernel<true, false>), dim3(nblocks), dim3(256), 0, stream, buf, chunk_tensor,
                  tensor_chunk_begin, tensor_count, tensor_select, host_mult, dev_mult, mask_nonfinite, nchunks,
                  (const double*)pos, partial, hist);
  } else {
    OS2S_LAUNCH((summary_chunks_kernel<false, false>), dim3(nblocks), dim3(256), 0, stream, buf, chunk_tensor,
                tensor_chunk_begin, tensor_count, tensor_select, host_mult, dev_mult, mask_nonfinite, nchunks,
                (const double*)pos, partial, hist);
  }
  OS2S_LAUNCH(summary_tensor_kernel, dim3(ntensors), dim3(256), 0, stream, (const double*)partial,
              tensor_chunk_begin, tensor_select, stats);
  return OS2S_OK;
}

extern "C" int os2s_summary_grad_mult(os2s_stream_t stream, const float* loss_scale, int world_size, float clip,
                                      const double* stats, const uint8_t* tensor_select, int ntensors, float* out) {
  OS2S_REQUIRE(out && world_size >= 1 && ntensors >= 0);
  OS2S_LAUNCH(summary_grad_mult_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, loss_scale, world_size, clip, stats,
              tensor_select, ntensors, out);
  return OS2S_OK;
}
