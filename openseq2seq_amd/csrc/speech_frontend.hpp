// Shared by the speech feature front ends (logmel.hip, librosa_features.hip, psf_features.hip, tts_features.hip):
// the sample load, the reflect-padded index, the twiddle table and the direct real DFT of a frame, the frame count
// of the python_speech_features paths, the per-frame partial sums, the dither noise, and the host function of the
// max |x| pass that crosses from the log-mel unit to the librosa one.
#pragma once
#include "os2s_common.hpp"
#include <type_traits>

namespace os2s {

// sample `index` of a [B, Nmax] float32 or int16 signal, as float
__device__ __forceinline__ float load_sample(const void* signal, int is_i16, long long index) {
  return is_i16 ? (float)reinterpret_cast<const int16_t*>(signal)[index] : reinterpret_cast<const float*>(signal)[index];
}

// index into an N-sample signal of position p of its reflect-padded extension (np.pad(mode='reflect'):
// ... 2 1 | 0 1 2 ... N-1 | N-2 N-3 ...), one reflection, then clamped into [0, N)
__device__ __forceinline__ long long reflect_index(long long p, long long N) {
  const long long i = p < 0 ? -p : (p >= N ? 2 * (N - 1) - p : p);
  return i < 0 ? 0 : (i >= N ? N - 1 : i);
}

// cs[i] = cos(2 pi i / n), sn[i] = sin(2 pi i / n), strided over the workgroup; the caller owns the barrier
template <typename T>
__device__ __forceinline__ void fill_twiddles(T* cs, T* sn, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    if constexpr (std::is_same<T, float>::value) sincospif(2.0f * (float)i / (float)n, &sn[i], &cs[i]);
    else sincospi(2.0 * (double)i / (double)n, &sn[i], &cs[i]);
  }
}

// bin k of the n-point real DFT of x, re + i im, over the support [lo, hi) of x: summed for i = lo .. hi-1 ascending
// with an incremental phase index (k i mod n) into the twiddle table. k < n, so one compare and subtract wraps it.
template <typename T>
__device__ __forceinline__ void dft_bin(const T* x, const T* cs, const T* sn, int lo, int hi, int k, int n, T& re,
                                        T& im) {
  re = 0;
  im = 0;
  int idx = (int)(((long long)k * lo) % n);
  for (int i = lo; i < hi; ++i) {
    re += x[i] * cs[idx];
    im -= x[i] * sn[idx];
    idx += k;
    if (idx >= n) idx -= n;
  }
}

// frames of an n-sample utterance on the python_speech_features paths: 1 + ceil((n - n_win) / n_step), at least one
// (`live`), and that count rounded up to a multiple of pad_to (`padded`)
struct PsfFrames { int live, padded; };
__host__ __device__ inline PsfFrames psf_frame_count(int n, int n_win, int n_step, int pad_to) {
  const int live = n <= n_win ? 1 : 1 + (n - n_win + n_step - 1) / n_step;
  const int rem = pad_to > 0 ? live % pad_to : 0;
  return {live, rem ? live + pad_to - rem : live};
}

// (sum, sum of squares) of one frame's features, over a workgroup of four waves, into partial_slot[0..1]: wave
// shuffle, one slot per wave, added in a fixed order by thread 0. red: LDS. Every thread of the workgroup calls it.
__device__ __forceinline__ void emit_frame_partial(double s1, double s2, double (*red)[4], double* partial_slot) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
  }
  if ((tid & 63) == 0) { red[0][tid >> 6] = s1; red[1][tid >> 6] = s2; }
  __syncthreads();
  if (tid == 0) {
    partial_slot[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    partial_slot[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// standard normal deviate of (seed, utterance b, sample i): Box-Muller over two counter hashes
__device__ __forceinline__ float gauss_noise(unsigned long long seed, int b, long long i) {
  const uint32_t h1 = hash_u32(seed, ((unsigned long long)b << 40) ^ (unsigned long long)(2 * i));
  const uint32_t h2 = hash_u32(seed, ((unsigned long long)b << 40) ^ (unsigned long long)(2 * i + 1));
  const float u1 = ((float)(h1 >> 8) + 1.0f) * (1.0f / 16777217.0f);
  const float u2 = (float)(h2 >> 8) * (1.0f / 16777216.0f);
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// logmel.hip: absmax[b] = max |x| of utterance b (zeroed first), walked in the log-mel path's units: nblk blocks
// of 32 frames of `hop` samples per utterance, the last one taking the tail.
int launch_absmax(hipStream_t stream, const void* signal, const int32_t* n_samples, int sample_is_int16, int B,
                  long long Nmax, int hop, int nblk, float* absmax);

}  // namespace os2s
