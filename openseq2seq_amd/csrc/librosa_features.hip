// The 'mfcc' and 'spectrogram' features of the librosa backend, gfx950 (get_speech_features_librosa,
// open_seq2seq/data/speech2text/speech_utils.py:354-417). Its 'logfbank' features are the tuned FFT path in
// logmel.hip, which also owns the max |x| pass used here. Neither is on a benchmarked path: one workgroup per
// frame, a direct real DFT of the frame against a twiddle table in LDS (the 'spectrogram' transform length is
// n_fft = win_length = int(sr * window_size) — 320 points at the defaults, not a power of two, and zero-padding
// would move the bins), one thread per bin, everything after the fp32 sample arithmetic in fp64.
//
//   'spectrogram' (:367-381): gain -> dither -> stft(n_fft = win_length, centred reflect padding, window_fn) ->
//       |.|^2, values <= 1e-30 raised to 1e-30 -> 10 log10 -> the first F bins. No pre-emphasis.
//   'mfcc' (:383-395): gain -> dither -> pre-emphasis 0.97 -> stft(n_fft, win_length) -> S = |.|^2 ->
//       librosa.feature.mfcc(sr, S = S, n_mfcc = F, n_mels = 2F). librosa uses a given S AS IT STANDS: the mel
//       filter bank and power_to_db run only when S is None, and n_mels is ignored. The reference therefore
//       computes  dct(S, axis = 0, type = 2, norm = 'ortho')[:F]  — the orthonormal DCT-II along the n_fft / 2 + 1
//       LINEAR frequency bins of the POWER spectrum, with no mel scale and no logarithm — and so does this kernel
//       (dct: the host's [F][n_fft / 2 + 1] table). A drop-in reproduces what the reference computes, not what
//       the name suggests.
// Both end as the 'logfbank' path does (:411-417): per-feature (norm_per_feature) or global mean / std over the
// utterance's frames, each replaced by features_mean / features_std_dev when the configuration gives them.
// The gain, the dither and the pre-emphasis are float32 operations in the reference too (it normalises
// signal.astype(np.float32)); they are done here with the same roundings, so with dither = 0 the transform's
// input is the reference's bit for bit.
#include "speech_frontend.hpp"

namespace os2s {

struct SpecArgs {
  const void* signal;      // [B, Nmax] float32 or int16
  const int32_t* n_samples;
  int sample_is_int16;
  int B;
  long long Nmax;
  int n_fft, win_length, hop, F;
  int mfcc;                // 1: pre-emphasis + DCT projection of the power spectrum; 0: 10 log10 of the first F bins
  const double* window;    // [n_fft]: window_fn(win_length), centred, zero padded
  const double* dct;       // [F][n_fft / 2 + 1] (mfcc)
  float preemph, dither, fixed_gain;
  unsigned long long seed;
  const float* absmax;     // [B]
  double* plane;           // [B, Tmax, F] features before the normalisation
  int Tmax;
};

__global__ __launch_bounds__(256) void spec_frames_kernel(SpecArgs p) {
  extern __shared__ __attribute__((aligned(16))) double lds_spec[];
  const int n_fft = p.n_fft, nbins = n_fft / 2 + 1;
  double* const x = lds_spec;          // [n_fft] windowed frame
  double* const cs = x + n_fft;        // [n_fft]
  double* const sn = cs + n_fft;       // [n_fft]
  double* const ps = sn + n_fft;       // [nbins] power spectrum
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const long long N = min((long long)p.n_samples[b], p.Nmax);      // never past the row
  const int Tb = 1 + (int)(N / p.hop);
  if (t >= Tb || N < 1) return;                                     // (workgroup-uniform)
  const float gain = p.fixed_gain > 0.f ? p.fixed_gain : 1.0f / (p.absmax[b] + 1e-5f);
  auto sample = [&](long long i) -> float {
    float v = load_sample(p.signal, p.sample_is_int16, b * p.Nmax + i) * gain;
    if (p.dither > 0.f) v += p.dither * gauss_noise(p.seed, b, i);
    return v;
  };
  for (int j = tid; j < n_fft; j += 256) {
    const double w = p.window[j];
    double xv = 0.0;
    if (w != 0.0) {
      const long long pidx = (long long)t * p.hop - n_fft / 2 + j;   // index into the reflect-padded signal
      const long long i = reflect_index(pidx, N);  // (clips shorter than n_fft / 2 + 1: undefined in the reference)
      float v = sample(i);
      if (p.mfcc && i > 0) v = __fsub_rn(v, __fmul_rn(p.preemph, sample(i - 1)));
      xv = w * (double)v;
    }
    x[j] = xv;
  }
  fill_twiddles(cs, sn, n_fft);
  __syncthreads();
  const int lo = (n_fft - p.win_length) / 2, hi = lo + p.win_length;   // the window's support
  for (int k = tid; k < nbins; k += 256) {
    double re, im;
    dft_bin(x, cs, sn, lo, hi, k, n_fft, re, im);
    ps[k] = re * re + im * im;
  }
  __syncthreads();
  double* const out = p.plane + ((long long)b * p.Tmax + t) * p.F;
  for (int m = tid; m < p.F; m += 256) {
    double v;
    if (p.mfcc) {
      v = 0.0;
      const double* const d = p.dct + (long long)m * nbins;
      for (int k = 0; k < nbins; ++k) v += d[k] * ps[k];
    } else {
      v = 10.0 * log10(fmax(ps[m], 1e-30));
    }
    out[m] = v;
  }
}

constexpr int kSpecMaxF = 1024;

// mean and 1 / std of one utterance, two passes over its plane in frame order (np.mean, np.std with ddof = 0):
// per feature, or — norm_per_feature = 0 — one pair for the whole utterance (the per-feature sums added in
// feature order). Given statistics replace the computed ones. stats [B][2][F].
__global__ __launch_bounds__(256) void spec_stats_kernel(const double* __restrict__ plane,
                                                         const int32_t* __restrict__ n_samples, long long Nmax, int hop,
                                                         int Tmax, int F, int norm_per_feature,
                                                         const double* __restrict__ given_mean,
                                                         const double* __restrict__ given_std,
                                                         double* __restrict__ stats) {
  __shared__ double red[kSpecMaxF];
  __shared__ double total;
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long N = min((long long)n_samples[b], Nmax);
  const int Tb = min(1 + (int)(N / hop), Tmax);
  const double* const x = plane + (long long)b * Tmax * F;
  for (int f = tid; f < F; f += 256) {
    double s = 0.0;
    for (int t = 0; t < Tb; ++t) s += x[(long long)t * F + f];
    red[f] = s;
  }
  __syncthreads();
  if (tid == 0 && !norm_per_feature) {
    double s = 0.0;
    for (int f = 0; f < F; ++f) s += red[f];
    total = s / ((double)Tb * F);
  }
  __syncthreads();
  double mu[kSpecMaxF / 256];
  for (int f = tid, j = 0; f < F; f += 256, ++j) mu[j] = norm_per_feature ? red[f] / (double)Tb : total;
  __syncthreads();
  for (int f = tid, j = 0; f < F; f += 256, ++j) {
    double s = 0.0;
    for (int t = 0; t < Tb; ++t) {
      const double d = x[(long long)t * F + f] - mu[j];
      s += d * d;
    }
    red[f] = s;
  }
  __syncthreads();
  if (tid == 0 && !norm_per_feature) {
    double s = 0.0;
    for (int f = 0; f < F; ++f) s += red[f];
    total = s / ((double)Tb * F);
  }
  __syncthreads();
  for (int f = tid, j = 0; f < F; f += 256, ++j) {
    const double var = norm_per_feature ? red[f] / (double)Tb : total;
    stats[((long long)b * 2 + 0) * F + f] = given_mean ? given_mean[f] : mu[j];
    stats[((long long)b * 2 + 1) * F + f] = 1.0 / (given_std ? given_std[f] : sqrt(var));
  }
}

__global__ __launch_bounds__(256) void spec_normalize_kernel(const double* __restrict__ plane,
                                                             const double* __restrict__ stats,
                                                             const int32_t* __restrict__ n_samples, long long Nmax,
                                                             int hop, int Tmax, int Tpad, int F,
                                                             bf16_t* __restrict__ out_bf16, float* __restrict__ out_f32,
                                                             int32_t* __restrict__ out_len) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long N = min((long long)n_samples[b], Nmax);
  const int Tb = min(1 + (int)(N / hop), Tmax);
  const long long per = (long long)Tpad * F;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < per; i += (long long)gridDim.x * 256) {
    const int t = (int)(i / F), f = (int)(i - (long long)t * F);
    float v = 0.f;
    if (t < Tb)
      v = (float)((plane[((long long)b * Tmax + t) * F + f] - stats[((long long)b * 2 + 0) * F + f]) *
                  stats[((long long)b * 2 + 1) * F + f]);
    out_bf16[(long long)b * per + i] = f2bf(v);
    if (out_f32) out_f32[(long long)b * per + i] = v;
  }
  if (blockIdx.x == 0 && tid == 0) out_len[b] = Tb;
}

}  // namespace os2s

using namespace os2s;

extern "C" size_t os2s_librosa_features_workspace_bytes(int B, int Tmax, int F) {
  // fp64 plane | max |x| per utterance | mean, 1 / std per utterance and feature
  return (size_t)B * Tmax * F * 8 + ((size_t)B * 4 + 255) / 256 * 256 + (size_t)B * 2 * F * 8 + 256;
}

static int librosa_features(hipStream_t stream, const void* signal, const int32_t* n_samples, int sample_is_int16,
                            int B, long long Nmax, int n_fft, int win_length, int hop, int F, int mfcc,
                            const double* window, const double* dct, float preemph, float dither,
                            unsigned long long seed, float fixed_gain, int norm_per_feature,
                            const double* features_mean, const double* features_std, int Tmax, int Tpad,
                            uint16_t* out_bf16, float* out_f32, int32_t* out_len, void* workspace,
                            size_t workspace_bytes) {
  OS2S_REQUIRE(signal && n_samples && window && out_bf16 && out_len && workspace && (dct || !mfcc));
  OS2S_REQUIRE(B >= 1 && Nmax >= 1 && hop >= 1 && Tmax >= 1 && Tpad >= Tmax && F >= 1);
  OS2S_REQUIRE(n_fft >= 16 && win_length >= 1 && win_length <= n_fft);
  const int nbins = n_fft / 2 + 1;
  const size_t smem = ((size_t)3 * n_fft + nbins) * sizeof(double);
  if (F > kSpecMaxF || smem > 48 * 1024) return OS2S_ERR_UNSUPPORTED;
  if (workspace_bytes < os2s_librosa_features_workspace_bytes(B, Tmax, F)) return OS2S_ERR_WORKSPACE;
  char* w = (char*)workspace;
  double* plane = (double*)w;
  w += (size_t)B * Tmax * F * 8;
  float* absmax = (float*)w;
  w += ((size_t)B * 4 + 255) / 256 * 256;
  double* stats = (double*)w;
  if (fixed_gain <= 0.f) {   // the log-mel path's max |x| pass, over blocks of 32 frames
    const int rc = launch_absmax(stream, signal, n_samples, sample_is_int16, B, Nmax, hop, ceil_div(Tmax, 32), absmax);
    if (rc != OS2S_OK) return rc;
  }
  SpecArgs s;
  s.signal = signal; s.n_samples = n_samples; s.sample_is_int16 = sample_is_int16; s.B = B; s.Nmax = Nmax;
  s.n_fft = n_fft; s.win_length = win_length; s.hop = hop; s.F = F; s.mfcc = mfcc; s.window = window; s.dct = dct;
  s.preemph = preemph; s.dither = dither; s.fixed_gain = fixed_gain; s.seed = seed; s.absmax = absmax;
  s.plane = plane; s.Tmax = Tmax;
  OS2S_LAUNCH(spec_frames_kernel, dim3(Tmax, B), dim3(256), smem, stream, s);
  OS2S_LAUNCH(spec_stats_kernel, dim3(B), dim3(256), 0, stream, plane, n_samples, Nmax, hop, Tmax, F,
              norm_per_feature, features_mean, features_std, stats);
  OS2S_LAUNCH(spec_normalize_kernel, dim3(64, B), dim3(256), 0, stream, plane, stats, n_samples, Nmax, hop, Tmax,
              Tpad, F, out_bf16, out_f32, out_len);
  return OS2S_OK;
}

extern "C" int os2s_librosa_mfcc(os2s_stream_t stream, const void* signal, const int32_t* n_samples,
                                 int sample_is_int16, int B, long long Nmax, int n_fft, int win_length, int hop,
                                 int n_mfcc, const double* window, const double* dct, float preemph, float dither,
                                 unsigned long long seed, float fixed_gain, int norm_per_feature,
                                 const double* features_mean, const double* features_std, int Tmax, int Tpad,
                                 uint16_t* out_bf16, float* out_f32, int32_t* out_len, void* workspace,
                                 size_t workspace_bytes) {
  OS2S_REQUIRE(n_mfcc <= n_fft / 2 + 1);
  return librosa_features((hipStream_t)stream, signal, n_samples, sample_is_int16, B, Nmax, n_fft, win_length, hop,
                          n_mfcc, 1, window, dct, preemph, dither, seed, fixed_gain, norm_per_feature, features_mean,
                          features_std, Tmax, Tpad, out_bf16, out_f32, out_len, workspace, workspace_bytes);
}

extern "C" int os2s_librosa_spectrogram(os2s_stream_t stream, const void* signal, const int32_t* n_samples,
                                        int sample_is_int16, int B, long long Nmax, int n_win, int hop,
                                        int num_features, const double* window, float dither,
                                        unsigned long long seed, float fixed_gain, int norm_per_feature,
                                        const double* features_mean, const double* features_std, int Tmax,
                                        int Tpad, uint16_t* out_bf16, float* out_f32, int32_t* out_len,
                                        void* workspace, size_t workspace_bytes) {
  OS2S_REQUIRE(num_features <= n_win / 2 + 1);      // the reference's assertion (speech_utils.py:377-378)
  return librosa_features((hipStream_t)stream, signal, n_samples, sample_is_int16, B, Nmax, n_win, n_win, hop,
                          num_features, 0, window, nullptr, 0.f, dither, seed, fixed_gain, norm_per_feature,
                          features_mean, features_std, Tmax, Tpad, out_bf16, out_f32, out_len, workspace,
                          workspace_bytes);
}
