// 'spectrogram' features of the python_speech_features backend (the DeepSpeech2 configs:
// input_type 'spectrogram', 160 bins of a 320-point spectrum), gfx950 — the per-utterance
// arithmetic of get_speech_features_psf (open_seq2seq/data/speech2text/speech_utils.py:444-535):
//   s16 = int16(trunc(x / (max|x| + 1e-5) * 32767))                 (normalize_signal, :216-222)
//   frames of n_win samples every n_step, zero-padded tail, SYMMETRIC Hann (np.hanning)
//   lps = 10 log10(max(|rfft(frame, n_win)|^2 / n_win, 1e-30)) [- max over the utterance]
//   features = (lps[:, :F] - mean) / std over the whole utterance, frames rounded up to pad_to
// The global-max term of logpowspec(norm=1) shifts every value of the utterance by the same
// constant and cancels in the mean / std normalisation: it is not computed. The zero frames added
// to reach a multiple of pad_to (-300 dB rows) DO enter mean and std, as in the reference.
// n_win = 320 is not a power of two: direct real DFT in fp32 with the twiddles in LDS, one
// workgroup per frame, one thread per bin (a data-layer op: ~51 k MAC per frame).
#include "speech_frontend.hpp"

namespace os2s {

__global__ __launch_bounds__(256) void psf_absmax_kernel(const void* __restrict__ signal, int is_i16,
                                                        long long sig_stride,
                                                        const int32_t* __restrict__ n_samples,
                                                        float* __restrict__ gain) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const int n = (int)min((long long)n_samples[b], sig_stride);   // never past the row (as logmel.hip)
  float m = 0.f;
  for (int i = threadIdx.x; i < n; i += 256)
    m = fmaxf(m, fabsf(load_sample(signal, is_i16, (long long)b * sig_stride + i)));
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) gain[b] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) + 1e-5f;
}

// s16 of the header: sample `index` over d = max|x| + 1e-5, times 32767, astype(np.int16) (toward zero)
__device__ __forceinline__ float psf_s16(const void* signal, int is_i16, long long index, float d) {
  return truncf((load_sample(signal, is_i16, index) / d) * 32767.0f);
}

// What both frame kernels open with: frame 0 publishes the utterance's frame count (pad_to rounding included), and
// a frame past that count writes zero partials and is done (false).
__device__ __forceinline__ bool psf_frame_begin(const PsfFrames& fc, int b, int t, int32_t* frames_out, double* slot) {
  if (t == 0 && threadIdx.x == 0) frames_out[b] = fc.padded;
  if (t < fc.padded) return true;
  if (threadIdx.x == 0) slot[0] = slot[1] = 0.0;
  return false;
}

// frames_out[b] = frames of utterance b incl. the pad_to rounding; plane[b, t, :] = lps; per-frame
// partial (sum, sum^2) of the F kept bins for the utterance statistics
__global__ __launch_bounds__(256) void psf_logpowspec_kernel(
    const void* __restrict__ signal, int is_i16, long long sig_stride, const int32_t* __restrict__ n_samples,
    const float* __restrict__ denom, int n_win, int n_step, int pad_to, int F, int T,
    float* __restrict__ plane, double* __restrict__ partial, int32_t* __restrict__ frames_out) {
  extern __shared__ float sm[];
  float* x = sm;                 // [n_win] windowed frame
  float* cs = sm + n_win;        // [n_win]
  float* sn = sm + 2 * n_win;    // [n_win]
  __shared__ double red[2][4];
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int n = (int)min((long long)n_samples[b], sig_stride);   // never past the row
  double* const slot = partial + ((long long)b * T + t) * 2;
  if (!psf_frame_begin(psf_frame_count(n, n_win, n_step, pad_to), b, t, frames_out, slot)) return;
  const float d = denom[b];
  for (int i = tid; i < n_win; i += 256) {
    const long long j = (long long)t * n_step + i;
    const float v = j < n ? psf_s16(signal, is_i16, (long long)b * sig_stride + j, d) : 0.f;
    // np.hanning(M)[i] = 0.5 - 0.5 cos(2 pi i / (M - 1))
    const float w = 0.5f - 0.5f * cospif(2.0f * (float)i / (float)(n_win - 1));
    x[i] = v * w;
  }
  fill_twiddles(cs, sn, n_win);
  __syncthreads();
  double s1 = 0.0, s2 = 0.0;
  for (int k = tid; k < F; k += 256) {
    float re, im;
    dft_bin(x, cs, sn, 0, n_win, k, n_win, re, im);
    const float ps = fmaxf((re * re + im * im) / (float)n_win, 1e-30f);
    const float lps = 10.0f * log10f(ps);
    plane[((long long)b * T + t) * F + k] = lps;
    s1 += (double)lps;
    s2 += (double)lps * (double)lps;
  }
  emit_frame_partial(s1, s2, red, slot);
}

// mean / std over the utterance (fixed summation order), then (x - mean) / std -> bf16 (+ fp32)
__global__ __launch_bounds__(256) void psf_normalize_kernel(const float* __restrict__ plane,
                                                           const double* __restrict__ partial,
                                                           const int32_t* __restrict__ frames_out, int F,
                                                           int T, bf16_t* __restrict__ out16,
                                                           float* __restrict__ out32) {
  __shared__ double sh[2];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int frames = frames_out[b];
  if (tid == 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int t = 0; t < frames; ++t) { s1 += partial[((long long)b * T + t) * 2]; s2 += partial[((long long)b * T + t) * 2 + 1]; }
    const double cnt = (double)frames * F;
    const double mean = s1 / cnt;
    const double var = fmax(s2 / cnt - mean * mean, 0.0);
    sh[0] = mean;
    sh[1] = 1.0 / sqrt(var);
  }
  __syncthreads();
  const float mean = (float)sh[0], rstd = (float)sh[1];
  const long long per = (long long)T * F;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < per; i += (long long)gridDim.x * 256) {
    const int t = (int)(i / F);
    const float v = t < frames ? (plane[(long long)b * per + i] - mean) * rstd : 0.f;
    out16[(long long)b * per + i] = f2bf(v);
    if (out32) out32[(long long)b * per + i] = v;
  }
}

// 'logfbank' features of the python_speech_features backend (the toy Wave2Letter / residual-TDNN test
// configurations of the reference: backend psf by default, input_type 'logfbank', 40 filters) —
// get_speech_features_psf (speech_utils.py:517-535) -> psf.logfbank(signal, samplerate, winlen, winstep,
// nfilt, nfft = 512, lowfreq = 0, highfreq = sr / 2, preemph = 0.97) of python_speech_features 0.6:
//   s16 as above, zero-padded to the pad_to frame count;  y[j] = s16[j] - 0.97 s16[j-1]  (y[0] = s16[0]; the
//   first padding sample is -0.97 s16[n-1], not zero)
//   frames of n_win samples every n_step, RECTANGULAR window, zero-padded to nfft
//   pspec = |rfft(frame, nfft)|^2 / nfft;  feat = pspec . fb^T  (fb: triangular HTK-mel filters, host table
//   [nfilt][nfft/2 + 1]);  feat == 0 -> 2.220446e-16 (numpy double eps);  features = ln(feat)
//   then (features - mean) / std over the whole utterance, pad frames included (ln(eps) rows)
// One workgroup per frame: direct real DFT of the n_win live samples against a 512-entry twiddle table in
// LDS (nfft = 512 has a fast transform, but this is a data-layer op of ~82 k MAC per frame), power spectrum
// in LDS, one thread per filter.
//
// MFCC = true: the 'mfcc' features of the same backend (speech_utils.py:504-515 -> psf.mfcc(numcep = F,
// nfilt = 2F, nfft = 512, lowfreq = 0, highfreq = sr / 2, preemph = 0.97, ceplifter = 2F, appendEnergy = False),
// rectangular window): the nfilt log energies of the frame stay in LDS and one thread per coefficient applies
// the host table dctl [ncep][nfilt] = lifter(m) * orthonormal DCT-II(m, j); the plane holds the ncep cepstra.
// A pad_to frame has ln(eps) in every filter: its cepstrum is a constant c0 and (rounding aside) zeros.
template <bool MFCC>
__global__ __launch_bounds__(256) void psf_logfbank_kernel(
    const void* __restrict__ signal, int is_i16, long long sig_stride, const int32_t* __restrict__ n_samples,
    const float* __restrict__ denom, int n_win, int n_step, int pad_to, int nfilt, int nfft,
    const float* __restrict__ fb, const float* __restrict__ dctl, int ncep, int T, float* __restrict__ plane,
    double* __restrict__ partial, int32_t* __restrict__ frames_out) {
  extern __shared__ float sm[];
  float* x = sm;                 // [n_win] pre-emphasised frame
  float* cs = sm + n_win;        // [nfft]
  float* sn = cs + nfft;         // [nfft]
  float* ps = sn + nfft;         // [nfft / 2 + 1]
  float* le = ps + nfft / 2 + 1; // [nfilt] log filterbank energies (MFCC only)
  __shared__ double red[2][4];
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int nbins = nfft / 2 + 1;
  const int n = (int)min((long long)n_samples[b], sig_stride);
  const PsfFrames fc = psf_frame_count(n, n_win, n_step, pad_to);
  double* const slot = partial + ((long long)b * T + t) * 2;
  if (!psf_frame_begin(fc, b, t, frames_out, slot)) return;
  const float d = denom[b];
  auto s16 = [&](long long j) -> float {
    return j < 0 || j >= n ? 0.f : psf_s16(signal, is_i16, (long long)b * sig_stride + j, d);
  };
  // the reference pads the SIGNAL (by whole strides, to the pad_to frame count) before psf.logfbank runs its
  // pre-emphasis over it; framesig then zero-pads the pre-emphasised signal to complete the last frame. So
  // y[n] = -0.97 s16[n-1] exists only when that signal padding happened (plen > n), and y[j] = 0 past plen.
  // (python: 1 + int(ceil((n - n_win) / n_step)) is <= 1 for n <= n_win: ceil of a non-positive quotient;
  // for n < n_win - n_step it is <= 0 — such clips (< 10 ms) do not occur: frames >= 1 is kept)
  const long long plen = (long long)n + (long long)(fc.padded - fc.live) * n_step;
  for (int i = tid; i < n_win; i += 256) {
    const long long j = (long long)t * n_step + i;
    x[i] = j >= plen ? 0.f : (j == 0 ? s16(0) : s16(j) - 0.97f * s16(j - 1));
  }
  fill_twiddles(cs, sn, nfft);
  __syncthreads();
  for (int k = tid; k < nbins; k += 256) {
    float re, im;
    dft_bin(x, cs, sn, 0, n_win, k, nfft, re, im);
    ps[k] = (re * re + im * im) / (float)nfft;
  }
  __syncthreads();
  double s1 = 0.0, s2 = 0.0;
  for (int m = tid; m < nfilt; m += 256) {
    float e = 0.f;
    const float* const f = fb + (long long)m * nbins;
    for (int k = 0; k < nbins; ++k) e += ps[k] * f[k];
    const float v = logf(e == 0.f ? 2.220446049250313e-16f : e);
    if (MFCC) {
      le[m] = v;
    } else {
      plane[((long long)b * T + t) * nfilt + m] = v;
      s1 += (double)v;
      s2 += (double)v * (double)v;
    }
  }
  if (MFCC) {
    __syncthreads();
    for (int m = tid; m < ncep; m += 256) {
      float c = 0.f;
      const float* const d = dctl + (long long)m * nfilt;
      for (int j = 0; j < nfilt; ++j) c += le[j] * d[j];
      plane[((long long)b * T + t) * ncep + m] = c;
      s1 += (double)c;
      s2 += (double)c * (double)c;
    }
  }
  emit_frame_partial(s1, s2, red, slot);
}

}  // namespace os2s

using namespace os2s;

extern "C" size_t os2s_psf_spectrogram_workspace_bytes(int B, int T, int F) {
  return (size_t)B * 4 + (size_t)B * T * F * 4 + (size_t)B * T * 2 * 8 + 64;
}

// The three feature types of the psf backend share everything but the frame kernel: max |x| -> frames (plane of
// F features per frame + per-frame partial sums) -> utterance mean / std and store. Workspace: denom | partial | plane.
enum PsfMode { kPsfSpectrogram, kPsfLogfbank, kPsfMfcc };

static int psf_features(os2s_stream_t stream_, PsfMode mode, const void* signal, int sample_is_int16,
                        const int32_t* n_samples, int B, long long Nmax, int n_win, int n_step, int pad_to, int F,
                        int nfilt, int nfft, const float* fb, const float* dctl, int Tpad, uint16_t* out_bf16,
                        float* out_f32, int32_t* out_len, void* workspace, size_t workspace_bytes) {
  OS2S_REQUIRE(signal && n_samples && out_bf16 && out_len && workspace);
  OS2S_REQUIRE(B >= 1 && n_win >= 16 && n_step >= 1 && Tpad >= 1 && F >= 1);
  if (mode != kPsfSpectrogram) OS2S_REQUIRE(fb && nfilt >= 1 && nfilt <= 4096 && nfft >= n_win && (nfft & (nfft - 1)) == 0);
  if (workspace_bytes < os2s_psf_spectrogram_workspace_bytes(B, Tpad, F)) return OS2S_ERR_WORKSPACE;
  const size_t lds = sizeof(float) * (mode == kPsfSpectrogram ? (size_t)3 * n_win
                                      : (size_t)n_win + 2 * (size_t)nfft + nfft / 2 + 1 + (mode == kPsfMfcc ? nfilt : 0));
  if (lds > 48 * 1024) return OS2S_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = reinterpret_cast<char*>(workspace);
  float* denom = reinterpret_cast<float*>(ws);
  size_t off = ((size_t)B * 4 + 63) / 64 * 64;
  double* partial = reinterpret_cast<double*>(ws + off);
  off += (size_t)B * Tpad * 2 * 8;
  float* plane = reinterpret_cast<float*>(ws + off);
  OS2S_LAUNCH(psf_absmax_kernel, dim3(B), dim3(256), 0, stream, signal, sample_is_int16, Nmax, n_samples, denom);
  if (mode == kPsfSpectrogram)
    OS2S_LAUNCH(psf_logpowspec_kernel, dim3(Tpad, B), dim3(256), lds, stream, signal, sample_is_int16, Nmax,
                n_samples, denom, n_win, n_step, pad_to, F, Tpad, plane, partial, out_len);
  else if (mode == kPsfLogfbank)
    OS2S_LAUNCH(psf_logfbank_kernel<false>, dim3(Tpad, B), dim3(256), lds, stream, signal, sample_is_int16, Nmax,
                n_samples, denom, n_win, n_step, pad_to, nfilt, nfft, fb, (const float*)nullptr, 0, Tpad, plane,
                partial, out_len);
  else
    OS2S_LAUNCH(psf_logfbank_kernel<true>, dim3(Tpad, B), dim3(256), lds, stream, signal, sample_is_int16, Nmax,
                n_samples, denom, n_win, n_step, pad_to, nfilt, nfft, fb, dctl, F, Tpad, plane, partial, out_len);
  OS2S_LAUNCH(psf_normalize_kernel, dim3(64, B), dim3(256), 0, stream, plane, partial, out_len, F, Tpad, out_bf16,
              out_f32);
  return OS2S_OK;
}

extern "C" int os2s_psf_spectrogram(os2s_stream_t stream, const void* signal, int sample_is_int16,
                                    const int32_t* n_samples, int B, long long Nmax, int n_win,
                                    int n_step, int pad_to, int num_features, int Tpad,
                                    uint16_t* out_bf16, float* out_f32, int32_t* out_len,
                                    void* workspace, size_t workspace_bytes) {
  OS2S_REQUIRE(num_features <= n_win / 2 + 1);   // the reference's assertion (speech_utils.py:501-502)
  return psf_features(stream, kPsfSpectrogram, signal, sample_is_int16, n_samples, B, Nmax, n_win, n_step, pad_to,
                      num_features, 0, 0, nullptr, nullptr, Tpad, out_bf16, out_f32, out_len, workspace,
                      workspace_bytes);
}

// 'logfbank' of the psf backend (see psf_logfbank_kernel): fb = [nfilt][nfft/2 + 1] fp32 filter table on the
// device (python_speech_features.get_filterbanks; the host layer builds it). nfft: a power of two >= n_win.
// Workspace as os2s_psf_spectrogram_workspace_bytes(B, Tpad, nfilt).
extern "C" int os2s_psf_logfbank(os2s_stream_t stream, const void* signal, int sample_is_int16,
                                 const int32_t* n_samples, int B, long long Nmax, int n_win, int n_step,
                                 int pad_to, int nfilt, int nfft, const float* fb, int Tpad,
                                 uint16_t* out_bf16, float* out_f32, int32_t* out_len, void* workspace,
                                 size_t workspace_bytes) {
  return psf_features(stream, kPsfLogfbank, signal, sample_is_int16, n_samples, B, Nmax, n_win, n_step, pad_to, nfilt,
                      nfilt, nfft, fb, nullptr, Tpad, out_bf16, out_f32, out_len, workspace, workspace_bytes);
}

// 'mfcc' of the psf backend (psf_logfbank_kernel<true>): fb = [nfilt][nfft/2 + 1] filter table as for
// os2s_psf_logfbank, dctl = [numcep][nfilt] fp32 DCT-II x lifter table (device; the host layer builds both).
// Workspace as os2s_psf_spectrogram_workspace_bytes(B, Tpad, numcep): only the cepstra reach memory.
extern "C" int os2s_psf_mfcc(os2s_stream_t stream, const void* signal, int sample_is_int16,
                             const int32_t* n_samples, int B, long long Nmax, int n_win, int n_step, int pad_to,
                             int numcep, int nfilt, int nfft, const float* fb, const float* dctl, int Tpad,
                             uint16_t* out_bf16, float* out_f32, int32_t* out_len, void* workspace,
                             size_t workspace_bytes) {
  OS2S_REQUIRE(dctl && numcep <= nfilt);
  return psf_features(stream, kPsfMfcc, signal, sample_is_int16, n_samples, B, Nmax, n_win, n_step, pad_to, numcep,
                      nfilt, nfft, fb, dctl, Tpad, out_bf16, out_f32, out_len, workspace, workspace_bytes);
}
