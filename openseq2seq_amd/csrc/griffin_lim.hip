// Griffin-Lim vocoder (open_seq2seq/models/text2speech.py:182-198, called by save_audio :111-179): librosa's
// stft / istft pair with its defaults (hop = n_fft/4, periodic Hann(n_fft), center=True with reflect padding,
// istft divided by the window sum of squares and trimmed by n_fft/2 at each end) as two exact-fp32 direct-DFT
// GEMMs per iteration on v_mfma_f32_32x32x2_f32, all utterances of a ragged batch in one grid.
//
//   analysis + projection   X^T[bin, t] = sum_n A[n, bin] * frame_t[n]        (M = bins, N = frames, K = n_fft)
//       The frames are read from the utterance's signal tile in LDS by Toeplitz addressing (frame t starts at
//       t * hop; the reflect padding is applied while the tile is staged). The re and the im accumulator of a
//       (bin, frame) pair sit in the same lane and register, so the epilogue writes Y = M * X / |X| directly.
//   synthesis + overlap-add out[j, n] = sum_{r < 4} sum_c Y^T[c, j - r] * S[c, r, n]  (M = hop blocks, N = hop, K = 4 * 2Kp)
//       times 1 / window_sumsquare, written to the other of two signal buffers: no atomics, no scatter.
//
// Spectra are kept TRANSPOSED, [channel][frame] with the frame index contiguous, so that both kernels read
// their MFMA operands and write their results as 128-byte rows of consecutive lanes.
//
// Summation. An MFMA accumulator is a k-ordered fp32 fma chain, and the products here are long: n_fft terms in
// the analysis, 4 * 2Kp (3328 at n_fft 800) in the synthesis. One chain that long is several times less accurate
// than a blocked sgemm or an FFT, and 50 iterations on a short utterance amplify the difference (n_fft 800, 9
// frames: 2e-4 of the float64 run where the float32 matrix form on the host gives 1e-5). So both kernels sum in
// two levels: chains of kSumBlock k steps into a fresh accumulator, each added to a running total. The order is
// fixed, so a run is bit-reproducible and an utterance's result does not depend on its batch-mates.
#include "os2s_common.hpp"

namespace {
using os2s::f32x16;

constexpr int kFrameTile = 64;   // frames (analysis) / hop blocks (synthesis) per wave tile: two 32-wide MFMA tiles
constexpr int kMaxWaves = 8;
constexpr int kSumBlock = 64;    // k steps per fma chain, about sqrt of the longest product: see "Summation"

__device__ __forceinline__ int utt_frames(const int32_t* lengths, int b, int T_max) {
  const int t = lengths[b];
  return t > T_max ? T_max : t;       // < 4: the utterance is skipped by every kernel (the host layer rejects it)
}

// row of a 32x32 accumulator held in register r by lane half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---------------------------------------------------------------------------------------------------------
// M = clip(mag, 0, clip_max) ** power (no clip when clip_max <= 0), Y0 = M * exp(2 pi i phase0), transposed into
// the [channel][frame] layout; flags[b] = 1 when a magnitude of the utterance is not finite.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gl_init_kernel(const float* __restrict__ mag, const float* __restrict__ phase0,
                                                      const int32_t* __restrict__ lengths, int T_max, int K, int Kp,
                                                      float power, float clip_max, float* __restrict__ Mt,
                                                      float* __restrict__ Yt, int32_t* __restrict__ flags) {
  const int b = blockIdx.y;
  const int Tb = utt_frames(lengths, b, T_max);
  if (Tb < 4) return;
  const long long n = (long long)Tb * K;
  const float* mb = mag + (size_t)b * T_max * K;
  const float* pb = phase0 + (size_t)b * T_max * K;
  float* Mb = Mt + (size_t)b * Kp * T_max;
  float* Yb = Yt + (size_t)b * 2 * Kp * T_max;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(i / K), k = (int)(i - (long long)t * K);
    float m = mb[i];
    bad |= !isfinite(m);
    if (clip_max > 0.f) m = fminf(fmaxf(m, 0.f), clip_max);
    if (power != 1.f) m = powf(m, power);
    float s, c;
    sincospif(2.f * pb[i], &s, &c);
    Mb[(size_t)k * T_max + t] = m;
    Yb[(size_t)k * T_max + t] = m * c;
    Yb[(size_t)(Kp + k) * T_max + t] = m * s;
  }
  if (bad) flags[b] = 1;
}

// ---------------------------------------------------------------------------------------------------------
// analysis + projection. grid (frame tiles of 64, bin-tile groups, B); blockDim = 64 * waves, wave w of group g
// owns the 32 bins starting at 32 * (g * waves + w). basis [n_fft][2 * Kp]: cos * window in columns [0, Kp),
// -sin * window in [Kp, 2 Kp), columns >= K zero.
// LDS: the padded-signal tile [64 frames], hop block q of it at q * (hop + pad) with (hop + pad) % 32 == 1, so
// the 32 lanes of a ds_read_b32 group (32 consecutive frames, one sample offset) fall into 32 banks.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * kMaxWaves) gl_analysis_kernel(
    const float* __restrict__ sig, long long sig_stride, const int32_t* __restrict__ lengths,
    const float* __restrict__ basis, const float* __restrict__ Mt, float* __restrict__ Yt, int T_max, int n_fft,
    int K, int Kp, int lds_row) {
  extern __shared__ float tile[];
  const int b = blockIdx.z;
  const int Tb = utt_frames(lengths, b, T_max);
  const int t0 = blockIdx.x * kFrameTile;
  if (Tb < 4 || t0 >= Tb) return;
  const int hop = n_fft >> 2;
  const int L = hop * (Tb - 1);
  const float* x = sig + (size_t)b * sig_stride;

  // stage hop blocks t0 .. t0 + 66 of the reflect-padded signal (padded index p <-> sample p - n_fft/2)
  const int nblk = kFrameTile + 3;
  for (int i = threadIdx.x; i < nblk * hop; i += blockDim.x) {
    const int q = i / hop, o = i - q * hop;
    int s = (t0 + q) * hop + o - 2 * hop;
    if (s < 0) s = -s;
    if (s >= L) s = 2 * (L - 1) - s;
    tile[q * lds_row + o] = (s >= 0 && s < L) ? x[s] : 0.f;     // beyond the reflection: frames >= Tb only
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int bin0 = 32 * (blockIdx.y * (blockDim.x >> 6) + wave);
  if (bin0 >= Kp) return;
  f32x16 re0 = {0}, im0 = {0}, re1 = {0}, im1 = {0};
  const float* bp = basis + (size_t)h * 2 * Kp + bin0 + j;      // A operand: A[i = bin][k = h]
  const float* f0 = tile + j * lds_row + h;                     // B operand: B[k = h][j = frame]
  const float* f1 = f0 + 32 * lds_row;
  for (int q = 0; q < 4; ++q) {
    for (int k0 = 0; k0 < hop; k0 += kSumBlock) {
      const int nk = hop - k0 < kSumBlock ? hop - k0 : kSumBlock;
      const float* g0 = f0 + k0;
      const float* g1 = f1 + k0;
      f32x16 cr0 = {0}, ci0 = {0}, cr1 = {0}, ci1 = {0};
#pragma unroll 4
      for (int k = 0; k < nk; k += 2) {
        const float ac = bp[0], as = bp[Kp];
        const float x0 = g0[k], x1 = g1[k];
        cr0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, x0, cr0, 0, 0, 0);
        ci0 = __builtin_amdgcn_mfma_f32_32x32x2f32(as, x0, ci0, 0, 0, 0);
        cr1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, x1, cr1, 0, 0, 0);
        ci1 = __builtin_amdgcn_mfma_f32_32x32x2f32(as, x1, ci1, 0, 0, 0);
        bp += (size_t)4 * Kp;
      }
      re0 += cr0;
      im0 += ci0;
      re1 += cr1;
      im1 += ci1;
    }
    f0 += lds_row;
    f1 += lds_row;
  }

  // epilogue: Y = M * X / |X| (1 + 0i where |X| == 0), lanes = consecutive frames
  const float* Mb = Mt + (size_t)b * Kp * T_max;
  float* Yb = Yt + (size_t)b * 2 * Kp * T_max;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int t = t0 + 32 * f + j;
    if (t >= Tb) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int bin = bin0 + acc_row(r, h);
      if (bin >= K) continue;
      const float xr = f ? re1[r] : re0[r], xi = f ? im1[r] : im0[r];
      const float a = hypotf(xr, xi);
      const float m = Mb[(size_t)bin * T_max + t];
      const float pr = a > 0.f ? xr / a : 1.f, pi = a > 0.f ? xi / a : 0.f;
      Yb[(size_t)bin * T_max + t] = m * pr;
      Yb[(size_t)(Kp + bin) * T_max + t] = m * pi;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// synthesis + overlap-add. One wave per tile of 64 hop blocks x 32 samples; wave tiles are numbered
// (block tile, sample tile) and dealt to waves in order: grid (ceil(tiles / waves), 1, B), no LDS.
// synth [2 * Kp][4][hopP]: row c < Kp = w_c / n_fft * cos * window, row Kp + c = -w_c / n_fft * sin * window
// (w = 1 for DC and Nyquist, else 2), split into the four hop blocks a frame covers; columns >= hop zero.
// Padded hop block jb (jb = 2 .. Tb, the blocks istft keeps) sums frames jb - 3 .. jb; frames outside
// [0, Tb) contribute zero. inv_wss [3][hopP]: first kept block (frames 0 .. 2), interior, last (Tb-3 .. Tb-1).
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gl_synthesis_kernel(
    const float* __restrict__ Yt, const int32_t* __restrict__ lengths, const float* __restrict__ synth,
    const float* __restrict__ inv_wss, float* __restrict__ out, long long out_stride, int T_max, int n_fft, int Kp,
    int hopP, int32_t* __restrict__ flags) {
  const int b = blockIdx.z;
  const int Tb = utt_frames(lengths, b, T_max);
  if (Tb < 4) return;
  const int hop = n_fft >> 2;
  const int ntile_n = hopP >> 5;
  const int wt = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int jt = wt / ntile_n, nt = wt - jt * ntile_n;
  const int jb0 = 2 + jt * kFrameTile;                 // first padded hop block of the tile
  if (jb0 > Tb) return;
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const float* Yb = Yt + (size_t)b * 2 * Kp * T_max + (size_t)h * T_max;      // A[i = hop block][k = h]
  const float* sp = synth + ((size_t)h * 4) * hopP + nt * 32 + j;             // B[k = h][j = sample]
  f32x16 acc0 = {0}, acc1 = {0};
  for (int r = 0; r < 4; ++r) {
    const int ta = jb0 + j - r, tb = ta + 32;
    const bool va = ta >= 0 && ta < Tb, vb = tb >= 0 && tb < Tb;
    const float* ya = Yb + (va ? ta : 0);
    const float* yb = Yb + (vb ? tb : 0);
    const float* s = sp + r * hopP;
    for (int c0 = 0; c0 < 2 * Kp; c0 += kSumBlock) {      // 2 * Kp is a multiple of 64
      f32x16 c0acc = {0}, c1acc = {0};
#pragma unroll 4
      for (int c = 0; c < kSumBlock; c += 2) {
        const float w = s[0];
        const float a0 = va ? ya[0] : 0.f, a1 = vb ? yb[0] : 0.f;
        c0acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, w, c0acc, 0, 0, 0);
        c1acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, w, c1acc, 0, 0, 0);
        ya += (size_t)2 * T_max;
        yb += (size_t)2 * T_max;
        s += (size_t)8 * hopP;
      }
      acc0 += c0acc;
      acc1 += c1acc;
    }
  }
  const int n = nt * 32 + j;
  if (n >= hop) return;
  float* ob = out + (size_t)b * out_stride;
  bool bad = false;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jb = jb0 + 32 * f + acc_row(r, h);
      if (jb > Tb) continue;
      const int cls = jb == 2 ? 0 : (jb == Tb ? 2 : 1);
      const float v = (f ? acc1[r] : acc0[r]) * inv_wss[cls * hopP + n];
      bad |= !isfinite(v);
      ob[(size_t)(jb - 2) * hop + n] = v;
    }
  }
  if (flags && bad) flags[b] = 1;
}

inline int analysis_lds_row(int hop) {
  int pad = (1 - hop) % 32;
  if (pad < 0) pad += 32;
  return hop + pad;
}
inline bool gl_args_ok(int B, int T_max, int n_fft) {
  return B >= 1 && T_max >= 4 && n_fft >= 64 && n_fft <= 2048 && n_fft % 8 == 0;
}
inline size_t align256(size_t n) { return (n + 255) / 256 * 256; }
}  // namespace

static_assert(kSumBlock % 2 == 0 && 64 % kSumBlock == 0, "the synthesis sums 2 * Kp channels in whole blocks");

extern "C" int os2s_griffin_lim_kpad(int n_fft) { return (n_fft / 2 + 1 + 31) / 32 * 32; }
extern "C" int os2s_griffin_lim_hop_pad(int n_fft) { return (n_fft / 4 + 31) / 32 * 32; }

extern "C" size_t os2s_griffin_lim_workspace_bytes(int B, int T_max, int n_fft) {
  if (!gl_args_ok(B, T_max, n_fft)) return 0;
  const size_t Kp = (size_t)os2s_griffin_lim_kpad(n_fft);
  const size_t spec = (size_t)B * Kp * T_max * sizeof(float);
  const size_t sig = (size_t)B * (n_fft / 4) * (T_max - 1) * sizeof(float);
  return align256(spec) + align256(2 * spec) + align256(sig);
}

extern "C" int os2s_griffin_lim(os2s_stream_t stream_, const float* mag, const int32_t* lengths, const float* phase0,
                                const float* basis_analysis, const float* basis_synthesis, const float* inv_wss,
                                int B, int T_max, int n_fft, float power, float clip_max, int n_iters, float* out,
                                int32_t* flags, void* workspace, size_t workspace_bytes) {
  hipStream_t stream = (hipStream_t)stream_;
  OS2S_REQUIRE(mag && lengths && phase0 && basis_analysis && basis_synthesis && inv_wss && out && flags && workspace);
  OS2S_REQUIRE(gl_args_ok(B, T_max, n_fft) && n_iters >= 0 && B <= 65535);
  if (workspace_bytes < os2s_griffin_lim_workspace_bytes(B, T_max, n_fft)) return OS2S_ERR_WORKSPACE;
  const int K = n_fft / 2 + 1, Kp = os2s_griffin_lim_kpad(n_fft), hop = n_fft / 4;
  const int hopP = os2s_griffin_lim_hop_pad(n_fft);
  const size_t spec = (size_t)B * Kp * T_max * sizeof(float);
  const long long sig_stride = (long long)hop * (T_max - 1);
  float* Mt = (float*)workspace;
  float* Yt = (float*)((char*)workspace + align256(spec));
  float* sig2 = (float*)((char*)Yt + align256(2 * spec));

  // bins >= K of Y stay zero for the whole run (their synthesis rows are zero too, and 0 * garbage could be NaN);
  // samples past an utterance's end stay zero in both signal buffers
  if (hipMemsetAsync(workspace, 0, os2s_griffin_lim_workspace_bytes(B, T_max, n_fft), stream) != hipSuccess ||
      hipMemsetAsync(out, 0, (size_t)B * sig_stride * sizeof(float), stream) != hipSuccess ||
      hipMemsetAsync(flags, 0, (size_t)B * sizeof(int32_t), stream) != hipSuccess)
    return OS2S_ERR_LAUNCH;

  const long long per_utt = (long long)T_max * K;
  OS2S_LAUNCH(gl_init_kernel, dim3((unsigned)os2s::ceil_div(per_utt, 256 * 8), B), dim3(256), 0, stream, mag, phase0,
              lengths, T_max, K, Kp, power, clip_max, Mt, Yt, flags);

  // analysis geometry: the bin tiles are split evenly over as few workgroups of <= 8 waves as possible
  const int nbt = Kp / 32;
  const int groups = os2s::ceil_div(nbt, kMaxWaves), waves = os2s::ceil_div(nbt, groups);
  const int lds_row = analysis_lds_row(hop);
  const size_t lds = (size_t)(kFrameTile + 3) * lds_row * sizeof(float);
  OS2S_REQUIRE(lds <= 160 * 1024);
  const int ft = os2s::ceil_div(T_max, kFrameTile);
  // synthesis geometry: kept hop blocks 2 .. T_max
  const int wtiles = os2s::ceil_div(T_max - 1, kFrameTile) * (hopP / 32);
  const dim3 sgrid((unsigned)os2s::ceil_div(wtiles, 4), 1, B);

  // launch i writes signal buffer (n_iters - i) % 2, so the last one writes `out`
  for (int i = 0; i <= n_iters; ++i) {
    float* dst = ((n_iters - i) & 1) ? sig2 : out;
    float* src = ((n_iters - i) & 1) ? out : sig2;
    if (i > 0)
      OS2S_LAUNCH_LDS(gl_analysis_kernel, dim3(ft, groups, B), dim3(64 * waves), lds, stream, (const float*)src, sig_stride,
                      lengths, basis_analysis, (const float*)Mt, Yt, T_max, n_fft, K, Kp, lds_row);
    OS2S_LAUNCH(gl_synthesis_kernel, sgrid, dim3(256), 0, stream, (const float*)Yt, lengths, basis_synthesis, inv_wss,
                dst, sig_stride, T_max, n_fft, Kp, hopP, i == 0 ? flags : (int32_t*)nullptr);
  }
  return OS2S_OK;
}
