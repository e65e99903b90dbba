// Shared by the attention-RNN decoder's teacher-forced pass (attn_decoder.hip) and the Tacotron2 step kernels
// (tacotron_infer.hip): argument blocks, block-wide reductions, and the host functions that cross the two units.
#pragma once
#include "os2s_common.hpp"

namespace os2s {

constexpr int kAttnThreads = 512;
constexpr int kAttnWaves = kAttnThreads / 64;
constexpr int kLocKMax = 32;   // location filter taps held in registers (U == 128: 2 units / lane)
constexpr int kLocParts = 4;        // unit parts (32 units each)
constexpr int kLocUnits = 32;
constexpr int kLocCtxParts = 8;

__device__ __forceinline__ float tanh_fast(float x) { return 1.f - 2.f / (1.f + __expf(2.f * x)); }

// Zoneout of one (unit, sample) of a cell's STATE stores (os2s_attn_decoder_t.zoneout_mode; the cell's output
// is never touched). mode 1: Bernoulli(1 - p) masks from the counter hash over the layer's logical [B, T, H]
// tensor (element idx), one seed for h and one for c; a zoned element is an exact copy of the old state.
// mode 2: p old + (1 - p) new in fp32, rounded once. hst / cst come in holding the new state.
__device__ __forceinline__ void zoneout_state(int mode, float p, unsigned long long seed_h, unsigned long long seed_c,
                                              unsigned long long idx, float hn, bf16_t hprev, float cn, float cprev,
                                              bf16_t& hst, float& cst) {
  if (mode == 1) {
    const float keep = 1.f - p;
    const int sh = (int)(idx & 7);
    if (!((dropout_bits8(seed_h, idx >> 3, keep) >> sh) & 1u)) hst = hprev;
    if (!((dropout_bits8(seed_c, idx >> 3, keep) >> sh) & 1u)) cst = cprev;
  } else {
    hst = f2bf(p * bf2f(hprev) + (1.f - p) * hn);
    cst = p * cprev + (1.f - p) * cn;
  }
}

__device__ __forceinline__ float block_sum(float x, float* red) {
  x = wave_sum_dpp(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < kAttnWaves; ++w) s += red[w];
  return s;
}
__device__ __forceinline__ float block_max(float x, float* red) {
  x = wave_max_dpp(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < kAttnWaves; ++w) s = fmaxf(s, red[w]);
  return s;
}

// Location-sensitive attention: Conv1D(K taps -> F filters, bias) followed by the bias-free
// dense F -> U has no non-linearity in between, so per call the two are folded into ONE
// filter  Wck[k,u] = sum_f conv_w[k,f] dense_w[f,u],  bd[u] = sum_f conv_b[f] dense_w[f,u]:
//   location[s,u] = sum_k cum[s + k - padl] Wck[k,u] + bd[u]
// (F x fewer multiply-adds in the loop, Wck lives in registers: lane owns 2 units). The
// gradient w.r.t. conv_w / conv_b / dense_w is recovered from dWck, d(bd) after the loop.
struct AdAttn {
  int B, T, S, H, M, U, t, mode, use_bias, loc_k, Kc0, last;
  const int32_t* src_len;
  const int32_t* tgt_len;
  const bf16_t* yq;      // query input rows: yq + b*yq_bs + t*yq_ts
  long long yq_bs, yq_ts;
  const bf16_t* wq;      // [U, H]
  const bf16_t* keys;    // [B, S, U]
  const bf16_t* values;  // [B, S, M]
  const float* v; const float* g; const float* bias;
  const float* wck;      // [K, U] folded location filter followed by bd [U]   (mode 2)
  float* cum_seq;        // [B, T+1, S]
  float* align_seq;      // [B, T, S]
  float* q_seq;          // [B, T, U]
  bf16_t* ctx;           // raw context rows: ctx + b*ctx_bs + t*ctx_ts
  long long ctx_bs, ctx_ts;
  bf16_t* cat0;          // [B, T+1, Kc0]
  float attn_in_keep;
  unsigned long long attn_in_seed;
  // backward only
  const bf16_t* dctx_ext; long long dctx_bs, dctx_ts;   // external gradient of ctx rows or null
  const float* dattn;    // [B, M] gradient w.r.t. the attention part of cat0[t+1] (null when last)
  bf16_t* dctx_seq;      // [B, T, M] total context gradient (for the dvalues pass)
  float* dcum;           // [B, S] carry (mode 2)
  bf16_t* dpre_seq;      // [B, T, S, U] score pre-activation gradients (dkeys = sum over T)
  bf16_t* dq_seq;        // [B, T, U]
  float* dhq;            // [B, H]
  float* dnv_acc;        // [B, U]
  float* dbd_acc;        // [B, U]      (mode 2)
  float* dwck_acc;       // [B, K, U]   (mode 2)
};

struct AdLoc {
  float* e_part;      // [B, kLocParts, S] partial scores (forward)
  float* dal;         // [B, S] d(alignment) incl. the carried state gradient (backward)
  float* dcum_part;   // [B, kLocParts, S] this step's state-gradient contributions per unit part
};

struct TiLstm {
  int B, H, K, Ka;                   // K = Ka + Kb input columns
  const bf16_t* in_a; long long lda; // row b: in_a + b * lda  (Ka columns; Ka == 0: unused)
  const bf16_t* in_b; long long ldb; // row b: in_b + b * ldb  (K - Ka columns)
  const void* w;                     // [4H, K] e4m3 (FP8) or bf16
  const float* scale;                // [4H] row scales (FP8)
  const float* bias;                 // [4H] or null
  float forget_bias;
  const float* c_prev; long long ldc_prev;   // row b at c_prev + b * ldc_prev, or null (zeros)
  float* c_out; long long ldc_out;
  bf16_t* h1; long long ldh1;        // h destinations (row b at h + b * ld; either may be null)
  bf16_t* h2; long long ldh2;        //   h2 takes the output dropout (training: the cell's OUTPUT, not its state)
  const int32_t* state;              // state[1] != 0: decoding has ended (null: no stop flag — the training pass)
  // training pass (os2s_attn_decoder_fwd): input projection of the step, saved gates, output dropout
  const bf16_t* gx; long long ldgx;  // row b: gx + b * ldgx, [4H] (or null)
  bf16_t* gates; long long ldgates;  // row b: gates + b * ldgates, [4H] = i, f, g, o activations (or null)
  float out_keep; unsigned long long out_seed; long long drop_t, drop_T;   // element index ((b * T + t) * H + j)
  // zoneout of the state stores (c_out, h1): mode 0 off; h_prev = the state row the step read (row b at
  // h_prev + b * ldh1); mode 1 indexes its masks like the output dropout (drop_t, drop_T)
  int zo_mode; float zo_p; unsigned long long zo_seed_h, zo_seed_c; const bf16_t* h_prev;
};

// attn_decoder.hip:
int ad_check(const os2s_attn_decoder_t* d);
void ad_fill_attn(const os2s_attn_decoder_t* d, AdAttn& a);
bool loc_split(const os2s_attn_decoder_t* d);     // the split location-attention kernels apply
int ad_launch_fold_location(hipStream_t stream, const os2s_attn_decoder_t* d);   // conv + dense -> d->loc_ws
// tacotron_infer.hip: the training pass's cells and scores on the step kernels (false: keep the round-3 kernels)
bool ad_fast_cells(const os2s_attn_decoder_t* d);
int ad_launch_fast_cell(hipStream_t stream, const os2s_attn_decoder_t* d, int l, int t);
int ad_launch_fast_scores(hipStream_t stream, const AdAttn& at, const AdLoc& lx, const os2s_attn_decoder_t* d);

}  // namespace os2s
