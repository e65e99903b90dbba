// Attention-RNN decoders (teacher-forced training pass and step-wise inference), gfx950.
//
// Reference semantics (tf.contrib.seq2seq.dynamic_decode over an AttentionWrapper cell):
//   * RNNDecoderWithAttention, attention_type gnmt / gnmt_v2
//     (open_seq2seq/decoders/rnn_decoders.py:147-321, parts/rnns/gnmt.py:32-79): the bottom
//     LSTM layer is the attention cell, cell_inputs = concat(inputs, previous attention)
//     (parts/rnns/attention_wrapper.py:1720-1760), query = its output, normalised Bahdanau
//     score (:482-539), attention = context (attention_layer_size=None, :1388-1415).
//   * Tacotron2Decoder (decoders/tacotron2_decoder.py:257-420): AttentionWrapper around a
//     MultiRNNCell of L LSTMCells (output dropout), LocationSensitiveAttention with
//     cumulative alignments (attention_wrapper.py:641-715, 749-878), output = concat(h, ctx).
//
// Structure: everything that does not depend on the previous step is hoisted out of the
// loop by the caller (input projection of all T steps, memory keys, layers above the
// attention cell, output projections, all weight gradients) and runs as large MFMA GEMMs.
// The loop itself is 2-3 launches per step forward and 3-4 backward, all state lives in
// per-step sequence buffers (slot t = input of step t), so a call can run any range of
// steps [t_begin, t_end) — the same entry point serves training and incremental decoding:
//   cell kernel   : gates = gx[t] + cat[t] . Wcat^T (split-K MFMA tile, rnn_tile.hpp),
//                   LSTM cell in the epilogue, h -> cat[t+1] (recurrence), dropped h -> y
//   attention     : one workgroup per sample: query projection, (location features),
//                   score, masked softmax, context; context -> ctx[t] and cat0[t+1]
//   backward      : d(attention input) GEMM, attention backward per sample (recomputes the
//                   tanh terms; accumulates dkeys, per-sample parameter partials), cell
//                   backward (two fused transposed GEMMs + gate derivatives).
#include <algorithm>
#include "attn_decoder_common.hpp"
#include "rnn_tile.hpp"

namespace os2s {

constexpr int kAdWaves = 8;

// ------------------------------------------------------------------ cell forward
struct AdCellFwd {
  int B, T, H, Kc, t;
  float forget_bias;
  const int32_t* lens;
  const bf16_t* cat;   // [B, T+1, Kc]
  const bf16_t* w;     // [4H, Kc]
  const uint8_t* w8;   // e4m3 copy of w [4H, Kc] (or null) ...
  const float* w8_scale;  // ... and its per-row scales [4H]
  const float* bias;   // [4H] or null
  const bf16_t* gx;    // [B, T, 4H] or null
  float* c_seq;        // [B, T, H]
  bf16_t* gates;       // [B, T, 4H] or null
  bf16_t* h_next;      // cat + column offset of the recurrent part
  bf16_t* y;           // dropped output, row (b,t) at y + b*y_bs + t*y_ts
  long long y_bs, y_ts;
  float out_keep;
  unsigned long long out_seed;
  int zo_mode;         // zoneout of the STATE stores (h_next, c_seq): 0 off, 1 sampled masks, 2 expectation blend
  float zo_p;
  unsigned long long zo_seed_h, zo_seed_c;
};

// One workgroup = 8 hidden units x 32 samples: the 32 tile rows are (gate, unit) pairs
// (row = 8*gate + unit), so H/8 workgroups stream disjoint 32-row slices of the weights and
// after the split-K reduction a lane owns all four gates of one (unit, sample).
// (20 slices per wave so that the Tacotron2 decoder LSTM, Kc = 2560, needs one round of loads instead
// of a second, mostly empty one: 46.1 vs 46.4 us per forward step — not kept.)
__global__ __launch_bounds__(64 * kAdWaves) void ad_cell_fwd_kernel(AdCellFwd p) {
  __shared__ float red[kAdWaves * 16 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int j0 = blockIdx.x * 8, b0 = blockIdx.y * 32;
  const int H = p.H;
  // the epilogue operands of this lane's (unit, sample) are fetched BEFORE the weight stream so that
  // their round trip overlaps it instead of following the reduction (as rnn.hip does)
  const int eb = b0 + l31, ej = j0 + wave + 4 * lhi;
  const bool elive = wave < 4 && eb < p.B && ej < H && !(p.lens && p.t >= p.lens[eb]);
  float e_gx[4] = {0.f, 0.f, 0.f, 0.f}, e_bias[4] = {0.f, 0.f, 0.f, 0.f}, e_sc[4] = {1.f, 1.f, 1.f, 1.f};
  float e_cprev = 0.f;
  if (elive) {
    const long long erow = (long long)eb * p.T + p.t;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (p.w8) e_sc[g] = p.w8_scale[g * H + ej];
      if (p.gx) e_gx[g] = bf2f(p.gx[erow * (4 * H) + (long long)g * H + ej]);
      if (p.bias) e_bias[g] = p.bias[g * H + ej];
    }
    if (p.t > 0) e_cprev = p.c_seq[(erow - 1) * H + ej];
  }
  f32x16 accw;
#pragma unroll
  for (int e = 0; e < 16; ++e) accw[e] = 0.f;
  {
    const int g = l31 >> 3, uu = min(j0 + (l31 & 7), H - 1);
    const int brow = b0 + l31;
    const bf16_t* irow = brow < p.B ? p.cat + ((long long)brow * (p.T + 1) + p.t) * p.Kc : nullptr;
    if (p.w8) {
      tile_gemm_prefetch_w8<kAdWaves, 16>(p.w8 + ((long long)g * H + uu) * p.Kc, irow, p.Kc, accw, p.w8, p.cat);
    } else {
      const bf16_t* wrow = p.w + ((long long)g * H + uu) * p.Kc;
      tile_gemm_prefetch<kAdWaves, 16>(wrow, irow, p.Kc, accw, p.w);
    }
  }
  float pre[4];
  tile_reduce_units<kAdWaves>(accw, red, pre);
  if (wave >= 4) return;
  const int b = b0 + l31;
  if (b >= p.B) return;
  if (p.lens && p.t >= p.lens[b]) return;   // finished sample: buffers stay zero
  const int j = j0 + wave + 4 * lhi;
  if (j >= H) return;
  const long long row = (long long)b * p.T + p.t;
#pragma unroll
  for (int g = 0; g < 4; ++g) pre[g] = pre[g] * e_sc[g] + e_gx[g] + e_bias[g];   // (scale: e4m3 weight rows)
  const float cprev = e_cprev;
  const float ig = sigmoidf_(pre[0]), gg = tanhf(pre[1]);
  const float fg = sigmoidf_(pre[2] + p.forget_bias), og = sigmoidf_(pre[3]);
  const float cn = cprev * fg + ig * gg;
  float hn = tanhf(cn) * og;
  // zoneout replaces the state the cell reads at step t + 1 (never the output y below)
  float cst = cn;
  bf16_t hst = f2bf(hn);
  if (p.zo_mode) {
    const bf16_t hprev = p.h_next[((long long)b * (p.T + 1) + p.t) * p.Kc + j];
    zoneout_state(p.zo_mode, p.zo_p, p.zo_seed_h, p.zo_seed_c, (unsigned long long)row * H + j, hn, hprev, cn,
                  cprev, hst, cst);
  }
  p.c_seq[row * H + j] = cst;
  if (p.gates) {
    bf16_t* gp = p.gates + row * (4 * H) + j;
    gp[0] = f2bf(ig); gp[H] = f2bf(fg); gp[2 * H] = f2bf(gg); gp[3 * H] = f2bf(og);
  }
  p.h_next[((long long)b * (p.T + 1) + p.t + 1) * p.Kc + j] = hst;
  if (p.out_keep < 1.f) {
    const unsigned long long idx = (unsigned long long)row * H + j;
    const uint32_t bits = dropout_bits8(p.out_seed, idx >> 3, p.out_keep);
    hn = ((bits >> (j & 7)) & 1u) ? hn / p.out_keep : 0.f;
  }
  p.y[(long long)b * p.y_bs + (long long)p.t * p.y_ts + j] = f2bf(hn);
}

// ------------------------------------------------------------------ attention (shared)
// development aid (build with -DOS2S_ATTN_PHASE_TIMERS): phase timestamps (s_memtime) of
// workgroup 0, read by os2s_debug_attn_phases / tools/bench_attn_decoder.py
#ifdef OS2S_ATTN_PHASE_TIMERS
__device__ long long g_attn_dbg[2][16];
#define AD_TICK(k, i) do { if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) g_attn_dbg[k][i] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define AD_TICK(k, i) do { } while (0)
#endif

// LDS carve-up (floats) shared by the forward and backward attention kernels
struct AttnLds {
  float *hq, *q, *nv, *bs, *e, *red, *cum, *scratch;
  uint32_t* keys;   // resident: [S][U/2] bf16 pairs of this sample's keys (staged once per launch);
                    // streamed: [kAttnWaves][U/2], the key row each wave is working on
};
constexpr int kCtxSplitMax = 8;
// Two residency modes of the keys in the one-workgroup-per-sample kernels (non-location modes). Resident: all
// S rows of the sample are staged in LDS before the score loop. Streamed: a wave fetches the row of its source
// position from global memory with 16-byte loads (the next row is in flight while the current one is used) and
// passes it through a row buffer of its own, because the score loops give a lane the unit pairs 2*lane + 128*i
// — a 4-byte interleave — while a 16-byte load delivers four neighbouring pairs. Every key element is read once
// per launch in both modes, the loops read the same pairs in the same order, so the results are bit-identical;
// the streamed footprint does not grow with S * U.
__host__ __device__ inline size_t attn_lds_floats(int H, int M, int U, int S, int mode, int K, bool bwd,
                                                  bool resident = true) {
  size_t n = (size_t)H + 3 * U + S + 64 + (resident ? (size_t)S * U / 2 : (size_t)kAttnWaves * U / 2);
  if (mode == 2) n += (size_t)(S + kLocKMax);
  size_t scratch = (size_t)kCtxSplitMax * M;     // forward: context partials
  if (bwd)   // dctx, dalign, de, dcum, dq/dnv partials, dWck
    scratch = (size_t)M + 3 * S + 2 * (size_t)kAttnWaves * U + (mode == 2 ? (size_t)K * U : 0);
  return n + scratch + 64;
}
__device__ __forceinline__ AttnLds attn_lds_carve(float* base, int H, int U, int S, int mode, int K,
                                                  bool resident = true) {
  AttnLds l;
  l.hq = base; base += H;
  l.q = base; base += U;
  l.nv = base; base += U;
  l.bs = base; base += U;
  l.e = base; base += S;
  l.red = base; base += 64;
  l.cum = nullptr;
  if (mode == 2) { l.cum = base; base += S + kLocKMax; }
  l.keys = reinterpret_cast<uint32_t*>(base); base += resident ? (size_t)S * U / 2 : (size_t)kAttnWaves * U / 2;
  l.scratch = base;
  return l;
}

// score parameters -> LDS: nv (normalised v for mode 1), bs (bias (+ folded location bias))
__device__ __forceinline__ void attn_load_score_params(const AdAttn& p, const AttnLds& l) {
  const int tid = threadIdx.x, U = p.U;
  float ss = 0.f;
  for (int u = tid; u < U; u += kAttnThreads) {
    const float v = p.v[u];
    l.nv[u] = v;
    ss += v * v;
    float b = ((p.mode == 1 || (p.mode == 2 && p.use_bias)) && p.bias) ? p.bias[u] : 0.f;
    if (p.mode == 2) b += p.wck[p.loc_k * U + u];
    l.bs[u] = b;
  }
  if (p.mode == 1) {
    const float tot = block_sum(ss, l.red);
    const float sc = p.g[0] * rsqrtf(tot);
    for (int u = tid; u < U; u += kAttnThreads) l.nv[u] *= sc;
  }
  __syncthreads();
}

// this sample's keys -> LDS with 16-byte coalesced loads (all in flight at once; the latency
// hides behind the query projection)
__device__ __forceinline__ void attn_stage_keys(const AdAttn& p, const AttnLds& l, int b, int slen) {
  const int n16 = slen * p.U / 8;
  const u32x4* src = reinterpret_cast<const u32x4*>(p.keys + (long long)b * p.S * p.U);
  u32x4* dst = reinterpret_cast<u32x4*>(l.keys);
  for (int i = threadIdx.x; i < n16; i += kAttnThreads) dst[i] = src[i];
}

// cumulative alignments (state BEFORE step t), zero-padded for the SAME convolution
__device__ __forceinline__ void attn_load_cum(const AdAttn& p, const AttnLds& l, int b) {
  const int S = p.S, K = p.loc_k, padl = (K - 1) / 2;
  const float* cum = p.cum_seq + ((long long)b * (p.T + 1) + p.t) * S;
  for (int i = threadIdx.x; i < S + kLocKMax; i += kAttnThreads) {
    const int s = i - padl;
    l.cum[i] = (s >= 0 && s < S) ? cum[s] : 0.f;
  }
}

// pre-activation of the score for (s, unit pair u, u+1) without the location term; krow = the U/2 pairs of row s
__device__ __forceinline__ void attn_pre2(const AttnLds& l, const uint32_t* krow, int u, float& x0, float& x1) {
  const uint32_t kv = krow[u >> 1];
  x0 = bflo(kv) + l.q[u] + l.bs[u];
  x1 = bfhi(kv) + l.q[u + 1] + l.bs[u + 1];
}

// Streamed keys: the 16-byte pieces of one key row that a lane fetches (U <= 1024: at most 128 pieces, two per
// lane). attn_row_fetch issues the loads (addresses clamped, never under a branch on the data), attn_row_put
// hands the row to the wave's LDS row buffer. LDS operations of one wave complete in order; the wave barriers
// only keep the compiler from moving a lane's reads across another lane's writes.
constexpr int kRowPieces = 2;
struct AttnRow { u32x4 v[kRowPieces]; };
__device__ __forceinline__ AttnRow attn_row_fetch(const AdAttn& p, int b, int s) {
  const int lane = threadIdx.x & 63, n16 = p.U / 8;
  const u32x4* src = reinterpret_cast<const u32x4*>(p.keys + ((long long)b * p.S + s) * p.U);
  AttnRow r;
#pragma unroll
  for (int i = 0; i < kRowPieces; ++i) r.v[i] = src[min(lane + 64 * i, n16 - 1)];
  return r;
}
__device__ __forceinline__ void attn_row_put(const AdAttn& p, uint32_t* krow, const AttnRow& r) {
  const int lane = threadIdx.x & 63, n16 = p.U / 8;
  __builtin_amdgcn_wave_barrier();       // the reads of the previous row come first
#pragma unroll
  for (int i = 0; i < kRowPieces; ++i)
    if (lane + 64 * i < n16) reinterpret_cast<u32x4*>(krow)[lane + 64 * i] = r.v[i];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// finished sample (t >= tgt_len[b]) in location mode: the cumulative alignments carry over, row t + 1 =
// row t (the state of impute_finished); every other buffer of the step stays as the caller zeroed it
__device__ __forceinline__ void attn_carry_cum(const AdAttn& p, int b) {
  if (p.mode != 2) return;
  float* cum = p.cum_seq + ((long long)b * (p.T + 1) + p.t) * p.S;
  for (int sp = threadIdx.x; sp < p.S; sp += blockDim.x) cum[p.S + sp] = cum[sp];
}

// ------------------------------------------------------------------ attention forward
// RES: keys resident in LDS (always in location mode); !RES: streamed, see attn_lds_floats
template <bool RES>
__global__ __launch_bounds__(kAttnThreads) void ad_attn_fwd_kernel(AdAttn p) {
  extern __shared__ float lds_raw[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (p.tgt_len && p.t >= p.tgt_len[b]) { attn_carry_cum(p, b); return; }
  const int H = p.H, M = p.M, U = p.U, S = p.S, K = p.loc_k;
  const AttnLds l = attn_lds_carve(lds_raw, H, U, S, p.mode, K, RES);
  const int slen = min(max(p.src_len[b], 0), S);
  AD_TICK(0, 0);
  // query input
  const bf16_t* yq = p.yq + (long long)b * p.yq_bs + (long long)p.t * p.yq_ts;
  for (int h8 = tid; h8 < H / 8; h8 += kAttnThreads) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(yq + h8 * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) { l.hq[h8 * 8 + 2 * e] = bflo(v[e]); l.hq[h8 * 8 + 2 * e + 1] = bfhi(v[e]); }
  }
  if constexpr (RES) attn_stage_keys(p, l, b, slen);
  if (p.mode == 2) attn_load_cum(p, l, b);
  attn_load_score_params(p, l);   // ends with a barrier
  AD_TICK(0, 1);
  // q[u] = hq . Wq[u, :]  — 8 units per wave per batch, all their loads in flight together
  constexpr int UB = 8;
  for (int u0 = wave * UB; u0 < U; u0 += UB * kAttnWaves) {
    float part[UB];
#pragma unroll
    for (int i = 0; i < UB; ++i) part[i] = 0.f;
    for (int h = lane * 8; h < H; h += 1024) {
      u32x4 wv[UB][2];
#pragma unroll
      for (int i = 0; i < UB; ++i)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
          // unconditional (clamped) loads: a load under a branch is waited for at the join,
          // which would serialise the round trips
          wv[i][hh] = *reinterpret_cast<const u32x4*>(p.wq + (long long)min(u0 + i, U - 1) * H +
                                                      min(h + 512 * hh, H - 8));
#pragma unroll
      for (int i = 0; i < UB; ++i)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
          if (h + 512 * hh < H) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              part[i] += bflo(wv[i][hh][e]) * l.hq[h + 512 * hh + 2 * e] +
                         bfhi(wv[i][hh][e]) * l.hq[h + 512 * hh + 2 * e + 1];
          }
    }
#pragma unroll
    for (int i = 0; i < UB; ++i) {
      const float s = wave_sum_dpp(part[i]);
      if (lane == 0 && u0 + i < U) {
        l.q[u0 + i] = s;
        p.q_seq[((long long)b * p.T + p.t) * U + u0 + i] = s;
      }
    }
  }
  __syncthreads();
  AD_TICK(0, 2);
  // scores: one wave per source position, a lane owns unit pairs
  if (p.mode == 2) {
    float wk[kLocKMax][2];
#pragma unroll
    for (int k = 0; k < kLocKMax; ++k) {
      wk[k][0] = wk[k][1] = 0.f;
      if (k < K) {
        const f32x2 w = *reinterpret_cast<const f32x2*>(p.wck + (long long)k * U + 2 * lane);
        wk[k][0] = w[0]; wk[k][1] = w[1];
      }
    }
    // a wave owns a contiguous range of source positions and slides a 32-entry register
    // window over the padded cumulative alignments: slot (j + k) & 31 holds cum[s + k] at the
    // j-th step of a 32-step block, so each step costs ONE new LDS read
    const int chunk = (slen + kAttnWaves - 1) / kAttnWaves;
    const int c0 = wave * chunk, c1 = min(c0 + chunk, slen);
    const float qb0 = l.q[2 * lane] + l.bs[2 * lane], qb1 = l.q[2 * lane + 1] + l.bs[2 * lane + 1];
    const float nv0 = l.nv[2 * lane], nv1 = l.nv[2 * lane + 1];
    if (c0 < c1) {
      float cw[kLocKMax];
#pragma unroll
      for (int k = 0; k < kLocKMax; ++k) cw[k] = l.cum[c0 + k];
      for (int s0 = c0; s0 < c1; s0 += kLocKMax) {
#pragma unroll
        for (int j = 0; j < kLocKMax; ++j) {
          const int s = s0 + j;
          if (s < c1) {
            const uint32_t kv = l.keys[(s * U) / 2 + lane];
            float x0 = bflo(kv) + qb0, x1 = bfhi(kv) + qb1;
#pragma unroll
            for (int k = 0; k < kLocKMax; ++k) {
              x0 += cw[(j + k) & 31] * wk[k][0];
              x1 += cw[(j + k) & 31] * wk[k][1];
            }
            float part = nv0 * tanh_fast(x0) + nv1 * tanh_fast(x1);
            part = wave_sum_dpp(part);
            if (lane == 0) l.e[s] = part;
            cw[j & 31] = s < S ? l.cum[s + kLocKMax] : 0.f;
          }
        }
      }
    }
  } else {
    AttnRow nxt;
    if constexpr (!RES) nxt = attn_row_fetch(p, b, max(min(wave, slen - 1), 0));
    for (int s = wave; s < slen; s += kAttnWaves) {
      const uint32_t* krow = l.keys + (RES ? (s * U) >> 1 : (wave * U) >> 1);
      if constexpr (!RES) {
        const AttnRow cur = nxt;
        nxt = attn_row_fetch(p, b, min(s + kAttnWaves, slen - 1));
        attn_row_put(p, l.keys + ((wave * U) >> 1), cur);
      }
      float part = 0.f;
      for (int u = 2 * lane; u < U; u += 128) {
        if (p.mode == 3) {        // Luong: score = keys . query (query = cell output, w_q = I)
          const uint32_t kv = krow[u >> 1];
          part += bflo(kv) * l.q[u] + bfhi(kv) * l.q[u + 1];
        } else {
          float x0, x1;
          attn_pre2(l, krow, u, x0, x1);
          part += l.nv[u] * tanh_fast(x0) + l.nv[u + 1] * tanh_fast(x1);
        }
      }
      part = wave_sum_dpp(part);
      if (lane == 0) l.e[s] = part;
    }
  }
  __syncthreads();
  AD_TICK(0, 3);
  // masked softmax over s < slen
  float mx = -INFINITY;
  for (int s = tid; s < slen; s += kAttnThreads) mx = fmaxf(mx, l.e[s]);
  mx = block_max(mx, l.red);
  float sum = 0.f;
  for (int s = tid; s < slen; s += kAttnThreads) {
    const float ex = __expf(l.e[s] - mx);
    l.e[s] = ex;
    sum += ex;
  }
  sum = block_sum(sum, l.red);
  const float inv = slen > 0 ? 1.f / sum : 0.f;
  float* al_out = p.align_seq + ((long long)b * p.T + p.t) * S;
  for (int s = tid; s < S; s += kAttnThreads) {
    const float a = s < slen ? l.e[s] * inv : 0.f;
    l.e[s] = a;
    al_out[s] = a;
    if (p.mode == 2) {
      const long long ci = ((long long)b * (p.T + 1) + p.t) * S + s;
      p.cum_seq[ci + S] = p.cum_seq[ci] + a;
    }
  }
  __syncthreads();
  AD_TICK(0, 4);
  // context = sum_s align[s] * values[b, s, :]: 8-column groups x nsplit slices of s
  const int CG = min(M / 8, kAttnThreads);
  const int nsplit = min(kAttnThreads / CG, kCtxSplitMax);
  float* part = l.scratch;   // [nsplit][M]
  for (int c0 = 0; c0 < M / 8; c0 += CG) {
    const int cg = c0 + tid % CG, sp = tid / CG;
    if (sp < nsplit && cg < M / 8) {
      float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const bf16_t* vp = p.values + (long long)b * S * M + cg * 8;
#pragma unroll 16
      for (int s = sp; s < slen; s += nsplit) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(vp + (long long)s * M);
        const float a = l.e[s];
#pragma unroll
        for (int e = 0; e < 4; ++e) { a8[2 * e] += a * bflo(v[e]); a8[2 * e + 1] += a * bfhi(v[e]); }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) part[sp * M + cg * 8 + e] = a8[e];
    }
  }
  __syncthreads();
  AD_TICK(0, 5);
  bf16_t* ctx = p.ctx + (long long)b * p.ctx_bs + (long long)p.t * p.ctx_ts;
  bf16_t* cat = p.cat0 + ((long long)b * (p.T + 1) + p.t + 1) * p.Kc0;
  for (int m8 = tid; m8 < M / 8; m8 += kAttnThreads) {
    float c8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      c8[e] = 0.f;
      for (int sp = 0; sp < nsplit; ++sp) c8[e] += part[sp * M + m8 * 8 + e];
    }
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack2bf(c8[2 * e], c8[2 * e + 1]);
    *reinterpret_cast<u32x4*>(ctx + m8 * 8) = o;
    if (p.attn_in_keep < 1.f) {
      const unsigned long long idx8 = (((unsigned long long)b * (p.T + 1) + p.t + 1) * M) / 8 + m8;
      const uint32_t bits = dropout_bits8(p.attn_in_seed, idx8, p.attn_in_keep);
      const float ik = 1.f / p.attn_in_keep;
#pragma unroll
      for (int e = 0; e < 8; ++e) c8[e] = ((bits >> e) & 1u) ? c8[e] * ik : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack2bf(c8[2 * e], c8[2 * e + 1]);
    }
    *reinterpret_cast<u32x4*>(cat + m8 * 8) = o;
  }
  AD_TICK(0, 6);
}

// ------------------------------------------------------------------ d(attention input) GEMM
struct AdDattn {
  int B, M, K;
  const bf16_t* wT;     // [M rows, K] (first M rows of Wcat0^T)
  const bf16_t* dg;     // rows: dg + b*ld
  long long ld;
  float* out;           // [B, M]
};
// Backward GEMMs: 32-row tiles, the reduction split over 16 waves so that every load of a
// wave (one 16-wide k-slice per 256 of K) is in flight at once.
constexpr int kBwdWaves = 16;

// sum the partial tiles of the 16 waves; wave q < 4 receives rows 8q + 4*(lane>>5) + e
// (e < 4) of the tile: out[e] += sum_w acc_w[4q + e]. Two passes of 8 registers keep the
// LDS buffer at 32 KB. `red`: kBwdWaves*8*64 floats.
__device__ __forceinline__ void tile_reduce_quarters16(const f32x16& acc, float* red, float (&out)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
#pragma unroll
    for (int r = 0; r < 8; ++r) red[(wave * 8 + r) * 64 + lane] = acc[ps * 8 + r];
    __syncthreads();
    if ((wave >> 1) == ps && wave < 4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float s = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < kBwdWaves; ++w2) s += red[(w2 * 8 + 4 * (wave & 1) + e) * 64 + lane];
        out[e] += s;
      }
    }
    __syncthreads();
  }
}

// 8 output rows per workgroup (rows 8..31 of the MFMA tile are padding): M = 512 attention
// inputs are 64 workgroups instead of 16.
__global__ __launch_bounds__(64 * kBwdWaves) void ad_dattn_kernel(AdDattn p) {
  __shared__ float red[kBwdWaves * 4 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int j0 = blockIdx.x * 8, b0 = blockIdx.y * 32;
  f32x16 accw;
#pragma unroll
  for (int e = 0; e < 16; ++e) accw[e] = 0.f;
  const bf16_t* wrow = (l31 < 8 && j0 + l31 < p.M) ? p.wT + (long long)(j0 + l31) * p.K : nullptr;
  const int brow = b0 + l31;
  const bf16_t* irow = brow < p.B ? p.dg + (long long)brow * p.ld : nullptr;
  tile_gemm_prefetch<kBwdWaves, 8>(wrow, irow, p.K, accw, p.wT);
  float acc[4];
  tile_reduce_rows8<kBwdWaves>(accw, red, acc);
  if (wave >= 1) return;
  const int b = b0 + l31, j = j0 + 4 * lhi;
  if (b >= p.B || j >= p.M) return;
  f32x4 o = {acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<f32x4*>(p.out + (long long)b * p.M + j) = o;
}

// The same product cut kDaSplit ways along the reduction, one FULL 32-row tile per workgroup and ONE
// round of loads per wave; the pieces of a tile meet through a ticket exactly as in
// ad_cell_bwd_split_kernel (deterministic: the last arriver sums the slabs in piece order).
// M = 512, K = 4096: 16 x 8 = 128 workgroups of one round instead of 64 of two.
constexpr int kDaSplit = 8;
constexpr int kDaWaves = 8;
constexpr int kDaSlices = 4;
constexpr int kDaSlabFloats = 16 * 64;

struct AdDattnSplit {
  AdDattn g;
  float* part;   // [M/32][B/32][kDaSplit][kDaSlabFloats]
  int* ticket;   // [M/32][B/32], zero before and after every launch
};

__global__ __launch_bounds__(64 * kDaWaves) void ad_dattn_split_kernel(AdDattnSplit ps) {
  const AdDattn& p = ps.g;
  __shared__ float red[kDaWaves * 16 * 64];       // 32 KB
  __shared__ int s_ticket;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mb = blockIdx.x, kq = blockIdx.y, bb = blockIdx.z;
  const int j0 = mb * 32, b0 = bb * 32;
  const bool vrow = j0 + l31 < p.M;
  const int brow = b0 + l31;
  const bool vcol = brow < p.B;
  const bf16_t* const wr = p.wT + (long long)(vrow ? j0 + l31 : 0) * p.K;
  const bf16_t* const gr = p.dg + (long long)(vcol ? brow : 0) * p.ld;
  const int nit = (p.K + 15) >> 4, nper = (nit + kDaSplit - 1) / kDaSplit;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int base = 0; base < nper; base += kDaWaves * kDaSlices) {
    u32x4 wa[kDaSlices], ga[kDaSlices];
#pragma unroll
    for (int i = 0; i < kDaSlices; ++i) {
      const int s = kq * nper + base + wave + kDaWaves * i;
      const int ko = min(s * 16 + lhi * 8, p.K - 8);
      wa[i] = *reinterpret_cast<const u32x4*>(wr + ko);
      ga[i] = *reinterpret_cast<const u32x4*>(gr + ko);
    }
#pragma unroll
    for (int i = 0; i < kDaSlices; ++i) {
      const int sl = base + wave + kDaWaves * i, s = kq * nper + sl;
      const bool kv = sl < nper && s < nit && s * 16 + lhi * 8 < p.K;
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, (kv && vrow) ? wa[i] : zero),
                                                    __builtin_bit_cast(bf16x8, (kv && vcol) ? ga[i] : zero), acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[r];
  __syncthreads();
  float* const slab0 = ps.part + ((size_t)(mb * gridDim.z + bb) * kDaSplit) * kDaSlabFloats;
#pragma unroll
  for (int q = 0; q < kDaSlabFloats / (64 * kDaWaves); ++q) {
    const int o = tid + 64 * kDaWaves * q;
    float s = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < kDaWaves; ++w2) s += red[w2 * 16 * 64 + o];
    slab0[(size_t)kq * kDaSlabFloats + o] = s;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int* const ticket = ps.ticket + mb * gridDim.z + bb;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_ticket = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (s_ticket != kDaSplit - 1) return;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  // wave g < 4: rows 8g + 4*lhi + e of the tile (accumulator registers 4g + e), column = sample l31
  if (wave >= 4 || !vcol) return;
  const int j = j0 + 8 * wave + 4 * lhi;
  if (j >= p.M) return;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  for (int pc = 0; pc < kDaSplit; ++pc) {
    const float* const sl = slab0 + (size_t)pc * kDaSlabFloats;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] += sl[(4 * wave + e) * 64 + lane];
  }
  *reinterpret_cast<f32x4*>(p.out + (long long)brow * p.M + j) = o;
}

// ------------------------------------------------------------------ attention backward
// sum over the 64 lanes of 32 per-lane values; lane L returns the total of value (L >> 1)
// same for 16 values: lane L returns the total of value (L >> 2)
__device__ __forceinline__ float wave_reduce16(float (&v)[16]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    const int off = 32 >> st, half = 8 >> st;
    const bool hi = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float send = hi ? v[i] : v[i + half];
      const float keep = hi ? v[i + half] : v[i];
      v[i] = keep + __shfl_xor(send, off, 64);
    }
  }
  float r = v[0] + __shfl_xor(v[0], 2, 64);
  return r + __shfl_xor(r, 1, 64);
}

__device__ __forceinline__ float wave_reduce32(float (&v)[32]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int st = 0; st < 5; ++st) {
    const int off = 32 >> st, half = 16 >> st;
    const bool hi = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float send = hi ? v[i] : v[i + half];
      const float keep = hi ? v[i + half] : v[i];
      v[i] = keep + __shfl_xor(send, off, 64);
    }
  }
  return v[0] + __shfl_xor(v[0], 1, 64);
}

// UP: unit pairs per lane of the non-location score loop (4: U <= 512, 8: U <= 1024); RES as in the forward
template <bool LOC, int UP = 4, bool RES = true>
__global__ __launch_bounds__(kAttnThreads) void ad_attn_bwd_kernel(AdAttn p) {
  static_assert(!LOC || RES, "location mode keeps its keys in LDS");
  extern __shared__ float lds_raw[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (p.tgt_len && p.t >= p.tgt_len[b]) return;
  const int H = p.H, M = p.M, U = p.U, S = p.S, K = p.loc_k;
  const AttnLds l = attn_lds_carve(lds_raw, H, U, S, p.mode, K, RES);
  float* dctx = l.scratch;            // [M]
  float* dal = dctx + M;              // [S]
  float* de = dal + S;                // [S]
  float* dcum_l = de + S;             // [S]   (mode 2)
  float* dqp = dcum_l + S;            // [waves][U]
  float* dnvp = dqp + kAttnWaves * U; // [waves][U]
  float* dwk_l = dnvp + kAttnWaves * U;   // [K][U]  (mode 2)
  const int slen = min(max(p.src_len[b], 0), S);
  const long long row = (long long)b * p.T + p.t;
  AD_TICK(1, 0);
  // total context gradient
  {
    const bf16_t* ext = p.dctx_ext ? p.dctx_ext + (long long)b * p.dctx_bs + (long long)p.t * p.dctx_ts : nullptr;
    for (int m8 = tid; m8 < M / 8; m8 += kAttnThreads) {
      float c8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (ext) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(ext + m8 * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) { c8[2 * e] = bflo(v[e]); c8[2 * e + 1] = bfhi(v[e]); }
      }
      if (!p.last) {
        const float* da = p.dattn + (long long)b * M + m8 * 8;
        uint32_t bits = 0xffu;
        float ik = 1.f;
        if (p.attn_in_keep < 1.f) {
          const unsigned long long idx8 = (((unsigned long long)b * (p.T + 1) + p.t + 1) * M) / 8 + m8;
          bits = dropout_bits8(p.attn_in_seed, idx8, p.attn_in_keep);
          ik = 1.f / p.attn_in_keep;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) if ((bits >> e) & 1u) c8[e] += da[e] * ik;
      }
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack2bf(c8[2 * e], c8[2 * e + 1]);
      *reinterpret_cast<u32x4*>(p.dctx_seq + row * M + m8 * 8) = o;
#pragma unroll
      for (int e = 0; e < 8; ++e) dctx[m8 * 8 + e] = c8[e];
    }
  }
  AD_TICK(1, 1);
  if constexpr (RES) attn_stage_keys(p, l, b, slen);
  for (int u = tid; u < U; u += kAttnThreads) l.q[u] = p.q_seq[row * U + u];
  for (int s = tid; s < S; s += kAttnThreads) l.e[s] = p.align_seq[row * S + s];
  if (p.mode == 2) {
    attn_load_cum(p, l, b);
    for (int s = tid; s < S; s += kAttnThreads) dcum_l[s] = p.dcum[(long long)b * S + s];
    for (int i = tid; i < K * U; i += kAttnThreads) dwk_l[i] = 0.f;
  }
  attn_load_score_params(p, l);   // barrier inside
  AD_TICK(1, 2);
  // dalign[s] = dctx . values[b,s,:] (+ carry of the cumulative-alignment state)
#pragma unroll 8
  for (int s = wave; s < slen; s += kAttnWaves) {
    float part = 0.f;
    const bf16_t* vp = p.values + ((long long)b * S + s) * M;
    for (int m = lane * 8; m < M; m += 512) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(vp + m);
#pragma unroll
      for (int e = 0; e < 4; ++e) part += bflo(v[e]) * dctx[m + 2 * e] + bfhi(v[e]) * dctx[m + 2 * e + 1];
    }
    part = wave_sum_dpp(part);
    if (lane == 0) dal[s] = part + (p.mode == 2 ? dcum_l[s] : 0.f);
  }
  __syncthreads();
  AD_TICK(1, 3);
  float dot = 0.f;
  for (int s = tid; s < slen; s += kAttnThreads) dot += l.e[s] * dal[s];
  dot = block_sum(dot, l.red);
  for (int s = tid; s < S; s += kAttnThreads) de[s] = s < slen ? l.e[s] * (dal[s] - dot) : 0.f;
  __syncthreads();
  AD_TICK(1, 4);
  // through the score: dpre[s,u] = de[s] * nv[u] * (1 - tanh^2)
  if constexpr (LOC) {
    // U == 128: a lane owns ONE unit; a pair of waves covers the 128 units of a contiguous
    // range of source positions. Three 32-entry register windows slide with s (slot
    // (j + k) & 31 at the j-th step of a 32-step block): cw = padded cumulative alignments,
    // gw = partial state gradient c_u[s - padl + k] = sum_k' dpre[s',u] Wck[k',u] (a lane-local
    // convolution along s; the sum over units happens once per emitted position), so the
    // loop needs one LDS read and one wave reduction per position.
    const int padl = (K - 1) / 2;
    const int u = (wave & 1) * 64 + lane, grp = wave >> 1, ngrp = kAttnWaves / 2;
    const int chunk = (slen + ngrp - 1) / ngrp;
    const int c0 = grp * chunk, c1 = min(c0 + chunk, slen);
    float dq0 = 0.f, dn0 = 0.f;
    if (c0 < c1) {
      float wk[kLocKMax], dwk[kLocKMax], cw[kLocKMax], gw[kLocKMax];
#pragma unroll
      for (int k = 0; k < kLocKMax; ++k) {
        dwk[k] = 0.f;
        gw[k] = 0.f;
        wk[k] = k < K ? p.wck[(long long)k * U + u] : 0.f;
        cw[k] = l.cum[c0 + k];
      }
      const float nv0 = l.nv[u], qb = l.q[u] + l.bs[u];
      const bf16_t* kl = reinterpret_cast<const bf16_t*>(l.keys) + u;
      bf16_t* dps = p.dpre_seq + (row * S) * U + u;   // dpre of this step: dkeys = sum over steps
      // run kLocKMax steps past the end so that every window slot is emitted
      for (int s0 = c0; s0 < c1 + kLocKMax; s0 += kLocKMax) {
#pragma unroll
        for (int j = 0; j < kLocKMax; ++j) {
          const int s = s0 + j;
          if (s < c1) {
            float x0 = bf2f(kl[s * U]) + qb;
#pragma unroll
            for (int k = 0; k < kLocKMax; ++k) x0 += cw[(j + k) & 31] * wk[k];
            const float t0 = tanh_fast(x0);
            const float des = de[s];
            const float d0 = des * nv0 * (1.f - t0 * t0);
            dq0 += d0;
            dn0 += des * t0;
            dps[(long long)s * U] = f2bf(d0);
#pragma unroll
            for (int k = 0; k < kLocKMax; ++k) {
              dwk[k] += cw[(j + k) & 31] * d0;
              gw[(j + k) & 31] += d0 * wk[k];
            }
          }
          if (s < c1 + kLocKMax) {
            // slot j is complete: it is the state gradient at position s - padl
            const float gsum = wave_sum_dpp(gw[j & 31]);
            gw[j & 31] = 0.f;
            const int s2 = s - padl;
            if (lane == 0 && s2 >= 0 && s2 < S) atomicAdd(&dcum_l[s2], gsum);
            cw[j & 31] = s < S ? l.cum[s + kLocKMax] : 0.f;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kLocKMax; ++k)
        if (k < K) atomicAdd(&dwk_l[k * U + u], dwk[k]);
    }
    dqp[wave * U + u] = dq0;
    dnvp[wave * U + u] = dn0;
    dqp[wave * U + (u ^ 64)] = 0.f;
    dnvp[wave * U + (u ^ 64)] = 0.f;
  } else {
    float dq_acc[2 * UP], dnv_acc[2 * UP];   // a lane owns the unit pairs 2 * lane + 128 * i, i < UP
#pragma unroll
    for (int i = 0; i < 2 * UP; ++i) { dq_acc[i] = 0.f; dnv_acc[i] = 0.f; }
    AttnRow nxt;
    if constexpr (!RES) nxt = attn_row_fetch(p, b, max(min(wave, slen - 1), 0));
    for (int s = wave; s < slen; s += kAttnWaves) {
      const uint32_t* krow = l.keys + (RES ? (s * U) >> 1 : (wave * U) >> 1);
      if constexpr (!RES) {
        const AttnRow cur = nxt;
        nxt = attn_row_fetch(p, b, min(s + kAttnWaves, slen - 1));
        attn_row_put(p, l.keys + ((wave * U) >> 1), cur);
      }
      const float des = de[s];
#pragma unroll
      for (int i = 0; i < UP; ++i) {
        const int u = 2 * lane + 128 * i;
        if (u < U) {
          if (p.mode == 3) {      // Luong: d score / d key = query, d score / d query = key
            const uint32_t kv = krow[u >> 1];
            dq_acc[2 * i] += des * bflo(kv);
            dq_acc[2 * i + 1] += des * bfhi(kv);
            *reinterpret_cast<uint32_t*>(p.dpre_seq + (row * S + s) * U + u) =
                pack2bf(des * l.q[u], des * l.q[u + 1]);
          } else {
            float x0, x1;
            attn_pre2(l, krow, u, x0, x1);
            const float t0 = tanh_fast(x0), t1 = tanh_fast(x1);
            const float d0 = des * l.nv[u] * (1.f - t0 * t0), d1 = des * l.nv[u + 1] * (1.f - t1 * t1);
            dq_acc[2 * i] += d0;
            dq_acc[2 * i + 1] += d1;
            dnv_acc[2 * i] += des * t0;
            dnv_acc[2 * i + 1] += des * t1;
            *reinterpret_cast<uint32_t*>(p.dpre_seq + (row * S + s) * U + u) = pack2bf(d0, d1);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < UP; ++i) {
      const int u = 2 * lane + 128 * i;
      if (u < U) {
        dqp[wave * U + u] = dq_acc[2 * i]; dqp[wave * U + u + 1] = dq_acc[2 * i + 1];
        dnvp[wave * U + u] = dnv_acc[2 * i]; dnvp[wave * U + u + 1] = dnv_acc[2 * i + 1];
      }
    }
  }
  __syncthreads();
  AD_TICK(1, 5);
  for (int u = tid; u < U; u += kAttnThreads) {
    float dq = 0.f, dn = 0.f;
#pragma unroll
    for (int w = 0; w < kAttnWaves; ++w) { dq += dqp[w * U + u]; dn += dnvp[w * U + u]; }
    p.dq_seq[row * U + u] = f2bf(dq);
    p.dnv_acc[(long long)b * U + u] += dn;
    if (p.mode == 2) p.dbd_acc[(long long)b * U + u] += dq;
  }
  if (p.mode == 2) {
    for (int s = tid; s < S; s += kAttnThreads) p.dcum[(long long)b * S + s] = dcum_l[s];
    float* dwa = p.dwck_acc + (long long)b * K * U;
    for (int i = tid; i < K * U; i += kAttnThreads) dwa[i] += dwk_l[i];
  }
  __syncthreads();
  AD_TICK(1, 6);
  // d(query input) = dq . Wq runs on the matrix cores inside the top cell's backward kernel
}

// ------------------------------------------------------------------ location-sensitive attention, split
// The one-workgroup-per-sample kernels above spend their time in VALU work on ONE compute unit
// (scores: 200 positions x 128 units x (32 location taps + tanh); their gradient: three times that)
// and in memory round trips nothing overlaps (Wq: 256 KB per sample, values: 410 KB per sample, both
// L2-cold after the cell kernels streamed 32 MB of weights). For the location-sensitive mode
// (U == 128) a step is therefore cut over kLocParts x B workgroups by UNITS and over kLocCtxParts x B
// by context columns / source positions:
//   forward : ad_loc_scores_kernel   (part, b): q and the partial scores of 32 units, all positions
//             ad_loc_context_kernel  (cols, b): sum of the partial scores, masked softmax, alignments /
//                                               cumulative alignments, context columns
//   backward: ad_loc_dalign_kernel   (rows, b): total context gradient, d(alignment) of a range of positions
//             ad_loc_score_bwd_kernel(part, b): softmax backward, score gradient of 32 units
// A unit's quantities (q, dq, dnv, dWck column, dpre column) have ONE owner; what is summed over
// units crosses workgroups through small global buffers written by their owners and summed by the
// next kernel in a fixed order (partial scores [B, parts, S]; partial state gradients [B, parts, S]):
// no atomics on global memory, no spinning.
constexpr int kLocStreams = 16;     // position streams per workgroup: a half wave = the 32 units of a stream

// sum over the 32 lanes of a half wave; valid in lanes 16..31 of each half
__device__ __forceinline__ float half_sum_dpp(float x) {
  x += dpp_mov<0xB1, 0xf>(0.f, x);    // quad_perm [1,0,3,2]
  x += dpp_mov<0x4E, 0xf>(0.f, x);    // quad_perm [2,3,0,1]
  x += dpp_mov<0x124, 0xf>(0.f, x);   // row_ror:4
  x += dpp_mov<0x128, 0xf>(0.f, x);   // row_ror:8
  x += dpp_mov<0x142, 0xa>(0.f, x);   // row_bcast:15 into rows 1, 3
  return x;
}

__host__ __device__ inline size_t loc_fwd_lds_floats(int H, int S) {
  return (size_t)H + 3 * kLocUnits + (S + kLocKMax) + (size_t)S * kLocUnits / 2 + 64;
}

__device__ __forceinline__ void ad_loc_scores_body(const AdAttn& p, const AdLoc& x) {
  extern __shared__ float lds_raw[];
  const int part = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (p.tgt_len && p.t >= p.tgt_len[b]) return;
  const int H = p.H, U = p.U, S = p.S, K = p.loc_k;
  float* hq = lds_raw;
  float* q = hq + H;
  float* nv = q + kLocUnits;
  float* bs = nv + kLocUnits;
  float* cum = bs + kLocUnits;                                   // [S + kLocKMax], zero padded
  uint16_t* keys = reinterpret_cast<uint16_t*>(cum + S + kLocKMax);   // [S][32] bf16
  const int slen = min(max(p.src_len[b], 0), S);
  const int u0 = part * kLocUnits;
  const long long row = (long long)b * p.T + p.t;
  // this wave's rows of Wq do not depend on anything staged below: requested first, so that their round trip
  // overlaps the staging (and its barrier) instead of following it
  constexpr int UB = kLocUnits / kAttnWaves;
  u32x4 wv0[UB][2];
#pragma unroll
  for (int i = 0; i < UB; ++i)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
      wv0[i][hh] = *reinterpret_cast<const u32x4*>(p.wq + (long long)(u0 + wave * UB + i) * H +
                                                   min(lane * 8 + 512 * hh, H - 8));
  __builtin_amdgcn_sched_barrier(0);
  // query input, this part's key columns (64 B per position), padded cumulative alignments
  const bf16_t* yq = p.yq + (long long)b * p.yq_bs + (long long)p.t * p.yq_ts;
  for (int h8 = tid; h8 < H / 8; h8 += kAttnThreads) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(yq + h8 * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) { hq[h8 * 8 + 2 * e] = bflo(v[e]); hq[h8 * 8 + 2 * e + 1] = bfhi(v[e]); }
  }
  {
    const bf16_t* kb = p.keys + (long long)b * S * U + u0;
    for (int i = tid; i < slen * 4; i += kAttnThreads) {
      const int sp = i >> 2, c = i & 3;
      *reinterpret_cast<u32x4*>(keys + sp * kLocUnits + c * 8) =
          *reinterpret_cast<const u32x4*>(kb + (long long)sp * U + c * 8);
    }
    const int padl = (K - 1) / 2;
    const float* cs = p.cum_seq + ((long long)b * (p.T + 1) + p.t) * S;
    for (int i = tid; i < S + kLocKMax; i += kAttnThreads) {
      const int sp = i - padl;
      cum[i] = (sp >= 0 && sp < S) ? cs[sp] : 0.f;
    }
  }
  if (tid < kLocUnits) {
    const int u = u0 + tid;
    nv[tid] = p.v[u];
    bs[tid] = ((p.use_bias && p.bias) ? p.bias[u] : 0.f) + p.wck[(long long)K * U + u];
  }
  __syncthreads();
  // q[u] = hq . Wq[u, :] for the 32 units of the part: 4 units per wave
  {
    float acc[UB];
#pragma unroll
    for (int i = 0; i < UB; ++i) acc[i] = 0.f;
    for (int h = lane * 8; h < H; h += 1024) {
      u32x4 wv[UB][2];
#pragma unroll
      for (int i = 0; i < UB; ++i)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
          wv[i][hh] = h == lane * 8 ? wv0[i][hh]
                                    : *reinterpret_cast<const u32x4*>(p.wq + (long long)(u0 + wave * UB + i) * H +
                                                                      min(h + 512 * hh, H - 8));
#pragma unroll
      for (int i = 0; i < UB; ++i)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
          if (h + 512 * hh < H) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              acc[i] += bflo(wv[i][hh][e]) * hq[h + 512 * hh + 2 * e] + bfhi(wv[i][hh][e]) * hq[h + 512 * hh + 2 * e + 1];
          }
    }
#pragma unroll
    for (int i = 0; i < UB; ++i) {
      const float sq = wave_sum_dpp(acc[i]);
      if (lane == 0) {
        q[wave * UB + i] = sq;
        p.q_seq[row * U + u0 + wave * UB + i] = sq;
      }
    }
  }
  __syncthreads();
  // partial scores: a half wave = the 32 units of one stream of positions; 32-entry register window
  // over the padded cumulative alignments (slot (j + k) & 31 holds cum[s + k] at the j-th step of a
  // 32-step block: one new LDS read per position)
  const int ul = lane & 31, st = wave * 2 + (lane >> 5);
  float wk[kLocKMax];
#pragma unroll
  for (int k = 0; k < kLocKMax; ++k) wk[k] = k < K ? p.wck[(long long)k * U + u0 + ul] : 0.f;
  const int chunk = (slen + kLocStreams - 1) / kLocStreams;
  const int c0 = st * chunk, c1 = min(c0 + chunk, slen);
  const float qb = q[ul] + bs[ul], nv0 = nv[ul];
  float* eo = x.e_part + ((long long)b * kLocParts + part) * S;
  float cw[kLocKMax];
#pragma unroll
  for (int k = 0; k < kLocKMax; ++k) cw[k] = cum[min(c0, S) + k];
  for (int i0 = 0; i0 < chunk; i0 += kLocKMax) {        // uniform trip count: the streams stay in step
#pragma unroll
    for (int j = 0; j < kLocKMax; ++j) {
      const int sp = c0 + i0 + j;
      if (i0 + j < chunk) {
        float x0 = qb;
        if (sp < c1) x0 += bf2f(keys[sp * kLocUnits + ul]);
#pragma unroll
        for (int k = 0; k < kLocKMax; ++k) x0 += cw[(j + k) & 31] * wk[k];
        float pr = half_sum_dpp(nv0 * tanh_fast(x0));
        if (ul == 31 && sp < c1) eo[sp] = pr;
        cw[j & 31] = sp < S ? cum[sp + kLocKMax] : 0.f;
      }
    }
  }
}

__global__ __launch_bounds__(kAttnThreads) void ad_loc_scores_kernel(AdAttn p, AdLoc x) { ad_loc_scores_body(p, x); }
// sum of the partial scores -> masked softmax -> alignments (+ cumulative) -> context columns
__global__ __launch_bounds__(256) void ad_loc_context_kernel(AdAttn p, AdLoc x, int ncg, int nsp) {
  extern __shared__ float lds_raw[];
  const int cpart = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (p.tgt_len && p.t >= p.tgt_len[b]) {
    if (cpart == 0) attn_carry_cum(p, b);
    return;
  }
  const int M = p.M, S = p.S;
  float* e = lds_raw;                  // [S]
  float* red = e + S;                  // [8]
  float* part = red + 8;               // [nsp][ncg * 8]
  const int slen = min(max(p.src_len[b], 0), S);
  const float* ep = x.e_part + (long long)b * kLocParts * S;
  float mx = -INFINITY;
  for (int sp = tid; sp < slen; sp += 256) {
    float v = ep[sp];
#pragma unroll
    for (int q = 1; q < kLocParts; ++q) v += ep[q * S + sp];
    e[sp] = v;
    mx = fmaxf(mx, v);
  }
  mx = wave_max_dpp(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
  for (int sp = tid; sp < slen; sp += 256) {
    const float ex = __expf(e[sp] - mx);
    e[sp] = ex;
    sum += ex;
  }
  sum = wave_sum_dpp(sum);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = sum;
  __syncthreads();
  sum = red[4] + red[5] + red[6] + red[7];
  const float inv = slen > 0 ? 1.f / sum : 0.f;
  const long long row = (long long)b * p.T + p.t;
  for (int sp = tid; sp < S; sp += 256) {
    const float a = sp < slen ? e[sp] * inv : 0.f;
    e[sp] = a;
    if (cpart == 0) {
      p.align_seq[row * S + sp] = a;
      const long long ci = ((long long)b * (p.T + 1) + p.t) * S + sp;
      p.cum_seq[ci + S] = p.cum_seq[ci] + a;
    }
  }
  __syncthreads();
  // context columns [cpart * ncg * 8, + ncg * 8): thread = (8-column group, slice of the positions)
  const int MQ = ncg * 8, m0 = cpart * MQ;
  const int cg = tid % ncg, sq = tid / ncg;
  if (sq < nsp) {
    float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bf16_t* vp = p.values + (long long)b * S * M + m0 + cg * 8;
#pragma unroll 8
    for (int sp = sq; sp < slen; sp += nsp) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(vp + (long long)sp * M);
      const float a = e[sp];
#pragma unroll
      for (int k = 0; k < 4; ++k) { a8[2 * k] += a * bflo(v[k]); a8[2 * k + 1] += a * bfhi(v[k]); }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) part[sq * MQ + cg * 8 + k] = a8[k];
  }
  __syncthreads();
  if (tid < ncg) {
    float c8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      c8[k] = 0.f;
      for (int q = 0; q < nsp; ++q) c8[k] += part[q * MQ + tid * 8 + k];
    }
    const int m8 = (m0 >> 3) + tid;
    bf16_t* ctx = p.ctx + (long long)b * p.ctx_bs + (long long)p.t * p.ctx_ts;
    bf16_t* cat = p.cat0 + ((long long)b * (p.T + 1) + p.t + 1) * p.Kc0;
    u32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = pack2bf(c8[2 * k], c8[2 * k + 1]);
    *reinterpret_cast<u32x4*>(ctx + m8 * 8) = o;
    if (p.attn_in_keep < 1.f) {
      const unsigned long long idx8 = (((unsigned long long)b * (p.T + 1) + p.t + 1) * M) / 8 + m8;
      const uint32_t bits = dropout_bits8(p.attn_in_seed, idx8, p.attn_in_keep);
      const float ik = 1.f / p.attn_in_keep;
#pragma unroll
      for (int k = 0; k < 8; ++k) c8[k] = ((bits >> k) & 1u) ? c8[k] * ik : 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = pack2bf(c8[2 * k], c8[2 * k + 1]);
    }
    *reinterpret_cast<u32x4*>(cat + m8 * 8) = o;
  }
}

// total context gradient of the step (every workgroup of a sample computes it; part 0 stores it) and
// d(alignment)[s] = dctx . values[b, s, :] + carried state gradient, for a range of positions. The
// state-gradient carry dcum[b, s] is owned here: dcum += the previous backward step's per-part
// contributions, summed in part order.
__global__ __launch_bounds__(256) void ad_loc_dalign_kernel(AdAttn p, AdLoc x) {
  extern __shared__ float lds_raw[];
  const int rp = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (p.tgt_len && p.t >= p.tgt_len[b]) return;
  const int M = p.M, S = p.S;
  float* dctx = lds_raw;   // [M]
  const int slen = min(max(p.src_len[b], 0), S);
  const long long row = (long long)b * p.T + p.t;
  const bf16_t* ext = p.dctx_ext ? p.dctx_ext + (long long)b * p.dctx_bs + (long long)p.t * p.dctx_ts : nullptr;
  for (int m8 = tid; m8 < M / 8; m8 += 256) {
    float c8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ext) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(ext + m8 * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) { c8[2 * e] = bflo(v[e]); c8[2 * e + 1] = bfhi(v[e]); }
    }
    if (!p.last) {
      const float* da = p.dattn + (long long)b * M + m8 * 8;
      uint32_t bits = 0xffu;
      float ik = 1.f;
      if (p.attn_in_keep < 1.f) {
        const unsigned long long idx8 = (((unsigned long long)b * (p.T + 1) + p.t + 1) * M) / 8 + m8;
        bits = dropout_bits8(p.attn_in_seed, idx8, p.attn_in_keep);
        ik = 1.f / p.attn_in_keep;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) if ((bits >> e) & 1u) c8[e] += da[e] * ik;
    }
    if (rp == 0) {
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack2bf(c8[2 * e], c8[2 * e + 1]);
      *reinterpret_cast<u32x4*>(p.dctx_seq + row * M + m8 * 8) = o;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) dctx[m8 * 8 + e] = c8[e];
  }
  __syncthreads();
  const int chunk = (S + kLocCtxParts - 1) / kLocCtxParts;
  const int c0 = rp * chunk, c1 = min(c0 + chunk, S);
  // the state-gradient carry of this range (all S: positions past slen still receive contributions
  // through the filter's halo, they are never read back into a live alignment)
  float* carry = dctx + M;   // [chunk]
  for (int sp = c0 + tid; sp < c1; sp += 256) {
    float d = p.dcum[(long long)b * S + sp];
    const float* dp = x.dcum_part + (long long)b * kLocParts * S + sp;
#pragma unroll
    for (int q = 0; q < kLocParts; ++q) d += dp[q * S];
    p.dcum[(long long)b * S + sp] = d;
    carry[sp - c0] = d;
  }
  __syncthreads();
  const int e1 = min(c1, slen);
#pragma unroll 4
  for (int sp = c0 + wave; sp < e1; sp += 4) {
    float pr = 0.f;
    const bf16_t* vp = p.values + ((long long)b * S + sp) * M;
    for (int m = lane * 8; m < M; m += 512) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(vp + m);
#pragma unroll
      for (int e = 0; e < 4; ++e) pr += bflo(v[e]) * dctx[m + 2 * e] + bfhi(v[e]) * dctx[m + 2 * e + 1];
    }
    pr = wave_sum_dpp(pr);
    if (lane == 0) x.dal[(long long)b * S + sp] = pr + carry[sp - c0];
  }
}

// state-gradient slots a stream emits: its chunk of positions + one filter width, in whole 32-step blocks
__host__ __device__ inline int loc_bwd_slab_pitch(int S) {
  const int chunk = (S + kLocStreams - 1) / kLocStreams;
  return ((chunk + kLocKMax + kLocKMax - 1) / kLocKMax) * kLocKMax;
}
__host__ __device__ inline size_t loc_bwd_lds_floats(int S, int K) {
  // q, nv, bs | e, dal, de | cum (padded) | dcum_l (padded) | dwk_l per stream | dqp, dnvp | red | keys | dslab
  return (size_t)3 * kLocUnits + 3 * S + (S + kLocKMax) + (S + 2 * kLocKMax) +
         (size_t)kLocStreams * K * kLocUnits + 2 * (size_t)kLocStreams * kLocUnits + 64 + (size_t)S * kLocUnits / 2 +
         (size_t)kLocStreams * loc_bwd_slab_pitch(S);
}

__global__ __launch_bounds__(kAttnThreads) void ad_loc_score_bwd_kernel(AdAttn p, AdLoc x) {
  extern __shared__ float lds_raw[];
  const int part = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (p.tgt_len && p.t >= p.tgt_len[b]) return;
  const int U = p.U, S = p.S, K = p.loc_k;
  float* q = lds_raw;
  float* nv = q + kLocUnits;
  float* bs = nv + kLocUnits;
  float* e = bs + kLocUnits;                 // [S] alignments
  float* dal = e + S;                        // [S]
  float* de = dal + S;                       // [S]
  float* cum = de + S;                       // [S + kLocKMax]
  float* dcum_l = cum + S + kLocKMax;        // [S + 2 kLocKMax]: index = position + kLocKMax
  float* dwk_l = dcum_l + S + 2 * kLocKMax;  // [streams][K][32]: every stream's filter-gradient columns
  float* dqp = dwk_l + kLocStreams * K * kLocUnits;   // [streams][32]
  float* dnvp = dqp + kLocStreams * kLocUnits;
  float* red = dnvp + kLocStreams * kLocUnits;
  uint16_t* keys = reinterpret_cast<uint16_t*>(red + 64);
  // [streams][pitch]: the state-gradient slots of every stream, summed over the streams in order below
  // (an LDS float atomic per slot let up to four streams race on one position: last-bit differences
  // from run to run)
  float* dslab = red + 64 + (size_t)S * kLocUnits / 2;
  const int spitch = loc_bwd_slab_pitch(S);
  const int slen = min(max(p.src_len[b], 0), S);
  const int u0 = part * kLocUnits;
  const long long row = (long long)b * p.T + p.t;
  AD_TICK(1, 0);
  {
    const bf16_t* kb = p.keys + (long long)b * S * U + u0;
    for (int i = tid; i < slen * 4; i += kAttnThreads) {
      const int sp = i >> 2, c = i & 3;
      *reinterpret_cast<u32x4*>(keys + sp * kLocUnits + c * 8) =
          *reinterpret_cast<const u32x4*>(kb + (long long)sp * U + c * 8);
    }
    const int padl = (K - 1) / 2;
    const float* cs = p.cum_seq + ((long long)b * (p.T + 1) + p.t) * S;
    for (int i = tid; i < S + kLocKMax; i += kAttnThreads) {
      const int sp = i - padl;
      cum[i] = (sp >= 0 && sp < S) ? cs[sp] : 0.f;
    }
    for (int sp = tid; sp < S; sp += kAttnThreads) {
      e[sp] = p.align_seq[row * S + sp];
      dal[sp] = sp < slen ? x.dal[(long long)b * S + sp] : 0.f;
    }
  }
  if (tid < kLocUnits) {
    const int u = u0 + tid;
    q[tid] = p.q_seq[row * U + u];
    nv[tid] = p.v[u];
    bs[tid] = ((p.use_bias && p.bias) ? p.bias[u] : 0.f) + p.wck[(long long)K * U + u];
  }
  __syncthreads();
  AD_TICK(1, 1);
  float dot = 0.f;
  for (int sp = tid; sp < slen; sp += kAttnThreads) dot += e[sp] * dal[sp];
  dot = block_sum(dot, red);
  for (int sp = tid; sp < S; sp += kAttnThreads) de[sp] = sp < slen ? e[sp] * (dal[sp] - dot) : 0.f;
  __syncthreads();
  AD_TICK(1, 2);
  // score gradient of this part's 32 units: three 32-entry register windows slide with s (slot
  // (j + k) & 31 at the j-th step of a block): cw = padded cumulative alignments, gw = partial state
  // gradient sum_k' dpre[s', u] Wck[k', u] (lane-local along s; the sum over the 32 units once per
  // emitted position), dwk = the filter-gradient column of the unit
  const int padl = (K - 1) / 2;
  const int ul = lane & 31, st = wave * 2 + (lane >> 5), u = u0 + ul;
  const int chunk = (slen + kLocStreams - 1) / kLocStreams;
  const int c0 = st * chunk, c1 = min(c0 + chunk, slen);
  float dq0 = 0.f, dn0 = 0.f;
  {
    float wk[kLocKMax], dwk[kLocKMax], cw[kLocKMax], gw[kLocKMax];
#pragma unroll
    for (int k = 0; k < kLocKMax; ++k) {
      dwk[k] = 0.f;
      gw[k] = 0.f;
      wk[k] = k < K ? p.wck[(long long)k * U + u] : 0.f;
      cw[k] = cum[min(c0, S) + k];
    }
    const float nv0 = nv[ul], qb = q[ul] + bs[ul];
    bf16_t* dps = p.dpre_seq + (row * S) * U + u;
    // chunk + kLocKMax steps: the last kLocKMax only emit the remaining window slots. The branch
    // around the arithmetic is WAVE-uniform (the lower stream of the wave still has a position; the
    // upper stream runs with a zero score gradient once it is past its range): a per-lane branch here
    // made the compiler spill the four register windows (3.7 KB of scratch per lane)
    const int c0a = __builtin_amdgcn_readfirstlane(wave * 2 * chunk);
    for (int i0 = 0; i0 < chunk + kLocKMax; i0 += kLocKMax) {
#pragma unroll
      for (int j = 0; j < kLocKMax; ++j) {
        const int i = i0 + j, sp = c0 + i;
        {   // (whole 32-step blocks: the steps past chunk + kLocKMax emit zero slots — a second branch
            //  level around this body made the compiler spill the register windows: 3.6 KB of scratch)
          if (i < chunk && c0a + i < slen) {
            const bool on = sp < c1;
            float x0 = (on ? bf2f(keys[sp * kLocUnits + ul]) : 0.f) + qb;
#pragma unroll
            for (int k = 0; k < kLocKMax; ++k) x0 += cw[(j + k) & 31] * wk[k];
            const float t0 = tanh_fast(x0);
            const float des = on ? de[sp] : 0.f;
            const float d0 = des * nv0 * (1.f - t0 * t0);
            dq0 += d0;
            dn0 += des * t0;
            if (on) dps[(long long)sp * U] = f2bf(d0);
#pragma unroll
            for (int k = 0; k < kLocKMax; ++k) {
              dwk[k] += cw[(j + k) & 31] * d0;
              gw[(j + k) & 31] += d0 * wk[k];
            }
          }
          // slot j is complete: the state gradient at position sp - padl (of this stream's range)
          const float gsum = half_sum_dpp(gw[j & 31]);
          gw[j & 31] = 0.f;
          if (ul == 31 && i < spitch) dslab[st * spitch + i] = gsum;      // position c0 + i - padl
          cw[j & 31] = sp < S ? cum[min(sp, S) + kLocKMax] : 0.f;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kLocKMax; ++k)
      if (k < K) dwk_l[(st * K + k) * kLocUnits + ul] = dwk[k];     // summed over the streams below, in order
  }
  AD_TICK(1, 3);
  dqp[st * kLocUnits + ul] = dq0;
  dnvp[st * kLocUnits + ul] = dn0;
  __syncthreads();
  AD_TICK(1, 4);
  if (tid < kLocUnits) {
    float dq = 0.f, dn = 0.f;
#pragma unroll
    for (int w = 0; w < kLocStreams; ++w) { dq += dqp[w * kLocUnits + tid]; dn += dnvp[w * kLocUnits + tid]; }
    p.dq_seq[row * U + u0 + tid] = f2bf(dq);
    p.dnv_acc[(long long)b * U + u0 + tid] += dn;
    p.dbd_acc[(long long)b * U + u0 + tid] += dq;
  }
  float* dpo = x.dcum_part + ((long long)b * kLocParts + part) * S;
  {
    // position sp was slot sp + padl - w * chunk of stream w (slots 0 .. nemit - 1 were written by every stream)
    const int nemit = ((chunk + 2 * kLocKMax - 1) / kLocKMax) * kLocKMax;
    for (int sp = tid; sp < S; sp += kAttnThreads) {
      float a = 0.f;
      for (int w = 0; w < kLocStreams; ++w) {
        const int i = sp + padl - w * chunk;
        if (i >= 0 && i < nemit) a += dslab[w * spitch + i];
      }
      dpo[sp] = a;
    }
  }
  float* dwa = p.dwck_acc + (long long)b * K * U;
  for (int i = tid; i < K * kLocUnits; i += kAttnThreads) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < kLocStreams; ++w) a += dwk_l[w * K * kLocUnits + i];
    dwa[(i / kLocUnits) * U + u0 + (i % kLocUnits)] += a;
  }
  AD_TICK(1, 5);
  AD_TICK(1, 6);
}

// ---- score gradient of the location-sensitive attention on the matrix cores ------------------------------------
// ad_loc_score_bwd_kernel's arithmetic (softmax backward, score gradient of one 32-unit part of one sample) with its
// 36 KB of unrolled register-window code replaced by four small MFMA products:
//   x[s,u]     = keys + q + bias + sum_k cum[s+k-p] Wck[k,u]            (as the forward: A = Toeplitz rows of cum)
//   d0[s,u]    = de[s] v[u] (1 - tanh^2 x)                               -> dpre_seq (bf16), dq = sum_s d0, dv += sum_s de tanh x
//   dWck[k,u] += sum_s cum[s+k-p] d0[s,u]        A = Toeplitz COLUMNS of cum (taps x positions), B = d0^T[u][s]
//   G[s,k]     = sum_u d0[s,u] Wck[k,u]          A = d0[s][u], B = Wck;   dcum[c] = sum_k G[c + p - k][k]
// every operand bf16 hi + lo (three MFMAs per product). Waves 0-3 own the four 16x16 tiles of dWck over all
// positions, waves 4-7 the position tiles of G: no cross-wave sums, fixed summation order (deterministic).
constexpr int kSbD0sPitch = 40;                      // bf16 elements per position row of d0[s][u]
__host__ __device__ inline size_t ad_score_bwd_mfma_lds_floats(int S) {
  const size_t Sp = ((size_t)S + 31) & ~(size_t)31;
  return 64 + (Sp + 48) + 3 * Sp + Sp * kLocUnits / 2 + Sp * kSbD0sPitch + (size_t)kLocUnits * (Sp + 8) +
         Sp * 33 + 2 * (size_t)kAttnWaves * 4 * kLocUnits + 64;
}

__global__ __launch_bounds__(kAttnThreads) void ad_loc_score_bwd_mfma_kernel(AdAttn p, AdLoc x) {
  extern __shared__ float lds_raw[];
  const int part = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int U = p.U, S = p.S, K = p.loc_k;
  const int Sp = (S + 31) & ~31, TP = Sp + 8;
  float* qb = lds_raw;                               // [32]
  float* nv = qb + kLocUnits;                        // [32]
  float* cum = nv + kLocUnits;                       // [Sp + 48] zero padded, cum[i] = cumulative[i - padl]
  float* de = cum + Sp + 48;                         // [Sp] softmax-backward of the alignments, zero past the length
  float* ea = de + Sp;                               // [Sp] alignments   (scratch of the preamble)
  float* da = ea + Sp;                               // [Sp] d(alignment)
  uint16_t* keys = reinterpret_cast<uint16_t*>(da + Sp);                    // [Sp][32] bf16
  uint16_t* d0s_hi = keys + (size_t)Sp * kLocUnits;                         // [Sp][40] bf16: d0[s][u]
  uint16_t* d0s_lo = d0s_hi + (size_t)Sp * kSbD0sPitch;
  uint16_t* d0t_hi = d0s_lo + (size_t)Sp * kSbD0sPitch;                     // [32][Sp + 8] bf16: d0^T[u][s]
  uint16_t* d0t_lo = d0t_hi + (size_t)kLocUnits * TP;
  float* G = reinterpret_cast<float*>(d0t_lo + (size_t)kLocUnits * TP);     // [Sp][33]
  float* pq = G + (size_t)Sp * 33;                   // [waves][4][32] partial dq
  float* pn = pq + kAttnWaves * 4 * kLocUnits;       // [waves][4][32] partial dv terms
  float* red = pn + kAttnWaves * 4 * kLocUnits;      // [64]
  const int slen = min(max(p.src_len[b], 0), S);
  const int u0 = part * kLocUnits;
  const long long row = (long long)b * p.T + p.t;
  const int padl = (K - 1) / 2;
  const int r16 = lane & 15, kb = lane >> 4;
  // the folded location filter: forward B operand (taps x units) ...
  float wf[2][8];
#pragma unroll
  for (int ut = 0; ut < 2; ++ut)
#pragma unroll
    for (int j = 0; j < 8; ++j) wf[ut][j] = p.wck[(long long)min(kb * 8 + j, K - 1) * U + u0 + ut * 16 + r16];
  // ... and as the B operand of G (units x taps): tap = nt * 16 + r16, units kb * 8 ... + 8 (contiguous)
  float wg[2][8];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const float* wr = p.wck + (long long)min(nt * 16 + r16, K - 1) * U + u0 + kb * 8;
    const f32x4 a = *reinterpret_cast<const f32x4*>(wr), c = *reinterpret_cast<const f32x4*>(wr + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { wg[nt][j] = a[j]; wg[nt][4 + j] = c[j]; }
  }
  {
    const float* cs = p.cum_seq + ((long long)b * (p.T + 1) + p.t) * S;
    for (int i = tid; i < Sp + 48; i += kAttnThreads) {
      const int sp = i - padl;
      cum[i] = (sp >= 0 && sp < S) ? cs[sp] : 0.f;
    }
    const bf16_t* kp = p.keys + (long long)b * S * U + u0;
    for (int i = tid; i < slen * 4; i += kAttnThreads) {
      const int sp = i >> 2, c = i & 3;
      *reinterpret_cast<u32x4*>(keys + sp * kLocUnits + c * 8) = *reinterpret_cast<const u32x4*>(kp + (long long)sp * U + c * 8);
    }
    for (int sp = tid; sp < Sp; sp += kAttnThreads) {
      ea[sp] = sp < slen ? p.align_seq[row * S + sp] : 0.f;
      da[sp] = sp < slen ? x.dal[(long long)b * S + sp] : 0.f;
    }
  }
  if (tid < kLocUnits) {
    const int u = u0 + tid;
    qb[tid] = p.q_seq[row * U + u] + ((p.use_bias && p.bias) ? p.bias[u] : 0.f) + p.wck[(long long)K * U + u];
    nv[tid] = p.v[u];
  }
  __syncthreads();
  // softmax backward: de[s] = a[s] (dal[s] - sum_s' a[s'] dal[s'])
  float dot = 0.f;
  for (int sp = tid; sp < slen; sp += kAttnThreads) dot += ea[sp] * da[sp];
  dot = block_sum(dot, red);
  for (int sp = tid; sp < Sp; sp += kAttnThreads) de[sp] = sp < slen ? ea[sp] * (da[sp] - dot) : 0.f;
  bf16x8 bh[2], bl[2];
#pragma unroll
  for (int ut = 0; ut < 2; ++ut)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float w = kb * 8 + j < K ? wf[ut][j] : 0.f;
      const __bf16 hi = (__bf16)w;
      bh[ut][j] = hi;
      bl[ut][j] = (__bf16)(w - (float)hi);
    }
  __syncthreads();
  // ---- phase A: score gradient of every 16-position tile (all tiles up to Sp: dead ones write zeros) ----------
  const float q0 = qb[r16], q1 = qb[16 + r16], v0 = nv[r16], v1 = nv[16 + r16];
  float dq0 = 0.f, dq1 = 0.f, dn0 = 0.f, dn1 = 0.f;
  bf16_t* dps = p.dpre_seq + (row * S) * U + u0;
#pragma unroll 1
  for (int pt = wave; pt < Sp / 16; pt += kAttnWaves) {
    const float* cp = cum + pt * 16 + r16 + kb * 8;
    bf16x8 ah, al;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float c = cp[j];
      const __bf16 hi = (__bf16)c;
      ah[j] = hi;
      al[j] = (__bf16)(c - (float)hi);
    }
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[1], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[1], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[1], acc1, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int sp = pt * 16 + 4 * kb + i;
      const bool on = sp < slen;
      const uint16_t* kr = keys + sp * kLocUnits + r16;
      const float t0 = tanh_fast(acc0[i] + q0 + (on ? bf2f(kr[0]) : 0.f));
      const float t1 = tanh_fast(acc1[i] + q1 + (on ? bf2f(kr[16]) : 0.f));
      const float des = de[sp];
      const float d0 = des * v0 * (1.f - t0 * t0), d1 = des * v1 * (1.f - t1 * t1);
      dq0 += d0; dq1 += d1;
      dn0 += des * t0; dn1 += des * t1;
      const bf16_t h0 = f2bf(d0), h1 = f2bf(d1);
      const bf16_t l0 = f2bf(d0 - bf2f(h0)), l1 = f2bf(d1 - bf2f(h1));
      if (on) {
        dps[(long long)sp * U + r16] = h0;
        dps[(long long)sp * U + 16 + r16] = h1;
      }
      d0s_hi[sp * kSbD0sPitch + r16] = h0; d0s_hi[sp * kSbD0sPitch + 16 + r16] = h1;
      d0s_lo[sp * kSbD0sPitch + r16] = l0; d0s_lo[sp * kSbD0sPitch + 16 + r16] = l1;
      d0t_hi[r16 * TP + sp] = h0; d0t_hi[(16 + r16) * TP + sp] = h1;
      d0t_lo[r16 * TP + sp] = l0; d0t_lo[(16 + r16) * TP + sp] = l1;
    }
  }
  pq[(wave * 4 + kb) * kLocUnits + r16] = dq0; pq[(wave * 4 + kb) * kLocUnits + 16 + r16] = dq1;
  pn[(wave * 4 + kb) * kLocUnits + r16] = dn0; pn[(wave * 4 + kb) * kLocUnits + 16 + r16] = dn1;
  __syncthreads();
  if (wave < 4) {
    // ---- phase B: dWck tile (taps mt * 16 ..., units nt * 16 ...) over all positions ---------------------------
    const int mt = wave >> 1, nt = wave & 1;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ks = 0; ks < Sp / 32; ++ks) {
      const float* cp = cum + ks * 32 + kb * 8 + mt * 16 + r16;      // row = tap, 8 consecutive positions
      bf16x8 ah, al;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float c = cp[j];
        const __bf16 hi = (__bf16)c;
        ah[j] = hi;
        al[j] = (__bf16)(c - (float)hi);
      }
      const bf16x8 th = *reinterpret_cast<const bf16x8*>(d0t_hi + (nt * 16 + r16) * TP + ks * 32 + kb * 8);
      const bf16x8 tl = *reinterpret_cast<const bf16x8*>(d0t_lo + (nt * 16 + r16) * TP + ks * 32 + kb * 8);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, th, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, th, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, tl, acc, 0, 0, 0);
    }
    float* dwa = p.dwck_acc + (long long)b * K * U + u0 + nt * 16 + r16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = mt * 16 + 4 * kb + i;
      if (k < K) dwa[(long long)k * U] += acc[i];
    }
  } else {
    // ---- phase C: G[s, k] = sum_u d0[s, u] Wck[k, u] for the position tiles of this wave ---------------------------
    bf16x8 gh[2], gl[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float w = nt * 16 + r16 < K ? wg[nt][j] : 0.f;
        const __bf16 hi = (__bf16)w;
        gh[nt][j] = hi;
        gl[nt][j] = (__bf16)(w - (float)hi);
      }
#pragma unroll 1
    for (int pt = wave - 4; pt < Sp / 16; pt += 4) {
      const bf16x8 sh = *reinterpret_cast<const bf16x8*>(d0s_hi + (pt * 16 + r16) * kSbD0sPitch + kb * 8);
      const bf16x8 sl = *reinterpret_cast<const bf16x8*>(d0s_lo + (pt * 16 + r16) * kSbD0sPitch + kb * 8);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sh, gh[nt], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sl, gh[nt], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sh, gl[nt], acc, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) G[(pt * 16 + 4 * kb + i) * 33 + nt * 16 + r16] = acc[i];
      }
    }
  }
  __syncthreads();
  // ---- phase D: state gradient along the anti-diagonals of G; dq / dv sums in a fixed order ------------------------
  float* dpo = x.dcum_part + ((long long)b * kLocParts + part) * S;
  for (int c = tid; c < S; c += kAttnThreads) {
    float a = 0.f;
    for (int k = 0; k < K; ++k) {
      const int sp = c + padl - k;
      if (sp >= 0 && sp < Sp) a += G[sp * 33 + k];
    }
    dpo[c] = a;
  }
  if (tid < kLocUnits) {
    float dq = 0.f, dn = 0.f;
    for (int w = 0; w < kAttnWaves * 4; ++w) { dq += pq[w * kLocUnits + tid]; dn += pn[w * kLocUnits + tid]; }
    p.dq_seq[row * U + u0 + tid] = f2bf(dq);
    p.dnv_acc[(long long)b * U + u0 + tid] += dn;
    p.dbd_acc[(long long)b * U + u0 + tid] += dq;
  }
}

// the backward pass's score-gradient launch on the MFMA kernel (same conditions as the forward fast path)
static bool ad_fast_score_bwd(const os2s_attn_decoder_t* d) {
  return ad_fast_cells(d) && ad_score_bwd_mfma_lds_floats(d->S) * sizeof(float) <= 160 * 1024 && d->U % 4 == 0;
}
static int ad_launch_fast_score_bwd(hipStream_t stream, const AdAttn& at, const AdLoc& lx,
                                    const os2s_attn_decoder_t* d) {
  const size_t lds = ad_score_bwd_mfma_lds_floats(d->S) * sizeof(float);
  OS2S_LAUNCH_LDS(ad_loc_score_bwd_mfma_kernel, dim3(kLocParts, d->B), dim3(kAttnThreads), lds, stream, at, lx);
  return OS2S_OK;
}

// ------------------------------------------------------------------ cell backward
// One (unit, sample) of the cell backward under zoneout (mode 1). g_h / g_c: the gradients reaching the ZONED
// h'_t (dgB . WB^T + the carry) and c'_t (the carry); the mask sends each to the new value or past the cell to
// step t - 1. c_seq[t] holds the zoned c': the unzoned c_new that tanh saw is c_seq[t] where the mask kept it
// and is otherwise recomputed from the saved gates and c_seq[t-1].
__device__ __forceinline__ void zoneout_cell_bwd(uint32_t mh, uint32_t mc, float dy, float g_h, float g_c, float ig,
                                                 float fg, float gg, float og, float cz, float cprev, float& di,
                                                 float& dj, float& df, float& dout, float& ndc, float& ndh) {
  const float dh = dy + (mh ? g_h : 0.f);
  const float cn = mc ? cz : cprev * fg + ig * gg;
  const float tc = tanhf(cn);
  const float dc = dh * og * (1.f - tc * tc) + (mc ? g_c : 0.f);
  di = dc * gg * ig * (1.f - ig);
  dj = dc * ig * (1.f - gg * gg);
  df = dc * cprev * fg * (1.f - fg);
  dout = dh * tc * og * (1.f - og);
  ndc = dc * fg + (mc ? 0.f : g_c);
  ndh = mh ? 0.f : g_h;
}

struct AdCellBwd {
  int B, T, H, t, last, KA, KB, KQ;
  float forget_bias;
  const int32_t* lens;
  const bf16_t* dy_ext; long long dy_bs, dy_ts;   // gradient of the (dropped) output or null
  const bf16_t* dgA; long long dgA_ld; const bf16_t* wAT; long long wAT_ld;   // upper layer, same step
  const bf16_t* dgB; long long dgB_ld; const bf16_t* wBT; long long wBT_ld;   // own layer, step t+1
  const bf16_t* dq; long long dq_ld; const bf16_t* wqT;                       // query layer: dq . Wq (top layer)
  const bf16_t* gates;   // [B,T,4H]
  const float* c_seq;    // [B,T,H]
  float* dc_carry;       // [B,H]
  bf16_t* dg_out;        // [B,T,4H]
  float out_keep;
  unsigned long long out_seed;
  int zo;                // zoneout mode 1: c_seq holds the zoned state, dh_carry is live
  float zo_keep;         // 1 - zoneout_prob
  unsigned long long zo_seed_h, zo_seed_c;
  float* dh_carry;       // [B,H] gradient of the zoned h' that its mask sent past the cell (zoneout only)
  float* part;           // split kernel: [H/32][B/32][kCbSplit] partial tiles
  int* ticket;           // split kernel: [H/32][B/32], zero before and after every launch
};

// dh = dropout'(dy_ext + dgA . WA^T + dq . Wq) + dgB . WB^T, then the LSTM gate derivatives.
// One workgroup = kCellBwdRows hidden units x 32 samples: with 32-row tiles a 1024-unit layer was
// 32 workgroups (an eighth of the chip), each streaming two 256 KB weight slices next to the two
// [32, 4H] gate-gradient blocks every workgroup reads anyway; 8-row tiles give 128 workgroups and
// 64 KB slices (rows 8..31 of the MFMA tile are padding). Both products are accumulated before
// ONE reduction through LDS.
constexpr int kCellBwdRows = 8;
constexpr int kCellBwdCols = 32;   // samples per workgroup. (Fetching wave 0's epilogue operands before the
                                   // products — in registers: spills at the 128-register budget of 16 waves; by
                                   // LDS-DMA: no spill — left the step at 95 us either way: not kept.)
                                   // (8 samples per workgroup — a quarter of the
                                   // gate-gradient bytes per CU, 4x the workgroups re-reading the weight
                                   // slices — was slower: 29.8 vs 26.4 us; the step is five dependent
                                   // rounds of loads, not bytes per CU.)
__global__ __launch_bounds__(64 * kBwdWaves) void ad_cell_bwd_kernel(AdCellBwd p) {
  __shared__ float red[kBwdWaves * 8 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int j0 = blockIdx.x * kCellBwdRows, b0 = blockIdx.y * kCellBwdCols;
  const int H = p.H;
  const bool vrow = l31 < kCellBwdRows && j0 + l31 < H;
  const int brow = b0 + l31;
  const bool vcol = l31 < kCellBwdCols && brow < p.B;
  f32x16 accwM, accwB;
#pragma unroll
  for (int e = 0; e < 16; ++e) { accwM[e] = 0.f; accwB[e] = 0.f; }
  if (p.KA > 0)
    tile_gemm_prefetch<kBwdWaves, 8>(vrow ? p.wAT + (long long)(j0 + l31) * p.wAT_ld : nullptr,
                                      vcol ? p.dgA + (long long)brow * p.dgA_ld : nullptr, p.KA, accwM, p.wAT);
  if (p.KQ > 0)
    tile_gemm_prefetch<kBwdWaves, 2>(vrow ? p.wqT + (long long)(j0 + l31) * p.KQ : nullptr,
                                     vcol ? p.dq + (long long)brow * p.dq_ld : nullptr, p.KQ, accwM, p.wqT);
  if (!p.last && p.KB > 0)
    tile_gemm_prefetch<kBwdWaves, 8>(vrow ? p.wBT + (long long)(j0 + l31) * p.wBT_ld : nullptr,
                                      vcol ? p.dgB + (long long)brow * p.dgB_ld : nullptr, p.KB, accwB, p.wBT);
  // rows 0..7 of the tile = accumulator elements 0..3 (row 4*(lane>>5) + e): 8 floats per lane and wave
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[(wave * 8 + e) * 64 + lane] = accwM[e];
    red[(wave * 8 + 4 + e) * 64 + lane] = accwB[e];
  }
  __syncthreads();
  if (wave >= 1) return;
  float accM[4], accB[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float sm = 0.f, sb = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < kBwdWaves; ++w2) {
      sm += red[(w2 * 8 + e) * 64 + lane];
      sb += red[(w2 * 8 + 4 + e) * 64 + lane];
    }
    accM[e] = sm; accB[e] = sb;
  }
  const int b = b0 + l31;
  if (l31 >= kCellBwdCols || b >= p.B) return;
  if (p.lens && p.t >= p.lens[b]) return;
  const int j = j0 + 4 * lhi;
  if (j >= H) return;
  const long long row = (long long)b * p.T + p.t;
  float dyv[4] = {accM[0], accM[1], accM[2], accM[3]};
  if (p.dy_ext) {
    const u32x2 v = *reinterpret_cast<const u32x2*>(p.dy_ext + (long long)b * p.dy_bs + (long long)p.t * p.dy_ts + j);
    dyv[0] += bflo(v[0]); dyv[1] += bfhi(v[0]); dyv[2] += bflo(v[1]); dyv[3] += bfhi(v[1]);
  }
  if (p.out_keep < 1.f) {
    const unsigned long long idx = (unsigned long long)row * H + j;
    const uint32_t bits = dropout_bits8(p.out_seed, idx >> 3, p.out_keep) >> (j & 4);
    const float inv = 1.f / p.out_keep;
#pragma unroll
    for (int e = 0; e < 4; ++e) dyv[e] = ((bits >> e) & 1u) ? dyv[e] * inv : 0.f;
  }
  float sv[4][4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const u32x2 v = *reinterpret_cast<const u32x2*>(p.gates + row * (4 * H) + (long long)g * H + j);
    sv[g][0] = bflo(v[0]); sv[g][1] = bfhi(v[0]); sv[g][2] = bflo(v[1]); sv[g][3] = bfhi(v[1]);
  }
  f32x4 dcarry = {0.f, 0.f, 0.f, 0.f};
  if (!p.last) dcarry = *reinterpret_cast<const f32x4*>(p.dc_carry + (long long)b * H + j);
  const f32x4 cv = *reinterpret_cast<const f32x4*>(p.c_seq + row * H + j);
  f32x4 cprev = {0.f, 0.f, 0.f, 0.f};
  if (p.t > 0) cprev = *reinterpret_cast<const f32x4*>(p.c_seq + (row - 1) * H + j);
  f32x4 ndc;
  float dpre[4][4];
  if (p.zo) {
    f32x4 hcarry = {0.f, 0.f, 0.f, 0.f};
    if (!p.last) hcarry = *reinterpret_cast<const f32x4*>(p.dh_carry + (long long)b * H + j);
    const unsigned long long idx = (unsigned long long)row * H + j;
    const uint32_t mh = dropout_bits8(p.zo_seed_h, idx >> 3, p.zo_keep) >> (j & 4);
    const uint32_t mc = dropout_bits8(p.zo_seed_c, idx >> 3, p.zo_keep) >> (j & 4);
    f32x4 ndh;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float nc, nh;
      zoneout_cell_bwd((mh >> e) & 1u, (mc >> e) & 1u, dyv[e], accB[e] + hcarry[e], dcarry[e], sv[0][e], sv[1][e],
                       sv[2][e], sv[3][e], cv[e], cprev[e], dpre[0][e], dpre[1][e], dpre[2][e], dpre[3][e], nc, nh);
      ndc[e] = nc; ndh[e] = nh;
    }
    *reinterpret_cast<f32x4*>(p.dh_carry + (long long)b * H + j) = ndh;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float dh = dyv[e] + accB[e];
      const float ig = sv[0][e], fg = sv[1][e], gg = sv[2][e], og = sv[3][e];
      const float tc = tanhf(cv[e]);
      const float dc = dh * og * (1.f - tc * tc) + dcarry[e];
      dpre[0][e] = dc * gg * ig * (1.f - ig);         // i
      dpre[1][e] = dc * ig * (1.f - gg * gg);         // j
      dpre[2][e] = dc * cprev[e] * fg * (1.f - fg);   // f
      dpre[3][e] = dh * tc * og * (1.f - og);         // o
      ndc[e] = dc * fg;
    }
  }
  *reinterpret_cast<f32x4*>(p.dc_carry + (long long)b * H + j) = ndc;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    u32x2 pk;
    pk[0] = pack2bf(dpre[g][0], dpre[g][1]);
    pk[1] = pack2bf(dpre[g][2], dpre[g][3]);
    *reinterpret_cast<u32x2*>(p.dg_out + row * (4 * H) + (long long)g * H + j) = pk;
  }
}

// ---- the same, cut kCbSplit ways along the reduction ----------------------------------------------
// The kernel above is five DEPENDENT rounds of loads per workgroup (two 4H-deep products of 2 rounds
// each + the query product) and every one of its 128 workgroups re-reads both [32, 4H] gate-gradient
// blocks for 8 useful rows of its MFMA tiles (512 KB of activations next to 128 KB of weights). Here a
// workgroup owns a FULL 32-unit tile and one quarter of the reduction of both products: one round of
// loads (8 + 8 slices per wave, all issued before the first MFMA), 128 KB of weights + 128 KB of
// activations per workgroup, the same 128 workgroups for H = 1024. The four partial tiles of a hidden
// block meet through a ticket (stores -> release -> one atomic per workgroup; the workgroup that draws
// the last ticket acquires, sums the four slabs in piece order — deterministic — and runs the gate
// derivatives; nobody spins). The epilogue operands are requested before the products by every piece
// (they are 30 registers; only the last arriver uses them), so the reducer's chain is slab reads only.
// Tacotron2 decoder shape (H = 1024, B = 32), backward time per decoder step: 95.8 us with the kernel
// above, 88.8 / 78.7 / 80.2 us cut 2 / 4 / 8 ways (-DOS2S_CB_SPLIT=n -DOS2S_CB_SLICES=m to rebuild one).
#ifndef OS2S_CB_SPLIT
#define OS2S_CB_SPLIT 4
#define OS2S_CB_SLICES 8
#endif
constexpr int kCbSplit = OS2S_CB_SPLIT;
constexpr int kCbWaves = 8;
constexpr int kCbSlices = OS2S_CB_SLICES;         // 16-deep slices per wave and product and batch
constexpr int kCbSlabFloats = 2 * 16 * 64;        // (M, B) x 16 accumulator registers x 64 lanes

__global__ __launch_bounds__(64 * kCbWaves) void ad_cell_bwd_split_kernel(AdCellBwd p) {
  __shared__ float red[kCbWaves * 32 * 64];       // 64 KB
  __shared__ int s_ticket;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hb = blockIdx.x, kq = blockIdx.y, bb = blockIdx.z;
  const int j0 = hb * 32, b0 = bb * 32;
  const int H = p.H;
  const bool vrow = j0 + l31 < H;
  const int brow = b0 + l31;
  const bool vcol = brow < p.B;
  // ---- epilogue operands of (sample l31, units j0 + 8*wave + 4*lhi .. +3), waves 0..3 ------------------
  const int ej = j0 + 8 * wave + 4 * lhi;
  const bool elive = wave < 4 && vcol && ej < H && !(p.lens && p.t >= p.lens[brow]);
  const long long erow = (long long)brow * p.T + p.t;
  u32x2 e_dy = {0u, 0u}, e_g[4];
  f32x4 e_dcarry = {0.f, 0.f, 0.f, 0.f}, e_cv = {0.f, 0.f, 0.f, 0.f}, e_cprev = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < 4; ++g) e_g[g] = u32x2{0u, 0u};
  if (elive) {
    if (p.dy_ext) e_dy = *reinterpret_cast<const u32x2*>(p.dy_ext + (long long)brow * p.dy_bs + (long long)p.t * p.dy_ts + ej);
#pragma unroll
    for (int g = 0; g < 4; ++g) e_g[g] = *reinterpret_cast<const u32x2*>(p.gates + erow * (4 * H) + (long long)g * H + ej);
    if (!p.last) e_dcarry = *reinterpret_cast<const f32x4*>(p.dc_carry + (long long)brow * H + ej);
    e_cv = *reinterpret_cast<const f32x4*>(p.c_seq + erow * H + ej);
    if (p.t > 0) e_cprev = *reinterpret_cast<const f32x4*>(p.c_seq + (erow - 1) * H + ej);
  }
  // ---- this piece of the two products (+ the whole query product in piece 0) ---------------------------
  f32x16 accM, accB;
#pragma unroll
  for (int e = 0; e < 16; ++e) { accM[e] = 0.f; accB[e] = 0.f; }
  const u32x4 zero = {0u, 0u, 0u, 0u};
  const bool doA = p.KA > 0, doB = !p.last && p.KB > 0;
  const bf16_t* const wA = p.wAT + (long long)(vrow ? j0 + l31 : 0) * p.wAT_ld;
  const bf16_t* const gA = p.dgA + (long long)(vcol ? brow : 0) * p.dgA_ld;
  const bf16_t* const wB = p.wBT + (long long)(vrow ? j0 + l31 : 0) * p.wBT_ld;
  const bf16_t* const gB = p.dgB + (long long)(vcol ? brow : 0) * p.dgB_ld;
  const int nitA = doA ? (p.KA + 15) >> 4 : 0, nitB = doB ? (p.KB + 15) >> 4 : 0;
  const int nperA = (nitA + kCbSplit - 1) / kCbSplit, nperB = (nitB + kCbSplit - 1) / kCbSplit;
  const int nper = max(nperA, nperB);
  u32x4 qa = zero, qb = zero;
  const bool doQ = p.KQ > 0 && kq == 0 && wave * 16 < p.KQ;       // KQ <= 16 * kCbWaves (checked by the host side)
  if (doQ) {
    const int ko = min(wave * 16 + lhi * 8, p.KQ - 8);
    qa = *reinterpret_cast<const u32x4*>(p.wqT + (long long)(vrow ? j0 + l31 : 0) * p.KQ + ko);
    qb = *reinterpret_cast<const u32x4*>(p.dq + (long long)(vcol ? brow : 0) * p.dq_ld + ko);
  }
  for (int base = 0; base < nper; base += kCbWaves * kCbSlices) {
    u32x4 wa[kCbSlices], ga[kCbSlices], wb[kCbSlices], gb[kCbSlices];
    if (doA) {
#pragma unroll
      for (int i = 0; i < kCbSlices; ++i) {
        const int s = kq * nperA + base + wave + kCbWaves * i;
        const int ko = min(s * 16 + lhi * 8, p.KA - 8);
        wa[i] = *reinterpret_cast<const u32x4*>(wA + ko);
        ga[i] = *reinterpret_cast<const u32x4*>(gA + ko);
      }
    }
    if (doB) {
#pragma unroll
      for (int i = 0; i < kCbSlices; ++i) {
        const int s = kq * nperB + base + wave + kCbWaves * i;
        const int ko = min(s * 16 + lhi * 8, p.KB - 8);
        wb[i] = *reinterpret_cast<const u32x4*>(wB + ko);
        gb[i] = *reinterpret_cast<const u32x4*>(gB + ko);
      }
    }
    if (doA) {
#pragma unroll
      for (int i = 0; i < kCbSlices; ++i) {
        const int sl = base + wave + kCbWaves * i, s = kq * nperA + sl;
        const bool kv = sl < nperA && s < nitA && s * 16 + lhi * 8 < p.KA;
        accM = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, (kv && vrow) ? wa[i] : zero),
                                                       __builtin_bit_cast(bf16x8, (kv && vcol) ? ga[i] : zero), accM, 0, 0, 0);
      }
    }
    if (doB) {
#pragma unroll
      for (int i = 0; i < kCbSlices; ++i) {
        const int sl = base + wave + kCbWaves * i, s = kq * nperB + sl;
        const bool kv = sl < nperB && s < nitB && s * 16 + lhi * 8 < p.KB;
        accB = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, (kv && vrow) ? wb[i] : zero),
                                                       __builtin_bit_cast(bf16x8, (kv && vcol) ? gb[i] : zero), accB, 0, 0, 0);
      }
    }
  }
  if (doQ) {
    const bool kv = wave * 16 + lhi * 8 < p.KQ;
    accM = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, (kv && vrow) ? qa : zero),
                                                   __builtin_bit_cast(bf16x8, (kv && vcol) ? qb : zero), accM, 0, 0, 0);
  }
  // ---- workgroup sum of the 8 waves' tiles -> this piece's slab ------------------------------------------
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    red[(wave * 32 + r) * 64 + lane] = accM[r];
    red[(wave * 32 + 16 + r) * 64 + lane] = accB[r];
  }
  __syncthreads();
  float* const slab0 = p.part + ((size_t)(hb * gridDim.z + bb) * kCbSplit) * kCbSlabFloats;
#pragma unroll
  for (int q = 0; q < kCbSlabFloats / (64 * kCbWaves); ++q) {
    const int o = tid + 64 * kCbWaves * q;        // (register row rr = o / 64, lane o % 64)
    float s = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < kCbWaves; ++w2) s += red[w2 * 32 * 64 + o];
    slab0[(size_t)kq * kCbSlabFloats + o] = s;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int* const ticket = p.ticket + hb * gridDim.z + bb;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_ticket = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (s_ticket != kCbSplit - 1) return;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // zero before and after every launch
  }
  __syncthreads();
  if (!elive) return;
  // ---- last arriver: the four slabs in piece order, then the gate derivatives -----------------------------
  float accm[4] = {0.f, 0.f, 0.f, 0.f}, accb[4] = {0.f, 0.f, 0.f, 0.f};
  for (int pc = 0; pc < kCbSplit; ++pc) {
    const float* const sl = slab0 + (size_t)pc * kCbSlabFloats;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      accm[e] += sl[(4 * wave + e) * 64 + lane];
      accb[e] += sl[(16 + 4 * wave + e) * 64 + lane];
    }
  }
  float dyv[4] = {accm[0] + bflo(e_dy[0]), accm[1] + bfhi(e_dy[0]), accm[2] + bflo(e_dy[1]), accm[3] + bfhi(e_dy[1])};
  if (p.out_keep < 1.f) {
    const unsigned long long idx = (unsigned long long)erow * H + ej;
    const uint32_t bits = dropout_bits8(p.out_seed, idx >> 3, p.out_keep) >> (ej & 4);
    const float inv = 1.f / p.out_keep;
#pragma unroll
    for (int e = 0; e < 4; ++e) dyv[e] = ((bits >> e) & 1u) ? dyv[e] * inv : 0.f;
  }
  float sv[4][4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    sv[g][0] = bflo(e_g[g][0]); sv[g][1] = bfhi(e_g[g][0]); sv[g][2] = bflo(e_g[g][1]); sv[g][3] = bfhi(e_g[g][1]);
  }
  f32x4 ndc;
  float dpre[4][4];
  if (p.zo) {
    f32x4 hcarry = {0.f, 0.f, 0.f, 0.f};
    if (!p.last) hcarry = *reinterpret_cast<const f32x4*>(p.dh_carry + (long long)brow * H + ej);
    const unsigned long long idx = (unsigned long long)erow * H + ej;
    const uint32_t mh = dropout_bits8(p.zo_seed_h, idx >> 3, p.zo_keep) >> (ej & 4);
    const uint32_t mc = dropout_bits8(p.zo_seed_c, idx >> 3, p.zo_keep) >> (ej & 4);
    f32x4 ndh;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float nc, nh;
      zoneout_cell_bwd((mh >> e) & 1u, (mc >> e) & 1u, dyv[e], accb[e] + hcarry[e], e_dcarry[e], sv[0][e], sv[1][e],
                       sv[2][e], sv[3][e], e_cv[e], e_cprev[e], dpre[0][e], dpre[1][e], dpre[2][e], dpre[3][e], nc, nh);
      ndc[e] = nc; ndh[e] = nh;
    }
    *reinterpret_cast<f32x4*>(p.dh_carry + (long long)brow * H + ej) = ndh;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float dh = dyv[e] + accb[e];
      const float ig = sv[0][e], fg = sv[1][e], gg = sv[2][e], og = sv[3][e];
      const float tc = tanhf(e_cv[e]);
      const float dc = dh * og * (1.f - tc * tc) + e_dcarry[e];
      dpre[0][e] = dc * gg * ig * (1.f - ig);         // i
      dpre[1][e] = dc * ig * (1.f - gg * gg);         // j
      dpre[2][e] = dc * e_cprev[e] * fg * (1.f - fg); // f
      dpre[3][e] = dh * tc * og * (1.f - og);         // o
      ndc[e] = dc * fg;
    }
  }
  *reinterpret_cast<f32x4*>(p.dc_carry + (long long)brow * H + ej) = ndc;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    u32x2 pk;
    pk[0] = pack2bf(dpre[g][0], dpre[g][1]);
    pk[1] = pack2bf(dpre[g][2], dpre[g][3]);
    *reinterpret_cast<u32x2*>(p.dg_out + erow * (4 * H) + (long long)g * H + ej) = pk;
  }
}

// ------------------------------------------------------------------ post-loop passes
// dmem[b,s,m] = sum_t align[b,t,s] * dctx[b,t,m]   (bf16 out, zero past src_len)
// One workgroup per (256 columns, 16 source positions, sample): 13 x 2 x 32 = 832 workgroups for the
// Tacotron2 shapes (the first version looped over the source positions inside 64 workgroups and took
// 6.2 ms per step). The 16 alignment values of a time step are the same for every thread (scalar
// loads); four time steps are in flight per iteration.
__global__ __launch_bounds__(256) void ad_dvalues_kernel(const float* __restrict__ align,
                                                         const bf16_t* __restrict__ dctx,
                                                         const int32_t* __restrict__ src_len,
                                                         const int32_t* __restrict__ tgt_len, int T,
                                                         int S, int M, bf16_t* __restrict__ dmem) {
  const int b = blockIdx.z, s0 = blockIdx.y * 16, m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int slen = min(max(src_len[b], 0), S);
  const int tl = tgt_len ? min(max(tgt_len[b], 0), T) : T;
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  if (s0 < slen) {
    const bf16_t* dc = dctx + (long long)b * T * M + m;
    const float* al = align + (long long)b * T * S + s0;
    int t = 0;
    for (; t + 4 <= tl; t += 4) {
      float d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) d[u] = bf2f(dc[(long long)(t + u) * M]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* ar = al + (long long)(t + u) * S;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] += (s0 + i < S ? ar[i] : 0.f) * d[u];
      }
    }
    for (; t < tl; ++t) {
      const float d = bf2f(dc[(long long)t * M]);
      const float* ar = al + (long long)t * S;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] += (s0 + i < S ? ar[i] : 0.f) * d;
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (s0 + i < S) dmem[((long long)b * S + s0 + i) * M + m] = f2bf(s0 + i < slen ? acc[i] : 0.f);
}

// Wck[k,u] = sum_f conv_w[k,f] dense_w[f,u];  bd[u] = sum_f conv_b[f] dense_w[f,u]  (out: [K+1, U])
__global__ void ad_fold_location_kernel(const float* __restrict__ conv_w, const float* __restrict__ conv_b,
                                        const float* __restrict__ dense_w, int K, int F, int U,
                                        float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (K + 1) * U) return;
  const int k = i / U, u = i - k * U;
  float a = 0.f;
  for (int f = 0; f < F; ++f) a += (k < K ? conv_w[k * F + f] : conv_b[f]) * dense_w[f * U + u];
  out[i] = a;
}

// gradients of conv_w [K,F], conv_b [F], dense_w [F,U] from d(Wck) and d(bd) partials per sample
__global__ __launch_bounds__(256) void ad_unfold_location_grads_kernel(
    const float* __restrict__ dwck_acc, const float* __restrict__ dbd_acc, int B, int K, int F, int U,
    const float* __restrict__ conv_w, const float* __restrict__ conv_b, const float* __restrict__ dense_w,
    float* __restrict__ dconv_w, float* __restrict__ dconv_b, float* __restrict__ ddense_w,
    float* __restrict__ tmp /* [(K+1)*U] */) {
  const int tid = threadIdx.x;
  for (int i = tid; i < (K + 1) * U; i += 256) {
    float a = 0.f;
    if (i < K * U) { for (int b = 0; b < B; ++b) a += dwck_acc[(long long)b * K * U + i]; }
    else { for (int b = 0; b < B; ++b) a += dbd_acc[(long long)b * U + (i - K * U)]; }
    tmp[i] = a;
  }
  __syncthreads();
  for (int i = tid; i < (K + 1) * F; i += 256) {   // d conv_w[k,f] (k < K), d conv_b[f] (k == K)
    const int k = i / F, f = i - k * F;
    float a = 0.f;
    for (int u = 0; u < U; ++u) a += tmp[k * U + u] * dense_w[f * U + u];
    if (k < K) dconv_w[k * F + f] += a; else dconv_b[f] += a;
  }
  for (int i = tid; i < F * U; i += 256) {
    const int f = i / U, u = i - f * U;
    float a = conv_b[f] * tmp[K * U + u];
    for (int k = 0; k < K; ++k) a += conv_w[k * F + f] * tmp[k * U + u];
    ddense_w[i] += a;
  }
}

// dkeys[b,s,u] = sum_{t < tgt_len[b]} dpre_seq[b,t,s,u]   (zero past src_len)
__global__ __launch_bounds__(256) void ad_dkeys_kernel(const bf16_t* __restrict__ dpre_seq,
                                                       const int32_t* __restrict__ src_len,
                                                       const int32_t* __restrict__ tgt_len, int T,
                                                       int S, int U, float* __restrict__ dkeys) {
  const int b = blockIdx.y;
  const long long su = (long long)S * U;
  const long long i8 = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i8 >= su) return;
  const int s = (int)(i8 / U);
  const int slen = min(max(src_len[b], 0), S);
  const int tl = tgt_len ? min(max(tgt_len[b], 0), T) : T;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (s < slen) {
    const bf16_t* src = dpre_seq + (long long)b * T * su + i8;
#pragma unroll 8
    for (int t = 0; t < tl; ++t) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(src + (long long)t * su);
#pragma unroll
      for (int e = 0; e < 4; ++e) { a[2 * e] += bflo(v[e]); a[2 * e + 1] += bfhi(v[e]); }
    }
  }
  float* o = dkeys + (long long)b * su + i8;
  *reinterpret_cast<f32x4*>(o) = f32x4{a[0], a[1], a[2], a[3]};
  *reinterpret_cast<f32x4*>(o + 4) = f32x4{a[4], a[5], a[6], a[7]};
}

// gradient of the score vector parameters from d(normalised v) partials [B,U]
__global__ __launch_bounds__(256) void ad_score_vec_grads_kernel(const float* __restrict__ dnv_acc,
                                                                 int B, int U, int mode,
                                                                 const float* __restrict__ v,
                                                                 const float* __restrict__ g,
                                                                 float* __restrict__ dv,
                                                                 float* __restrict__ dg) {
  __shared__ float red[8];
  __shared__ float dn[1024];
  const int tid = threadIdx.x;
  float vv = 0.f, dv_dot = 0.f;
  for (int u = tid; u < U; u += 256) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dnv_acc[(long long)b * U + u];
    dn[u] = s;
    vv += v[u] * v[u];
    dv_dot += s * v[u];
  }
  __syncthreads();
  if (mode != 1) {
    for (int u = tid; u < U; u += 256) dv[u] += dn[u];
    return;
  }
  vv = wave_sum_dpp(vv);
  dv_dot = wave_sum_dpp(dv_dot);
  if ((tid & 63) == 0) { red[tid >> 6] = vv; red[4 + (tid >> 6)] = dv_dot; }
  __syncthreads();
  vv = red[0] + red[1] + red[2] + red[3];
  dv_dot = red[4] + red[5] + red[6] + red[7];
  const float rn = rsqrtf(vv), gg = g[0];
  // nv = g * v / |v|:  dg = sum dn*v/|v|;  dv = g*(dn/|v| - v*(dn.v)/|v|^3)
  for (int u = tid; u < U; u += 256) dv[u] += gg * (dn[u] * rn - v[u] * dv_dot * rn * rn * rn);
  if (tid == 0) dg[0] += dv_dot * rn;
}

}  // namespace os2s

using namespace os2s;

#ifdef OS2S_ATTN_PHASE_TIMERS
extern "C" int os2s_debug_attn_phases(long long* out32) {
  return hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_attn_dbg), sizeof(long long) * 32) == hipSuccess ? 0 : -1;
}
#endif

static size_t attn_lds_bytes(const os2s_attn_decoder_t* d, bool bwd, bool resident = true) {
  return attn_lds_floats(d->H, d->M, d->U, d->S, d->score_mode, d->loc_k, bwd, resident) * sizeof(float);
}

// A/B switches: attn_decoder.attn_split = 0: the one-workgroup-per-sample attention kernels; attn_decoder.cell_split
// = 0: the one-workgroup-per-8-units cell backward. No workspace size depends on either.
static int g_attn_split = 1, g_cell_split = 1;
static os2s::OptionReg r_attn_split("attn_decoder.attn_split", &g_attn_split, "OS2S_ATTN_SPLIT");
static os2s::OptionReg r_cell_split("attn_decoder.cell_split", &g_cell_split, "OS2S_CELL_SPLIT");

// Where the one-workgroup-per-sample attention kernel of a forward (bwd = false) or backward launch keeps the
// keys, from that launch's own LDS footprint: resident while it fits (every shape that ran before streaming
// existed stays resident), else streamed, else refused. Location mode has the resident form only, and one
// budget, the backward's, for both passes, as it always had.
enum { kKeysRefused = 0, kKeysLds = 1, kKeysStreamed = 2 };
static int attn_keys_mode(const os2s_attn_decoder_t* d, bool bwd) {
  if (d->score_mode == 2) return attn_lds_bytes(d, true) <= (size_t)kLdsMax ? kKeysLds : kKeysRefused;
  if (attn_lds_bytes(d, bwd) <= (size_t)kLdsMax) return kKeysLds;
  return attn_lds_bytes(d, bwd, false) <= (size_t)kLdsMax ? kKeysStreamed : kKeysRefused;
}

// the split location-attention kernels apply
bool os2s::loc_split(const os2s_attn_decoder_t* d) {
  return g_attn_split != 0 && d->score_mode == 2 && d->U == kLocParts * kLocUnits && d->M % 8 == 0 &&
         loc_fwd_lds_floats(d->H, d->S) * sizeof(float) <= 64 * 1024 &&
         loc_bwd_lds_floats(d->S, d->loc_k) * sizeof(float) <= 160 * 1024;
}

extern "C" size_t os2s_attn_decoder_loc_ws_floats(int B, int S, int U, int loc_k) {
  return (size_t)(loc_k + 1) * U + (size_t)B * kLocParts * S;
}

int os2s::ad_check(const os2s_attn_decoder_t* d) {
  OS2S_REQUIRE(d && d->B >= 1 && d->T >= 1 && d->S >= 1 && (d->L == 1 || d->L == 2));
  OS2S_REQUIRE(d->H % 8 == 0 && d->M % 8 == 0 && d->U % 8 == 0 && d->U >= 8 && d->U <= 1024);
  OS2S_REQUIRE(d->score_mode >= 0 && d->score_mode <= 3);
  OS2S_REQUIRE(d->zoneout_mode >= 0 && d->zoneout_mode <= 2);
  if (d->zoneout_mode) OS2S_REQUIRE(d->zoneout_prob >= 0.f && d->zoneout_prob < 1.f);
  if (d->score_mode == 3 && d->U != d->H) return OS2S_ERR_UNSUPPORTED;     // Luong: the query IS the cell output
  OS2S_REQUIRE(d->t_begin >= 0 && d->t_begin <= d->t_end && d->t_end <= d->T);
  OS2S_REQUIRE(d->wcat[0] && d->wq && d->v && d->keys && d->values && d->src_len && d->gx0);
  OS2S_REQUIRE(d->cat[0] && d->c_seq[0] && d->align_seq && d->q_seq && d->y_top && d->ctx);
  if (d->L == 2) OS2S_REQUIRE(d->wcat[1] && d->cat[1] && d->c_seq[1]);
  if (d->score_mode == 1) OS2S_REQUIRE(d->g && d->b);
  if (d->score_mode == 2) {
    OS2S_REQUIRE(d->loc_k >= 1 && d->loc_k <= kLocKMax && d->loc_f >= 1 && d->U == 128);
    OS2S_REQUIRE(d->conv_w && d->conv_b && d->dense_w && d->cum_seq && d->loc_ws);
    if (d->use_bias) OS2S_REQUIRE(d->b);
  }
  // the other modes are judged per pass, by the entry point that launches it (attn_keys_mode)
  if (d->score_mode == 2 && attn_keys_mode(d, true) == kKeysRefused) return OS2S_ERR_UNSUPPORTED;
  return OS2S_OK;
}

void os2s::ad_fill_attn(const os2s_attn_decoder_t* d, AdAttn& a) {
  a.B = d->B; a.T = d->T; a.S = d->S; a.H = d->H; a.M = d->M; a.U = d->U;
  a.mode = d->score_mode; a.use_bias = d->use_bias; a.loc_k = d->loc_k;
  a.Kc0 = d->M + d->H;
  a.src_len = d->src_len; a.tgt_len = d->tgt_len;
  a.yq = (const bf16_t*)d->y_top; a.yq_bs = d->y_top_bs; a.yq_ts = d->y_top_ts;
  a.wq = (const bf16_t*)d->wq; a.keys = (const bf16_t*)d->keys; a.values = (const bf16_t*)d->values;
  a.v = d->v; a.g = d->g; a.bias = d->b; a.wck = d->loc_ws;
  a.cum_seq = d->cum_seq; a.align_seq = d->align_seq; a.q_seq = d->q_seq;
  a.ctx = (bf16_t*)d->ctx; a.ctx_bs = d->ctx_bs; a.ctx_ts = d->ctx_ts;
  a.cat0 = (bf16_t*)d->cat[0];
  a.attn_in_keep = d->attn_in_keep; a.attn_in_seed = d->attn_in_seed;
  a.dctx_ext = nullptr; a.dattn = nullptr; a.dctx_seq = nullptr; a.dcum = nullptr; a.dpre_seq = nullptr;
  a.dq_seq = nullptr; a.dhq = nullptr; a.dnv_acc = nullptr; a.dbd_acc = nullptr;
  a.dwck_acc = nullptr; a.last = 0; a.dctx_bs = a.dctx_ts = 0;
}

int os2s::ad_launch_fold_location(hipStream_t stream, const os2s_attn_decoder_t* d) {
  OS2S_LAUNCH(ad_fold_location_kernel, dim3(ceil_div((d->loc_k + 1) * d->U, 256)), dim3(256), 0, stream, d->conv_w,
              d->conv_b, d->dense_w, d->loc_k, d->loc_f, d->U, d->loc_ws);
  return OS2S_OK;
}

extern "C" int os2s_attn_decoder_fwd(os2s_stream_t stream_, const os2s_attn_decoder_t* d) {
  const int rc = ad_check(d);
  if (rc != OS2S_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int keys_mode = attn_keys_mode(d, false);
  if (keys_mode == kKeysRefused) return OS2S_ERR_UNSUPPORTED;
  const size_t lds = attn_lds_bytes(d, false, keys_mode == kKeysLds);
  const int B = d->B, T = d->T, H = d->H, M = d->M, L = d->L;
  AdAttn at;
  ad_fill_attn(d, at);
  if (d->score_mode == 2) {
    const int r2 = ad_launch_fold_location(stream, d);
    if (r2 != OS2S_OK) return r2;
  }
  // location-sensitive attention: the step is cut over kLocParts x B / ctx_parts x B workgroups
  const bool split = loc_split(d);
  AdLoc lx;
  lx.e_part = split ? d->loc_ws + (size_t)(d->loc_k + 1) * d->U : nullptr;
  lx.dal = nullptr; lx.dcum_part = nullptr;
  int ctx_parts = kLocCtxParts;
  while (ctx_parts > 1 && M % (8 * ctx_parts)) ctx_parts >>= 1;
  const int ncg = M / (8 * ctx_parts);
  const int nsp = 256 / ncg < 32 ? 256 / ncg : 32;
  const size_t lds_s = loc_fwd_lds_floats(H, d->S) * sizeof(float);
  const size_t lds_c = ((size_t)d->S + 8 + (size_t)nsp * ncg * 8) * sizeof(float);
  if (split && ncg > 256) return OS2S_ERR_UNSUPPORTED;
  dim3 cgrid(ceil_div(H, 8), ceil_div(B, 32));
  const bool fast = split && ad_fast_cells(d);
  for (int t = d->t_begin; t < d->t_end; ++t) {
    for (int l = 0; l < L; ++l) {
      if (fast) {
        const int r2 = ad_launch_fast_cell(stream, d, l, t);
        if (r2 != OS2S_OK) return r2;
        continue;
      }
      AdCellFwd c;
      c.B = B; c.T = T; c.H = H; c.t = t; c.forget_bias = d->forget_bias; c.lens = d->tgt_len;
      c.Kc = l == 0 ? M + H : 2 * H;
      c.cat = (const bf16_t*)d->cat[l]; c.w = (const bf16_t*)d->wcat[l]; c.bias = d->bias[l];
      c.w8 = d->wcat8[l]; c.w8_scale = d->wcat8_scale[l];
      if (c.w8 && !c.w8_scale) return OS2S_ERR_INVALID_ARG;
      c.gx = l == 0 ? (const bf16_t*)d->gx0 : nullptr;
      c.c_seq = d->c_seq[l]; c.gates = (bf16_t*)d->gates[l];
      c.h_next = (bf16_t*)d->cat[l] + (l == 0 ? M : H);
      if (l == L - 1) { c.y = (bf16_t*)d->y_top; c.y_bs = d->y_top_bs; c.y_ts = d->y_top_ts; }
      else { c.y = (bf16_t*)d->cat[l + 1]; c.y_bs = (long long)(T + 1) * 2 * H; c.y_ts = 2 * H; }
      c.out_keep = d->out_keep; c.out_seed = d->out_seed[l];
      c.zo_mode = d->zoneout_mode; c.zo_p = d->zoneout_prob;
      c.zo_seed_h = d->zoneout_seed_h[l]; c.zo_seed_c = d->zoneout_seed_c[l];
      OS2S_LAUNCH(ad_cell_fwd_kernel, cgrid, dim3(64 * kAdWaves), 0, stream, c);
    }
    at.t = t;
    if (split) {
      if (fast) {
        const int r2 = ad_launch_fast_scores(stream, at, lx, d);
        if (r2 != OS2S_OK) return r2;
      } else {
        OS2S_LAUNCH(ad_loc_scores_kernel, dim3(kLocParts, B), dim3(kAttnThreads), lds_s, stream, at, lx);
      }
      OS2S_LAUNCH(ad_loc_context_kernel, dim3(ctx_parts, B), dim3(256), lds_c, stream, at, lx, ncg, nsp);
    } else if (keys_mode == kKeysLds) {
      OS2S_LAUNCH_LDS(ad_attn_fwd_kernel<true>, dim3(B), dim3(kAttnThreads), lds, stream, at);
    } else {
      OS2S_LAUNCH_LDS(ad_attn_fwd_kernel<false>, dim3(B), dim3(kAttnThreads), lds, stream, at);
    }
  }
  return OS2S_OK;
}

extern "C" size_t os2s_attn_decoder_bwd_workspace_bytes(const os2s_attn_decoder_t* d) {
  if (!d) return 0;
  const size_t B = d->B;
  size_t n = B * d->M + B * d->H + 2 * B * d->H + B * d->S + B * d->U;
  if (d->zoneout_mode) n += 2 * B * d->H;      // the h carries of the two layers
  if (d->score_mode == 2) n += B * d->U + B * d->loc_k * d->U + (size_t)(d->loc_k + 1) * d->U;
  if (d->score_mode == 2) n += B * d->S + B * kLocParts * d->S;     // split kernels: dal, dcum_part
  // cell backward cut along the reduction: partial tiles + tickets per (32 units, 32 samples)
  const size_t nblk = (size_t)ceil_div(d->H, 32) * ceil_div(d->B, 32);
  n += nblk * kCbSplit * kCbSlabFloats + nblk + 64;
  const size_t nda = (size_t)ceil_div(d->M, 32) * ceil_div(d->B, 32);        // d(attention input), same scheme
  n += nda * kDaSplit * kDaSlabFloats + nda + 64;
  return n * sizeof(float) + 1024;
}

static bool cell_split(const os2s_attn_decoder_t* d) { return g_cell_split != 0 && d->U <= 16 * kCbWaves && d->H % 8 == 0; }

extern "C" int os2s_attn_decoder_bwd(os2s_stream_t stream_, const os2s_attn_decoder_t* d,
                                     const os2s_attn_decoder_grads_t* gr, void* workspace,
                                     size_t workspace_bytes) {
  const int rc = ad_check(d);
  if (rc != OS2S_OK) return rc;
  OS2S_REQUIRE(gr && workspace && d->gates[0] && gr->wcatT[0] && gr->wqT && gr->dg[0] && gr->dq_seq && gr->dctx_seq && gr->dkeys && gr->dpre_seq && gr->dmem);
  OS2S_REQUIRE(gr->dy_top || gr->dctx_ext);
  OS2S_REQUIRE(gr->dv);
  if (d->L == 2) OS2S_REQUIRE(d->gates[1] && gr->wcatT[1] && gr->dg[1]);
  if (d->score_mode == 1) OS2S_REQUIRE(gr->dg_scalar);
  if (d->score_mode == 2) OS2S_REQUIRE(gr->dconv_w && gr->dconv_b && gr->ddense_w);
  if (workspace_bytes < os2s_attn_decoder_bwd_workspace_bytes(d)) return OS2S_ERR_WORKSPACE;
  OS2S_REQUIRE(d->t_begin == 0 && d->t_end == d->T);
  if (d->zoneout_mode == 2) return OS2S_ERR_UNSUPPORTED;     // the expectation blend is the eval / infer form
  hipStream_t stream = (hipStream_t)stream_;
  const int keys_mode = attn_keys_mode(d, true);
  if (keys_mode == kKeysRefused) return OS2S_ERR_UNSUPPORTED;
  const size_t lds = attn_lds_bytes(d, true, keys_mode == kKeysLds);
  const int B = d->B, T = d->T, H = d->H, M = d->M, L = d->L, U = d->U, S = d->S;
  const int K = d->loc_k, F = d->loc_f;
  if (hipMemsetAsync(workspace, 0, os2s_attn_decoder_bwd_workspace_bytes(d), stream) != hipSuccess) return OS2S_ERR_LAUNCH;
  float* ws = (float*)workspace;
  float* dattn = ws; ws += (size_t)B * M;
  float* dhq = ws; ws += (size_t)B * H;
  float* dcc[2]; dcc[0] = ws; ws += (size_t)B * H; dcc[1] = ws; ws += (size_t)B * H;
  float* dhc[2] = {nullptr, nullptr};          // zoneout: the carries of the zoned h' (next to those of c': 16-byte rows)
  if (d->zoneout_mode) { dhc[0] = ws; ws += (size_t)B * H; dhc[1] = ws; ws += (size_t)B * H; }
  float* dcum = ws; ws += (size_t)B * S;
  float* dnv_acc = ws; ws += (size_t)B * U;
  float *dbd_acc = nullptr, *dwck_acc = nullptr, *unfold_tmp = nullptr;
  if (d->score_mode == 2) {
    dbd_acc = ws; ws += (size_t)B * U;
    dwck_acc = ws; ws += (size_t)B * K * U;
    unfold_tmp = ws; ws += (size_t)(K + 1) * U;
  }
  const bool split = loc_split(d);
  AdLoc lx;
  lx.e_part = nullptr; lx.dal = nullptr; lx.dcum_part = nullptr;
  if (d->score_mode == 2) {
    lx.dal = ws; ws += (size_t)B * S;
    lx.dcum_part = ws; ws += (size_t)B * kLocParts * S;
  }
  const size_t ncb = (size_t)ceil_div(H, 32) * ceil_div(B, 32);
  float* const cb_part = ws; ws += ncb * kCbSplit * kCbSlabFloats;
  int* const cb_ticket = reinterpret_cast<int*>(ws); ws += ncb;
  const bool csplit = cell_split(d);
  const size_t nda = (size_t)ceil_div(M, 32) * ceil_div(B, 32);
  float* const da_part = ws; ws += nda * kDaSplit * kDaSlabFloats;
  int* const da_ticket = reinterpret_cast<int*>(ws); ws += nda;
  const size_t lds_da = ((size_t)M + ceil_div(S, kLocCtxParts)) * sizeof(float);
  const size_t lds_sb = loc_bwd_lds_floats(S, K) * sizeof(float);
  // gate gradients of finished steps are zero; dkeys accumulates
  for (int l = 0; l < L; ++l)
    if (hipMemsetAsync(gr->dg[l], 0, (size_t)B * T * 4 * H * 2, stream) != hipSuccess) return OS2S_ERR_LAUNCH;
  if (hipMemsetAsync(gr->dq_seq, 0, (size_t)B * T * U * 2, stream) != hipSuccess) return OS2S_ERR_LAUNCH;
  if (hipMemsetAsync(gr->dctx_seq, 0, (size_t)B * T * M * 2, stream) != hipSuccess) return OS2S_ERR_LAUNCH;

  AdAttn at;
  ad_fill_attn(d, at);
  at.dctx_ext = (const bf16_t*)gr->dctx_ext; at.dctx_bs = gr->dctx_bs; at.dctx_ts = gr->dctx_ts;
  at.dattn = dattn; at.dctx_seq = (bf16_t*)gr->dctx_seq; at.dcum = dcum; at.dpre_seq = (bf16_t*)gr->dpre_seq;
  at.dq_seq = (bf16_t*)gr->dq_seq; at.dhq = dhq; at.dnv_acc = dnv_acc; at.dbd_acc = dbd_acc;
  at.dwck_acc = dwck_acc;
  const long long GH = 4LL * H;
  dim3 cgrid(ceil_div(H, kCellBwdRows), ceil_div(B, kCellBwdCols));
  const bool fast_sb = split && ad_fast_score_bwd(d);
  for (int t = T - 1; t >= 0; --t) {
    const int last = (t == T - 1);
    if (!last) {
      AdDattn g;
      g.B = B; g.M = M; g.K = (int)GH; g.wT = (const bf16_t*)gr->wcatT[0];
      g.dg = (const bf16_t*)gr->dg[0] + (long long)(t + 1) * GH; g.ld = (long long)T * GH; g.out = dattn;
      if (csplit && M % 4 == 0) {
        AdDattnSplit gs;
        gs.g = g; gs.part = da_part; gs.ticket = da_ticket;
        OS2S_LAUNCH(ad_dattn_split_kernel, dim3(ceil_div(M, 32), kDaSplit, ceil_div(B, 32)), dim3(64 * kDaWaves), 0,
                    stream, gs);
      } else {
        OS2S_LAUNCH(ad_dattn_kernel, dim3(ceil_div(M, 8), ceil_div(B, 32)), dim3(64 * kBwdWaves), 0, stream, g);
      }
    }
    at.t = t; at.last = last;
    if (split) {
      OS2S_LAUNCH(ad_loc_dalign_kernel, dim3(kLocCtxParts, B), dim3(256), lds_da, stream, at, lx);
      if (fast_sb) {
        const int r2 = ad_launch_fast_score_bwd(stream, at, lx, d);
        if (r2 != OS2S_OK) return r2;
      } else {
        OS2S_LAUNCH_LDS(ad_loc_score_bwd_kernel, dim3(kLocParts, B), dim3(kAttnThreads), lds_sb, stream, at, lx);
      }
    } else if (d->score_mode == 2) { OS2S_LAUNCH_LDS(ad_attn_bwd_kernel<true>, dim3(B), dim3(kAttnThreads), lds, stream, at); }
    else if (keys_mode == kKeysLds) {
      if (U <= 512) { OS2S_LAUNCH_LDS(ad_attn_bwd_kernel<false>, dim3(B), dim3(kAttnThreads), lds, stream, at); }
      else { OS2S_LAUNCH_LDS((ad_attn_bwd_kernel<false, 8>), dim3(B), dim3(kAttnThreads), lds, stream, at); }
    } else {
      if (U <= 512) { OS2S_LAUNCH_LDS((ad_attn_bwd_kernel<false, 4, false>), dim3(B), dim3(kAttnThreads), lds, stream, at); }
      else { OS2S_LAUNCH_LDS((ad_attn_bwd_kernel<false, 8, false>), dim3(B), dim3(kAttnThreads), lds, stream, at); }
    }
    for (int l = L - 1; l >= 0; --l) {
      AdCellBwd c;
      c.B = B; c.T = T; c.H = H; c.t = t; c.last = last; c.forget_bias = d->forget_bias; c.lens = d->tgt_len;
      c.dy_ext = nullptr; c.dy_bs = c.dy_ts = 0;
      c.dgA = nullptr; c.wAT = nullptr; c.KA = 0; c.dgA_ld = c.wAT_ld = 0;
      c.dq = nullptr; c.wqT = nullptr; c.KQ = 0; c.dq_ld = 0;
      if (l == L - 1) {
        c.dy_ext = (const bf16_t*)gr->dy_top; c.dy_bs = gr->dy_top_bs; c.dy_ts = gr->dy_top_ts;
        c.dq = (const bf16_t*)gr->dq_seq + (long long)t * U; c.dq_ld = (long long)T * U;
        c.wqT = (const bf16_t*)gr->wqT; c.KQ = U;
      } else {   // output feeds the layer above at the same step (columns 0..H of its cat)
        c.dgA = (const bf16_t*)gr->dg[l + 1] + (long long)t * GH; c.dgA_ld = (long long)T * GH;
        c.wAT = (const bf16_t*)gr->wcatT[l + 1]; c.wAT_ld = GH; c.KA = (int)GH;
      }
      c.dgB = (const bf16_t*)gr->dg[l] + (long long)(t + 1) * GH; c.dgB_ld = (long long)T * GH;
      c.wBT = (const bf16_t*)gr->wcatT[l] + (long long)(l == 0 ? M : H) * GH; c.wBT_ld = GH; c.KB = (int)GH;
      c.gates = (const bf16_t*)d->gates[l]; c.c_seq = d->c_seq[l]; c.dc_carry = dcc[l];
      c.dg_out = (bf16_t*)gr->dg[l]; c.out_keep = d->out_keep; c.out_seed = d->out_seed[l];
      c.zo = d->zoneout_mode == 1; c.zo_keep = 1.f - d->zoneout_prob;
      c.zo_seed_h = d->zoneout_seed_h[l]; c.zo_seed_c = d->zoneout_seed_c[l]; c.dh_carry = dhc[l];
      c.part = cb_part; c.ticket = cb_ticket;
      if (csplit) {
        OS2S_LAUNCH(ad_cell_bwd_split_kernel, dim3(ceil_div(H, 32), kCbSplit, ceil_div(B, 32)), dim3(64 * kCbWaves), 0,
                    stream, c);
      } else {
        OS2S_LAUNCH(ad_cell_bwd_kernel, cgrid, dim3(64 * kBwdWaves), 0, stream, c);
      }
    }
  }
  OS2S_LAUNCH(ad_dkeys_kernel, dim3(ceil_div((long long)S * U / 8, 256), B), dim3(256), 0, stream,
              (const bf16_t*)gr->dpre_seq, d->src_len, d->tgt_len, T, S, U, gr->dkeys);
  OS2S_LAUNCH(ad_dvalues_kernel, dim3(ceil_div(M, 256), ceil_div(S, 16), B), dim3(256), 0, stream, d->align_seq,
              (const bf16_t*)gr->dctx_seq, d->src_len, d->tgt_len, T, S, M, (bf16_t*)gr->dmem);
  OS2S_LAUNCH(ad_score_vec_grads_kernel, dim3(1), dim3(256), 0, stream, dnv_acc, B, U, d->score_mode,
              d->v, d->g, gr->dv, gr->dg_scalar);
  if (d->score_mode == 2) {
    OS2S_LAUNCH(ad_unfold_location_grads_kernel, dim3(1), dim3(256), 0, stream, dwck_acc, dbd_acc, B, K,
                F, U, d->conv_w, d->conv_b, d->dense_w, gr->dconv_w, gr->dconv_b, gr->ddense_w, unfold_tmp);
  }
  return OS2S_OK;
}

// ---- e4m3 weight copies -----------------------------------------------------------------------
// q[r, k] = e4m3(w[r, k] / scale[r]), scale[r] = max_k |w[r, k]| / 448 (OCP e4m3fn: largest finite
// value 448; an all-zero row gets scale 1). One wave per row, two passes over the row.
namespace os2s {
__global__ __launch_bounds__(256) void quantize_rows_e4m3_kernel(const bf16_t* __restrict__ w, int rows,
                                                               int K, uint8_t* __restrict__ q,
                                                               float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const bf16_t* wr = w + (long long)r * K;
  float amax = 0.f;
  for (int k = lane * 8; k < K; k += 512) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(wr + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fmaxf(fabsf(bflo(v[e])), fabsf(bfhi(v[e]))));
  }
  amax = wave_max(amax);
  const float sc = amax > 0.f ? amax / 448.f : 1.f;
  const float inv = 1.f / sc;
  if (lane == 0) scale[r] = sc;
  for (int k = lane * 8; k < K; k += 512) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(wr + k);
    u32x2 o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float a0 = fminf(fmaxf(bflo(v[2 * h]) * inv, -448.f), 448.f);
      const float a1 = fminf(fmaxf(bfhi(v[2 * h]) * inv, -448.f), 448.f);
      const float a2 = fminf(fmaxf(bflo(v[2 * h + 1]) * inv, -448.f), 448.f);
      const float a3 = fminf(fmaxf(bfhi(v[2 * h + 1]) * inv, -448.f), 448.f);
      int pk = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, 0, false);
      pk = __builtin_amdgcn_cvt_pk_fp8_f32(a2, a3, pk, true);
      o[h] = (uint32_t)pk;
    }
    *reinterpret_cast<u32x2*>(q + (long long)r * K + k) = o;
  }
}
}  // namespace os2s

extern "C" int os2s_quantize_rows_e4m3(os2s_stream_t stream, const uint16_t* w, int rows, int K,
                                       uint8_t* q, float* scale) {
  using namespace os2s;
  OS2S_REQUIRE(w && q && scale && rows >= 1 && K >= 8 && K % 8 == 0);
  OS2S_LAUNCH(quantize_rows_e4m3_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, w,
              rows, K, q, scale);
  return OS2S_OK;
}
