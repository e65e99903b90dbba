// Final-state classification head of the LSTM language model's text-classification phase, gfx950.
//
// Reference: encoders/lm_encoders.py:362-373 (the last layer's final state, h or concat([h, c], axis=1), through
// tf.layers.Dense to fc_dim = num_classes logits) and losses/cross_entropy_loss.py (tf.losses.softmax_cross_entropy
// of one-hot labels: the per-sample -sum_c y_c log softmax(logits)_c, summed and divided by B).
//   logits[b,c] = bias[c] + sum_d s[b,d] W[c,d]          s[b] = hT[b] or [hT[b], cT[b]], D = H or 2H
//   loss        = (1/B) sum_b sum_c y[b,c] (lse_b - logits[b,c])
//   dlogits     = (softmax * sum_c y_c - y) / B * loss scale
//   dW[c,d]    += sum_b dlogits[b,c] s[b,d],  dbias[c] += sum_b dlogits[b,c],  ds[b,d] = sum_c dlogits[b,c] W[c,d]
// The state never exists concatenated: the kernels take the two fp32 [B,H] pointers, and an 8-unit chunk of d lies
// wholly in one of them because H % 8 == 0. C <= 16 classes sit in registers. Three launches:
//   1. forward: one wave per sample, lane l owns the chunks l, l + 64, ...; C wave reductions;
//   2. loss: one workgroup; thread i takes samples i, i + 256, ... and the 256 partial losses are summed by a
//      fixed LDS tree;
//   3. backward: workgroups [0, B) are one wave per sample for ds (lane-local, no reduction); the workgroups after
//      them hold one thread per (class, chunk) of dW, which walks the batch in order, and the last C threads of the
//      grid's tail do the same for dbias. No atomics anywhere: every output is bit-identical on a rerun.
// Everything is fp32 except W, the parameter store's bf16 compute copy.
#include "os2s_common.hpp"

namespace os2s {

constexpr int kClsMax = 16;

__device__ __forceinline__ void cls_ld8(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}
__device__ __forceinline__ void cls_st8(float* p, const float (&v)[8]) {
  const f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
  *reinterpret_cast<f32x4*>(p) = a;
  *reinterpret_cast<f32x4*>(p + 4) = b;
}
__device__ __forceinline__ void cls_ld8bf(const bf16_t* p, float (&v)[8]) {
  const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[2 * e] = bflo(q[e]); v[2 * e + 1] = bfhi(q[e]); }
}
// the 8 units of chunk ch of sample b's state: chunks [0, H/8) are h, [H/8, 2H/8) are c
__device__ __forceinline__ const float* cls_state(const float* h, const float* c, int b, int H, int ch) {
  const int hch = H >> 3;
  return ch < hch ? h + (long long)b * H + ch * 8 : c + (long long)b * H + (ch - hch) * 8;
}

struct ClsFwdArgs {
  const float* h; const float* c;   // [B,H]; c null: D = H
  const bf16_t* w;                  // [C,D]
  const float* bias;                // [C] or null
  float* logits;                    // [B,C]
  int B, H, C;
};

__global__ __launch_bounds__(64) void text_cls_fwd_kernel(ClsFwdArgs p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int D = p.c ? 2 * p.H : p.H, nchunk = D >> 3;
  float acc[kClsMax];
#pragma unroll
  for (int k = 0; k < kClsMax; ++k) acc[k] = 0.f;
  for (int ch = lane; ch < nchunk; ch += 64) {
    float s[8];
    cls_ld8(cls_state(p.h, p.c, b, p.H, ch), s);
#pragma unroll
    for (int k = 0; k < kClsMax; ++k) {
      if (k < p.C) {                // wave-uniform
        float w[8];
        cls_ld8bf(p.w + (long long)k * D + ch * 8, w);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k] += s[e] * w[e];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kClsMax; ++k) {
    if (k < p.C) {
      const float v = wave_sum(acc[k]);
      if (lane == k) p.logits[(long long)b * p.C + k] = v + (p.bias ? p.bias[k] : 0.f);
    }
  }
}

struct ClsLossArgs {
  const float* logits;              // [B,C]
  const float* labels;              // [B,C] dense (one-hot or soft)
  const float* scale_dev;           // device loss scale or null (1)
  float* loss;                      // [1]
  float* dlogits;                   // [B,C] or null
  int B, C;
};

__global__ __launch_bounds__(256) void text_cls_loss_kernel(ClsLossArgs p) {
  __shared__ float red[256];
  const int tid = threadIdx.x, C = p.C;
  const float invB = 1.f / (float)p.B;
  const float gs = p.dlogits ? invB * (p.scale_dev ? p.scale_dev[0] : 1.f) : 0.f;
  float part = 0.f;
  for (int b = tid; b < p.B; b += 256) {
    float l[kClsMax], y[kClsMax], ex[kClsMax];
    float m = -INFINITY;
    int km = 0;                     // the first largest logit
#pragma unroll
    for (int k = 0; k < kClsMax; ++k) {
      l[k] = k < C ? p.logits[(long long)b * C + k] : -INFINITY;
      y[k] = k < C ? p.labels[(long long)b * C + k] : 0.f;
      if (l[k] > m) { m = l[k]; km = k; }
    }
    // log sum exp of the shifted logits as log1p of the sum WITHOUT the largest term (which is exp(0) = 1): the
    // loss of a confidently right sample, log(1 + tiny), keeps its relative accuracy
    float rest = 0.f, ysum = 0.f;
#pragma unroll
    for (int k = 0; k < kClsMax; ++k) {
      ex[k] = 0.f;
      if (k < C) {
        l[k] -= m;                  // <= 0
        ex[k] = k == km ? 1.f : expf(l[k]);
        if (k != km) rest += ex[k];
        ysum += y[k];
      }
    }
    const float lse = log1pf(rest), se = 1.f + rest;
    float lb = 0.f;
#pragma unroll
    for (int k = 0; k < kClsMax; ++k) {
      if (k < C) {
        lb += y[k] * (lse - l[k]);  // both parts >= 0: no cancellation
        if (p.dlogits) p.dlogits[(long long)b * C + k] = (ex[k] / se * ysum - y[k]) * gs;
      }
    }
    part += lb;
  }
  red[tid] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) p.loss[0] = red[0] * invB;
}

struct ClsBwdArgs {
  const float* h; const float* c;   // [B,H]; c null: D = H
  const bf16_t* w;                  // [C,D]
  const float* dlogits;             // [B,C]
  float* dw;                        // [C,D], accumulated into
  float* dbias;                     // [C] or null, accumulated into
  float* dh; float* dc;             // [B,H] written; dc null exactly when c is
  int B, H, C, wblocks;             // wblocks: workgroups of the dW part
};

__global__ __launch_bounds__(64) void text_cls_bwd_kernel(ClsBwdArgs p) {
  const int lane = threadIdx.x, C = p.C, H = p.H;
  const int D = p.c ? 2 * H : H, nchunk = D >> 3, hch = H >> 3;
  if ((int)blockIdx.x < p.B) {      // the state gradient of one sample
    const int b = blockIdx.x;
    float dl[kClsMax];
#pragma unroll
    for (int k = 0; k < kClsMax; ++k) dl[k] = k < C ? p.dlogits[(long long)b * C + k] : 0.f;
    for (int ch = lane; ch < nchunk; ch += 64) {
      float ds[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) ds[e] = 0.f;
#pragma unroll
      for (int k = 0; k < kClsMax; ++k) {
        if (k < C) {
          float w[8];
          cls_ld8bf(p.w + (long long)k * D + ch * 8, w);
#pragma unroll
          for (int e = 0; e < 8; ++e) ds[e] += dl[k] * w[e];
        }
      }
      float* out = ch < hch ? p.dh + (long long)b * H + ch * 8 : p.dc + (long long)b * H + (ch - hch) * 8;
      cls_st8(out, ds);
    }
    return;
  }
  const int wb = (int)blockIdx.x - p.B;
  if (wb < p.wblocks) {             // one thread per (class, chunk) of dW, the batch walked in order
    const int i = wb * 64 + lane;
    if (i >= C * nchunk) return;
    const int k = i / nchunk, ch = i - k * nchunk;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int b = 0; b < p.B; ++b) {
      float s[8];
      cls_ld8(cls_state(p.h, p.c, b, H, ch), s);
      const float g = p.dlogits[(long long)b * C + k];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += g * s[e];
    }
    float* out = p.dw + (long long)k * D + ch * 8;
    float cur[8];
    cls_ld8(out, cur);
#pragma unroll
    for (int e = 0; e < 8; ++e) cur[e] += acc[e];
    cls_st8(out, cur);
    return;
  }
  if (p.dbias && lane < C) {        // the last workgroup: dbias
    float acc = 0.f;
    for (int b = 0; b < p.B; ++b) acc += p.dlogits[(long long)b * C + lane];
    p.dbias[lane] += acc;
  }
}

}  // namespace os2s

using namespace os2s;

static bool text_cls_shape_ok(int H, int C) { return H >= 8 && H <= 2048 && H % 8 == 0 && C >= 2 && C <= kClsMax; }

extern "C" int os2s_text_cls_fwd(os2s_stream_t stream, const float* hT, const float* cT, const uint16_t* w,
                                 const float* bias, int B, int H, int C, float* logits) {
  OS2S_REQUIRE(hT && w && logits && B >= 1);
  if (!text_cls_shape_ok(H, C)) return OS2S_ERR_UNSUPPORTED;
  ClsFwdArgs a;
  a.h = hT; a.c = cT; a.w = (const bf16_t*)w; a.bias = bias; a.logits = logits; a.B = B; a.H = H; a.C = C;
  OS2S_LAUNCH(text_cls_fwd_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  return OS2S_OK;
}

extern "C" int os2s_softmax_xent_dense(os2s_stream_t stream, const float* logits, const float* labels, int B, int C,
                                       const float* grad_scale_dev, float* loss, float* dlogits) {
  OS2S_REQUIRE(logits && labels && loss && B >= 1);
  if (C < 2 || C > kClsMax) return OS2S_ERR_UNSUPPORTED;
  ClsLossArgs a;
  a.logits = logits; a.labels = labels; a.scale_dev = grad_scale_dev; a.loss = loss; a.dlogits = dlogits;
  a.B = B; a.C = C;
  OS2S_LAUNCH(text_cls_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  return OS2S_OK;
}

extern "C" int os2s_text_cls_bwd(os2s_stream_t stream, const float* hT, const float* cT, const uint16_t* w,
                                 const float* dlogits, int B, int H, int C, float* dw, float* dbias, float* dhT,
                                 float* dcT) {
  OS2S_REQUIRE(hT && w && dlogits && dw && dhT && B >= 1);
  OS2S_REQUIRE((cT == nullptr) == (dcT == nullptr));
  if (!text_cls_shape_ok(H, C)) return OS2S_ERR_UNSUPPORTED;
  ClsBwdArgs a;
  a.h = hT; a.c = cT; a.w = (const bf16_t*)w; a.dlogits = dlogits; a.dw = dw; a.dbias = dbias; a.dh = dhT; a.dc = dcT;
  a.B = B; a.H = H; a.C = C;
  a.wblocks = ceil_div((long long)C * ((cT ? 2 * H : H) / 8), 64);
  OS2S_LAUNCH(text_cls_bwd_kernel, dim3(B + a.wblocks + 1), dim3(64), 0, (hipStream_t)stream, a);
  return OS2S_OK;
}
