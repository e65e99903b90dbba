"""Attention kernels on their own at the Transformer-big training shape (B=256 sequences, lengths
U[8,56], 16 heads of 64, QKV packed [tokens, 3*1024], attention dropout 0.1): microseconds per launch
for self-attention (encoder), causal self-attention (decoder) and cross attention, forward and
backward, against the HBM time of the bytes each launch has to move and the MFMA time of the FLOPs it
executes (4 L^2 dh forward, 10 L^2 dh backward per head and sentence, halved under the causal mask).

  python tools/bench_attention.py [--batch 256] [--iters 50] [--min_len 8] [--max_len 56] [--head_dim 64]

Sentence lengths are U[min_len, max_len]. Up to --max_len 64 the launches are the one-tile kernels of
csrc/attention.hip (attn_fwd_kernel / attn_bwd_kernel<DH, kDrop>); beyond it the tile-walking training kernels
(attn_fwd_long_kernel<DH, kDrop> there, the two-launch backward of csrc/attention_long.hpp), called with max_len
rounded up to the kernels' 64-token tile. --head_dim 8 / 16 / 32 / 64 / 128 keeps the model width of 1024: 1024 /
head_dim heads, scale head_dim ** -0.5. To compare rows, keep batch * mean length about equal.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_US = 8e6       # 8 TB/s (spec)
MFMA_FLOPS_PER_US = 2.5e9    # 2.5 PFLOP/s dense bf16 (spec)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=256)
  ap.add_argument("--iters", type=int, default=50)
  ap.add_argument("--keep", type=float, default=0.9)
  ap.add_argument("--min_len", type=int, default=8)
  ap.add_argument("--max_len", type=int, default=56)
  ap.add_argument("--head_dim", type=int, default=64, choices=(8, 16, 32, 64, 128))
  args = ap.parse_args()
  if not 1 <= args.min_len <= args.max_len:
    ap.error("need 1 <= min_len <= max_len")
  from openseq2seq_amd import capi
  dev = torch.device("cuda:0")
  rng = np.random.RandomState(0)
  D, dh = 1024, args.head_dim
  H, scale = D // dh, dh ** -0.5
  lq = rng.randint(args.min_len, args.max_len + 1, size=args.batch)
  lk = rng.randint(args.min_len, args.max_len + 1, size=args.batch)
  T = capi.ATTENTION_TILE
  max_len = (args.max_len + T - 1) // T * T
  print("lengths U[%d,%d], batch %d, max_len %d, %d heads of %d: %s kernels" %
        (args.min_len, args.max_len, args.batch, max_len, H, dh, "one-tile" if max_len <= T else "tile-walking"))

  def cu(l):
    return torch.tensor([0] + list(np.cumsum(l)), dtype=torch.int32, device=dev)

  def timed(fn):
    for _ in range(5):
      fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
      fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.iters

  for name, causal, cross in (("self", False, False), ("causal", True, False), ("cross", False, True)):
    lkk = lk if cross else lq
    nq, nk = int(lq.sum()), int(lkk.sum())
    cq, ck = cu(lq), cu(lkk)
    if cross:
      qb = torch.randn(nq, D, device=dev).to(torch.bfloat16)
      kvb = torch.randn(nk, 2 * D, device=dev).to(torch.bfloat16)
      q, k, v = qb, kvb[:, :D], kvb[:, D:]
    else:
      qkv = torch.randn(nq, 3 * D, device=dev).to(torch.bfloat16)
      q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    do = torch.randn(nq, D, device=dev).to(torch.bfloat16)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    o, lse = capi.attention_fwd(q, k, v, cq, ck, H, max_len, causal, scale, args.keep, 1, dh=dh)
    tf = timed(lambda: capi.attention_fwd(q, k, v, cq, ck, H, max_len, causal, scale, args.keep, 1, dh=dh))
    tb = timed(lambda: capi.attention_bwd(q, k, v, do, lse, dq, dk, dv, cq, ck, H, max_len, causal, scale,
                                          args.keep, 1, dh=dh))
    fb = (2 * nq + 2 * nk) * D * 2            # q, o + k, v
    bb = (3 * nq + 4 * nk) * D * 2            # q, do, dq + k, v, dk, dv
    pairs = float((lq.astype(np.float64) * lkk).sum()) * (0.5 if causal else 1.0)    # live (query, key) pairs
    ff, bf = 4 * pairs * dh * H, 10 * pairs * dh * H
    print("%-6s tokens q=%d k=%d  fwd %.1f us (HBM time %.1f us, MFMA time %.2f us = %.1f%% of peak)  "
          "bwd %.1f us (HBM time %.1f us, MFMA time %.2f us = %.1f%% of peak)" %
          (name, nq, nk, tf, fb / HBM_BYTES_PER_US, ff / MFMA_FLOPS_PER_US, 100 * ff / MFMA_FLOPS_PER_US / tf,
           tb, bb / HBM_BYTES_PER_US, bf / MFMA_FLOPS_PER_US, 100 * bf / MFMA_FLOPS_PER_US / tb))


if __name__ == "__main__":
  main()
