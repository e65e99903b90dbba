"""The dense wide-head cross-attention (csrc/attention_wide.hip) on its own at Centaur's shapes: B = 32 utterances,
one head of 512, the source padded to S = 184 characters, Tq = 500 decoder steps (1000 frames at reduction factor 2),
attention dropout 0.1: microseconds per launch, forward and backward (two launches), against the HBM time of the
bytes a call has to move (q, k, v, o and the fp32 probabilities, which are an output) and the MFMA time of its FLOPs
(4 Tq S D forward, 10 Tq S D backward per head and utterance).

  python tools/bench_attention_wide.py [--batch 32] [--tq 500] [--src 184] [--head_dim 512] [--heads 1] [--iters 50]

--tq 1 is the last step's share of a free-running decode pass (one query against the whole source).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_US = 8e6       # 8 TB/s (spec)
MFMA_FLOPS_PER_US = 2.5e9    # 2.5 PFLOP/s dense bf16 (spec)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--tq", type=int, default=500)
  ap.add_argument("--src", type=int, default=184)
  ap.add_argument("--head_dim", type=int, default=512, choices=(32, 64, 128, 256, 512))
  ap.add_argument("--heads", type=int, default=1)
  ap.add_argument("--keep", type=float, default=0.9)
  ap.add_argument("--iters", type=int, default=50)
  args = ap.parse_args()
  from openseq2seq_amd import _lib, capi
  dev = torch.device("cuda:0")
  B, Tq, S, D, H = args.batch, args.tq, args.src, args.head_dim, args.heads
  C, scale = H * D, D ** -0.5
  g = torch.Generator(device="cpu").manual_seed(0)
  q = torch.randn(B, Tq, C, generator=g).to(torch.bfloat16).to(dev)
  kv = torch.randn(B, S, 2 * C, generator=g).to(torch.bfloat16).to(dev)
  k, v = kv[:, :, :C], kv[:, :, C:]
  d_o = torch.randn(B, Tq, C, generator=g).to(torch.bfloat16).to(dev)
  lens = torch.randint(64, S + 1, (B,), generator=g)
  kb = (torch.arange(S)[None, :] >= lens[:, None]).float().mul(-1e9).to(dev)
  dq, dkv = torch.empty_like(q), torch.empty_like(kv)
  dk, dv = dkv[:, :, :C], dkv[:, :, C:]

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

  # the entry points themselves, on buffers allocated once: the wrappers of capi.py allocate their outputs per call,
  # which at these sizes costs the host more than the kernels take
  o, p, _ = capi.attention_wide_fwd(q, k, v, kb, H, scale, args.keep, 1)
  ds = torch.empty((B, H, Tq, S), dtype=torch.bfloat16, device=dev)
  st = capi._stream()
  ptr = lambda t: _lib.c_void_p(t.data_ptr())
  fargs = (st, ptr(q), ptr(k), ptr(v), ptr(kb), None, ptr(o), ptr(p), None, B, H, D, Tq, S, C, 2 * C, 2 * C, C, 0, 0,
           scale, args.keep, 1)
  bargs = (st, ptr(q), ptr(k), ptr(v), ptr(d_o), ptr(p), ptr(ds), ptr(dq), ptr(dk), ptr(dv), B, H, D, Tq, S, C, 2 * C,
           2 * C, C, C, 2 * C, 2 * C, scale, args.keep, 1)
  tf = timed(lambda: _lib.C.os2s_attention_wide_fwd(*fargs))
  tb = timed(lambda: _lib.C.os2s_attention_wide_bwd(*bargs))
  pb = B * H * Tq * S * 4
  fb = (2 * B * Tq + 2 * B * S) * C * 2 + pb                   # q, o, k, v, p out
  bb = (3 * B * Tq + 5 * B * S) * C * 2 + 2 * pb + 2 * (pb // 2)     # q, do, dq, k, v (twice), dk, dv; p twice; dS out + in
  ff, bf = 4.0 * B * H * Tq * S * D, 10.0 * B * H * Tq * S * D
  print("B %d, %d head(s) of %d, Tq %d, S %d, keep %.2f" % (B, H, D, Tq, S, args.keep))
  print("fwd %.1f us (HBM time %.1f us, MFMA time %.2f us = %.1f%% of peak)" %
        (tf, fb / HBM_BYTES_PER_US, ff / MFMA_FLOPS_PER_US, 100 * ff / MFMA_FLOPS_PER_US / tf))
  print("bwd %.1f us (HBM time %.1f us, MFMA time %.2f us = %.1f%% of peak)" %
        (tb, bb / HBM_BYTES_PER_US, bf / MFMA_FLOPS_PER_US, 100 * bf / MFMA_FLOPS_PER_US / tb))


if __name__ == "__main__":
  main()
