#!/usr/bin/env python
"""Micro-benchmarks of the kernels of one Transformer-big beam-search step (N = 256 beam rows):
skinny GEMMs per shape, the logits GEMM, decode attention, LayerNorm, the beam kernels.

  --mx    the MXFP8 skinny kernel (os2s_gemm_skinny_mx: every forced tile and the by-shape choice) next to the bf16
          skinny kernel's by-shape choice and the LDS-tiled bf16 GEMM the logits take, alternated in one process
  --step  ms per beam-search step of Transformer-big, 64 sentences x beam 4 (the workload of
          bench.py --only-transformer-infer), 'mxfp8_decode' off and on, two models alternated in one process"""
import argparse
import os
import time
import sys

import torch
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "lt"))
import lt_backend  # noqa: E402  (hipBLASLt comparison harness, tools only; loads its library at the first call)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openseq2seq_amd import _lib, capi  # noqa: E402


def timeit(fn, reps=20, warm=3):
  """GPU time per call: `reps` calls captured in one hipGraph (no host launch cost)."""
  for _ in range(warm):
    fn()
  torch.cuda.synchronize()
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for _ in range(reps):
      fn()
  g.replay()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(5):
    g.replay()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) * 1e3 / (5 * reps)


DECODE_SHAPES = {"proj 1024x1024": (1024, 1024), "qkv 3072x1024": (3072, 1024), "ffn-in 4096x1024": (4096, 1024),
                 "ffn-out 1024x4096": (1024, 4096), "logits 32768x1024": (32768, 1024)}
MX_TILES = ["32x32", "64x64", "64x128", "128x256", "256x256"]      # tile 0 .. 4 of capi.gemm_skinny_mx (m x n)


def bench_mx(dev, rows=256, rounds=5):
  """us per call, median over `rounds` alternated rounds, and the spread (max - min) / median of the bf16 column."""
  bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
  for name, (n, k) in DECODE_SHAPES.items():
    x, w = bf(rows, k), bf(n, k) * k ** -0.5
    wq, ws = capi.quantize_mx(w)
    cols = {"bf16 skinny": lambda: capi.gemm_skinny(x, w), "bf16 gemm": lambda: capi.gemm(x, w)}
    t = {c: [] for c in list(cols) + MX_TILES + ["mx auto"]}
    for _ in range(rounds):
      for c, fn in cols.items():
        t[c].append(timeit(fn))
      for v, c in enumerate(MX_TILES):
        t[c].append(timeit(lambda: capi.gemm_skinny_mx(x, wq, ws, tile=v)))
      t["mx auto"].append(timeit(lambda: capi.gemm_skinny_mx(x, wq, ws)))
    med = {c: sorted(v)[len(v) // 2] for c, v in t.items()}
    base = min(med["bf16 skinny"], med["bf16 gemm"])
    spread = max((max(v) - min(v)) / med[c] for c, v in t.items())
    print("%-18s rows %d  " % (name, rows) + "  ".join("%s %.1f" % (c, med[c]) for c in t) +
          "  us | best mx / best bf16 %.2f, spread %.1f %%" % (min(med[c] for c in MX_TILES) / base, 100 * spread),
          flush=True)


def bench_step(dev, batch=64, rounds=4):
  from openseq2seq_amd.configs.transformer import transformer_config
  models = {}
  for on in (False, True):
    model_cls, params = transformer_config(batch_size_per_gpu=batch)
    params["decoder_params"]["mxfp8_decode"] = on
    torch.manual_seed(0)
    models[on] = model_cls(params, mode="infer", hvd=None, device=dev)
    models[on].compile()
  data = models[False].get_data_layer().synthetic_batch(dev, seed=7)
  ms = {False: [], True: []}
  for r in range(rounds + 1):
    for on in (False, True):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      ids, _ = models[on].infer_batch(data)
      torch.cuda.synchronize()
      if r > 0:                     # round 0 warms up
        ms[on].append(1e3 * (time.perf_counter() - t0) / int(ids.shape[1]))
  for on in (False, True):
    print("mxfp8_decode %-5s ms per decode step (encoder included): %s  median %.4f" %
          (on, " ".join("%.4f" % v for v in ms[on]), sorted(ms[on])[len(ms[on]) // 2]), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--mx", action="store_true")
  ap.add_argument("--step", action="store_true")
  args = ap.parse_args()
  dev = torch.device("cuda:0")
  if args.mx or args.step:
    if args.mx:
      bench_mx(dev)
    if args.step:
      bench_step(dev)
    return
  N, D, H, F, V = 256, 1024, 16, 4096, 32768
  bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
  x, xf = bf(N, D), bf(N, F)
  for name, (n, k, inp) in {"qkv 3072x1024": (3 * D, D, x), "proj 1024x1024": (D, D, x),
                            "ffn-in 4096x1024": (F, D, x), "ffn-out 1024x4096": (D, F, xf),
                            "logits 32768x1024": (V, D, x)}.items():
    w = bf(n, k)
    try:     # gemm_skinny.variant: 0 = reg, 2 = l64, 1 = l32, 3 = wide, -1 = by shape
      t, t1, t3, t4 = [(_lib.set_option("gemm_skinny.variant", v), timeit(lambda: capi.gemm_skinny(inp, w)))[1]
                       for v in (0, 2, 1, 3)]
    finally:
      _lib.set_option("gemm_skinny.variant", -1)
    t5 = timeit(lambda: capi.gemm_skinny(inp, w))
    t2 = timeit(lambda: lt_backend.matmul_lt(inp, w, b_is_t=True))
    print("gemm %-18s reg %6.1f  lds64 %6.1f  lds32 %6.1f  wide %6.1f  auto %6.1f  hipBLASLt %6.1f us  (W %.1f MB)"
          % (name, t, t1, t3, t4, t5, t2, n * k * 2 / 1e6), flush=True)
  Tmax, step = 106, 50
  kc, vc = bf(N, Tmax, D), bf(N, Tmax, D)
  anc = torch.randint(0, N, (N, Tmax), device=dev, dtype=torch.int32)
  qkv = bf(N, 3 * D)
  t = timeit(lambda: capi.decode_self_attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], kc, vc, anc, H, step, 0.125))
  print("decode self-attention step %d: %.1f us (ideal %.1f us @8TB/s)" % (step, t, N * (step + 1) * D * 4 / 8e6))
  B, beam, S = 64, 4, 40
  cu = torch.arange(B + 1, device=dev, dtype=torch.int32) * S
  kv = bf(B * S, 2 * D)
  t = timeit(lambda: capi.decode_cross_attention(x, kv[:, :D], kv[:, D:], cu, beam, H, S, 0.125))
  print("decode cross-attention S=%d: %.1f us" % (S, t))
  g, b = torch.ones(D, device=dev), torch.zeros(D, device=dev)
  t = timeit(lambda: capi.layernorm_fwd(x, g, b, save=False))
  print("layernorm [256,1024]: %.1f us" % t)
  st = capi.BeamState(torch.zeros(B, dtype=torch.int32, device=dev), beam, V, 200, 0.6, 1)
  logits = bf(N, V)

  st2 = capi.BeamState(torch.zeros(B, dtype=torch.int32, device=dev), beam, V, 100000, 0.6, 1)
  t = timeit(lambda: st2.step(logits), reps=20)
  print("beam step (row top-k + select): %.1f us" % t)


if __name__ == "__main__":
  main()
