"""An eval-mode separable conv + BatchNorm + ReLU layer of QuartzNet 15x5 as ONE fused MXFP8 launch against the bf16
chain, each as TDNNEncoder issues it, at the five stride-1 layer classes of quartznet15x5_LibriSpeech.py and the
256 -> 512 transition (B = 32, the ragged lengths of bench.py's synthetic batch after the stride-2 first layer):

  bf16: os2s_depthwise_conv1d_fwd + os2s_conv1d_fwd (K = 1) + os2s_bn_finalize + os2s_bn_act_fwd
  vN:   os2s_bn_finalize + os2s_sepconv1d_fwd_mx_variant(variant = N) with scale / shift / ReLU / mask (the weight copy
        is cached), for every N of --variant: 0 the register-window FIR, 1 the depthwise phase on the matrix pipe
  vN block end: os2s_bn_finalize + the same launch with the identity epilogue + os2s_bn_act_fwd: the main branch of a
        residual block end, against the same bf16 chain (the residual branch is common to both)

Chain times from device events around windows of back-to-back chains, every shape warmed up, all chains alternated
inside one process; the median of the windows next to their spread ((max - min) / median). These are call times of
the chain, not a kernel's share of peak. `takes` is the rule parts/cnns/conv_blocks.py::mx_sep_wins / mx_sep_variant
encode: the fastest chain, if its median beats every other chain's by more than the larger of the two spreads.
`at K = 1`: the chain with a one-tap depthwise kernel; what it takes off the chain is the cost of the taps. rel L2:
the fused layer output against the bf16 one.
Prints a markdown table; --out writes it to a file as well.

  python tools/bench_sepconv_mx.py [--out sepconv_mx.md] [--windows 7] [--variant 0 1]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from openseq2seq_amd import capi  # noqa: E402

# (Cin, Cout, K): the first layer of a block of the next width, then the five classes of the 15 blocks
SHAPES = [(256, 256, 33), (256, 256, 39), (256, 512, 51), (512, 512, 51), (512, 512, 63), (512, 512, 75)]


def bench_lengths(B):
  """Frames per utterance of bench.py's synthetic batch (durations U[2, 16.7] s, 10 ms hop) after the stride-2 layer."""
  dur = np.random.RandomState(1234).uniform(2.0, 16.7, size=B)
  frames = np.array([1 + int(d * 16000) // 160 for d in dur], np.int64)
  lens = (frames + 1) // 2
  return lens, int(-(-int(frames.max()) // 16) * 16) // 2


def window(fn, n):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(n):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / n


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--calls", type=int, default=1000, help="chains per window")
  ap.add_argument("--variant", type=int, nargs="+", default=[0, 1], choices=[-1, 0, 1],
                  help="kernel variants of os2s_sepconv1d_fwd_mx_variant to time (0: FIR, 1: matrix pipe, -1: by shape)")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_sepconv_mx.py measures on the GPU; none found")
  dev = torch.device("cuda:0")
  B = args.batch
  lens_h, T = bench_lengths(B)
  lens = torch.from_numpy(lens_h.astype(np.int32)).to(dev)
  vs = args.variant
  per_v = lambda fmt: " | ".join(fmt % v for v in vs)
  lines = ["B = %d, T = %d, live rows %d of %d" % (B, T, int(lens_h.sum()), B * T), "",
           "| Cin | Cout | K | bf16 chain us | spread | of which depthwise / pointwise us | " +
           per_v("v%d chain us | spread | at K = 1 us | / bf16 | block-end chain us | spread | / bf16 | rel L2 vs bf16") +
           " | plain: takes | block end: takes |",
           "|---" * (6 + 8 * len(vs) + 2) + "|"]
  for cin, cout, K in SHAPES:
    torch.manual_seed(cin + cout + K)
    x = torch.randn(B, T, cin, device=dev).clamp_min(0.0).to(torch.bfloat16)       # a ReLU output
    x *= (torch.arange(T, device=dev)[None, :] < lens[:, None])[..., None]
    d = torch.randn(K, cin, device=dev) * (2.0 / K) ** 0.5
    w = (torch.randn(1, cout, cin, device=dev) * (2.0 / cin) ** 0.5).to(torch.bfloat16)
    gamma, beta = 0.5 + torch.rand(cout, device=dev), torch.randn(cout, device=dev) * 0.1
    mean, var = torch.randn(cout, device=dev) * 0.1, 0.5 + torch.rand(cout, device=dev)
    sc, sh = torch.empty(cout, device=dev), torch.empty(cout, device=dev)
    y = torch.empty(B, T, cout, device=dev, dtype=torch.bfloat16)
    out16 = torch.empty_like(y)
    wq, ws = capi.quantize_mx(w.view(cout, cin))
    zbuf = []

    def finalize():
      capi.bn_finalize(None, B * T, gamma, beta, 1e-3, 0.9, False, mean, var, None, None, sc, sh)

    def depthwise():
      zbuf[:] = [capi.depthwise_conv1d_fwd(x, d, in_len=lens)]

    def pointwise():
      capi.conv1d_fwd(zbuf[0], w, pad_left=0, tout=T, out=y)

    def bf16():
      depthwise()
      pointwise()
      finalize()
      capi.bn_act_fwd([y], [sc], [sh], out16, lens, 1, 1.0, 0)

    d1, y8 = d[:1].contiguous(), torch.empty_like(y)
    outs = {v: torch.empty_like(y) for v in vs}
    scratch = torch.empty_like(y)

    def mx(v, taps=d, out=None):   # the plain layer; taps = d1: a one-tap depthwise, what is left is not the tap loop
      def f():
        finalize()
        capi.sepconv1d_fwd_mx(x, taps, wq, ws, in_len=lens, out_len=lens, ch_scale=sc, ch_shift=sh, act=1,
                              out=scratch if out is None else out, variant=v)
      return f

    def mx_end(v):    # a residual block end's main branch: identity epilogue, then the BatchNorm / activation pass
      def f():
        finalize()
        capi.sepconv1d_fwd_mx(x, d, wq, ws, in_len=lens, out_len=lens, out=y8, variant=v)
        capi.bn_act_fwd([y8], [sc], [sh], scratch, lens, 1, 1.0, 0)
      return f
    fns = {"bf16": bf16, "dw": depthwise, "pw": pointwise}
    for v in vs:
      fns.update({("mx", v): mx(v, out=outs[v]), ("k1", v): mx(v, d1), ("end", v): mx_end(v)})
    for f in fns.values():
      for _ in range(3):
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(args.windows):                    # alternate the chains
      for k, f in fns.items():
        t[k].append(window(f, args.calls) * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}

    def takes(kind):  # the fastest chain, if it beats every other by more than the larger of the two spreads
      best = min(["bf16"] + [(kind, v) for v in vs], key=lambda k: med[k])
      clear = all(med[best] < med[k] * (1.0 - max(spread[best], spread[k]))
                  for k in ["bf16"] + [(kind, v) for v in vs] if k != best)
      name = best if best == "bf16" else "v%d" % best[1]
      return name if clear else name + " (inside the spread)"
    cells = []
    for v in vs:
      mx(v, out=outs[v])()
      bf16()
      rel = float((outs[v].float() - out16.float()).norm() / out16.float().norm())
      cells.append("%.1f | %.1f %% | %.1f | %.2f | %.1f | %.1f %% | %.2f | %.2e" % (
          med["mx", v], 100 * spread["mx", v], med["k1", v], med["mx", v] / med["bf16"], med["end", v],
          100 * spread["end", v], med["end", v] / med["bf16"], rel))
    lines.append("| %d | %d | %d | %.1f | %.1f %% | %.1f / %.1f | %s | %s | %s |" % (
        cin, cout, K, med["bf16"], 100 * spread["bf16"], med["dw"], med["pw"], " | ".join(cells), takes("mx"),
        takes("end")))
    print(lines[-1], flush=True)
    del x, w, y, out16, outs, scratch, wq
  text = "\n".join(lines) + "\n"
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text)


if __name__ == "__main__":
  main()
