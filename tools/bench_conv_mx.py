"""An eval-mode conv + BatchNorm + ReLU layer of Jasper 10x5 on the MXFP8 path against the bf16 path, each chain as
TDNNEncoder issues it, at every stride-1 layer shape of jasper10x5_LibriSpeech_nvgrad_masks.py (B = 32, the ragged
lengths of bench.py's synthetic batch after the stride-2 first layer):

  mx:   os2s_mx_quantize_rows (activation) + os2s_bn_finalize + os2s_conv1d_fwd_mx with scale / shift / ReLU / mask
  bf16: os2s_conv1d_fwd + os2s_bn_finalize + os2s_bn_act_fwd

Chain times from device events around windows of back-to-back chains, every shape warmed up, the two chains
alternated inside one process; the median of the windows next to their spread ((max - min) / median). FLOP/s = 2 B T
Cin Cout K over the chain time of the PADDED batch (a call time, not a kernel's share of peak). `wins` is the rule
parts/cnns/conv_blocks.py::mx_conv_wins encodes: the mx median beats the bf16 median by more than both spreads.
Prints a markdown table; --out writes it to a file as well.

  python tools/bench_conv_mx.py [--out conv_mx.md] [--windows 7]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from openseq2seq_amd import capi  # noqa: E402
from openseq2seq_amd.configs.jasper import jasper_convnet_layers  # noqa: E402


def layer_shapes():
  """(Cin, Cout, K, dil) of every stride-1 layer class of the config, in order of first appearance."""
  out, cin = [], 64
  for blk in jasper_convnet_layers():
    for _ in range(blk["repeat"]):
      s = (cin, blk["num_channels"], blk["kernel_size"][0], blk["dilation"][0])
      if blk["stride"][0] == 1 and s not in out:
        out.append(s)
      cin = blk["num_channels"]
  return out


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


def block_ends(args, dev, B, T, lens_h, lens):
  """--block-ends: the ten dense-residual block ends of Jasper 10x5 in eval mode (end k: Cout x Cout x K main
  convolution + k + 1 residual 1x1 branches), three chains as the layers issue them, alternated in one process:

    bf16:   os2s_conv1d_fwd + bn_finalize, the dense-residual end (dres_bn_fwd + the concatenated 1x1 GEMM), bn_act_fwd
    mx:     the same with the main convolution on os2s_conv1d_fwd_mx (identity epilogue) where mx_conv_wins — the block
            end of 'mxfp8_inference' before the fused launch; equal to bf16 where that rule keeps bf16
    fused:  quantise x + os2s_conv1d_block_end_fwd_mx; fused+src: the same plus the quantiser of the newest source
            (the block's input, when the block's first layer kept bf16 and did not leave its MXFP8 copy)

  The source copies of the dense-residual pass (one per source and pass, shared by all ends) are not timed, and the
  dense-residual end runs on the timing stream, not next to the block's layers: both favour bf16 / mx."""
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.parts.cnns import conv_blocks as cb
  from openseq2seq_amd.parts.cnns.dense_residual import DenseResidualPlan
  blocks = [blk for blk in jasper_convnet_layers() if blk.get("residual")]
  widths, ks = [blk["num_channels"] for blk in blocks], [blk["kernel_size"][0] for blk in blocks]
  src_c = [jasper_convnet_layers()[0]["num_channels"]] + widths[:-1]
  torch.manual_seed(0)
  store = FlatParams(dev)
  mains = [cb.ConvBN(store, "m%d" % k, "m%d/bn" % k, widths[k], widths[k], ks[k]) for k in range(len(blocks))]
  res = [[cb.ConvBN(store, "e%d/r%d" % (k, i), "e%d/bn%d" % (k, i), src_c[i], widths[k], 1,
                    initializer=cb.glorot_uniform_conv) for i in range(k + 1)] for k in range(len(blocks))]
  store.finalize()
  for L in mains + [br for e in res for br in e]:
    L.gamma.master.copy_(0.5 + torch.rand(L.cout))
    L.beta.master.copy_(torch.randn(L.cout) * 0.1)
    L.moving_mean.copy_(torch.randn(L.cout) * 0.1)
    L.moving_var.copy_(0.5 + torch.rand(L.cout))
  mask = (torch.arange(T, device=dev)[None, :] < lens[:, None])[..., None]

  def act(c):                                        # a masked ReLU output
    return cb.Act((torch.randn(B, T, c, device=dev).clamp_min(0.0) * mask).to(torch.bfloat16), lens,
                  requires_grad=False)
  cb.mx_block_end_wins = lambda cout, k, sources: True      # every class is measured, whatever the rule says today
  srcs = [act(c) for c in src_c]
  dpass = DenseResidualPlan(res, dev).begin(False)
  for s in srcs:
    dpass.add_source(s)
  lines = ["B = %d, T = %d, live rows %d of %d" % (B, T, int(lens_h.sum()), B * T), "",
           "| end | Cout | K | sources (channels) | bf16 ms | mx ms | fused ms | fused+src ms | fused / min(bf16, mx) "
           "| fused+src / min | spread bf16 / mx / fused | wins | rel L2 fused vs bf16 |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
  for k, main in enumerate(mains):
    x = act(widths[k])
    outs = {}

    def old(mx):
      main.mxfp8, x.mx = mx, None
      outs[mx] = cb.conv_bn_dres_actv(main, x, dpass.forward_end(k), lens, "relu", False, None).data

    def fused(cold=False):
      main.mxfp8, x.mx = True, None
      if cold:
        srcs[k].mx = None
      outs["fused"] = cb.conv_bn_res_bn_actv(main, res[k], x, srcs[:k + 1], lens, "relu", False, None).data
    fns = {"bf16": lambda: old(False), "mx": lambda: old(True), "fused": fused, "fused+src": lambda: fused(True)}
    n = max(8, int(3e13 / (2.0 * B * T * widths[k] * (widths[k] * ks[k] + sum(src_c[:k + 1])))))
    for f in fns.values():
      for _ in range(3):
        f()
    torch.cuda.synchronize()
    t = {name: [] for name in fns}
    for _ in range(args.windows):                    # alternate the chains
      for name, f in fns.items():
        t[name].append(window(f, n))
    med = {name: statistics.median(v) for name, v in t.items()}
    spread = {name: (max(v) - min(v)) / med[name] for name, v in t.items()}
    best = min(med["bf16"], med["mx"])
    worst_spread = max(spread.values())
    rel = float((outs["fused"].float() - outs[False].float()).norm() / outs[False].float().norm())
    lines.append("| %d | %d | %d | %d (%d) | %.3f | %.3f | %.3f | %.3f | %.2f | %.2f | %.1f %% / %.1f %% / %.1f %% | %s "
                 "| %.2e |" % (
                     k, widths[k], ks[k], k + 1, sum(src_c[:k + 1]), med["bf16"], med["mx"], med["fused"],
                     med["fused+src"], med["fused"] / best, med["fused+src"] / best, 100 * spread["bf16"],
                     100 * spread["mx"], 100 * spread["fused"],
                     "yes" if med["fused+src"] / best < 1.0 - worst_spread else "no", rel))
    print(lines[-1], flush=True)
  return lines


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--block-ends", action="store_true", help="the dense-residual block ends instead of the plain layers")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_conv_mx.py measures on the GPU; none found")
  dev = torch.device("cuda:0")
  B = args.batch
  lens_h, T = bench_lengths(B)
  lens = torch.from_numpy(lens_h.astype(np.int32)).to(dev)
  if args.block_ends:
    text = "\n".join(block_ends(args, dev, B, T, lens_h, lens)) + "\n"
    print(text)
    if args.out:
      with open(args.out, "w") as f:
        f.write(text)
    return
  lines = ["B = %d, T = %d, live rows %d of %d" % (B, T, int(lens_h.sum()), B * T), "",
           "| Cin | Cout | K | dil | bf16 chain ms (TF/s) | mx chain ms (TF/s) | of which quantise ms | mx / bf16 "
           "| spread bf16 / mx | wins | rel L2 mx vs bf16 |", "|---|---|---|---|---|---|---|---|---|---|---|"]
  for cin, cout, K, dil in layer_shapes():
    torch.manual_seed(cin + cout + K)
    x = torch.randn(B, T, cin, device=dev).clamp_min(0.0).to(torch.bfloat16)       # a ReLU output
    x *= (torch.arange(T, device=dev)[None, :] < lens[:, None])[..., None]
    w = (torch.randn(K, cout, cin, device=dev) * (2.0 / (K * cin)) ** 0.5).to(torch.bfloat16)
    gamma, beta = 0.5 + torch.rand(cout, device=dev), torch.randn(cout, device=dev) * 0.1
    mean, var = torch.randn(cout, device=dev) * 0.1, 0.5 + torch.rand(cout, device=dev)
    sc, sh = torch.empty(cout, device=dev), torch.empty(cout, device=dev)
    y = torch.empty(B, T, cout, device=dev, dtype=torch.bfloat16)
    out16, out8 = torch.empty_like(y), torch.empty_like(y)
    wq, ws = capi.quantize_mx(w.view(K * cout, cin))
    xq, xs = capi.quantize_mx(x.view(B * T, cin))

    def finalize():
      capi.bn_finalize(None, B * T, gamma, beta, 1e-3, 0.9, False, mean, var, None, None, sc, sh)

    def bf16():
      capi.conv1d_fwd(x, w, dil=dil, in_len=lens, out=y)
      finalize()
      capi.bn_act_fwd([y], [sc], [sh], out16, lens, 1, 1.0, 0)

    def quant():
      capi.quantize_mx(x.view(B * T, cin), xq, xs)

    def mx():
      quant()
      finalize()
      capi.conv1d_fwd_mx(xq.view(B, T, cin), xs, wq, ws, k=K, dil=dil, in_len=lens, out_len=lens, ch_scale=sc,
                         ch_shift=sh, act=1, out=out8)
    fns = {"bf16": bf16, "mx": mx, "quant": quant}
    fl = 2.0 * B * T * cin * cout * K
    n = max(8, int(1e14 / fl))                       # 1e14 FLOP per window: 0.1 - 0.3 s at the rates seen
    for f in fns.values():
      for _ in range(3):
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(args.windows):                    # alternate the chains
      for k, f in fns.items():
        t[k].append(window(f, n))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
    ratio = med["mx"] / med["bf16"]
    wins = ratio < 1.0 - max(spread["bf16"], spread["mx"])
    rel = float((out8.float() - out16.float()).norm() / out16.float().norm())
    lines.append("| %d | %d | %d | %d | %.3f (%.0f) | %.3f (%.0f) | %.3f | %.2f | %.1f %% / %.1f %% | %s | %.2e |" % (
        cin, cout, K, dil, med["bf16"], fl / med["bf16"] / 1e9, med["mx"], fl / med["mx"] / 1e9, med["quant"], ratio,
        100 * spread["bf16"], 100 * spread["mx"], "yes" if wins else "no", rel))
    print(lines[-1], flush=True)
    del x, w, y, out16, out8, xq, wq
  text = "\n".join(lines) + "\n"
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text)


if __name__ == "__main__":
  main()
