"""bf16 os2s_gemm_nt against the MXFP8 path (os2s_mx_quantize_rows of the activation + os2s_gemm_nt_mx on a weight
copy quantised once) at the Transformer-big Dense shapes of an eval pass: M = 16 384 tokens, K and N in
{1024, 4096}, and the logits matmul onto the 32 768-row embedding table.

Call times from device events around windows of back-to-back launches, every shape warmed up, the two paths
alternated inside one process and the best of several windows kept next to the spread; FLOP/s = 2 M N K over that
time (a call time, not a kernel's share of peak). Prints a markdown table; --out writes it to a file as well.

  python tools/bench_gemm_mx.py [--out mxfp8.md] [--windows 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from openseq2seq_amd import capi  # noqa: E402

SHAPES = [(16384, 1024, 1024), (16384, 4096, 1024), (16384, 1024, 4096), (16384, 4096, 4096),
          (16384, 32768, 1024)]       # (M, N, K); the last one is the logits matmul


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
  ap.add_argument("--windows", type=int, default=5)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_gemm_mx.py measures on the GPU; none found")
  dev = torch.device("cuda:0")
  lines = ["| M | N | K | bf16 gemm_nt ms (TF/s) | quantise a ms | gemm_nt_mx ms (TF/s) | quantise + mx ms | mx path / bf16 "
           "| spread bf16 / mx | rel L2 bf16, mx vs fp32 |", "|---|---|---|---|---|---|---|---|---|---|"]
  for M, N, K in SHAPES:
    torch.manual_seed(M + N + K)
    a = torch.randn(M, K, device=dev).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device=dev)
    y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    wq, ws = capi.quantize_mx(w)
    aq, asc = capi.quantize_mx(a)
    fns = {"bf16": lambda: capi.gemm_nt(a, w, out=y, bias=bias),
           "quant": lambda: capi.quantize_mx(a, aq, asc),
           "mx": lambda: capi.gemm_nt_mx(aq, asc, wq, ws, out=y, bias=bias),
           "path": lambda: capi.gemm_nt_mx(*capi.quantize_mx(a, aq, asc), wq, ws, out=y, bias=bias)}
    n = max(8, int(2e14 / (2.0 * M * N * K)))            # 2e14 FLOP per window: 0.1 - 0.2 s at the rates seen
    for f in fns.values():
      for _ in range(3):
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(args.windows):                        # alternate the paths
      for k, f in fns.items():
        t[k].append(window(f, n))
    best = {k: min(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / min(v) for k, v in t.items()}
    # accuracy on a slice (fp32 reference of the bf16 operands)
    ref = a[:512].float() @ w[:2048].float().t() + bias[:2048]
    capi.gemm_nt(a, w, out=y, bias=bias)
    e16 = float((y[:512, :2048].float() - ref).norm() / ref.norm())
    fns["path"]()
    e8 = float((y[:512, :2048].float() - ref).norm() / ref.norm())
    fl = 2.0 * M * N * K
    lines.append("| %d | %d | %d | %.3f (%.0f) | %.3f | %.3f (%.0f) | %.3f | %.2f | %.1f %% / %.1f %% | %.2e, %.2e |" % (
        M, N, K, best["bf16"], fl / best["bf16"] / 1e9, best["quant"], best["mx"], fl / best["mx"] / 1e9, best["path"],
        best["path"] / best["bf16"], 100 * spread["bf16"], 100 * spread["path"], e16, e8))
    print(lines[-1], flush=True)
    del a, w, y, aq, wq
  text = "\n".join(lines) + "\n"
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text)


if __name__ == "__main__":
  main()
