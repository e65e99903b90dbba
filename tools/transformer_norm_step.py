"""Transformer-big train step (configs/transformer.py, the bench.py workload: 256 pairs, synthetic batch) per
norm_params type, and the kernel time of each normalisation family from a rocprofv3 kernel-trace summary.

    python tools/transformer_norm_step.py --norm l2 l1 bn [--steps 30 --warmup 10]
        one JSON line per norm type: ms per step (the types interleaved over --rounds, one model each)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o a -- \\
        python tools/transformer_norm_step.py --norm bn --steps 5 --warmup 3
    python tools/transformer_norm_step.py --summarize DIR [--steps 5]
        total kernel time per step of each norm family in DIR's kernel_stats.csv
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NORMS = {
    "l2": None,                                  # the default path (no norm_params)
    "l1": {"type": "layernorm_L1", "epsilon": 1e-6},
    "bn": {"type": "batch_norm", "momentum": 0.95, "epsilon": 1e-5, "center_scale": False},   # transformer-bn.py
}

# kernel-name fragments of each family (the parameter-gradient reductions included)
FAMILIES = {
    # csrc/layernorm.hip: template <bool kL1, ...>, the kind is the first argument of the demangled name
    "layernorm_L2": ("layernorm_fwd_kernel<false", "layernorm_bwd_kernel<false", "layernorm_any_fwd_kernel<false",
                     "layernorm_any_bwd_kernel<false"),
    "layernorm_L1": ("layernorm_fwd_kernel<true", "layernorm_bwd_kernel<true", "layernorm_any_fwd_kernel<true",
                     "layernorm_any_bwd_kernel<true"),
    "batch_norm": ("bn_stats_kernel", "bn_finalize_kernel", "token_bn_apply_kernel", "token_bn_bwd_reduce_kernel",
                   "token_bn_bwd_apply_kernel"),
    "bn_bwd_finalize (all families' parameter gradients)": ("bn_bwd_finalize_kernel",),
}


def build(kind, dev):
  from openseq2seq_amd.configs.transformer import transformer_config
  model_cls, params = transformer_config(batch_size_per_gpu=256)
  if NORMS[kind] is not None:
    params["encoder_params"]["norm_params"] = dict(NORMS[kind])
    params["decoder_params"]["norm_params"] = dict(NORMS[kind])
  model = model_cls(params, mode="train", device=dev)
  model.compile()
  return model, model.get_data_layer().synthetic_batch(dev, seed=1234)


def timed(model, batch, steps, warmup):
  import torch
  for _ in range(warmup):
    model.train_step(batch)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(steps):
    loss = model.train_step(batch)
  torch.cuda.synchronize()
  return 1000.0 * (time.perf_counter() - t0) / steps, float(loss.float().mean().cpu()) if hasattr(loss, "float") else loss


def summarize(d, steps):
  f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))[0]
  rows = list(csv.DictReader(open(f)))
  out = {}
  for fam, keys in FAMILIES.items():
    sel = [r for r in rows if any(k in r["Name"] for k in keys)]
    out[fam] = {"us_per_step": sum(float(r["TotalDurationNs"]) for r in sel) / 1e3 / steps,
                "launches_per_step": sum(int(r["Calls"]) for r in sel) / steps,
                "kernels": sorted({r["Name"].split("(")[0] for r in sel})}
  out["all_kernels_us_per_step"] = sum(float(r["TotalDurationNs"]) for r in rows) / 1e3 / steps
  print(json.dumps(out))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--norm", nargs="*", default=["l2", "l1", "bn"], choices=sorted(NORMS))
  ap.add_argument("--steps", type=int, default=30)
  ap.add_argument("--warmup", type=int, default=10)
  ap.add_argument("--rounds", type=int, default=1)
  ap.add_argument("--summarize", default=None)
  a = ap.parse_args()
  if a.summarize:
    summarize(a.summarize, a.steps)
    return
  import torch
  dev = torch.device("cuda:0")
  models = {k: build(k, dev) for k in a.norm}
  res = {k: [] for k in a.norm}
  for _ in range(a.rounds):
    for k in a.norm:
      ms, loss = timed(models[k][0], models[k][1], a.steps, a.warmup)
      res[k].append(ms)
      assert loss == loss, (k, loss)
  for k in a.norm:
    print(json.dumps({"norm": k, "norm_params": NORMS[k], "ms_per_step": res[k], "steps": a.steps,
                      "warmup": a.warmup, "workload": "Transformer-big train step, 256 pairs, synthetic batch"}))


if __name__ == "__main__":
  main()
