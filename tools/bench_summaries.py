"""What a summary step costs: the Jasper 10x5 synthetic train step of bench.py's shapes (batch 32) with
save_summaries_steps = 1 (every summary kind of the reference's configs) and 0, and the statistics pass by itself
over the model's own flat buffers (variables + gradients, with histograms), in both bucket-counting modes, against
the bandwidth floor bytes / HBM rate.

  python tools/bench_summaries.py [--steps 20] [--warmup 5] [--batch 32] [--hbm-tbs 6.29] [--json out.json]

Prints one JSON line. Times are host clocks around work that ends in a device synchronise (steps) and device events
(the pass)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SUMMARIES = ["learning_rate", "variables", "gradients", "variable_norm", "gradient_norm", "global_gradient_norm",
             "larc_summaries", "loss_scale"]


def build(batch, logdir, every, dev):
  from openseq2seq_amd.configs.jasper import jasper10x5_config
  cls, params = jasper10x5_config(batch_size_per_gpu=batch, use_horovod=False, max_steps=100000)
  params["summaries"] = SUMMARIES
  if every:
    params["logdir"], params["save_summaries_steps"] = logdir, every
  m = cls(params, mode="train", hvd=None, device=dev)
  m.compile()
  return m


def time_steps(m, batch, steps, warmup, with_step):
  for i in range(warmup):
    m.train_step(batch, i if with_step else None)
  torch.cuda.synchronize()
  times = []
  for i in range(steps):
    t0 = time.perf_counter()
    m.train_step(batch, warmup + i if with_step else None)
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) * 1e3)
  times.sort()
  return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1]}


def time_pass(m, reps, hist, mode):
  from openseq2seq_amd import capi
  from openseq2seq_amd.optimizers.summaries import logical_count
  s, dev = m.store, m.store.device
  nt = len(s.params)
  counts = [logical_count(p) for p in s.params]
  cd = torch.tensor(counts, dtype=torch.int64, device=dev)
  sel = torch.ones(nt, dtype=torch.uint8, device=dev)
  stats = torch.zeros((nt, 6), dtype=torch.float64, device=dev)
  h = torch.zeros((nt, capi.summary_num_buckets()), dtype=torch.int32, device=dev).view(torch.uint32) if hist else None
  ws = capi.summary_stats_workspace(s.chunk_tensor.numel(), dev)
  out = {}
  # (a constant buffer: every value in one bucket, the worst case for the LDS atomics)
  for name, buf in (("variables", s._master), ("gradients", s._grads), ("constant", torch.full_like(s._master, 0.05))):
    best = None
    for _ in range(reps + 1):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      capi.summary_stats(buf, s.chunk_tensor, s.tensor_chunk_begin, cd, sel, stats, h, workspace=ws,
                         max_count=max(counts), combine_lanes=bool(mode))
      e1.record()
      torch.cuda.synchronize()
      t = e0.elapsed_time(e1)
      best = t if best is None else min(best, t)
    out[name + "_ms"] = best
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--hbm-tbs", type=float, default=6.29, help="measured HBM rate of a float4 copy, TB/s")
  ap.add_argument("--json", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_summaries.py needs a GPU")
  dev = torch.device("cuda:0")
  torch.cuda.set_device(dev)
  logdir = tempfile.mkdtemp(prefix="os2s_summaries_")
  res = {"batch": args.batch, "steps": args.steps}
  try:
    off = build(args.batch, None, 0, dev)
    batch = off.get_data_layer().synthetic_batch(dev, seed=1234)
    res["step_summaries_off"] = time_steps(off, batch, args.steps, args.warmup, False)
    flat_bytes = off.store.total * 4
    res["flat_buffer_bytes"] = flat_bytes
    res["floor_ms_two_buffers"] = 2 * flat_bytes / (args.hbm_tbs * 1e12) * 1e3
    for hist, mode, key in ((True, 0, "pass_hist_per_lane"), (True, 1, "pass_hist_combined"), (False, 0, "pass_no_hist")):
      r = time_pass(off, 5, hist, mode)
      r["total_ms"] = r["variables_ms"] + r["gradients_ms"]
      r["ratio_to_floor"] = r["total_ms"] / res["floor_ms_two_buffers"]
      res[key] = r
    del off
    torch.cuda.empty_cache()
    on = build(args.batch, logdir, 1, dev)
    assert on.open_summaries() is not None
    res["step_summaries_every_step"] = time_steps(on, batch, args.steps, args.warmup, True)
    on.close_summaries()
    res["event_file_bytes"] = sum(os.path.getsize(os.path.join(logdir, f)) for f in os.listdir(logdir))
  finally:
    shutil.rmtree(logdir, ignore_errors=True)
  line = json.dumps(res)
  print(line)
  if args.json:
    with open(args.json, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
