#!/usr/bin/env python
"""Times the train step of example_configs/lm/lstm_lm_synthetic.py (not part of the bench.py contract):
  python tools/bench_lm.py [--steps 20] [--warmup 5] [--batch 160] [--bptt 96]
Prints one JSON line: median and mean step time over the timed steps (each step synchronised), tokens per second,
and the recurrence's launch count per step (two launches per layer and time step forward, two backward less the
last step's product, plus the init / parameter-sum launches)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--batch", type=int, default=160)
  ap.add_argument("--bptt", type=int, default=96)
  a = ap.parse_args()
  import torch
  from openseq2seq_amd.utils.utils import create_model, get_base_config
  cfg = os.path.join(REPO, "example_configs", "lm", "lstm_lm_synthetic.py")
  args, base, model_cls, module = get_base_config(["--config_file=" + cfg, "--mode=train", "--benchmark",
                                                   "--batch_size_per_gpu=%d" % a.batch])
  module["train_params"]["data_layer_params"]["bptt"] = a.bptt
  model = create_model(args, base, module, model_cls, None)
  batches = model.get_data_layer().iterate_batches(model._device, seed=1)
  times = []
  for step in range(a.warmup + a.steps):
    batch = next(batches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = model.train_step(batch)
    torch.cuda.synchronize()
    if step >= a.warmup:
      times.append(time.perf_counter() - t0)
  layers = len(model.get_encoder().layers)
  launches = layers * (2 * a.bptt + 1 + 2 * a.bptt - 1 + 1)
  med = statistics.median(times)
  print(json.dumps({"config": "lstm_lm_synthetic", "batch": a.batch, "bptt": a.bptt, "steps": a.steps,
                    "step_ms_median": round(med * 1e3, 2), "step_ms_mean": round(statistics.mean(times) * 1e3, 2),
                    "step_ms_min": round(min(times) * 1e3, 2), "tokens_per_s": round(a.batch * a.bptt / med, 1),
                    "recurrence_launches_per_step": launches, "loss": float(loss.cpu()[0])}))


if __name__ == "__main__":
  main()
