#!/usr/bin/env python
"""Times the train step of example_configs/lm/lstm_lm_synthetic.py (not part of the bench.py contract):
  python tools/bench_lm.py [--steps 20] [--warmup 5] [--batch 160] [--bptt 96]
With --vocab / --num_sampled (and --layers / --units / --emb) the same model is built at other sizes over a Zipf
corpus of that vocabulary written to the temp dir; the shapes of the reference's lm/lstm-wkt103-mixed.py, trained
with the sampled softmax, are
  python tools/bench_lm.py --vocab 267735 --num_sampled 8192 --batch 224 --units 1024 --emb 320
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


def _sized_config(a):
  """A config file like example_configs/lm/lstm_lm_synthetic.py at the sizes asked for; the corpus has vocab - 2
  words (the dictionary adds '<unk>' and '<eos>')."""
  import tempfile
  from openseq2seq_amd.data.lm.synthetic import write_zipf_corpus
  vocab = a.vocab if a.vocab is not None else 33002
  root = os.path.join(tempfile.gettempdir(), "os2s_lm_bench_%d_v%d" % (os.getuid(), vocab))
  if not os.path.exists(os.path.join(root, "raw", "test.txt")):
    write_zipf_corpus(os.path.join(root, "raw"), vocab=vocab - 2, train_tokens=max(1200000, 4 * vocab))
  path = os.path.join(root, "config.py")
  with open(path, "w") as f:
    f.write("from open_seq2seq.configs.lstm_lm import lstm_lm_config\n"
            "base_model, base_params, train_params, eval_params, infer_params = lstm_lm_config(\n"
            "    %r, %r, layers=%d, num_units=%d, emb_size=%d, seed_tokens='w0 w1 w2', num_sampled=%r)\n"
            % (os.path.join(root, "raw"), os.path.join(root, "processed"), a.layers, a.units, a.emb, a.num_sampled))
  return path


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--batch", type=int, default=160)
  ap.add_argument("--bptt", type=int, default=96)
  ap.add_argument("--vocab", type=int, default=None, help="vocabulary size (writes a corpus of that many words)")
  ap.add_argument("--num_sampled", type=int, default=None, help="train with the sampled softmax")
  ap.add_argument("--layers", type=int, default=3)
  ap.add_argument("--units", type=int, default=896)
  ap.add_argument("--emb", type=int, default=256)
  a = ap.parse_args()
  import torch
  from openseq2seq_amd.utils.utils import create_model, get_base_config
  cfg = os.path.join(REPO, "example_configs", "lm", "lstm_lm_synthetic.py")
  name = "lstm_lm_synthetic"
  if a.vocab is not None or a.num_sampled is not None or (a.layers, a.units, a.emb) != (3, 896, 256):
    cfg, name = _sized_config(a), "lstm_lm_sized"
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
  if a.vocab is not None:
    assert model.get_data_layer().vocab_size == a.vocab, model.get_data_layer().vocab_size
  layers = len(model.get_encoder().layers)
  launches = layers * (2 * a.bptt + 1 + 2 * a.bptt - 1 + 1)
  med = statistics.median(times)
  print(json.dumps({"config": name, "vocab": model.get_data_layer().vocab_size, "num_sampled": a.num_sampled,
                    "layers": layers, "units": a.units, "emb": a.emb, "batch": a.batch, "bptt": a.bptt, "steps": a.steps,
                    "step_ms_median": round(med * 1e3, 2), "step_ms_mean": round(statistics.mean(times) * 1e3, 2),
                    "step_ms_min": round(min(times) * 1e3, 2), "tokens_per_s": round(a.batch * a.bptt / med, 1),
                    "recurrence_launches_per_step": launches, "loss": float(loss.cpu()[0])}))


if __name__ == "__main__":
  main()
