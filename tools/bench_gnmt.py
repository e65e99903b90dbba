#!/usr/bin/env python
"""Times openseq2seq_amd.configs.nmt.gnmt_like_config (en-de-gnmt-like-4GPUs.py: 7-layer GNMT encoder, 8-layer
gnmt_v2 decoder, 1024 units, attention_layer_size 1024) on synthetic batches; not part of the bench.py contract:
  python tools/bench_gnmt.py [--steps 10] [--warmup 3] [--batch 32] [--max_length 50] [--beam 10]
                             [--decode_len 24] [--weight_tied] [--no_train] [--no_decode]
Prints one JSON line: median / mean / min train-step time (each step synchronised) and tokens per second; for the
beam search (infer mode, batch 1 as the config's infer section, one source sentence of --decode_len tokens, at
most 2 x that many steps) the time of one decode, the steps it ran and the ms per step."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--max_length", type=int, default=50)
  ap.add_argument("--vocab", type=int, default=32768)
  ap.add_argument("--beam", type=int, default=10)
  ap.add_argument("--decode_len", type=int, default=24)
  ap.add_argument("--decodes", type=int, default=3)
  ap.add_argument("--weight_tied", action="store_true")
  ap.add_argument("--no_train", action="store_true")
  ap.add_argument("--no_decode", action="store_true")
  a = ap.parse_args()
  import torch
  from openseq2seq_amd.configs.nmt import gnmt_like_config
  from openseq2seq_amd.decoders import BeamSearchRNNDecoderWithAttention
  dev = torch.device("cuda:0")
  out = {"config": "gnmt_like", "weight_tied": a.weight_tied, "batch": a.batch, "max_length": a.max_length}
  cls, params = gnmt_like_config(batch_size_per_gpu=a.batch, vocab=a.vocab, weight_tied=a.weight_tied,
                                 max_length=a.max_length)
  if not a.no_train:
    model = cls(copy.deepcopy(params), mode="train", hvd=None, device=dev)
    model.compile()
    # full-length sentences: the shape the limits are about (B x max_length x max_length attention)
    batch = model.get_data_layer().synthetic_batch(dev, seed=1, fixed_len=a.max_length)
    times, loss = [], None
    for step in range(a.warmup + a.steps):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      loss = model.train_step(batch)
      torch.cuda.synchronize()
      if step >= a.warmup:
        times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    out.update({"steps": a.steps, "step_ms_median": round(med * 1e3, 2),
                "step_ms_mean": round(statistics.mean(times) * 1e3, 2), "step_ms_min": round(min(times) * 1e3, 2),
                "tokens_per_s": round(batch["num_tokens"] / med, 1), "loss": float(loss.cpu()[0])})
    del model
    torch.cuda.empty_cache()
  if not a.no_decode:
    p2 = copy.deepcopy(params)
    p2["batch_size_per_gpu"] = 1
    p2["decoder"] = BeamSearchRNNDecoderWithAttention
    p2["decoder_params"] = dict(p2["decoder_params"], beam_width=a.beam, length_penalty=1.0)
    infer = cls(p2, mode="infer", hvd=None, device=dev)
    infer.compile()
    batch = infer.get_data_layer().synthetic_batch(dev, seed=2, fixed_len=a.decode_len)
    dtimes, nsteps = [], 0
    for i in range(1 + a.decodes):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      ids, lens = infer.infer_batch(batch)
      torch.cuda.synchronize()
      if i >= 1:
        dtimes.append(time.perf_counter() - t0)
      nsteps = int(ids.shape[1])
    dmed = statistics.median(dtimes)
    out.update({"beam": a.beam, "decode_src_len": a.decode_len, "decode_steps": nsteps,
                "decode_ms_median": round(dmed * 1e3, 2), "decode_ms_per_step": round(dmed * 1e3 / max(nsteps, 1), 3)})
  print(json.dumps(out))


if __name__ == "__main__":
  main()
