#!/usr/bin/env python
"""Times the text-classification train step at the shapes of the reference's transfer configs on synthetic ragged
batches (not part of the bench.py contract):
  python tools/bench_textcls.py [--config sst|imdb] [--steps 20] [--warmup 5]
sst: sst-wkt2.py (B = 20, reviews of 5 .. 96 tokens); imdb: imdb-wkt2.py (B = 16, 20 .. 256 tokens); both 3 layers
of 896 / 896 / 256 units over a 33 278-word vocabulary, classifier on [h, c], the configs' dropout, Adam.
Prints one JSON line:
  step_ms_*          the whole train step, each step synchronised (host clock around the step)
  launches           kernel launches of the recurrence per step, from the shapes (per layer: init + 2 T forward,
                     2 T - 1 + parameter sum backward) and of the head (3)
  recurrence_ms      the recurrence entries alone (forward + state-gradient backward of the three layers at the
                     step's T), device events, median of --reps calls
  head_us            the head's three launches (forward, loss, backward), device events over --reps calls each
A processed corpus and a vocabulary file are generated into a temporary directory from a seed."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"sst": (5, 96), "imdb": (20, 256)}
VOCAB = 33278


def write_corpus(root, lo, hi, n=640):
  proc = os.path.join(root, "proc")
  os.makedirs(proc, exist_ok=True)
  rng = random.Random(5)
  vocab = os.path.join(root, "vocab.txt")
  with open(vocab, "w") as f:
    for i, w in enumerate(["<unk>", "<eos>"] + ["w%d" % k for k in range(VOCAB - 2)]):
      f.write("%d\t%s\t%d\n" % (i, w, VOCAB - i))
    f.write("%d\n" % VOCAB)
  for split in ("train", "valid", "test"):
    with open(os.path.join(proc, split + ".ids"), "w") as ids, open(os.path.join(proc, split + ".rat"), "w") as rat:
      for _ in range(n):
        ids.write("\t".join(str(rng.randrange(2, VOCAB)) for _ in range(rng.randint(lo, hi))) + "\n")
        rat.write("%d\n" % rng.randrange(2))
  return proc, vocab


def event_time(fn, reps):
  """Median milliseconds of fn() by device events, after three warm-up calls."""
  import torch
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  out = []
  for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    out.append(a.elapsed_time(b))
  return statistics.median(out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--config", choices=sorted(SHAPES), default="sst")
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--reps", type=int, default=20)
  a = ap.parse_args()
  import torch
  from openseq2seq_amd import capi
  from openseq2seq_amd.configs.text_cls import text_cls_config
  from openseq2seq_amd.models.lstm_lm import LSTMLM
  lo, hi = SHAPES[a.config]
  root = tempfile.mkdtemp(prefix="os2s_textcls_bench_")
  proc, vocab = write_corpus(root, lo, hi)
  _, base, train, _, _ = text_cls_config(a.config, proc, vocab, max_steps=a.warmup + a.steps)
  base.update(train)
  model = LSTMLM(params=base, mode="train", hvd=None)
  model.compile()
  batches = model.get_data_layer().iterate_batches(model._device, seed=1)
  times, ts = [], []
  for step in range(a.warmup + a.steps):
    batch = next(batches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = model.train_step(batch)
    torch.cuda.synchronize()
    if step >= a.warmup:
      times.append(time.perf_counter() - t0)
      ts.append(int(batch["source_tensors"][0].shape[1]))
  # ---- the pieces alone, at the last batch's shape
  enc = model.get_encoder()
  dev = model._device
  ids, lens = batch["source_tensors"]
  B, T = ids.shape
  lens = lens.to(torch.int32).contiguous()
  runs = []
  for layer in enc.layers:
    H = layer.H
    gx = torch.randn(B, T, 4 * H, device=dev).to(torch.bfloat16)
    ln = torch.stack([p.master for p in layer.ln])
    runs.append((layer, H, gx, ln, torch.randn(B, T, H, device=dev).to(torch.bfloat16)))
  top = len(runs) - 1
  state_grad = (torch.randn(B, enc.last, device=dev), torch.randn(B, enc.last, device=dev))

  def recurrence():
    for k, (layer, H, gx, ln, dy) in enumerate(runs):
      r = capi.lnlstm_layer_fwd(gx, layer.wh.w16.view(4 * H, H), ln, lens, H, layer.forget_bias, save=True,
                                want_state=k == top)
      dhT, dcT = state_grad if k == top else (None, None)
      capi.lnlstm_layer_bwd_state(layer.wh.wt16.view(H, 4 * H), ln, lens, None if k == top else dy, dhT, dcT,
                                  r["xhat"], r["s_hat"], r["rstd"], H, layer.forget_bias)

  C = enc._fc_dim
  hT, cT = torch.randn(B, enc.last, device=dev), torch.randn(B, enc.last, device=dev)
  w16 = enc.proj.w16.view(C, -1)
  y = torch.nn.functional.one_hot(torch.randint(0, C, (B,), device=dev), C).float()
  logits = capi.text_cls_fwd(hT, cT, w16, enc.bias.master)
  _, dl = capi.softmax_xent_dense(logits, y)
  dw, db = torch.zeros_like(enc.proj.grad.view(C, -1)), torch.zeros_like(enc.bias.grad)
  head = {"fwd": event_time(lambda: capi.text_cls_fwd(hT, cT, w16, enc.bias.master), a.reps) * 1e3,
          "loss": event_time(lambda: capi.softmax_xent_dense(logits, y), a.reps) * 1e3,
          "bwd": event_time(lambda: capi.text_cls_bwd(hT, cT, w16, dl, dw, db), a.reps) * 1e3}
  rec_ms = event_time(recurrence, a.reps)
  med = statistics.median(times)
  layers = len(enc.layers)
  print(json.dumps({"config": a.config, "batch": int(B), "T_timed_steps": [min(ts), max(ts)], "T_pieces": int(T),
                    "steps": a.steps, "step_ms_median": round(med * 1e3, 2),
                    "step_ms_mean": round(statistics.mean(times) * 1e3, 2), "step_ms_min": round(min(times) * 1e3, 2),
                    "launches": {"recurrence": layers * (1 + 2 * int(T) + 2 * int(T) - 1 + 1), "head": 3},
                    "recurrence_ms": round(rec_ms, 3), "head_us": {k: round(v, 1) for k, v in head.items()},
                    "head_share_of_pieces": round(sum(head.values()) * 1e-3 / (rec_ms + sum(head.values()) * 1e-3), 5),
                    "loss": float(loss.cpu()[0])}))


if __name__ == "__main__":
  main()
