#!/usr/bin/env python
"""Times the Griffin-Lim vocoder (os2s_griffin_lim) at the infer mode's batch shape: B = 32 utterances of 500
frames, n_fft 800 (M-AILABS), 50 iterations, with device events; next to it the NumPy restatement of the
reference's librosa loop (np.fft, float32 in / complex64 out like librosa) on ONE utterance on the host.
Writes profiles/griffin_lim_bench.json.

FLOP count: per iteration one analysis and one synthesis product of 2 * T * n_fft * 2K each (K = n_fft/2 + 1
bins, re and im), plus the first synthesis: B * T * (2 * n_iters + 1) * 2 * n_fft * 2K."""
from __future__ import print_function

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def numpy_griffin_lim(mag, phase, n_iters, n_fft):
  """The reference loop (models/text2speech.py:182-198) with np.fft in librosa's precision; mag [K, T]."""
  hop = n_fft // 4
  win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)).astype(np.float32)
  T = mag.shape[1]
  wss = np.zeros(n_fft + hop * (T - 1), np.float32)
  for t in range(T):
    wss[t * hop:t * hop + n_fft] += win ** 2

  def istft(Y):
    fr = np.fft.irfft(Y.T, n=n_fft, axis=1).astype(np.float32) * win
    y = np.zeros(n_fft + hop * (T - 1), np.float32)
    for t in range(T):
      y[t * hop:t * hop + n_fft] += fr[t]
    y /= np.maximum(wss, 1e-30)
    return y[n_fft // 2:-(n_fft // 2)]

  def stft(x):
    xp = np.pad(x, n_fft // 2, mode="reflect")
    idx = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]
    return np.fft.rfft(xp[idx] * win, axis=1).astype(np.complex64).T

  x = istft((mag * np.exp(2j * np.pi * phase)).astype(np.complex64))
  for _ in range(n_iters):
    X = stft(x)
    a = np.abs(X)
    P = np.where(a > 0, X / np.maximum(a, 1e-30), 1.0 + 0j)
    x = istft((mag * P).astype(np.complex64))
  return x


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--frames", type=int, default=500)
  ap.add_argument("--n_fft", type=int, default=800)
  ap.add_argument("--iters", type=int, default=50)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(REPO, "profiles", "griffin_lim_bench.json"))
  args = ap.parse_args()
  from openseq2seq_amd.models.text2speech import griffin_lim_batch
  dev = torch.device("cuda:0")
  B, T, n_fft, K = args.batch, args.frames, args.n_fft, args.n_fft // 2 + 1
  rng = np.random.RandomState(0)
  mags = np.abs(rng.randn(B, T, K)).astype(np.float32) * np.exp(-np.arange(K) / 80.0).astype(np.float32)
  phase = rng.rand(B, T, K).astype(np.float32)
  mags_d, phase_d = torch.from_numpy(mags).to(dev), torch.from_numpy(phase).to(dev)
  lens = [T] * B
  griffin_lim_batch(mags_d, lens, 2, n_fft, phase=phase_d)       # tables, code objects
  torch.cuda.synchronize()
  times = []
  for _ in range(args.reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sig, flags = griffin_lim_batch(mags_d, lens, args.iters, n_fft, phase=phase_d)
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1))
  ms = float(np.median(times))
  flop = float(B) * T * (2 * args.iters + 1) * 2.0 * n_fft * 2 * K
  t0 = time.perf_counter()
  numpy_griffin_lim(mags[0].T, phase[0].T, args.iters, n_fft)
  cpu_s = time.perf_counter() - t0
  res = {"what": "griffin_lim", "batch": B, "frames": T, "n_fft": n_fft, "iters": args.iters,
         "gpu_ms_per_batch_median": round(ms, 3), "gpu_ms_all": [round(t, 3) for t in times],
         "gpu_ms_per_utterance": round(ms / B, 4), "tflops_fp32": round(flop / (ms * 1e-3) / 1e12, 2),
         "numpy_one_utterance_s": round(cpu_s, 3), "numpy_batch_estimate_s": round(cpu_s * B, 2),
         "flags_set": int(flags.sum().item()),
         "device": torch.cuda.get_device_name(0)}
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
  print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
  main()
