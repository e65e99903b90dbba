"""Inputs and the fp64 NumPy oracle of the summary-statistics tests (tests/test_summary_stats_gpu.py).

Oracle of one tensor: v = fp32(x * m) with m = fp32(host_mult * dev_mult), widened to float64; bucket(v) =
np.searchsorted(limits, v, side="right"); sums with math.fsum (exactly rounded)."""
import math

import numpy as np

from openseq2seq_amd.utils.summary import DBL_MAX, NUM_BUCKETS, bucket_limits

HOST_MULT = 1.0 / 3.0
DEV_MULT = 1.0 / 1024.0


def multiplier(host_mult=HOST_MULT, dev_mult=DEV_MULT):
  return np.float32(host_mult) * np.float32(dev_mult)


def edge_values():
  """fp32 inputs x whose products x * m land on the fp32 neighbours on both sides of every finite non-zero limit,
  both signs (x = neighbour / m, and its own two neighbours: the fp32 rounding of x * m decides the bucket), plus
  +-0, denormals, +-FLT_MAX, magnitudes below 1e-12 and NaN / +-Inf."""
  lim = bucket_limits()
  pos = lim[776:-1]                       # 1e-12 .. the last finite limit
  m = np.float64(multiplier())
  with np.errstate(over="ignore"):
    below = np.nextafter(pos.astype(np.float32), np.float32(0))           # fp32 values around each limit
    above = np.nextafter(pos.astype(np.float32), np.float32(np.inf))
    around = np.concatenate([pos.astype(np.float32), below, above])
    x = (around.astype(np.float64) / m).astype(np.float32)                # overflows to inf for the top limits: kept
    x = np.concatenate([x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(np.inf)), around])
  x = np.concatenate([x, -x])
  fmax, tiny = np.finfo(np.float32).max, np.finfo(np.float32).tiny
  special = np.array([0.0, -0.0, 1e-45, -1e-45, tiny, -tiny, tiny / 4, -tiny / 4, fmax, -fmax, 1e-13, -1e-13,
                      3e-10, -3e-10, 1e-30, -1e-30, np.nan, -np.nan, np.inf, -np.inf, 1.0, -1.0, 0.05, -0.05],
                     np.float32)
  return np.concatenate([x, special]).astype(np.float32)


def oracle(x, count, m, mask_nonfinite):
  """(stats dict, counts uint32 [1551]) of the leading `count` elements of fp32 array x."""
  lim = bucket_limits()
  with np.errstate(over="ignore", invalid="ignore", under="ignore"):
    v32 = (x[:count].astype(np.float32) * np.float32(m)).astype(np.float32)
  v = v32.astype(np.float64)
  fin = np.isfinite(v)
  if mask_nonfinite:
    v = np.where(fin, v, 0.0)
    nonfinite = 0
  else:
    nonfinite = int((~fin).sum())
    v = v[fin]
  counts = np.bincount(np.searchsorted(lim, v, side="right"), minlength=NUM_BUCKETS).astype(np.uint32)
  assert counts.size == NUM_BUCKETS
  stats = {"min": float(v.min()) if v.size else DBL_MAX, "max": float(v.max()) if v.size else -DBL_MAX,
           "num": float(v.size), "sum": math.fsum(v), "sum_squares": math.fsum(v * v), "nonfinite": float(nonfinite),
           "abs_sum": math.fsum(np.abs(v))}
  return stats, counts
