"""os2s_summary_stats against the fp64 NumPy oracle of tests/_summary_cases.py: one flat buffer with tensors on both
sides of every chunk boundary, a 64-chunk constant tensor (every value in one bucket: the contention case), a tensor
with a logical count below its size and values on both sides of every bucket limit.

Required: bucket counts, num, nonfinite, min and max exact; |sum - ref| <= n * 2^-52 * sum|v| and the same for
sum_squares with sum v^2 (what fixed-order double accumulation of n terms allows); two runs bit-identical."""
import numpy as np
import pytest
import torch

import _summary_cases as cases
from openseq2seq_amd.utils.summary import NUM_BUCKETS

pytestmark = pytest.mark.gpu

FIELDS = ("min", "max", "num", "sum", "sum_squares", "nonfinite")
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def layout(cuda):
  from openseq2seq_amd import capi
  chunk = capi.opt_chunk_elems()
  edge = cases.edge_values()
  rng = np.random.RandomState(7)
  sizes = [1, 7, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 64 * chunk, 2 * chunk + 9, edge.size]
  counts = list(sizes)
  counts[7] = chunk + 3                     # logical count below the size: the tail is real memory, never counted
  tensors = []
  for i, n in enumerate(sizes):
    if i == 6:
      x = np.full(n, 0.05 * 3 * 1024, np.float32)        # the contention case: one bucket
    elif i == 8:
      x = edge
    else:
      x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3)).astype(np.float32)
      x[rng.randint(0, n, max(1, n // 50))] = edge[rng.randint(0, edge.size, max(1, n // 50))]
    tensors.append(x)
  begins, off = [], 0
  for n in sizes:
    begins.append(off // chunk)
    off += -(-n // chunk) * chunk
  begins.append(off // chunk)
  flat = np.full(off, np.float32(777.0), np.float32)   # padding that would show in every statistic if it were read
  chunk_tensor = np.zeros(off // chunk, np.int32)
  for i, x in enumerate(tensors):
    flat[begins[i] * chunk:begins[i] * chunk + x.size] = x
    chunk_tensor[begins[i]:begins[i + 1]] = i
  m = cases.multiplier()
  ref = {mask: [cases.oracle(x, c, m, mask) for x, c in zip(tensors, counts)] for mask in (False, True)}
  dev = dict(flat=torch.from_numpy(flat).to(cuda), chunk_tensor=torch.from_numpy(chunk_tensor).to(cuda),
             begins=torch.tensor(begins, dtype=torch.int32, device=cuda),
             counts=torch.tensor(counts, dtype=torch.int64, device=cuda),
             dev_mult=torch.tensor([cases.DEV_MULT], dtype=torch.float32, device=cuda))
  return dict(dev=dev, counts=counts, ref=ref, nt=len(sizes), device=cuda)


def _run(layout, mask, select=None, hist=True, combine_lanes=False):
  from openseq2seq_amd import capi
  d, nt, dev = layout["dev"], layout["nt"], layout["device"]
  sel = torch.ones(nt, dtype=torch.uint8, device=dev)
  if select is not None:
    sel[:] = torch.tensor(select, dtype=torch.uint8)
  stats = torch.full((nt, 6), SENTINEL, dtype=torch.float64, device=dev)
  counts = torch.full((nt, NUM_BUCKETS), 99, dtype=torch.int32, device=dev).view(torch.uint32) if hist else None
  capi.summary_stats(d["flat"], d["chunk_tensor"], d["begins"], d["counts"], sel, stats, counts,
                     host_mult=cases.HOST_MULT, dev_mult=d["dev_mult"], mask_nonfinite=mask,
                     combine_lanes=combine_lanes, max_count=max(layout["counts"]))
  torch.cuda.synchronize()
  return stats.cpu().numpy(), (counts.view(torch.int32).cpu().numpy().view(np.uint32) if hist else None)


def _check(layout, mask, stats, counts, tensors):
  for t in tensors:
    ref, ref_counts = layout["ref"][mask][t]
    got = dict(zip(FIELDS, stats[t]))
    n = ref["num"]
    print("tensor %d mask %d: num %d nonfinite %d sum err %.3e (bound %.3e) sumsq err %.3e (bound %.3e)"
          % (t, mask, n, ref["nonfinite"], abs(got["sum"] - ref["sum"]), n * 2.0 ** -52 * ref["abs_sum"],
             abs(got["sum_squares"] - ref["sum_squares"]), n * 2.0 ** -52 * ref["sum_squares"]))
    for k in ("min", "max", "num", "nonfinite"):
      assert got[k] == ref[k], (t, k, got[k], ref[k])
    assert abs(got["sum"] - ref["sum"]) <= n * 2.0 ** -52 * ref["abs_sum"], t
    assert abs(got["sum_squares"] - ref["sum_squares"]) <= n * 2.0 ** -52 * ref["sum_squares"], t
    if counts is not None:
      bad = np.nonzero(counts[t] != ref_counts)[0]
      assert bad.size == 0, (t, bad[:8], counts[t][bad[:8]], ref_counts[bad[:8]])
      assert int(counts[t].sum()) == int(n)


@pytest.mark.parametrize("mask", [False, True])
def test_against_oracle(layout, mask):
  stats, counts = _run(layout, mask)
  _check(layout, mask, stats, counts, range(layout["nt"]))
  if not mask:
    assert stats[8][5] == 4.0               # NaN, -NaN, +Inf, -Inf of the edge values
  again_stats, again_counts = _run(layout, mask)
  assert stats.tobytes() == again_stats.tobytes() and counts.tobytes() == again_counts.tobytes()


def test_deselected_tensor_is_left_untouched(layout):
  select = [1] * layout["nt"]
  select[5] = 0
  stats, counts = _run(layout, False, select)
  assert np.all(stats[5] == SENTINEL) and np.all(counts[5] == 99)
  _check(layout, False, stats, counts, [t for t in range(layout["nt"]) if t != 5])


def test_without_histogram_and_combined_lanes_mode(layout):
  stats, _ = _run(layout, False, hist=False)
  _check(layout, False, stats, None, range(layout["nt"]))
  full, counts = _run(layout, False)
  assert stats.tobytes() == full.tobytes()          # the sums do not depend on whether buckets are counted
  stats1, counts1 = _run(layout, False, combine_lanes=True)
  assert stats1.tobytes() == full.tobytes() and counts1.tobytes() == counts.tobytes()


def test_empty_tensor_and_size_limit(layout):
  from openseq2seq_amd import capi, _lib
  d, nt, dev = layout["dev"], layout["nt"], layout["device"]
  zero = torch.zeros(nt, dtype=torch.int64, device=dev)
  sel = torch.ones(nt, dtype=torch.uint8, device=dev)
  stats = torch.zeros((nt, 6), dtype=torch.float64, device=dev)
  hist = torch.zeros((nt, NUM_BUCKETS), dtype=torch.int32, device=dev).view(torch.uint32)
  capi.summary_stats(d["flat"], d["chunk_tensor"], d["begins"], zero, sel, stats, hist, max_count=0)
  s = stats.cpu().numpy()
  dbl_max = np.finfo(np.float64).max
  assert np.all(s[:, 0] == dbl_max) and np.all(s[:, 1] == -dbl_max) and np.all(s[:, 2:] == 0.0)
  assert int(hist.view(torch.int32).abs().sum()) == 0
  with pytest.raises(_lib.Os2sError, match="invalid argument"):      # 32-bit bucket counts
    capi.summary_stats(d["flat"], d["chunk_tensor"], d["begins"], zero, sel, stats, hist, max_count=1 << 32)
  capi.summary_stats(d["flat"], d["chunk_tensor"], d["begins"], zero, sel, stats, None, max_count=1 << 32)
  torch.cuda.synchronize()
