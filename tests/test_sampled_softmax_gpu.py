"""csrc/sampled_softmax.hip against tests/_sampled_softmax_cases.py.

Sampler: ids in draw order and num_tries equal the sequential Python loop exactly -- one bitmap word, repeats inside
one round of tries, many rounds, the largest bitmap, the try cap with its fill; log Q to fp32 rounding.
Loss and gradients (the product path parts/sampled_softmax.forward / backward: gather, GEMM, loss kernel, compact
GEMMs, scatter, true-row kernel) against the fp64 restatement R. The bound is relative, not a constant: the device's
max error against R may be at most twice the error R_b (R with the device's bf16 roundings) has against R, plus the
fp32 floor K 2^-24 max|R| of a K-term fp32 accumulation (K = the longest sum behind the tensor, + 8 for the fast
exp / log). Both errors are printed. Hit columns of dlogits are exactly 0, untouched table rows stay bit-zero, two
deterministic runs are bit-identical, and default (atomic) mode differs from deterministic mode by no more than
atomic-mode runs over permuted rows differ among themselves (measured: bias gradient 1.2e-07 against 1.2e-07, table
gradient 6.0e-08 against 1.2e-07; profiles/sampled_softmax_first_measurements.md)."""
import numpy as np
import pytest
import torch

import _sampled_softmax_cases as ssc

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24


# ---------------------------------------------------------------- sampler
def _seed_with_repeat_in_first_round(V, round_size=64):
  for seed in range(1, 100):
    k = ssc.draw_classes(V, seed, round_size)
    if len(set(k.tolist())) < round_size:
      return seed
  raise AssertionError("no seed with a repeated class in the first round")


@pytest.mark.parametrize("V,S,seed,cap", [(16, 8, 11, None), (200, 64, None, None), (40000, 1024, 13, None),
                                          (1 << 20, 4096, 14, None), (64, 32, 5, 40), (2, 1, 3, None)])
def test_sampler_equals_the_sequential_loop(cuda, V, S, seed, cap):
  from openseq2seq_amd import capi
  if seed is None:
    seed = _seed_with_repeat_in_first_round(V)
    k = ssc.draw_classes(V, seed, 64)
    assert len(set(k.tolist())) < 64          # one round of tries contains a repeated class
  ids, tries = ssc.sample(V, S, seed, cap)
  if cap is not None:
    assert tries == cap                       # the cap bites: the fill path
  got_ids, got_tries, got_lq = capi.sampled_softmax_candidates(V, S, seed, cap)
  assert got_tries == tries
  assert np.array_equal(got_ids, ids)
  lq = ssc.log_q(ids, tries, V)
  assert np.abs(got_lq - lq).max() <= 4 * EPS32 * max(1.0, np.abs(lq).max())


def test_sampler_padding_and_seeds(cuda):
  from openseq2seq_amd import capi
  V, S = 200, 61
  b = capi.sampled_softmax_bounds(V).cuda()
  ids, tries, lq = capi.sampled_softmax_sample(b, V, S, 21)
  assert ids.numel() == 64 and (ids[S:] == -1).all() and (lq[S:] == 0).all()
  ids2, tries2, lq2 = capi.sampled_softmax_sample(b, V, S, 21)
  assert torch.equal(ids, ids2) and torch.equal(tries, tries2) and torch.equal(lq, lq2)
  ids3, _, _ = capi.sampled_softmax_sample(b, V, S, 22)
  assert not torch.equal(ids, ids3)


def test_unsupported_sizes_raise_value_error(cuda):
  from openseq2seq_amd import capi
  for V, S in ((1, 1), (16, 9), (16, 0), ((1 << 20) + 8, 8)):
    with pytest.raises(ValueError):
      capi.sampled_softmax_candidates(V, S, 1)


# ---------------------------------------------------------------- loss and gradients
def _device_case(c, V):
  dev = torch.device("cuda")
  S = len(c["ids"])
  spad = -(-S // 8) * 8
  ids = torch.full((spad,), -1, dtype=torch.int32)
  ids[:S] = torch.from_numpy(c["ids"]).int()
  lq = torch.zeros(spad)
  lq[:S] = torch.from_numpy(ssc.log_q(c["ids"], c["tries"], V)).float()
  cand = (ids.to(dev), torch.tensor([c["tries"]], dtype=torch.int32, device=dev), lq.to(dev))
  return dict(x=torch.from_numpy(c["x"]).to(torch.bfloat16).to(dev), W=torch.from_numpy(c["W"]).to(torch.bfloat16).to(dev),
              b=torch.from_numpy(c["b"]).float().to(dev), labels=torch.from_numpy(c["labels"]).int().to(dev),
              cand=cand, S=S)


def _run(d, V, scale, scale_dev=None, perm=None):
  """One forward + backward of the product path; returns host copies."""
  from openseq2seq_amd.parts import sampled_softmax
  x, labels = d["x"], d["labels"]
  if perm is not None:
    x, labels = x[perm].contiguous(), labels[perm].contiguous()
  N, D = x.shape
  loss, st = sampled_softmax.forward(x, d["W"], d["b"], labels, d["cand"], d["S"], V, scale, scale_dev, True)
  dlogits = st.dlogits.float().cpu().double().numpy()[:, :d["S"]].copy()
  pad = st.dlogits.float().cpu().numpy()[:, d["S"]:]
  dx = torch.zeros((N, D), dtype=torch.bfloat16, device=x.device)
  dW = torch.zeros((V, D), dtype=torch.float32, device=x.device)
  db = torch.zeros(V, dtype=torch.float32, device=x.device)
  sampled_softmax.backward(st, dx, False, dW, db)
  torch.cuda.synchronize()
  dxh = dx.float().cpu()
  if perm is not None:
    inv = torch.empty_like(perm.cpu())
    inv[perm.cpu()] = torch.arange(N)
    dxh = dxh[inv]
  return dict(row_loss=st.row_loss.cpu().double().numpy(), loss=float(loss.cpu()[0]), dlogits=dlogits, pad=pad,
              dx=dxh.double().numpy(), dW=dW.cpu().double().numpy(), db=db.cpu().double().numpy(),
              dW32=dW.cpu(), db32=db.cpu(), dx16=dxh)


SHAPES = [(5, 8, 40, 16), (70, 320, 1000, 200), (33, 64, 3000, 1024)]


@pytest.mark.parametrize("with_scale_dev", [False, True])
@pytest.mark.parametrize("N,D,V,S", SHAPES)
def test_loss_and_gradients_against_the_fp64_restatement(cuda, N, D, V, S, with_scale_dev):
  c = ssc.make_case(N, D, V, S, seed=100 + N)
  assert ssc.count_hit_rows(c["labels"], c["ids"]) >= 3
  d = _device_case(c, V)
  scale = 1.0 / N
  ls = 64.0 if with_scale_dev else 1.0
  scale_dev = torch.tensor([ls], dtype=torch.float32, device="cuda") if with_scale_dev else None
  got = _run(d, V, scale, scale_dev)
  r = ssc.reference(c["x"], c["W"], c["b"], c["labels"], c["ids"], c["tries"], V, scale, gs=scale * ls)
  rb = ssc.reference(c["x"], c["W"], c["b"], c["labels"], c["ids"], c["tries"], V, scale, gs=scale * ls, rb=True)
  # the longest fp32 sum behind each tensor
  terms = dict(row_loss=D + S + 1, dx=S + 1, dW=N, db=N)
  for key in ("row_loss", "dx", "dW", "db"):
    e_dev = np.abs(got[key] - r[key]).max()
    e_rb = np.abs(rb[key] - r[key]).max()
    floor = (terms[key] + 8) * EPS32 * np.abs(r[key]).max()
    print("%s N=%d D=%d V=%d S=%d scale_dev=%s: device %.3e  R_b %.3e  floor %.3e"
          % (key, N, D, V, S, with_scale_dev, e_dev, e_rb, floor))
    assert e_dev <= 2.0 * e_rb + floor, (key, e_dev, e_rb, floor)
  # the loss is the fp64 sum of the device's row losses, rounded once to fp32
  row_bound = 2.0 * np.abs(rb["row_loss"] - r["row_loss"]).max() + (D + S + 9) * EPS32 * np.abs(r["row_loss"]).max()
  print("loss: device %.3e, bound %.3e" % (abs(got["loss"] - r["loss"]), scale * N * row_bound + 2 * EPS32 * abs(r["loss"])))
  assert abs(got["loss"] - r["loss"]) <= scale * N * row_bound + 2 * EPS32 * abs(r["loss"])
  assert r["hit"].sum() >= 3 and (got["dlogits"][r["hit"]] == 0.0).all()
  assert not got["pad"].any()                    # padding columns carry no gradient
  untouched = np.setdiff1d(np.arange(V), np.concatenate([c["ids"], c["labels"]]))
  assert len(untouched)
  assert not got["dW32"][untouched].view(torch.int32).any() and not got["db32"][untouched].view(torch.int32).any()


def test_forward_without_gradient_leaves_the_logits(cuda):
  from openseq2seq_amd.parts import sampled_softmax
  N, D, V, S = 5, 8, 40, 16
  c = ssc.make_case(N, D, V, S, seed=105)
  d = _device_case(c, V)
  loss, st = sampled_softmax.forward(d["x"], d["W"], d["b"], d["labels"], d["cand"], S, V, 1.0 / N, None, False)
  loss2, _ = sampled_softmax.forward(d["x"], d["W"], d["b"], d["labels"], d["cand"], S, V, 1.0 / N, None, True)
  assert st.dlogits is None and st.dtrue is None and torch.equal(loss, loss2)


def test_deterministic_mode_is_bit_identical_and_default_mode_is_within_reordering(cuda):
  from openseq2seq_amd import capi
  N, D, V, S = 70, 320, 1000, 200
  c = ssc.make_case(N, D, V, S, seed=170)
  c["labels"][10:40] = c["labels"][5]           # thirty rows add into one table row
  d = _device_case(c, V)
  prev = capi.deterministic()
  try:
    capi.set_deterministic(True)
    a, b = _run(d, V, 1.0 / N), _run(d, V, 1.0 / N)
    for key in ("dW32", "db32", "dx16"):
      assert torch.equal(a[key], b[key]), key
    capi.set_deterministic(False)
    g = torch.Generator().manual_seed(0)
    # the floor is a maximum over run pairs, the gap one more draw of the same quantity: 32 row orders give 528
    # pairs, enough for the maximum to reach what a reordering of these sums can do
    runs = [_run(d, V, 1.0 / N)] + [_run(d, V, 1.0 / N, perm=torch.randperm(N, generator=g).cuda()) for _ in range(32)]
  finally:
    capi.set_deterministic(prev)
  for key in ("dW", "db"):
    floor = max(np.abs(p[key] - q[key]).max() for i, p in enumerate(runs) for q in runs[i + 1:])
    gap = np.abs(runs[0][key] - a[key]).max()
    others = [np.abs(p[key] - a[key]).max() for p in runs[1:]]
    print("%s: default vs deterministic %.3e (permuted rows: %.3e .. %.3e), between atomic-mode runs %.3e"
          % (key, gap, min(others), max(others), floor))
    assert gap <= floor, (key, gap, floor)
  assert torch.equal(runs[0]["dx16"], a["dx16"])
