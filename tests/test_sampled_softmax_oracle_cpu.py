"""The sampled-softmax oracle of tests/_sampled_softmax_cases.py checked on the CPU, before anything on the GPU is
held to it: the sequential sampler draws classes with the log-uniform probabilities, its ids are distinct and in
range, a small try cap takes the fill path; the explicit fp64 gradients of R equal torch autograd of the same loss;
an accidental hit carries no probability mass and exactly zero gradient; and with log Q -> 0 and the candidates
covering every class but the row's label R is the full softmax cross entropy."""
import numpy as np
import torch

import _sampled_softmax_cases as ssc


def test_draw_frequencies_follow_the_log_uniform_law():
  V, n = 200, 200000
  k = ssc.draw_classes(V, seed=12345, n=n)
  assert k.min() >= 0 and k.max() <= V - 1
  p = np.log((np.arange(V) + 2.0) / (np.arange(V) + 1.0)) / np.log(V + 1.0)
  assert abs(p.sum() - 1.0) < 1e-12
  cnt = np.bincount(k, minlength=V)
  z = (cnt - n * p) / np.sqrt(n * p * (1 - p))
  print("max |z| %.2f, chi2/dof %.3f" % (np.abs(z).max(), float((z * z * (1 - p)).sum() / (V - 1))))
  assert np.abs(z).max() < 4.5


def test_ids_are_distinct_and_in_range():
  for V, S, seed in ((16, 8, 1), (200, 64, 2), (40000, 1024, 3)):
    ids, tries = ssc.sample(V, S, seed)
    assert len(ids) == S == len(set(ids.tolist())) and ids.min() >= 0 and ids.max() < V
    assert S <= tries <= 16 * S + 64
    # the stopping try drew the last id, and every earlier try drew one of the ids before it
    k = ssc.draw_classes(V, seed, tries)
    assert k[-1] == ids[-1] and set(k[:-1].tolist()) == set(ids[:-1].tolist())


def test_small_cap_takes_the_fill_path():
  V, S, cap = 64, 32, 40
  ids, tries = ssc.sample(V, S, seed=5, max_tries=cap)
  drawn = []
  for k in ssc.draw_classes(V, 5, cap):
    if k not in drawn:
      drawn.append(int(k))
  assert len(drawn) < S, "the cap must bite for this test"
  assert tries == cap and ids[:len(drawn)].tolist() == drawn
  rest = [k for k in range(V) if k not in drawn][:S - len(drawn)]
  assert ids[len(drawn):].tolist() == rest and len(set(ids.tolist())) == S


def _torch_loss(x, W, b, labels, ids, tries, V, scale):
  lq_l = torch.from_numpy(ssc.log_q(labels, tries, V))
  lq_s = torch.from_numpy(ssc.log_q(ids, tries, V))
  lab, sid = torch.from_numpy(labels), torch.from_numpy(ids)
  true = (x * W[lab]).sum(1) + b[lab] - lq_l
  samp = x @ W[sid].t() + b[sid] - lq_s
  samp = samp.masked_fill(sid[None, :] == lab[:, None], float("-inf"))
  z = torch.cat([true[:, None], samp], dim=1)
  return scale * (torch.logsumexp(z, dim=1) - true).sum()


def test_explicit_gradients_equal_autograd():
  V, S, N, D = 40, 16, 9, 8
  c = ssc.make_case(N, D, V, S, seed=7)
  assert ssc.count_hit_rows(c["labels"], c["ids"]) >= 3
  scale = 1.0 / N
  r = ssc.reference(c["x"], c["W"], c["b"], c["labels"], c["ids"], c["tries"], V, scale)
  x, W, b = (torch.from_numpy(c[k]).requires_grad_(True) for k in ("x", "W", "b"))
  loss = _torch_loss(x, W, b, c["labels"], c["ids"], c["tries"], V, scale)
  loss.backward()
  assert abs(float(loss.detach()) - r["loss"]) < 1e-12
  for got, ref in ((x.grad, r["dx"]), (W.grad, r["dW"]), (b.grad, r["db"])):
    assert np.abs(got.numpy() - ref).max() < 1e-13
  untouched = np.setdiff1d(np.arange(V), np.concatenate([c["ids"], c["labels"]]))
  assert len(untouched) and not r["dW"][untouched].any() and not r["db"][untouched].any()


def test_accidental_hit_has_no_mass_and_zero_gradient():
  V, S, N, D = 40, 16, 9, 8
  c = ssc.make_case(N, D, V, S, seed=8)
  r = ssc.reference(c["x"], c["W"], c["b"], c["labels"], c["ids"], c["tries"], V, 1.0)
  assert r["hit"].sum() >= 3
  assert (r["p"][:, 1:][r["hit"]] == 0.0).all() and (r["dlogits"][r["hit"]] == 0.0).all()
  assert np.abs(r["p"].sum(1) - 1.0).max() < 1e-12


def test_full_coverage_without_log_q_is_the_full_softmax(monkeypatch):
  """Known answer independent of the sampler: candidates = every class but the labels, log Q = 0."""
  V, N, D = 12, 6, 8
  g = np.random.RandomState(3)
  x, W, b = g.randn(N, D), g.randn(V, D), g.randn(V)
  labels = np.array([3, 7, 3, 7, 3, 7])
  ids = np.array([k for k in range(V) if k not in (3, 7)])
  monkeypatch.setattr(ssc, "log_q", lambda ids, num_tries, V: np.zeros(len(ids)))
  # a row's label is the `true` column; the OTHER label is missing from its candidates: add both as candidates, the
  # row's own one is then an accidental hit and drops out
  ids = np.concatenate([ids, [3, 7]])
  r = ssc.reference(x, W, b, labels, ids, 1, V, 1.0 / N)
  logits = torch.from_numpy(x @ W.T + b)
  full = torch.nn.functional.cross_entropy(logits, torch.from_numpy(labels), reduction="none").numpy()
  assert np.abs(r["row_loss"] - full).max() < 1e-12
  assert abs(r["loss"] - full.mean()) < 1e-12
