"""Training summaries end to end: the smallest LM of configs.lstm_lm.lstm_lm_config (units 16, embedding 8, 2 layers)
runs four steps with save_summaries_steps = 2 and every summary kind, once with max_grad_norm and once with
larc_params (mixed precision with the Backoff loss scaler, so that the loss scale is a device value other than 1).

Bounds (u = 2^-24, the relative rounding of the fp32 `simple_value` a scalar is stored as):
  variable_norm vs torch.norm of the fp32 master in float64: 2u (one rounding to fp32, slack for the double sums)
  sqrt(sum gradient_norm^2) vs the logged global norm: 4u (u per norm, half of 2u after the root, u for the global)
  clipped global norm <= max_grad_norm * (1 + 16u): the clip factor is three fp32 operations, the multiplier one
    more, the per-element products round in both directions
  LARC scalars recomputed from the LOGGED norms and learning rate: 8u (three rounded inputs, one rounded output)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
KINDS = ["learning_rate", "gradients", "gradient_norm", "global_gradient_norm", "variables", "variable_norm",
         "larc_summaries", "loss_scale"]
LARC = {"larc_eta": 0.002, "larc_mode": "clip"}
CLIP = 0.01
CONFIG = """
from open_seq2seq.configs.lstm_lm import lstm_lm_config
base_model, base_params, train_params, eval_params, infer_params = lstm_lm_config(
    %(raw)r, %(proc)r, batch_size_per_gpu=4, bptt=6, layers=2, num_units=16, emb_size=8, learning_rate=0.01,
    dropout=False, logdir=%(logdir)r, max_steps=4)
train_params["data_layer_params"].update(shuffle=False, rand_start=False)
base_params.update(%(extra)r)
"""


@pytest.fixture(autouse=True)
def _deterministic_kernels():
  from openseq2seq_amd import capi
  prev = capi.deterministic()
  capi.set_deterministic(True)
  try:
    yield
  finally:
    capi.set_deterministic(prev)


def _model(tmp, name, extra):
  sys.path.insert(0, REPO)
  from openseq2seq_amd.data.lm.synthetic import write_cycle_corpus
  from openseq2seq_amd.utils.utils import create_model, get_base_config
  raw = write_cycle_corpus(str(tmp / "raw"))
  path = str(tmp / (name + ".py"))
  logdir = str(tmp / ("log_" + name))
  with open(path, "w") as f:
    f.write(CONFIG % dict(raw=raw, proc=str(tmp / "proc"), logdir=logdir, extra=extra))
  args, base, model_cls, module = get_base_config(["--config_file=" + path, "--mode=train"])
  return create_model(args, base, module, model_cls, None), logdir


def _run(tmp, name, extra):
  """Four steps; returns (per-step merged values {step: {tag: value}}, float64 master norms before steps 0 and 2,
  the model)."""
  from openseq2seq_amd import capi
  from openseq2seq_amd.optimizers.summaries import logical_count
  from openseq2seq_amd.utils import summary as S
  prev = capi.deterministic()
  capi.set_deterministic(True)
  try:
    model, logdir = _model(tmp, name, extra)
    assert model.open_summaries() is not None
    batches = model.get_data_layer().iterate_batches(model._device)
    norms = {}
    for step in range(4):
      if step % 2 == 0:
        torch.cuda.synchronize()
        norms[step] = [float(p._master.reshape(-1)[:logical_count(p)].double().norm()) for p in model.store.params]
      model.train_step(next(batches), step)
    model.close_summaries()
    torch.cuda.synchronize()
  finally:
    capi.set_deterministic(prev)
  (path,) = S.event_files(logdir)
  merged = {}
  for _, step, values in S.read_events(path)[1:]:
    merged.setdefault(step, {}).update(values)
  return merged, norms, model


@pytest.fixture(scope="module")
def runs(cuda, tmp_path_factory):
  tmp = tmp_path_factory.mktemp("summaries")
  mixed = {"dtype": "mixed", "loss_scaling": "Backoff", "larc_params": LARC, "summaries": KINDS,
           "save_summaries_steps": 2}
  return {
      "clip": _run(tmp, "clip", {"max_grad_norm": CLIP, "summaries": KINDS, "save_summaries_steps": 2}),
      "larc": _run(tmp, "larc", dict(mixed, os2s_async_optimizer=False)),
      "larc_async": _run(tmp, "larc_async", dict(mixed, os2s_async_optimizer=True)),
  }


def _expected_tags(model, which, step):
  from openseq2seq_amd.utils import summary as S
  tags = {"train_loss", "learning_rate", S.OPT_PREFIX + "global_gradient_norm"}
  if model.steps_in_epoch:
    tags.add("epoch")
  if step > 0:
    tags.add("global_step/sec")
  if which == "clip":
    tags.add(S.OPT_PREFIX + "global_clipped_gradient_norm")
  else:
    tags.add(S.OPT_PREFIX + "loss_scale")
  per_var = ["gradients", "variables", "gradient_norm", "variable_norm"]
  if which != "clip":
    per_var += ["larc_clip_on", "larc_grad_update", "larc_final_lr"]
  for p in model.store.params:
    assert p.name.endswith(":0") or ":" not in p.name
    for k in per_var:
      tags.add("%s%s/%s" % (S.OPT_PREFIX, k, p.name.replace(":", "_")))
  return tags


@pytest.mark.parametrize("which", ["clip", "larc"])
def test_steps_and_tags(runs, which):
  merged, _, model = runs[which]
  assert sorted(merged) == [0, 2]
  for step in (0, 2):
    assert set(merged[step]) == _expected_tags(model, which, step)
    assert math.isfinite(merged[step]["train_loss"])
    assert merged[step]["learning_rate"] == pytest.approx(0.01, rel=2 * U)
  if which == "larc":
    assert merged[0]["Loss_Optimization/loss_scale"] == 2.0 ** 14


@pytest.mark.parametrize("which", ["clip", "larc"])
def test_variable_norms_and_histogram_counts(runs, which):
  from openseq2seq_amd.optimizers.summaries import logical_count
  merged, norms, model = runs[which]
  for step in (0, 2):
    for i, p in enumerate(model.store.params):
      var = p.name.replace(":", "_")
      got, ref = merged[step]["Loss_Optimization/variable_norm/" + var], norms[step][i]
      assert abs(got - ref) <= 2 * U * ref, (step, p.name, got, ref)
      for kind in ("variables", "gradients"):
        h = merged[step]["Loss_Optimization/%s/%s" % (kind, var)]
        assert h["num"] == logical_count(p) == sum(h["bucket"]), (step, kind, p.name)
        assert h["min"] <= h["max"] and len(h["bucket"]) == len(h["bucket_limit"])


def test_global_norm_without_clipping(runs):
  merged, _, model = runs["larc"]
  for step in (0, 2):
    gn = [merged[step]["Loss_Optimization/gradient_norm/" + p.name.replace(":", "_")] for p in model.store.params]
    tot = math.sqrt(math.fsum(g * g for g in gn))
    glob = merged[step]["Loss_Optimization/global_gradient_norm"]
    print("step %d: sqrt(sum gradient_norm^2) %.9g global_gradient_norm %.9g" % (step, tot, glob))
    assert glob > 0 and abs(tot - glob) <= 4 * U * glob


def test_global_norm_with_clipping(runs):
  merged, _, model = runs["clip"]
  for step in (0, 2):
    gn = [merged[step]["Loss_Optimization/gradient_norm/" + p.name.replace(":", "_")] for p in model.store.params]
    tot = math.sqrt(math.fsum(g * g for g in gn))
    pre = merged[step]["Loss_Optimization/global_gradient_norm"]
    clipped = merged[step]["Loss_Optimization/global_clipped_gradient_norm"]
    print("step %d: pre-clip %.9g clipped %.9g sqrt(sum gradient_norm^2) %.9g" % (step, pre, clipped, tot))
    assert abs(tot - clipped) <= 4 * U * clipped
    assert clipped <= CLIP * (1 + 16 * U)
    assert pre > CLIP                    # (the run does clip: the norms above are those of rescaled gradients)
    assert clipped >= CLIP * (1 - 16 * U)


def test_larc_scalars(runs):
  merged, _, model = runs["larc"]
  for step in (0, 2):
    lr = merged[step]["learning_rate"]
    for p in model.store.params:
      var = p.name.replace(":", "_")
      v = merged[step]["Loss_Optimization/variable_norm/" + var]
      g = merged[step]["Loss_Optimization/gradient_norm/" + var]
      u = max(LARC["larc_eta"] * v / (lr * (g + 1e-7)), 1e-7)
      clip_on = merged[step]["Loss_Optimization/larc_clip_on/" + var]
      if abs(u - 1.0) > 8 * U:
        assert clip_on == (1.0 if u < 1.0 else 0.0), (step, p.name, u)
      u = min(u, 1.0)
      got_u = merged[step]["Loss_Optimization/larc_grad_update/" + var]
      got_lr = merged[step]["Loss_Optimization/larc_final_lr/" + var]
      assert abs(got_u - u) <= 8 * U * u, (step, p.name, got_u, u)
      assert abs(got_lr - lr * u) <= 8 * U * lr * u, (step, p.name, got_lr, lr * u)


def test_run_async_gives_the_same_events(runs):
  a, b = runs["larc"][0], runs["larc_async"][0]
  assert sorted(a) == sorted(b) == [0, 2]
  for step in a:
    assert set(a[step]) == set(b[step])
    for tag, va in a[step].items():
      if tag == "global_step/sec":
        continue
      vb = b[step][tag]
      if isinstance(va, float) and math.isnan(va):
        assert math.isnan(vb), (step, tag)
      else:
        assert va == vb, (step, tag, va, vb)


def test_no_event_file_without_save_summaries_steps(cuda, tmp_path):
  from openseq2seq_amd.utils import summary as S
  model, logdir = _model(tmp_path, "off", {"summaries": KINDS})
  assert model.open_summaries() is None
  batches = model.get_data_layer().iterate_batches(model._device)
  for step in range(2):
    model.train_step(next(batches), step)
  model.close_summaries()
  torch.cuda.synchronize()
  assert S.event_files(logdir) == [] and model.train_op._summ is None
