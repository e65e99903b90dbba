"""The LSTM language model trained with the sampled softmax, end to end through run.py: data layer ->
LMSampledEncoder (LayerNorm-LSTM kernels, candidate sampler on the side stream) -> BasicSampledSequenceLoss -> Adam,
checkpoint, full-softmax eval, greedy generation.

The cycle corpus of tests/test_lm_e2e_gpu.py (period 7 over a 16-word vocabulary), 2 layers, H = 32, E = 16 tied,
bptt 12, batch 8, num_sampled = 8 (half the vocabulary: the most the sampler takes), every keep probability 1.0,
deterministic kernels. After 300 steps through run.py's train path the FULL softmax of eval mode, restored from the
saved checkpoint, must score the validation stream below 1/2 ln 16 and greedy generation must continue the cycle;
two trainings under the same seed give identical losses."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = """
from open_seq2seq.configs.lstm_lm import lstm_lm_config
base_model, base_params, train_params, eval_params, infer_params = lstm_lm_config(
    %(raw)r, %(proc)r, batch_size_per_gpu=8, bptt=12, layers=2, num_units=32, emb_size=16, learning_rate=0.01,
    dropout=False, seed_tokens="c1 c4", num_tokens_gen=10, logdir=%(logdir)r, max_steps=%(steps)d, num_sampled=8)
base_params["print_loss_steps"] = 100
train_params["data_layer_params"].update(shuffle=False, rand_start=False)
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


def _config(tmp_path, name, steps):
  from openseq2seq_amd.data.lm.synthetic import write_cycle_corpus
  raw = write_cycle_corpus(str(tmp_path / "raw"))
  path = str(tmp_path / (name + ".py"))
  with open(path, "w") as f:
    f.write(CONFIG % dict(raw=raw, proc=str(tmp_path / "proc"), logdir=str(tmp_path / ("log_" + name)), steps=steps))
  return path


def test_sampled_training_learns_the_cycle(cuda, tmp_path):
  sys.path.insert(0, REPO)
  import run
  from openseq2seq_amd.encoders import LMEncoder, LMSampledEncoder
  from openseq2seq_amd.losses import BasicSampledSequenceLoss
  from openseq2seq_amd.utils.utils import create_model, get_base_config
  cfg = _config(tmp_path, "cycle", 300)
  args, base, model_cls, module = get_base_config(["--config_file=" + cfg, "--mode=train"])
  model = create_model(args, base, module, model_cls, None)
  enc = model.get_encoder()
  assert type(enc) is LMSampledEncoder and enc.sampled and model.get_data_layer().vocab_size == 16
  assert type(model.get_loss_computator()) is BasicSampledSequenceLoss
  run.train(model, args)
  # ---- the full softmax of eval mode from the saved checkpoint
  args, base, model_cls, module = get_base_config(["--config_file=" + cfg, "--mode=eval"])
  emodel = create_model(args, base, module, model_cls, None)
  assert type(emodel.get_encoder()) is LMEncoder
  run.restore_latest(emodel, 0)
  res = run.run_eval(None, emodel, 0)
  print("full-softmax eval loss %.4f (1/2 ln 16 = %.4f)" % (res["eval_loss"], 0.5 * math.log(16)))
  assert res["batches"] >= 1 and res["eval_loss"] < 0.5 * math.log(16), res
  # ---- generation from the saved checkpoint
  out = str(tmp_path / "gen.txt")
  args, base, model_cls, module = get_base_config(["--config_file=" + cfg, "--mode=infer", "--infer_output_file=" + out])
  imodel = create_model(args, base, module, model_cls, None)
  run.restore_latest(imodel, 0)
  run.infer(imodel, args, 0)
  rows = [l.split() for l in open(out).read().strip().splitlines()]
  cycle = ["c%d" % i for i in range(7)]
  assert rows == [[cycle[(cycle.index(s) + 1 + i) % 7] for i in range(10)] for s in ("c1", "c4")], rows


def test_same_seed_gives_identical_losses(cuda, tmp_path):
  sys.path.insert(0, REPO)
  from openseq2seq_amd.utils.utils import create_model, get_base_config
  cfg = _config(tmp_path, "twice", 30)
  runs = []
  for _ in range(2):
    args, base, model_cls, module = get_base_config(["--config_file=" + cfg, "--mode=train"])
    model = create_model(args, base, module, model_cls, None)
    batches = model.get_data_layer().iterate_batches(model._device)
    runs.append([float(model.train_step(next(batches)).cpu()[0]) for _ in range(30)])
  a, b = runs
  assert all(math.isfinite(v) for v in a)
  assert sum(a[-5:]) / 5 < sum(a[:5]) / 5 - 0.3, (a[:5], a[-5:])
  assert a == b


# ---------------------------------------------------------------- one train step against the chained oracle
def _oracle_step(var, src, tgt, n_layers, ids, tries, rounded):
  """tests/_lm_model_oracle.py's network (tied embedding -> LayerNorm-LSTM layers, the recurrence oracle of
  tests/_lnlstm_cases.py) with the sampled softmax R of tests/_sampled_softmax_cases.py as its head: loss and
  gradients by reference variable name. rounded: R_b, a bf16 round where the device stores bf16."""
  import numpy as np
  import torch
  import _lnlstm_cases as C
  import _sampled_softmax_cases as ssc
  from _lm_model_oracle import CELL, LN, SCOPE
  rd = C.rb if rounded else (lambda x: x)
  t = lambda a: torch.as_tensor(np.asarray(a)).double()
  src, tgt = torch.as_tensor(np.asarray(src)).long(), np.asarray(tgt).reshape(-1)
  B, T = src.shape
  P = rd(t(var[SCOPE + "/dense/kernel"]).t())
  bias = t(var[SCOPE + "/dense/bias"])
  V = P.shape[0]
  cur, layers = P[src], []
  for k in range(n_layers):
    K = t(var[(CELL % k) + "/kernel"])
    n_in = cur.shape[2]
    Wx, Wh = rd(K[:n_in].t()), rd(K[n_in:].t())
    ln = torch.stack([t(var["%s/%s/%s" % (CELL % k, s, g)]) for s in LN for g in ("gamma", "beta")])
    fw = C.forward_oracle(rd(cur @ Wx.t()), Wh, ln, None, rounded=rounded, dtype=torch.float64)
    layers.append((cur, Wx, Wh, ln, fw))
    cur = fw["y"]
  r = ssc.reference(cur.reshape(B * T, -1).numpy(), P.numpy(), bias.numpy(), tgt, ids, tries, V, 1.0 / (B * T),
                    rb=rounded)
  grads = {SCOPE + "/dense/bias": torch.from_numpy(r["db"])}
  dP = torch.from_numpy(r["dW"])
  dcur = torch.from_numpy(r["dx"]).view(B, T, -1)
  for k in range(n_layers - 1, -1, -1):
    x, Wx, Wh, ln, fw = layers[k]
    bw = C.backward_oracle(fw["xhat"], fw["s_hat"], fw["rstd"], dcur, Wh, ln, None, rounded=rounded, dtype=torch.float64)
    d2 = bw["dgx"].reshape(B * T, -1)
    hprev = torch.cat([torch.zeros_like(fw["y"][:, :1]), fw["y"][:, :-1]], dim=1)
    grads[(CELL % k) + "/kernel"] = torch.cat([x.reshape(B * T, -1).t() @ d2, hprev.reshape(B * T, -1).t() @ d2], dim=0)
    for i, s in enumerate(LN):
      grads["%s/%s/gamma" % (CELL % k, s)] = bw["dln"][2 * i]
      grads["%s/%s/beta" % (CELL % k, s)] = bw["dln"][2 * i + 1]
    dcur = rd(d2 @ Wx).view(B, T, -1)
  grads[SCOPE + "/dense/kernel"] = dP.index_add(0, src.reshape(-1), dcur.reshape(B * T, -1)).t()
  return dict(loss=torch.tensor(r["loss"]), grads=grads, hits=int(r["hit"].sum()))


def test_one_train_step_against_the_chained_oracle(cuda):
  """(B, T, V, S) = (2, 5, 40, 16), E = 8 tied, layers of 16 and 8 units: the loss and every parameter gradient, by
  reference variable name. The device's max error against R may be at most twice R_b's own, plus the fp32 floor
  (K + 8) 2^-24 max|R| of a K = 64 term accumulation (the longest sum here: 4 H = 64 gate columns, B T = 10 rows,
  S + 1 = 17 logits)."""
  import types
  import numpy as np
  import torch
  import _sampled_softmax_cases as ssc
  from test_ref_exec_lm_gpu import _reference_grads
  from openseq2seq_amd.configs.lstm_lm import lstm_lm_config
  from openseq2seq_amd.encoders import LMSampledEncoder
  from openseq2seq_amd.losses import BasicSampledSequenceLoss
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.parts.dense import SeedSeq
  from openseq2seq_amd.parts.tape import Tape
  from openseq2seq_amd.utils import checkpoint as ck
  B, T, V, S, NL = 2, 5, 40, 16, 2
  _, base, _, _, _ = lstm_lm_config("unused", "unused", num_units=16, emb_size=8, layers=NL, dropout=False,
                                    num_sampled=S)
  torch.manual_seed(5)
  store = FlatParams(cuda)
  enc = LMSampledEncoder(dict(base["encoder_params"], vocab_size=V, end_token=1, batch_size=B), None,
                         mode="train").build(store)
  lossf = BasicSampledSequenceLoss(dict(base["loss_params"], tgt_vocab_size=V, batch_size=B), None)
  store.finalize()
  with torch.no_grad():
    enc.bias.master[:V] = torch.randn(V, device=cuda) * 0.1          # dense/bias starts at zero: give it values
  var = ck.model_variables(types.SimpleNamespace(store=store, params={"dtype": "float32"}))
  seed = 9
  ids, tries = ssc.sample(V, S, SeedSeq(seed).next())
  g = np.random.RandomState(2)
  src = g.randint(0, V, size=(B, T))
  tgt = g.randint(0, V, size=(B, T))
  tgt.reshape(-1)[:3] = ids[[1, 5, 9]]                                # three accidental hits
  lens = torch.full((B,), T, dtype=torch.int32, device=cuda)
  tape = Tape()
  store.zero_grads()
  e = enc.encode({"source_tensors": [torch.from_numpy(src).int().to(cuda), lens], "tape": tape, "seeds": SeedSeq(seed)})
  assert e["inputs"].shape == (B, T, 8) and e["num_sampled"] == S and "weights" in e and "bias" in e
  L = lossf.compute_loss({"decoder_output": e, "target_tensors": [torch.from_numpy(tgt).int().to(cuda), lens]})
  tape.backward()
  torch.cuda.synchronize()
  assert np.array_equal(e["sampled"]["candidates"][0].cpu().numpy()[:S], ids)
  assert int(e["sampled"]["candidates"][1].cpu()[0]) == tries
  R = _oracle_step(var, src, tgt, NL, ids, tries, rounded=False)
  Rb = _oracle_step(var, src, tgt, NL, ids, tries, rounded=True)
  assert R["hits"] >= 3
  got = _reference_grads(store)
  assert set(got) == set(R["grads"])
  fails = []

  def check(what, dev, r, rb_):
    dev, r, rb_ = (torch.as_tensor(np.asarray(a)).double() for a in (dev, r, rb_))
    e_dev, e_rb = float((dev - r).abs().max()), float((rb_ - r).abs().max())
    floor = (64 + 8) * 2.0 ** -24 * float(r.abs().max())
    ok = e_dev <= 2.0 * e_rb + floor
    print("  %-4s %s: device %.3e  R_b %.3e  floor %.3e" % ("ok" if ok else "FAIL", what, e_dev, e_rb, floor))
    if not ok:
      fails.append((what, e_dev, e_rb, floor))

  check("loss", L.float().cpu().numpy().reshape(()), R["loss"], Rb["loss"])
  for n in sorted(got):
    assert tuple(got[n].shape) == tuple(R["grads"][n].shape), n
    check("grad/" + n, got[n], R["grads"][n], Rb["grads"][n])
  assert not fails, fails
