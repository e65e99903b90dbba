"""The LSTM language model end to end through run.py: data layer -> LMEncoder (LayerNorm-LSTM kernels) ->
BasicSequenceLoss -> Adam, checkpoint, greedy generation.

Corpus: a period-7 token cycle (seven words on one long line, so no '<eos>' falls inside it) over a 16-word
vocabulary, written as a raw corpus into a tmp dir. Model: 2 layers, H = 32, E = 16 (tied), bptt 12, batch 8, Adam,
every keep probability 1.0, 300 steps through run.py's train path. The training loss must end below 1/2 ln 16: ln 16
is the uniform predictor's loss and the sequence has zero entropy given one token. Then the checkpoint the loop
saved (reference variable names) is restored into an infer-mode model: seed_tokens of two words, num_tokens_gen 10,
every row must continue the cycle for all ten tokens; a second restore gives the same ids. Eval mode from the
same checkpoint must score the validation stream below the same bound.
A second short run with the wkt2 config's dropout values (0.6 / 0.7 / 0.37) only has to produce finite, decreasing
loss and identical losses under the same seed twice."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = """
from open_seq2seq.configs.lstm_lm import lstm_lm_config
base_model, base_params, train_params, eval_params, infer_params = lstm_lm_config(
    %(raw)r, %(proc)r, batch_size_per_gpu=8, bptt=12, layers=2, num_units=32, emb_size=16, learning_rate=0.01,
    dropout=%(dropout)r, seed_tokens="c1 c4", num_tokens_gen=10, logdir=%(logdir)r, max_steps=%(steps)d)
base_params["print_loss_steps"] = 100
train_params["data_layer_params"].update(shuffle=False, rand_start=False)
"""


@pytest.fixture(autouse=True)
def _deterministic_kernels():
  """No fp32 atomics across workgroups (the embedding scatter): a seed's trajectory is the same on every run."""
  from openseq2seq_amd import capi
  prev = capi.deterministic()
  capi.set_deterministic(True)
  try:
    yield
  finally:
    capi.set_deterministic(prev)


def _config(tmp_path, name, dropout, steps):
  from openseq2seq_amd.data.lm.synthetic import write_cycle_corpus
  raw = write_cycle_corpus(str(tmp_path / "raw"))
  path = str(tmp_path / (name + ".py"))
  with open(path, "w") as f:
    f.write(CONFIG % dict(raw=raw, proc=str(tmp_path / "proc"), dropout=dropout, logdir=str(tmp_path / ("log_" + name)),
                          steps=steps))
  return path


def test_lm_learns_the_cycle_and_generates_it(cuda, tmp_path):
  sys.path.insert(0, REPO)
  import run
  from openseq2seq_amd.utils import checkpoint
  from openseq2seq_amd.utils.utils import create_model, get_base_config
  cfg = _config(tmp_path, "cycle", False, 300)
  args, base, model_cls, module = get_base_config(["--config_file=" + cfg, "--mode=train"])
  model = create_model(args, base, module, model_cls, None)
  dl = model.get_data_layer()
  assert dl.vocab_size == 16 and model.get_encoder().layers[1].H == 16
  run.train(model, args)
  batch = next(dl.iterate_batches(model._device))
  loss = float(model.train_step(batch).cpu()[0])
  print("final training loss %.4f (1/2 ln 16 = %.4f)" % (loss, 0.5 * math.log(16)))
  assert loss < 0.5 * math.log(16), loss
  prefix = checkpoint.latest_checkpoint(base["logdir"])
  names = set(checkpoint.open_checkpoint(prefix).keys())
  cell = "ForwardPass/rnn_encoder_awd/decoder/multi_rnn_cell/cell_%d/weight_drop_layer_norm_basic_lstm_cell/"
  assert {"ForwardPass/rnn_encoder_awd/dense/kernel", "ForwardPass/rnn_encoder_awd/dense/bias", cell % 0 + "kernel",
          cell % 1 + "state/gamma", cell % 1 + "transform/beta"} <= names
  assert not any("EncoderEmbeddingMatrix" in n or n.endswith(("/wx_0", "/wh")) for n in names)
  # ---- eval mode from the saved checkpoint: one pass over the validation stream (the same cycle)
  args, base, model_cls, module = get_base_config(["--config_file=" + cfg, "--mode=eval"])
  emodel = create_model(args, base, module, model_cls, None)
  run.restore_latest(emodel, 0)
  res = run.run_eval(None, emodel, 0)
  assert res["batches"] >= 1 and res["eval_loss"] < 0.5 * math.log(16), res
  # ---- generation from the saved checkpoint
  rows = []
  for k in range(2):
    out = str(tmp_path / ("gen%d.txt" % k))
    args, base, model_cls, module = get_base_config(["--config_file=" + cfg, "--mode=infer",
                                                     "--infer_output_file=" + out])
    imodel = create_model(args, base, module, model_cls, None)
    run.restore_latest(imodel, 0)
    run.infer(imodel, args, 0)
    rows.append([l.split() for l in open(out).read().strip().splitlines()])
  cycle = ["c%d" % i for i in range(7)]
  want = [[cycle[(cycle.index(s) + 1 + i) % 7] for i in range(10)] for s in ("c1", "c4")]
  assert rows[0] == want, rows[0]
  assert rows[1] == rows[0]


def test_lm_trains_with_the_configs_dropout(cuda, tmp_path):
  sys.path.insert(0, REPO)
  from openseq2seq_amd.utils.utils import create_model, get_base_config
  cfg = _config(tmp_path, "drop", True, 40)
  runs = []
  for _ in range(2):
    args, base, model_cls, module = get_base_config(["--config_file=" + cfg, "--mode=train"])
    model = create_model(args, base, module, model_cls, None)
    batches = model.get_data_layer().iterate_batches(model._device)
    runs.append([float(model.train_step(next(batches)).cpu()[0]) for _ in range(40)])
  a, b = runs
  assert all(math.isfinite(v) for v in a)
  assert sum(a[-5:]) / 5 < sum(a[:5]) / 5 - 0.3, (a[:5], a[-5:])
  assert a == b
