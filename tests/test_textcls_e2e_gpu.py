"""The text classifier end to end through run.py: SSTDataLayer -> LMClassifierEncoder (LayerNorm-LSTM kernels,
final-state head) -> CrossEntropyLoss -> Adam, checkpoint, eval, infer; and the transfer from a language model.

Toy task: a processed folder in tmp_path over a 20-word vocabulary, reviews of 3 - 12 tokens, label = whether the
marker token occurs. Network: 2 layers of 16 / 8 units, [h, c] classifier, fixed seeds, deterministic kernels.
train_eval for 200 steps: the mean loss of the last 10 steps is below that of the first 10; eval from the saved
checkpoint reports accuracy / precision / recall / f1 / eval_loss; infer writes the TSV with its header and one row
per test sample, predictions in {0, 1}. Record (not a gate), MI355X, when this file was written: mean loss 0.700
(first 10 steps) -> 0.032 (last 10), eval accuracy 0.967 on the 60 validation reviews (precision 1.0, recall 0.933,
F1 0.966, eval_loss 0.148), test accuracy 1.0 on the 40 test reviews.

Transfer: a tiny language model is trained for 2 steps and saved; a classifier started with load_model takes its
cells bit for bit while dense/kernel, dense/bias and EncoderEmbeddingMatrix keep their fresh initial values; with a
checkpoint of its own in logdir that one is restored instead, in training and in eval mode."""
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARKER = 5
CONFIG = """
from open_seq2seq.configs.text_cls import text_cls_config
base_model, base_params, train_params, eval_params, infer_params = text_cls_config(
    "sst", %(proc)r, %(vocab)r, load_model=%(load_model)r, batch_size_per_gpu=20, max_length=10, layers=2,
    num_units=16, emb_size=8, learning_rate=0.01, dropout=False, logdir=%(logdir)r, max_steps=%(steps)d)
base_params["print_loss_steps"] = 1
base_params["eval_steps"] = 100
train_params["data_layer_params"]["shuffle_buffer_size"] = 64
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


def write_vocab(path, n):
  words = ["<unk>", "<eos>"] + ["w%d" % i for i in range(n - 2)]
  with open(path, "w") as f:
    for i, w in enumerate(words):
      f.write("%d\t%s\t%d\n" % (i, w, 100 - i))
    f.write("%d\n" % n)
  return path


def write_task(folder, vocab_size, sizes=(("train", 400), ("valid", 60), ("test", 40))):
  rng = random.Random(11)
  os.makedirs(folder, exist_ok=True)
  plain = [i for i in range(2, vocab_size) if i != MARKER]
  for split, n in sizes:
    with open(os.path.join(folder, split + ".ids"), "w") as ids, open(os.path.join(folder, split + ".rat"), "w") as rat:
      for k in range(n):
        review = [rng.choice(plain) for _ in range(rng.randint(3, 12))]
        if k % 2:
          review[rng.randrange(len(review))] = MARKER
        ids.write("\t".join(map(str, review)) + "\n")
        rat.write("%d\n" % (k % 2))
  return folder


def _config(tmp_path, name, proc, vocab, steps, load_model=None):
  path = str(tmp_path / (name + ".py"))
  with open(path, "w") as f:
    f.write(CONFIG % dict(proc=proc, vocab=vocab, load_model=load_model, logdir=str(tmp_path / ("log_" + name)),
                          steps=steps))
  return path


def _model(cfg, mode, *extra):
  from openseq2seq_amd.utils.utils import create_model, get_base_config
  args, base, model_cls, module = get_base_config(["--config_file=" + cfg, "--mode=" + mode] + list(extra))
  return create_model(args, base, module, model_cls, None), args, base


def test_classifier_learns_the_marker_task(cuda, tmp_path, capsys):
  sys.path.insert(0, REPO)
  import run
  proc = write_task(str(tmp_path / "proc"), 20)
  cfg = _config(tmp_path, "toy", proc, write_vocab(str(tmp_path / "vocab.txt"), 20), 200)
  model, args, base = _model(cfg, "train_eval")
  from openseq2seq_amd.encoders import LMClassifierEncoder
  assert type(model.get_encoder()) is LMClassifierEncoder and model.get_encoder().layers[1].H == 8
  run.train(model, args, final_eval=True)
  out = capsys.readouterr().out
  losses = [float(m) for m in re.findall(r"step \d+ loss ([-0-9.einf]+)", out)]
  assert len(losses) == 200 and all(np.isfinite(losses))
  first, last = float(np.mean(losses[:10])), float(np.mean(losses[-10:]))
  assert last < first, (first, last)
  assert "EVAL Accuracy" in out
  # ---- eval from the saved checkpoint
  emodel, _, _ = _model(cfg, "eval")
  run.restore_latest(emodel, 0)
  res = run.run_eval(None, emodel, 0)
  assert {"accuracy", "precision", "recall", "f1", "eval_loss"} <= set(res), res
  assert 0.0 <= res["accuracy"] <= 1.0 and np.isfinite(res["eval_loss"])
  with capsys.disabled():
    print("toy task: loss %.4f -> %.4f, eval %s" % (first, last, res))
  # ---- infer: the TSV
  tsv = str(tmp_path / "pred.tsv")
  imodel, iargs, _ = _model(cfg, "infer", "--infer_output_file=" + tsv)
  run.restore_latest(imodel, 0)
  run.infer(imodel, iargs, 0)
  lines = open(tsv).read().rstrip("\n").split("\n")
  assert lines[0] == "Source\tPred\tLabel" and len(lines) == 1 + 40
  rows = [l.split("\t") for l in lines[1:]]
  assert all(len(r) == 3 and r[1] in ("0", "1") and r[2] in ("0", "1") for r in rows)
  assert [r[2] for r in rows] == [str(k % 2) for k in range(40)]
  assert all(("w%d" % (MARKER - 2) in r[0].split()) == (r[2] == "1") for r in rows)


def _masters(model):
  return {p.name: p.master.detach().cpu().clone() for p in model.store.params}


def test_transfer_from_a_language_model(cuda, tmp_path, capsys):
  sys.path.insert(0, REPO)
  import run
  from openseq2seq_amd.data.lm.synthetic import write_cycle_corpus
  from openseq2seq_amd.utils import checkpoint
  from openseq2seq_amd.utils.utils import create_model, get_base_config
  # ---- the language model: 2 steps, saved under the reference's names
  raw = write_cycle_corpus(str(tmp_path / "raw"))
  lm_cfg = str(tmp_path / "lm.py")
  lm_log = str(tmp_path / "log_lm")
  with open(lm_cfg, "w") as f:
    f.write("from open_seq2seq.configs.lstm_lm import lstm_lm_config\n"
            "base_model, base_params, train_params, eval_params, infer_params = lstm_lm_config(\n"
            "    %r, %r, batch_size_per_gpu=8, bptt=12, layers=2, num_units=16, emb_size=8, dropout=False,\n"
            "    logdir=%r, max_steps=2)\n" % (raw, str(tmp_path / "lm_proc"), lm_log))
  lm, lm_args, _ = _model(lm_cfg, "train")
  run.train(lm, lm_args)
  lm_vars = _masters(lm)
  vocab = os.path.join(str(tmp_path / "lm_proc"), "vocab.txt")
  V = lm.get_data_layer().vocab_size
  assert V == 16 and checkpoint.latest_checkpoint(lm_log) is not None
  # ---- a classifier on the language model's vocabulary, started with load_model
  proc = write_task(str(tmp_path / "proc"), V)
  cfg = _config(tmp_path, "cls", proc, vocab, 3, load_model=lm_log)
  fresh_cfg = _config(tmp_path, "fresh", proc, vocab, 3)
  fresh, _, _ = _model(fresh_cfg, "train")
  init = _masters(fresh)                                     # the same random_seed: the same initial values
  model, args, base = _model(cfg, "train")
  assert all(torch.equal(init[n], v) for n, v in _masters(model).items())
  capsys.readouterr()
  assert run.restore_for_training(model, args, 0) == 0
  out = capsys.readouterr().out
  got = _masters(model)
  cells = [n for n in got if "/cells/cell_" in n]
  own = [n for n in got if n not in cells]
  assert len(cells) == 24 and sorted(n.rsplit("/", 2)[-2] + "/" + n.rsplit("/", 1)[-1] for n in own) == \
      ["dense/bias", "dense/kernel", "rnn_encoder_awd/EncoderEmbeddingMatrix"]
  for n in cells:
    assert torch.equal(got[n].view(torch.int32), lm_vars[n].view(torch.int32)), n
    assert not torch.equal(got[n], init[n]) or n.endswith(("gamma", "beta")), n
  for n in own:
    assert torch.equal(got[n].view(torch.int32), init[n].view(torch.int32)), n
  listed, skipped = out.split("VARS_SKIPPED")
  assert "VARS_TO_LOAD" in listed and all(n in listed for n in cells) and all(n in skipped for n in own)
  assert model.global_step() == 0
  # ---- a checkpoint of its own in logdir wins, in training and in eval mode
  run.train(model, args)                                     # 3 steps, then saves into logdir
  trained = _masters(model)
  assert not torch.equal(trained[own[0]], init[own[0]])
  again, args2, _ = _model(cfg, "train")
  run.restore_for_training(again, args2, 0)
  emodel, _, _ = _model(cfg, "eval")
  run.restore_latest(emodel, 0)
  for m in (again, emodel):
    now = _masters(m)
    for n in trained:
      assert torch.equal(now[n].view(torch.int32), trained[n].view(torch.int32)), n
