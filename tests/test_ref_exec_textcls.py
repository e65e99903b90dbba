"""The text-classification phase of the LSTM language model against the reference's executed code, on the CPU
(tests/golden/ref_exec_textcls.npz, written by tests/golden/make_ref_exec_textcls.py from the reference's own
LMEncoder with fc_dim = 3, WeightDropLayerNormBasicLSTMCell and CrossEntropyLoss; ragged lengths [6, 1, 4, 3];
once on the final h, once on [h, c]).

* With the reference present the generator is run again and must reproduce the committed file (skip otherwise).
* The float64 model oracle (tests/_textcls_model_oracle.py: the language-model oracle's layers under sequence
  lengths, the final state, the head) reproduces the fixture's logits, loss and every variable's gradient (25
  variables: dense/kernel, dense/bias, EncoderEmbeddingMatrix and eleven per cell) to fp32 round-off, under the
  rule of tests/test_ref_exec_lm.py: e32 = max|oracle in fp32 - oracle in fp64| per tensor and
  |oracle64 - fixture| <= 4 e32 + 2^-23 |fixture| elementwise.
* The checkpoint name -> shape table of LMClassifierEncoder equals the fixture's variable names and shapes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _textcls_model_oracle as M
from _lm_model_oracle import SCOPE
from test_ref_exec_lm import _gen

HERE = os.path.dirname(os.path.abspath(__file__))
RUNS = (("h", False), ("hc", True))


def load(tag):
  full = np.load(os.path.join(HERE, "golden", "ref_exec_textcls.npz"))
  d = {k[len(tag) + 1:]: full[k] for k in full.files if k.startswith(tag + "/")}
  d["config"] = full["config"]
  return d, [str(n) for n in d["var_names"]]


def encoder_params(d, use_cell_state):
  B, T, V, E, H, NL, C = [int(v) for v in d["config"]]
  return dict(vocab_size=V, emb_size=E, encoder_layers=NL, encoder_use_skip_connections=False,
              core_cell="WeightDropLayerNormBasicLSTMCell", core_cell_params=dict(num_units=H, forget_bias=1.0),
              end_token=1, batch_size=B, use_cudnn_rnn=False, cudnn_rnn_type=None, encoder_dp_input_keep_prob=1.0,
              encoder_dp_output_keep_prob=1.0, encoder_last_input_keep_prob=1.0, encoder_last_output_keep_prob=1.0,
              recurrent_keep_prob=1.0, encoder_emb_keep_prob=1.0, fc_use_bias=True, weight_tied=True,
              awd_initializer=False, dtype="float32", fc_dim=C, use_cell_state=use_cell_state)


def test_fixture_reproduced_by_the_reference():
  """In a process of its own (see tests/test_ref_exec_lm.py)."""
  if not _gen().gen.reference_available():
    pytest.skip("the reference is not present")
  r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_ref_exec_textcls.py"), "--check"],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
  assert r.returncode == 0 and "textcls: reproduced" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("tag,cell", RUNS)
def test_oracle_reproduces_the_fixture_cpu(tag, cell):
  d, names = load(tag)
  B, T, V, E, H, NL, C = [int(v) for v in d["config"]]
  assert d["lens"].tolist() == [6, 1, 4, 3] and tuple(d["logits"].shape) == (B, C)
  var = {n: d["var/" + n] for n in names}
  o64 = M.run(var, d["src"], d["lens"], d["labels"], NL, cell)
  o32 = M.run(var, d["src"], d["lens"], d["labels"], NL, cell, dtype=torch.float32)
  assert len(names) == 25 and set(o64["grads"]) == set(names)
  assert tuple(d["shape/" + SCOPE + "/dense/kernel"]) == ((2 if cell else 1) * E, C)

  def check(what, a64, a32, fix):
    e32 = float((a32.double() - a64).abs().max())
    f = torch.as_tensor(np.asarray(fix)).double()
    err = (a64 - f).abs()
    assert bool((err <= 4.0 * e32 + 2.0 ** -23 * f.abs()).all()), (what, float(err.max()), e32)

  check("logits", o64["logits"], o32["logits"], d["logits"])
  check("loss", o64["loss"], o32["loss"], d["loss"])
  for n in names:
    assert tuple(o64["grads"][n].shape) == tuple(d["grad/" + n].shape), n
    assert float(np.abs(d["grad/" + n]).max()) > 0.0, n
    check("grad/" + n, o64["grads"][n], o32["grads"][n], d["grad/" + n])


@pytest.mark.parametrize("tag,cell", RUNS)
def test_checkpoint_names_and_shapes_cpu(tag, cell):
  from openseq2seq_amd.encoders import LMClassifierEncoder
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.utils import checkpoint as ck
  d, names = load(tag)
  store = FlatParams(torch.device("cpu"))
  LMClassifierEncoder(encoder_params(d, cell), None, mode="train").build(store)
  table = ck.variable_shapes(store.params)
  assert table == {n: tuple(int(v) for v in d["shape/" + n]) for n in names}
  assert [p.name for p in store.params[:3]] == names[:3]   # the reference's creation order
