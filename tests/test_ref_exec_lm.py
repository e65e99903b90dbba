"""The LSTM language model against the reference's executed code, on the CPU (tests/golden/ref_exec_lm.npz, written
by tests/golden/make_ref_exec_lm.py from the reference's own LMEncoder, WeightDropLayerNormBasicLSTMCell and
BasicSequenceLoss).

* With the reference present the generator is run again and must reproduce the committed file (skip otherwise).
* The float64 oracle of the layer (tests/_lnlstm_cases.py, composed into the model by tests/_lm_model_oracle.py),
  fed the fixture's variables and inputs, reproduces the fixture's logits, loss and all 24 gradients to fp32
  round-off. The fixture is an fp32 evaluation, so the bound is taken from the oracle itself: e32 = max|oracle in
  fp32 - oracle in fp64| per tensor, and |oracle64 - fixture| <= 4 e32 + 2^-23 |fixture| elementwise (the factor of
  the 4 n_q rule: another order of the same fp32 operations; the second term is one fp32 ulp of the stored value,
  without which a scalar such as the loss is held to a single draw of e32).
* The checkpoint name -> shape table written for the fixture's architecture equals the fixture's variable names
  and shapes."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _lm_model_oracle as M

HERE = os.path.dirname(os.path.abspath(__file__))


def _gen():
  spec = importlib.util.spec_from_file_location("make_ref_exec_lm", os.path.join(HERE, "golden", "make_ref_exec_lm.py"))
  m = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(m)
  return m


def load():
  d = dict(np.load(os.path.join(HERE, "golden", "ref_exec_lm.npz")))
  names = [str(n) for n in d["var_names"]]
  return d, names


def test_fixture_reproduced_by_the_reference():
  """In a process of its own, as the other test_ref_exec_* tests do: this one may already hold the package's
  open_seq2seq import alias, which would hand the generator the device classes instead of the reference's."""
  if not _gen().gen.reference_available():
    pytest.skip("the reference is not present")
  r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_ref_exec_lm.py"), "--check"],
                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
  assert r.returncode == 0 and "lm: reproduced" in r.stdout, r.stdout[-2000:]


def test_oracle_reproduces_the_fixture_cpu():
  d, names = load()
  B, T, V, E, H, NL = [int(v) for v in d["config"]]
  var = {n: d["var/" + n] for n in names}
  o64 = M.run(var, d["src"], d["tgt"], NL)
  o32 = M.run(var, d["src"], d["tgt"], NL, dtype=torch.float32)
  assert len(names) == 24 and set(o64["grads"]) == set(names)

  def check(what, a64, a32, fix):
    e32 = float((a32.double() - a64).abs().max())
    f = torch.as_tensor(np.asarray(fix)).double()
    err = (a64 - f).abs()
    assert bool((err <= 4.0 * e32 + 2.0 ** -23 * f.abs()).all()), (what, float(err.max()), e32)

  check("logits", o64["logits"], o32["logits"], d["logits"])
  check("loss", o64["loss"], o32["loss"], d["loss"])
  for n in names:
    assert tuple(o64["grads"][n].shape) == tuple(d["grad/" + n].shape), n
    check("grad/" + n, o64["grads"][n], o32["grads"][n], d["grad/" + n])
  assert abs(float(d["loss"]) - np.log(V)) < 0.2          # near the uniform predictor, as an untrained model is


def test_checkpoint_names_and_shapes_cpu():
  from openseq2seq_amd.encoders import LMEncoder
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.utils import checkpoint as ck
  d, names = load()
  B, T, V, E, H, NL = [int(v) for v in d["config"]]
  store = FlatParams(torch.device("cpu"))
  LMEncoder(encoder_params(d), None, mode="train").build(store)
  table = ck.variable_shapes(store.params)
  assert table == {n: tuple(int(v) for v in d["shape/" + n]) for n in names}
  # not tied: the embedding matrix is a variable of its own, [V, E]
  store = FlatParams(torch.device("cpu"))
  LMEncoder(dict(encoder_params(d), weight_tied=False), None, mode="train").build(store)
  table = ck.variable_shapes(store.params)
  assert table[M.SCOPE + "/EncoderEmbeddingMatrix"] == (V, E)
  assert table[M.SCOPE + "/dense/kernel"] == (H, V) and table[(M.CELL % 1) + "/kernel"] == (2 * H, 4 * H)


def encoder_params(d):
  B, T, V, E, H, NL = [int(v) for v in d["config"]]
  return dict(vocab_size=V, emb_size=E, encoder_layers=NL, encoder_use_skip_connections=False,
              core_cell="WeightDropLayerNormBasicLSTMCell", core_cell_params=dict(num_units=H, forget_bias=1.0),
              end_token=1, batch_size=B, use_cudnn_rnn=False, cudnn_rnn_type=None, encoder_dp_input_keep_prob=1.0,
              encoder_dp_output_keep_prob=1.0, encoder_last_input_keep_prob=1.0, encoder_last_output_keep_prob=1.0,
              recurrent_keep_prob=1.0, encoder_emb_keep_prob=1.0, fc_use_bias=True, weight_tied=True,
              awd_initializer=False, dtype="float32")
