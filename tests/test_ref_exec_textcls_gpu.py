"""The device text classifier against the REFERENCE'S OWN CODE (tests/golden/ref_exec_textcls.npz: LMEncoder with
fc_dim = 3 + WeightDropLayerNormBasicLSTMCell + CrossEntropyLoss executed from their files; B = 4, T = 6, V = 17,
E = 8, H = 16, two layers of widths 16 and 8, weight_tied, lengths [6, 1, 4, 3]; once on the final h, once on
[h, c]).

The device LMClassifierEncoder + CrossEntropyLoss are loaded by the reference's variable names from the fixture
through utils/checkpoint.py; one forward + backward pass must give the model oracle's logits, loss and all 25
variable gradients (reference layout) under the rule of tests/test_ref_exec_lm_gpu.py: |got - R_b| <= 4 n_q +
2^-7 |R_b| elementwise, R_b the oracle model with a bf16 round where the device stores bf16, n_q = max|R_b - R|
per tensor from the oracle alone (tests/_textcls_model_oracle.py; tests/test_ref_exec_textcls.py holds R to the
fixture itself at fp32 round-off). It reads only tests/golden/.

A second pass with the transfer configs' dropout (output 0.8, embedding matrix 0.7) must be finite, differ from the
first, and give the same bits under the same seeds."""
import os
import types

import numpy as np
import pytest
import torch

import _textcls_model_oracle as M
from test_ref_exec_lm_gpu import _reference_grads
from test_ref_exec_textcls import RUNS, encoder_params, load

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _deterministic_kernels():
  """No fp32 atomics in the embedding scatter: the same seeds give the same bits."""
  from openseq2seq_amd import capi
  prev = capi.deterministic()
  capi.set_deterministic(True)
  try:
    yield
  finally:
    capi.set_deterministic(prev)


def _device_model(cuda, d, names, cell, tmp_path, **over):
  from openseq2seq_amd.encoders import LMClassifierEncoder
  from openseq2seq_amd.losses import CrossEntropyLoss
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.utils import checkpoint as ck
  store = FlatParams(cuda)
  enc = LMClassifierEncoder(dict(encoder_params(d, cell), **over), None, mode="train").build(store)
  lossf = CrossEntropyLoss({}, None)
  store.finalize()
  path = os.path.join(str(tmp_path), "ref.npz")
  np.savez(path, **{n: d["var/" + n] for n in names})
  model = types.SimpleNamespace(store=store, params={"dtype": "float32"})
  assert ck.load(model, path, restore_optimizer=False) == []
  written = ck.model_variables(model)
  for n in names:
    assert written[n].shape == d["var/" + n].shape and np.array_equal(written[n], d["var/" + n]), n
  return store, enc, lossf


def _step(cuda, store, enc, lossf, d, seed):
  from openseq2seq_amd.parts.dense import SeedSeq
  from openseq2seq_amd.parts.tape import Tape
  B, T, V, E, H, NL, C = [int(v) for v in d["config"]]
  src = torch.from_numpy(d["src"]).to(cuda)
  lens = torch.from_numpy(d["lens"]).to(cuda)
  tgt = [torch.from_numpy(d["labels"]).to(cuda), torch.full((B,), C, dtype=torch.int32, device=cuda)]
  tape = Tape()
  store.zero_grads()
  e = enc.encode({"source_tensors": [src, lens], "tape": tape, "seeds": SeedSeq(seed)})
  L = lossf.compute_loss({"decoder_output": e, "target_tensors": tgt})
  tape.backward()
  torch.cuda.synchronize()
  return e, L


@pytest.mark.parametrize("tag,cell", RUNS)
def test_device_classifier_reproduces_the_reference_code(cuda, tmp_path, tag, cell):
  d, names = load(tag)
  B, T, V, E, H, NL, C = [int(v) for v in d["config"]]
  store, enc, lossf = _device_model(cuda, d, names, cell, tmp_path)
  e, L = _step(cuda, store, enc, lossf, d, 3)
  var = {n: d["var/" + n] for n in names}
  R = M.run(var, d["src"], d["lens"], d["labels"], NL, cell)
  Rb = M.run(var, d["src"], d["lens"], d["labels"], NL, cell, rounded=True)
  got = _reference_grads(store)
  assert set(got) == set(names) and len(names) == 25
  fails = []

  def check(what, g, r, rb_):
    g = torch.as_tensor(np.asarray(g)).double()
    nq = float((rb_ - r).abs().max())
    err = (g - rb_).abs()
    bound = 4.0 * nq + 2.0 ** -7 * rb_.abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("  %-4s %s n_q %.3e max err %.3e err/bound %.3e" % ("ok" if worst <= 1.0 else "FAIL", what, nq,
                                                             float(err.max()), worst))
    if not bool((err <= bound).all()):
      fails.append((what, nq, float(err.max()), worst))

  assert e["logits"].dtype == torch.float32 and tuple(e["logits"].shape) == (B, C) and e["outputs"][0] is e["logits"]
  check("logits", e["logits"].cpu().numpy(), R["logits"], Rb["logits"])
  check("loss", L.cpu().numpy().reshape(()), R["loss"], Rb["loss"])
  for n in names:
    assert got[n].shape == d["grad/" + n].shape, n
    check("grad/" + n, got[n], R["grads"][n], Rb["grads"][n])
  assert not fails, fails


@pytest.mark.parametrize("tag,cell", RUNS)
def test_device_classifier_dropout_is_seeded(cuda, tmp_path, tag, cell):
  d, names = load(tag)
  drop = dict(encoder_dp_output_keep_prob=0.8, encoder_last_output_keep_prob=0.8, encoder_emb_keep_prob=0.7)
  store, enc, lossf = _device_model(cuda, d, names, cell, tmp_path, **drop)
  e1, L1 = _step(cuda, store, enc, lossf, d, 7)
  g1 = store.grads.clone()
  e2, L2 = _step(cuda, store, enc, lossf, d, 7)
  assert torch.equal(e1["logits"].view(torch.int32), e2["logits"].view(torch.int32)) and torch.equal(L1, L2)
  assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0.0 and bool(torch.isfinite(L1).all())
  assert torch.equal(g1.view(torch.int32), store.grads.view(torch.int32))
  store2, enc2, lossf2 = _device_model(cuda, d, names, cell, tmp_path)
  e0, _ = _step(cuda, store2, enc2, lossf2, d, 7)
  assert not torch.equal(e1["logits"].view(torch.int32), e0["logits"].view(torch.int32))
