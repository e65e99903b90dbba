"""The device LSTM language model against the REFERENCE'S OWN CODE (tests/golden/ref_exec_lm.npz: LMEncoder +
WeightDropLayerNormBasicLSTMCell + BasicSequenceLoss executed from their files, B = 3, T = 5, V = 17, E = 8, H = 16,
two layers of widths 16 and 8, weight_tied).

The device LMEncoder + BasicSequenceLoss are loaded by the reference's variable names from the fixture through
utils/checkpoint.py; one forward + backward pass must give the oracle model's logits, loss and all 24 variable
gradients (reference layout, assembled as checkpoint.model_variables assembles the variables) under the rule of
tests/_lnlstm_cases.py: |got - R_b| <= 4 n_q + 2^-7 |R_b| elementwise, R_b the oracle model with a bf16 round
where the device stores bf16, n_q = max|R_b - R| per tensor from the oracle alone (tests/_lm_model_oracle.py;
tests/test_ref_exec_lm.py holds R to the fixture itself at fp32 round-off). It reads only tests/golden/.

A second pass with the config's dropout values (0.6 / 0.7 / 0.37) must be finite, differ from the first, and give
the same bits under the same seeds. Generation (infer mode) must stop early on end_token and carry its state:
the ids of a T-step greedy run equal those recomputed from the train-mode logits of the generated prefix."""
import os
import types

import numpy as np
import pytest
import torch

import _lm_model_oracle as M
from test_ref_exec_lm import encoder_params, load

pytestmark = pytest.mark.gpu


def _device_model(cuda, d, names, tmp_path, mode="train", **over):
  from openseq2seq_amd.encoders import LMEncoder
  from openseq2seq_amd.losses import BasicSequenceLoss
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.utils import checkpoint as ck
  B, T, V, E, H, NL = [int(v) for v in d["config"]]
  store = FlatParams(cuda)
  enc = LMEncoder(dict(encoder_params(d), **over), None, mode=mode).build(store)
  lossf = BasicSequenceLoss(dict(tgt_vocab_size=V, batch_size=B, offset_target_by_one=False,
                                 average_across_timestep=True, do_mask=False), None)
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
  src = torch.from_numpy(d["src"]).to(cuda)
  tgt = torch.from_numpy(d["tgt"]).to(cuda)
  lens = torch.from_numpy(d["lens"]).to(cuda)
  tape = Tape()
  store.zero_grads()
  e = enc.encode({"source_tensors": [src, lens], "tape": tape, "seeds": SeedSeq(seed)})
  L = lossf.compute_loss({"decoder_output": e, "target_tensors": [tgt, lens]})
  tape.backward()
  torch.cuda.synchronize()
  return e, L


def _reference_grads(store):
  """{reference name: gradient in the reference's layout}, assembled from the device gradients the way
  checkpoint.model_variables assembles the variables."""
  from openseq2seq_amd.utils import checkpoint as ck
  groups = ck.lstm_kernel_groups(store.params)
  grouped = {p.name for ps in groups.values() for p in ps}
  out = {ref: np.concatenate([p.grad.detach().cpu().numpy()[0].T for p in ps], axis=0) for ref, ps in groups.items()}
  for p in store.params:
    if p.name not in grouped:
      for n, a in ck.export_param(ck.reference_name(p.name)[0], p.shape, p.kind, p.grad.detach().cpu().numpy(),
                                  getattr(p, "logical_out", None)):
        out[n] = a
  return out


def test_device_lm_reproduces_the_reference_code(cuda, tmp_path):
  d, names = load()
  B, T, V, E, H, NL = [int(v) for v in d["config"]]
  store, enc, lossf = _device_model(cuda, d, names, tmp_path)
  e, L = _step(cuda, store, enc, lossf, d, 3)
  var = {n: d["var/" + n] for n in names}
  R = M.run(var, d["src"], d["tgt"], NL)
  Rb = M.run(var, d["src"], d["tgt"], NL, rounded=True)
  got = _reference_grads(store)
  assert set(got) == set(names)
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

  assert e["outputs"][0].shape == (B, T, V)
  check("logits", e["logits"].float().cpu().numpy()[:, :, :V], R["logits"], Rb["logits"])
  assert bool((e["logits"].float().cpu()[:, :, V:] == 0).all()) or enc.Vpad == V
  check("loss", L.float().cpu().numpy().reshape(()), R["loss"], Rb["loss"])
  for n in names:
    assert got[n].shape == d["grad/" + n].shape, n
    check("grad/" + n, got[n], R["grads"][n], Rb["grads"][n])
  assert not fails, fails


def test_device_lm_dropout_is_seeded(cuda, tmp_path):
  d, names = load()
  drop = dict(encoder_dp_output_keep_prob=0.6, encoder_last_output_keep_prob=0.6, recurrent_keep_prob=0.7,
              encoder_emb_keep_prob=0.37)
  store, enc, lossf = _device_model(cuda, d, names, tmp_path, **drop)
  e1, L1 = _step(cuda, store, enc, lossf, d, 7)
  g1 = store.grads.clone()
  e2, L2 = _step(cuda, store, enc, lossf, d, 7)
  assert torch.equal(e1["logits"].view(torch.int16), e2["logits"].view(torch.int16)) and torch.equal(L1, L2)
  assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0.0
  assert float((g1 - store.grads).abs().max()) <= 1e-5 * float(g1.abs().max())     # fp32 atomics of the scatter
  e3, L3 = _step(cuda, store, enc, lossf, d, 8)
  assert not torch.equal(e1["logits"].view(torch.int16), e3["logits"].view(torch.int16))
  store2, enc2, lossf2 = _device_model(cuda, d, names, tmp_path)
  e0, _ = _step(cuda, store2, enc2, lossf2, d, 7)
  assert not torch.equal(e1["logits"].view(torch.int16), e0["logits"].view(torch.int16))


def test_device_lm_generation(cuda, tmp_path):
  """Greedy generation carries the state: its ids are the argmax of the train-mode (no dropout) logits over the
  same prefix, step by step; it stops once every row has emitted end_token."""
  d, names = load()
  B, T, V, E, H, NL = [int(v) for v in d["config"]]
  seeds = [3, 11]
  store, gen, _ = _device_model(cuda, d, names, tmp_path, mode="infer", seed_tokens=seeds, num_tokens_gen=6,
                                end_token=V + 5)
  out = gen.encode({"source_tensors": [None, None]})
  ids = out["outputs"][0].cpu()
  assert ids.shape == (2, 6) and out["logits"].shape == (2, 6, V)
  assert out["final_sequence_lengths"].cpu().tolist() == [6, 6]
  store, ev, _ = _device_model(cuda, d, names, tmp_path, mode="eval", batch_size=2)
  prefix = torch.cat([torch.tensor(seeds, dtype=torch.int32).view(2, 1), ids[:, :-1].to(torch.int32)], dim=1).to(cuda)
  lens = torch.full((2,), 6, dtype=torch.int32, device=cuda)
  full = ev.encode({"source_tensors": [prefix, lens]})["logits"][:, :, :V].float().cpu()
  assert torch.equal(full.argmax(dim=2), ids.long())
  step = out["logits"].float().cpu()        # the same arithmetic through GEMMs of other row counts: bf16 ulps apart
  assert bool(((full - step).abs() <= 2.0 ** -6 * (1.0 + full.abs())).all())
  # early stop: with end_token = the first generated id of both rows (if they agree) or of row 0 and a 1-step cap
  first = int(ids[0, 0])
  store, gen2, _ = _device_model(cuda, d, names, tmp_path, mode="infer", seed_tokens=[seeds[0]], num_tokens_gen=6,
                                 end_token=first)
  out2 = gen2.encode({"source_tensors": [None, None]})
  assert out2["outputs"][0].shape == (1, 1) and out2["final_sequence_lengths"].cpu().tolist() == [1]
