"""CPU side of the any-width Transformer: the reference's toy acceptance configuration in the tree, and a shared
embedding whose vocabulary is no multiple of 8 (device table padded, checkpoint variable at its logical shape)."""
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CFG = "/root/reference/example_configs/text2text/toy-reversal/nmt-reversal-TT.py"
needs_ref = pytest.mark.skipif(not os.path.isfile(REF_CFG), reason="reference checkout not present")


def _load(cfg, mode):
  from openseq2seq_amd.utils.utils import get_base_config
  _, base, model_cls, mod = get_base_config(["--config_file=" + cfg, "--mode=" + mode])
  return base, model_cls, {k: mod.get(k) for k in ("train_params", "eval_params", "infer_params")}


@needs_ref
@pytest.mark.parametrize("mode", ["train", "infer"])
def test_tt_config_is_the_references(mode):
  """example_configs/text2text/toy-reversal/nmt-reversal-TT.py resolves to the same dictionaries as the reference's
  file of that name: every parameter value, the three data splits, the classes."""
  ours = _load(os.path.join(REPO, "example_configs/text2text/toy-reversal/nmt-reversal-TT.py"), mode)
  ref = _load(REF_CFG, mode)
  assert ours[0] == ref[0]
  assert ours[1] is ref[1]
  assert ours[2] == ref[2]


def test_tt_config_values():
  """The values the issue names, held without the reference checkout."""
  base, _, mod = _load(os.path.join(REPO, "example_configs/text2text/toy-reversal/nmt-reversal-TT.py"), "train")
  e, d = base["encoder_params"], base["decoder_params"]
  assert (e["hidden_size"], e["num_heads"], e["encoder_layers"], d["num_hidden_layers"]) == (128, 8, 2, 2)
  assert e["filter_size"] == d["filter_size"] == 512 and d["hidden_size"] == 128 and d["num_heads"] == 8
  assert base["lr_policy_params"] == {"learning_rate": 1.0, "warmup_steps": 200, "d_model": 128}
  assert (d["beam_size"], d["alpha"], d["extra_decode_length"]) == (5, 1.0, 2)
  assert base["max_steps"] == 800 and base["batch_size_per_gpu"] == 64
  assert "pad_embeddings_2_eight" not in e
  for split in mod.values():
    assert "pad_vocab_to_eight" not in split["data_layer_params"]


def _cpu_store(monkeypatch):
  """A FlatParams whose finalize() gives every parameter a CPU master from its initializer (no device buffers)."""
  from openseq2seq_amd.optimizers import flat_params

  def finalize(self, need_m2=False):
    torch.manual_seed(5)
    for p, init in zip(self.params, self._inits):
      p.master = init(tuple(p.shape)) if callable(init) else init.clone().float()
    self.finalized = True
  monkeypatch.setattr(flat_params.FlatParams, "finalize", finalize)
  monkeypatch.setattr(flat_params.FlatParams, "refresh_compute_copies", lambda self: None)
  return flat_params.FlatParams(torch.device("cpu"))


def test_unpadded_vocabulary_keeps_its_logical_checkpoint_shape(monkeypatch, tmp_path):
  """V = 14, D = 128: the device table has 16 rows (rows 14, 15 zero), the variable is written and read as
  [14, 128] under the reference's name, and reading it back leaves the padding rows zero."""
  from openseq2seq_amd.parts.transformer.layers import SharedEmbedding
  from openseq2seq_amd.utils import checkpoint as ck
  store = _cpu_store(monkeypatch)
  emb = SharedEmbedding(store, "ForwardPass/transformer_encoder/embedding_shared_weights", 14, 128)
  assert (emb.V, emb.Vpad) == (14, 16) and emb.weights.shape == (1, 16, 128) and emb.weights.logical_out == 14
  store.finalize()
  w = emb.weights.master.numpy()
  assert np.all(w[0, 14:] == 0) and np.all(np.abs(w[0, :14]).sum(-1) > 0)
  name = "ForwardPass/transformer_encoder/embedding_shared_weights/embedding_and_softmax/weights"
  (n, arr), = ck.export_param(emb.weights.name, emb.weights.shape, "conv", w, emb.weights.logical_out)
  assert n == name and arr.shape == (14, 128)
  np.testing.assert_array_equal(arr, w[0, :14])

  class M(object):
    params = {"dtype": "float32"}
  M.store = store
  variables = ck.model_variables(M())
  assert variables[name].shape == (14, 128)
  back = ck.import_param(emb.weights.name, emb.weights.shape, "conv", {name: arr + 1.0}, emb.weights.logical_out)
  assert back.shape == (1, 16, 128)
  np.testing.assert_array_equal(back[0, :14], arr + 1.0)
  assert np.all(back[0, 14:] == 0)


def test_vocabulary_padding_options_keep_their_meaning(monkeypatch):
  """pad_vocab_to_eight: the extra rows are real vocabulary (V itself grows, nothing is logical); a multiple of 8
  has no padding at all."""
  from openseq2seq_amd.parts.transformer.layers import SharedEmbedding
  store = _cpu_store(monkeypatch)
  a = SharedEmbedding(store, "a", 45, 32, pad_vocab_to_eight=True)
  b = SharedEmbedding(store, "b", 96, 32)
  assert (a.V, a.Vpad, a.weights.logical_out) == (48, 48, None)
  assert (b.V, b.Vpad, b.weights.logical_out) == (96, 96, None)
  store.finalize()
  assert np.all(np.abs(a.weights.master.numpy()[0]).sum(-1) > 0)


# ---- the fixtures at the TT config's widths (tests/golden/make_ref_exec_narrow.py) ------------------------------
def _narrow():
  import importlib.util
  import sys
  here = os.path.dirname(os.path.abspath(__file__))
  for p in (here, REPO):
    if p not in sys.path:
      sys.path.insert(0, p)
  spec = importlib.util.spec_from_file_location("make_ref_exec_narrow",
                                                os.path.join(here, "golden", "make_ref_exec_narrow.py"))
  m = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(m)
  return m


@pytest.mark.skipif(not os.path.isdir("/root/reference/open_seq2seq"), reason="reference checkout not present")
def test_narrow_generator_reproduces_the_committed_fixtures():
  import subprocess
  import sys
  r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "golden", "make_ref_exec_narrow.py"), "--check"],
                     capture_output=True, text=True, timeout=900)
  assert r.returncode == 0 and r.stdout.count("reproduced") == 2, r.stdout + r.stderr


def test_oracle_reproduces_the_reference_transformer_at_tt_widths():
  """oracle/transformer.py against the reference's executed code at d_model 128, 8 heads of 16, V = 14 unpadded
  (forward 1e-5, gradients 1e-4, as tests/test_ref_exec_transformer.py holds the other fixtures)."""
  _narrow()
  import ref_exec_util as rx
  from oracle import transformer as ot
  from test_ref_exec_transformer import oracle_params, rel
  d, names = rx.load("transformer_tt")
  B, S, T, V, D, H, F, NL = [int(v) for v in d["config"]]
  assert (V, D, H, F, NL) == (14, 128, 8, 512, 2)
  assert tuple(d["shape/" + names[0]]) == (14, 128) and d["logits"].shape == (B, T, 14)
  PE, PD, leaves = oracle_params(d, NL)
  assert sorted(leaves) == sorted(names)
  src, tgt = torch.from_numpy(d["src"]).long(), torch.from_numpy(d["tgt"]).long()
  enc_out, bias = ot.encoder(src, PE, H)
  logits = ot.decoder_pass(tgt, enc_out, bias, PD, H)
  loss = ot.padded_xent_smoothing(logits, tgt, float(d["label_smoothing"]))
  loss.backward()
  live = d["src"] != 0
  assert rel(enc_out.detach().numpy()[live], d["enc_out"][live]) < 1e-5
  assert rel(logits.detach().numpy(), d["logits"]) < 1e-5
  assert abs(float(loss.detach()) - float(d["loss"])) < 1e-5 * abs(float(d["loss"]))
  for n in names:
    rx.check_gradient(d, n, leaves[n].grad.numpy(), 1e-4)


def test_oracle_reproduces_the_reference_beam_decode_at_tt_widths():
  """The oracle's beam search over the oracle's decoder returns the reference's top beams exactly (beam 5, alpha 1.0,
  V = 14); at least half of the rows are stable under the generator's perturbations, some end early, some do not."""
  g = _narrow()
  from oracle import beam_search as obs
  from oracle import transformer as ot
  from test_ref_exec_transformer import oracle_params
  d = dict(np.load(os.path.join(REPO, "tests", "golden", "ref_exec_transformer_infer_tt.npz")))
  C = g.BEAM
  B, S, V, D, H, F, NL = C["dims"]
  names = [str(n) for n in d["var_names"]]
  arrays = {n: g.beam_variable(n, tuple(int(v) for v in d["shape/" + n])) for n in names}
  PE, PD, leaves = oracle_params(d, NL, names, arrays=arrays)
  assert sorted(leaves) == sorted(names)
  with torch.no_grad():
    src = torch.from_numpy(d["src"]).long()
    enc_out, bias = ot.encoder(src, PE, H)

    def fn(ids, i, cache):
      tgt = torch.from_numpy(np.concatenate([ids[:, 1:], np.zeros((ids.shape[0], 1), ids.dtype)], 1)).long()
      logits = ot.decoder_pass(tgt, torch.from_numpy(cache["enc"]), torch.from_numpy(cache["bias"]), PD, H)
      return logits[:, i, :].numpy(), cache
    ids, _ = obs.sequence_beam_search(fn, np.zeros(B, np.int32), {"enc": enc_out.numpy(), "bias": bias.numpy()},
                                      V, C["beam"], C["alpha"], S + C["extra"], 1)
  assert np.array_equal(ids[:, 0, 1:], d["ids"]), (ids[:, 0, 1:], d["ids"])
  assert int(d["stable"].sum()) * 2 >= B
  lens = [int((r != 0).sum()) for r in d["ids"]]
  assert min(lens) < max(lens)
