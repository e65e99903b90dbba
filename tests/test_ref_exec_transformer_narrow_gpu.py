"""The HIP Transformer path against the REFERENCE'S OWN CODE at widths below Transformer-base, in the mould (and with
the bounds) of tests/test_ref_exec_transformer_gpu.py: logits rel-L2 3e-2, loss 2e-2, every variable's gradient with
cosine > 0.98 and rel-L2 < 0.2 against the oracle's tensors (which reproduce the fixture's to 1e-4), and the stored
(norm, seeded projection) rule at 0.2.

  transformer          d_model 32, 4 heads of 8, V 45 -> 48 (pad_embeddings_2_eight): the fixture that could only be
                       held against the CPU oracle while the kernels took head dim 64 and LayerNorm rows of 512 / 1024
  transformer_tt       the toy-reversal TT config's widths: d_model 128, 8 heads of 16, filter 512, 2 + 2 layers,
                       V = 14 UNPADDED (device table 16 rows, checkpoint variable [14, 128])
  transformer_infer_tt beam search at the same widths, beam 5, alpha 1.0: rows the reference keeps under 2^-7
                       perturbations (`stable`) exactly, at least half of all rows
(tests/golden/make_ref_exec.py, tests/golden/make_ref_exec_narrow.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_exec_util as rx  # noqa: E402

pytestmark = pytest.mark.gpu


def _narrow_gen():
  import importlib.util
  spec = importlib.util.spec_from_file_location("make_ref_exec_narrow",
                                                os.path.join(HERE, "golden", "make_ref_exec_narrow.py"))
  m = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(m)
  return m


@pytest.mark.parametrize("fixture,pad", [("transformer", True), ("transformer_tt", False)])
def test_device_transformer_reproduces_the_reference_code_narrow(cuda, fixture, pad):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders.transformer_encoder import TransformerEncoder
  from openseq2seq_amd.decoders.transformer_decoder import TransformerDecoder
  from openseq2seq_amd.losses.sequence_loss import PaddedCrossEntropyLossWithSmoothing
  from openseq2seq_amd.parts.cnns.conv_blocks import Tape
  from openseq2seq_amd.parts.transformer.layers import SeedSeq
  from openseq2seq_amd.parts.transformer import packing
  from openseq2seq_amd.utils import checkpoint
  d, names = rx.load(fixture)
  B, S, T, V, D, H, F, NL = [int(v) for v in d["config"]]
  padp = {"pad_embeddings_2_eight": True} if pad else {}
  store = FlatParams(cuda)
  enc = TransformerEncoder(dict({"encoder_layers": NL, "hidden_size": D, "num_heads": H, "attention_dropout": 0.0,
                                 "filter_size": F, "src_vocab_size": V, "relu_dropout": 0.0,
                                 "layer_postprocess_dropout": 0.0, "remove_padding": True, "dtype": "mixed"}, **padp),
                           None, mode="train").build(store)
  dec = TransformerDecoder({"EOS_ID": 1, "layer_postprocess_dropout": 0.0, "num_hidden_layers": NL,
                            "hidden_size": D, "num_heads": H, "attention_dropout": 0.0, "relu_dropout": 0.0,
                            "filter_size": F, "batch_size": B, "tgt_vocab_size": V, "beam_size": 4, "alpha": 0.6,
                            "extra_decode_length": 5, "dtype": "mixed"}, None, mode="train").build(store)
  lossf = PaddedCrossEntropyLossWithSmoothing(dict({"label_smoothing": float(d["label_smoothing"]),
                                                    "tgt_vocab_size": V, "batch_size": B, "dtype": "mixed"}, **padp),
                                              None)
  store.finalize(need_m2=False)
  # ---- the reference's variables, by the reference's names -------------------------------------------------
  tf_arrays = rx.variables(d, names)
  used = set()
  for p in store.params:
    a = checkpoint.import_param(p.name, p.shape, p.kind, tf_arrays, getattr(p, "logical_out", None))
    assert a is not None and tuple(a.shape) == tuple(p.shape), (p.name, None if a is None else a.shape, p.shape)
    p.master.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda).view_as(p.master))
    for tf_name, tf_a in checkpoint.export_param(p.name, p.shape, p.kind, a, getattr(p, "logical_out", None)):
      used.add(tf_name)
      assert tuple(tf_a.shape) == tuple(tf_arrays[tf_name].shape), (tf_name, tf_a.shape)     # [14, 128], not [16, 128]
  assert used == set(names), "the device model holds exactly the reference's variables, under the reference's names"
  store.refresh_compute_copies()
  # ---- one forward + backward pass on the packed batch --------------------------------------------------------
  src, sl, tgt, tl = d["src"], d["src_len"], d["tgt"], d["tgt_len"]
  batch = {'source_tensors': [torch.from_numpy(src).to(cuda), torch.from_numpy(sl).to(cuda)],
           'target_tensors': [torch.from_numpy(tgt).to(cuda), torch.from_numpy(tl).to(cuda)],
           'packed_source': packing.to_device(packing.pack_ids(src, sl), cuda),
           'packed_target': packing.to_device(packing.pack_ids(tgt, tl, shift_right=True), cuda)}
  tape = Tape()
  store.zero_grads()
  e = enc.encode({'source_tensors': batch['source_tensors'], 'tape': tape, 'seeds': SeedSeq(1),
                  'packed_source': batch['packed_source']})
  dd = dec.decode({'encoder_output': e, 'target_tensors': batch['target_tensors'], 'tape': tape,
                   'packed_target': batch['packed_target']})
  L = lossf.compute_loss({'decoder_output': dd, 'target_tensors': batch['target_tensors']})
  tape.backward()
  torch.cuda.synchronize()
  # ---- against the reference's numbers ----------------------------------------------------------------------------
  ref_loss = float(d["loss"])
  assert abs(float(L.cpu()[0]) - ref_loss) <= 2e-2 * abs(ref_loss), (float(L.cpu()[0]), ref_loss)
  Vl = d["logits"].shape[-1]                    # the reference's logits width: the logical vocabulary
  lg_all = dd["logits"].float().cpu().numpy()
  assert lg_all.shape[1] == -(-Vl // 8) * 8
  lg = lg_all[:, :Vl]
  ref_rows = np.concatenate([d["logits"][b, :tl[b]] for b in range(B)], 0)
  assert lg.shape == ref_rows.shape, (lg.shape, ref_rows.shape)
  r = rx.rel(lg, ref_rows)
  assert r < 3e-2, r
  from test_ref_exec_transformer import oracle_params
  from oracle import transformer as ot
  PE, PD, leaves = oracle_params(d, NL, names)
  s_ids, t_ids = torch.from_numpy(src).long(), torch.from_numpy(tgt).long()
  o_enc, o_bias = ot.encoder(s_ids, PE, H)
  ot.padded_xent_smoothing(ot.decoder_pass(t_ids, o_enc, o_bias, PD, H), t_ids, float(d["label_smoothing"])).backward()
  worst, worst_cos = 0.0, (1.0, "")
  for p in store.params:
    g = p.grad.detach().float().cpu().numpy()
    if getattr(p, "logical_out", None) is not None:
      assert not g[:, p.logical_out:].any(), "the padding rows of the table take no gradient"
    for tf_name, tf_g in checkpoint.export_param(p.name, p.shape, p.kind, g, getattr(p, "logical_out", None)):
      n = tf_name
      ref = leaves[n].grad.numpy()
      rx.check_gradient(d, n, ref, 1e-4)
      worst = max(worst, rx.check_gradient(d, n, tf_g, 0.2))
      cos = float((tf_g.astype(np.float64) * ref).sum() / (np.linalg.norm(tf_g) * np.linalg.norm(ref) + 1e-30))
      worst_cos = min(worst_cos, (cos, n))
      assert cos > 0.98 and rx.rel(tf_g, ref) < 0.2, (n, cos, rx.rel(tf_g, ref))
  print("%s, device vs the reference's code: loss %.5f vs %.5f, logits rel-L2 %.2e, worst gradient cosine %.4f (%s), "
        "worst projection error %.2e" % (fixture, float(L.cpu()[0]), ref_loss, r, worst_cos[0], worst_cos[1], worst))


def test_device_beam_search_reproduces_the_reference_code_narrow(cuda, tmp_path):
  """TransformerDecoder.predict executed from the reference's files at d_model 128, 8 heads of 16, V 14 unpadded, beam
  5, alpha 1.0 against the HIP beam search, restored from a checkpoint file that holds the reference graph's variables
  under the reference's names and shapes ([14, 128] for the shared embedding)."""
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders.transformer_encoder import TransformerEncoder
  from openseq2seq_amd.decoders.transformer_decoder import TransformerDecoder
  from openseq2seq_amd.utils import checkpoint, tensor_bundle
  g = _narrow_gen()
  d = dict(np.load(os.path.join(HERE, "golden", "ref_exec_transformer_infer_tt.npz")))
  C = g.BEAM
  B, S, V, D, H, F, NL = C["dims"]
  names = [str(n) for n in d["var_names"]]
  arrays = {n: g.beam_variable(n, tuple(int(v) for v in d["shape/" + n])) for n in names}
  assert arrays["ForwardPass/transformer_encoder/embedding_shared_weights/embedding_and_softmax/weights"].shape == (V, D)
  prefix = str(tmp_path / "model.ckpt-0")
  tensor_bundle.write_bundle(prefix, dict(arrays, global_step=np.asarray(0, np.int64)))
  store = FlatParams(cuda)
  enc = TransformerEncoder({"encoder_layers": NL, "hidden_size": D, "num_heads": H, "attention_dropout": 0.1,
                            "filter_size": F, "src_vocab_size": V, "relu_dropout": 0.1,
                            "layer_postprocess_dropout": 0.1, "remove_padding": True, "dtype": "mixed"}, None,
                           mode="infer").build(store)
  dec = TransformerDecoder({"EOS_ID": 1, "layer_postprocess_dropout": 0.1, "num_hidden_layers": NL, "hidden_size": D,
                            "num_heads": H, "attention_dropout": 0.1, "relu_dropout": 0.1, "filter_size": F,
                            "batch_size": B, "tgt_vocab_size": V, "beam_size": C["beam"], "alpha": C["alpha"],
                            "extra_decode_length": C["extra"], "dtype": "mixed"}, None, mode="infer").build(store)
  store.finalize()

  class M(object):
    params = {"dtype": "mixed"}
  M.store = store
  assert checkpoint.load(M(), prefix, restore_optimizer=False, strict=True) == []
  src, sl = torch.from_numpy(d["src"]).to(cuda), torch.from_numpy(d["src_len"]).to(cuda)
  e = enc.encode({"source_tensors": [src, sl]})
  out = dec.decode({"encoder_output": e})
  torch.cuda.synchronize()
  ids = out["outputs"][0].cpu().numpy()
  assert ids.max() < V, "no id from the table's padding rows"
  ref = d["ids"]
  T = max(ids.shape[1], ref.shape[1])
  pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], T - a.shape[1]), a.dtype)], 1)      # noqa: E731
  ids, ref = pad(ids), pad(ref)
  exact = [bool(np.array_equal(ids[b], ref[b])) for b in range(B)]
  print("rows reproduced exactly:", exact, "stable under perturbation:", d["stable"].tolist())
  for b in range(B):
    if not exact[b]:
      print("row", b, "device", ids[b].tolist(), "reference", ref[b].tolist())
    if d["stable"][b]:
      assert exact[b], (b, ids[b].tolist(), ref[b].tolist())
  assert sum(exact) * 2 >= B
