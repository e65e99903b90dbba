"""Shared by tests/test_transformer_long_e2e_gpu.py: a small Transformer, a batch with GIVEN sentence lengths, and
the forward + backward comparison against the CPU fp32 oracle (oracle/transformer.py, padded [B, L] like the
reference) that tests/test_transformer_e2e_gpu.py runs on short sentences."""
import numpy as np
import torch


def build(cuda, dims, dropout=0.0):
  D, H, F, V, NL = dims
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders.transformer_encoder import TransformerEncoder
  from openseq2seq_amd.decoders.transformer_decoder import TransformerDecoder
  from openseq2seq_amd.losses.sequence_loss import PaddedCrossEntropyLossWithSmoothing
  torch.manual_seed(0)
  store = FlatParams(cuda)
  enc = TransformerEncoder({"encoder_layers": NL, "hidden_size": D, "num_heads": H,
                            "attention_dropout": dropout, "filter_size": F, "src_vocab_size": V,
                            "relu_dropout": dropout, "layer_postprocess_dropout": dropout,
                            "remove_padding": True, "dtype": "mixed"}, None, mode="train").build(store)
  dec = TransformerDecoder({"EOS_ID": 1, "layer_postprocess_dropout": dropout,
                            "num_hidden_layers": NL, "hidden_size": D, "num_heads": H,
                            "attention_dropout": dropout, "relu_dropout": dropout,
                            "filter_size": F, "batch_size": 4, "tgt_vocab_size": V, "beam_size": 4,
                            "alpha": 0.6, "extra_decode_length": 50, "dtype": "mixed"}, None,
                           mode="train").build(store)
  loss = PaddedCrossEntropyLossWithSmoothing({"label_smoothing": 0.1, "tgt_vocab_size": V,
                                              "batch_size": 4, "dtype": "mixed"}, None)
  store.finalize(need_m2=True)
  return store, enc, dec, loss


def batch_of(cuda, src_lens, tgt_lens, V, seed=1):
  """Random token ids (EOS = 1 last) for the given sentence lengths: (batch dict, src, sl, tgt, tl)."""
  from openseq2seq_amd.parts.transformer import packing
  rng = np.random.RandomState(seed)

  def draw(lens):
    lens = np.asarray(lens, np.int32)
    ids = np.zeros((len(lens), int(lens.max())), np.int32)
    for b in range(len(lens)):
      ids[b, :lens[b] - 1] = rng.randint(4, V, size=lens[b] - 1)
      ids[b, lens[b] - 1] = 1
    return ids, lens
  src, sl = draw(src_lens)
  tgt, tl = draw(tgt_lens)
  batch = {'source_tensors': [torch.from_numpy(src).to(cuda), torch.from_numpy(sl).to(cuda)],
           'target_tensors': [torch.from_numpy(tgt).to(cuda), torch.from_numpy(tl).to(cuda)],
           'packed_source': packing.to_device(packing.pack_ids(src, sl), cuda),
           'packed_target': packing.to_device(packing.pack_ids(tgt, tl, shift_right=True), cuda)}
  return batch, src, sl, tgt, tl


def oracle_params(store, dims):
  """Device parameters (bf16 compute copies for matrices) -> oracle dicts with autograd, and the leaves by name."""
  D, H, F, V, NL = dims

  def w(name):   # Dense kernel [1,Cout,Cin] -> [Cin,Cout]
    return store.by_name(name + "/kernel").w16.float().cpu()[0].t().contiguous().requires_grad_(True)

  def v(name):
    return store.by_name(name).master.cpu().clone().requires_grad_(True)

  leaves = {}

  def ln(prefix):
    d = {"scale": v(prefix + "/layer_norm_scale"), "bias": v(prefix + "/layer_norm_bias")}
    leaves[prefix + "/layer_norm_scale"] = d["scale"]
    leaves[prefix + "/layer_norm_bias"] = d["bias"]
    return d

  def att_self(prefix):
    qkv = w(prefix + "/qkv")
    leaves[prefix + "/qkv/kernel"] = qkv
    o = w(prefix + "/output_transform")
    leaves[prefix + "/output_transform/kernel"] = o
    return {"q": qkv[:, :D], "k": qkv[:, D:2 * D], "v": qkv[:, 2 * D:], "o": o}

  def att_cross(prefix):
    q, kv, o = w(prefix + "/q"), w(prefix + "/kv"), w(prefix + "/output_transform")
    leaves[prefix + "/q/kernel"], leaves[prefix + "/kv/kernel"] = q, kv
    leaves[prefix + "/output_transform/kernel"] = o
    return {"q": q, "k": kv[:, :D], "v": kv[:, D:], "o": o}

  def ffn(prefix):
    d = {"w1": w(prefix + "/filter_layer"), "b1": v(prefix + "/filter_layer/bias"),
         "w2": w(prefix + "/output_layer"), "b2": v(prefix + "/output_layer/bias")}
    leaves[prefix + "/filter_layer/kernel"], leaves[prefix + "/filter_layer/bias"] = d["w1"], d["b1"]
    leaves[prefix + "/output_layer/kernel"], leaves[prefix + "/output_layer/bias"] = d["w2"], d["b2"]
    return d

  shared = "ForwardPass/transformer_encoder/embedding_shared_weights/embedding_and_softmax/weights"
  emb = store.by_name(shared).w16.float().cpu()[0].clone().requires_grad_(True)
  leaves[shared] = emb
  e, dc = "ForwardPass/transformer_encoder", "ForwardPass/transformer_decoder"
  PE = {"emb": emb, "layers": [], "ln_out": ln(e + "/layer_normalization")}
  PD = {"emb": emb, "layers": [], "ln_out": ln(dc + "/layer_normalization")}
  for n in range(NL):
    ls = "%s/layer_%d" % (e, n)
    PE["layers"].append({"ln1": ln(ls + "/self_attention/layer_normalization"),
                         "att": att_self(ls + "/self_attention/self_attention"),
                         "ln2": ln(ls + "/ffn/layer_normalization"),
                         "ffn": ffn(ls + "/ffn/feed_foward_network")})
    ls = "%s/layer_%d" % (dc, n)
    PD["layers"].append({"ln1": ln(ls + "/self_attention/layer_normalization"),
                         "self": att_self(ls + "/self_attention/self_attention"),
                         "ln2": ln(ls + "/encdec_attention/layer_normalization"),
                         "cross": att_cross(ls + "/encdec_attention/attention"),
                         "ln3": ln(ls + "/ffn/layer_normalization"),
                         "ffn": ffn(ls + "/ffn/feed_foward_network")})
  return PE, PD, leaves


def fwd_bwd(cuda, dims, src_lens, tgt_lens, tol):
  """One training forward + backward at dropout 0 on the device (packed tokens) and in the oracle (padded): the
  loss, the logits at the non-pad positions and every parameter gradient within `tol`."""
  D, H, F, V, NL = dims
  from openseq2seq_amd.parts.cnns.conv_blocks import Tape
  from openseq2seq_amd.parts.transformer.layers import SeedSeq
  from oracle import transformer as ot
  store, enc, dec, lossf = build(cuda, dims)
  batch, src, sl, tgt, tl = batch_of(cuda, src_lens, tgt_lens, V)
  tape = Tape()
  store.zero_grads()
  e = enc.encode({'source_tensors': batch['source_tensors'], 'tape': tape, 'seeds': SeedSeq(1),
                  'packed_source': batch['packed_source']})
  d = dec.decode({'encoder_output': e, 'target_tensors': batch['target_tensors'], 'tape': tape,
                  'packed_target': batch['packed_target']})
  L = lossf.compute_loss({'decoder_output': d, 'target_tensors': batch['target_tensors']})
  tape.backward()
  torch.cuda.synchronize()
  PE, PD, leaves = oracle_params(store, dims)
  s_ids, t_ids = torch.from_numpy(src).long(), torch.from_numpy(tgt).long()
  enc_out, bias = ot.encoder(s_ids, PE, H)
  logits = ot.decoder_pass(t_ids, enc_out, bias, PD, H)
  loss = ot.padded_xent_smoothing(logits, t_ids, 0.1)
  loss.backward()
  torch.testing.assert_close(L.cpu()[0], loss.detach(), rtol=tol["loss"], atol=tol["loss"])
  lg = d["logits"].float().cpu()
  ref_rows = torch.cat([logits[b, :tl[b]] for b in range(len(tl))], 0).detach()
  rel = float((lg - ref_rows).norm() / ref_rows.norm())
  assert rel < tol["logits"], rel
  worst = (1.0, "")
  for name, leaf in leaves.items():
    got = store.by_name(name).grad.cpu()
    ref = leaf.grad
    if name.endswith("/kernel"):
      ref = ref.t()[None]
    elif name.endswith("weights"):
      ref = ref[None]
    cos = float(torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0))
    relerr = float((got - ref).norm() / (ref.norm() + 1e-12))
    worst = min(worst, (cos, name))
    assert cos > tol["cos"], (name, cos, relerr)
    assert relerr < tol["rel"], (name, cos, relerr)
  print("worst cosine", worst, "logits rel", rel)
