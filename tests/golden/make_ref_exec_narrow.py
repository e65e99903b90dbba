"""Fixture generator at the widths of the reference's toy Transformer configuration (example_configs/text2text/
toy-reversal/nmt-reversal-TT.py): executes the REFERENCE'S OWN TransformerEncoder / TransformerDecoder /
PaddedCrossEntropyLossWithSmoothing (on the TF stand-in of make_ref_exec.py) at d_model 128, 8 heads of 16,
filter 512, 2 + 2 layers and a vocabulary of 14 that is NOT padded to a multiple of 8.

    python tests/golden/make_ref_exec_narrow.py [--check] [name ...]

transformer_tt        train mode, every dropout probability 0, a ragged batch of 3: logits, loss and (norm, seeded
                      projection) of every variable's gradient. Variables come from make_ref_exec.seeded_array.
transformer_infer_tt  infer mode, TransformerDecoder.predict under sequence_beam_search with beam 5, alpha 1.0,
                      extra_decode_length 2: the top beam's ids, and `stable` — the rows whose winner the reference
                      keeps when every matrix is perturbed by 2^-7 relative (six draws), as transformer_infer_d512.
Neither stores a full tensor of variables or gradients.
"""
import argparse
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_exec as gen  # noqa: E402

DIMS = (3, 11, 9, 14, 128, 8, 512, 2)       # B, S, T, V, D, H, F, layers
SEED = 37
BEAM = dict(dims=(6, 11, 14, 128, 8, 512, 2), beam=5, alpha=1.0, extra=2, seed=59, emb_gain=2.0, mat_gain=3.0,
            eos_gain=1.0, perturbations=6, src_len=[11, 7, 9, 4, 10, 6])


def _classes(imp):
  return (imp("open_seq2seq.encoders.transformer_encoder").TransformerEncoder,
          imp("open_seq2seq.decoders.transformer_decoder").TransformerDecoder,
          imp("open_seq2seq.losses.sequence_loss").PaddedCrossEntropyLossWithSmoothing)


def _params(tf, dims, dropout, beam=4, alpha=0.6, extra=5):
  B, V, D, H, F, NL = dims
  enc = dict(encoder_layers=NL, hidden_size=D, num_heads=H, attention_dropout=dropout, filter_size=F,
             src_vocab_size=V, relu_dropout=dropout, layer_postprocess_dropout=dropout, remove_padding=True,
             dtype=tf.float32)                 # no pad_embeddings_2_eight: the table is [14, 128]
  dec = dict(EOS_ID=1, layer_postprocess_dropout=dropout, num_hidden_layers=NL, hidden_size=D, num_heads=H,
             attention_dropout=dropout, relu_dropout=dropout, filter_size=F, batch_size=B, tgt_vocab_size=V,
             beam_size=beam, alpha=alpha, extra_decode_length=extra, GO_SYMBOL=1, PAD_SYMBOL=0, END_SYMBOL=1,
             dtype=tf.float32)
  return enc, dec


def transformer_tt():
  tf, imp = gen._install()
  tf.reset_default_graph()
  tf.set_random_seed(SEED)
  TransformerEncoder, TransformerDecoder, Loss = _classes(imp)
  rng = np.random.RandomState(SEED)
  B, S, T, V, D, H, F, NL = DIMS
  src_len = np.array([11, 7, 4], np.int32)
  tgt_len = np.array([6, 9, 3], np.int32)
  src = np.zeros((B, S), np.int32)
  tgt = np.zeros((B, T), np.int32)
  for b in range(B):
    src[b, :src_len[b]] = rng.randint(2, V, size=src_len[b])
    tgt[b, :tgt_len[b]] = rng.randint(2, V, size=tgt_len[b])
  enc_params, dec_params = _params(tf, (B, V, D, H, F, NL), 0.0)
  loss_params = dict(batch_size=B, tgt_vocab_size=V, label_smoothing=0.1, dtype=tf.float32)
  with tf.variable_scope("ForwardPass"):
    encoder = TransformerEncoder(enc_params, None, mode="train")
    decoder = TransformerDecoder(dec_params, None, mode="train")
    loss_fn = Loss(loss_params, None)
    tgt_t, tgt_len_t = tf.constant(tgt), tf.constant(tgt_len)
    enc_out = encoder.encode({"source_tensors": [tf.constant(src), tf.constant(src_len)]})
    dec_out = decoder.decode({"encoder_output": enc_out, "target_tensors": [tgt_t, tgt_len_t]})
    loss = loss_fn.compute_loss({"decoder_output": dec_out, "target_tensors": [tgt_t, tgt_len_t]})
  tvars = tf.trainable_variables()
  names = [v.name.split(":")[0] for v in tvars]
  with tf.Session() as sess:
    for n, v in zip(names, tvars):
      v.load(gen.seeded_array(n, tuple(v._var.shape), SEED))
    vals = sess.run({"enc": enc_out["outputs"], "bias": enc_out["inputs_attention_bias"], "logits": dec_out["logits"],
                     "loss": loss, "grads": tf.gradients(loss, tvars)})
  out = {"src": src, "src_len": src_len, "tgt": tgt, "tgt_len": tgt_len, "enc_out": vals["enc"],
         "enc_bias": vals["bias"], "logits": vals["logits"], "loss": np.float32(vals["loss"]),
         "config": np.array([B, S, T, V, D, H, F, NL], np.int32), "label_smoothing": np.float32(0.1),
         "var_names": np.array(names), "seed": np.int32(SEED)}
  for n, v, g in zip(names, tvars, vals["grads"]):
    out["shape/" + n] = np.array(tuple(v._var.shape), np.int32)
    out["gproj/" + n] = gen.projection(n, g, SEED)
  return out


def beam_variable(name, shape, perturbation=None):
  """The variable values of the beam-search fixture (the scheme of make_ref_exec.transformer_beam_variable):
  seeded_array, matrices times mat_gain, the EOS row of the shared embedding times eos_gain; perturbation k: every
  matrix entry times 1 + 2^-7 u, u ~ U(-1, 1)."""
  C = BEAM
  a = gen.seeded_array(name, shape, C["seed"])
  if name.endswith("embedding_and_softmax/weights"):
    a = a * np.float32(C["emb_gain"])
    a[1] *= np.float32(C["eos_gain"])
  elif a.ndim == 2:
    a = a * np.float32(C["mat_gain"])
  if a.ndim == 2 and perturbation is not None:
    rs = np.random.RandomState((zlib.crc32(name.encode()) + 1000 * perturbation) % (2 ** 31))
    a = a * (1 + np.float32(2.0 ** -7) * rs.uniform(-1, 1, a.shape).astype(np.float32))
  return a


def transformer_infer_tt():
  C = BEAM
  tf, imp = gen._install()
  tf.reset_default_graph()
  tf.set_random_seed(C["seed"])
  TransformerEncoder, TransformerDecoder, _ = _classes(imp)
  rng = np.random.RandomState(C["seed"])
  B, S, V, D, H, F, NL = C["dims"]
  src_len = np.array(C["src_len"], np.int32)
  src = np.zeros((B, S), np.int32)
  for b in range(B):
    src[b, :src_len[b]] = rng.randint(2, V, size=src_len[b])
  enc_params, dec_params = _params(tf, (B, V, D, H, F, NL), 0.1, C["beam"], C["alpha"], C["extra"])
  with tf.variable_scope("ForwardPass"):
    encoder = TransformerEncoder(enc_params, None, mode="infer")
    decoder = TransformerDecoder(dec_params, None, mode="infer")
    enc_out = encoder.encode({"source_tensors": [tf.constant(src), tf.constant(src_len)]})
    dec_out = decoder.decode({"encoder_output": enc_out})
  gvars = tf.trainable_variables()
  names = [v.name.split(":")[0] for v in gvars]
  with tf.Session() as sess:
    for n, v in zip(names, gvars):
      v.load(beam_variable(n, tuple(v._var.shape)))
    ids = sess.run(dec_out["outputs"][0]).astype(np.int32)
    stable = np.ones(B, np.bool_)
    for k in range(C["perturbations"]):
      for n, v in zip(names, gvars):
        v.load(beam_variable(n, tuple(v._var.shape), perturbation=k))
      ids_k = sess.run(dec_out["outputs"][0])
      stable &= np.array([ids_k.shape == ids.shape and np.array_equal(ids_k[b], ids[b]) for b in range(B)])
  out = {"src": src, "src_len": src_len, "ids": ids, "stable": stable, "var_names": np.array(names)}
  for n, v in zip(names, gvars):
    out["shape/" + n] = np.array(tuple(v._var.shape), np.int32)
  return out


GENERATORS = {"transformer_tt": transformer_tt, "transformer_infer_tt": transformer_infer_tt}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("names", nargs="*", default=sorted(GENERATORS))
  ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed files")
  args = ap.parse_args()
  if not gen.reference_available():
    raise SystemExit("%s not found: fixtures can only be generated where the reference checkout is" % gen.PKG)
  rc = 0
  for n in args.names:
    out = {k: np.asarray(v) for k, v in GENERATORS[n]().items()}
    path = gen.fixture_path(n)
    if args.check:
      bad = gen.compare(out, dict(np.load(path)))
      print("%s: %s" % (n, "reproduced" if not bad else "DIFFERS in %s" % bad))
      rc |= bool(bad)
    else:
      np.savez_compressed(path, **out)
      print("%s: %d arrays, %.1f KB -> %s" % (n, len(out), os.path.getsize(path) / 1e3, os.path.relpath(path, gen.REPO)))
  return rc


if __name__ == "__main__":
  sys.exit(main())
