"""Fixture generator for the Transformer's norm_params and regularizer: executes the REFERENCE'S OWN
TransformerEncoder / TransformerDecoder / PaddedCrossEntropyLossWithSmoothing (on the TF stand-in of
make_ref_exec.py) and writes tests/golden/ref_exec_tnorm_*.npz.

    python tests/golden/make_ref_exec_norms.py [--check] [name ...]

(a) train mode, d_model 512, an EQUAL-LENGTH batch (the reference's BatchNorm statistics over B * T_max positions
    are then the device's statistics over the real tokens), one fixture per norm: batch_norm without and with
    center_scale (with its regularizer), layernorm_L1, layernorm_L2 with eps 1e-5. Stored: the loss with and
    without the regularization loss, logits, (norm, seeded projection) of every trainable variable's gradient of
    the data loss, the names of ALL global variables, and the moving statistics after the step's UPDATE_OPS.
(b) batch_norm in infer mode on a RAGGED batch with non-trivial moving statistics loaded: the beam-search ids on the
    beam fixture's variables, with the rows that survive 2^-7 perturbations of every matrix marked `stable`, and
    the encoder output on those and on the train fixtures' moderate seeded_array variables.
"""
import argparse
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_exec as gen  # noqa: E402

DIMS = (3, 9, 9, 90, 512, 8, 1024, 2)      # B, S, T, V, D, H, F, layers
NORMS = {
    "bn": dict(type="batch_norm", momentum=0.95, epsilon=1e-5, center_scale=False),
    "bn_cs": dict(type="batch_norm", momentum=0.95, epsilon=1e-5, center_scale=True, regularizer="l2",
                  regularizer_params={"scale": 0.002}),    # not the encoder's 0.001: which scale reaches gamma / beta
    "l1": dict(type="layernorm_L1", epsilon=1e-6),
    "l2_eps": dict(type="layernorm_L2", epsilon=1e-5),
}
REG_SCALE = {"bn": 0.0, "bn_cs": 0.001, "l1": 0.0, "l2_eps": 0.0}   # the encoder's / decoder's l2_regularizer
SEED = {"bn": 41, "bn_cs": 43, "l1": 47, "l2_eps": 53}


def moving_value(name, shape, seed):
  """Non-trivial moving statistics for the infer fixture: mean 0.3 N(0, 1), variance exp(0.5 N(0, 1))."""
  rs = np.random.RandomState((zlib.crc32(("moving/" + name).encode()) + seed) % (2 ** 31))
  x = rs.standard_normal(shape).astype(np.float32)
  return np.exp(np.float32(0.5) * x) if name.endswith("moving_variance") else np.float32(0.3) * x


def _norm_params(tf, key):
  p = dict(NORMS[key])
  if p.get("regularizer") == "l2":
    p["regularizer"] = tf.contrib.layers.l2_regularizer
  return p


def train(key):
  tf, imp = gen._install()
  tf.reset_default_graph()
  seed = SEED[key]
  tf.set_random_seed(seed)
  TransformerEncoder = imp("open_seq2seq.encoders.transformer_encoder").TransformerEncoder
  TransformerDecoder = imp("open_seq2seq.decoders.transformer_decoder").TransformerDecoder
  Loss = imp("open_seq2seq.losses.sequence_loss").PaddedCrossEntropyLossWithSmoothing
  rng = np.random.RandomState(seed)
  B, S, T, V, D, H, F, NL = DIMS
  src_len = np.full(B, S, np.int32)
  tgt_len = np.full(B, T, np.int32)
  src = rng.randint(2, V, size=(B, S)).astype(np.int32)
  tgt = rng.randint(2, V, size=(B, T)).astype(np.int32)
  reg = {}
  if REG_SCALE[key] > 0:
    reg = dict(regularizer=tf.contrib.layers.l2_regularizer, regularizer_params={"scale": REG_SCALE[key]})
  norm = _norm_params(tf, key)
  enc_params = dict(encoder_layers=NL, hidden_size=D, num_heads=H, attention_dropout=0.0, filter_size=F,
                    src_vocab_size=V, relu_dropout=0.0, layer_postprocess_dropout=0.0, remove_padding=True,
                    pad_embeddings_2_eight=True, dtype=tf.float32, norm_params=norm, **reg)
  dec_params = dict(EOS_ID=1, layer_postprocess_dropout=0.0, num_hidden_layers=NL, hidden_size=D, num_heads=H,
                    attention_dropout=0.0, relu_dropout=0.0, filter_size=F, batch_size=B, tgt_vocab_size=V,
                    beam_size=4, alpha=0.6, extra_decode_length=5, GO_SYMBOL=1, PAD_SYMBOL=0, END_SYMBOL=1,
                    dtype=tf.float32, norm_params=norm, **reg)
  loss_params = dict(batch_size=B, tgt_vocab_size=V, label_smoothing=0.1, pad_embeddings_2_eight=True,
                     dtype=tf.float32)
  with tf.variable_scope("ForwardPass"):
    encoder = TransformerEncoder(enc_params, None, mode="train")
    decoder = TransformerDecoder(dec_params, None, mode="train")
    loss_fn = Loss(loss_params, None)
    src_t, src_len_t = tf.constant(src), tf.constant(src_len)
    tgt_t, tgt_len_t = tf.constant(tgt), tf.constant(tgt_len)
    enc_out = encoder.encode({"source_tensors": [src_t, src_len_t]})
    dec_out = decoder.decode({"encoder_output": enc_out, "target_tensors": [tgt_t, tgt_len_t]})
    loss = loss_fn.compute_loss({"decoder_output": dec_out, "target_tensors": [tgt_t, tgt_len_t]})
  reg_losses = tf.get_collection(tf.GraphKeys.REGULARIZATION_LOSSES)
  total = loss + tf.add_n(reg_losses) if reg_losses else loss
  tvars = tf.trainable_variables()
  names = [v.name.split(":")[0] for v in tvars]
  gvars = tf.global_variables()
  moving = [v for v in gvars if "moving_" in v.name]
  with tf.Session() as sess:
    for n, v in zip(names, tvars):
      v.load(gen.seeded_array(n, tuple(v._var.shape), seed))
    grads = tf.gradients(loss, tvars)
    vals = sess.run({"logits": dec_out["logits"], "loss": loss, "total": total, "grads": grads})
    sess.run(tf.get_collection(tf.GraphKeys.UPDATE_OPS))
    mv = sess.run(list(moving))
  out = {"src": src, "src_len": src_len, "tgt": tgt, "tgt_len": tgt_len, "logits": vals["logits"],
         "loss": np.float32(vals["loss"]), "loss_total": np.float32(vals["total"]),
         "config": np.array(DIMS, np.int32), "label_smoothing": np.float32(0.1), "var_names": np.array(names),
         "global_names": np.array([v.name.split(":")[0] for v in gvars]), "seed": np.int32(seed),
         "reg_scale": np.float32(REG_SCALE[key]), "moving_names": np.array([v.name.split(":")[0] for v in moving])}
  for v, a in zip(moving, mv):
    out["moving/" + v.name.split(":")[0]] = a.astype(np.float32)
  for n, v, g in zip(names, tvars, vals["grads"]):
    out["shape/" + n] = np.array(tuple(v._var.shape), np.int32)
    out["gproj/" + n] = gen.projection(n, g, seed)
  return out


def canonical(name):
  return name.replace("/batch_normalization_1/", "/batch_normalization/")


BN_INFER = dict(gen.TRANSFORMER_BEAM, seed=59, src_len=[11, 7, 9, 4])


def infer_bn():
  C = BN_INFER
  tf, imp = gen._install()
  tf.reset_default_graph()
  tf.set_random_seed(C["seed"])
  TransformerEncoder = imp("open_seq2seq.encoders.transformer_encoder").TransformerEncoder
  TransformerDecoder = imp("open_seq2seq.decoders.transformer_decoder").TransformerDecoder
  rng = np.random.RandomState(C["seed"])
  B, S, V, D, H, F, NL = C["dims"]
  src_len = np.array(C["src_len"], np.int32)
  src = np.zeros((B, S), np.int32)
  for b in range(B):
    src[b, :src_len[b]] = rng.randint(2, V, size=src_len[b])
  norm = _norm_params(tf, "bn_cs")
  enc_params = dict(encoder_layers=NL, hidden_size=D, num_heads=H, attention_dropout=0.1, filter_size=F,
                    src_vocab_size=V, relu_dropout=0.1, layer_postprocess_dropout=0.1, remove_padding=True,
                    dtype=tf.float32, norm_params=norm)
  dec_params = dict(EOS_ID=1, layer_postprocess_dropout=0.1, num_hidden_layers=NL, hidden_size=D, num_heads=H,
                    attention_dropout=0.1, relu_dropout=0.1, filter_size=F, batch_size=B, tgt_vocab_size=V,
                    beam_size=C["beam"], alpha=0.6, extra_decode_length=C["extra"], GO_SYMBOL=1, PAD_SYMBOL=0,
                    END_SYMBOL=1, dtype=tf.float32, norm_params=norm)
  with tf.variable_scope("ForwardPass"):
    encoder = TransformerEncoder(enc_params, None, mode="infer")
    decoder = TransformerDecoder(dec_params, None, mode="infer")
    enc_out = encoder.encode({"source_tensors": [tf.constant(src), tf.constant(src_len)]})
    dec_out = decoder.decode({"encoder_output": enc_out})
  tvars = tf.trainable_variables()
  names = [v.name.split(":")[0] for v in tvars]
  moving = [v for v in tf.global_variables() if "moving_" in v.name]
  mnames = [v.name.split(":")[0] for v in moving]
  with tf.Session() as sess:
    # the reference's decode step calls each decoder BatchNorm a second time, and tf.layers.batch_normalization
    # creates a second variable set there ('batch_normalization_1'); both sets hold the same values here
    for n, v in zip(mnames, moving):
      v.load(moving_value(canonical(n), tuple(v._var.shape), C["seed"]))
    for n, v in zip(names, tvars):
      v.load(gen.transformer_beam_variable(canonical(n), tuple(v._var.shape), C["seed"]))
    enc, ids = sess.run([enc_out["outputs"], dec_out["outputs"][0]])
    ids = ids.astype(np.int32)
    stable = np.ones(B, np.bool_)
    for k in range(C["perturbations"]):
      for n, v in zip(names, tvars):
        v.load(gen.transformer_beam_variable(canonical(n), tuple(v._var.shape), C["seed"], perturbation=k))
      ids_k = sess.run(dec_out["outputs"][0])
      stable &= np.array([ids_k.shape == ids.shape and np.array_equal(ids_k[b], ids[b]) for b in range(B)])
    # the beam variables' matrices carry gain 3 (a sharp output distribution, near one-hot attention that a bf16 ulp
    # can move): the encoder output is ALSO recorded on the moderate seeded_array variables of the train fixtures
    for n, v in zip(names, tvars):
      v.load(gen.seeded_array(canonical(n), tuple(v._var.shape), C["seed"]))
    enc_seeded = sess.run(enc_out["outputs"])
  enc_rows = np.concatenate([enc[b, :src_len[b]] for b in range(B)], 0).astype(np.float32)
  enc_seeded_rows = np.concatenate([enc_seeded[b, :src_len[b]] for b in range(B)], 0).astype(np.float32)
  out = {"src": src, "src_len": src_len, "enc_out": enc_rows, "enc_out_seeded": enc_seeded_rows, "ids": ids, "stable": stable,
         "var_names": np.array(names), "moving_names": np.array(mnames), "seed": np.int32(C["seed"]),
         "config": np.array(list(C["dims"]) + [C["beam"], C["extra"]], np.int32)}
  for n, v in zip(names, tvars):
    out["shape/" + n] = np.array(tuple(v._var.shape), np.int32)
  return out


GENERATORS = {"tnorm_bn": lambda: train("bn"), "tnorm_bn_cs": lambda: train("bn_cs"),
              "tnorm_l1": lambda: train("l1"), "tnorm_l2_eps": lambda: train("l2_eps"),
              "tnorm_bn_infer": infer_bn}


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
      print("%s: %d arrays, %.1f KB -> %s" % (n, len(out), os.path.getsize(path) / 1e3,
                                             os.path.relpath(path, gen.REPO)))
  return rc


if __name__ == "__main__":
  sys.exit(main())
