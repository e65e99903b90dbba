"""Fixture generator of the LSTM language model's text-classification phase: executes the REFERENCE'S OWN
LMEncoder._encode (encoders/lm_encoders.py, fc_dim != vocab_size), WeightDropLayerNormBasicLSTMCell.call and
CrossEntropyLoss (losses/cross_entropy_loss.py) on the TF stand-in of make_ref_exec.py, installed as
make_ref_exec_lm._install_lm does, and writes tests/golden/ref_exec_textcls.npz: data only (ids, lengths, labels,
variables, logits, loss, every gradient, the variable names with their shapes).

    python tests/golden/make_ref_exec_textcls.py [--check]

Two runs of one network, keys prefixed h/ and hc/: use_cell_state False (dense/kernel [8, 3]) and True ([16, 3]).
Train mode, every keep probability 1.0, B = 4, T = 6, V = 17, E = 8, H = 16, 2 layers (widths 16 and 8: weight_tied
makes the last layer emb_size wide, and the embedding is still its own variable in this phase), C = 3, lengths
[6, 1, 4, 3] (the ids past a length are the padding id 1). gamma / beta / bias are loaded away from 1 / 0 so that
a swapped pair shows."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_exec as gen  # noqa: E402
from make_ref_exec_lm import _install_lm  # noqa: E402

DIMS = dict(B=4, T=6, V=17, E=8, H=16, NL=2, C=3)
LENS = (6, 1, 4, 3)
SEED = 211
RUNS = (("h", False), ("hc", True))


def fixture_path():
  return os.path.join(HERE, "ref_exec_textcls.npz")


def run(use_cell_state, seed=SEED):
  tf, imp, Cell = _install_lm()
  tf.reset_default_graph()
  tf.set_random_seed(seed)
  LMEncoder = imp("open_seq2seq.encoders.lm_encoders").LMEncoder
  Loss = imp("open_seq2seq.losses.cross_entropy_loss").CrossEntropyLoss
  rng = np.random.RandomState(seed)
  B, T, V, E, H, NL, C = (DIMS[k] for k in ("B", "T", "V", "E", "H", "NL", "C"))
  lens = np.asarray(LENS, np.int32)
  src = rng.randint(2, V, size=(B, T)).astype(np.int32)
  src[2, 1] = src[0, 3]                      # a repeated token
  src[np.arange(T)[None, :] >= lens[:, None]] = 1
  labels = np.eye(C, dtype=np.int32)[rng.randint(0, C, size=B)]
  enc_params = dict(vocab_size=V, emb_size=E, encoder_layers=NL, encoder_use_skip_connections=False, core_cell=Cell,
                    core_cell_params=dict(num_units=H, forget_bias=1.0), end_token=1, batch_size=B,
                    use_cudnn_rnn=False, cudnn_rnn_type=None, encoder_dp_input_keep_prob=1.0,
                    encoder_dp_output_keep_prob=1.0, encoder_last_input_keep_prob=1.0,
                    encoder_last_output_keep_prob=1.0, recurrent_keep_prob=1.0, encoder_emb_keep_prob=1.0,
                    fc_use_bias=True, weight_tied=True, awd_initializer=False, dtype=tf.float32, fc_dim=C,
                    use_cell_state=use_cell_state,
                    initializer=tf.random_uniform_initializer, initializer_params=dict(minval=-0.5, maxval=0.5))
  with tf.variable_scope("ForwardPass"):
    encoder = LMEncoder(enc_params, None, mode="train")
    loss_fn = Loss(dict(dtype=tf.float32), None)
    src_t, len_t, lab_t = tf.constant(src), tf.constant(lens), tf.constant(labels)
    enc_out = encoder.encode({"source_tensors": [src_t, len_t]})
    loss = loss_fn.compute_loss({"decoder_output": enc_out,
                                 "target_tensors": [lab_t, tf.constant(np.full((B,), C, np.int32))]})
  tvars = tf.trainable_variables()
  names = [v.name.split(":")[0] for v in tvars]
  with tf.Session() as sess:
    for n, v in zip(names, tvars):
      if n.endswith(("/gamma", "/beta", "/bias")):
        v.load(gen._np(v._var) + 0.1 * rng.standard_normal(tuple(v._var.shape)).astype(np.float32))
    grads = tf.gradients(loss, tvars)
    vals = sess.run({"logits": enc_out["logits"], "loss": loss, "grads": grads, "vars": list(tvars)})
  out = {"src": src, "lens": lens, "labels": labels, "logits": np.asarray(vals["logits"], np.float32),
         "loss": np.float32(vals["loss"]), "var_names": np.array(names)}
  for n, v, g in zip(names, vals["vars"], vals["grads"]):
    out["var/" + n] = np.asarray(v, np.float32)
    out["grad/" + n] = np.asarray(g, np.float32)
    out["shape/" + n] = np.array(np.shape(v), np.int32)
  return out


def textcls():
  out = {"config": np.array([DIMS[k] for k in ("B", "T", "V", "E", "H", "NL", "C")], np.int32), "seed": np.int32(SEED)}
  for tag, cell in RUNS:
    for k, v in run(cell).items():
      out["%s/%s" % (tag, k)] = v
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--check", action="store_true", help="re-run and compare with the committed file")
  args = ap.parse_args()
  if not gen.reference_available():
    raise SystemExit("the reference is not present")
  got = textcls()
  if args.check:
    want = dict(np.load(fixture_path()))
    bad = gen.compare(got, want)
    print("textcls: %s" % ("reproduced" if not bad else bad))
    raise SystemExit(1 if bad else 0)
  np.savez_compressed(fixture_path(), **got)
  for tag, _ in RUNS:
    print("wrote %s %s (%d variables, loss %.4f)" % (fixture_path(), tag, len(got[tag + "/var_names"]),
                                                     float(got[tag + "/loss"])))


if __name__ == "__main__":
  main()
