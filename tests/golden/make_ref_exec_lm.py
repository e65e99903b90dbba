"""Fixture generator of the LSTM language model: executes the REFERENCE'S OWN LMEncoder._encode
(encoders/lm_encoders.py), WeightDropLayerNormBasicLSTMCell.call (parts/rnns/weight_drop.py) and BasicSequenceLoss
(losses/sequence_loss.py) on the TF stand-in of make_ref_exec.py and writes tests/golden/ref_exec_lm.npz: data
only (ids, variables, logits, loss, every gradient, the variable names with their shapes).

    python tests/golden/make_ref_exec_lm.py [--check]

lm   train mode, every keep probability 1.0, B = 3, T = 5, V = 17 (no multiple of 8), E = 8, H = 16, 2 layers
     (widths 16 and 8: weight_tied makes the last layer emb_size wide), weight_tied, fc_use_bias, the loss as the
     LM configs set it (offset_target_by_one False, average_across_timestep True, do_mask False). The gamma / beta
     values are loaded away from 1 / 0 so that a swapped pair shows.

Two adjustments to make_ref_exec._install(), both inside this script: its stub of
open_seq2seq.parts.rnns.weight_drop is replaced by the reference's real module, and tf.contrib.layers.layer_norm
is wrapped so that reuse=True is honoured (the stand-in ignores it: the cell creates gamma / beta itself and then
calls layer_norm(reuse=True, scope=name)): the wrapper enters tf.variable_scope(scope, reuse=reuse) and calls the
stand-in's function with scope=tf.get_variable_scope().
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_exec as gen  # noqa: E402

DIMS = dict(B=3, T=5, V=17, E=8, H=16, NL=2)
SEED = 101


def fixture_path(name="lm"):
  return os.path.join(HERE, "ref_exec_%s.npz" % name)


def _install_lm():
  tf, imp = gen._install()
  inner = tf.contrib.layers.layer_norm

  def layer_norm(inputs, reuse=None, scope=None, **kw):
    with tf.variable_scope(scope, reuse=reuse):
      return inner(inputs, reuse=reuse, scope=tf.get_variable_scope(), **kw)

  tf.contrib.layers.layer_norm = layer_norm
  sys.modules.pop("open_seq2seq.parts.rnns.weight_drop", None)
  cell = imp("open_seq2seq.parts.rnns.weight_drop").WeightDropLayerNormBasicLSTMCell
  return tf, imp, cell


def lm(seed=SEED):
  tf, imp, Cell = _install_lm()
  tf.reset_default_graph()
  tf.set_random_seed(seed)
  LMEncoder = imp("open_seq2seq.encoders.lm_encoders").LMEncoder
  Loss = imp("open_seq2seq.losses.sequence_loss").BasicSequenceLoss
  rng = np.random.RandomState(seed)
  B, T, V, E, H, NL = (DIMS[k] for k in ("B", "T", "V", "E", "H", "NL"))
  stream = rng.randint(0, V, size=(B, T + 1)).astype(np.int32)
  stream[1, 2] = stream[0, 1]                # a repeated token
  src, tgt = stream[:, :-1].copy(), stream[:, 1:].copy()
  lens = np.full((B,), T, np.int32)
  enc_params = dict(vocab_size=V, emb_size=E, encoder_layers=NL, encoder_use_skip_connections=False, core_cell=Cell,
                    core_cell_params=dict(num_units=H, forget_bias=1.0), end_token=1, batch_size=B,
                    use_cudnn_rnn=False, cudnn_rnn_type=None, encoder_dp_input_keep_prob=1.0,
                    encoder_dp_output_keep_prob=1.0, encoder_last_input_keep_prob=1.0,
                    encoder_last_output_keep_prob=1.0, recurrent_keep_prob=1.0, encoder_emb_keep_prob=1.0,
                    fc_use_bias=True, weight_tied=True, awd_initializer=False, dtype=tf.float32,
                    initializer=tf.random_uniform_initializer, initializer_params=dict(minval=-0.5, maxval=0.5))
  loss_params = dict(tgt_vocab_size=V, batch_size=B, offset_target_by_one=False, average_across_timestep=True,
                     do_mask=False, dtype=tf.float32)
  with tf.variable_scope("ForwardPass"):
    encoder = LMEncoder(enc_params, None, mode="train")
    loss_fn = Loss(loss_params, None)
    src_t, tgt_t, len_t = tf.constant(src), tf.constant(tgt), tf.constant(lens)
    enc_out = encoder.encode({"source_tensors": [src_t, len_t]})
    loss = loss_fn.compute_loss({"decoder_output": enc_out, "target_tensors": [tgt_t, len_t]})
  tvars = tf.trainable_variables()
  names = [v.name.split(":")[0] for v in tvars]
  with tf.Session() as sess:
    for n, v in zip(names, tvars):
      if n.endswith(("/gamma", "/beta", "/bias")):
        v.load(gen._np(v._var) + 0.1 * rng.standard_normal(tuple(v._var.shape)).astype(np.float32))
    grads = tf.gradients(loss, tvars)
    vals = sess.run({"logits": enc_out["logits"], "loss": loss, "grads": grads, "vars": list(tvars)})
  out = {"src": src, "tgt": tgt, "lens": lens, "logits": vals["logits"].astype(np.float32),
         "loss": np.float32(vals["loss"]), "config": np.array([B, T, V, E, H, NL], np.int32),
         "var_names": np.array(names), "seed": np.int32(seed)}
  for n, v, g in zip(names, vals["vars"], vals["grads"]):
    out["var/" + n] = np.asarray(v, np.float32)
    out["grad/" + n] = np.asarray(g, np.float32)
    out["shape/" + n] = np.array(np.shape(v), np.int32)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--check", action="store_true", help="re-run and compare with the committed file")
  args = ap.parse_args()
  if not gen.reference_available():
    raise SystemExit("the reference is not present")
  got = lm()
  if args.check:
    want = dict(np.load(fixture_path()))
    bad = gen.compare(got, want)
    print("lm: %s" % ("reproduced" if not bad else bad))
    raise SystemExit(1 if bad else 0)
  np.savez_compressed(fixture_path(), **got)
  print("wrote %s (%d variables, loss %.4f)" % (fixture_path(), len(got["var_names"]), float(got["loss"])))


if __name__ == "__main__":
  main()
