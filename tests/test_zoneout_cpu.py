"""CPU tests of zoneout on the Tacotron 2 LSTMs: the oracle's state replacement against the reference's own
ZoneoutWrapper, its gradient split against finite differences and autograd, the conditions on the GPU cases'
inputs, the host rules of Tacotron2Encoder / Tacotron2Decoder and the layout of os2s_rnn_zoneout_t. The oracle
lives in tests/_zoneout_cases.py."""
import ctypes
import os
import subprocess
import sys
import types

import pytest
import torch

import _zoneout_cases as Z
from test_abi_structs import HEADER, REPO, _compiler, _header_fields

REFERENCE = "/root/reference/open_seq2seq/parts/rnns/zoneout.py"


def _report(fails):
  assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ 1. the reference's file
@pytest.mark.skipif(not os.path.exists(REFERENCE), reason="reference checkout not present")
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("training", [True, False])
def test_state_replacement_equals_the_references_zoneout_wrapper(monkeypatch, p, training):
  """parts/rnns/zoneout.py executed where it lies, on stand-ins for its two TensorFlow imports: a minimal
  RNNCell / LSTMStateTuple and a dropout that applies the mask the test supplies (x * mask / keep_prob, what
  tf.nn.dropout computes). Equal to 1e-12 in float64, both branches."""
  class RNNCell(object):
    pass

  class LSTMStateTuple(tuple):
    def __new__(cls, c, h):
      return tuple.__new__(cls, (c, h))

  g = torch.Generator().manual_seed(int(p * 10) + 2 * training)
  B, H = 3, 16
  queue = [(torch.rand(B, H, generator=g) < 1.0 - p).double() for _ in range(2)]      # masks for c, then h
  used = []

  def dropout(x, keep_prob, seed=None):
    m = queue[len(used)]
    used.append(m)
    return x * m / keep_prob

  rnn_cell_impl = types.ModuleType("tensorflow.python.ops.rnn_cell_impl")
  rnn_cell_impl.RNNCell, rnn_cell_impl.LSTMStateTuple = RNNCell, LSTMStateTuple
  nn_ops = types.ModuleType("tensorflow.python.ops.nn_ops")
  nn_ops.dropout = dropout
  ops = types.ModuleType("tensorflow.python.ops")
  ops.rnn_cell_impl, ops.nn_ops = rnn_cell_impl, nn_ops
  python = types.ModuleType("tensorflow.python")
  python.ops = ops
  tf = types.ModuleType("tensorflow")
  tf.python = python
  for name, mod in (("tensorflow", tf), ("tensorflow.python", python), ("tensorflow.python.ops", ops),
                    ("tensorflow.python.ops.rnn_cell_impl", rnn_cell_impl), ("tensorflow.python.ops.nn_ops", nn_ops)):
    monkeypatch.setitem(sys.modules, name, mod)
  ns = {"__name__": "reference_zoneout"}
  exec(compile(open(REFERENCE).read(), REFERENCE, "exec"), ns)

  new_c, new_h, old_c, old_h, out = (torch.randn(B, H, generator=g, dtype=torch.float64) for _ in range(5))

  class Cell(RNNCell):
    state_size = (H, H)
    output_size = H

    def __call__(self, inputs, state, scope=None):
      return out, LSTMStateTuple(new_c, new_h)

  wrapped = ns["ZoneoutWrapper"](Cell(), p, is_training=training)
  got_out, (got_c, got_h) = wrapped(None, LSTMStateTuple(old_c, old_h))
  assert got_out is out                       # the output is the wrapped cell's, untouched
  assert len(used) == (2 if training else 0)
  zo = dict(mode=Z.SAMPLE if training else Z.BLEND, p=p)
  want_c = Z.zoneout_state(new_c, old_c, zo, queue[0])
  want_h = Z.zoneout_state(new_h, old_h, zo, queue[1])
  assert float((got_c - want_c).abs().max()) <= 1e-12 and float((got_h - want_h).abs().max()) <= 1e-12
  assert float((got_c - new_c).abs().max()) > 1e-3      # the case replaces something


# ------------------------------------------------------------------------------------------ off = the parent's oracles
def test_decoder_oracle_without_zoneout_is_the_parents_cpu():
  """attention_decoder_zo with zoneout off against oad.attention_decoder on the same leaves: outputs and every
  gradient bit for bit; dec_reference(OFF) is that run."""
  for name in ("zo_ragged", "zo_h8"):
    case = Z.DEC_CASES[name][0]
    d = Z.dec_inputs(name)
    mode = Z.adc.MODES[case[7]]

    def run(fn, *zo):
      leaf = lambda t: None if t is None else t.double().clone().requires_grad_(True)
      P = dict(wcat=[leaf(w) for w in d["wcat"]], bias=[leaf(b) for b in d["bias"]], wq=leaf(d["wq"]), wmem=None,
               v=leaf(d["v"]), g=leaf(d["g"]), b=leaf(d["b"]), conv_w=leaf(d["conv_w"]), conv_b=leaf(d["conv_b"]),
               dense_w=leaf(d["dense_w"]))
      gx0, vals, keys = leaf(d["gx0"]), leaf(d["values"]), leaf(d["keys"])
      out = fn(P, gx0, d["values"].double(), d["src_len"], d["tgt_len"], *zo, 1.0, mode, keys_override=keys,
               values_override=vals)
      ((out["y"] * d["dy"].double()).sum() + (out["ctx"] * d["dctx"].double()).sum()).backward()
      leaves = [gx0, vals, keys] + P["wcat"] + [t for t in (P["wq"], P["v"], P["conv_w"], P["dense_w"]) if t is not None]
      return out, [t.grad for t in leaves]

    want, gwant = run(Z.oad.attention_decoder, None, None)
    for zo in (None, dict(mode=Z.OFF, p=0.5)):
      got, ggot = run(Z.attention_decoder_zo, zo)
      for q in ("y", "ctx", "align"):
        assert torch.equal(got[q], want[q]), (name, q)
      assert all(torch.equal(a, b) for a, b in zip(ggot, gwant)), name
    R = Z.dec_reference(name, Z.OFF)
    assert torch.equal(R["y"], want["y"].detach()) and torch.equal(R["grads"]["dg0"], gwant[0])


@pytest.mark.parametrize("reverse", [False, True])
def test_rnn_oracle_without_zoneout_is_the_parents_cpu(reverse):
  g = torch.Generator().manual_seed(5)
  B, T, In, H = 4, 5, 6, 8
  x = torch.randn(B, T, In, generator=g, dtype=torch.float64)
  wx, wh = torch.randn(In, 4 * H, generator=g, dtype=torch.float64), torch.randn(H, 4 * H, generator=g, dtype=torch.float64) * 0.3
  bias = torch.randn(4 * H, generator=g, dtype=torch.float64) * 0.1
  lens = torch.tensor([5, 1, 3, 4])
  want = Z.orn.lstm_tf(x, lens, wx, wh, bias, 1.0, reverse)
  got = Z.lstm_tf_zo(x, lens, wx, wh, bias, 1.0, reverse, None)
  assert torch.equal(got["y"], want)
  assert torch.equal(got["h_seq"], want) and torch.equal(got["c_seq"], got["c_new"])
  # and the hand-written backward without masks is rc.backward_oracle's
  dy = torch.randn(B, T, H, generator=g, dtype=torch.float64)
  whk = wh.t().contiguous()
  a = Z.lstm_tf_zo_bwd(got["gates"], got["c_seq"], dy, whk, lens, reverse)
  b = Z.rc.backward_oracle(Z.rc.LSTM_TF, got["gates"], got["c_seq"], got["y"], dy, whk, lens, reverse)["dgx"]
  assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ 2. the gradient split
def test_zoneout_gradient_split_against_finite_differences():
  """Two steps of an H = 4 cell in float64: autograd through m new + (1 - m) old (what the decoder oracle
  differentiates) against central finite differences."""
  g = torch.Generator().manual_seed(11)
  B, T, H = 2, 2, 4
  mk = lambda: (torch.rand(B, T, H, generator=g) < 0.5).double()
  zo = dict(mode=Z.SAMPLE, p=0.5, mh=mk(), mc=mk())
  assert 0 < float(zo["mh"].sum()) < B * T * H and 0 < float(zo["mc"].sum()) < B * T * H
  w = (torch.randn(4 * H, 2 * H, generator=g, dtype=torch.float64) * 0.5).requires_grad_(True)
  x = torch.randn(B, T, H, generator=g, dtype=torch.float64).requires_grad_(True)
  h0 = torch.randn(B, H, generator=g, dtype=torch.float64).requires_grad_(True)
  c0 = torch.randn(B, H, generator=g, dtype=torch.float64).requires_grad_(True)

  def f(w, x, h0, c0):
    h, c, outs = h0, c0, []
    for t in range(T):
      hn, cn = Z.oad.lstm_cell(torch.cat([x[:, t], h], -1), c, w, None, 1.0)
      h = Z.zoneout_state(hn, h, zo, zo["mh"][:, t])
      c = Z.zoneout_state(cn, c, zo, zo["mc"][:, t])
      outs.append(hn)
    return torch.stack(outs + [h, c], 1)       # outputs and the final state

  assert torch.autograd.gradcheck(f, (w, x, h0, c0), eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("reverse", [False, True])
def test_rnn_backward_oracle_equals_autograd(reverse):
  """The hand-written m / 1 - m split of lstm_tf_zo_bwd (the form the kernels implement, teacher-forced on the
  saved gates and the zoned c_seq, c_new recomputed where m_c zoned it) against autograd through lstm_tf_zo."""
  g = torch.Generator().manual_seed(13)
  B, T, H = 3, 4, 4
  lens = torch.tensor([4, 1, 3])
  mk = lambda: (torch.rand(B, T, H, generator=g) < 0.5).double()
  zo = dict(mode=Z.SAMPLE, p=0.5, mh=mk(), mc=mk())
  gx = torch.randn(B, T, 4 * H, generator=g, dtype=torch.float64).requires_grad_(True)
  wh = (torch.randn(H, 4 * H, generator=g, dtype=torch.float64) * 0.5).requires_grad_(True)
  eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, dtype=torch.float64)
  out = Z.lstm_tf_zo(gx, lens, eye, wh, zero, 1.0, reverse, zo)
  dy = torch.randn(B, T, H, generator=g, dtype=torch.float64)
  out["y"].backward(dy)
  got = Z.lstm_tf_zo_bwd(out["gates"].detach(), out["c_seq"].detach(), dy, wh.detach().t().contiguous(), lens, reverse, zo)
  assert float((got - gx.grad).abs().max()) <= 1e-12
  # dWh = dg^T . (the zoned state one step earlier in processing order): h_seq, not y
  hs = out["h_seq"].detach()
  z = torch.zeros(B, 1, H, dtype=torch.float64)
  hprev = torch.cat([hs[:, 1:], z], 1) if reverse else torch.cat([z, hs[:, :-1]], 1)
  dwh = torch.einsum("btg,bth->hg", got, hprev)
  assert float((dwh - wh.grad).abs().max()) <= 1e-12
  ys = out["y"].detach()
  yprev = torch.cat([ys[:, 1:], z], 1) if reverse else torch.cat([z, ys[:, :-1]], 1)
  assert float((torch.einsum("btg,bth->hg", got, yprev) - wh.grad).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------ the GPU cases' inputs
@pytest.mark.parametrize("name", sorted(Z.DEC_CASES))
def test_decoder_case_conditions_cpu(name):
  """The conditions of _attn_decoder_cases.check_inputs on the zoneout oracle, the mask conditions, and y moved
  by zoneout (the masks are the library's: hash_mask, held to it by the GPU tests)."""
  with Z.registered():
    fails = Z.adc.check_inputs(name, Z.dec_reference(name, Z.SAMPLE))
  _report(fails + Z.dec_conditions(name))


def test_decoder_case_table_reaches_the_kernels_it_names():
  """The host predicates, restated: which forward / backward cell kernel a case takes."""
  for name, (case, p, tgt, _, option) in Z.DEC_CASES.items():
    B, T, S, L, H, M, U, mode = case[:8]
    fast = tgt is None and mode == 2 and B <= 32 and H % 64 == 0 and M % 64 == 0
    assert fast == (name in ("zo_b32_fast", "zo_t1")), name
    assert (option == "attn_decoder.cell_split") == (name == "zo_b33")
    assert T >= 3 or name == "zo_t1"
  assert Z.DEC_CASES["zo_h72"][0][4] % 64 != 0 and Z.DEC_CASES["zo_h8"][0][4] == 8


@pytest.mark.parametrize("name", sorted(Z.RNN_CASES))
def test_rnn_case_conditions_cpu(name):
  live = Z.rnn_live(name)
  fails = []
  for d, m in enumerate(Z.rnn_masks(name)):
    fails += Z.mask_conditions([m["mh"], m["mc"]], live, Z.RNN_P[Z.SAMPLE], "%s dir %d" % (name, d))
  on, off = Z.rnn_forward_ref(name, Z.SAMPLE, False), Z.rnn_forward_ref(name, Z.OFF, False)
  nq = Z.rc.noise_floor()[Z.rc.LSTM_TF]["y"]
  for d in range(2):
    moved = (on[d]["y"] - off[d]["y"]).abs() > 10.0 * (4.0 * nq + 2.0 ** -7 * off[d]["y"].abs())
    if not bool(moved.any()):
      fails.append("%s dir %d: zoneout moves no element of y by ten bounds" % (name, d))
  # true-t mask indexing differs from processing-order indexing on the reverse direction of a short sample
  lens = Z.rnn_inputs(name)["lens"]
  assert int(lens.min()) < Z.RNN_CASES[name][1]
  _report(fails)


# ------------------------------------------------------------------------------------------ 3. host rules
POST = [{"kernel_size": [5], "stride": [1], "num_channels": -1, "padding": "SAME", "activation_fn": None}]


def _dec_params(**kw):
  p = {"attention_layer_size": 128, "attention_type": "location", "decoder_cell_units": 64,
       "decoder_cell_type": "LSTMCell", "decoder_layers": 2, "enable_prenet": True, "prenet_layers": 2,
       "prenet_units": 64, "enable_postnet": True, "postnet_conv_layers": POST, "dtype": "mixed"}
  p.update(kw)
  return p


def _enc_params(**kw):
  p = {"cnn_dropout_prob": 0.0, "rnn_dropout_prob": 0.0, "src_emb_size": 64,
       "conv_layers": [{"kernel_size": [5], "stride": [1], "num_channels": 64, "padding": "SAME"}],
       "activation_fn": "relu", "num_rnn_layers": 1, "rnn_cell_dim": 32, "use_cudnn_rnn": False,
       "rnn_type": "LSTMCell", "rnn_unidirectional": False, "dtype": "mixed"}
  p.update(kw)
  return p


def test_both_classes_construct_with_zoneout():
  from openseq2seq_amd.decoders import Tacotron2Decoder
  from openseq2seq_amd.encoders import Tacotron2Encoder
  for mode in ("train", "eval", "infer"):
    Tacotron2Decoder(_dec_params(zoneout_prob=0.1, dropout_prob=0.), None, mode=mode)
    Tacotron2Encoder(_enc_params(zoneout_prob=0.1), None, mode=mode)


def test_zoneout_value_errors():
  from openseq2seq_amd.decoders import Tacotron2Decoder
  from openseq2seq_amd.encoders import Tacotron2Encoder
  for bad in (-0.1, 1.0, 1.5):
    with pytest.raises(ValueError):
      Tacotron2Decoder(_dec_params(zoneout_prob=bad, dropout_prob=0.), None, mode="train")
    with pytest.raises(ValueError):
      Tacotron2Encoder(_enc_params(zoneout_prob=bad), None, mode="train")
  with pytest.raises(ValueError):       # zoneout next to output dropout
    Tacotron2Decoder(_dec_params(zoneout_prob=0.1, dropout_prob=0.1), None, mode="train")
  with pytest.raises(ValueError):       # ... which is the default
    Tacotron2Decoder(_dec_params(zoneout_prob=0.1), None, mode="train")
  for mode in ("train", "eval"):        # the cuDNN classes have no zoneout
    with pytest.raises(ValueError):
      Tacotron2Encoder(_enc_params(zoneout_prob=0.1, use_cudnn_rnn=True, rnn_type="CudnnLSTM"), None, mode=mode)
  enc = Tacotron2Encoder(_enc_params(zoneout_prob=0.1, use_cudnn_rnn=True, rnn_type="CudnnLSTM"), None, mode="infer")
  assert enc._zoneout == 0.0            # ignored in infer, as the reference's compatible cells ignore it


def test_other_guards_and_the_schema_stay():
  from openseq2seq_amd.decoders import Tacotron2Decoder
  from openseq2seq_amd.encoders import Tacotron2Encoder
  with pytest.raises(NotImplementedError):
    Tacotron2Decoder(_dec_params(zoneout_prob=0.1, dropout_prob=0., decoder_layers=3), None, mode="train")
  with pytest.raises(NotImplementedError):
    Tacotron2Encoder(_enc_params(zoneout_prob=0.1, rnn_unidirectional=True), None, mode="train")
  with pytest.raises(Exception) as e:
    Tacotron2Decoder(_dec_params(zoneout_probability=0.1), None, mode="train")
  assert not isinstance(e.value, NotImplementedError) and "zoneout_probability" in str(e.value)
  with pytest.raises(Exception) as e:
    Tacotron2Encoder(_enc_params(zoneout=0.1), None, mode="train")
  assert "zoneout" in str(e.value)


# ------------------------------------------------------------------------------------------ 4. struct layout
def test_rnn_zoneout_struct_mirror_matches_the_header(tmp_path):
  """os2s_rnn_zoneout_t against capi._RnnZoneout, the way tests/test_abi_structs.py checks the other structs."""
  from openseq2seq_amd import capi
  t, S = "os2s_rnn_zoneout_t", capi._RnnZoneout
  names = _header_fields(t)
  lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "os2s.h"', "int main(void) {",
           '  printf("sizeof %%zu\\n", sizeof(%s));' % t]
  lines += ['  printf("%s %%zu\\n", offsetof(%s, %s));' % (n, t, n) for n in names]
  lines += ["  return 0;", "}"]
  src, exe = tmp_path / "layout.c", tmp_path / "layout"
  src.write_text("\n".join(lines) + "\n")
  subprocess.run([_compiler(), "-std=c99", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
  c = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
  assert [f[0] for f in S._fields_] == names
  assert ctypes.sizeof(S) == int(c["sizeof"])
  for n in names:
    assert getattr(S, n).offset == int(c[n]), n
  assert REPO
