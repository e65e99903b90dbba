"""CPU: the Transformer's norm_params (parts/transformer/common.py:11-106) and regularizer
(encoders/transformer_encoder.py:71-75, decoders/transformer_decoder.py:80-84) on the host side — every norm type
constructs, under the reference's variable names; the l2 scale reaches exactly the variables the reference
regularises; the reference's example configs that set them load and construct; the norm fixtures reproduce.

The l2 scales pinned here are the fp32 semantics of the reference (tf.contrib.layers.l2_regularizer on each
variable). Under dtype "mixed" the same per-variable scale is applied to the fp32 master copy by the optimizer
(FlatParams.tensor_l2, as for the conv layers; optimizers/mp_wrapper.py:58-90), which the fp32 fixtures cannot pin."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "example_configs")),
                               reason="reference checkout not present")

NORMS = {
    "layernorm_L2_eps": {"type": "layernorm_L2", "epsilon": 1e-5},
    "layernorm_L1": {"type": "layernorm_L1"},
    "batch_norm": {"type": "batch_norm", "momentum": 0.95, "epsilon": 1e-5, "center_scale": False},
    "batch_norm_cs": {"type": "batch_norm", "momentum": 0.95, "epsilon": 1e-5, "center_scale": True,
                      "regularizer": "l2", "regularizer_params": {"scale": 0.002}},
}
BN = "transformer__batch_norm/batch_normalization"


def _l2_regularizer(scale):      # stands for tf.contrib.layers.l2_regularizer: only "not None" is read
  return scale


def _build(norm_params, regularizer=None, mode="train", D=512, NL=2):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders.transformer_encoder import TransformerEncoder
  from openseq2seq_amd.decoders.transformer_decoder import TransformerDecoder
  extra = {}
  if norm_params is not None:
    extra["norm_params"] = norm_params
  if regularizer is not None:
    extra.update(regularizer=_l2_regularizer, regularizer_params={"scale": regularizer})
  store = FlatParams(torch.device("cpu"))
  enc = TransformerEncoder(dict({"encoder_layers": NL, "hidden_size": D, "num_heads": D // 64,
                                 "attention_dropout": 0.1, "filter_size": 2 * D, "src_vocab_size": 96,
                                 "relu_dropout": 0.1, "layer_postprocess_dropout": 0.1, "remove_padding": True},
                                **extra), None, mode=mode).build(store)
  dec = TransformerDecoder(dict({"EOS_ID": 1, "layer_postprocess_dropout": 0.1, "num_hidden_layers": NL,
                                 "hidden_size": D, "num_heads": D // 64, "attention_dropout": 0.1,
                                 "relu_dropout": 0.1, "filter_size": 2 * D, "batch_size": 2, "tgt_vocab_size": 96,
                                 "beam_size": 2, "alpha": 0.6, "extra_decode_length": 2}, **extra),
                           None, mode=mode).build(store)
  return store, enc, dec


def _norm_scopes(NL=2):
  out = []
  for n in range(NL):
    out += ["ForwardPass/transformer_encoder/layer_%d/%s" % (n, s) for s in ("self_attention", "ffn")]
    out += ["ForwardPass/transformer_decoder/layer_%d/%s" % (n, s)
            for s in ("self_attention", "encdec_attention", "ffn")]
  return out + ["ForwardPass/transformer_encoder", "ForwardPass/transformer_decoder"]


@pytest.mark.parametrize("kind", sorted(NORMS))
def test_every_norm_type_constructs_under_the_reference_names(kind):
  from openseq2seq_amd.parts.transformer import layers as L
  norm = NORMS[kind]
  store, enc, dec = _build(norm)
  names = {p.name for p in store.params}
  scopes = _norm_scopes()
  for s in scopes:
    if norm["type"] == "batch_norm":
      assert s + "/" + BN + "/moving_mean" in store.state and s + "/" + BN + "/moving_variance" in store.state
      has = norm["center_scale"]
      assert (s + "/" + BN + "/gamma" in names) == has and (s + "/" + BN + "/beta" in names) == has
      assert not any(n.startswith(s + "/layer_normalization/") for n in names)
    else:
      assert s + "/layer_normalization/layer_norm_scale" in names
      assert s + "/layer_normalization/layer_norm_bias" in names
      assert not store.state
  norms = [enc.output_normalization, dec.output_normalization] + \
      [l[k] for l in enc.layers + dec.layers for k in ("ln1", "ln2", "ln3") if k in l]
  assert len(norms) == len(scopes)
  cls = {"layernorm_L2": L.LayerNorm, "layernorm_L1": L.LayerNormL1, "batch_norm": L.TokenBatchNorm}[norm["type"]]
  assert all(type(n) is cls for n in norms)
  assert all(n.eps == norm.get("epsilon", 1e-6) for n in norms)
  if norm["type"] == "batch_norm":
    assert all(n.momentum == 0.95 and n.training for n in norms)


def test_defaults_are_unchanged():
  """Without norm_params: layernorm_L2, eps 1e-6, no state, no l2 anywhere."""
  from openseq2seq_amd.parts.transformer import layers as L
  store, enc, dec = _build(None)
  norms = [enc.output_normalization, dec.output_normalization] + \
      [l[k] for l in enc.layers + dec.layers for k in ("ln1", "ln2", "ln3") if k in l]
  assert all(type(n) is L.LayerNorm and n.eps == 1e-6 for n in norms)
  assert not store.state and all(p.l2 == 0.0 for p in store.params)


def test_batch_norm_defaults_and_modes():
  from openseq2seq_amd.parts.transformer import layers as L
  _, enc, dec = _build({"type": "batch_norm"}, mode="infer")
  n = enc.output_normalization
  assert type(n) is L.TokenBatchNorm and n.eps == 1e-4 and n.momentum == 0.95 and not n.training
  assert n.gamma is not None                        # center_scale defaults to True (common.py:20)
  assert not dec.layers[0]["ln3"].training


def test_unknown_norm_type_is_rejected():
  with pytest.raises(ValueError):
    _build({"type": "group_norm"})


@pytest.mark.parametrize("kind", ["layernorm_L2_eps", "batch_norm_cs", "batch_norm"])
def test_regularized_variables_and_scales(kind):
  """l2 on the q/k/v/output kernels and the FFN kernels and biases (scale of the encoder's / decoder's regularizer),
  on BatchNorm gamma / beta with center_scale (scale of norm_params' regularizer); nothing on the embedding or the
  LayerNorm scale / bias."""
  store, _, _ = _build(NORMS[kind], regularizer=0.001)
  for p in store.params:
    leaf = p.name.rsplit("/", 2)
    if "embedding_and_softmax" in p.name or "/layer_normalization/" in p.name:
      want = 0.0
    elif "/" + BN + "/" in p.name:
      want = 0.002
    elif p.name.endswith("/kernel") and leaf[-2] in ("qkv", "q", "kv", "output_transform", "filter_layer",
                                                      "output_layer"):
      want = 0.001
    elif p.name.endswith("/bias") and leaf[-2] in ("filter_layer", "output_layer"):
      want = 0.001
    else:
      raise AssertionError("unexpected variable " + p.name)
    assert p.l2 == pytest.approx(want), (p.name, p.l2, want)


def test_regularizer_scale_zero_means_none():
  store, _, _ = _build(None, regularizer=0.0)
  assert all(p.l2 == 0.0 for p in store.params)


@needs_ref
@pytest.mark.parametrize("cfg,kind", [("transformer-bn.py", "batch_norm"), ("transformer-nvgrad.py", "layernorm_L2")])
def test_reference_configs_load_and_construct(cfg, kind):
  from openseq2seq_amd.utils.utils import get_base_config
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.parts.transformer import layers as L
  path = os.path.join(REF, "example_configs", "text2text", "en-de", cfg)
  _, base, _, _ = get_base_config(["--config_file=" + path, "--mode=train"])
  ep = dict(base["encoder_params"], src_vocab_size=96, encoder_layers=1)
  dp = dict(base["decoder_params"], tgt_vocab_size=96, num_hidden_layers=1, batch_size=2)
  assert ep["norm_params"]["type"] == kind
  store = FlatParams(torch.device("cpu"))
  enc = base["encoder"](ep, None, mode="train").build(store)
  base["decoder"](dp, None, mode="train").build(store)
  n = enc.output_normalization
  assert n.eps == float(ep["norm_params"]["epsilon"])
  if kind == "batch_norm":
    assert type(n) is L.TokenBatchNorm and n.gamma is None and n.momentum == 0.95
    assert any(p.l2 == pytest.approx(0.001) for p in store.params)       # the regularizer of transformer-bn.py
    assert len(store.state) == 2 * (2 + 3 + 2)


@needs_ref
def test_norm_fixtures_reproduce():
  r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_ref_exec_norms.py"), "--check"],
                     cwd=REPO, capture_output=True, text=True, timeout=1800)
  assert r.returncode == 0, r.stdout + r.stderr
