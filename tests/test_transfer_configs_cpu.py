"""The reference's text-classification configs (example_configs/transfer/*.py) load unchanged through
get_base_config in train, eval and infer mode and resolve to this package's LSTMLM, LMEncoder, FakeDecoder,
IMDBDataLayer / SSTDataLayer and CrossEntropyLoss; with fc_dim the encoder parameters pass check_params and build
as LMClassifierEncoder with the reference's variables in its creation order. imdb-wkt2-cudnn.py is refused by
name when the encoder is BUILT; a bare LMEncoder(fc_dim=2) still refuses and points to the subclass. Skips without
the reference."""
import glob
import os

import pytest
import torch

import ref_exec_util as rx

import openseq2seq_amd as pkg
from openseq2seq_amd.utils.utils import get_base_config

REF = os.path.join(rx.gen.REF, "example_configs", "transfer")
CUDNN = "imdb-wkt2-cudnn.py"
CONFIGS = sorted(c for c in glob.glob(os.path.join(REF, "*.py")) if os.path.basename(c) != CUDNN)


def _classifier(base, mode, classes=2):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  params = dict(base["encoder_params"], vocab_size=33278, end_token=7, batch_size=base["batch_size_per_gpu"],
                fc_dim=classes)
  if "regularizer" in base:                                  # LSTMLM hands the model's regulariser to the encoder
    params.update(regularizer=base["regularizer"], regularizer_params=base.get("regularizer_params", {}))
  store = FlatParams(torch.device("cpu"))
  return pkg.encoders.LMClassifierEncoder(params, None, mode=mode).build(store), store


@pytest.mark.parametrize("mode", ["train", "eval", "infer"])
def test_reference_transfer_configs_load(mode):
  if not CONFIGS:
    pytest.skip("the reference is not present")
  assert len(CONFIGS) == 5
  for cfg in CONFIGS:
    args, base, model, module = get_base_config(["--config_file=" + cfg, "--mode=" + mode])
    assert model is pkg.models.LSTMLM and base["encoder"] is pkg.encoders.LMEncoder
    assert base["decoder"] is pkg.decoders.FakeDecoder and base["loss"] is pkg.losses.CrossEntropyLoss
    want = pkg.data.SSTDataLayer if os.path.basename(cfg).startswith("sst") else pkg.data.IMDBDataLayer
    for part in ("train_params", "eval_params", "infer_params"):
      assert module[part]["data_layer"] is want
      assert issubclass(module[part]["data_layer"], pkg.data.TextClassificationDataLayer)
    enc, store = _classifier(base, mode)
    ep = base["encoder_params"]
    last = ep["emb_size"] if ep.get("weight_tied", False) else ep["core_cell_params"]["num_units"]
    D = last * (2 if ep.get("use_cell_state", False) else 1)
    names = [p.name for p in store.params]
    scope = "ForwardPass/rnn_encoder_awd/"
    assert names[:3] == [scope + "dense/kernel", scope + "dense/bias", scope + "EncoderEmbeddingMatrix"]
    assert tuple(store.params[0].shape) == (1, 2, D) and tuple(store.params[1].shape) == (2,)
    assert tuple(store.params[2].shape) == (33278, ep["emb_size"])
    assert len(names) == 3 + 12 * ep["encoder_layers"] and all("/cells/cell_" in n for n in names[3:])
    # the l2 regulariser is wired to the Dense kernel only
    assert store.params[0].l2 > 0 and all(p.l2 == 0 for p in store.params[1:])


def test_cudnn_classification_config_is_refused_at_build_time():
  cfg = os.path.join(REF, CUDNN)
  if not os.path.exists(cfg):
    pytest.skip("the reference is not present")
  args, base, model, module = get_base_config(["--config_file=" + cfg, "--mode=train"])
  assert base["encoder"] is pkg.encoders.LMEncoder and base["encoder_params"]["use_cudnn_rnn"]
  with pytest.raises(NotImplementedError, match="use_cudnn_rnn"):
    _classifier(base, "train")


def test_bare_lm_encoder_still_refuses_the_classification_phase():
  from openseq2seq_amd.configs.lstm_lm import lstm_lm_config
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  _, base, _, _, _ = lstm_lm_config("unused", "unused", num_units=16, emb_size=8, layers=2)
  for key, value in (("fc_dim", 2), ("use_cell_state", True)):
    params = dict(base["encoder_params"], vocab_size=17, end_token=1, batch_size=2, **{key: value})
    with pytest.raises(NotImplementedError, match=key) as e:
      pkg.encoders.LMEncoder(params, None, mode="train").build(FlatParams(torch.device("cpu")))
    assert "LMClassifierEncoder" in str(e.value)


def test_classifier_rejects_more_classes_than_the_head_holds():
  from openseq2seq_amd.configs.text_cls import text_cls_config
  _, base, train, _, _ = text_cls_config("imdb", "unused", "unused", num_units=16, emb_size=8, layers=2)
  assert train["data_layer"] is pkg.data.IMDBDataLayer and base["loss"] is pkg.losses.CrossEntropyLoss
  enc, store = _classifier(base, "train", classes=10)
  assert tuple(store.params[0].shape) == (1, 10, 16)
  with pytest.raises(NotImplementedError, match="fc_dim"):
    _classifier(base, "train", classes=17)
