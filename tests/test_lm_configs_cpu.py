"""The reference's five language-model configs (example_configs/lm/*.py) load unchanged through get_base_config in
train and infer mode and resolve to this package's LSTMLM, LMEncoder, FakeDecoder, WKTDataLayer and
BasicSequenceLoss; LMEncoder(params + vocab_size / end_token / batch_size) passes check_params;
lstm-wkt103-mixed.py raises the num_sampled NotImplementedError when the encoder is BUILT for training, and not
before. Skips without the reference. The own config example_configs/lm/lstm_lm_synthetic.py is only checked for
its factory (it writes a corpus when loaded)."""
import glob
import os

import pytest
import torch

import ref_exec_util as rx

import openseq2seq_amd as pkg
from openseq2seq_amd.utils.utils import get_base_config

REF = os.path.join(rx.gen.REF, "example_configs", "lm")
CONFIGS = sorted(glob.glob(os.path.join(REF, "*.py")))


def _encoder(base, mode, **extra):
  params = dict(base["encoder_params"], vocab_size=33278, end_token=7, batch_size=base["batch_size_per_gpu"], **extra)
  return base["encoder"](params, None, mode=mode)


@pytest.mark.parametrize("mode", ["train", "infer"])
def test_reference_lm_configs_load(mode):
  if not CONFIGS:
    pytest.skip("the reference is not present")
  assert len(CONFIGS) == 5
  for cfg in CONFIGS:
    args, base, model, module = get_base_config(["--config_file=" + cfg, "--mode=" + mode])
    assert model is pkg.models.LSTMLM and base["encoder"] is pkg.encoders.LMEncoder
    assert base["decoder"] is pkg.decoders.FakeDecoder
    for part in ("train_params", "eval_params", "infer_params"):
      assert module[part]["data_layer"] is pkg.data.WKTDataLayer
    sampled = os.path.basename(cfg) == "lstm-wkt103-mixed.py"
    assert base["loss"] is (pkg.losses.BasicSampledSequenceLoss if sampled else pkg.losses.BasicSequenceLoss)
    enc = _encoder(base, mode, **({"seed_tokens": [3, 4]} if mode == "infer" else {}))      # check_params passes
    assert enc.params["vocab_size"] == 33278


def test_sampled_softmax_is_refused_at_build_time():
  cfg = os.path.join(REF, "lstm-wkt103-mixed.py")
  if not os.path.exists(cfg):
    pytest.skip("the reference is not present")
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  args, base, model, module = get_base_config(["--config_file=" + cfg, "--mode=train"])
  enc = _encoder(base, "train")                          # constructing it is fine
  with pytest.raises(NotImplementedError, match="num_sampled"):
    enc.build(FlatParams(torch.device("cpu")))
  _encoder(base, "eval").build(FlatParams(torch.device("cpu")))        # the full softmax of eval mode is built


@pytest.mark.parametrize("key,value", [("input_weight_keep_prob", 0.5), ("recurrent_weight_keep_prob", 0.5),
                                       ("weight_variational", True), ("encoder_use_skip_connections", True),
                                       ("encoder_dp_input_keep_prob", 0.5), ("variational_recurrent", True),
                                       ("time_major", True), ("fc_dim", 2), ("use_cell_state", True)])
def test_unbuilt_parameters_raise_by_name(key, value):
  from openseq2seq_amd.configs.lstm_lm import lstm_lm_config
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  _, base, _, _, _ = lstm_lm_config("unused", "unused", num_units=16, emb_size=8, layers=2)
  params = dict(base["encoder_params"], vocab_size=17, end_token=1, batch_size=2)
  params[key] = value
  with pytest.raises(NotImplementedError) as e:
    pkg.encoders.LMEncoder(params, None, mode="train").build(FlatParams(torch.device("cpu")))
  assert (key if key != "fc_dim" else "fc_dim") in str(e.value)
