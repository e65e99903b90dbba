"""Sampled-softmax training of the language model, the CPU side: lstm-wkt103-mixed.py loads and LMSampledEncoder of
its parameters builds for training (the reference's vocabulary of 267 735 words) where LMEncoder refuses; the three
configurations the sampled softmax cannot serve raise ValueError naming their parameter; LSTMLM._create_encoder
picks the subclass only for a training with num_sampled < vocab_size; BasicSampledSequenceLoss constructs."""
import os

import pytest
import torch

import ref_exec_util as rx

import openseq2seq_amd as pkg
from openseq2seq_amd.configs.lstm_lm import lstm_lm_config
from openseq2seq_amd.optimizers.flat_params import FlatParams
from openseq2seq_amd.utils.utils import get_base_config

CFG = os.path.join(rx.gen.REF, "example_configs", "lm", "lstm-wkt103-mixed.py")
WKT103_VOCAB = 267735


def _small(**extra):
  _, base, _, _, _ = lstm_lm_config("unused", "unused", num_units=16, emb_size=8, layers=2, dropout=False,
                                    num_sampled=8)
  assert base["loss"] is pkg.losses.BasicSampledSequenceLoss
  return dict(base["encoder_params"], vocab_size=40, end_token=1, batch_size=2, **extra)


def test_wkt103_config_builds_the_sampled_encoder():
  if not os.path.exists(CFG):
    pytest.skip("the reference is not present")
  args, base, model, module = get_base_config(["--config_file=" + CFG, "--mode=train"])
  assert base["loss"] is pkg.losses.BasicSampledSequenceLoss and base["encoder_params"]["num_sampled"] == 8192
  params = dict(base["encoder_params"], vocab_size=WKT103_VOCAB, end_token=7, batch_size=base["batch_size_per_gpu"])
  store = FlatParams(torch.device("cpu"))
  enc = pkg.encoders.LMSampledEncoder(params, None, mode="train").build(store)
  assert enc.sampled and enc.sampler.S == 8192 and enc.sampler.V == WKT103_VOCAB
  names = [p.name for p in store.params]
  assert names[0].endswith("dense/kernel") and names[1].endswith("dense/bias")     # the variables of LMEncoder
  assert not any(n.endswith("EncoderEmbeddingMatrix") for n in names)              # weight_tied
  loss = base["loss"](dict(base["loss_params"], batch_size=224, tgt_vocab_size=WKT103_VOCAB), None)
  assert loss._average_across_timestep and not loss._do_mask and not loss._offset_target_by_one


def test_sampled_encoder_is_lm_encoder_outside_training():
  enc = pkg.encoders.LMSampledEncoder(_small(), None, mode="eval").build(FlatParams(torch.device("cpu")))
  assert not enc.sampled and not hasattr(enc, "sampler")
  with pytest.raises(NotImplementedError, match="num_sampled"):
    pkg.encoders.LMEncoder(_small(), None, mode="train").build(FlatParams(torch.device("cpu")))
  with pytest.raises(NotImplementedError, match="num_sampled"):       # the cuDNN-form LM keeps the refusal
    pkg.encoders.LMSampledEncoder(_small(use_cudnn_rnn=True, cudnn_rnn_type="CudnnLSTM"), None,
                                  mode="train").build(FlatParams(torch.device("cpu")))


@pytest.mark.parametrize("extra,name", [(dict(fc_use_bias=False), "fc_use_bias"),
                                        (dict(weight_tied=False), "emb_size"),
                                        (dict(num_sampled=21), "num_sampled"),
                                        (dict(num_sampled=0), "num_sampled")])
def test_value_errors_name_their_parameter(extra, name):
  with pytest.raises(ValueError, match=name):
    pkg.encoders.LMSampledEncoder(_small(**extra), None, mode="train").build(FlatParams(torch.device("cpu")))


def test_untied_sampled_encoder_of_equal_widths_builds():
  params = _small(weight_tied=False)
  params["core_cell_params"] = dict(params["core_cell_params"], num_units=8)
  store = FlatParams(torch.device("cpu"))
  enc = pkg.encoders.LMSampledEncoder(params, None, mode="train").build(store)
  assert enc.emb is not None and tuple(enc.emb.shape) == (40, 8)


@pytest.mark.parametrize("mode,num_sampled,cudnn,want", [("train", 8, False, "LMSampledEncoder"),
                                                         ("train", 40, False, "LMEncoder"),
                                                         ("train", None, False, "LMEncoder"),
                                                         ("eval", 8, False, "LMEncoder"),
                                                         ("infer", 8, False, "LMEncoder"),
                                                         ("train", 8, True, "LMEncoder")])
def test_create_encoder_picks_the_subclass_only_for_sampled_training(mode, num_sampled, cudnn, want):
  ep = _small(seed_tokens=[1, 2], use_cudnn_rnn=cudnn)
  if num_sampled is None:
    del ep["num_sampled"]
  else:
    ep["num_sampled"] = num_sampled
  model = pkg.models.LSTMLM.__new__(pkg.models.LSTMLM)
  model._params = {"encoder": pkg.encoders.LMEncoder, "encoder_params": ep, "dtype": "mixed"}
  model._mode, model._lm_phase = mode, True
  assert type(model._create_encoder()).__name__ == want
