# pylint: skip-file
"""A tiny Transformer (https://arxiv.org/abs/1706.03762) on the toy task of reversing sequences — the
reference's Transformer acceptance configuration (example_configs/text2text/toy-reversal/nmt-reversal-TT.py)
with its parameter values unchanged: d_model 128, 8 heads of 16, filter 512, 2 + 2 layers, LazyAdam under
transformer_policy (learning rate 1.0, 200 warm-up steps), beam 5 / alpha 1.0 / extra_decode_length 2, the
14-token vocabularies as the data layer reads them (no padding to a multiple of 8), dtype float32 as the
reference has it (this package computes in bf16 with fp32 master weights whatever the dtype says).
transformer-reversal-512.py next to this file is the same task at d_model 512 with a retuned learning rate.

Data: python -m openseq2seq_amd.test_utils.create_reversed_examples writes toy_text_data/."""
from __future__ import absolute_import, division, print_function
from open_seq2seq.models import Text2Text
from open_seq2seq.encoders import TransformerEncoder
from open_seq2seq.decoders import TransformerDecoder
from open_seq2seq.data.text2text.text2text import ParallelTextDataLayer
from open_seq2seq.losses import PaddedCrossEntropyLossWithSmoothing
from open_seq2seq.data.text2text.text2text import SpecialTextTokens
from open_seq2seq.optimizers.lr_policies import transformer_policy
import tensorflow as tf

base_model = Text2Text
d_model = 128
num_layers = 2
data_root = "toy_text_data/"


def _text(source, target, **kw):
  """data_layer_params of one split (tgt_vocab of the infer split is the source vocabulary, as in the reference)"""
  return dict({
    "src_vocab_file": data_root + "vocab/source.txt",
    "tgt_vocab_file": data_root + "vocab/target.txt",
    "source_file": data_root + source,
    "target_file": data_root + target,
    "delimiter": " ",
    "special_tokens_already_in_vocab": False,
    "use_start_token": False,
  }, **kw)


base_params = {
  "use_horovod": False,
  "num_gpus": 1,
  "batch_size_per_gpu": 64,
  "max_steps": 800,
  "save_summaries_steps": 50,
  "print_loss_steps": 50,
  "print_samples_steps": 50,
  "eval_steps": 50,
  "save_checkpoint_steps": 300,
  "logdir": "ReversalTask-Transformer-Transformer",
  "dtype": tf.float32,

  "optimizer": tf.contrib.opt.LazyAdamOptimizer,
  "optimizer_params": {"beta1": 0.9, "beta2": 0.997, "epsilon": 0.000000001},
  "lr_policy": transformer_policy,
  "lr_policy_params": {"learning_rate": 1.0, "warmup_steps": 200, "d_model": d_model},

  "encoder": TransformerEncoder,
  "encoder_params": {
    "encoder_layers": num_layers, "hidden_size": d_model, "num_heads": 8,
    "attention_dropout": 0.1, "filter_size": 4 * d_model, "relu_dropout": 0.1,
    "layer_postprocess_dropout": 0.1, "remove_padding": True,
  },

  "decoder": TransformerDecoder,
  "decoder_params": {
    "layer_postprocess_dropout": 0.1, "num_hidden_layers": num_layers, "hidden_size": d_model,
    "num_heads": 8, "attention_dropout": 0.1, "relu_dropout": 0.1, "filter_size": 4 * d_model,
    "beam_size": 5, "alpha": 1.0, "extra_decode_length": 2,
    "EOS_ID": SpecialTextTokens.EOS_ID.value,
    "GO_SYMBOL": SpecialTextTokens.S_ID.value,
    "END_SYMBOL": SpecialTextTokens.EOS_ID.value,
    "PAD_SYMBOL": SpecialTextTokens.PAD_ID.value,
  },

  "loss": PaddedCrossEntropyLossWithSmoothing,
  "loss_params": {},
}

train_params = {
  "data_layer": ParallelTextDataLayer,
  "data_layer_params": _text("train/source.txt", "train/target.txt", shuffle=True, repeat=True, max_length=56),
}

eval_params = {
  "data_layer": ParallelTextDataLayer,
  # repeat: the dev set is evaluated many times during a run
  "data_layer_params": _text("dev/source.txt", "dev/target.txt", shuffle=False, repeat=True, max_length=56),
}

infer_params = {
  "batch_size_per_gpu": 1,
  "data_layer": ParallelTextDataLayer,
  "data_layer_params": _text("test/source.txt", "test/target.txt", shuffle=False, repeat=False, max_length=256,
                             tgt_vocab_file=data_root + "vocab/source.txt"),
}
