"""Programmatic equivalent of example_configs/text2text/en-de/en-de-nmt-small.py
(2-layer bidirectional LSTM-512 encoder with embedding, 2-layer GNMT-v2 attention decoder,
BasicSequenceLoss, Adam 1e-3 + LARC, batch 128) on synthetic token batches of the config's
shape (32 k BPE vocabulary, max_length 50), and of en-de-gnmt-like-4GPUs.py /
en-de-gnmt-like-weight-tied-2GPUs.py (gnmt_like_config)."""
from ..data.text2text.text2text import ParallelTextDataLayer
from ..decoders.rnn_decoders import RNNDecoderWithAttention
from ..encoders.rnn_encoders import BidirectionalRNNEncoderWithEmbedding, GNMTLikeEncoderWithEmbedding
from ..losses.sequence_loss import BasicSequenceLoss
from ..models.text2text import Text2Text
from ..optimizers.lr_policies import exp_decay, fixed_lr


def nmt_small_config(batch_size_per_gpu=128, max_steps=100000, vocab=32768):
  cell = {"num_units": 512, "forget_bias": 1.0}
  base_params = {
      "random_seed": 0, "use_horovod": True, "batch_size_per_gpu": batch_size_per_gpu,
      "max_steps": max_steps,
      "optimizer": "Adam", "optimizer_params": {},
      "lr_policy": fixed_lr, "lr_policy_params": {"learning_rate": 0.001},
      "larc_params": {"larc_eta": 0.001},
      "dtype": "mixed", "loss_scaling": "Backoff",
      "encoder": BidirectionalRNNEncoderWithEmbedding,
      "encoder_params": {
          "core_cell": "LSTMCell", "core_cell_params": cell, "encoder_layers": 2,
          "encoder_dp_input_keep_prob": 0.8, "encoder_dp_output_keep_prob": 1.0,
          "encoder_use_skip_connections": False, "src_emb_size": 512, "use_swap_memory": True,
      },
      "decoder": RNNDecoderWithAttention,
      "decoder_params": {
          "core_cell": "LSTMCell", "core_cell_params": cell, "decoder_layers": 2,
          "decoder_dp_input_keep_prob": 0.8, "decoder_dp_output_keep_prob": 1.0,
          "decoder_use_skip_connections": False, "GO_SYMBOL": 2, "END_SYMBOL": 1,
          "tgt_emb_size": 512, "attention_type": "gnmt_v2", "attention_layer_size": 512,
          "use_swap_memory": True,
      },
      "loss": BasicSequenceLoss,
      "loss_params": {"offset_target_by_one": True, "average_across_timestep": False, "do_mask": True},
      "data_layer": ParallelTextDataLayer,
      "data_layer_params": {
          "src_vocab_file": None, "tgt_vocab_file": None, "source_file": "", "target_file": "",
          "delimiter": " ", "shuffle": True, "repeat": True, "max_length": 50,
          "synthetic_vocab_size": vocab,
      },
  }
  return Text2Text, base_params


def gnmt_like_config(batch_size_per_gpu=32, max_steps=340000, vocab=32768, weight_tied=False, units=1024,
                     encoder_layers=7, decoder_layers=8, max_length=50):
  """en-de-gnmt-like-4GPUs.py: 7-layer GNMT encoder (one bidirectional layer, then unidirectional ones with skip
  connections), 8-layer gnmt_v2 decoder with skip connections, 1024 units, attention_layer_size 1024, Adam with the
  luong10 decay, uniform(-0.1, 0.1) initialisation, batch 32 per GPU, max_length 50; weight_tied = the
  en-de-gnmt-like-weight-tied-2GPUs.py variant (the decoder embedding is the output projection). Mixed precision,
  as the config's own comment offers; synthetic token batches. units / layers scale the model down for tests."""
  cell = {"num_units": units, "forget_bias": 1.0}
  init = {"initializer": "random_uniform_initializer", "initializer_params": {"minval": -0.1, "maxval": 0.1}}
  decoder_params = dict(init, **{
      "core_cell": "LSTMCell", "core_cell_params": cell, "decoder_layers": decoder_layers,
      "decoder_dp_input_keep_prob": 0.8, "decoder_dp_output_keep_prob": 1.0,
      "decoder_use_skip_connections": True, "GO_SYMBOL": 2, "END_SYMBOL": 1,
      "tgt_emb_size": units, "attention_type": "gnmt_v2", "attention_layer_size": units,
  })
  if weight_tied:
    decoder_params["weight_tied"] = True
  base_params = {
      "random_seed": 0, "use_horovod": False, "batch_size_per_gpu": batch_size_per_gpu,
      "max_steps": max_steps,
      "optimizer": "Adam", "optimizer_params": {},
      "lr_policy": exp_decay,
      "lr_policy_params": {"learning_rate": 0.0008, "begin_decay_at": 170000, "decay_steps": 17000,
                           "decay_rate": 0.5, "use_staircase_decay": True, "min_lr": 0.0000005},
      "max_grad_norm": 32768.0,
      "dtype": "mixed", "loss_scaling": "Backoff",
      "encoder": GNMTLikeEncoderWithEmbedding,
      "encoder_params": dict(init, **{
          "core_cell": "LSTMCell", "core_cell_params": cell, "encoder_layers": encoder_layers,
          "encoder_dp_input_keep_prob": 0.8, "encoder_dp_output_keep_prob": 1.0,
          "encoder_use_skip_connections": True, "src_emb_size": units,
      }),
      "decoder": RNNDecoderWithAttention,
      "decoder_params": decoder_params,
      "loss": BasicSequenceLoss,
      "loss_params": {"offset_target_by_one": True, "average_across_timestep": True, "do_mask": True},
      "data_layer": ParallelTextDataLayer,
      "data_layer_params": {
          "src_vocab_file": None, "tgt_vocab_file": None, "source_file": "", "target_file": "",
          "delimiter": " ", "shuffle": True, "repeat": True, "max_length": max_length,
          "synthetic_vocab_size": vocab,
      },
  }
  return Text2Text, base_params
