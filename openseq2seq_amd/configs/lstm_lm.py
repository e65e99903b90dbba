"""Programmatic equivalent of example_configs/lm/lstm-wkt2-fp32.py (AWD-style LSTM language model: LMEncoder of
WeightDropLayerNormBasicLSTMCell layers, weight-tied embedding, FakeDecoder, BasicSequenceLoss averaged over all
entries, Adam at a fixed learning rate), with the sizes as arguments."""
from ..data.lm.lmdata import WKTDataLayer
from ..decoders.fake_decoder import FakeDecoder
from ..encoders.lm_encoders import LMEncoder
from ..losses.sequence_loss import BasicSampledSequenceLoss, BasicSequenceLoss
from ..models.lstm_lm import LSTMLM
from ..optimizers.lr_policies import fixed_lr
from ..parts.rnns.weight_drop import WeightDropLayerNormBasicLSTMCell


def lstm_lm_config(data_root, processed_data_folder, batch_size_per_gpu=160, bptt=96, layers=3, num_units=896,
                   emb_size=256, learning_rate=4e-4, dropout=True, seed_tokens="The", num_tokens_gen=10,
                   logdir=None, max_steps=None, num_sampled=None):
  """Returns (base_model, base_params, train_params, eval_params, infer_params). dropout: the wkt2 config's keep
  probabilities (output 0.6, recurrent 0.7, embedding matrix 0.37), else 1.0 everywhere. num_sampled: train with the
  sampled softmax of lstm-wkt103-mixed.py (BasicSampledSequenceLoss; eval stays the full softmax)."""
  keep = (lambda v: v) if dropout else (lambda v: 1.0)
  base_params = {
      "random_seed": 0, "use_horovod": False, "num_gpus": 1, "batch_size_per_gpu": batch_size_per_gpu,
      "processed_data_folder": processed_data_folder,
      "optimizer": "Adam", "optimizer_params": {},
      "lr_policy": fixed_lr, "lr_policy_params": {"learning_rate": learning_rate},
      "dtype": "float32",
      "encoder": LMEncoder,
      "encoder_params": {
          "initializer": "random_uniform_initializer", "initializer_params": {"minval": -0.1, "maxval": 0.1},
          "use_cudnn_rnn": False, "cudnn_rnn_type": None,
          "core_cell": WeightDropLayerNormBasicLSTMCell,
          "core_cell_params": {"num_units": num_units, "forget_bias": 1.0},
          "encoder_layers": layers,
          "encoder_dp_input_keep_prob": 1.0, "encoder_dp_output_keep_prob": keep(0.6),
          "encoder_last_input_keep_prob": 1.0, "encoder_last_output_keep_prob": keep(0.6),
          "recurrent_keep_prob": keep(0.7), "encoder_emb_keep_prob": keep(0.37),
          "encoder_use_skip_connections": False, "emb_size": emb_size, "num_tokens_gen": num_tokens_gen,
          "sampling_prob": 0.0, "fc_use_bias": True, "weight_tied": True, "awd_initializer": False,
      },
      "decoder": FakeDecoder,
      "regularizer": "l2_regularizer", "regularizer_params": {"scale": 2e-6},
      "loss": BasicSequenceLoss,
      "loss_params": {"offset_target_by_one": False, "average_across_timestep": True, "do_mask": False},
  }
  if num_sampled is not None:
    base_params["encoder_params"]["num_sampled"] = int(num_sampled)
    base_params["loss"] = BasicSampledSequenceLoss
  if logdir is not None:
    base_params["logdir"] = logdir
  if max_steps is not None:
    base_params["max_steps"] = max_steps
  else:
    base_params["num_epochs"] = 1500
  train_params = {"data_layer": WKTDataLayer, "data_layer_params": {
      "data_root": data_root, "rand_start": True, "shuffle": True, "shuffle_buffer_size": 25000, "repeat": True,
      "bptt": bptt}}
  eval_params = {"data_layer": WKTDataLayer, "data_layer_params": {
      "data_root": data_root, "shuffle": False, "repeat": False, "bptt": bptt}}
  infer_params = {"data_layer": WKTDataLayer, "data_layer_params": {
      "data_root": data_root, "shuffle": False, "repeat": False, "rand_start": False, "bptt": bptt,
      "seed_tokens": seed_tokens}}
  return LSTMLM, base_params, train_params, eval_params, infer_params
