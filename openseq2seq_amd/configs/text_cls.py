"""Programmatic equivalent of example_configs/transfer/sst-wkt2.py and imdb-wkt2.py (a trained LSTM language model
fine-tuned into a sentiment classifier: the LayerNorm-LSTM stack of configs/lstm_lm.py, the classifier on the last
layer's final state [h, c], CrossEntropyLoss, Adam at a fixed 1e-4, load_model naming the language model's
checkpoint folder), with the sizes as arguments. dataset 'sst': SSTDataLayer, batch 20, max_length 96; 'imdb':
IMDBDataLayer, batch 16, max_length 256."""
from ..data.lm.lmdata import IMDBDataLayer, SSTDataLayer
from ..decoders.fake_decoder import FakeDecoder
from ..encoders.lm_encoders import LMEncoder
from ..losses.cross_entropy_loss import CrossEntropyLoss
from ..models.lstm_lm import LSTMLM
from ..optimizers.lr_policies import fixed_lr
from ..parts.rnns.weight_drop import WeightDropLayerNormBasicLSTMCell

DATASETS = {"sst": (SSTDataLayer, 20, 96), "imdb": (IMDBDataLayer, 16, 256)}


def text_cls_config(dataset, processed_data_folder, lm_vocab_file, data_root=None, load_model=None,
                    batch_size_per_gpu=None, eval_batch_size_per_gpu=None, max_length=None, layers=3, num_units=896,
                    emb_size=256, learning_rate=1e-4, dropout=True, use_cell_state=True, binary=True, logdir=None,
                    max_steps=None):
  """Returns (base_model, base_params, train_params, eval_params, infer_params). dropout: the configs' keep
  probabilities (output 0.8, embedding matrix 0.7), else 1.0 everywhere."""
  layer, batch, length = DATASETS[dataset]
  batch = batch_size_per_gpu or batch
  length = max_length or length
  keep = (lambda v: v) if dropout else (lambda v: 1.0)
  base_params = {
      "random_seed": 0, "use_horovod": False, "num_gpus": 1, "batch_size_per_gpu": batch,
      "eval_batch_size_per_gpu": eval_batch_size_per_gpu or batch,
      "lm_vocab_file": lm_vocab_file, "processed_data_folder": processed_data_folder,
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
          "encoder_dp_input_keep_prob": 1.0, "encoder_dp_output_keep_prob": keep(0.8),
          "encoder_last_input_keep_prob": 1.0, "encoder_last_output_keep_prob": keep(0.8),
          "recurrent_keep_prob": 1.0, "encoder_emb_keep_prob": keep(0.7),
          "encoder_use_skip_connections": False, "emb_size": emb_size, "num_tokens_gen": 10,
          "sampling_prob": 0.0, "fc_use_bias": True, "weight_tied": True, "awd_initializer": False,
          "use_cell_state": use_cell_state,
      },
      "decoder": FakeDecoder,
      "regularizer": "l2_regularizer", "regularizer_params": {"scale": 2e-6},
      "loss": CrossEntropyLoss,
  }
  for key, value in (("logdir", logdir), ("load_model", load_model), ("max_steps", max_steps)):
    if value is not None:
      base_params[key] = value
  if max_steps is None:
    base_params["num_epochs"] = 120
  extra = {"binary": binary} if dataset == "imdb" else {}
  train_params = {"data_layer": layer, "data_layer_params": dict(
      extra, data_root=data_root, shuffle=True, shuffle_buffer_size=25000, repeat=True, max_length=length)}
  if data_root is None:
    del train_params["data_layer_params"]["data_root"]
  eval_params = {"data_layer": layer, "data_layer_params": dict(extra, shuffle=False, repeat=False, max_length=length)}
  infer_params = {"data_layer": layer, "data_layer_params": dict(extra, shuffle=False, repeat=False,
                                                                 max_length=length)}
  return LSTMLM, base_params, train_params, eval_params, infer_params
