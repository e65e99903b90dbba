"""The cell class token of the LSTM language-model configs: `from open_seq2seq.parts.rnns.weight_drop import
WeightDropLayerNormBasicLSTMCell`. Configs only NAME the cell ("core_cell": WeightDropLayerNormBasicLSTMCell);
LMEncoder recognises the token and builds LNLSTMLayer (parts/rnns/rnn_layers.py on csrc/lnlstm.hip) from
core_cell_params."""


class WeightDropLayerNormBasicLSTMCell(object):
  def __init__(self, *args, **kwargs):
    raise TypeError("WeightDropLayerNormBasicLSTMCell is a configuration token here: LMEncoder builds the layer")
