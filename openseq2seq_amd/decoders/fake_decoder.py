"""FakeDecoder — open_seq2seq/decoders/lm_decoders.py: the language model's encoder already ends in the output
layer, so the decoder half of the EncoderDecoderModel passes the encoder's output dictionary through."""
from __future__ import absolute_import, division, print_function

from .decoder import Decoder


class FakeDecoder(Decoder):
  def __init__(self, params, model, name="fake_decoder", mode='train'):
    super(FakeDecoder, self).__init__(params, model, name, mode)

  def build(self, store, *args, **kwargs):
    return self

  def _decode(self, input_dict):
    return input_dict['encoder_output']
