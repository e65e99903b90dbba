"""LSTMLM — open_seq2seq/models/lstm_lm.py: the LSTM language model shell. The vocabulary size, the end token, the
batch size and the seed tokens flow from the WKTDataLayer into the encoder parameters, tgt_vocab_size / batch_size
into the loss; the objects-per-step metric counts source + target tokens; maybe_print_logs / evaluate / infer print
what the reference prints. The text-classification phase (IMDB / SST data layers) is not built."""
from __future__ import absolute_import, division, print_function

import copy
import random

import numpy as np

from .encoder_decoder import EncoderDecoderModel
from ..data.lm.lmdata import WKTDataLayer
from ..parts.dense import SeedSeq
from ..utils.utils import deco_print


def array_to_string(row, vocab, delim=' '):
  return delim.join(vocab[int(i)] for i in row)


class LSTMLM(EncoderDecoderModel):
  def _build_forward_pass_objects(self, store):
    self._data_layer = self._create_data_layer()
    dl = self._data_layer
    self._lm_phase = isinstance(dl, WKTDataLayer)
    if not self._lm_phase:
      raise NotImplementedError("data_layer %s (the text-classification phase; WKTDataLayer is built)"
                                % type(dl).__name__)
    ep = self.params['encoder_params']
    ep['vocab_size'], ep['end_token'], ep['batch_size'] = dl.vocab_size, dl.end_token, dl.batch_size
    ep['seed_tokens'] = dl.params['seed_tokens']
    if 'regularizer' not in ep and 'regularizer' in self.params:      # encoders/lm_encoders.py:155-163
      ep['regularizer'] = copy.deepcopy(self.params['regularizer'])
      ep['regularizer_params'] = copy.deepcopy(self.params.get('regularizer_params', {}))
    self._encoder = self._create_encoder()
    self._decoder = self._create_decoder()
    self._encoder.build(store)
    self._decoder.build(store)
    if self.mode in ("train", "eval"):
      self.params['loss_params']['batch_size'] = dl.batch_size
      self.params['loss_params']['tgt_vocab_size'] = dl.vocab_size
      self._loss_computator = self._create_loss()
    self.delimiter = dl.delimiter

  def _create_data_layer(self):
    if 'processed_data_folder' in self.params:                        # models/model.py:325-326
      self.params.setdefault('data_layer_params', {})
      self.params['data_layer_params'] = dict(self.params['data_layer_params'],
                                              processed_data_folder=self.params['processed_data_folder'])
    return super(LSTMLM, self)._create_data_layer()

  def _forward(self, batch, tape, want_grad=True):
    seeds = SeedSeq(self._seed * 7919 + self._step_count)
    enc = self._encoder.encode({'source_tensors': batch['source_tensors'], 'tape': tape, 'seeds': seeds})
    dec = self._decoder.decode({'encoder_output': enc, 'target_tensors': batch['target_tensors'], 'tape': tape})
    scale_dev = self._train_op.loss_scale_view if self._train_op is not None else None
    loss = self._loss_computator.compute_loss({'decoder_output': dec, 'target_tensors': batch['target_tensors'],
                                               'loss_scale_dev': scale_dev, 'want_grad': want_grad})
    return loss, dec

  def _forward_backward(self, batch, tape):
    return self._forward(batch, tape)[0]

  # ---- eval / infer ------------------------------------------------------------------------------------------
  def infer_batch(self, batch):
    """infer: the generated ids [seeds, steps] and their lengths (the seed tokens come from the data layer's
    parameters, as in the reference; the batch only tells how many rows there are)."""
    assert self.mode == "infer"
    enc = self._encoder.encode({'source_tensors': batch['source_tensors']})
    dec = self._decoder.decode({'encoder_output': enc})
    return dec['outputs'][0], dec['final_sequence_lengths']

  def infer(self, input_values, output_values):
    vocab = self.get_data_layer().corp.dictionary.idx2word
    seed_tokens = self.params['encoder_params']['seed_tokens']
    for i in range(len(seed_tokens)):
      print('Seed:', vocab[seed_tokens[i]] + '\n')
      deco_print("Output: " + array_to_string(output_values[0][i], vocab=vocab, delim=self.delimiter), offset=4)
    return []

  def finalize_inference(self, results_per_batch, output_file):
    """Prints seed and continuation as the reference's infer() does and writes one generated row per line."""
    vocab = self.get_data_layer().corp.dictionary.idx2word
    with open(output_file, 'w') as out:
      for ids, _ in results_per_batch[:1]:          # every batch generates from the same seed tokens
        rows = ids.cpu().numpy()
        self.infer(None, [rows])
        for row in rows:
          out.write(array_to_string(row, vocab=vocab, delim=self.delimiter) + '\n')
    return {}

  def maybe_print_logs(self, input_values, output_values, training_step):
    x, len_x = input_values['source_tensors']
    y, len_y = input_values['target_tensors']
    vocab = self.get_data_layer().corp.dictionary.idx2word
    deco_print("Train Source[0]:     " + array_to_string(x[0][:int(len_x[0])], vocab=vocab, delim=self.delimiter),
               offset=4)
    deco_print("Train Target[0]:     " + array_to_string(y[0][:int(len_y[0])], vocab=vocab, delim=self.delimiter),
               offset=4)
    return {}

  def evaluate(self, device=None, max_batches=None):
    """One pass over the validation stream: mean loss per token and perplexity; one batch in ten prints source,
    target and the argmax prediction of its first row, as the reference's evaluate() does."""
    dl = self.get_data_layer()
    vocab = dl.corp.dictionary.idx2word
    if max_batches is None and dl.params.get('repeat', False):
      max_batches = max(dl.get_size_in_samples() // dl.batch_size, 1)
    total, n = 0.0, 0
    for k, batch in enumerate(dl.iterate_batches(device or self._device, drop_remainder=True)):
      if max_batches is not None and k >= max_batches:
        break
      loss, dec = self._forward(batch, None, want_grad=False)
      total += float(loss.cpu()[0])
      n += 1
      if random.random() > 0.9:
        x, y = batch['source_tensors'][0][0].cpu().numpy(), batch['target_tensors'][0][0].cpu().numpy()
        pred = np.argmax(dec['outputs'][0][0].float().cpu().numpy(), axis=-1)
        for tag, row in (("Source[0]:     ", x), ("Target[0]:     ", y), ("Prediction[0]: ", pred)):
          deco_print("*****EVAL " + tag + array_to_string(row, vocab=vocab, delim=self.delimiter), offset=4)
    mean = total / max(n, 1)
    return {"eval_loss": mean, "perplexity": float(np.exp(min(mean, 50.0))), "batches": n}

  def _get_num_objects_per_step(self, batch):
    """Source tokens + target tokens."""
    n = batch['source_tensors'][1].sum()
    if 'target_tensors' in batch:
      n = n + batch['target_tensors'][1].sum()
    return n
