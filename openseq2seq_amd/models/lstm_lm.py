"""LSTMLM — open_seq2seq/models/lstm_lm.py: the LSTM language model shell. The vocabulary size, the end token, the
batch size and the seed tokens flow from the WKTDataLayer into the encoder parameters, tgt_vocab_size / batch_size
into the loss; the objects-per-step metric counts source + target tokens; maybe_print_logs / evaluate / infer print
what the reference prints.

Over a TextClassificationDataLayer (IMDBDataLayer / SSTDataLayer) the same class is the sentiment classifier of
example_configs/transfer: fc_dim = num_classes flows into the encoder, which is built as LMClassifierEncoder in
place of the configured LMEncoder; the loss is CrossEntropyLoss. evaluate returns the accuracy (computed per batch
and averaged), with two classes precision / recall / F1 from counts summed over the batches, and eval_loss; infer
writes the TSV Source / Pred / Label and prints the test accuracy."""
from __future__ import absolute_import, division, print_function

import copy
import random

import numpy as np

from .encoder_decoder import EncoderDecoderModel
from ..data.lm.lmdata import TextClassificationDataLayer, WKTDataLayer
from ..encoders.lm_encoders import LMClassifierEncoder, LMEncoder, LMSampledEncoder
from ..utils import metrics
from ..parts.dense import SeedSeq
from ..utils.utils import deco_print


def array_to_string(row, vocab, delim=' '):
  return delim.join(vocab[int(i)] for i in row)


class LSTMLM(EncoderDecoderModel):
  def _build_forward_pass_objects(self, store):
    self._data_layer = self._create_data_layer()
    dl = self._data_layer
    self._lm_phase = isinstance(dl, WKTDataLayer)
    if not self._lm_phase and not isinstance(dl, TextClassificationDataLayer):
      raise NotImplementedError("data_layer %s (WKTDataLayer and the TextClassificationDataLayer family are built)"
                                % type(dl).__name__)
    ep = self.params['encoder_params']
    ep['vocab_size'], ep['end_token'], ep['batch_size'] = dl.vocab_size, dl.end_token, dl.batch_size
    self._print_f1 = False
    if self._lm_phase:
      ep['seed_tokens'] = dl.params['seed_tokens']
    else:
      ep['fc_dim'] = dl.num_classes
      self._print_f1 = dl.num_classes == 2
    if 'regularizer' not in ep and 'regularizer' in self.params:      # encoders/lm_encoders.py:155-163
      ep['regularizer'] = copy.deepcopy(self.params['regularizer'])
      ep['regularizer_params'] = copy.deepcopy(self.params.get('regularizer_params', {}))
    self._encoder = self._create_encoder()
    self._decoder = self._create_decoder()
    self._encoder.build(store)
    self._decoder.build(store)
    if self.mode in ("train", "eval"):
      if self._lm_phase:
        self.params['loss_params']['batch_size'] = dl.batch_size
        self.params['loss_params']['tgt_vocab_size'] = dl.vocab_size
      self._loss_computator = self._create_loss()
    self.delimiter = dl.delimiter

  def _create_data_layer(self):
    for key in ('lm_vocab_file', 'processed_data_folder'):            # models/model.py:323-326
      if key in self.params:
        self.params['data_layer_params'] = dict(self.params.get('data_layer_params', {}), **{key: self.params[key]})
    cls = self.params['data_layer']
    if isinstance(cls, type) and issubclass(cls, TextClassificationDataLayer) and self.mode != 'train' and \
        'eval_batch_size_per_gpu' in self.params:                     # models/model.py:319-322
      train_batch = self.params['batch_size_per_gpu']
      self.params['batch_size_per_gpu'] = self.params['eval_batch_size_per_gpu']
      try:
        return super(LSTMLM, self)._create_data_layer()
      finally:
        self.params['batch_size_per_gpu'] = train_batch
    return super(LSTMLM, self)._create_data_layer()

  def _create_encoder(self):
    cls = self.params['encoder']
    if not self._lm_phase and cls is LMEncoder:
      # the classification network is LMEncoder's subclass (LMEncoder itself refuses fc_dim / use_cell_state)
      return LMClassifierEncoder(params=self.params['encoder_params'], mode=self.mode, model=self)
    ep = self.params['encoder_params']
    if self._lm_phase and cls is LMEncoder and self.mode == 'train' and not ep.get('use_cudnn_rnn', False) and \
        ep.get('num_sampled', ep['vocab_size']) < ep['vocab_size']:
      # sampled softmax training (encoders/lm_encoders.py:375-381): the subclass that stops before the output layer
      return LMSampledEncoder(params=ep, mode=self.mode, model=self)
    return super(LSTMLM, self)._create_encoder()

  def _forward(self, batch, tape, want_grad=True):
    seeds = SeedSeq(self._seed * 7919 + self._step_count)
    enc = self._encoder.encode({'source_tensors': batch['source_tensors'], 'tape': tape, 'seeds': seeds})
    dec = self._decoder.decode({'encoder_output': enc, 'target_tensors': batch.get('target_tensors'), 'tape': tape})
    if self._loss_computator is None:
      return None, dec
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
    if not self._lm_phase:
      # classification: the (source text, predicted class, label) rows of the batch, as the reference's infer()
      _, dec = self._forward(batch, None, want_grad=False)
      values = {k: [t.cpu().numpy() for t in batch[k]] for k in ('source_tensors', 'target_tensors') if k in batch}
      return self.infer(values, [dec['outputs'][0].cpu().numpy()])
    enc = self._encoder.encode({'source_tensors': batch['source_tensors']})
    dec = self._decoder.decode({'encoder_output': enc})
    return dec['outputs'][0], dec['final_sequence_lengths']

  def infer(self, input_values, output_values):
    vocab = self.get_data_layer().corp.dictionary.idx2word
    if not self._lm_phase:
      x, len_x = input_values['source_tensors']
      y = input_values['target_tensors'][0] if 'target_tensors' in input_values else None
      return [(array_to_string(x[i][:int(len_x[i])], vocab=vocab, delim=self.delimiter),
               int(np.argmax(output_values[0][i])), None if y is None else int(np.argmax(y[i])))
              for i in range(len(x))]
    seed_tokens = self.params['encoder_params']['seed_tokens']
    for i in range(len(seed_tokens)):
      print('Seed:', vocab[seed_tokens[i]] + '\n')
      deco_print("Output: " + array_to_string(output_values[0][i], vocab=vocab, delim=self.delimiter), offset=4)
    return []

  def finalize_inference(self, results_per_batch, output_file):
    """Prints seed and continuation as the reference's infer() does and writes one generated row per line."""
    if not self._lm_phase:
      return self._finalize_classification(results_per_batch, output_file)
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
    if not self._lm_phase:
      y, out = np.asarray(y), np.asarray(output_values[0])
      deco_print("TRAIN Target[0]:     " + str(np.argmax(y[0])), offset=4)
      deco_print("TRAIN Prediction[0]:     " + str(out[0]), offset=4)
      labels, preds = np.argmax(y, 1), np.argmax(out, axis=-1)
      print('Labels', labels)
      print('Preds', preds)
      deco_print("Accuracy: {:.4f}".format(metrics.accuracy(labels, preds)), offset=4)
      if self._print_f1:
        deco_print("Precision: {:.4f} | Recall: {:.4f} | F1: {:.4f}".format(
            metrics.precision(labels, preds), metrics.recall(labels, preds), metrics.f1(labels, preds)), offset=4)
      return {}
    deco_print("Train Target[0]:     " + array_to_string(y[0][:int(len_y[0])], vocab=vocab, delim=self.delimiter),
               offset=4)
    return {}

  def _finalize_classification(self, results_per_batch, output_file):
    """The TSV Source / Pred / Label, one row per sample, and the test numbers the reference prints."""
    preds, labels = [], []
    with open(output_file, 'w') as out:
      out.write('\t'.join(['Source', 'Pred', 'Label']) + '\n')
      for results in results_per_batch:
        for x, pred, y in results:
          out.write('\t'.join([x, str(pred), str(y)]) + '\n')
          preds.append(pred)
          labels.append(y)
    if labels and labels[0] is not None:
      preds, labels = np.asarray(preds), np.asarray(labels)
      deco_print("TEST Accuracy: {:.4f}".format(metrics.accuracy(labels, preds)), offset=4)
      if self._print_f1 and labels.sum() > 0 and preds.sum() > 0:
        deco_print("TEST Precision: {:.4f} | Recall: {:.4f} | F1: {:.4f}".format(
            metrics.precision(labels, preds), metrics.recall(labels, preds), metrics.f1(labels, preds)), offset=4)
    return {}

  def _evaluate_classification(self, device, max_batches):
    """finalize_evaluation of the reference: the mean of the per-batch accuracies; with two classes precision /
    recall / F1 from the counts summed over the batches (0 when there is no true positive)."""
    dl = self.get_data_layer()
    vocab = dl.corp.dictionary.idx2word
    if max_batches is None and dl.params.get('repeat', False):
      max_batches = max(-(-dl.get_size_in_samples() // dl.batch_size), 1)
    accs, total = [], 0.0
    true_pos = pred_pos = actual_pos = 0.0
    for k, batch in enumerate(dl.iterate_batches(device or self._device, drop_remainder=False)):
      if max_batches is not None and k >= max_batches:
        break
      loss, dec = self._forward(batch, None, want_grad=False)
      total += float(loss.cpu()[0])
      x, len_x = (t.cpu().numpy() for t in batch['source_tensors'])
      y = batch['target_tensors'][0].cpu().numpy()
      out = dec['outputs'][0].cpu().numpy()
      deco_print("*****EVAL Source[0]:     " + array_to_string(x[0][:int(len_x[0])], vocab=vocab,
                                                                delim=self.delimiter), offset=4)
      deco_print("EVAL Target[0]:     " + str(np.argmax(y[0])), offset=4)
      deco_print("EVAL Prediction[0]:     " + str(out[0]), offset=4)
      labels, preds = np.argmax(y, 1), np.argmax(out, axis=-1)
      print('Labels', labels)
      print('Preds', preds)
      accs.append(float(metrics.accuracy(labels, preds)))
      if self._print_f1:
        true_pos += float(metrics.true_positives(labels, preds))
        pred_pos += float(np.sum(preds))
        actual_pos += float(np.sum(labels))
    res = {"accuracy": float(np.mean(accs)) if accs else 0.0, "eval_loss": total / max(len(accs), 1),
           "batches": len(accs)}
    deco_print("EVAL Accuracy: {:.4f}".format(res["accuracy"]), offset=4)
    if self._print_f1:
      prec = rec = f1 = 0.0
      if true_pos > 0:
        prec, rec = true_pos / pred_pos, true_pos / actual_pos
        f1 = 2.0 * prec * rec / (rec + prec)
        deco_print("EVAL Precision: {:.4f} | Recall: {:.4f} | F1: {:.4f} | True pos: {}".format(prec, rec, f1, true_pos),
                   offset=4)
      res.update(precision=prec, recall=rec, f1=f1)
    return res

  def evaluate(self, device=None, max_batches=None):
    """One pass over the validation stream: mean loss per token and perplexity; one batch in ten prints source,
    target and the argmax prediction of its first row, as the reference's evaluate() does."""
    if not self._lm_phase:
      return self._evaluate_classification(device, max_batches)
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
