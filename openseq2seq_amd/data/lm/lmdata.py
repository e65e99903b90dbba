"""WKTDataLayer — the behaviour of open_seq2seq/data/lm/lmdata.py:15-176 without tf.data: windows of `bptt` tokens
over the id stream of a split, n = (size - start - 1) // bptt of them, source [begin, begin + bptt) and the target
shifted by one; `rand_start` draws start from [0, bptt) once per pass; `small` cuts the stream to 9004 ids (200 in
eval mode); workers take every num_workers-th window (Dataset.shard); shuffling goes through a buffer of
shuffle_buffer_size windows (-1: get_size_in_samples()), as Dataset.shuffle does; in infer mode one row per seed
token. get_size_in_samples as in the reference, (size - start) // bptt.

TextClassificationDataLayer / IMDBDataLayer / SSTDataLayer (:178-362): the reviews of a processed sentiment corpus
on the language model's vocabulary (lm_vocab_file). A review longer than max_length keeps its LAST max_length
tokens; the label is a one-hot int [num_classes] (IMDB: 2, or 10 with binary False; SST: 2); a batch is padded
with the '<eos>' id to its longest review; source lengths are the review lengths, target lengths num_classes.
`small` (IMDB) keeps 4 batches of reviews (2 in eval mode); workers take every num_workers-th review of a pass;
shuffling and `repeat` as for WKTDataLayer. train / eval / infer read the train / valid / test split."""
from __future__ import absolute_import, division, print_function

import random

import numpy as np
import torch

from ..data_layer import DataLayer
from .lmutils import Corpus, IMDBCorpus, SSTCorpus


class WKTDataLayer(DataLayer):
  @staticmethod
  def get_required_params():
    return dict(DataLayer.get_required_params(), **{'repeat': bool, 'bptt': int})

  @staticmethod
  def get_optional_params():
    return dict(DataLayer.get_optional_params(), **{
        'data_root': str, 'rand_start': bool, 'small': bool, 'use_targets': bool, 'delimiter': str,
        'map_parallel_calls': int, 'prefetch_buffer_size': int, 'pad_lengths_to_eight': bool,
        'pad_vocab_to_eight': bool, 'seed_tokens': str, 'shuffle_buffer_size': int, 'processed_data_folder': str,
    })

  def __init__(self, params, model, num_workers=1, worker_id=0):
    super(WKTDataLayer, self).__init__(params, model, num_workers, worker_id)
    p = self.params
    self._processed_data_folder = p.get('processed_data_folder', 'wkt-processed_data')
    self._data_root = p.get('data_root', None)
    self.corp = Corpus(self._data_root, self._processed_data_folder)
    d = self.corp.dictionary
    self.end_token = d.word2idx[d.EOS]
    # (a seed word the vocabulary lacks maps to '<unk>', as in tokenised text; the reference raises KeyError, also
    # for its default seed 'The' on a corpus without that word)
    p['seed_tokens'] = [d.word2idx.get(t, d.word2idx[d.UNK]) for t in p.get('seed_tokens', 'The').split()]
    mode = p['mode']
    if mode == 'train':
      self.corp.content = self.corp.train
    elif mode == 'eval':
      self.corp.content = self.corp.valid
    else:
      self.corp.content = p['seed_tokens']
    self.batch_size = p['batch_size']
    if mode not in ('train', 'eval'):
      self.batch_size = min(len(self.corp.content), p['batch_size'])
    self.vocab_file = (self._processed_data_folder, 'vocab.txt')
    self.bptt = p['bptt']
    self.rand_start = p.get('rand_start', False)
    self._shuffle_buffer_size = p.get('shuffle_buffer_size', -1)
    self.delimiter = p.get('delimiter', ' ')
    self._small = p.get('small', False)
    self.start = 0
    if self._small:
      self.corp.content = self.corp.content[:200 if mode == 'eval' else 9004]
    if p.get('pad_vocab_to_eight', False):
      raise NotImplementedError("pad_vocab_to_eight (the reference applies it to the id stream; no config sets it)")
    self.dataset_size = len(self.corp.content)
    self.vocab_size = len(d.idx2word)
    self._input_tensors = {}

  # ---- the reference's protocol ------------------------------------------------------------------------
  def build_graph(self):
    pass

  @property
  def input_tensors(self):
    return self._input_tensors

  def get_size_in_samples(self):
    if self.params['mode'] in ('train', 'eval'):
      return (self.dataset_size - self.start) // self.bptt
    return len(self.corp.content)

  # ---- windows ---------------------------------------------------------------------------------------------
  def windows(self, rng=random):
    """One pass of (source, target) windows of this worker, in stream order."""
    if self.params['mode'] not in ('train', 'eval'):
      for i, seed in enumerate(self.corp.content):
        if i % self._num_workers == self._worker_id:
          yield [seed], [seed]
      return
    if self.rand_start:
      self.start = rng.randint(0, self.bptt - 1)
    content, bptt = self.corp.content, self.bptt
    for i in range((self.dataset_size - self.start - 1) // bptt):
      if i % self._num_workers != self._worker_id:
        continue
      begin = self.start + i * bptt
      yield content[begin:begin + bptt], content[begin + 1:begin + bptt + 1]

  def _shuffled(self, it, rng):
    size = self._shuffle_buffer_size
    if size == -1:
      size = self.get_size_in_samples()
    buf = []
    for item in it:
      buf.append(item)
      if len(buf) > max(size, 1):
        yield buf.pop(rng.randrange(len(buf)))
    while buf:
      yield buf.pop(rng.randrange(len(buf)))

  # ---- the drivers' protocol (run.py, Model) ------------------------------------------------------------------
  def has_files(self):
    return True

  def iterate_batches(self, device, seed=0, drop_remainder=None):
    """Batches dict(source_tensors=[ids int32 [B,T], lens int32 [B]], target_tensors=[...]) on `device`; repeats
    for ever under 'repeat' (train and eval modes)."""
    rng = random.Random(seed)
    train_like = self.params['mode'] in ('train', 'eval')
    if drop_remainder is None:
      drop_remainder = self.params['mode'] == 'train'
    while True:
      it = self.windows(rng)
      if self.params.get('shuffle', False):
        it = self._shuffled(it, rng)
      rows = []
      for item in it:
        rows.append(item)
        if len(rows) == self.batch_size:
          yield self._batch(rows, device, train_like)
          rows = []
      if rows and not drop_remainder:
        yield self._batch(rows, device, train_like)
      if not (self.params.get('repeat', False) and train_like):
        return

  @staticmethod
  def _batch(rows, device, with_targets):
    def side(k):
      ids = torch.from_numpy(np.asarray([r[k] for r in rows], dtype=np.int32)).to(device)
      return [ids, torch.full((ids.shape[0],), ids.shape[1], dtype=torch.int32, device=device)]
    out = {'source_tensors': side(0)}
    if with_targets:
      out['target_tensors'] = side(1)
    return out


class TextClassificationDataLayer(DataLayer):
  @staticmethod
  def get_required_params():
    return dict(DataLayer.get_required_params(), **{
        'lm_vocab_file': str, 'shuffle': bool, 'repeat': bool, 'max_length': int, 'processed_data_folder': str,
    })

  @staticmethod
  def get_optional_params():
    return dict(DataLayer.get_optional_params(), **{
        'rand_start': bool, 'small': bool, 'use_targets': bool, 'delimiter': str, 'map_parallel_calls': int,
        'prefetch_buffer_size': int, 'pad_lengths_to_eight': bool, 'pad_vocab_to_eight': bool,
        'shuffle_buffer_size': int, 'data_root': str, 'binary': bool, 'num_classes': int, 'get_stats': bool,
    })

  def __init__(self, params, model, num_workers=1, worker_id=0):
    super(TextClassificationDataLayer, self).__init__(params, model, num_workers, worker_id)
    p = self.params
    self._data_root = p.get('data_root', None)
    self._binary = p.get('binary', True)
    self._get_stats = p.get('get_stats', False)
    self._lm_vocab_file = p['lm_vocab_file']
    self._processed_data_folder = p['processed_data_folder']
    self._shuffle_buffer_size = p.get('shuffle_buffer_size', -1)
    self._small = p.get('small', False)
    self._max_length = p['max_length']
    self.delimiter = p.get('delimiter', ' ')
    self.batch_size = p['batch_size']
    if p.get('pad_lengths_to_eight', False) and self._max_length % 8 != 0:
      raise ValueError("If padding to 8 in data layer, then max_length should be multiple of 8")
    self._input_tensors = {}

  def _take_split(self, corp):
    """The split of this mode becomes corp.content; the sizes and the '<eos>' id follow."""
    self.corp = corp
    mode = self.params['mode']
    corp.content = corp.train if mode == 'train' else corp.valid if mode == 'eval' else corp.test
    d = corp.dictionary
    self.vocab_size = len(d.idx2word)
    self.EOS_ID = self.end_token = d.word2idx[d.EOS]

  # ---- the reference's protocol ------------------------------------------------------------------------
  def build_graph(self):
    pass

  @property
  def input_tensors(self):
    return self._input_tensors

  def get_size_in_samples(self):
    return self.dataset_size

  # ---- samples ---------------------------------------------------------------------------------------------
  def samples(self):
    """One pass of this worker's (review ids, one-hot label), in corpus order."""
    for i, (review, raw_rating) in enumerate(self.corp.content):
      if i % self._num_workers != self._worker_id:
        continue
      rating = np.zeros(self.num_classes, dtype=np.int32)
      rating[raw_rating] = 1
      yield review[-self._max_length:], rating

  _shuffled = WKTDataLayer._shuffled

  # ---- the drivers' protocol (run.py, Model) ------------------------------------------------------------------
  def has_files(self):
    return True

  def iterate_batches(self, device, seed=0, drop_remainder=None):
    """Batches dict(source_tensors=[ids int32 [B,T] padded with '<eos>', lens int32 [B]], target_tensors=[one-hot
    int32 [B,C], int32 [B] = C]) on `device`; repeats for ever under 'repeat' (train and eval modes)."""
    rng = random.Random(seed)
    if drop_remainder is None:
      drop_remainder = False
    while True:
      it = self.samples()
      if self.params['shuffle']:
        it = self._shuffled(it, rng)
      rows = []
      for item in it:
        rows.append(item)
        if len(rows) == self.batch_size:
          yield self._batch(rows, device)
          rows = []
      if rows and not drop_remainder:
        yield self._batch(rows, device)
      if not (self.params['repeat'] and self.params['mode'] in ('train', 'eval')):
        return

  def _batch(self, rows, device):
    lens = np.asarray([len(r[0]) for r in rows], dtype=np.int32)
    ids = np.full((len(rows), max(int(lens.max()), 1)), self.EOS_ID, dtype=np.int32)
    for i, (review, _) in enumerate(rows):
      ids[i, :len(review)] = review
    labels = np.stack([r[1] for r in rows])
    return {'source_tensors': [torch.from_numpy(ids).to(device), torch.from_numpy(lens).to(device)],
            'target_tensors': [torch.from_numpy(labels).to(device),
                               torch.full((len(rows),), self.num_classes, dtype=torch.int32, device=device)]}


class IMDBDataLayer(TextClassificationDataLayer):
  """The IMDB reviews (aclImdb): two classes, or the ten ratings with binary False."""

  def __init__(self, params, model, num_workers=1, worker_id=0):
    super(IMDBDataLayer, self).__init__(params, model, num_workers, worker_id)
    self.num_classes = 2 if self._binary else 10
    self._take_split(IMDBCorpus(self._data_root, self._processed_data_folder, self._lm_vocab_file, self._binary,
                                get_stats=self._get_stats))
    if self._small:
      self.corp.content = self.corp.content[:self.batch_size * (2 if self.params['mode'] == 'eval' else 4)]
    self.dataset_size = len(self.corp.content)


class SSTDataLayer(TextClassificationDataLayer):
  """The Stanford Sentiment Treebank, binary: two classes."""

  def __init__(self, params, model, num_workers=1, worker_id=0):
    super(SSTDataLayer, self).__init__(params, model, num_workers, worker_id)
    self.num_classes = 2
    self._take_split(SSTCorpus(self._data_root, self._processed_data_folder, self._lm_vocab_file,
                               get_stats=self._get_stats))
    self.dataset_size = len(self.corp.content)
