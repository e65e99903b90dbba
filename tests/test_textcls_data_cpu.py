"""IMDBDataLayer / SSTDataLayer and the classification metrics on tiny processed folders built in tmp_path:
truncation to the LAST max_length tokens, '<eos>' padding, lengths, one-hot labels, binary False -> 10 classes,
`small`, two-worker sharding, repeat / drop_remainder, the ImportError of raw preprocessing without nltk, get_stats
refused by name, and the five metric functions against hand-computed counts."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from openseq2seq_amd.data import IMDBDataLayer, SSTDataLayer, TextClassificationDataLayer
from openseq2seq_amd.data.lm import lmutils
from openseq2seq_amd.utils import metrics

WORDS = ["<unk>", "<eos>", "a", "b", "c", "d", "e", "f"]
CPU = torch.device("cpu")


def write_vocab(path):
  with open(path, "w") as f:
    for i, w in enumerate(WORDS):
      f.write("%d\t%s\t%d\n" % (i, w, 10 - i))
    f.write("%d\n" % len(WORDS))
  return path


def write_split(folder, split, rows):
  os.makedirs(folder, exist_ok=True)
  with open(os.path.join(folder, split + ".ids"), "w") as ids, open(os.path.join(folder, split + ".rat"), "w") as rat:
    for review, rating in rows:
      ids.write("\t".join(str(i) for i in review) + "\n")
      rat.write("%d\n" % rating)


TRAIN = [([2, 3, 4, 5, 6, 7, 2, 3], 1), ([4], 0), ([5, 6, 7], 1), ([2, 2], 0), ([3, 4, 5, 6], 1), ([7, 6], 0),
         ([2, 3, 4], 1), ([5], 0), ([6, 7, 2, 3, 4], 1)]
VALID = [([2, 3], 0), ([4, 5, 6], 1), ([7], 1)]
TEST = [([3, 3, 3], 1), ([4, 4], 0)]


@pytest.fixture
def folder(tmp_path):
  proc = str(tmp_path / "proc")
  for split, rows in (("train", TRAIN), ("valid", VALID), ("test", TEST)):
    write_split(proc, split, rows)
  return proc, write_vocab(str(tmp_path / "vocab.txt"))


def layer(cls, folder, mode="train", workers=1, worker=0, **extra):
  proc, vocab = folder
  params = dict(dict(lm_vocab_file=vocab, processed_data_folder=proc, shuffle=False, repeat=False, max_length=5,
                     batch_size=4, mode=mode), **extra)
  return cls(params, None, num_workers=workers, worker_id=worker)


def test_batches_truncate_pad_and_label(folder):
  dl = layer(SSTDataLayer, folder)
  assert isinstance(dl, TextClassificationDataLayer) and dl.has_files()
  assert dl.num_classes == 2 and dl.vocab_size == len(WORDS) and dl.end_token == 1
  assert dl.get_size_in_samples() == len(TRAIN)
  batches = list(dl.iterate_batches(CPU))
  assert [b["source_tensors"][0].shape[0] for b in batches] == [4, 4, 1]
  ids, lens = batches[0]["source_tensors"]
  y, ylen = batches[0]["target_tensors"]
  assert ids.dtype == torch.int32 and lens.dtype == torch.int32 and y.dtype == torch.int32
  assert lens.tolist() == [5, 1, 3, 2] and tuple(ids.shape) == (4, 5)
  assert ids[0].tolist() == [5, 6, 7, 2, 3]                  # the LAST five of eight tokens
  assert ids[1].tolist() == [4, 1, 1, 1, 1] and ids[2].tolist() == [5, 6, 7, 1, 1]       # '<eos>' padding
  assert y.tolist() == [[0, 1], [1, 0], [0, 1], [1, 0]] and ylen.tolist() == [2, 2, 2, 2]
  assert tuple(batches[2]["source_tensors"][0].shape) == (1, 5)       # padded to the batch's longest review
  assert [b["source_tensors"][0].shape[0] for b in dl.iterate_batches(CPU, drop_remainder=True)] == [4, 4]


def test_modes_read_their_split(folder):
  assert layer(SSTDataLayer, folder, "eval").get_size_in_samples() == len(VALID)
  test = layer(IMDBDataLayer, folder, "infer")
  rows = list(test.iterate_batches(CPU))
  assert len(rows) == 1 and rows[0]["source_tensors"][0].tolist() == [[3, 3, 3], [4, 4, 1]]
  assert rows[0]["target_tensors"][0].tolist() == [[0, 1], [1, 0]]


def test_imdb_ten_classes_and_small(folder, tmp_path):
  proc10 = str(tmp_path / "proc10")
  for split in ("train", "valid", "test"):
    write_split(proc10, split, [([2, 3], 9), ([4], 0), ([5, 6], 4)])
  dl = layer(IMDBDataLayer, (proc10, folder[1]), binary=False)
  assert dl.num_classes == 10
  y = next(iter(dl.iterate_batches(CPU)))["target_tensors"]
  assert tuple(y[0].shape) == (3, 10) and y[0].argmax(1).tolist() == [9, 0, 4] and y[0].sum(1).tolist() == [1, 1, 1]
  assert y[1].tolist() == [10, 10, 10]
  small = layer(IMDBDataLayer, folder, small=True, batch_size=2)
  assert small.get_size_in_samples() == 8                    # 4 batches of reviews
  assert layer(IMDBDataLayer, folder, "eval", small=True, batch_size=1).get_size_in_samples() == 2


def test_two_workers_cover_each_sample_once(folder):
  seen = []
  for w in range(2):
    dl = layer(SSTDataLayer, folder, workers=2, worker=w, max_length=8)
    for b in dl.iterate_batches(CPU):
      ids, lens = b["source_tensors"]
      seen += [tuple(ids[i, :int(lens[i])].tolist()) for i in range(ids.shape[0])]
  assert sorted(seen) == sorted(tuple(r) for r, _ in TRAIN)


def test_repeat_and_shuffle(folder):
  dl = layer(SSTDataLayer, folder, repeat=True)
  got = list(itertools.islice(dl.iterate_batches(CPU, drop_remainder=True), 5))
  assert len(got) == 5 and torch.equal(got[0]["source_tensors"][0], got[2]["source_tensors"][0])
  sh = layer(SSTDataLayer, folder, shuffle=True, max_length=8)
  a = [b["source_tensors"][1].tolist() for b in sh.iterate_batches(CPU, seed=3)]
  b = [b["source_tensors"][1].tolist() for b in sh.iterate_batches(CPU, seed=3)]
  assert a == b and sorted(sum(a, [])) == sorted(len(r) for r, _ in TRAIN)
  assert a != [b["source_tensors"][1].tolist() for b in layer(SSTDataLayer, folder, max_length=8).iterate_batches(CPU)]


@pytest.mark.parametrize("cls", [IMDBDataLayer, SSTDataLayer])
def test_raw_preprocessing_needs_nltk(cls, folder, tmp_path, monkeypatch):
  monkeypatch.setitem(sys.modules, "nltk", None)            # as on a machine without nltk
  monkeypatch.setitem(sys.modules, "nltk.tokenize", None)
  raw = tmp_path / "raw"
  for sub in ("train/pos", "train/neg", "test/pos", "test/neg"):
    (raw / sub).mkdir(parents=True)
  (raw / "train" / "pos" / "0_9.txt").write_text("a b")
  for name in ("train", "val", "test"):
    (raw / (name + ".csv")).write_text("sentence,label\na b,1\n")
  with pytest.raises(ImportError, match="nltk"):
    layer(cls, (str(tmp_path / "fresh"), folder[1]), data_root=str(raw))
  with pytest.raises(ValueError, match="data_root"):
    layer(cls, (str(tmp_path / "fresh2"), folder[1]))


def test_get_stats_is_refused_by_name(folder):
  with pytest.raises(NotImplementedError, match="get_stats"):
    layer(SSTDataLayer, folder, get_stats=True)


def test_tokenize_follows_the_reference_steps(folder):
  corp = lmutils.SSTCorpus(None, folder[0], folder[1])
  split = lambda txt: txt.split()                           # stands in for nltk's word_tokenize
  assert corp.tokenize("a-b `c 'd Xyz dont", split) == "a - b ' c ' d xyz don't"
  imdb = lmutils.IMDBCorpus(None, folder[0], folder[1])
  assert imdb.tokenize("a<br />b.c etc", split) == "a b . c etc"


def test_metrics_against_hand_counts():
  labels = np.array([1, 0, 1, 1, 0, 0, 1, 0])
  preds = np.array([1, 1, 0, 1, 0, 0, 1, 1])
  assert metrics.true_positives(labels, preds) == 3
  assert metrics.accuracy(labels, preds) == 5 / 8
  assert metrics.recall(labels, preds) == 3 / 4
  assert metrics.precision(labels, preds) == 3 / 5
  assert abs(metrics.f1(labels, preds) - 2 * 0.75 * 0.6 / 1.35) < 1e-12
  assert metrics.f1(np.array([1, 1]), np.array([0, 0])) == 0
  assert metrics.accuracy(np.array([3, 9, 0]), np.array([3, 1, 0])) == 2 / 3
