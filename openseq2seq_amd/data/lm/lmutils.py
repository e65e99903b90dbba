"""Vocabulary and corpus files of the WikiText language-model data — the behaviour of
open_seq2seq/data/lm/lmutils.py:14-168 (Dictionary, Corpus), written against it: the same raw -> processed pipeline
(four regex substitutions per line, tokens re-joined by single blanks), the same vocab.txt (three tab-separated
columns id, word, count; '<unk>' as id 0 with count 0 first; the words of train.txt by falling count, its first
line skipped, '<eos>' counted once per line; words seen fewer than `limit` times cut, and the line that cuts them
holds the vocabulary size alone) and the same tab-separated *.ids files. An existing processed folder is read
back instead of rebuilt. No nltk: only the IMDB / SST corpora of the reference use it.

One deliberate difference: WikiText's raw file names (wiki.{train,valid,test}.raw) are READ under those names; the
reference renames them to {train,valid,test}.txt inside data_root first."""
from __future__ import absolute_import, division, print_function

import collections
import os
import re

import numpy as np

SPLITS = ("train", "valid", "test")
# (pattern, replacement) in the order applied; 'etc .' is a regular expression: its dot matches any character
SUBSTITUTIONS = (("@-@", "-"), ("-", " - "), ("etc .", "etc."))
CONTRACTION = ("n 't", " n't")


class Dictionary(object):
  UNK, EOS = "<unk>", "<eos>"

  def __init__(self, limit=3, vocab_link=None):
    self.word2idx, self.idx2word, self.counter = {}, [], collections.Counter()
    if vocab_link and os.path.isfile(vocab_link):
      self.load_vocab(vocab_link)

  def add_word(self, word):
    idx = self.word2idx.get(word)
    if idx is None:
      idx = self.word2idx[word] = len(self.idx2word)
      self.idx2word.append(word)
    self.counter[idx] += 1
    return idx

  def load_vocab(self, vocab_link):
    with open(vocab_link, "r") as f:
      lines = f.readlines()
    self.idx2word = [0] * int(lines[-1].strip())
    for line in lines[:-1]:
      idx, word, count = line.strip().split("\t")
      idx = int(idx)
      self.word2idx[word] = idx
      self.idx2word[idx] = word
      self.counter[idx] = int(count)
    for special in (self.UNK, self.EOS):
      if special not in self.word2idx:
        self.add_word(special)

  def __len__(self):
    return len(self.idx2word)


def processed_exists(proc_path):
  return os.path.isdir(proc_path) and all(os.path.exists(os.path.join(proc_path, s + ".ids")) for s in SPLITS)


def _ids_text(ids):
  return "\t".join(str(i) for i in ids)


class Corpus(object):
  VOCAB = "vocab.txt"

  def __init__(self, raw_path, proc_path, change_contraction=True, limit=3):
    os.makedirs(proc_path, exist_ok=True)
    self.limit, self.change_contraction = limit, change_contraction
    self.dictionary = Dictionary(limit)
    if processed_exists(proc_path):
      self.dictionary.load_vocab(os.path.join(proc_path, self.VOCAB))
      self.train, self.valid, self.test = (self.load_ids(os.path.join(proc_path, s + ".ids")) for s in SPLITS)
      return
    if not raw_path:
      raise ValueError("data_root [directory to the original data] must be specified")
    self.preprocess(raw_path, proc_path)
    self.create_dictionary(proc_path, os.path.join(proc_path, "train.txt"))
    self.dictionary = Dictionary(limit)
    self.dictionary.load_vocab(os.path.join(proc_path, self.VOCAB))
    self.train, self.valid, self.test = (self.tokenize(proc_path, proc_path, s + ".txt") for s in SPLITS)

  @staticmethod
  def _raw_file(raw_path, split):
    wiki = os.path.join(raw_path, "wiki.%s.raw" % split)
    plain = os.path.join(raw_path, split + ".txt")
    return wiki if (os.path.isfile(wiki) and not os.path.isfile(plain)) else plain

  def clean_line(self, line):
    for pat, rep in SUBSTITUTIONS + ((CONTRACTION,) if self.change_contraction else ()):
      line = re.sub(pat, rep, line)
    return " ".join(tok.strip() for tok in line.split())

  def preprocess(self, raw_path, proc_path):
    for split in SPLITS:
      with open(self._raw_file(raw_path, split), "r") as src, open(os.path.join(proc_path, split + ".txt"), "w") as dst:
        for line in src:
          dst.write(self.clean_line(line) + "\n")

  def create_dictionary(self, proc_path, filename):
    """Words enter the dictionary only from the train file (whose first line is skipped)."""
    d = self.dictionary
    d.add_word(d.UNK)
    with open(filename, "r") as f:
      f.readline()
      for line in f:
        for word in line.split() + [d.EOS]:
          d.add_word(word)
    with open(os.path.join(proc_path, self.VOCAB), "w") as f:
      f.write("\t".join(["0", d.UNK, "0"]) + "\n")
      for idx, (token_id, count) in enumerate(d.counter.most_common(), start=1):
        if count < self.limit:
          f.write("%d\n" % idx)
          return
        f.write("\t".join([str(idx), d.idx2word[token_id], str(count)]) + "\n")

  def tokenize(self, raw_path, proc_path, filename):
    d = self.dictionary
    unk = d.word2idx[d.UNK]
    ids = []
    with open(os.path.join(raw_path, filename), "r") as f:
      for line in f:
        ids.extend(d.word2idx.get(w, unk) for w in line.split() + [d.EOS])
    with open(os.path.join(proc_path, filename[:-3] + "ids"), "w") as out:
      out.write(_ids_text(ids))
    return np.asarray(ids)

  @staticmethod
  def load_ids(filename):
    with open(filename, "r") as f:
      return np.asarray([int(i) for i in f.read().strip().split("\t")])
