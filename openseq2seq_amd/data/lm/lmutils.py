"""Vocabulary and corpus files of the WikiText language-model data — the behaviour of
open_seq2seq/data/lm/lmutils.py:14-168 (Dictionary, Corpus), written against it: the same raw -> processed pipeline
(four regex substitutions per line, tokens re-joined by single blanks), the same vocab.txt (three tab-separated
columns id, word, count; '<unk>' as id 0 with count 0 first; the words of train.txt by falling count, its first
line skipped, '<eos>' counted once per line; words seen fewer than `limit` times cut, and the line that cuts them
holds the vocabulary size alone) and the same tab-separated *.ids files. An existing processed folder is read
back instead of rebuilt.

IMDBCorpus / SSTCorpus (lmutils.py:170-490): sentiment corpora on the LANGUAGE MODEL'S vocabulary (lm_vocab_link).
A processed folder holds {train,valid,test}.ids (one review per line, tab-separated ids) and .rat (one integer
label per line); it is read back without any further import. Building one from the raw data (aclImdb folders of
.txt files; binary_sst csv files with the columns sentence / label) follows the reference's steps: character
substitutions, nltk's word_tokenize, a second chance for out-of-vocabulary tokens (a leading apostrophe split off,
lower case, eight unapostrophed contractions repaired, tokenised again), quote and 'etc.' repairs, ids with
'<unk>' for what is still unknown; IMDB moves 1000 shuffled training reviews to the validation split. nltk (and
pandas for SST) are imported only there; without nltk the ImportError says so. get_stats (histogram plots through
matplotlib) is not built.

One deliberate difference: WikiText's raw file names (wiki.{train,valid,test}.raw) are READ under those names; the
reference renames them to {train,valid,test}.txt inside data_root first."""
from __future__ import absolute_import, division, print_function

import collections
import glob
import os
import random
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


# ------------------------------------------------------------------------------------------ sentiment corpora
# (pattern, replacement) applied to a raw review before word_tokenize; IMDB_ONLY comes first for IMDB
IMDB_ONLY = (("<br />", " "), ("\u0096", " "), ("\u0097", " "))
RAW_SUBS = (("-", " - "), (r"\+", " + "), (r"\*", " * "), ("/", " / "), ("`", "'"))
IMDB_DOT = ((r"\.", " . "),)                       # after '-', before '+', as the reference orders them
IMDB_MS = ((r" ms \.", " ms."), (r"Ms \.", "Ms."))
JOINED_SUBS = (("''", '"'), ("' '", '"'), ("``", '"'), (r"etc \.", "etc. "), (" etc ", " etc. "))
# the reference's repairs of contractions written without the apostrophe ('wouldnt' becomes "wounldn't" there too)
OOV_SUBS = (("thats", "that's"), ("wouldnt", "wounldn't"), ("couldnt", "couldn't"), ("cant", "can't"),
            ("dont", "don't"), ("didnt", "didn't"), ("isnt", "isn't"), ("wasnt", "wasn't"))


def _word_tokenize():
  try:
    from nltk.tokenize import word_tokenize
  except ImportError as e:
    raise ImportError("building an IMDB / SST corpus from raw data needs nltk (nltk.tokenize.word_tokenize), which "
                      "is not installed; a processed folder ({train,valid,test}.ids and .rat) loads without it") from e
  return word_tokenize


def _sub_all(txt, subs):
  for pat, rep in subs:
    txt = re.sub(pat, rep, txt)
  return txt


class SentimentCorpus(object):
  """What IMDBCorpus and SSTCorpus share: the dictionary of the language model, the processed-folder files, the
  tokenisation of one raw review."""
  PRE_SUBS = RAW_SUBS

  def __init__(self, raw_path, proc_path, lm_vocab_link, get_stats=False):
    if get_stats:
      raise NotImplementedError("get_stats (length statistics and histogram plots of the corpus)")
    exists = processed_exists(proc_path)
    os.makedirs(proc_path, exist_ok=True)
    self.dictionary = Dictionary(vocab_link=lm_vocab_link)
    self.raw_path, self.proc_path = raw_path, proc_path
    if exists:
      print('Loading corpus from processed data ...')
      self.train, self.valid, self.test = (self.load_ids(s) for s in SPLITS)
      return
    print('Creating corpus from raw data ...')
    if not raw_path:
      raise ValueError("data_root [directory to the original data] must be specified")
    self.preprocess()

  def tokenize(self, txt, word_tokenize=None):
    word_tokenize = word_tokenize or _word_tokenize()
    known = self.dictionary.word2idx
    words = []
    for token in word_tokenize(_sub_all(txt, self.PRE_SUBS)):
      if token not in known and token.startswith("'"):
        words.append("'")
        token = token[1:]
      if token in known:
        words.append(token)
      else:
        words.extend(word_tokenize(_sub_all(token.lower(), OOV_SUBS)))
    return _sub_all(" ".join(words), JOINED_SUBS)

  def txt2ids(self, token_file, rating_file):
    unk = self.dictionary.word2idx[self.dictionary.UNK]
    with open(rating_file, "r") as f:
      ratings = [int(line.strip()) for line in f]
    with open(token_file, "r") as f:
      reviews = [[self.dictionary.word2idx.get(tok, unk) for tok in line.strip().split()] for line in f]
    return list(zip(reviews, ratings))

  def ids2file(self):
    for split in SPLITS:
      with open(os.path.join(self.proc_path, split + ".ids"), "w") as ids, \
           open(os.path.join(self.proc_path, split + ".rat"), "w") as rat:
        for review, rating in getattr(self, split):
          ids.write(_ids_text(review) + "\n")
          rat.write("%d\n" % rating)

  def load_ids(self, split):
    with open(os.path.join(self.proc_path, split + ".rat"), "r") as f:
      ratings = [int(line.strip()) for line in f]
    with open(os.path.join(self.proc_path, split + ".ids"), "r") as f:
      reviews = [[int(i) for i in line.strip().split("\t")] for line in f]
    return list(zip(reviews, ratings))


class IMDBCorpus(SentimentCorpus):
  """aclImdb: {train,test}/{pos,neg}/<id>_<rating>.txt. binary: label 1 for pos, 0 for neg; else rating - 1 (ten
  classes)."""
  PRE_SUBS = IMDB_ONLY + RAW_SUBS[:1] + IMDB_DOT + RAW_SUBS[1:] + IMDB_MS

  def __init__(self, raw_path, proc_path, lm_vocab_link, binary=True, get_stats=False):
    self.binary = binary
    super(IMDBCorpus, self).__init__(raw_path, proc_path, lm_vocab_link, get_stats)

  def preprocess_folder(self, split):
    word_tokenize = _word_tokenize()
    token_file = os.path.join(self.proc_path, split + ".tok")
    rating_file = os.path.join(self.proc_path, split + ".inter.rat")
    with open(token_file, "w") as tok, open(rating_file, "w") as rat:
      for sent in ("pos", "neg"):
        for name in glob.glob(os.path.join(self.raw_path, split, sent, "*.txt")):
          with open(name, "r") as f:
            tok.write(self.tokenize(f.read(), word_tokenize) + "\n")
          rating = int(sent == "pos") if self.binary else int(name[name.rfind("_") + 1:-4]) - 1
          rat.write("%d\n" % rating)
    return self.txt2ids(token_file, rating_file)

  def preprocess(self, val_count=1000):
    train = self.preprocess_folder("train")
    random.shuffle(train)
    self.train, self.valid = train[val_count:], train[:val_count]
    self.test = self.preprocess_folder("test")
    self.ids2file()


class SSTCorpus(SentimentCorpus):
  """binary_sst: {train,val,test}.csv with the columns sentence and label."""

  def preprocess_file(self, raw_split, split):
    word_tokenize = _word_tokenize()
    import pandas as pd
    data = pd.read_csv(os.path.join(self.raw_path, raw_split + ".csv"))
    token_file = os.path.join(self.proc_path, split + ".tok")
    rating_file = os.path.join(self.proc_path, split + ".rat")
    with open(token_file, "w") as tok, open(rating_file, "w") as rat:
      for _, row in data.iterrows():
        tok.write(self.tokenize(row["sentence"], word_tokenize) + "\n")
        rat.write("%s\n" % row["label"])
    return self.txt2ids(token_file, rating_file)

  def preprocess(self):
    self.train = self.preprocess_file("train", "train")
    self.valid = self.preprocess_file("val", "valid")
    self.test = self.preprocess_file("test", "test")
    self.ids2file()
