"""Raw corpora generated on the fly for the LSTM language model: the files a WikiText download would hold
(train.txt / valid.txt / test.txt under a data_root), so that WKTDataLayer runs its own raw -> processed pipeline on
them. No dataset files needed."""
from __future__ import absolute_import, division, print_function

import os

import numpy as np


def write_zipf_corpus(data_root, vocab=33000, train_tokens=1200000, eval_tokens=40000, line_len=40, seed=0):
  """Words w0 .. w<vocab-1>; every word occurs at least three times in train.txt (the dictionary cuts rarer
  ones), the rest of the stream is Zipf-distributed. Returns data_root."""
  os.makedirs(data_root, exist_ok=True)
  rng = np.random.RandomState(seed)
  for split, n in (("train", train_tokens), ("valid", eval_tokens), ("test", eval_tokens)):
    ids = np.minimum(rng.zipf(1.2, size=n) - 1, vocab - 1)
    if split == "train":
      floor = np.repeat(np.arange(vocab), 3)
      ids = np.concatenate([ids[:max(n - floor.size, 0)], floor])
      rng.shuffle(ids)
    with open(os.path.join(data_root, split + ".txt"), "w") as f:
      f.write("\n")                                      # the dictionary skips the first line of train.txt
      for a in range(0, ids.size, line_len):
        f.write(" ".join("w%d" % i for i in ids[a:a + line_len]) + "\n")
  return data_root


def write_cycle_corpus(data_root, period=7, fillers=7, repeats=200):
  """A zero-entropy stream: ONE long line that repeats the words c0 .. c<period-1>, so the id stream is a cycle of
  `period` tokens with no '<eos>' inside it (the dictionary appends one per line). Three leading lines of `fillers`
  other words bring the vocabulary to 1 ('<unk>') + period + 1 ('<eos>') + fillers entries. Returns data_root."""
  os.makedirs(data_root, exist_ok=True)
  cycle = " ".join("c%d" % i for i in range(period))
  head = " ".join("f%d" % i for i in range(fillers))
  for split in ("train", "valid", "test"):
    with open(os.path.join(data_root, split + ".txt"), "w") as f:
      f.write("\n")
      if split == "train" and fillers:
        f.write((head + "\n") * 3)
      f.write(" ".join([cycle] * (repeats if split == "train" else 20)) + "\n")
  return data_root
