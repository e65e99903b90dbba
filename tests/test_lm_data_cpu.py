"""The language-model data layer (openseq2seq_amd/data/lm) on the CPU: a twelve-line raw corpus goes through
Corpus (vocab.txt and *.ids text checked, a second construction reads the processed folder back), WKTDataLayer
windows for bptt 4 with rand_start off and on (target = source shifted by one), the `small` cuts, two-worker
sharding disjoint and complete, seed_tokens -> ids and the infer batch. With the reference present its own
lmutils.py (imported by path, an nltk stub in sys.modules) must write the same files byte for byte."""
import filecmp
import importlib.util
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

import ref_exec_util as rx

from openseq2seq_amd.data import Corpus, WKTDataLayer

REF = os.path.join(rx.gen.PKG, "data", "lm", "lmutils.py")
WORDS = ["alpha", "beta", "gamma", "delta", "well-known", "etc", "isn", "'t", "x@-@y", "<unk>", "The"]


def write_raw(root, lines=12):
  rng = random.Random(3)
  os.makedirs(root, exist_ok=True)
  for split, n in (("train", lines), ("valid", 4), ("test", 3)):
    with open(os.path.join(root, split + ".txt"), "w") as f:
      for _ in range(n):
        f.write(" " + " ".join(rng.choice(WORDS) for _ in range(9)) + " The etc . isn 't \n")
  return root


def test_corpus_files_cpu(tmp_path):
  raw, proc = write_raw(str(tmp_path / "data")), str(tmp_path / "proc")
  c = Corpus(raw, proc)
  first = open(os.path.join(proc, "train.txt")).readline()
  assert "@" not in first and "well - known" in open(os.path.join(proc, "train.txt")).read()
  assert first.endswith("The etc. is n't\n") and "  " not in first and not first.startswith(" ")
  lines = open(os.path.join(proc, "vocab.txt")).read().split("\n")
  assert lines[0] == "0\t<unk>\t0" and lines[-1] == ""
  rows = [l.split("\t") for l in lines[1:-2]]
  assert [int(r[0]) for r in rows] == list(range(1, len(rows) + 1))
  counts = [int(r[2]) for r in rows]
  assert counts == sorted(counts, reverse=True) and min(counts) >= 3
  assert lines[-2] == str(len(rows) + 1) == str(len(c.dictionary))          # the count line comes last
  words = [r[1] for r in rows]
  assert "<eos>" in words and dict(zip(words, counts))["<eos>"] == 11        # one per line, the first line skipped
  ids = open(os.path.join(proc, "train.ids")).read()
  assert not ids.endswith("\n") and [int(t) for t in ids.split("\t")] == c.train.tolist()
  n_tokens = sum(len(l.split()) + 1 for l in open(os.path.join(proc, "train.txt")))
  assert len(c.train) == n_tokens and c.train.max() < len(c.dictionary)
  again = Corpus(None, proc)                                               # read back, no raw path needed
  assert np.array_equal(again.train, c.train) and np.array_equal(again.valid, c.valid)
  assert again.dictionary.idx2word == c.dictionary.idx2word
  with pytest.raises(ValueError):
    Corpus(None, str(tmp_path / "empty"))


def test_corpus_matches_the_reference_byte_for_byte(tmp_path):
  if not os.path.exists(REF):
    pytest.skip("the reference is not present")
  try:
    import pandas  # noqa: F401  (imported by the reference's module)
  except ImportError:
    pytest.skip("pandas, which the reference's lmutils.py imports, is not installed")
  stubs = {}
  for name in ("nltk", "nltk.tokenize"):
    if name not in sys.modules:
      stubs[name] = sys.modules[name] = types.ModuleType(name)
  sys.modules["nltk.tokenize"].word_tokenize = getattr(sys.modules["nltk.tokenize"], "word_tokenize", None)
  try:
    spec = importlib.util.spec_from_file_location("ref_lmutils", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
  finally:
    for name in stubs:
      sys.modules.pop(name, None)
  raw = write_raw(str(tmp_path / "data"))
  Corpus(raw, str(tmp_path / "mine"))
  ref.Corpus(raw, str(tmp_path / "theirs"))
  for f in ("vocab.txt", "train.ids", "valid.ids", "test.ids", "train.txt", "valid.txt", "test.txt"):
    assert filecmp.cmp(str(tmp_path / "mine" / f), str(tmp_path / "theirs" / f), shallow=False), f


def _layer(tmp_path, mode="train", workers=1, worker=0, **kw):
  raw, proc = write_raw(str(tmp_path / "data"), lines=40), str(tmp_path / "proc")
  params = dict(mode=mode, batch_size=4, repeat=False, shuffle=False, bptt=4, data_root=raw,
                processed_data_folder=proc)
  params.update(kw)
  return WKTDataLayer(params, None, num_workers=workers, worker_id=worker)


def test_windows_cpu(tmp_path):
  dl = _layer(tmp_path)
  stream = dl.corp.train
  w = list(dl.windows())
  assert len(w) == (len(stream) - 0 - 1) // 4 == dl.get_size_in_samples() - (1 if len(stream) % 4 == 0 else 0)
  for i, (s, t) in enumerate(w):
    assert np.array_equal(s, stream[4 * i:4 * i + 4]) and np.array_equal(t, stream[4 * i + 1:4 * i + 5])
  dl = _layer(tmp_path, rand_start=True)
  starts = set()
  for k in range(12):
    w = list(dl.windows(random.Random(k)))
    starts.add(dl.start)
    assert 0 <= dl.start < 4 and len(w) == (len(stream) - dl.start - 1) // 4
    assert np.array_equal(w[0][0], stream[dl.start:dl.start + 4]) and np.array_equal(w[0][1], stream[dl.start + 1:dl.start + 5])
  assert len(starts) > 1
  assert dl.get_size_in_samples() == (len(stream) - dl.start) // 4
  batches = list(_layer(tmp_path).iterate_batches(torch.device("cpu")))
  (src, slen), (tgt, tlen) = batches[0]["source_tensors"], batches[0]["target_tensors"]
  assert src.shape == (4, 4) and src.dtype == torch.int32 and slen.tolist() == [4] * 4 == tlen.tolist()
  assert torch.equal(src[:, 1:], tgt[:, :-1])
  assert len(batches) == len(list(_layer(tmp_path).windows())) // 4                 # train mode drops the remainder


def test_small_and_sharding_cpu(tmp_path):
  big = str(tmp_path / "big")
  os.makedirs(big)
  for split in ("train", "valid", "test"):
    with open(os.path.join(big, split + ".txt"), "w") as f:
      f.write("\n" + "a b c d e f g h i\n" * 1100)
  kw = dict(data_root=big, processed_data_folder=str(tmp_path / "bigproc"))
  assert _layer(tmp_path, small=True, **kw).dataset_size == 9004
  assert _layer(tmp_path, mode="eval", small=True, **kw).dataset_size == 200
  assert _layer(tmp_path, **kw).dataset_size == 1 + 1100 * 10
  whole = [tuple(s) for s, _ in _layer(tmp_path).windows()]
  parts = [[tuple(s) for s, _ in _layer(tmp_path, workers=2, worker=r).windows()] for r in range(2)]
  assert parts[0] == whole[0::2] and parts[1] == whole[1::2]
  assert len(parts[0]) + len(parts[1]) == len(whole)
  sh = _layer(tmp_path, shuffle=True, shuffle_buffer_size=5)
  got = [tuple(b["source_tensors"][0][r].tolist()) for b in sh.iterate_batches(torch.device("cpu"), seed=1,
                                                                              drop_remainder=False)
         for r in range(b["source_tensors"][0].shape[0])]
  assert sorted(got) == sorted(tuple(int(v) for v in s) for s in whole) and got != [tuple(int(v) for v in s) for s in whole]


def test_seed_tokens_and_infer_batch_cpu(tmp_path):
  dl = _layer(tmp_path, mode="infer", seed_tokens="The alpha beta", batch_size=8)
  d = dl.corp.dictionary
  assert dl.params["seed_tokens"] == [d.word2idx["The"], d.word2idx["alpha"], d.word2idx["beta"]]
  assert dl.batch_size == 3 and dl.get_size_in_samples() == 3 and dl.end_token == d.word2idx["<eos>"]
  batches = list(dl.iterate_batches(torch.device("cpu")))
  assert len(batches) == 1 and batches[0]["source_tensors"][0].tolist() == [[t] for t in dl.params["seed_tokens"]]
  assert dl.vocab_size == len(d)
