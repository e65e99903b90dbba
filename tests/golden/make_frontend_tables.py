"""Fixture generator for tests/test_frontend_tables.py: builds the six Speech2Text front ends and the Text2Speech
one on the CPU device (tables only: no kernel runs) at small parameters and writes their constant tables and frame
counts to tests/golden/frontend_tables.npz.

    python tests/golden/make_frontend_tables.py [--check]

The fixture pins what the host side uploads, so it is recorded BEFORE a change to the front-end classes and must
not be regenerated to make such a change pass. --check rebuilds the tables and compares them with the file.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "frontend_tables.npz")

COMMON = dict(sample_freq=16000, window_size=20e-3, window_stride=10e-3, pad_to=8)
CASES = {
    "psf_spectrogram": dict(backend="psf", input_type="spectrogram", num_audio_features=8),
    "psf_logfbank": dict(backend="psf", input_type="logfbank", num_audio_features=8),
    "psf_mfcc": dict(backend="psf", input_type="mfcc", num_audio_features=5),
    "librosa_logfbank": dict(backend="librosa", input_type="logfbank", num_audio_features=8),
    "librosa_mfcc": dict(backend="librosa", input_type="mfcc", num_audio_features=5, features_mean=0.25,
                         features_std_dev=[1.0, 2.0, 3.0, 4.0, 5.0]),
    "librosa_spectrogram": dict(backend="librosa", input_type="spectrogram", num_audio_features=8,
                                features_mean=[0.5 * i for i in range(8)], features_std_dev=2.0),
}
TABLES = ("window", "mel_start", "mel_len", "mel_wt", "fb", "dctl", "dct", "features_mean", "features_std")
FRAME_SAMPLES = (1, 319, 320, 321, 480, 481, 16000)


def front_ends():
  """name -> front end, built on the CPU device."""
  from openseq2seq_amd.data.speech2text.speech_utils import make_front_end
  from openseq2seq_amd.data.text2speech.speech_utils import TTSFeatureFrontEnd
  cpu = torch.device("cpu")
  fes = {name: make_front_end(dict(COMMON, **case), cpu) for name, case in CASES.items()}
  fes["tts"] = TTSFeatureFrontEnd(cpu, 16000, 64, 6, features_type="mel")
  return fes


def tables():
  """'<front end>/<table>' -> array, for every table the front end has, and '<front end>/frames'."""
  out = {}
  for name, fe in front_ends().items():
    for t in TABLES:
      value = getattr(fe, t, None)
      if value is not None:
        out["%s/%s" % (name, t)] = value.numpy()
    out[name + "/frames"] = np.array([fe.frames(n) for n in FRAME_SAMPLES], np.int64)
  return out


if __name__ == "__main__":
  ap = argparse.ArgumentParser()
  ap.add_argument("--check", action="store_true")
  args = ap.parse_args()
  got = tables()
  if args.check:
    want = np.load(OUT)
    assert sorted(want.files) == sorted(got), (sorted(want.files), sorted(got))
    bad = [k for k in got if got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    print("frontend_tables: %d arrays, %s" % (len(got), "all equal" if not bad else "DIFFER: %s" % bad))
    sys.exit(1 if bad else 0)
  np.savez_compressed(OUT, **got)
  print("wrote %s: %d arrays, %d bytes" % (OUT, len(got), os.path.getsize(OUT)))
