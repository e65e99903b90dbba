"""Fixture generator for the two 'mfcc' front ends: executes the REFERENCE'S OWN get_speech_features
(open_seq2seq/data/speech2text/speech_utils.py, where it lies) on the 0.44 s int16 test signal stored in
ref_exec_frontend.npz and writes tests/golden/ref_exec_frontend_mfcc.npz (features and durations only).

    python tests/golden/make_ref_exec_mfcc.py [--check]

The third-party libraries are the stand-ins of oracle/ref_shim/audio_libs, as for make_ref_exec.py's 'frontend'
fixture. Their librosa.feature module is empty; this generator attaches, in its own process, the one function the
'mfcc' path calls — librosa.feature.mfcc as librosa 0.6.3 publishes it:

    def mfcc(y=None, sr=22050, S=None, n_mfcc=20, dct_type=2, norm='ortho', **kwargs):
      if S is None: S = power_to_db(melspectrogram(y=y, sr=sr, **kwargs))
      return scipy.fftpack.dct(S, axis=0, type=dct_type, norm=norm)[:n_mfcc]

The reference passes S (the linear power STFT), so the mel / dB branch never runs and n_mels is ignored. When a real
librosa can be imported, its function is held against the stand-in once.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_exec as gen  # noqa: E402

NAME = "frontend_mfcc"
CASES = {
    "psf_mfcc": dict(backend="psf", input_type="mfcc", num_audio_features=13, pad_to=8),
    "librosa_mfcc": dict(backend="librosa", input_type="mfcc", num_audio_features=13, num_fft=512,
                         norm_per_feature=True, dither=0.0),
}


def mfcc(y=None, sr=22050, S=None, n_mfcc=20, dct_type=2, norm="ortho", **kwargs):      # noqa: N803
  from scipy.fftpack import dct
  if S is None:
    raise NotImplementedError("the reference's call site passes S; the mel / dB branch is not restated")
  return dct(S, axis=0, type=dct_type, norm=norm)[:n_mfcc]


def _check_against_real_librosa():
  """Only where librosa happens to be installed: the real function agrees with the stand-in."""
  try:
    import librosa
  except ImportError:
    return
  S = np.abs(np.random.RandomState(0).standard_normal((257, 9))).astype(np.float32)     # noqa: N806
  np.testing.assert_allclose(librosa.feature.mfcc(sr=16000, S=S, n_mfcc=13, n_mels=26), mfcc(S=S, n_mfcc=13),
                             rtol=1e-5, atol=1e-5)


def generate():
  _check_against_real_librosa()
  sys.path.insert(0, os.path.join(gen.REPO, "oracle", "ref_shim"))
  import audio_libs
  mods = audio_libs.install()
  mods["librosa.feature"].mfcc = mfcc
  assert mods["librosa"].feature is mods["librosa.feature"]
  gen._install()
  import importlib
  for k in [k for k in sys.modules if k.startswith("open_seq2seq.data.speech2text.speech_utils")]:
    del sys.modules[k]
  su = importlib.import_module("open_seq2seq.data.speech2text.speech_utils")
  sig = np.load(gen.fixture_path("frontend"))["signal"]
  assert sig.dtype == np.int16
  out = {}
  for case, params in CASES.items():
    feats, dur = su.get_speech_features(sig.copy(), 16000, dict(params))
    out[case + "/features"] = np.asarray(feats, np.float32)
    out[case + "/duration"] = np.float64(dur)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed file")
  args = ap.parse_args()
  if not gen.reference_available():
    raise SystemExit("%s not found: fixtures can only be generated where the reference checkout is" % gen.PKG)
  out = {k: np.asarray(v) for k, v in generate().items()}
  path = gen.fixture_path(NAME)
  if args.check:
    bad = gen.compare(out, dict(np.load(path)))
    print("%s: %s" % (NAME, "reproduced" if not bad else "DIFFERS in %s" % bad))
    return int(bool(bad))
  np.savez_compressed(path, **out)
  print("%s: %d arrays, %.1f KB -> %s" % (NAME, len(out), os.path.getsize(path) / 1e3,
                                         os.path.relpath(path, gen.REPO)))
  return 0


if __name__ == "__main__":
  sys.exit(main())
