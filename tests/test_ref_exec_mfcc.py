"""The 'mfcc' yardstick (tests/_mfcc_ref.py) against the REFERENCE'S OWN CODE.

tests/golden/ref_exec_frontend_mfcc.npz = open_seq2seq/data/speech2text/speech_utils.py:get_speech_features executed
from the reference's file (tests/golden/make_ref_exec_mfcc.py) on the 0.44 s int16 signal of ref_exec_frontend.npz,
with the stand-ins of oracle/ref_shim/audio_libs for python_speech_features / librosa and librosa.feature.mfcc as
librosa 0.6.3 publishes it (scipy.fftpack.dct of the S it is given):
  psf_mfcc      backend psf, 13 coefficients, pad_to 8           -> helper within 2e-5 (the bound of the psf paths
                in tests/test_ref_exec_frontend.py; measured 2.3e-7)
  librosa_mfcc  backend librosa, 13 coefficients, num_fft 512, norm_per_feature, dither 0 -> helper within 1e-4 of a
                standard deviation (the bound of the librosa paths there; measured 4.0e-6: the stand-in returns the
                STFT as complex64 as librosa does, and scipy's DCT of the float32 S stays in single precision)
Shapes, mean ~ 0 and std ~ 1 as the reference's own unit test asserts (speech_utils_test.py:45-85)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import _mfcc_ref as mref  # noqa: E402
import make_ref_exec_mfcc as genm  # noqa: E402


def _fixtures():
  return (np.load(os.path.join(HERE, "golden", "ref_exec_frontend_mfcc.npz")),
          np.load(os.path.join(HERE, "golden", "ref_exec_frontend.npz"))["signal"])


def test_helper_reproduces_the_reference_psf_mfcc():
  d, sig = _fixtures()
  p = genm.CASES["psf_mfcc"]
  f, dur = mref.psf_mfcc(sig, 16000, p["num_audio_features"], pad_to=p["pad_to"])
  ref = d["psf_mfcc/features"]
  assert f.shape == ref.shape and ref.shape[0] % 8 == 0 and ref.shape[1] == 13
  assert ref.shape[0] == -(-(1 + -(-(len(sig) - 320) // 160)) // 8) * 8          # framesig's count, rounded up to 8
  err = float(np.abs(f - ref).max())
  print("psf mfcc: max |helper - reference| = %.2e" % err)
  assert err < 2e-5 and float(dur) == float(d["psf_mfcc/duration"])
  assert abs(float(ref.mean())) < 1e-5 and abs(float(ref.std()) - 1) < 1e-5     # global normalisation


def test_helper_reproduces_the_reference_librosa_mfcc():
  d, sig = _fixtures()
  p = genm.CASES["librosa_mfcc"]
  f, dur = mref.librosa_mfcc(sig, 16000, p["num_audio_features"], num_fft=p["num_fft"],
                             norm_per_feature=p["norm_per_feature"])
  ref = d["librosa_mfcc/features"]
  assert f.shape == ref.shape == (1 + len(sig) // 160, 13)
  err = float(np.abs(f - ref).max())
  print("librosa mfcc: max |helper - reference| = %.2e" % err)
  assert err < 1e-4 and float(dur) == float(d["librosa_mfcc/duration"])
  assert np.abs(ref.mean(0)).max() < 1e-5 and np.abs(ref.std(0) - 1).max() < 1e-5   # per-feature normalisation
  # the single-precision evaluation the device test takes its error scale from is the same function
  f32, _ = mref.librosa_mfcc(sig, 16000, 13, num_fft=512, norm_per_feature=True, dtype=np.float32)
  assert f32.dtype == np.float32 and 0 < np.abs(f32 - f).max() < 1e-4


def test_helper_dct_is_scipys():
  from scipy.fftpack import dct
  x = np.random.RandomState(3).standard_normal((7, 26))
  np.testing.assert_allclose(mref.dct2_ortho(x, 13), dct(x, type=2, axis=1, norm="ortho")[:, :13], atol=1e-12)


def test_product_tables_match_the_helper():
  """The host tables the kernels read (DCT x lifter of the psf path, the plain DCT of the librosa path)."""
  from openseq2seq_amd.data.speech2text.speech_utils import dct_ortho_table, psf_mfcc_table
  x = np.random.RandomState(4).standard_normal((5, 26))
  np.testing.assert_allclose(x.dot(psf_mfcc_table(13, 26, 26).T), mref.lifter(mref.dct2_ortho(x, 13), 26), atol=1e-12)
  s = np.random.RandomState(5).standard_normal((5, 257))
  np.testing.assert_allclose(s.dot(dct_ortho_table(13, 257).T), mref.dct2_ortho(s, 13), atol=1e-12)


@pytest.mark.skipif(not os.path.isdir("/root/reference/open_seq2seq"), reason="reference checkout not present")
def test_generator_reproduces_the_committed_fixture():
  r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_ref_exec_mfcc.py"), "--check"],
                     capture_output=True, text=True, timeout=600)
  assert r.returncode == 0 and "reproduced" in r.stdout, r.stdout + r.stderr
