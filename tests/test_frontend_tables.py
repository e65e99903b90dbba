"""CPU: the constant tables the seven speech front ends upload (window, compact mel tables, psf filter bank, DCT
tables, given statistics) and their frame counts equal, exactly, what tests/golden/frontend_tables.npz recorded
(tests/golden/make_frontend_tables.py: the six Speech2Text front ends and the Text2Speech one on the CPU device at
16 kHz, 20 ms / 10 ms, pad_to 8)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_frontend_tables as gen  # noqa: E402

NAMES = sorted(gen.CASES) + ["tts"]
# the tables each front end must have: a missing attribute is a failure, not one comparison fewer
EXPECTED = {
    "psf_spectrogram": (),
    "psf_logfbank": ("fb",),
    "psf_mfcc": ("fb", "dctl"),
    "librosa_logfbank": ("window", "mel_start", "mel_len", "mel_wt"),
    "librosa_mfcc": ("window", "dct", "features_mean", "features_std"),
    "librosa_spectrogram": ("window", "features_mean", "features_std"),
    "tts": ("window", "mel_start", "mel_len", "mel_wt"),
}


@pytest.fixture(scope="module")
def golden():
  return np.load(gen.OUT)


@pytest.fixture(scope="module")
def built():
  return gen.tables()


def test_fixture_and_build_hold_the_same_arrays(golden, built):
  want = sorted(["%s/%s" % (n, t) for n in NAMES for t in EXPECTED[n]] + [n + "/frames" for n in NAMES])
  assert sorted(golden.files) == want
  assert sorted(built) == want


@pytest.mark.parametrize("name", NAMES)
def test_tables_equal_the_recorded_ones(golden, built, name):
  for t in EXPECTED[name]:
    key = "%s/%s" % (name, t)
    assert built[key].dtype == golden[key].dtype and built[key].shape == golden[key].shape, key
    assert np.array_equal(built[key], golden[key]), key


@pytest.mark.parametrize("name", NAMES)
def test_frame_counts_equal_the_recorded_ones(golden, built, name):
  assert len(gen.FRAME_SAMPLES) == 7
  assert np.array_equal(built[name + "/frames"], golden[name + "/frames"])
