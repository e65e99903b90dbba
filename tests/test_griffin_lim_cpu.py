"""Host side of the Griffin-Lim audio export: the float64 yardstick itself, inverse_mel / get_magnitude_spec
against a direct NumPy restatement of the reference (data/text2speech/text2speech.py:656-715,
speech_utils.py:236-284), the wav writer of save_audio, and the argument checks. No GPU."""
import struct

import numpy as np
import pytest
import torch

import _griffin_lim_ref as glr


@pytest.mark.parametrize("n_fft,T", [(64, 37), (800, 21), (1024, 9), (64, 4)])
def test_reference_round_trip(n_fft, T):
  """stft -> istft gives the signal back, the matrix form agrees with np.fft, and one projection step from the
  signal's own magnitudes and phases reproduces those magnitudes."""
  x, mag, _ = glr.make_signal(n_fft, T, 1)
  X = glr.stft(x, n_fft)
  assert X.shape == (n_fft // 2 + 1, T)
  assert glr.rel_l2(glr.istft(X, n_fft), x) <= 1e-12
  assert np.abs(glr.stft_matrix(x, n_fft) - X).max() <= 1e-10 * np.abs(X).max()
  assert glr.rel_l2(glr.istft_matrix(X, n_fft), x) <= 1e-12
  y = glr.istft(mag * glr.unit_phase(X), n_fft)
  assert glr.rel_l2(np.abs(glr.stft(y, n_fft)), mag) <= 1e-12
  assert glr.spectral_convergence(glr.griffin_lim(mag, np.angle(X) / (2 * np.pi), 2, n_fft), mag, n_fft) <= 1e-10


def test_fp32_emulation_tracks_fp64():
  for n_fft, T, bound in ((64, 37, 2e-5), (800, 21, 1e-4)):
    _, mag, ph = glr.make_signal(n_fft, T, 1)
    assert glr.rel_l2(glr.griffin_lim_fp32(mag, ph, 50, n_fft), glr.griffin_lim(mag, ph, 50, n_fft)) <= bound


def _layer(output_type, mel_type="htk", normalize=False, exp_mag=True, n_fft=64, n_mel=12, n_mag=None):
  from openseq2seq_amd.data.text2speech.text2speech import Text2SpeechDataLayer
  n_mag = n_fft // 2 + 1 if n_mag is None else n_mag
  naf = {"both": {"mel": n_mel, "magnitude": n_mag}, "mel": n_mel, "magnitude": n_mag}[output_type]
  p = {"dataset": "LJ", "n_fft": n_fft, "num_audio_features": naf, "output_type": output_type,
       "vocab_file": "missing.txt", "dataset_files": [], "dataset_location": "", "feature_normalize": normalize,
       "feature_normalize_mean": -3.0, "feature_normalize_std": 2.5, "mag_power": 2, "mel_type": mel_type,
       "data_min": {"mel": 1e-2, "magnitude": 1e-5} if output_type == "both" else 1e-5, "exp_mag": exp_mag,
       "batch_size": 2, "mode": "infer"}
  return Text2SpeechDataLayer(p, None), p


@pytest.mark.parametrize("mel_type", ["htk", "slaney"])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("output_type", ["mel", "both"])
def test_inverse_mel_matches_restatement(output_type, mel_type, normalize):
  from openseq2seq_amd.data.text2speech import speech_utils as su
  from openseq2seq_amd.data.speech2text.speech_utils import mel_basis_slaney
  dl, p = _layer(output_type, mel_type, normalize)
  assert dl.n_fft == 64 and dl.sampling_rate == 22050 and dl.max_normalization is False
  rng = np.random.RandomState(0)
  spec = rng.randn(7, 12).astype(np.float32) - 1.0
  basis = (su.mel_basis_htk if mel_type == "htk" else mel_basis_slaney)(22050, 64, 12).astype(np.float64)
  x = spec.astype(np.float64)
  if normalize:
    x = x * 2.5 - 3.0
  want = (np.exp(x) @ basis) ** 0.5
  got = dl.get_magnitude_spec(spec, is_mel=True)
  assert got.shape == (7, 33) and got.dtype == np.float64
  np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
  np.testing.assert_allclose(su.inverse_mel(x if not normalize else spec.astype(float), 22050, 64, 12, power=2.,
                                            feature_normalize=normalize, mean=-3.0, std=2.5, htk=mel_type == "htk"),
                             want, rtol=1e-12, atol=0)
  if output_type == "mel":      # a mel layer inverts whatever it is given
    np.testing.assert_allclose(dl.get_magnitude_spec(spec), want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("output_type,exp_mag", [("magnitude", False), ("both", True), ("both", False)])
def test_magnitude_spec_matches_restatement(output_type, exp_mag, normalize):
  dl, p = _layer(output_type, normalize=normalize, exp_mag=exp_mag, n_mag=29)
  rng = np.random.RandomState(1)
  spec = np.abs(rng.randn(5, 29)).astype(np.float32)
  x = spec.astype(np.float64)
  if normalize:
    x = x * 2.5 - 3.0
  pad = 1e-5 if (output_type == "both" and exp_mag) else np.log(1e-5)
  x = np.concatenate([x, np.full((5, 4), pad)], 1) / 2.0
  if output_type == "magnitude":
    x = np.exp(x)
  got = dl.get_magnitude_spec(spec)
  assert got.shape == (5, 33)
  np.testing.assert_allclose(got, x, rtol=1e-12, atol=0)


def _parse_wav(raw):
  assert raw[:4] == b"RIFF" and struct.unpack("<I", raw[4:8])[0] == len(raw) - 8 and raw[8:12] == b"WAVE"
  pos, chunks = 12, {}
  while pos < len(raw):
    tag, size = raw[pos:pos + 4], struct.unpack("<I", raw[pos + 4:pos + 8])[0]
    chunks[tag] = raw[pos + 8:pos + 8 + size]
    pos += 8 + size
  return chunks


def test_save_audio_writes_float_wav(tmp_path, monkeypatch, capsys):
  from openseq2seq_amd.models import text2speech as t2s
  rng = np.random.RandomState(2)
  signal = rng.randn(480).astype(np.float32) * 0.1
  seen = {}

  def stub(magnitudes, n_iters=50, n_fft=1024, phase=None):
    seen.update(mag=magnitudes, n_iters=n_iters, n_fft=n_fft)
    return signal.copy()

  monkeypatch.setattr(t2s, "griffin_lim", stub)
  mags = np.abs(rng.randn(31, 33)) * 3.0
  mags[0, 0], mags[1, 1] = -1.0, 300.0
  assert t2s.save_audio(mags, str(tmp_path), 12, 16000, n_fft=64, mode="eval", number=3, gl_iters=7) is None
  assert "WARNING: Eval audio was clipped at step 12" in capsys.readouterr().out
  np.testing.assert_array_equal(seen["mag"], np.clip(mags, 0, 255).T ** 1.5)
  assert seen["n_iters"] == 7 and seen["n_fft"] == 64
  chunks = _parse_wav((tmp_path / "sample_step12_3_eval.wav").read_bytes())
  tag, channels, rate, byte_rate, align, bits = struct.unpack("<HHIIHH", chunks[b"fmt "][:16])
  assert (tag, channels, rate, byte_rate, align, bits) == (3, 1, 16000, 64000, 4, 32)
  assert struct.unpack("<I", chunks[b"fact"])[0] == 480
  np.testing.assert_array_equal(np.frombuffer(chunks[b"data"], "<f4"), signal)
  # np.array format with max-normalisation; an unknown format warns and returns None
  out = t2s.save_audio(mags, str(tmp_path), 0, 16000, n_fft=64, save_format="np.array", max_normalization=True,
                       verbose=False)
  np.testing.assert_array_equal(out, signal / np.max(np.abs(signal)))
  assert t2s.save_audio(mags, str(tmp_path), 0, 16000, n_fft=64, save_format="tensorboard", verbose=False) is None
  assert "not understood" in capsys.readouterr().out


def test_argument_checks_raise_without_launching():
  from openseq2seq_amd.models.text2speech import griffin_lim_batch
  ok = torch.zeros((2, 8, 33))
  for n_fft, K in ((32, 17), (2056, 1029), (68, 35)):
    with pytest.raises(ValueError, match="n_fft must be a multiple of 8 with 64 <= n_fft <= 2048"):
      griffin_lim_batch(torch.zeros((1, 8, K)), [8], 1, n_fft)
  with pytest.raises(ValueError, match="4 <= frames"):
    griffin_lim_batch(ok, [8, 3], 1, 64)
  with pytest.raises(ValueError, match="frames <= 8"):
    griffin_lim_batch(ok, [8, 9], 1, 64)
  with pytest.raises(ValueError, match="n_fft/2 \\+ 1 = 33"):
    griffin_lim_batch(torch.zeros((2, 8, 32)), [8, 8], 1, 64)
