"""TEST INFRASTRUCTURE: NumPy float64 restatement of the two 'mfcc' paths of the reference's ASR front end
(open_seq2seq/data/speech2text/speech_utils.py), on top of oracle/speech_features.py — this file adds only the
DCT, the lifter and the orchestration:

  psf      (:470-489, 504-515, 529-533)  int16 re-quantisation, zero padding to a multiple of pad_to frames,
           psf.mfcc(numcep=F, nfilt=2F, nfft=512, lowfreq=0, highfreq=sr/2, preemph=0.97, ceplifter=2F,
           appendEnergy=False): log filterbank energies (oracle.psf_logfbank) -> DCT-II, orthonormal, first F ->
           lifter 1 + (L/2) sin(pi n / L) -> (x - mean) / std over the whole utterance, pad frames included
  librosa  (:354-365, 383-395, 411-417)  gain, dither, pre-emphasis, S = |stft|^2, then
           librosa.feature.mfcc(S=S, n_mfcc=F, n_mels=2F) == dct(S, axis=0, type=2, norm='ortho')[:F].T (librosa
           uses a given S as it stands: no mel filter bank, no logarithm), then mean / std per feature or global.

tests/test_ref_exec_mfcc.py holds both against the reference's executed code (tests/golden/ref_exec_frontend_mfcc.npz).
librosa_mfcc(..., dtype=np.float32) evaluates the librosa path's arithmetic in single precision: its distance
from the float64 result is the error scale the device test's bound is derived from."""
import math

import numpy as np

from oracle import speech_features as osf


def dct2_ortho(x, n_out):
  """scipy.fftpack.dct(x, type=2, axis=-1, norm='ortho')[..., :n_out], as a matrix product in x's precision."""
  n = x.shape[-1]
  k = np.arange(n_out)[:, None]
  j = np.arange(n)[None, :]
  basis = np.sqrt(2.0 / n) * np.cos(np.pi * k * (2 * j + 1) / (2.0 * n))
  basis[0] /= np.sqrt(2.0)
  return np.dot(x, basis.T.astype(x.dtype))


def lifter(cepstra, L):
  n = np.arange(cepstra.shape[1])
  return (1 + (L / 2.0) * np.sin(np.pi * n / L)) * cepstra if L > 0 else cepstra


def psf_mfcc(signal, sample_freq, num_features, pad_to=8, window_size=20e-3, window_stride=10e-3):
  """(features float64 [frames, num_features], audio_duration); no augmentation."""
  signal = (osf.normalize_signal(np.asarray(signal).astype(np.float32)) * 32767.0).astype(np.int16)
  audio_duration = len(signal) * 1.0 / sample_freq
  n_window_size = int(sample_freq * window_size)
  n_window_stride = int(sample_freq * window_stride)
  length = 1 + int(math.ceil((1.0 * signal.shape[0] - n_window_size) / n_window_stride))
  if pad_to > 0 and length % pad_to != 0:
    signal = np.pad(signal, (0, (pad_to - length % pad_to) * n_window_stride), mode='constant')
  logfb = osf.psf_logfbank(signal, sample_freq, window_size, window_stride, 2 * num_features, 512, 0,
                           sample_freq / 2, 0.97)
  features = lifter(dct2_ortho(logfb, num_features), 2 * num_features)
  if pad_to > 0:
    assert features.shape[0] % pad_to == 0
  return (features - np.mean(features)) / np.std(features), audio_duration


def _stft_power_f32(y, n_fft, hop, win_length, window_fn):
  """oracle.stft_power with every operation in float32 (numpy's rfft keeps single precision)."""
  win = (window_fn(win_length) if window_fn is not None else np.ones(win_length)).astype(np.float32)
  lpad = (n_fft - win_length) // 2
  fft_window = np.zeros(n_fft, np.float32)
  fft_window[lpad:lpad + win_length] = win
  yp = np.pad(np.asarray(y, np.float32), n_fft // 2, mode="reflect")
  nfr = 1 + (len(yp) - n_fft) // hop
  idx = np.arange(n_fft)[None, :] + hop * np.arange(nfr)[:, None]
  spec = np.fft.rfft(yp[idx] * fft_window[None, :], axis=1)
  assert spec.dtype == np.complex64
  return (spec.real ** 2 + spec.imag ** 2).T


def librosa_mfcc(signal, sample_freq, num_features, window_size=20e-3, window_stride=10e-3, window_fn=np.hanning,
                 num_fft=None, norm_per_feature=False, gain=None, mean=None, std_dev=None, dtype=np.float64):
  """(features [frames, num_features] in `dtype`, audio_duration); no augmentation, dither = 0."""
  signal = osf.normalize_signal(np.asarray(signal).astype(np.float32), gain)
  audio_duration = len(signal) * 1.0 / sample_freq
  n_window_size = int(sample_freq * window_size)
  n_window_stride = int(sample_freq * window_stride)
  num_fft = num_fft or 2 ** math.ceil(math.log2(window_size * sample_freq))
  signal = osf.preemphasis(signal, coeff=0.97)
  assert signal.dtype == np.float32                 # the reference's own precision up to here
  if dtype == np.float64:
    S = osf.stft_power(signal, num_fft, n_window_stride, n_window_size, window_fn)
  else:
    S = _stft_power_f32(signal, num_fft, n_window_stride, n_window_size, window_fn)
  features = dct2_ortho(S.T, num_features)
  assert features.dtype == dtype
  norm_axis = 0 if norm_per_feature else None
  if mean is None:
    mean = np.mean(features, axis=norm_axis)
  if std_dev is None:
    std_dev = np.std(features, axis=norm_axis)
  return (features - np.asarray(mean, dtype)) / np.asarray(std_dev, dtype), audio_duration
