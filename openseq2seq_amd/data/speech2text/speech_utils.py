"""Speech feature extraction front end — host side of
open_seq2seq/data/speech2text/speech_utils.py (get_speech_features :275-319,
get_speech_features_librosa :322-441, get_speech_features_psf :444-535): one launcher class per
(backend, input_type), see FRONT_ENDS. The per-sample arithmetic runs on the GPU
(csrc/logmel.hip, csrc/librosa_features.hip, csrc/psf_features.hip); the host only prepares constant tables once:
the analysis window, the mel filterbank (what the reference precomputes with
librosa.filters.mel in speech2text.py:167-183) and the DCT matrices of the 'mfcc' paths.

librosa 0.6.3 conventions used by the reference's call sites (librosa itself is not
vendored in the reference): window passed as the CALLABLE np.hanning => symmetric
Hann of win_length, zero-padded centred to n_fft; filters.mel defaults htk=False,
norm=1 => Slaney mel scale with area normalisation.
"""
from __future__ import absolute_import, division, print_function

import math

import numpy as np
import torch

from ... import capi

WINDOWS_FNS = {"hanning": np.hanning, "hamming": np.hamming, "none": None}


def _hz_to_mel(f):
  f = np.asanyarray(f, dtype=np.float64)
  f_sp, min_log_hz = 200.0 / 3, 1000.0
  logstep = np.log(6.4) / 27.0
  return np.where(f >= min_log_hz,
                  min_log_hz / f_sp + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep,
                  f / f_sp)


def _mel_to_hz(m):
  m = np.asanyarray(m, dtype=np.float64)
  f_sp, min_log_hz = 200.0 / 3, 1000.0
  min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
  return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_basis_slaney(sample_freq, n_fft, n_mels, fmin=0.0, fmax=None):
  """Equivalent of librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) (htk=False, norm=1)."""
  fmax = sample_freq / 2.0 if fmax is None else fmax
  fftfreqs = np.linspace(0, sample_freq / 2.0, 1 + n_fft // 2)
  mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
  fdiff = np.diff(mel_f)
  ramps = np.subtract.outer(mel_f, fftfreqs)
  w = np.zeros((n_mels, 1 + n_fft // 2))
  for i in range(n_mels):
    w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
  w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
  return w.astype(np.float32)


def compact_mel_tables(basis):
  """A [n_mels, n_bins] mel basis as the kernels read it: per filter the first non-zero bin and the length of its
  support (int32 [n_mels] each), and the weights of that support, [max length, n_mels] float32, zero padded."""
  n_mels = basis.shape[0]
  starts, lens = np.zeros(n_mels, np.int32), np.zeros(n_mels, np.int32)
  for m in range(n_mels):
    nz = np.nonzero(basis[m])[0]
    if len(nz):
      starts[m], lens[m] = nz[0], nz[-1] - nz[0] + 1
  wt = np.zeros((max(int(lens.max()), 1), n_mels), np.float32)
  for m in range(n_mels):
    wt[:lens[m], m] = basis[m, starts[m]:starts[m] + lens[m]]
  return starts, lens, wt


def psf_frame_count(n, n_win, n_step, pad_to):
  """Frames of an n-sample utterance on the psf paths, as psf_frame_count of csrc/speech_frontend.hpp:
  (1 + ceil((n - n_win) / n_step), at least one; that count rounded up to a multiple of pad_to)."""
  live = 1 if n <= n_win else 1 + -(-(n - n_win) // n_step)
  rem = live % pad_to if pad_to > 0 else 0
  return live, (live + pad_to - rem if rem else live)


class _FrontEnd(object):
  """What every launcher shares: the parameters of get_speech_features (speech_utils.py:289-311) that all paths
  read, the (backend, input_type) check, and the frame counts of a batch. A front end is called as
  fe(signal [B,Nmax] float32|int16 (device), n_samples int32 [B] (device), max_samples = host max(n_samples), which
  avoids a device sync and defaults to Nmax) -> (features bf16 [B,Tpad,F], frames int32 [B], fp32 copy or None)."""
  backend = input_type = None

  def __init__(self, params, device):
    self.device = device
    self.sample_freq = sr = params.get('sample_freq', 16000)
    if (params.get('backend', 'psf'), params.get('input_type')) != (self.backend, self.input_type):
      raise NotImplementedError("%s implements backend='%s', input_type='%s'"
                                % (type(self).__name__, self.backend, self.input_type))
    self.num_features = params['num_audio_features']
    self.win_length = int(sr * params.get('window_size', 20e-3))
    self.hop = int(sr * params.get('window_stride', 10e-3))
    self.pad_to = params.get('pad_to', 8)

  def _shape(self, signal, max_samples):
    """(tmax, tpad): the frames of the longest utterance, and that count rounded up to pad_to."""
    tmax = self.frames(int(max_samples) if max_samples is not None else signal.shape[1])
    return tmax, (-(-tmax // self.pad_to) * self.pad_to if self.pad_to > 0 else tmax)


class _PsfFrontEnd(_FrontEnd):
  """The python_speech_features backend (get_speech_features_psf, speech_utils.py:444-535): frames() includes the
  pad_to rounding; dither / gain / norm_per_feature do not exist on these paths."""
  backend = 'psf'
  nfft = 512          # psf.logfbank / psf.mfcc are called with nfft = 512

  def __init__(self, params, device):
    super(_PsfFrontEnd, self).__init__(params, device)
    self.gain = None
    self._tables(device)

  def _filterbank(self, nfilt, device):
    if self.win_length > self.nfft:
      raise NotImplementedError("psf.%s truncates frames longer than nfft = 512 (window_size > 32 ms)"
                                % self.input_type)
    fb = psf_filterbanks(nfilt, self.nfft, self.sample_freq, 0.0, self.sample_freq / 2.0)
    self.fb = torch.from_numpy(np.ascontiguousarray(fb, np.float32)).to(device)

  def frames(self, n_samples):
    return psf_frame_count(int(n_samples), self.win_length, self.hop, self.pad_to)[1]

  def _psf_args(self, signal, max_samples, want_f32):
    return dict(n_win=self.win_length, n_step=self.hop, pad_to=self.pad_to, tpad=self._shape(signal, max_samples)[1],
                want_f32=want_f32)


class PsfSpectrogramFrontEnd(_PsfFrontEnd):
  """Launcher for the 'spectrogram' features of the python_speech_features backend (the DeepSpeech2 configs)."""
  input_type = 'spectrogram'

  def _tables(self, device):
    if self.num_features > self.win_length // 2 + 1:        # speech_utils.py:501-502
      raise AssertionError("num_features for spectrogram should be <= (sample_freq * window_size // 2 + 1)")

  def __call__(self, signal, n_samples, max_samples=None, seed=0, want_f32=False):
    return capi.psf_spectrogram(signal, n_samples, num_features=self.num_features,
                                **self._psf_args(signal, max_samples, want_f32))


def psf_filterbanks(nfilt, nfft, samplerate, lowfreq=0.0, highfreq=None):
  """python_speech_features.get_filterbanks (0.6): nfilt triangular filters on the HTK mel scale
  (2595 log10(1 + f / 700)), corner bins floor((nfft + 1) * hz / samplerate), unnormalised: [nfilt, nfft/2 + 1]."""
  highfreq = highfreq or samplerate / 2.0
  hz2mel = lambda hz: 2595.0 * np.log10(1.0 + hz / 700.0)
  mel2hz = lambda mel: 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
  melpoints = np.linspace(hz2mel(lowfreq), hz2mel(highfreq), nfilt + 2)
  bins = np.floor((nfft + 1) * mel2hz(melpoints) / samplerate)
  fb = np.zeros([nfilt, nfft // 2 + 1])
  for j in range(nfilt):
    for i in range(int(bins[j]), int(bins[j + 1])):
      fb[j, i] = (i - bins[j]) / (bins[j + 1] - bins[j])
    for i in range(int(bins[j + 1]), int(bins[j + 2])):
      fb[j, i] = (bins[j + 2] - i) / (bins[j + 2] - bins[j + 1])
  return fb


class PsfLogfbankFrontEnd(PsfSpectrogramFrontEnd):
  """Launcher for the 'logfbank' features of the python_speech_features backend (get_speech_features_psf,
  speech_utils.py:517-535: psf.logfbank with nfft = 512, preemph = 0.97; the toy Wave2Letter / TDNN test
  configurations). Framing and padding as the spectrogram path."""
  input_type = 'logfbank'

  def _tables(self, device):
    self._filterbank(self.num_features, device)

  def __call__(self, signal, n_samples, max_samples=None, seed=0, want_f32=False):
    return capi.psf_logfbank(signal, n_samples, self.fb, nfft=self.nfft,
                             **self._psf_args(signal, max_samples, want_f32))


def dct_ortho_table(n_out, n_in):
  """scipy.fftpack.dct(x, type=2, norm='ortho') over n_in points, first n_out coefficients: [n_out, n_in]."""
  m = np.arange(n_out)[:, None]
  j = np.arange(n_in)[None, :]
  d = np.sqrt(2.0 / n_in) * np.cos(np.pi * m * (2 * j + 1) / (2.0 * n_in))
  d[0] *= np.sqrt(0.5)
  return d


def psf_mfcc_table(numcep, nfilt, ceplifter):
  """What psf.mfcc applies to the nfilt log filterbank energies of a frame, as one [numcep, nfilt] matrix: the
  orthonormal DCT-II along the filters, the first numcep coefficients, then psf.lifter: coefficient m times
  1 + (L / 2) sin(pi m / L)."""
  d = dct_ortho_table(numcep, nfilt)
  if ceplifter > 0:
    d *= 1.0 + (ceplifter / 2.0) * np.sin(np.pi * np.arange(numcep)[:, None] / ceplifter)
  return d


class PsfMfccFrontEnd(PsfLogfbankFrontEnd):
  """Launcher for the 'mfcc' features of the python_speech_features backend (get_speech_features_psf,
  speech_utils.py:504-515: psf.mfcc with numcep = F, nfilt = 2F, nfft = 512, preemph = 0.97, ceplifter = 2F,
  appendEnergy = False, rectangular window; example_configs/speech2text/lstm_small_1gpu.py). Framing and padding
  as the other psf paths."""
  input_type = 'mfcc'

  def _tables(self, device):
    nfilt = 2 * self.num_features
    self._filterbank(nfilt, device)
    dctl = psf_mfcc_table(self.num_features, nfilt, nfilt)
    self.dctl = torch.from_numpy(np.ascontiguousarray(dctl, np.float32)).to(device)

  def __call__(self, signal, n_samples, max_samples=None, seed=0, want_f32=False):
    return capi.psf_mfcc(signal, n_samples, self.fb, self.dctl, nfft=self.nfft,
                         **self._psf_args(signal, max_samples, want_f32))


class _LibrosaFrontEnd(_FrontEnd):
  """The librosa backend (get_speech_features_librosa, speech_utils.py:322-441): a centred STFT (frame count
  1 + n // hop) with the window_fn(win_length) window zero-padded centred to n_fft, dither, gain, and the
  normalisation options."""
  backend = 'librosa'
  window_dtype = np.float64

  def __init__(self, params, device):
    super(_LibrosaFrontEnd, self).__init__(params, device)
    self.n_fft = self._transform_length(params, params.get('window_size', 20e-3) * self.sample_freq)
    self.dither = params.get('dither', 0.0)
    self.norm_per_feature = params.get('norm_per_feature', False)
    self.gain = params.get('gain', None)
    wfn = WINDOWS_FNS[params.get('window', 'hanning')]
    full = np.zeros(self.n_fft, self.window_dtype)
    lp = (self.n_fft - self.win_length) // 2
    full[lp:lp + self.win_length] = wfn(self.win_length) if wfn is not None else np.ones(self.win_length)
    self.window = torch.from_numpy(full).to(device)
    self.features_mean = self._given(params.get('features_mean'))
    self.features_std = self._given(params.get('features_std_dev'))

  def _transform_length(self, params, win):
    return params.get('num_fft', None) or 2 ** math.ceil(math.log2(win))

  def _given(self, value):
    if value is None:
      return None
    full = np.array(np.broadcast_to(np.asarray(value, np.float64), (self.num_features,)))
    return torch.from_numpy(full).to(self.device)

  def frames(self, n_samples):
    return 1 + int(n_samples) // self.hop

  def _common(self, signal, max_samples, seed, want_f32):
    tmax, tpad = self._shape(signal, max_samples)
    return dict(hop=self.hop, tmax=tmax, tpad=tpad, dither=self.dither, seed=seed,
                fixed_gain=self.gain if self.gain is not None else -1.0, norm_per_feature=self.norm_per_feature,
                want_f32=want_f32)

  def _stats(self):
    return dict(features_mean=self.features_mean, features_std=self.features_std)


class LogMelFrontEnd(_LibrosaFrontEnd):
  """Constant tables + launcher for the 'logfbank' features of the librosa backend (the Jasper configs; params as
  in speech_utils.get_speech_features :275-306): the FFT path of csrc/logmel.hip, which reads a float32 window and
  the compact tables of the mel basis (params['mel_basis'], or librosa.filters.mel's)."""
  input_type = 'logfbank'
  window_dtype = np.float32

  def __init__(self, params, device):
    super(LogMelFrontEnd, self).__init__(params, device)
    self.n_mels = self.num_features
    basis = params.get('mel_basis', None)
    if basis is None:
      basis = mel_basis_slaney(self.sample_freq, self.n_fft, self.n_mels, 0, int(self.sample_freq / 2))
    self.mel_basis = np.asarray(basis, np.float32)
    self.mel_start, self.mel_len, self.mel_wt = (torch.from_numpy(t).to(device)
                                                 for t in compact_mel_tables(self.mel_basis))

  def __call__(self, signal, n_samples, max_samples=None, seed=0, want_f32=False):
    return capi.logmel(signal, n_samples, self.window, self.mel_start, self.mel_len, self.mel_wt,
                       n_mels=self.n_mels, n_fft=self.n_fft, **self._common(signal, max_samples, seed, want_f32))


class LibrosaMfccFrontEnd(_LibrosaFrontEnd):
  """Launcher for the 'mfcc' features of the librosa backend (get_speech_features_librosa, speech_utils.py:383-395).
  The reference hands librosa.feature.mfcc the LINEAR power STFT as S; librosa uses a given S as it stands (the mel
  filter bank and the dB conversion run only when S is None, n_mels is ignored), so the features are
  dct(S, axis=0, type=2, norm='ortho')[:F].T — the DCT-II along the n_fft / 2 + 1 frequency bins of the power
  spectrum, with no mel scale and no logarithm. This class reproduces that."""
  input_type = 'mfcc'

  def __init__(self, params, device):
    super(LibrosaMfccFrontEnd, self).__init__(params, device)
    self.dct = torch.from_numpy(dct_ortho_table(self.num_features, self.n_fft // 2 + 1)).to(device)

  def __call__(self, signal, n_samples, max_samples=None, seed=0, want_f32=False):
    return capi.librosa_mfcc(signal, n_samples, self.window, self.dct, win_length=self.win_length,
                             **self._common(signal, max_samples, seed, want_f32), **self._stats())


class LibrosaSpectrogramFrontEnd(_LibrosaFrontEnd):
  """Launcher for the 'spectrogram' features of the librosa backend (speech_utils.py:367-381): no pre-emphasis,
  stft(n_fft = win_length = int(sr * window_size)), 10 log10 of the power clamped at 1e-30, the first F bins."""
  input_type = 'spectrogram'

  def _transform_length(self, params, win):
    return self.win_length

  def __init__(self, params, device):
    super(LibrosaSpectrogramFrontEnd, self).__init__(params, device)
    if self.num_features > self.win_length // 2 + 1:        # speech_utils.py:377-378
      raise AssertionError("num_features for spectrogram should be <= (sample_freq * window_size // 2 + 1)")

  def __call__(self, signal, n_samples, max_samples=None, seed=0, want_f32=False):
    return capi.librosa_spectrogram(signal, n_samples, self.window, num_features=self.num_features,
                                    **self._common(signal, max_samples, seed, want_f32), **self._stats())


FRONT_ENDS = {
    ('psf', 'spectrogram'): PsfSpectrogramFrontEnd,        # DeepSpeech2
    ('psf', 'logfbank'): PsfLogfbankFrontEnd,              # the toy Wave2Letter configs
    ('psf', 'mfcc'): PsfMfccFrontEnd,                      # lstm_small_1gpu.py
    ('librosa', 'logfbank'): LogMelFrontEnd,               # Jasper, QuartzNet, Wave2Letter+
    ('librosa', 'mfcc'): LibrosaMfccFrontEnd,
    ('librosa', 'spectrogram'): LibrosaSpectrogramFrontEnd,
}


def front_end_class(params):
  """The front-end class of a Speech2TextDataLayer configuration, by (backend, input_type)."""
  key = (params.get('backend', 'psf'), params.get('input_type'))
  if key not in FRONT_ENDS:
    raise NotImplementedError("no GPU front end for backend=%r, input_type=%r" % key)
  return FRONT_ENDS[key]


def make_front_end(params, device):
  """The GPU front end of a Speech2TextDataLayer configuration."""
  return front_end_class(params)(params, device)


# ---- speed perturbation filter (resampy 'kaiser_best') --------------------------------------------
KAISER_BEST = dict(num_zeros=64, precision=9, rolloff=0.9475937167399596, beta=14.769656459379492)


def sinc_window(num_zeros=64, precision=9, rolloff=0.945, beta=14.769656459379492):
  """resampy.filters.sinc_window with a Kaiser taper: the right half of the band-limited
  interpolation filter, num_zeros * 2^precision + 1 taps (resampy's published construction;
  'kaiser_best' = KAISER_BEST). Returns (interp_win float32, num_table = 2^precision)."""
  num_bits = 2 ** precision
  n = num_bits * num_zeros
  sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
  taper = np.kaiser(2 * n + 1, beta)[n:]
  return (taper * sinc_win).astype(np.float32), num_bits


def read_wav(filename):
  """scipy.io.wavfile.read as used by get_speech_features_from_file (speech_utils.py:186-196):
  (sample_freq, int16 / float32 mono signal)."""
  from scipy.io import wavfile
  sample_freq, signal = wavfile.read(filename)
  if signal.ndim > 1:
    signal = signal[:, 0]
  return sample_freq, signal
