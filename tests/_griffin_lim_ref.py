"""Yardstick for the Griffin-Lim tests (not a test module): librosa.stft / librosa.istft at their defaults and
the reference's griffin_lim (open_seq2seq/models/text2speech.py:182-198), restated from librosa's documented
behaviour with np.fft in float64, plus a float32 emulation of the same algorithm in the form the device kernels
use (float32 matrix DFT with float32 accumulation, float32 overlap-add).

librosa defaults: hop = n_fft // 4, win_length = n_fft, periodic Hann window, center=True with np.pad(mode
"reflect") of n_fft // 2 samples at each end; istft overlap-adds the windowed inverse transforms, divides by the
window sum of squares where that exceeds tiny, and trims n_fft // 2 samples from each end, which leaves
hop * (T - 1) samples for T frames. magphase returns X / |X| with 1 + 0j where |X| == 0."""
import functools

import numpy as np


def hann(n_fft):
  return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)


def frames_of(x, n_fft):
  """[T, n_fft] frames of the reflect-padded signal, T = 1 + len(x) // hop."""
  hop = n_fft // 4
  xp = np.pad(x, n_fft // 2, mode="reflect")
  T = 1 + (len(xp) - n_fft) // hop
  idx = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]
  return xp[idx]


def stft(x, n_fft):
  """float64: complex [K, T] as librosa.stft(x, n_fft)."""
  return np.fft.rfft(frames_of(np.asarray(x, np.float64), n_fft) * hann(n_fft), axis=1).T


def overlap_add(frames, n_fft, dtype):
  """frames [T, n_fft] (already windowed) -> trimmed, window-normalised signal of hop * (T - 1) samples."""
  hop = n_fft // 4
  T = frames.shape[0]
  y = np.zeros(n_fft + hop * (T - 1), dtype)
  wss = np.zeros(n_fft + hop * (T - 1), np.float64)
  w2 = hann(n_fft) ** 2
  for t in range(T):
    y[t * hop:t * hop + n_fft] += frames[t]
    wss[t * hop:t * hop + n_fft] += w2
  nz = wss > np.finfo(np.float32).tiny
  y[nz] = (y[nz] / wss[nz].astype(dtype)).astype(dtype)
  return y[n_fft // 2:len(y) - n_fft // 2]


def istft(Y, n_fft):
  """float64: signal of librosa.istft(Y) for complex Y [K, T]."""
  return overlap_add(np.fft.irfft(Y.T, n=n_fft, axis=1) * hann(n_fft), n_fft, np.float64)


def unit_phase(X):
  a = np.abs(X)
  P = np.ones_like(X)
  nz = a > 0
  P[nz] = X[nz] / a[nz]
  return P


def griffin_lim(mag, phase0, n_iters, n_fft):
  """float64 reference: mag [K, T] >= 0, phase0 [K, T] in turns."""
  mag = np.asarray(mag, np.float64)
  x = istft(mag * np.exp(2j * np.pi * np.asarray(phase0, np.float64)), n_fft)
  for _ in range(n_iters):
    x = istft(mag * unit_phase(stft(x, n_fft)), n_fft)
  return x


# ------------------------------------------------------------------------------------------------------------------
# matrix form (what a direct-DFT kernel computes) and its float32 emulation
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dft_matrices(n_fft, dtype=np.float64):
  """A [n_fft, 2K] (windowed cos | -sin) and S [2K, n_fft] (Hermitian-weighted inverse basis times the window),
  computed in float64 and rounded once to `dtype`."""
  K = n_fft // 2 + 1
  n = np.arange(n_fft)
  ang = 2 * np.pi * ((n[:, None] * np.arange(K)[None, :]) % n_fft) / n_fft
  win = hann(n_fft)
  A = np.concatenate([np.cos(ang), -np.sin(ang)], 1) * win[:, None]
  w = np.full(K, 2.0)
  w[0] = w[-1] = 1.0
  S = np.concatenate([np.cos(ang).T * w[:, None], -np.sin(ang).T * w[:, None]], 0) / n_fft * win[None, :]
  return A.astype(dtype), S.astype(dtype)


def stft_matrix(x, n_fft, dtype=np.float64):
  K = n_fft // 2 + 1
  A, _ = dft_matrices(n_fft, dtype)
  X = frames_of(np.asarray(x, dtype), n_fft) @ A
  return (X[:, :K] + 1j * X[:, K:]).T


def istft_matrix(Y, n_fft, dtype=np.float64):
  _, S = dft_matrices(n_fft, dtype)
  Yr = np.concatenate([Y.real.T, Y.imag.T], 1).astype(dtype)
  return overlap_add(Yr @ S, n_fft, dtype)


def griffin_lim_fp32(mag, phase0, n_iters, n_fft):
  """The same algorithm with every array in float32 / complex64 (librosa's own precision)."""
  mag = np.asarray(mag, np.float32)
  ph = np.asarray(phase0, np.float32)
  Y = (mag * np.cos(2 * np.pi * ph.astype(np.float64)).astype(np.float32)
       + 1j * (mag * np.sin(2 * np.pi * ph.astype(np.float64)).astype(np.float32))).astype(np.complex64)
  x = istft_matrix(Y, n_fft, np.float32)
  for _ in range(n_iters):
    X = stft_matrix(x, n_fft, np.float32).astype(np.complex64)
    x = istft_matrix((mag * unit_phase(X)).astype(np.complex64), n_fft, np.float32)
  assert x.dtype == np.float32
  return x


def rel_l2(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def spectral_convergence(x, mag, n_fft):
  """|| |STFT(x)| - M || / || M || in float64."""
  return rel_l2(np.abs(stft(x, n_fft)), mag)


def make_signal(n_fft, T, seed):
  """Seeded harmonic-plus-noise signal of hop * (T - 1) samples, its STFT magnitudes [K, T] and a phase draw."""
  rng = np.random.RandomState(seed)
  hop = n_fft // 4
  n = np.arange(hop * (T - 1))
  f0 = 0.031 + 0.01 * rng.rand()
  x = sum(a * np.sin(2 * np.pi * f0 * h * n + rng.rand() * 6.28) for h, a in ((1, 1.0), (2, 0.5), (3, 0.3), (5, 0.2)))
  x = x * (0.6 + 0.4 * np.sin(2 * np.pi * n / (7.3 * hop))) + 0.05 * rng.randn(len(n))
  mag = np.abs(stft(x, n_fft))
  return x, mag, rng.rand(*mag.shape)
