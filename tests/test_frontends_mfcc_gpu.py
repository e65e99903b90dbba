"""The three front ends added beside log-mel / psf spectrogram / psf logfbank — psf 'mfcc' (os2s_psf_mfcc), librosa
'mfcc' (os2s_librosa_mfcc) and librosa 'spectrogram' (os2s_librosa_spectrogram) — against float64 NumPy:
tests/_mfcc_ref.py for the two 'mfcc' paths (held to the reference's executed code by tests/test_ref_exec_mfcc.py),
oracle/speech_features.py for the spectrogram. Every case builds its front end with make_front_end from the
parameter dict a configuration would carry, compares the fp32 copy (want_f32) with the yardstick, and checks
separately that the bf16 output IS the round-to-nearest-even of the fp32 copy and that rows >= frames[b] are zero.

Bounds (in units of one standard deviation: the features are normalised):
  psf mfcc             2e-3, the bound of the psf 'logfbank' case of tests/test_psf_spectrogram_gpu.py — the same
                       fp32 arithmetic (int16-range samples, direct fp32 DFT, fp32 filter sums, ln) plus a 26- or
                       40-term fp32 dot product.
  librosa spectrogram  2e-3, the bound of tests/test_logmel_gpu.py.
  librosa mfcc         the DCT of a LINEAR power spectrum cancels across 257 terms, so no sibling bound applies: the
                       yardstick is the error of a float32 NumPy evaluation of the same arithmetic
                       (_mfcc_ref.librosa_mfcc(dtype=float32): float32 frames, single-precision rfft, float32 DCT
                       and statistics) against the float64 helper on the SAME batch, computed on the CPU; the
                       device may differ from float64 by 4x that. Measured on an MI355X, over the 24 cases below:
                       float32 NumPy error 3.2e-7 ... 1.1e-5 (bound 1.3e-6 ... 4.4e-5), device 1.9e-7 ... 6.6e-6,
                       never above 0.7 of the float32 error: the kernel works in fp64 after the float32 sample
                       arithmetic the reference itself has, what is left is the rounding of its fp32 copy.
Measured for the other two: psf mfcc <= 3.7e-6, librosa spectrogram <= 9.5e-7 (bounds 2e-3).
Dither is 0 in every parity case; with dither > 0 only reproducibility per seed is asserted."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mfcc_ref as mref  # noqa: E402
from oracle import speech_features as osf  # noqa: E402

pytestmark = pytest.mark.gpu

SR = 16000
WINDOWS = {"hanning": np.hanning, "hamming": np.hamming}
# psf: n_win = 320, hop = 160 — n_win - 1 (one frame, padded to 8), n_win, n_win + 1, a multiple of the hop, and not
PSF_BATCHES = {"edges": [319, 320, 321, 1600], "ragged": [2345, 1600, 321, 4000]}
# librosa: from n_fft // 2 + 1 samples (257 for the 512-point 'mfcc' transform, 161 / 201 for the spectrogram)
MFCC_BATCHES = {"edges": [257, 512, 1600, 2345], "ragged": [3000, 257, 1601, 2400]}
SPEC_BATCHES = {"edges": [201, 320, 1600, 2345], "ragged": [3000, 201, 1601, 2400]}


@functools.lru_cache(maxsize=None)
def _signals(lens, dtype):
  """Voiced-speech-like, never silent: an amplitude-modulated tone plus noise; int16 at different levels."""
  out = []
  for i, n in enumerate(lens):
    rng = np.random.RandomState(100 + i)
    t = np.arange(n) / float(SR)
    s = 0.3 * np.sin(2 * np.pi * (110 + 30 * i) * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.05 * rng.randn(n)
    s = s.astype(np.float32)
    out.append((s / np.abs(s).max() * (3000 + 4000 * i)).astype(np.int16) if dtype == "i16" else s)
  return tuple(out)


def _case(cases, case, dtype):
  """The case's parameters; a fixed gain is given for float signals in [-1, 1] and scaled for int16 PCM."""
  kw = dict(cases[case])
  if "gain" in kw and dtype == "i16":
    kw["gain"] = kw["gain"] / 8192.0
  return kw


def _run(params, sigs, seed=0, slack=100):
  """make_front_end(params) on the ragged batch (Nmax larger than every row) -> out32, out16 (as float32 bits
  of the bf16), frames, and the front end."""
  from openseq2seq_amd.data.speech2text.speech_utils import make_front_end
  dev = torch.device("cuda:0")
  lens = [len(s) for s in sigs]
  host = np.zeros((len(sigs), max(lens) + slack), sigs[0].dtype)
  for b, s in enumerate(sigs):
    host[b, :len(s)] = s
  fe = make_front_end(params, dev)
  out16, frames, out32 = fe(torch.from_numpy(host).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev),
                            max_samples=max(lens), seed=seed, want_f32=True)
  torch.cuda.synchronize()
  return out32.cpu(), out16.cpu(), frames.cpu().numpy(), fe


def _check_layout(out32, out16, frames, fe, lens):
  """bf16 == RNE(fp32 copy) exactly; zero rows past frames[b]; frames as the host computes them."""
  assert out16.dtype == torch.bfloat16 and out32.dtype == torch.float32 and out16.shape == out32.shape
  assert torch.equal(out16.view(torch.int16), out32.to(torch.bfloat16).view(torch.int16))
  assert out32.shape[1] >= int(frames.max()) and (fe.pad_to <= 0 or out32.shape[1] % fe.pad_to == 0)
  for b, n in enumerate(lens):
    assert frames[b] == fe.frames(n)
    assert not out32[b, frames[b]:].any() and not out16[b, frames[b]:].float().any()
  assert torch.isfinite(out32).all()


# ---- psf 'mfcc' --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _psf_want(lens, dtype, F, pad_to):
  return tuple(mref.psf_mfcc(s, SR, F, pad_to=pad_to)[0] for s in _signals(lens, dtype))


@pytest.mark.parametrize("dtype", ["f32", "i16"])
@pytest.mark.parametrize("batch", sorted(PSF_BATCHES))
@pytest.mark.parametrize("F,pad_to", [(13, 8), (20, 8), (13, 0)])
def test_psf_mfcc(batch, dtype, F, pad_to):
  from openseq2seq_amd.data.speech2text.speech_utils import PsfMfccFrontEnd
  lens = tuple(PSF_BATCHES[batch])
  sigs = _signals(lens, dtype)
  params = dict(sample_freq=SR, input_type="mfcc", num_audio_features=F, pad_to=pad_to)       # backend: psf
  out32, out16, frames, fe = _run(params, sigs)
  assert isinstance(fe, PsfMfccFrontEnd) and out32.shape[2] == F
  _check_layout(out32, out16, frames, fe, lens)
  worst = 0.0
  for b, want in enumerate(_psf_want(lens, dtype, F, pad_to)):
    assert frames[b] == want.shape[0] and (pad_to == 0 or frames[b] % pad_to == 0)
    worst = max(worst, float(np.abs(out32[b, :frames[b]].numpy() - want).max()))
  print("psf mfcc %s %s F=%d pad_to=%d: max |device - float64| = %.2e" % (batch, dtype, F, pad_to, worst))
  assert worst <= 2e-3


def test_psf_mfcc_long_window_is_refused():
  from openseq2seq_amd.data.speech2text.speech_utils import make_front_end
  with pytest.raises(NotImplementedError, match="32 ms"):
    make_front_end(dict(sample_freq=SR, backend="psf", input_type="mfcc", num_audio_features=13,
                        window_size=40e-3), torch.device("cuda:0"))


# ---- librosa 'mfcc' ----------------------------------------------------------------------------------------------
MFCC_CASES = {
    "20ms_per_feature": dict(window_size=20e-3, norm_per_feature=True),
    "20ms_global": dict(window_size=20e-3, norm_per_feature=False),
    "25ms_per_feature": dict(window_size=25e-3, norm_per_feature=True),
    "25ms_global_hamming": dict(window_size=25e-3, norm_per_feature=False, window="hamming"),
    "fixed_gain": dict(window_size=20e-3, norm_per_feature=True, gain=0.37),
    "given_stats": dict(window_size=20e-3, norm_per_feature=True,
                        features_mean=np.linspace(-3.0, 2.0, 13), features_std_dev=np.linspace(0.5, 4.0, 13)),
}


@functools.lru_cache(maxsize=None)
def _mfcc_want(lens, dtype, case):
  """(float64 features, float32-evaluation features) per utterance."""
  kw = _case(MFCC_CASES, case, dtype)
  args = dict(window_size=kw["window_size"], window_fn=WINDOWS[kw.get("window", "hanning")],
              norm_per_feature=kw["norm_per_feature"], gain=kw.get("gain"), mean=kw.get("features_mean"),
              std_dev=kw.get("features_std_dev"))
  return tuple((mref.librosa_mfcc(s, SR, 13, **args)[0], mref.librosa_mfcc(s, SR, 13, dtype=np.float32, **args)[0])
               for s in _signals(lens, dtype))


@pytest.mark.parametrize("dtype", ["f32", "i16"])
@pytest.mark.parametrize("batch", sorted(MFCC_BATCHES))
@pytest.mark.parametrize("case", sorted(MFCC_CASES))
def test_librosa_mfcc(batch, dtype, case):
  from openseq2seq_amd.data.speech2text.speech_utils import LibrosaMfccFrontEnd
  lens = tuple(MFCC_BATCHES[batch])
  sigs = _signals(lens, dtype)
  params = dict(sample_freq=SR, backend="librosa", input_type="mfcc", num_audio_features=13, dither=0.0,
                pad_to=16, **_case(MFCC_CASES, case, dtype))
  out32, out16, frames, fe = _run(params, sigs)
  assert isinstance(fe, LibrosaMfccFrontEnd) and fe.n_fft == 512
  _check_layout(out32, out16, frames, fe, lens)
  err32 = worst = 0.0
  for b, (want, want32) in enumerate(_mfcc_want(lens, dtype, case)):
    assert frames[b] == want.shape[0] == 1 + lens[b] // 160
    err32 = max(err32, float(np.abs(want32.astype(np.float64) - want).max()))
    worst = max(worst, float(np.abs(out32[b, :frames[b]].numpy().astype(np.float64) - want).max()))
  print("librosa mfcc %s %s %s: float32 NumPy error %.2e (bound %.2e), max |device - float64| = %.2e"
        % (batch, dtype, case, err32, 4 * err32, worst))
  assert worst <= 4 * err32


# ---- librosa 'spectrogram' ---------------------------------------------------------------------------------------
SPEC_CASES = {
    "F96": dict(num_audio_features=96),
    "F161_per_feature": dict(num_audio_features=161, norm_per_feature=True),
    "F96_25ms_hamming": dict(num_audio_features=96, window_size=25e-3, window="hamming"),
    "F96_fixed_gain": dict(num_audio_features=96, gain=0.37),
    "F96_given_stats": dict(num_audio_features=96, norm_per_feature=True,
                            features_mean=np.linspace(-60.0, -20.0, 96), features_std_dev=np.linspace(5.0, 20.0, 96)),
}


@functools.lru_cache(maxsize=None)
def _spec_want(lens, dtype, case):
  kw = _case(SPEC_CASES, case, dtype)
  return tuple(osf.get_speech_features_librosa(
      s, SR, kw["num_audio_features"], "spectrogram", kw.get("window_size", 20e-3), 10e-3,
      WINDOWS[kw.get("window", "hanning")], norm_per_feature=kw.get("norm_per_feature", False), gain=kw.get("gain"),
      mean=kw.get("features_mean"), std_dev=kw.get("features_std_dev"))[0] for s in _signals(lens, dtype))


@pytest.mark.parametrize("dtype", ["f32", "i16"])
@pytest.mark.parametrize("batch", sorted(SPEC_BATCHES))
@pytest.mark.parametrize("case", sorted(SPEC_CASES))
def test_librosa_spectrogram(batch, dtype, case):
  from openseq2seq_amd.data.speech2text.speech_utils import LibrosaSpectrogramFrontEnd
  lens = tuple(SPEC_BATCHES[batch])
  sigs = _signals(lens, dtype)
  params = dict(sample_freq=SR, backend="librosa", input_type="spectrogram", dither=0.0, pad_to=8,
                **_case(SPEC_CASES, case, dtype))
  out32, out16, frames, fe = _run(params, sigs)
  assert isinstance(fe, LibrosaSpectrogramFrontEnd)
  assert fe.n_fft == fe.win_length == int(SR * params.get("window_size", 20e-3))
  _check_layout(out32, out16, frames, fe, lens)
  worst = 0.0
  for b, want in enumerate(_spec_want(lens, dtype, case)):
    assert frames[b] == want.shape[0] == 1 + lens[b] // 160
    worst = max(worst, float(np.abs(out32[b, :frames[b]].numpy() - want).max()))
  print("librosa spectrogram %s %s %s: max |device - float64| = %.2e" % (batch, dtype, case, worst))
  assert worst <= 2e-3


def test_librosa_spectrogram_num_features_assertion():
  """speech_utils.py:377-378: F <= n_win // 2 + 1 = 161, with the reference's message; the C ABI refuses too."""
  from openseq2seq_amd import _lib, capi
  from openseq2seq_amd.data.speech2text.speech_utils import make_front_end
  dev = torch.device("cuda:0")
  with pytest.raises(AssertionError, match=r"num_features for spectrogram should be <= \(sample_freq \* window_size // 2 \+ 1\)"):
    make_front_end(dict(sample_freq=SR, backend="librosa", input_type="spectrogram", num_audio_features=162), dev)
  with pytest.raises(_lib.Os2sError):
    capi.librosa_spectrogram(torch.zeros(1, 1000, device=dev), torch.tensor([1000], dtype=torch.int32, device=dev),
                             torch.ones(320, dtype=torch.float64, device=dev), hop=160, num_features=162, tmax=7, tpad=8)


@pytest.mark.parametrize("input_type,F", [("mfcc", 13), ("spectrogram", 96)])
def test_librosa_dither_is_seeded(input_type, F):
  """dither > 0: the same seed reproduces the features bit for bit, another seed does not."""
  sigs = _signals(tuple(MFCC_BATCHES["ragged"]), "f32")
  params = dict(sample_freq=SR, backend="librosa", input_type=input_type, num_audio_features=F, dither=1e-3)
  a, _, _, _ = _run(params, sigs, seed=5)
  b, _, _, _ = _run(params, sigs, seed=5)
  c, _, _, _ = _run(params, sigs, seed=6)
  quiet, _, _, _ = _run(dict(params, dither=0.0), sigs, seed=5)
  assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, quiet)
  assert torch.isfinite(a).all() and torch.isfinite(c).all()


def test_unbuilt_combination_names_both_keys():
  from openseq2seq_amd.data.speech2text.speech_utils import make_front_end
  with pytest.raises(NotImplementedError, match=r"backend='kaldi'.*input_type='mfcc'"):
    make_front_end(dict(backend="kaldi", input_type="mfcc", num_audio_features=13), torch.device("cuda:0"))
