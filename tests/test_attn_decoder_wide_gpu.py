"""The attention decoder loop beyond its old kernel limits, against the float64 oracle: attention widths that
are any multiple of 8 up to 1024 (the backward score loop of eight unit pairs per lane, the partial last
128-block, a single 16-byte block), Luong at 1024, and source lengths whose keys do not fit LDS and are
streamed from global memory (tests/_attn_wide_cases.py says which residency every case takes). Before the
feature every case here but luong_h128_s400, whose 400 x 128 keys fit LDS, ended in OS2S_ERR_INVALID_ARG or
OS2S_ERR_UNSUPPORTED; luong_h128_s700 is that case at a length that streams.

Per case: every assertion of compare() in tests/_attn_decoder_cases.py, unchanged (exact zeros on finished
steps and past src_len, a bit-identical second backward, the forward against R, gradients cos > 0.99,
rel < 0.1 — 0.98 / 0.15 for dg_scalar — and element-wise <= 0.1 max|ref|). Cases with T <= 2 are also held
to R_b within 4 n_q + floor, n_q = max(the existing table's noise floor, the case's own max|R_b - R|), both
from the oracle alone; luong_h1024's own alignment distance (1.9e-3) is 2.9 times the existing floor.

Then: strided outputs and sample isolation, step-wise calls against one call over the range (bit-identical:
greedy and beam decoding rely on it), the two key residencies against each other (the same inputs in a source
buffer short enough to stay in LDS and in one long enough to stream: bit-identical forward outputs and
gradients), and the shapes that are still refused."""
import pytest
import torch

import _attn_decoder_cases as C
import _attn_wide_cases as W

pytestmark = pytest.mark.gpu


def _report(fails):
  assert not fails, "\n".join(fails)


def _bwd_keys(name):
  L, mode = W.ALL[name][3], W.ALL[name][7]
  return ["dkeys", "dmem", "dq_seq", "dv"] + (["dg_scalar"] if mode == 1 else []) + ["dg%d" % l for l in range(L)]


@pytest.mark.parametrize("case", sorted(W.WIDE_CASES))
def test_attn_decoder_wide(cuda, case):
  got, fails = W.check_case(case, cuda)
  L, H, M = W.ALL[case][3], W.ALL[case][4], W.ALL[case][5]
  if case in W.STRIDED:
    print(" strided run")
    st = W.run_gpu(case, cuda, strided=True, second_backward=False)
    wide = st["wide"]
    guard = torch.cat([wide[:, :, :C.GUARD], wide[:, :, C.GUARD + H + M:]], dim=2)
    if not C.same_bits(guard, torch.full_like(guard, C.SENTINEL)):
      fails.append("%s: columns outside the y_top / ctx slices changed" % case)
    keys = ["y", "ctx", "align", "dkeys", "dmem", "dq_seq"] + ["dg%d" % l for l in range(L)]
    fails += W.compare_runs(case, got, st, keys, "strided == contiguous")
  if case in W.ISOLATION:
    print(" isolation run")
    alt = W.run_gpu(case, cuda, alt_sample0=True, second_backward=False)
    keys = ["y", "ctx", "align", "dkeys", "dmem"] + ["dg%d" % l for l in range(L)]
    fails += W.compare_runs(case, got, alt, keys, "samples 1.. unchanged by sample 0", rows=slice(1, None))
    if C.same_bits(got["y"][0], alt["y"][0]):
      fails.append("%s: sample 0 did not change with its inputs" % case)
  _report(fails)


@pytest.mark.parametrize("case", W.STEPWISE)
def test_stepwise_equals_whole_range(cuda, case):
  whole, steps = W.run_forward(case, cuda, stepwise=False), W.run_forward(case, cuda, stepwise=True)
  _report(W.compare_runs(case, whole, steps, W.FWD_KEYS, "forward(t, t + 1) for every t == forward()"))


@pytest.mark.parametrize("case", sorted(W.AB_STREAMED_S))
def test_key_residency_ab(cuda, case):
  """The same inputs with the keys resident (the case's own S) and streamed (source buffers of AB_STREAMED_S
  positions, src_len unchanged): same arithmetic in the same order, so every forward output and every returned
  gradient must come out bit-identical, and exactly zero in the added positions."""
  S, S_big = W.ALL[case][2], W.AB_STREAMED_S[case]
  lds = W.run_gpu(case, cuda, second_backward=False)
  streamed = W.run_gpu_padded(case, cuda, S_big)
  fails = []
  for k in ("align", "dkeys", "dmem"):      # [B, T, S] / [B, S, .]: the source axis is the one that grew
    ax = 2 if k == "align" else 1
    head, tail = streamed[k].narrow(ax, 0, S), streamed[k].narrow(ax, S, S_big - S)
    if float(tail.float().abs().sum()) != 0.0:
      fails.append("%s: %s not zero past the case's S" % (case, k))
    streamed[k] = head.contiguous()
  keys = [k for k in list(W.FWD_KEYS) + _bwd_keys(case)]
  _report(fails + W.compare_runs(case, lds, streamed, keys, "keys streamed == keys in LDS"))


@pytest.mark.parametrize("case", sorted(W.REFUSED))
def test_still_refused(cuda, case):
  """U beyond 1024 or no multiple of 8, and location mode off U = 128: OS2S_ERR_INVALID_ARG (-1); Luong with
  U != H: OS2S_ERR_UNSUPPORTED (-3)."""
  from openseq2seq_amd import _lib
  code = W.REFUSED[case][1]
  with pytest.raises(_lib.Os2sError, match=r"os2s_attn_decoder_fwd failed: .*\(code %d\)$" % code):
    W.run_gpu(case, cuda)
