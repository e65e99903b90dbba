"""Every dispatch class of the attention decoder loop (os2s_attn_decoder_fwd / os2s_attn_decoder_bwd)
against the float64 oracle (oracle/attn_decoder.py). The host code picks kernels by shape: loc_split,
ad_fast_cells, ad_fast_score_bwd, cell_split (U <= 128), the ctx_parts halving on M, ceil(B / 32) batch
tiles. tests/_attn_decoder_cases.py holds the smallest shapes that reach each class:

  loc_ragged, loc_ragged_t1     location attention with finished samples (tgt_len), T = 1 with lengths
  loc_b33                       second batch tile in mode 2, the non-fast kernels at H % 64 == 0
  loc_b32_fast                  the MFMA fast path at its B limit, S = 32 + 1
  loc_k2112, loc_k2624          the fast cell launch (gx, saved gates, output dropout on the first) at M + H = 33
                                and 41 k-chunks: ti_lstm_kernel's 9 x 4 geometry with dead slots and the second
                                round of 8 x 5; the backward kernels accept both widths
  loc_b1_s1                     one sample, one position, one tap, one filter
  loc_s31, loc_s32              S padding edges of both MFMA score kernels, even filter width (K = 2)
  loc_m96 / m80 / m72           ctx_parts 4 / 2 / 1, H = 72 (no multiple of 32 or 64)
  bahd_u256_l2, gnmt_u256_l2,   the unsplit cell backward below the top layer (dgA / wAT), ad_dattn_kernel,
  luong_h256_l2                 U = 256, two batch tiles
  tiny_h8_m8                    H = M = 8
  t1_gnmt, t1_luong_h128        T = 1: only the `last` branches of the backward
  t1_luong                      Luong with U != H: OS2S_ERR_UNSUPPORTED from ad_check, by design

and test_attn_decoder_ab_switches runs the kernels that only OS2S_ATTN_SPLIT=0 / OS2S_CELL_SPLIT=0 /
OS2S_AD_FAST=0 select, one fresh process per setting.

Per case (compare() in the helper): exact zeros of finished steps and of positions past src_len, a
bit-identical second backward, the cumulative-alignment recurrence, the project's forward tolerances
against the plain fp64 result R (y, ctx atol = rtol = 3e-2; alignments atol 5e-3), the norm-wise gradient
bounds of test_attn_decoder_gpu.py (cos > 0.99, rel < 0.1) and, new, an element-wise gradient bound
max|got - ref| <= 0.1 max|ref| per tensor, which a wrong or missing element cannot hide in. Cases with
T <= 2 are also held to R_b, the oracle with a straight-through bf16 round at the kernels' bf16 stores:
|got - R_b| <= 4 n_q + floor_q, n_q = max over these cases of max|R_b.q - R.q| (one more rounding per
store than R_b doubles n_q, two stores per step double it again), floor_y = floor_ctx = one bf16 ulp of
the element (2^-7 |R_b|), floor_align = 5e-4 (512 terms x |v| <= 3 x a few fp32 ulps of tanh_fast, passed
on at most twofold by the softmax). n_q is computed at run time; observed: see N_Q_OBSERVED below.

Conditions on the inputs, checked on the CPU with the oracle alone (test_inputs_cpu): every compared
reference gradient has max|ref| > 0; for S > 1 the largest alignment weight of R is below 0.99 (over
samples with more than one source position: src_len always contains 1, and a one-position softmax is 1
by definition); every sample has a live step. Cases with dropout use seeded Bernoulli masks there, since
the library's masks need the device; the device runs repeat the same conditions on the real R.

Strided runs: y_top / ctx are column slices of one [B, T, 8 + H + M + 8] tensor filled with a sentinel.
Rows of finished steps inside the slices are zeroed first, because the ABI leaves them untouched and asks
the caller to zero the sequence buffers; live rows keep the sentinel, so a row the kernels skip shows.

The children of test_attn_decoder_ab_switches apply the same assertions, the bit-identical second backward
included, with one exemption (second_backward_judged in the helper): the two OS2S_ATTN_SPLIT=0 children
log which tensors differ between the two backward passes instead of judging them. The one-workgroup
location backward that setting selects (ad_attn_bwd_kernel<true>) adds its state gradient and its filter
gradient with LDS float atomics, so the order of the additions varies from run to run. Observed on
loc_ragged: dv, dconv_w, dconv_b and ddense_w differ in the last bits; dg, dq_seq, dkeys and dmem came out
bit-identical, though the state gradient feeds the earlier steps and they may differ as well (bf16
storage hides most of it). The split kernels replaced those atomics by ordered slabs. Against the oracle
the one-workgroup kernel passes every bound.

Found by these tests: cum_seq rows of finished steps stayed zero instead of carrying the state (the
oracle carries it: cum = cum + live * align). ad_attn_fwd_kernel and ad_loc_context_kernel returned
before writing row t + 1 for t >= tgt_len[b]; they now copy row t first."""
import os
import subprocess
import sys

import pytest
import torch

import _attn_decoder_cases as C

REPO = C.REPO
RUN = sorted(n for n in C.CASES if n not in C.UNSUPPORTED)
# n_q as test_noise_floor_cpu printed it when this file was written (float64 oracle, the T <= 2 cases); the
# tests compute their own at run time. The largest |got - R_b| on the MI355X was 1.2e-4 (y), 3.1e-5 (ctx),
# 2.5e-6 (align), and exactly zero for y / ctx in most cases.
N_Q_OBSERVED = dict(y=1.768e-3, ctx=7.793e-3, align=6.536e-4)


def _report(fails):
  assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("case", RUN)
def test_inputs_cpu(case):
  R = C.reference(case)
  _report(C.check_inputs(case, R))
  d = C.build_inputs(case)
  B, T, S = C.CASES[case][:3]
  assert 1 in d["src_len"].tolist() and S in d["src_len"].tolist()
  if d["tgt_len"] is not None:
    assert 1 in d["tgt_len"].tolist() and T in d["tgt_len"].tolist()


def test_noise_floor_cpu():
  """n_q of the tight forward bound, from R and R_b alone. It must be a bf16 rounding: above zero, and no
  more than one bf16 ulp (2^-8 relative) of the largest reference element."""
  nq = C.noise_floor()
  print("n_q", nq)
  for q in ("y", "ctx", "align"):
    top = max(float(C.reference(n)[q].abs().max()) for n in C.TIGHT)
    assert 0.0 < nq[q] <= 2.0 * 2.0 ** -8 * max(top, 1.0), (q, nq[q], top)


def test_oracle_store_default_is_identity_cpu():
  """The oracle's `store` hook changes nothing unless it is passed."""
  name = "loc_s31"
  R = C.reference(name)
  d = C.build_inputs(name)
  P = dict(wcat=[w.double() for w in d["wcat"]], bias=[None if b is None else b.double() for b in d["bias"]],
           wq=d["wq"].double(), wmem=None, v=d["v"].double(), g=None, b=None, conv_w=d["conv_w"].double(),
           conv_b=d["conv_b"].double(), dense_w=d["dense_w"].double())
  out = C.oad.attention_decoder(P, d["gx0"].double(), d["values"].double(), d["src_len"], None, None, None, 1.0,
                                "location", keys_override=d["keys"].double(), values_override=d["values"].double(),
                                store=lambda t: t)
  for q in ("y", "ctx", "align"):
    assert torch.equal(out[q], R[q]), q
  Rb = C.reference(name, rounded=True)
  assert not torch.equal(Rb["y"], R["y"])
  assert torch.equal(Rb["y"], Rb["y"].to(torch.bfloat16).double())


# ---------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", RUN)
def test_attn_decoder_paths(cuda, case):
  got, fails = C.check_case(case, cuda)
  if case in C.STRIDED:
    print(" strided run")
    st = C.run_gpu(case, cuda, strided=True, second_backward=False)
    B, T, S, L, H, M, U = C.CASES[case][:7]
    wide = st["wide"]
    guard = torch.cat([wide[:, :, :C.GUARD], wide[:, :, C.GUARD + H + M:]], dim=2)
    if not C.same_bits(guard, torch.full_like(guard, C.SENTINEL)):
      fails.append("%s: columns outside the y_top / ctx slices changed" % case)
    keys = ["y", "ctx", "align", "dkeys", "dmem", "dq_seq"] + ["dg%d" % l for l in range(L)]
    fails += C.compare_runs(case, got, st, keys, "strided == contiguous")
  if case in C.ISOLATION:
    print(" isolation run")
    alt = C.run_gpu(case, cuda, alt_sample0=True, second_backward=False)
    L = C.CASES[case][3]
    keys = ["y", "ctx", "align", "dkeys", "dmem"] + ["dg%d" % l for l in range(L)]
    fails += C.compare_runs(case, got, alt, keys, "samples 1.. unchanged by sample 0", rows=slice(1, None))
    if C.same_bits(got["y"][0], alt["y"][0]):
      fails.append("%s: sample 0 did not change with its inputs" % case)
  _report(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(C.UNSUPPORTED))
def test_attn_decoder_unsupported(cuda, case):
  """Unsupported by design: ad_check, and with it the entry point, returns OS2S_ERR_UNSUPPORTED (-3)."""
  from openseq2seq_amd import _lib
  with pytest.raises(_lib.Os2sError, match=r"os2s_attn_decoder_fwd failed: .*\(code -3\)$"):
    C.run_gpu(case, cuda)


SWITCHES = [("OS2S_ATTN_SPLIT", "loc_ragged"), ("OS2S_ATTN_SPLIT", "loc_s32"),
            ("OS2S_CELL_SPLIT", "loc_b33"), ("OS2S_CELL_SPLIT", "gnmt_u256_l2"),
            ("OS2S_AD_FAST", "loc_b32_fast")]


@pytest.mark.gpu
def test_attn_decoder_ab_switches(cuda):
  """The kernels only the A/B switches select (each switch is read once per process): one fresh child
  per setting, one at a time, stopping at the first that fails."""
  for var, case in SWITCHES:
    env = {k: v for k, v in os.environ.items() if k not in ("OS2S_ATTN_SPLIT", "OS2S_CELL_SPLIT", "OS2S_AD_FAST")}
    env[var] = "0"
    r = subprocess.run([sys.executable, "-m", "tests._attn_decoder_cases", case], env=env, timeout=120, cwd=REPO,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "%s=0 %s: exit %d\n%s" % (var, case, r.returncode, r.stdout[-6000:])
