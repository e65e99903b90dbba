"""Helper of tests/test_attn_decoder_paths_gpu.py (not a test module): the case table that reaches every
dispatch class of os2s_attn_decoder_fwd / os2s_attn_decoder_bwd, the device run, the fp64 oracle run and
the comparison of the two.

  python -m tests._attn_decoder_cases CASE

runs one case on cuda:0, applies the assertions of compare() and exits non-zero on a mismatch (the A/B
switches OS2S_ATTN_SPLIT / OS2S_CELL_SPLIT / OS2S_AD_FAST are read when the library is loaded, so a setting given
through the environment needs a process of its own). One assertion has an exemption, see second_backward_judged().

Both sides consume the same bf16-rounded parameters and inputs and the same dropout masks. The oracle
runs in float64, once plainly (R) and, for the tight forward bound, once with a straight-through bf16
round at the places where the kernels store bf16 (R_b).

Kernels each case launches, read off the host predicates (every case also: ad_dkeys, ad_dvalues,
ad_score_vec_grads; every location case also: ad_fold_location, ad_unfold_location_grads):
  loc_ragged, loc_b33, loc_m96, loc_m80, loc_m72
      ad_cell_fwd, ad_loc_scores, ad_loc_context | ad_loc_dalign, ad_loc_score_bwd, ad_cell_bwd_split,
      ad_dattn_split (loc_ragged_t1: the same without ad_dattn_split, which needs a step t + 1)
  loc_b32_fast, loc_b1_s1, loc_s31, loc_s32
      ti_lstm, ad_loc_scores_mfma, ad_loc_context | ad_loc_dalign, ad_loc_score_bwd_mfma,
      ad_cell_bwd_split, ad_dattn_split
  loc_k2112, loc_k2624
      the same as loc_b32_fast, with ti_lstm in its 9 x 4 / two-round 8 x 5 geometry for layer 0
  bahd_u256_l2, gnmt_u256_l2, luong_h256_l2
      ad_cell_fwd, ad_attn_fwd | ad_attn_bwd<false>, ad_cell_bwd (both layers: dgA / wAT below the top),
      ad_dattn
  tiny_h8_m8      ad_cell_fwd, ad_attn_fwd | ad_attn_bwd<false>, ad_cell_bwd_split, ad_dattn_split
  t1_gnmt, t1_luong_h128
      ad_cell_fwd, ad_attn_fwd | ad_attn_bwd<false>, ad_cell_bwd_split
  OS2S_ATTN_SPLIT=0 loc_ragged, loc_s32
      ad_cell_fwd, ad_attn_fwd (mode 2) | ad_attn_bwd<true>, ad_cell_bwd_split, ad_dattn_split
  OS2S_CELL_SPLIT=0 loc_b33
      forward as above | ad_loc_dalign, ad_loc_score_bwd, ad_cell_bwd (L = 2), ad_dattn
  OS2S_AD_FAST=0 loc_b32_fast
      ad_cell_fwd, ad_loc_scores, ad_loc_context | ad_loc_dalign, ad_loc_score_bwd, ad_cell_bwd_split,
      ad_dattn_split"""
import functools
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
  sys.path.insert(0, REPO)

from oracle import attn_decoder as oad  # noqa: E402

CASES = {
    # name: B, T, S, L, H, M, U, mode, loc_k, loc_f, use_bias, attn_in_keep, out_keep, ragged_tgt
    "loc_ragged": (5, 6, 19, 2, 64, 64, 128, 2, 5, 4, True, 1.0, 0.9, True),
    "loc_ragged_t1": (3, 1, 9, 1, 64, 64, 128, 2, 3, 2, False, 1.0, 1.0, True),
    "loc_b33": (33, 3, 17, 2, 64, 64, 128, 2, 3, 4, False, 1.0, 1.0, False),
    "loc_b32_fast": (32, 2, 33, 2, 64, 64, 128, 2, 7, 8, False, 1.0, 1.0, False),
    "loc_b1_s1": (1, 2, 1, 1, 64, 64, 128, 2, 1, 1, False, 1.0, 1.0, False),
    "loc_s31": (3, 2, 31, 2, 64, 64, 128, 2, 2, 3, False, 1.0, 1.0, False),
    "loc_s32": (3, 2, 32, 2, 64, 64, 128, 2, 2, 3, False, 1.0, 1.0, False),
    "loc_m96": (4, 2, 21, 1, 72, 96, 128, 2, 5, 4, False, 1.0, 1.0, False),
    "loc_m80": (4, 2, 21, 1, 72, 80, 128, 2, 5, 4, False, 1.0, 1.0, False),
    "loc_m72": (4, 2, 21, 1, 72, 72, 128, 2, 5, 4, False, 1.0, 1.0, False),
    # ad_launch_fast_cell (gx, saved gates, output dropout) at ti_geom()'s wider classes: Kc = M + H = 2112 is 33
    # chunks (9 x 4 with three dead slots), 2624 is 41 (8 x 5, a second round holding one live chunk)
    "loc_k2112": (17, 2, 9, 2, 64, 2048, 128, 2, 5, 4, False, 1.0, 0.9, False),
    "loc_k2624": (17, 2, 9, 2, 64, 2560, 128, 2, 5, 4, False, 1.0, 1.0, False),
    "bahd_u256_l2": (33, 3, 13, 2, 64, 64, 256, 0, 0, 0, False, 1.0, 0.9, False),
    "gnmt_u256_l2": (5, 4, 13, 2, 64, 128, 256, 1, 0, 0, False, 0.8, 1.0, True),
    "luong_h256_l2": (4, 3, 10, 2, 256, 64, 256, 3, 0, 0, False, 1.0, 1.0, True),
    "tiny_h8_m8": (2, 2, 5, 1, 8, 8, 128, 0, 0, 0, False, 1.0, 1.0, False),
    "t1_gnmt": (4, 1, 7, 1, 64, 64, 128, 1, 0, 0, False, 1.0, 1.0, False),
    "t1_luong": (4, 1, 7, 1, 64, 64, 128, 3, 0, 0, False, 1.0, 1.0, False),
    "t1_luong_h128": (4, 1, 7, 1, 128, 64, 128, 3, 0, 0, False, 1.0, 1.0, False),
}
# Luong attention scores keys . (cell output): U != H is unsupported by design, and ad_check says so with
# OS2S_ERR_UNSUPPORTED. t1_luong_h128 is the same case at a width the mode accepts.
UNSUPPORTED = ("t1_luong",)
# target lengths the issue fixes; other ragged cases draw theirs (always containing 1 and T)
TGT_LEN = {"loc_ragged": [6, 1, 3, 6, 2], "loc_ragged_t1": [1, 1, 1]}
SEED = {}                              # per-case seed override (default: sum of the name's code points)
# attention vector scale (default 1.0): lowered until the largest alignment weight of R is below 0.99, so
# that the softmax backward is exercised (33 samples with two-position sources saturate at unit scale)
V_SCALE = {"loc_ragged": 0.5, "loc_ragged_t1": 0.5, "loc_b33": 0.1, "loc_b32_fast": 0.2, "loc_s31": 0.5,
           "loc_m96": 0.5, "loc_m80": 0.2, "bahd_u256_l2": 0.07, "loc_k2112": 0.1, "loc_k2624": 0.1}
MODES = {0: "bahdanau", 1: "bahdanau_norm", 2: "location", 3: "luong"}
STRIDED = tuple(n for n in CASES if n.startswith("loc_")) + ("bahd_u256_l2",)
ISOLATION = ("loc_b33", "bahd_u256_l2")
# T <= 2 and no dropout: the forward is also held to R_b
TIGHT = tuple(n for n in CASES if CASES[n][1] <= 2 and CASES[n][11] == 1.0 and CASES[n][12] == 1.0 and n not in UNSUPPORTED)
ATTN_IN_SEED, OUT_SEEDS = 77, (101, 202)
SENTINEL = -7.0                        # fill of the wider [B, T, 8 + H + M + 8] tensor of the strided runs
GUARD = 8


def _bf(t):
  return t.to(torch.bfloat16)


class _RoundBf16(torch.autograd.Function):
  """bf16 round of the value; the gradient passes through unchanged."""

  @staticmethod
  def forward(ctx, x):
    return x.to(torch.bfloat16).to(x.dtype)

  @staticmethod
  def backward(ctx, g):
    return g


def round_bf16(x):
  return _RoundBf16.apply(x)


@functools.lru_cache(maxsize=None)
def build_inputs(name):
  """bf16-rounded parameters and inputs of a case from a seeded CPU generator (CPU tensors)."""
  B, T, S, L, H, M, U, mode, K, F, use_bias, a_keep, o_keep, ragged = CASES[name]
  g = torch.Generator().manual_seed(SEED.get(name, sum(map(ord, name))))
  rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
  kc = [M + H, 2 * H]
  d = dict(name=name)
  d["wcat"] = [_bf(rn(4 * H, kc[l], sc=1.0 / math.sqrt(kc[l]))) for l in range(L)]
  d["bias"] = [None] + [rn(4 * H, sc=0.1) for _ in range(L - 1)]
  d["wq"] = _bf(rn(U, H, sc=1.0 / math.sqrt(H))) if mode != 3 else torch.eye(U).to(torch.bfloat16)
  wmem = _bf(rn(U, M, sc=1.0 / math.sqrt(M)))
  d["v"] = rn(U, sc=V_SCALE.get(name, 1.0))
  d["g"] = torch.tensor([1.3]) if mode == 1 else None
  d["b"] = rn(U, sc=0.1) if (mode == 1 or use_bias) else None
  d["conv_w"] = rn(K, F, sc=0.5) if mode == 2 else None
  d["conv_b"] = rn(F, sc=0.1) if mode == 2 else None
  d["dense_w"] = rn(F, U, sc=0.3) if mode == 2 else None
  d["gx0"] = _bf(rn(B, T, 4 * H, sc=0.7))
  memory = _bf(rn(B, S, M, sc=1.0))
  src_len = torch.randint(1, S + 1, (B,), generator=g, dtype=torch.int32)
  src_len[0] = S
  src_len[B - 1] = 1 if B > 1 else S
  tgt_len = None
  if name in TGT_LEN:
    tgt_len = torch.tensor(TGT_LEN[name], dtype=torch.int32)
  elif ragged:
    tgt_len = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    tgt_len[0] = T
    tgt_len[1] = 1
  d["src_len"], d["tgt_len"] = src_len, tgt_len
  d["dy"] = _bf(rn(B, T, H, sc=1.0))
  d["dctx"] = _bf(rn(B, T, M, sc=1.0))
  values_h, _ = oad.prepare_memory(memory.float(), src_len)
  d["values"] = _bf(values_h)
  d["keys"] = _bf(d["values"].float() @ wmem.float().t())
  # replacement of sample 0 for the isolation rerun
  d["gx0_alt"] = _bf(rn(T, 4 * H, sc=0.7))
  mem_alt = _bf(rn(S, M, sc=1.0))
  d["values_alt"] = mem_alt.clone()
  d["values_alt"][int(src_len[0]):] = 0
  d["keys_alt"] = _bf(d["values_alt"].float() @ wmem.float().t())
  assert int(src_len.min()) == 1 and int(src_len.max()) == S
  assert tgt_len is None or (int(tgt_len.min()) == 1 and int(tgt_len.max()) == T)
  return d


def live_steps(name):
  B, T = CASES[name][:2]
  tl = build_inputs(name)["tgt_len"]
  return torch.ones(B, T, dtype=torch.bool) if tl is None else (torch.arange(T)[None, :] < tl[:, None])


def dropout_masks(name, device):
  """(attention-input mask [B,T,M] or None, list of L output masks [B,T,H] or None), float64, scaled by
  1/keep. With a device: the library's own masks (capi.dropout_mask), the ones the kernels apply. Without
  (CPU-only checks of the inputs): seeded Bernoulli masks of the same keep probability."""
  B, T, S, L, H, M, U, mode, K, F, use_bias, a_keep, o_keep, ragged = CASES[name]
  if device is None:
    g = torch.Generator().manual_seed(1234 + sum(map(ord, name)))
    draw = lambda shape, keep: (torch.rand(*shape, generator=g) < keep).double() / keep
    amask = draw((B, T, M), a_keep) if a_keep < 1.0 else None
    omasks = [draw((B, T, H), o_keep) for _ in range(L)] if o_keep < 1.0 else None
    return amask, omasks
  from openseq2seq_amd import capi
  amask = omasks = None
  if a_keep < 1.0:
    m = capi.dropout_mask(ATTN_IN_SEED, B * (T + 1) * M, a_keep, device).view(B, T + 1, M).double().cpu() / a_keep
    amask = m[:, :T]       # row t multiplies attention_{t-1}
  if o_keep < 1.0:
    omasks = [capi.dropout_mask(sd, B * T * H, o_keep, device).view(B, T, H).double().cpu() / o_keep
              for sd in OUT_SEEDS[:L]]
  return amask, omasks


_REF_CACHE = {}


def reference(name, rounded=False, device=None):
  """The fp64 oracle on the case's rounded tensors: dict(y, ctx, align[, grads]) — R (rounded=False, with
  the autograd gradients of sum(y dy) + sum(ctx dctx)) or R_b (rounded=True, forward only). Computed once
  per (case, rounded, own / stand-in masks); callers must not modify the result."""
  B, T, S, L, H, M, U, mode, K, F, use_bias, a_keep, o_keep, ragged = CASES[name]
  has_dropout = a_keep < 1.0 or o_keep < 1.0        # without dropout there are no masks to tell apart
  key = (name, rounded, has_dropout and device is None)
  if key in _REF_CACHE:
    return _REF_CACHE[key]
  d = build_inputs(name)
  amask, omasks = dropout_masks(name, device)
  leaf = lambda t: None if t is None else t.double().clone().requires_grad_(not rounded)
  P = dict(wcat=[leaf(w) for w in d["wcat"]], bias=[leaf(b) for b in d["bias"]], wq=leaf(d["wq"]),
           wmem=None, v=leaf(d["v"]), g=leaf(d["g"]), b=leaf(d["b"]), conv_w=leaf(d["conv_w"]),
           conv_b=leaf(d["conv_b"]), dense_w=leaf(d["dense_w"]))
  gx0, vals, keys = leaf(d["gx0"]), leaf(d["values"]), leaf(d["keys"])
  out = oad.attention_decoder(P, gx0, d["values"].double(), d["src_len"], d["tgt_len"], amask, omasks, 1.0,
                              MODES[mode], keys_override=keys, values_override=vals,
                              store=round_bf16 if rounded else None)
  R = dict(y=out["y"].detach(), ctx=out["ctx"].detach(), align=out["align"].detach())
  if not rounded:
    loss = (out["y"] * d["dy"].double()).sum() + (out["ctx"] * d["dctx"].double()).sum()
    loss.backward()
    G = dict(dg0=gx0.grad, dvalues=vals.grad, dkeys=keys.grad)
    if mode != 3:
      G["dv"] = P["v"].grad
      G["dwq"] = P["wq"].grad
    if mode == 1:
      G["dg_scalar"] = P["g"].grad
    for l in range(L):
      G["dwcat%d" % l] = P["wcat"][l].grad
      if l > 0:
        G["dbias%d" % l] = P["bias"][l].grad
    if P["b"] is not None:
      G["db"] = P["b"].grad
    if mode == 2:
      G.update(dconv_w=P["conv_w"].grad, dconv_b=P["conv_b"].grad, ddense_w=P["dense_w"].grad)
    R["grads"] = G
  _REF_CACHE[key] = R
  return R


def structural_zeros(name):
  """Compared gradients that are zero whatever the seed: with T = 1 the only cat0 row is the zero initial
  state (dWcat0 = dg0^T cat0) and the only cumulative alignments are zero (dconv_w); with S = 1 the
  softmax is the constant 1 and nothing reaches the score. The device must give exact zeros there."""
  T, S, mode = CASES[name][1], CASES[name][2], CASES[name][7]
  z = set()
  if T == 1:
    z.add("dwcat0")
    if mode == 2:
      z.add("dconv_w")
  if S == 1:
    z |= {"dkeys", "dv", "dg_scalar", "dwq", "db", "dconv_w", "dconv_b", "ddense_w"}
  return z


def check_inputs(name, R):
  """Conditions on the reference without which a comparison proves nothing; returns the violations."""
  S = CASES[name][2]
  d = build_inputs(name)
  bad = []
  zeros = structural_zeros(name)
  for k, g in R["grads"].items():
    if k in zeros:
      if g is None or float(g.abs().max()) != 0.0:
        bad.append("%s: reference gradient %s is listed as structurally zero and is not" % (name, k))
    elif g is None or not float(g.abs().max()) > 0.0:
      bad.append("%s: reference gradient %s is zero" % (name, k))
  if S > 1:
    # a sample with one source position has the alignment 1 by definition: the bound is on the others
    many = d["src_len"] > 1
    top = float(R["align"][many].max())
    if not top < 0.99:
      bad.append("%s: largest alignment weight %.4f >= 0.99" % (name, top))
  if not bool(live_steps(name).any(dim=1).all()):
    bad.append("%s: a sample without a live step" % name)
  return bad


@functools.lru_cache(maxsize=None)
def noise_floor():
  """n_q = max over the T <= 2 cases of max|R_b.q - R.q| for q in y, ctx, align: what one bf16 rounding
  per store costs. From the oracle alone (these cases have no dropout)."""
  n = dict(y=0.0, ctx=0.0, align=0.0)
  for name in TIGHT:
    assert CASES[name][11] == 1.0 and CASES[name][12] == 1.0, name
    R, Rb = reference(name), reference(name, rounded=True)
    for q in n:
      n[q] = max(n[q], float((Rb[q] - R[q]).abs().max()))
  return n


def run_gpu(name, device, strided=False, alt_sample0=False, second_backward=True):
  """Forward and backward of one case through capi.AttnDecoder; CPU tensors of everything compared.
  strided: y_top / ctx are column slices of one [B, T, 8 + H + M + 8] tensor filled with SENTINEL (rows of
  finished steps zeroed, as the ABI asks of the caller); `wide` is returned for the guard-column check.
  alt_sample0: sample 0's gx0 / keys / values replaced (sample isolation)."""
  from openseq2seq_amd import capi
  B, T, S, L, H, M, U, mode, K, F, use_bias, a_keep, o_keep, ragged = CASES[name]
  d = build_inputs(name)
  dev = device
  gx0, keys, values = d["gx0"], d["keys"], d["values"]
  if alt_sample0:
    gx0, keys, values = gx0.clone(), keys.clone(), values.clone()
    gx0[0], keys[0], values[0] = d["gx0_alt"], d["keys_alt"], d["values_alt"]
  wide = None
  kw = {}
  if strided:
    wide = torch.full((B, T, GUARD + H + M + GUARD), SENTINEL, dtype=torch.bfloat16, device=dev)
    kw = dict(y_top=wide[:, :, GUARD:GUARD + H], ctx=wide[:, :, GUARD + H:GUARD + H + M])
    dead = ~live_steps(name).to(dev)
    kw["y_top"][dead] = 0
    kw["ctx"][dead] = 0
  dec = capi.AttnDecoder(B, T, S, L, H, M, U, mode, dev, use_bias=use_bias, loc_k=K, loc_f=F,
                         forget_bias=1.0, attn_in_keep=a_keep, attn_in_seed=ATTN_IN_SEED, out_keep=o_keep,
                         out_seeds=OUT_SEEDS, **kw)
  todev = lambda t: None if t is None else t.to(dev)
  dec.set_params([w.to(dev) for w in d["wcat"]], d["wq"].to(dev), d["v"].to(dev),
                 bias=[todev(b) for b in d["bias"]], g=todev(d["g"]), b=todev(d["b"]),
                 conv_w=todev(d["conv_w"]), conv_b=todev(d["conv_b"]), dense_w=todev(d["dense_w"]))
  dec.set_inputs(gx0.to(dev), keys.to(dev), values.to(dev), d["src_len"].to(dev), todev(d["tgt_len"]))
  dec.forward()              # a status other than OS2S_OK raises Os2sError (_lib's errcheck)
  wcatT = [w.t().contiguous().to(dev) for w in d["wcat"]]
  wqT = d["wq"].t().contiguous().to(dev)
  dy, dctx = d["dy"].to(dev), d["dctx"].to(dev)

  def backward():
    acc = dict(dv=torch.zeros(U, device=dev), dg_scalar=torch.zeros(1, device=dev))
    if mode == 2:
      acc.update(dconv_w=torch.zeros(K, F, device=dev), dconv_b=torch.zeros(F, device=dev),
                 ddense_w=torch.zeros(F, U, device=dev))
    out = dec.backward(wcatT, wqT, dy_top=dy, dctx_ext=dctx, dv=acc["dv"], dg=acc["dg_scalar"],
                       dconv_w=acc.get("dconv_w"), dconv_b=acc.get("dconv_b"), ddense_w=acc.get("ddense_w"))
    torch.cuda.synchronize()
    r = {k: v.cpu() for k, v in acc.items()}
    r.update(dkeys=out["dkeys"].cpu(), dmem=out["dmem"].cpu(), dq_seq=out["dq_seq"].cpu())
    for l in range(L):
      r["dg%d" % l] = out["dg"][l].cpu()
    return r

  got = backward()
  if second_backward:
    got["second"] = backward()
  got.update(y=dec.y_top.cpu(), ctx=dec.ctx.cpu(), align=dec.align_seq.cpu(),
             cum=None if dec.cum_seq is None else dec.cum_seq.cpu(),
             cat=[c.cpu() for c in dec.cat], wide=None if wide is None else wide.cpu())
  return got


def _bits(t):
  return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
  return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def got_grads(name, got):
  """The compared gradient tensors from the device run (float64); weight gradients derived as the host
  layer does, with GEMMs over the saved sequences."""
  B, T, S, L, H, M, U, mode, K, F, use_bias, a_keep, o_keep, ragged = CASES[name]
  G = dict(dg0=got["dg0"].double(), dvalues=got["dmem"].double(), dkeys=got["dkeys"].double())
  if mode != 3:
    G["dv"] = got["dv"].double()
  if mode == 1:
    G["dg_scalar"] = got["dg_scalar"].double()
  for l in range(L):
    dgl = got["dg%d" % l].double().reshape(B * T, 4 * H)
    cat = got["cat"][l][:, :T].double().reshape(B * T, -1)
    G["dwcat%d" % l] = dgl.t() @ cat
    if l > 0:
      G["dbias%d" % l] = dgl.sum(0)
  dq = got["dq_seq"].double().reshape(B * T, U)
  if mode != 3:
    G["dwq"] = dq.t() @ got["y"].double().reshape(B * T, H)
  if build_inputs(name)["b"] is not None:
    G["db"] = dq.sum(0)
  if mode == 2:
    G.update(dconv_w=got["dconv_w"].double(), dconv_b=got["dconv_b"].double(), ddense_w=got["ddense_w"].double())
  return G


def compare(name, got, R, Rb=None, nq=None, log=print, assert_second=True):
  """The assertions of one device run against the oracle; returns the list of failures (empty: pass) and
  logs every figure it judges. assert_second=False (second_backward_judged): the tensors that differ
  between the two backward passes are logged, not judged."""
  B, T, S, L, H, M, U, mode, K, F, use_bias, a_keep, o_keep, ragged = CASES[name]
  d = build_inputs(name)
  src_len = d["src_len"]
  live = live_steps(name)
  dead = ~live
  fails = []

  def check(ok, what, *figs):
    log("  %-4s %s %s" % ("ok" if ok else "FAIL", what, " ".join("%.3e" % f for f in figs)))
    if not ok:
      fails.append("%s: %s %s" % (name, what, " ".join("%.3e" % f for f in figs)))

  fails += check_inputs(name, R)
  y, ctx, al = got["y"].double(), got["ctx"].double(), got["align"].double()
  # ---- exact ------------------------------------------------------------------------------------
  for k, t in (("y", y), ("ctx", ctx), ("align", al)):
    check(float(t[dead].abs().sum()) == 0.0 if bool(dead.any()) else True, "%s rows of finished steps zero" % k)
  past = torch.arange(S)[None, :] >= src_len[:, None]                     # [B, S]
  check(float(al.transpose(1, 2)[past].abs().sum()) == 0.0, "align past src_len zero")
  for l in range(L):
    check(float(got["dg%d" % l].double()[dead].abs().sum()) == 0.0 if bool(dead.any()) else True,
          "dg%d rows of finished steps zero" % l)
  check(float(got["dkeys"][past].abs().sum()) == 0.0, "dkeys past src_len zero")
  check(float(got["dmem"].double()[past].abs().sum()) == 0.0, "dmem past src_len zero")
  if S == 1:
    check(bool((got["align"][live] == 1.0).all()), "S = 1: live alignments equal 1")
  if "second" in got:
    for k, t in got["second"].items():
      if assert_second:
        check(same_bits(got[k], t), "second backward bit-identical: %s" % k)
      else:
        log("  note second backward %s: %s" % ("bit-identical" if same_bits(got[k], t) else "DIFFERS", k))
  # ---- against the oracle -------------------------------------------------------------------------
  if mode == 2:
    cum = got["cum"]
    step = (cum[:, 1:] - (cum[:, :-1] + got["align"])).abs()                 # fp32, as the kernel adds
    check(float(step[live].max()) <= 1e-6, "cum[t+1] = cum[t] + align[t] on live steps", float(step[live].max()))
    if bool(dead.any()):
      check(torch.equal(cum[:, 1:][dead], cum[:, :-1][dead]), "cum unchanged on finished steps")
    check(float(cum[:, 0].abs().max()) == 0.0, "cum[0] zero")
  rows = (al.sum(-1)[live] - 1.0).abs().max()
  check(float(rows) <= 1e-4, "live alignment rows sum to 1", float(rows))
  for k, t, atol, rtol in (("y", y, 3e-2, 3e-2), ("ctx", ctx, 3e-2, 3e-2), ("align", al, 5e-3, 3e-2)):
    err = (t - R[k]).abs()
    check(bool((err <= atol + rtol * R[k].abs()).all()), "forward %s vs R (atol %g rtol %g): max err" % (k, atol, rtol),
          float(err.max()))
  if name in TIGHT:
    for k, t in (("y", y), ("ctx", ctx), ("align", al)):
      err = (t - Rb[k]).abs()
      floor = 5e-4 if k == "align" else Rb[k].abs() * 2.0 ** -7
      bound = 4.0 * nq[k] + floor
      check(bool((err <= bound).all()), "forward %s vs R_b, 4 n_q + floor (n_q %.3e): max err, max err/bound" % (k, nq[k]),
            float(err.max()), float((err / bound).max()))
  G, ref = got_grads(name, got), R["grads"]
  assert sorted(G) == sorted(ref), (sorted(G), sorted(ref))
  for k in sorted(G):
    a, b = G[k].flatten(), ref[k].flatten()
    if k in structural_zeros(name):
      check(float(a.abs().max()) == 0.0, "grad %s exactly zero (structural): max|got|" % k, float(a.abs().max()))
      continue
    cos = float(torch.nn.functional.cosine_similarity(a, b, dim=0))
    rel = float((a - b).norm() / (b.norm() + 1e-12))
    cos_min, rel_max = (0.98, 0.15) if k == "dg_scalar" else (0.99, 0.1)
    check(cos > cos_min and rel < rel_max, "grad %s norm-wise: cos, rel" % k, cos, rel)
    worst, top = float((a - b).abs().max()), float(b.abs().max())
    check(worst <= 0.1 * top, "grad %s element-wise: max|got - ref|, max|ref|" % k, worst, top)
  return fails


def compare_runs(name, a, b, keys, what, rows=slice(None), log=print):
  """Bit equality of two device runs over `keys` (samples `rows`); returns the failures."""
  fails = []
  for k in keys:
    ok = same_bits(a[k][rows], b[k][rows])
    log("  %-4s %s: %s" % ("ok" if ok else "FAIL", what, k))
    if not ok:
      fails.append("%s: %s: %s differs" % (name, what, k))
  return fails


def run_case(name, device, **kw):
  """Device run and oracle run (R, with the library's dropout masks) of one case: (got, R)."""
  got = run_gpu(name, device, **kw)
  return got, reference(name, device=device)


def second_backward_judged(name):
  """False only for a location-mode case while the option attn_decoder.attn_split is 0 (a process started with
  OS2S_ATTN_SPLIT=0, or an os2s_set_option call). That setting selects
  the one-workgroup location backward, ad_attn_bwd_kernel<true>, whose wave groups add the state gradient
  (dcum_l) and the filter gradient (dwk_l) with LDS float atomics: the order of the additions, and with it
  the last bits, vary from run to run. Everything downstream of the two can differ; compare() then logs
  which tensors did. Every other kernel, the other two switches' included, is held to bit identity."""
  from openseq2seq_amd import _lib
  return not (_lib.get_option("attn_decoder.attn_split") == 0 and CASES[name][7] == 2)


def check_case(name, device, log=print, assert_second=None):
  """run_case + compare; the failures."""
  if assert_second is None:
    assert_second = second_backward_judged(name)
  got, R = run_case(name, device)
  Rb = nq = None
  if name in TIGHT:
    Rb, nq = reference(name, rounded=True, device=device), noise_floor()
  return got, compare(name, got, R, Rb, nq, log=log, assert_second=assert_second)


def main(argv):
  if len(argv) != 2 or argv[1] not in CASES:
    print("usage: python -m tests._attn_decoder_cases {%s}" % ",".join(sorted(CASES)))
    return 2
  import __graft_entry__ as entry
  from openseq2seq_amd import _lib
  if not os.path.exists(_lib.LIB_PATH):
    entry.build()
  assert torch.cuda.is_available(), "needs a GPU"
  print("case %s  %s" % (argv[1], " ".join("%s=%s" % (k, os.environ[k]) for k in sorted(os.environ)
                                          if k.startswith("OS2S_"))))
  # every assertion of compare(); the reruns with strided outputs and a replaced sample are the parent's
  _, fails = check_case(argv[1], torch.device("cuda:0"))
  for f in fails:
    print("MISMATCH", f)
  return 1 if fails else 0


if __name__ == "__main__":
  sys.exit(main(sys.argv))
