"""Helper of tests/test_zoneout_cpu.py and tests/test_zoneout_gpu.py (not a test module): the float64 oracle of
zoneout on the attention decoder's LSTM stack and on the encoder's tf LSTMCell layer, the case tables, the
device runs and the comparisons.

Oracle. ZoneoutWrapper (parts/rnns/zoneout.py:39-68) returns the wrapped cell's output unchanged and replaces
only its state: zoneout_state() below is that replacement, and nothing else is added to the pieces of
oracle/attn_decoder.py (lstm_cell, the score functions, masked_softmax, location_features) and oracle/rnn.py.
With zoneout off attention_decoder_zo() reproduces oad.attention_decoder and lstm_tf_zo() reproduces
oracle.rnn.lstm_tf bit for bit (tests/test_zoneout_cpu.py).

Decoder cases (B, T, S, L, H, M, U, mode; out_keep = 1 everywhere) and what they reach:
  zo_ragged    5, 6, 19, 2, 64, 64, 128, location, tgt_len [6, 1, 3, 6, 2], p 0.5
               ad_cell_fwd + ad_cell_bwd_split, two layers, finished samples
  zo_b32_fast  32, 3, 33, 2, 64, 64, 128, location, p 0.5: ti_lstm as the training forward
  zo_b33       33, 3, 17, 2, 64, 64, 128, location, p 0.5, option attn_decoder.cell_split = 0: ad_cell_bwd
  zo_h8        2, 3, 5, 1, 8, 8, 128, bahdanau, p 0.5: one mask byte per row
  zo_h72       4, 3, 21, 1, 72, 96, 128, location, p 0.1: H not a multiple of 64
  zo_t1        3, 1, 9, 1, 64, 64, 128, location, p 0.5: nothing to zone from but zeros, empty carries (ti_lstm)
They are run through tests/_attn_decoder_cases.py (its build_inputs, got_grads and compare(), with compare()'s
own bounds), registered in its tables only for the duration of a call.

Encoder-layer cases (B, T, H), both directions in one launch, ragged lengths containing 1 and T:
  r_h64 5, 6, 64    r_b33_h72 33, 3, 72    r_h8 2, 3, 8
held to the bound tests/_rnn_cases.py applies to cell 2: |got - R_b| <= 4 n_q + 2^-7 |R_b| with its n_q.

Masks. m ~ Bernoulli(1 - p) from the library's counter hash with keep = 1 - p over the logical [B, T, H] tensor
of a layer (a direction), one seed for h and one for c. hash_mask() restates the hash on the CPU, so the oracle
and the conditions on the masks need no device; the GPU tests hold it to capi.dropout_mask bit for bit."""
import contextlib
import functools
import math
import os
import sys
from unittest import mock

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
  sys.path.insert(0, REPO)

import _attn_decoder_cases as adc  # noqa: E402
import _rnn_cases as rc  # noqa: E402
from oracle import attn_decoder as oad  # noqa: E402
from oracle import rnn as orn  # noqa: E402

OFF, SAMPLE, BLEND = 0, 1, 2          # os2s_attn_decoder_t.zoneout_mode / os2s_rnn_zoneout_t.mode
SEEDS_H, SEEDS_C = (303, 404), (505, 606)

# name: (adc.CASES tuple, p, tgt_len or None, attention vector scale, option to clear or None)
DEC_CASES = {
    "zo_ragged": ((5, 6, 19, 2, 64, 64, 128, 2, 5, 4, False, 1.0, 1.0, True), 0.5, [6, 1, 3, 6, 2], 0.5, None),
    "zo_b32_fast": ((32, 3, 33, 2, 64, 64, 128, 2, 7, 8, False, 1.0, 1.0, False), 0.5, None, 0.2, None),
    "zo_b33": ((33, 3, 17, 2, 64, 64, 128, 2, 3, 4, False, 1.0, 1.0, False), 0.5, None, 0.1,
               "attn_decoder.cell_split"),
    "zo_h8": ((2, 3, 5, 1, 8, 8, 128, 0, 0, 0, False, 1.0, 1.0, False), 0.5, None, 1.0, None),
    "zo_h72": ((4, 3, 21, 1, 72, 96, 128, 2, 5, 4, False, 1.0, 1.0, False), 0.1, None, 0.5, None),
    "zo_t1": ((3, 1, 9, 1, 64, 64, 128, 2, 3, 2, False, 1.0, 1.0, False), 0.5, None, 0.5, None),
}
BLEND_CASES = ("zo_ragged", "zo_h72")        # mode 2, stepped one t at a time
FWD_TOL = dict(y=(3e-2, 3e-2), ctx=(3e-2, 3e-2), align=(5e-3, 3e-2))      # compare()'s forward bounds


def keep_of(p):
  """1 - p as the kernels form it (fp32)."""
  return float(np.float32(1.0) - np.float32(p))


@contextlib.contextmanager
def registered():
  """The decoder cases in the tables of _attn_decoder_cases, for the duration of the block only."""
  with mock.patch.dict(adc.CASES, {n: c[0] for n, c in DEC_CASES.items()}), \
       mock.patch.dict(adc.TGT_LEN, {n: c[2] for n, c in DEC_CASES.items() if c[2] is not None}), \
       mock.patch.dict(adc.V_SCALE, {n: c[3] for n, c in DEC_CASES.items()}):
    yield


# adc.build_inputs draws gx0 at std 0.7 and the cell kernels at std 1 / sqrt(fan-in): the cell states stay small,
# |h| below 0.5, and zoneout moves y by less than ten forward bounds. Livelier gates (dec_conditions() holds the
# result to that condition):
GX0_SCALE, WCAT_SCALE = 3.0, 8.0


@functools.lru_cache(maxsize=None)
def dec_inputs(name):
  """adc.build_inputs of a registered case with a livelier input projection; callers must not modify it."""
  with registered():
    d = dict(adc.build_inputs(name))
  d["gx0"] = (d["gx0"].float() * GX0_SCALE).to(torch.bfloat16)
  d["wcat"] = [(w.float() * WCAT_SCALE).to(torch.bfloat16) for w in d["wcat"]]
  return d


def dec_live(name):
  with registered():
    return adc.live_steps(name)


# ------------------------------------------------------------------------------------------ the replacement
def zoneout_state(new, old, zo, mask=None):
  """ZoneoutWrapper.__call__ on one state part. zo None: the new state. mode SAMPLE (training):
  (1 - p) dropout(new - old, keep = 1 - p) + old = m new + (1 - m) old with the unscaled keep mask m;
  mode BLEND (not training): p old + (1 - p) new."""
  if zo is None or zo["mode"] == OFF:
    return new
  if zo["mode"] == SAMPLE:
    return mask * new + (1.0 - mask) * old
  return zo["p"] * old + (1.0 - zo["p"]) * new


def hash_mask(seed, n, keep):
  """The library's counter hash restated on the CPU (csrc/os2s_common.hpp, dropout_bits8: element 8 i + 4 k + e
  is kept iff the e-th 16-bit field of splitmix64((2 i + k) * golden + seed) is below keep * 65536): bool [n],
  n % 8 == 0. The GPU tests hold it to capi.dropout_mask bit for bit, so the conditions checked on the CPU are
  conditions on the masks the kernels apply."""
  assert n % 8 == 0
  u64 = np.uint64
  golden = u64(0x9E3779B97F4A7C15)
  thr = int(np.float32(keep) * np.float32(65536.0))
  idx4 = np.arange(n // 4, dtype=np.uint64)
  with np.errstate(over="ignore"):
    z = idx4 * golden + u64(int(seed) & (2 ** 64 - 1))
    z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
    z = z ^ (z >> u64(31))
  fields = np.stack([(z >> u64(16 * e)) & u64(0xFFFF) for e in range(4)], axis=1)      # [n/4, 4]
  return torch.from_numpy((fields < u64(thr)).reshape(-1))


def masks(shape, p, seeds):
  """[len(seeds) x mask `shape`] float64 keep masks (1 = the new state is kept) with keep = 1 - p."""
  n = int(np.prod(shape))
  return [hash_mask(sd, n, keep_of(p)).view(*shape).double() for sd in seeds]


def masks_match_the_library(shape, p, seeds, device):
  """hash_mask against capi.dropout_mask; the violations."""
  from openseq2seq_amd import capi
  n = int(np.prod(shape))
  bad = []
  for sd, m in zip(seeds, masks(shape, p, seeds)):
    lib = capi.dropout_mask(sd, n, keep_of(p), device).view(*shape).cpu()
    if not torch.equal(lib, m.bool()):
      bad.append("seed %d, keep %.3f: the CPU restatement of the counter hash differs from os2s_dropout_mask" % (sd, keep_of(p)))
  return bad


def mask_conditions(ms, live, p, what):
  """Conditions on the masks without which a comparison proves nothing; the violations."""
  bad = []
  for i, m in enumerate(ms):
    rows = m[live]                                    # [live rows, H]
    frac = float(rows.mean())
    if p == 0.5 and not 0.3 <= frac <= 0.7:
      bad.append("%s mask %d keeps %.3f, outside [0.3, 0.7]" % (what, i, frac))
    if not bool(((rows.sum(1) > 0) & (rows.sum(1) < rows.shape[1])).all()):
      bad.append("%s mask %d: a live row without a kept or without a zoned element" % (what, i))
  return bad


# ------------------------------------------------------------------------------------------ decoder oracle
def attention_decoder_zo(p, gx0, memory, src_len, tgt_len=None, zo=None, forget_bias=1.0, mode="location",
                         keys_override=None, values_override=None, store=None):
  """oad.attention_decoder (no dropout masks) with every layer's cell wrapped in zoneout: zo = None or
  dict(mode, p, mh = L x [B,T,H], mc = L x [B,T,H]). The output of a layer (next layer's input, query, y) stays
  the unzoned h; the state the same layer reads at step t + 1 is the zoned (c', h'). Returns oad's dict plus
  h_state / c_state (L x [B,T,H], the stored state after step t) and c_new (the unzoned cell state)."""
  if store is None:
    store = lambda t: t
  B, T, _ = gx0.shape
  L = len(p["wcat"])
  H = p["wq"].shape[1]
  values, mask = oad.prepare_memory(memory, src_len)
  if values_override is not None:
    values = values_override
  keys = keys_override if keys_override is not None else values @ p["wmem"].t()
  M, S = values.shape[2], values.shape[1]
  h = [gx0.new_zeros(B, H) for _ in range(L)]
  c = [gx0.new_zeros(B, H) for _ in range(L)]
  attn = gx0.new_zeros(B, M)
  cum = gx0.new_zeros(B, S)
  ys, ctxs, aligns = [], [], []
  hs, cs, cns = [[] for _ in range(L)], [[] for _ in range(L)], [[] for _ in range(L)]
  sampled = zo is not None and zo["mode"] == SAMPLE
  for t in range(T):
    live = None
    if tgt_len is not None:
      live = (t < torch.as_tensor(tgt_len)).to(gx0.dtype)[:, None]
    x = None
    nh, nc = [], []
    for l in range(L):
      if l == 0:
        hn, cn = oad.lstm_cell(torch.cat([attn, h[0]], -1), c[0], p["wcat"][0], gx0[:, t], forget_bias)
      else:
        hn, cn = oad.lstm_cell(torch.cat([x, h[l]], -1), c[l], p["wcat"][l], p["bias"][l], forget_bias)
      nh.append(store(zoneout_state(hn, h[l], zo, zo["mh"][l][:, t] if sampled else None)))
      nc.append(zoneout_state(cn, c[l], zo, zo["mc"][l][:, t] if sampled else None))
      cns[l].append(cn)
      x = store(hn)
    q = x @ p["wq"].t()
    if mode == "location":
      pre = keys + q[:, None, :] + oad.location_features(cum, p["conv_w"], p["conv_b"], p["dense_w"])
      if p.get("b") is not None:
        pre = pre + p["b"]
      score = (p["v"] * torch.tanh(pre)).sum(-1)
    elif mode == "bahdanau_norm":
      score = oad.bahdanau_score(q, keys, p["v"], p["g"], p["b"])
    elif mode == "luong":
      score = (keys * x[:, None, :]).sum(-1)
    else:
      score = oad.bahdanau_score(q, keys, p["v"])
    al = oad.masked_softmax(score, mask)
    ctx = store((al[:, :, None] * values).sum(1))
    if live is not None:
      for l in range(L):
        h[l] = live * nh[l] + (1 - live) * h[l]
        c[l] = live * nc[l] + (1 - live) * c[l]
      attn = live * ctx + (1 - live) * attn
      cum = cum + live * al
      ys.append(x * live)
      ctxs.append(ctx * live)
      aligns.append(al * live)
    else:
      h, c, attn = nh, nc, ctx
      cum = cum + al
      ys.append(x)
      ctxs.append(ctx)
      aligns.append(al)
    for l in range(L):
      hs[l].append(h[l])
      cs[l].append(c[l])
  st = lambda seqs: [torch.stack(s, 1) for s in seqs]
  return dict(y=torch.stack(ys, 1), ctx=torch.stack(ctxs, 1), align=torch.stack(aligns, 1), keys=keys,
              values=values, h_state=st(hs), c_state=st(cs), c_new=st(cns))


def dec_masks(name):
  """dict(mh, mc) of a decoder case: L masks [B,T,H] each."""
  B, T, S, L, H = DEC_CASES[name][0][:5]
  p = DEC_CASES[name][1]
  return dict(mh=masks((B, T, H), p, SEEDS_H[:L]), mc=masks((B, T, H), p, SEEDS_C[:L]))


_REF = {}


def dec_reference(name, zmode):
  """The fp64 oracle of a decoder case in the layout of adc.reference(): dict(y, ctx, align, h_state, c_state,
  c_new[, grads]); grads (of sum(y dy) + sum(ctx dctx)) for OFF and SAMPLE. Computed once per (case, mode);
  callers must not modify it."""
  key = (name, zmode)
  if key in _REF:
    return _REF[key]
  case, p = DEC_CASES[name][:2]
  B, T, S, L, H, M, U, mode = case[:8]
  d = dec_inputs(name)
  zo = None
  if zmode != OFF:
    zo = dict(mode=zmode, p=p, **(dec_masks(name) if zmode == SAMPLE else {}))
  want_grads = zmode != BLEND
  leaf = lambda t: None if t is None else t.double().clone().requires_grad_(want_grads)
  P = dict(wcat=[leaf(w) for w in d["wcat"]], bias=[leaf(b) for b in d["bias"]], wq=leaf(d["wq"]), wmem=None,
           v=leaf(d["v"]), g=leaf(d["g"]), b=leaf(d["b"]), conv_w=leaf(d["conv_w"]), conv_b=leaf(d["conv_b"]),
           dense_w=leaf(d["dense_w"]))
  gx0, vals, keys = leaf(d["gx0"]), leaf(d["values"]), leaf(d["keys"])
  out = attention_decoder_zo(P, gx0, d["values"].double(), d["src_len"], d["tgt_len"], zo, 1.0, adc.MODES[mode],
                             keys_override=keys, values_override=vals)
  R = {k: out[k].detach() for k in ("y", "ctx", "align")}
  for k in ("h_state", "c_state", "c_new"):
    R[k] = [t.detach() for t in out[k]]
  if want_grads:
    ((out["y"] * d["dy"].double()).sum() + (out["ctx"] * d["dctx"].double()).sum()).backward()
    G = dict(dg0=gx0.grad, dvalues=vals.grad, dkeys=keys.grad)
    if mode != 3:
      G["dv"], G["dwq"] = P["v"].grad, P["wq"].grad
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
  _REF[key] = R
  return R


def dec_conditions(name):
  """Conditions from the masks and the oracle alone: the mask fractions, kept and zoned elements in every live
  row, and (T > 1: at T = 1 the state is never read back) an oracle output y that zoneout moves by more than ten
  times compare()'s forward bound, so that a kernel that ignores the option fails."""
  case, p = DEC_CASES[name][:2]
  T = case[1]
  live = dec_live(name)
  m = dec_masks(name)
  bad = mask_conditions(m["mh"], live, p, name + " h") + mask_conditions(m["mc"], live, p, name + " c")
  if T > 1:
    on, off = dec_reference(name, SAMPLE), dec_reference(name, OFF)
    atol, rtol = FWD_TOL["y"]
    moved = (on["y"] - off["y"]).abs() > 10.0 * (atol + rtol * off["y"].abs())
    if not bool(moved.any()):
      bad.append("%s: zoneout moves no element of the oracle's y by more than ten forward bounds (max %.3e)"
                 % (name, float((on["y"] - off["y"]).abs().max())))
  return bad


# ------------------------------------------------------------------------------------------ decoder device run
def run_dec(name, device, zmode, p=None, backward=True, second_backward=True, stepwise=False):
  """adc.run_gpu with the zoneout fields set (contiguous outputs): forward over all steps at once or, stepwise,
  one os2s_attn_decoder_fwd call per step as the free-running fallback drives it; backward as adc.run_gpu's.
  Returns adc.run_gpu's dict plus c_seq and gates."""
  from openseq2seq_amd import capi
  case = DEC_CASES[name][0]
  B, T, S, L, H, M, U, mode, K, F, use_bias, a_keep, o_keep, ragged = case
  p = DEC_CASES[name][1] if p is None else p
  d = dec_inputs(name)
  dev = device
  dec = capi.AttnDecoder(B, T, S, L, H, M, U, mode, dev, use_bias=use_bias, loc_k=K, loc_f=F, forget_bias=1.0,
                         attn_in_keep=a_keep, attn_in_seed=adc.ATTN_IN_SEED, out_keep=o_keep,
                         out_seeds=adc.OUT_SEEDS, save=backward, zoneout_prob=p, zoneout_mode=zmode,
                         zoneout_seeds_h=SEEDS_H, zoneout_seeds_c=SEEDS_C)
  todev = lambda t: None if t is None else t.to(dev)
  dec.set_params([w.to(dev) for w in d["wcat"]], d["wq"].to(dev), d["v"].to(dev),
                 bias=[todev(b) for b in d["bias"]], g=todev(d["g"]), b=todev(d["b"]),
                 conv_w=todev(d["conv_w"]), conv_b=todev(d["conv_b"]), dense_w=todev(d["dense_w"]))
  dec.set_inputs(d["gx0"].to(dev), d["keys"].to(dev), d["values"].to(dev), d["src_len"].to(dev), todev(d["tgt_len"]))
  if stepwise:
    for t in range(T):
      dec.forward(t, t + 1)
  else:
    dec.forward()
  torch.cuda.synchronize()
  got = {}
  if backward:
    wcatT = [w.t().contiguous().to(dev) for w in d["wcat"]]
    wqT = d["wq"].t().contiguous().to(dev)
    dy, dctx = d["dy"].to(dev), d["dctx"].to(dev)

    def bwd():
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

    got = bwd()
    if second_backward:
      got["second"] = bwd()
  got.update(y=dec.y_top.cpu(), ctx=dec.ctx.cpu(), align=dec.align_seq.cpu(),
             cum=None if dec.cum_seq is None else dec.cum_seq.cpu(), cat=[c.cpu() for c in dec.cat], wide=None,
             c_seq=[c.cpu() for c in dec.c_seq])
  return got


def forward_fails(name, got, R, log=print):
  """compare()'s forward assertions alone (rows of finished steps zero, y / ctx / align within its bounds)."""
  live = dec_live(name)
  dead = ~live
  fails = []
  for k in ("y", "ctx", "align"):
    t = got[k].double()
    if bool(dead.any()) and float(t[dead].abs().sum()) != 0.0:
      fails.append("%s: %s rows of finished steps not zero" % (name, k))
    atol, rtol = FWD_TOL[k]
    err = (t - R[k]).abs()
    ok = bool((err <= atol + rtol * R[k].abs()).all())
    log("  %-4s %s forward %s vs R (atol %g rtol %g): max err %.3e" % ("ok" if ok else "FAIL", name, k, atol, rtol,
                                                                     float(err.max())))
    if not ok:
      fails.append("%s: forward %s max err %.3e" % (name, k, float(err.max())))
  return fails


def state_copy_fails(name, got, R, m, log=print):
  """Mode 1: on live steps the stored state is, bit for bit, the previous state where the mask zoned the element
  and the new one where it kept it. h: cat[l] row t + 1 against cat[l] row t / the layer's bf16 output (y_top,
  or the layer above's input columns); c: c_seq row t against row t - 1 (zeros at t = 0), and where kept against
  the oracle's unzoned c_new within compare()'s forward bound (the new cell state is stored nowhere else)."""
  case = DEC_CASES[name][0]
  B, T, S, L, H = case[:5]
  live = dec_live(name)[:, :, None]
  fails = []
  for l in range(L):
    hst, hprev = got["cat"][l][:, 1:, -H:], got["cat"][l][:, :T, -H:]
    hnew = got["y"] if l == L - 1 else got["cat"][l + 1][:, :T, :H]
    kept = m["mh"][l].bool()
    want = torch.where(kept, hnew, hprev)
    ok = torch.equal(adc._bits(torch.where(live, hst, torch.zeros((), dtype=hst.dtype)).contiguous()),
                     adc._bits(torch.where(live, want, torch.zeros((), dtype=hst.dtype)).contiguous()))
    log("  %-4s %s layer %d: stored h is the previous or the new one by the mask, bit for bit" % ("ok" if ok else "FAIL", name, l))
    if not ok:
      fails.append("%s: layer %d stored h does not follow the mask" % (name, l))
    cst = got["c_seq"][l]
    cprev = torch.cat([torch.zeros(B, 1, H), cst[:, :-1]], 1)
    zoned = live & ~m["mc"][l].bool()
    ok = torch.equal(adc._bits(cst[zoned].contiguous()), adc._bits(cprev[zoned].contiguous()))
    log("  %-4s %s layer %d: zoned c is the previous one, bit for bit (%d elements)" % ("ok" if ok else "FAIL", name, l, int(zoned.sum())))
    if not ok:
      fails.append("%s: layer %d zoned c is not a copy" % (name, l))
    keptc = live & m["mc"][l].bool()
    atol, rtol = FWD_TOL["y"]
    err = (cst.double() - R["c_new"][l]).abs()[keptc]
    ref = R["c_new"][l].abs()[keptc]
    ok = bool((err <= atol + rtol * ref).all())
    log("  %-4s %s layer %d: kept c vs the oracle's c_new: max err %.3e" % ("ok" if ok else "FAIL", name, l, float(err.max())))
    if not ok:
      fails.append("%s: layer %d kept c off the oracle by %.3e" % (name, l, float(err.max())))
  return fails


@contextlib.contextmanager
def option_cleared(name):
  """The named library option at 0 inside the block, restored afterwards (None: nothing)."""
  if name is None:
    yield
    return
  from openseq2seq_amd import _lib
  old = _lib.get_option(name)
  _lib.set_option(name, 0)
  try:
    yield
  finally:
    _lib.set_option(name, old)


# ------------------------------------------------------------------------------------------ encoder layer oracle
RNN_CASES = {"r_h64": (5, 6, 64, [6, 1, 4, 6, 2]), "r_b33_h72": (33, 3, 72, rc.RAGGED), "r_h8": (2, 3, 8, [3, 1])}
RNN_P = {SAMPLE: 0.5, BLEND: 0.1}
RNN_SEEDS_H, RNN_SEEDS_C = (707, 808), (909, 1010)       # per direction


@functools.lru_cache(maxsize=None)
def rnn_inputs(name):
  """bf16-rounded gx, wh, dy per direction (forward, reverse) and the lengths; CPU tensors."""
  B, T, H, lens = RNN_CASES[name]
  g = torch.Generator().manual_seed(sum(map(ord, name)))
  rn = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(torch.bfloat16)
  if lens == rc.RAGGED:
    lens = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    lens[0], lens[1] = T, 1
  else:
    lens = torch.tensor(lens, dtype=torch.int32)
  assert 1 in lens.tolist() and T in lens.tolist() and int(lens.min()) < T
  dirs = [dict(reverse=bool(r), gx=rn(B, T, 4 * H, sc=0.5), wh=rn(4 * H, H, sc=1.0 / math.sqrt(H)), dy=rn(B, T, H))
          for r in (0, 1)]
  return dict(lens=lens, dirs=dirs)


def rnn_live(name):
  B, T, H, _ = RNN_CASES[name]
  return torch.arange(T)[None, :] < rnn_inputs(name)["lens"].to(torch.int64)[:, None]


def rnn_masks(name):
  """Per direction dict(mh, mc) [B,T,H], indexed by the true time index."""
  B, T, H, _ = RNN_CASES[name]
  mh = masks((B, T, H), RNN_P[SAMPLE], RNN_SEEDS_H)
  mc = masks((B, T, H), RNN_P[SAMPLE], RNN_SEEDS_C)
  return [dict(mh=mh[d], mc=mc[d]) for d in range(2)]


def lstm_tf_zo(x, lens, wx, wh, bias, forget_bias=1.0, reverse=False, zo=None, rd=None):
  """oracle.rnn.lstm_tf with the cell wrapped in zoneout: zo = None or dict(mode, p, mh, mc [B,T,H] by true time
  index). rd: optional straight-through bf16 round applied where the step kernels store bf16 (the state fed to
  the next step's product, y, the saved gates, h_seq). Returns dict(y, gates (i, f, g, o activations), c_seq
  (zoned), h_seq (zoned), c_new), all [B,T,.] by true time index, zero past the lengths."""
  rd = rd or (lambda t: t)
  B, T, _ = x.shape
  H = wh.shape[0]
  if lens is None:
    lens = torch.full((B,), T)
  rev = (lambda t: orn._reverse_by_len(t, lens)) if reverse else (lambda t: t)
  xin = rev(x)
  sampled = zo is not None and zo["mode"] == SAMPLE
  mh, mc = (rev(zo["mh"]), rev(zo["mc"])) if sampled else (None, None)
  h = x.new_zeros(B, H)
  c = x.new_zeros(B, H)
  hb = h
  ys, gs, cs, hs, cns = [], [], [], [], []
  for t in range(T):
    z = xin[:, t] @ wx + hb @ wh + bias
    i, j, f, o = z.chunk(4, dim=-1)
    ig, fg, gg, og = torch.sigmoid(i), torch.sigmoid(f + forget_bias), torch.tanh(j), torch.sigmoid(o)
    cn = c * fg + ig * gg
    hn = torch.tanh(cn) * og
    live = (t < torch.as_tensor(lens)).to(x.dtype)[:, None]
    c = live * zoneout_state(cn, c, zo, mc[:, t] if sampled else None) + (1 - live) * c
    h = live * zoneout_state(hn, h, zo, mh[:, t] if sampled else None) + (1 - live) * h
    hb = rd(h)
    ys.append(rd(hn) * live)
    gs.append(rd(torch.cat([ig, fg, gg, og], -1)) * live)
    cs.append(c * live)
    hs.append(hb * live)
    cns.append(cn * live)
  return {k: rev(torch.stack(v, 1)) for k, v in (("y", ys), ("gates", gs), ("c_seq", cs), ("h_seq", hs), ("c_new", cns))}


def lstm_tf_zo_bwd(gates, c_seq, dy, wh, lens, reverse, zo=None, rounded=False):
  """rc.backward_oracle for the LSTMCell, teacher-forced on the saved gates and the (zoned) c_seq, with the mask
  split of mode SAMPLE: of the gradient reaching the zoned h'_t (dg_{s+1} . Wh + carry) and c'_t (carry), m goes
  to the new value and 1 - m past the cell to step s - 1; the unzoned c_new is c_seq[t] where m_c kept it, else
  c'_{t-1} f + i g. wh [4H, H] (rows i, j, f, o). Returns dgx [B,T,4H] (i, j, f, o)."""
  gates, c_seq, dy, wh = gates.double(), c_seq.double(), dy.double(), wh.double()
  B, T, H = dy.shape
  ln = rc.eff_lens(lens, B, T)
  rd = rc.rb if rounded else (lambda t: t)
  sampled = zo is not None and zo["mode"] == SAMPLE
  dgx = torch.zeros(B, T, 4 * H, dtype=torch.float64)
  dg_next = torch.zeros(B, 4 * H, dtype=torch.float64)
  carry = torch.zeros(B, H, dtype=torch.float64)
  dcarry = torch.zeros(B, H, dtype=torch.float64)
  bi = torch.arange(B)
  one = torch.ones(B, H, dtype=torch.float64)
  for s in range(T - 1, -1, -1):
    act = (s < ln)[:, None]
    t = ((ln - 1 - s) if reverse else torch.full_like(ln, s)).clamp(0, T - 1)
    tp = (t + 1 if reverse else t - 1).clamp(0, T - 1)
    mh = zo["mh"][bi, t] if sampled else one
    mc = zo["mc"][bi, t] if sampled else one
    g_h = dg_next @ wh + carry
    dh = dy[bi, t] + mh * g_h
    sv = gates[bi, t].view(B, 4, H)
    ig, fg, gg, og = sv[:, 0], sv[:, 1], sv[:, 2], sv[:, 3]
    cprev = c_seq[bi, tp] if s > 0 else torch.zeros(B, H, dtype=torch.float64)
    cn = torch.where(mc > 0, c_seq[bi, t], cprev * fg + ig * gg)
    tc = torch.tanh(cn)
    dc = dh * og * (1.0 - tc * tc) + mc * dcarry
    dpre = torch.stack([dc * gg * ig * (1.0 - ig), dc * ig * (1.0 - gg * gg), dc * cprev * fg * (1.0 - fg),
                        dh * tc * og * (1.0 - og)], dim=1).reshape(B, 4 * H)
    carry = torch.where(act, (1.0 - mh) * g_h, carry)
    dcarry = torch.where(act, dc * fg + (1.0 - mc) * dcarry, dcarry)
    dg_next = torch.where(act, rd(dpre), torch.zeros((), dtype=torch.float64))
    dgx[bi, t] = torch.where(act, rd(dpre), dgx[bi, t])
  return dgx


def rnn_forward_ref(name, zmode, rounded):
  """Forward oracle of both directions of an encoder-layer case (gx enters through an identity input kernel)."""
  B, T, H, _ = RNN_CASES[name]
  d = rnn_inputs(name)
  ms = rnn_masks(name) if zmode == SAMPLE else [None, None]
  eye = torch.eye(4 * H, dtype=torch.float64)
  out = []
  for x, m in zip(d["dirs"], ms):
    zo = None if zmode == OFF else dict(mode=zmode, p=RNN_P[zmode], **(m or {}))
    with torch.no_grad():
      out.append(lstm_tf_zo(x["gx"].double(), d["lens"], eye, x["wh"].double().t(), torch.zeros(4 * H, dtype=torch.float64),
                            rc.FORGET_BIAS, x["reverse"], zo, rd=adc.round_bf16 if rounded else None))
  return out


def run_rnn(name, device, zmode, backward=True):
  """Both directions of a case in one os2s_rnn_layer_{fwd,bwd}_zoneout launch per step; CPU tensors per direction:
  y, gates, c_seq, h_seq[, dgx]."""
  from openseq2seq_amd import capi
  B, T, H, _ = RNN_CASES[name]
  d = rnn_inputs(name)
  lens = d["lens"].to(device)
  dev = [{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in x.items()} for x in d["dirs"]]
  zo = dict(prob=RNN_P[zmode], mode=zmode, seeds_h=RNN_SEEDS_H, seeds_c=RNN_SEEDS_C)
  fw = capi.rnn_layer_fwd_multi(capi.CELL_LSTM_TF, [dict(gx=x["gx"], wh=x["wh"], bh=None, y=None, reverse=x["reverse"])
                                                    for x in dev], lens, H, forget_bias=rc.FORGET_BIAS, zoneout=zo)
  torch.cuda.synchronize()
  out = [dict(y=f[0].cpu(), gates=f[1].cpu(), c_seq=f[2].cpu(), h_seq=f[3].cpu()) for f in fw]
  if backward:
    bw = capi.rnn_layer_bwd_multi(capi.CELL_LSTM_TF,
                                  [dict(whT=x["wh"].t().contiguous(), dy=x["dy"], y=f[0], gates=f[1], c_seq=f[2],
                                        reverse=x["reverse"]) for x, f in zip(dev, fw)], lens, H,
                                  forget_bias=rc.FORGET_BIAS, zoneout=zo)
    torch.cuda.synchronize()
    for o, b in zip(out, bw):
      o["dgx"] = b[0].cpu()
  return out


def rnn_compare(name, got, Rb, nq, outputs, log=print):
  """rc.compare()'s assertions for cell 2 on `outputs` (h_seq is judged with y's n_q: the same bf16 store of an
  h): rows past the lengths exactly zero, live rows within 4 n_q + 2^-7 |R_b|. Returns the failures."""
  live = rnn_live(name)
  dead = ~live
  fails = []
  for d, (g, r) in enumerate(zip(got, Rb)):
    for q in outputs:
      n = nq["y" if q == "h_seq" else q]
      if q in ("y", "dgx", "h_seq") and bool(dead.any()) and not bool((g[q].double()[dead] == 0.0).all()):
        fails.append("%s dir %d: %s rows past the lengths not zero" % (name, d, q))
      a, ref = rc._live(g[q], live), rc._live(r[q], live)
      err = (a - ref).abs()
      bound = 4.0 * n + 2.0 ** -7 * ref.abs()
      ok = bool((err <= bound).all())
      worst = float(torch.nan_to_num(err / bound, nan=float("inf")).max())
      log("  %-4s %s dir %d %s vs R_b, 4 n_q + 2^-7 |R_b| (n_q %.3e): max err %.3e, max err/bound %.3e"
          % ("ok" if ok else "FAIL", name, d, q, n, float(torch.nan_to_num(err, nan=float("inf")).max()), worst))
      if not ok:
        fails.append("%s dir %d: %s err/bound %.3e" % (name, d, q, worst))
  return fails


def rnn_state_copy_fails(name, got, ms, log=print):
  """Mode 1, per direction and live step: h_seq[t] is h_seq at the previous step in processing order (zeros at the
  first) where m_h zoned the element and y[t] where it kept it; c_seq likewise where m_c zoned it. Bit for bit."""
  B, T, H, _ = RNN_CASES[name]
  live = rnn_live(name)[:, :, None]
  fails = []
  for d, (g, m) in enumerate(zip(got, ms)):
    rev = rnn_inputs(name)["dirs"][d]["reverse"]

    def prev(t):      # the tensor one step earlier in processing order; the first live step reads zeros
      z = torch.zeros_like(t[:, :1])
      return torch.cat([t[:, 1:], z], 1) if rev else torch.cat([z, t[:, :-1]], 1)

    # (the first processed step of a reversed sample is t = len - 1: the h_seq row behind it is past the length
    # and zero, the c_seq row there is never written and is replaced by the zero initial state below)
    hprev, cprev = prev(g["h_seq"]), prev(g["c_seq"])
    want = torch.where(m["mh"].bool(), g["y"], hprev)
    z16 = torch.zeros((), dtype=torch.bfloat16)
    ok = torch.equal(adc._bits(torch.where(live, g["h_seq"], z16).contiguous()),
                     adc._bits(torch.where(live, want, z16).contiguous()))
    log("  %-4s %s dir %d: h_seq is the previous state or y by the mask, bit for bit" % ("ok" if ok else "FAIL", name, d))
    if not ok:
      fails.append("%s dir %d: h_seq does not follow the mask" % (name, d))
    first = (torch.arange(T)[None, :] == (rnn_inputs(name)["lens"].to(torch.int64)[:, None] - 1)) if rev else \
        (torch.arange(T)[None, :] == 0).expand(B, T)
    cprev = torch.where(first[:, :, None], torch.zeros(()), cprev)
    zoned = live & ~m["mc"].bool()
    ok = torch.equal(adc._bits(g["c_seq"][zoned].contiguous()), adc._bits(cprev[zoned].contiguous()))
    log("  %-4s %s dir %d: zoned c_seq is the previous one, bit for bit (%d elements)" % ("ok" if ok else "FAIL", name, d, int(zoned.sum())))
    if not ok:
      fails.append("%s dir %d: zoned c_seq is not a copy" % (name, d))
  return fails
