"""Helper of the text-classification tests (not a test module): the case tables, a float64 oracle of the
LayerNorm-LSTM backward with a gradient on the final state (os2s_lnlstm_layer_bwd_state), and a float64 oracle of
the final-state classification head and its loss (csrc/text_cls.hip), each with the bound it is held to.

State-gradient backward. backward_state_oracle() is _lnlstm_cases.backward_oracle's recurrence, teacher-forced on
the saved xhat / s_hat / rstd, with dhT / dcT entering at step len_b - 1 (T - 1 without lens; nothing for a sample
of length 0): dhT joins dh of that step, dcT the gradient of that step's NORMALISED state c_t (cT is the carried
state, the output of the state LayerNorm), i.e. it passes through the state LayerNorm's backward. R plainly, R_b
with dgx rounded to bf16 as documented in _lnlstm_cases. The rule is that file's: |got - R_b| <= 4 n_q + 2^-7 |R_b|
elementwise on dgx and dln, n_q = max |R_b - R| from the oracle alone (state_noise_floor: teacher the forward R_b).
STATE_CASES are geometries of _lnlstm_cases.CASES, so the kernel instances are the ones listed there, with the
cell backward in its state form lnlstm_cell_bwd_kernel<NCH, true> whenever dy is absent or dhT given, which the
first three mixes are (the fourth, dy + dcT, is the plain instance behind the copied carry; a state call with dy and without dhT runs the plain <NCH, false>, so the dhT = dcT = NULL
comparison holds by construction and checks the dispatch): cb<1> (h8, t1_h24, b33_h24, keep07_h40, state_h24), cb<2> (h520), cb<4> (h1032,
h2048); b33_h24 holds the second batch tile
of the product backward; t1_h24 has no product launch at all (the entry step has no dhp); h8 has lengths 7, 1, 4,
0, 10 of T = 7: full length (entry at T - 1), length 1 (entry at the step that reads c0), length 0 (no entry) and
the clamp. MIXES: which of dy / dhT / dcT are given.

Head. One kernel instance per entry (C <= 16 classes are register arrays behind wave-uniform guards, no
templates), so HEAD_CASES vary what the one instance does:
  b1_h8_c2       one sample, one chunk: lanes 1..63 of the forward / state-gradient wave idle, one dW thread per
                 class; h only (cT NULL)
  b5_h8_c10      h + c: chunk 0 from hT, chunk 1 from cT; 20 dW threads; C = 10
  b33_h520_c3    D = 1040: 130 chunks, lanes 0, 1 own three chunks; dW spans 7 workgroups, the last partly idle
  b2_h2048_c2    the top of the contract, D = 4096: every lane owns 8 chunks
  b257_h24_c16   the loss workgroup's second round (sample 256 on thread 0), C = 16, h only
Outputs are fp32 sums, so the bound is the running-error bound of a sum of n terms evaluated in fp32 in any
order: |got - R| <= n 2^-23 S elementwise, S the oracle's sum of the absolute values of the terms, each stage
teacher-forced on the device's output of the stage before (the loss on the device logits, the backward on the
device dlogits). Terms:
  logits[b,c]   D products and the bias: n = D + 1
  loss          per sample and class y_c (lse_b - l_bc) with l the logits shifted by their maximum (both parts are
                >= 0: no cancellation), over B: n = B C + C (the C exponentials inside lse) + 8
  dlogits[b,c]  softmax_c ysum and y_c, scaled by loss_scale / B: n = 2 + C (the softmax denominator) + 8
  dW[c,d]       B products and the value accumulated into: n = B + 1;  dbias[c] likewise
  dhT / dcT     C products: n = C
The + 8 covers expf / log1pf (1 ulp each by the device library's documentation), the shift by the maximum, the
division and the two roundings of loss_scale / B; it is reasoned, not measured: each of these is at most one unit
of 2^-23 relative to a term. Logits of the cases are of order 1, so the shift's own rounding, |l - m| 2^-24
relative, stays below one such unit.

Measured on the MI355X when this file was written (the tests compute their own bounds), largest err / bound: state
gradient dgx 0.061 (h1032), dln 0.0096 (t1_h24), bit-identical to R_b on h8 / t1_h24 dgx; head logits 0.035, loss
0.051, dlogits 0.12, dW 0.31, dbias 0.25, dhT / dcT 0.40 (n = 2: b2_h2048_c2)."""
import functools
import math

import torch

import _lnlstm_cases as C

STATE_CASES = ("h8", "t1_h24", "b33_h24", "h520", "h1032", "h2048", "keep07_h40", "state_h24")
MIXES = {"state_only": (False, True, True), "all": (True, True, True), "h_only": (False, True, False),
         "dy_and_c": (True, False, True)}
STATE_MUTATIONS = ("entry_at_T", "no_dcT", "dcT_before_state_ln")
HEAD_MUTATIONS = ("c_then_h", "loss_over_BC")

# name: B, H, C, use_cell_state
HEAD_CASES = {
    "b1_h8_c2": (1, 8, 2, False),
    "b5_h8_c10": (5, 8, 10, True),
    "b33_h520_c3": (33, 520, 3, True),
    "b2_h2048_c2": (2, 2048, 2, True),
    "b257_h24_c16": (257, 24, 16, False),
}
SCALES = (1.0, 1024.0)
U = 2.0 ** -23


# ------------------------------------------------------------------------------------------ state gradient
@functools.lru_cache(maxsize=None)
def state_grads(case):
  """dhT, dcT ~ N(0,1) fp32 [B,H] of a case (CPU; callers must not modify them)."""
  s = C.spec(case)
  g = torch.Generator().manual_seed(sum(map(ord, "textcls-" + case)))
  return torch.randn(s["B"], s["H"], generator=g), torch.randn(s["B"], s["H"], generator=g)


def mix_inputs(case, mix):
  """(dy | None, dhT | None, dcT | None) of a gradient mix."""
  use_dy, use_h, use_c = MIXES[mix]
  dhT, dcT = state_grads(case)
  return (C.build_inputs(case)["dy"] if use_dy else None), (dhT if use_h else None), (dcT if use_c else None)


def backward_state_oracle(xhat, s_hat, rstd, dy, dhT, dcT, wh, ln, lens, mask=None, keep=1.0, c0=None,
                          forget_bias=C.FORGET_BIAS, rounded=False, mutate=None, dtype=torch.float64):
  """Backward through time in float64 with gradients on y (dy | None), hT (dhT | None) and cT (dcT | None).
  Returns dict(dgx [B,T,4H], dln [10,H])."""
  xhat, s_hat, rstd, wh, ln = (v.to(dtype) for v in (xhat, s_hat, rstd, wh, ln))
  B, T, H = s_hat.shape
  lnv = C.eff_lens(lens, B, T)
  last = torch.full_like(lnv, T - 1) if mutate == "entry_at_T" else lnv - 1
  rd = C.rb if rounded else C._id
  gam, bet = ln[0::2], ln[1::2]
  zero = torch.zeros((), dtype=dtype)
  zbh = torch.zeros(B, H, dtype=dtype)
  dy = torch.zeros(B, T, H, dtype=dtype) if dy is None else dy.to(dtype)
  dhT = zbh if dhT is None else dhT.to(dtype)
  dcT = zbh if dcT is None or mutate == "no_dcT" else dcT.to(dtype)
  dgx = torch.zeros(B, T, 4 * H, dtype=dtype)
  dln = torch.zeros(10, H, dtype=dtype)
  dcc = zbh
  dg_next = torch.zeros(B, 4 * H, dtype=dtype)
  for t in range(T - 1, -1, -1):
    act = (t < lnv)[:, None]
    enter = (last == t)[:, None]
    dh = dy[:, t] + dg_next @ wh + torch.where(enter, dhT, zero)
    xh, sh, rs = xhat[:, t].view(B, 4, H), s_hat[:, t], rstd[:, t]
    n = gam[None, :4] * xh + bet[None, :4]
    ig, tj, fg, og = C._sig(n[:, 0]), torch.tanh(n[:, 1]), C._sig(n[:, 2] + forget_bias), C._sig(n[:, 3])
    tc = torch.tanh(gam[4] * sh + bet[4])
    if t > 0:
      cprev = gam[4] * s_hat[:, t - 1] + bet[4]
    else:
      cprev = zbh if c0 is None else c0.to(dtype)
    dc = dh * og * (1.0 - tc * tc) + dcc
    if mutate != "dcT_before_state_ln":
      dc = dc + torch.where(enter, dcT, zero)
    ds = dc * gam[4]
    dct = rs[:, 4:5] * (ds - ds.mean(1, keepdim=True) - sh * (ds * sh).mean(1, keepdim=True))
    if mutate == "dcT_before_state_ln":
      dct = dct + torch.where(enter, dcT, zero)
    mk = torch.ones(B, H, dtype=dtype) if mask is None else mask[:, t].to(dtype) / keep
    dn = torch.stack([dct * tj * mk * ig * (1.0 - ig), dct * ig * mk * (1.0 - tj * tj),
                      dct * cprev * fg * (1.0 - fg), dh * tc * og * (1.0 - og)], dim=1)
    dx = dn * gam[None, :4]
    da = rs[:, :4, None] * (dx - dx.mean(2, keepdim=True) - xh * (dx * xh).mean(2, keepdim=True))
    a3 = act[:, :, None]
    dln[0:8:2] += torch.where(a3, dn * xh, zero).sum(0)
    dln[1:8:2] += torch.where(a3, dn, zero).sum(0)
    dln[8] += torch.where(act, dc * sh, zero).sum(0)
    dln[9] += torch.where(act, dc, zero).sum(0)
    dcc = torch.where(act, dct * fg, dcc)
    dg_next = torch.where(act, rd(da.reshape(B, 4 * H)), zero)
    dgx[:, t] = dg_next
  return dict(dgx=dgx, dln=dln)


def reference_state_bwd(case, mix, saved, rounded, mask=None, mutate=None):
  d = C.build_inputs(case)
  dy, dhT, dcT = mix_inputs(case, mix)
  with torch.no_grad():
    return backward_state_oracle(saved["xhat"], saved["s_hat"], saved["rstd"], dy, dhT, dcT, d["wh"], d["ln"],
                                 d["lens"], d["mask"] if mask is None else mask, d["keep"], d["c0"], rounded=rounded,
                                 mutate=mutate)


@functools.lru_cache(maxsize=None)
def state_noise_floor(case, mix):
  """n_q of dgx / dln: max |R_b - R| of the state-gradient backward, teacher-forced on the forward R_b."""
  Rb = C.reference_fwd(case, True)
  G, Gb = reference_state_bwd(case, mix, Rb, False), reference_state_bwd(case, mix, Rb, True)
  return {q: float((C._live(case, q, Gb[q]) - C._live(case, q, G[q])).abs().max()) for q in C.BWD_OUT}


def run_state_gpu(case, device, fw=None):
  """The forward of a case once (or `fw`, a dict of device tensors from an earlier call) and, per mix, the new
  backward. Returns (fw on the device, {mix: dict(dgx, dln) on the CPU}, extras) where extras holds the runs the
  exact checks need: 'zeros_dy' (state_only with dy = zeros), 'plain' (os2s_lnlstm_layer_bwd), 'state_null'
  (the new entry with dhT = dcT = NULL), 'again' (mix 'all' a second time)."""
  from openseq2seq_amd import capi
  s = C.spec(case)
  H = s["H"]
  d = C.build_inputs(case)
  dev = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in d.items()}
  if fw is None:
    fw = capi.lnlstm_layer_fwd(dev["gx"], dev["wh"], dev["ln"], dev["lens"], H, C.FORGET_BIAS, d["keep"], d["seed"],
                               dev["h0"], dev["c0"], save=True, want_state=True)
  whT = dev["wh"].t().contiguous()

  def bwd(dy, dhT, dcT):
    to = lambda v: None if v is None else v.to(device)
    dgx, dln = capi.lnlstm_layer_bwd_state(whT, dev["ln"], dev["lens"], to(dy), to(dhT), to(dcT), fw["xhat"],
                                           fw["s_hat"], fw["rstd"], H, C.FORGET_BIAS, d["keep"], d["seed"], dev["c0"])
    return dict(dgx=dgx.cpu(), dln=dln.cpu())

  out = {mix: bwd(*mix_inputs(case, mix)) for mix in MIXES}
  dhT, dcT = state_grads(case)
  extras = dict(zeros_dy=bwd(torch.zeros_like(d["dy"]), dhT, dcT), state_null=bwd(d["dy"], None, None),
                again=bwd(*mix_inputs(case, "all")))
  dgx, dln = capi.lnlstm_layer_bwd(whT, dev["ln"], dev["lens"], dev["dy"], fw["xhat"], fw["s_hat"], fw["rstd"], H,
                                   C.FORGET_BIAS, d["keep"], d["seed"], dev["c0"])
  extras["plain"] = dict(dgx=dgx.cpu(), dln=dln.cpu())
  torch.cuda.synchronize()
  return fw, out, extras


# ------------------------------------------------------------------------------------------ head
@functools.lru_cache(maxsize=None)
def head_inputs(case):
  """Inputs of a head case from a seeded CPU generator: states ~ N(0,1) fp32, W ~ U(+-1/sqrt(D)) drawn
  bf16-representable, bias 0.1 N, labels one-hot except row 0, which is soft (a random distribution scaled by 0.9,
  so sum_c y_c != 1 shows in dlogits), g0W / g0b the values the gradients are accumulated into."""
  B, H, Cn, cell = HEAD_CASES[case]
  D = 2 * H if cell else H
  g = torch.Generator().manual_seed(sum(map(ord, "head-" + case)))
  h, c = torch.randn(B, H, generator=g), (torch.randn(B, H, generator=g) if cell else None)
  w = ((torch.rand(Cn, D, generator=g) * 2 - 1) / math.sqrt(D)).to(torch.bfloat16)
  bias = 0.1 * torch.randn(Cn, generator=g)
  y = torch.nn.functional.one_hot(torch.randint(0, Cn, (B,), generator=g), Cn).float()
  soft = torch.rand(Cn, generator=g)
  y[0] = 0.9 * soft / soft.sum()
  g0w, g0b = torch.randn(Cn, D, generator=g), torch.randn(Cn, generator=g)
  return dict(h=h, c=c, w=w, bias=bias, y=y, g0w=g0w, g0b=g0b, B=B, H=H, C=Cn, D=D)


def _state(h, c, mutate=None):
  if c is None:
    return h.double()
  return torch.cat([c, h] if mutate == "c_then_h" else [h, c], dim=1).double()


def head_fwd_oracle(h, c, w, bias, mutate=None):
  """(logits [B,C], S, n): float64 value, sum of absolute terms, number of terms."""
  s, w, bias = _state(h, c, mutate), w.double(), bias.double()
  return s @ w.t() + bias, s.abs() @ w.abs().t() + bias.abs(), s.shape[1] + 1


def xent_oracle(logits, y, scale=1.0, mutate=None):
  """dict(loss=(R, S, n), dlogits=(R, S, n)) of softmax cross-entropy with dense labels, from given logits."""
  l, y = logits.double(), y.double()
  B, Cn = l.shape
  sh = l - l.max(1, keepdim=True).values
  lse = torch.log(torch.exp(sh).sum(1, keepdim=True))
  terms = y * (lse - sh)
  div = B * Cn if mutate == "loss_over_BC" else B
  p, ysum = torch.exp(sh - lse), y.sum(1, keepdim=True)
  k = scale / B
  return dict(loss=(terms.sum() / div, terms.abs().sum() / div, B * Cn + Cn + 8),
              dlogits=((p * ysum - y) * k, ((p * ysum).abs() + y.abs()) * k, 2 + Cn + 8))


def head_bwd_oracle(h, c, w, dl, g0w, g0b, mutate=None):
  """dict(dw, dbias, ds = (R, S, n)) from given dlogits; ds [B,D] is [dhT, dcT]."""
  s, w, dl = _state(h, c, mutate), w.double(), dl.double()
  B, Cn = dl.shape
  return dict(dw=(g0w.double() + dl.t() @ s, g0w.double().abs() + dl.abs().t() @ s.abs(), B + 1),
              dbias=(g0b.double() + dl.sum(0), g0b.double().abs() + dl.abs().sum(0), B + 1),
              ds=(dl @ w, dl.abs() @ w.abs(), Cn))


def head_within(got, ref, what, log=None):
  """got against ref = (R, S, n) under n 2^-23 S. Returns (ok, max err / bound)."""
  R, S, n = ref
  err = (got.double() - R).abs()
  bound = n * U * S
  ok = bool((err <= bound).all())                    # a NaN fails
  ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), err))
  worst = float(torch.nan_to_num(ratio, nan=float("inf")).max())
  if log:
    log("  %-4s %s: n %d, max err %.3e, max err/bound %.3e" % ("ok" if ok else "FAIL", what, n, float(err.max()), worst))
  return ok, worst


def run_head_gpu(case, scale, device, want_grad=True):
  """The three entries on the device. Returns CPU tensors dict(logits, loss, dlogits, dw, dbias, dh, dc)."""
  from openseq2seq_amd import capi
  d = head_inputs(case)
  to = lambda v: None if v is None else v.to(device)
  h, c, w, bias, y = to(d["h"]), to(d["c"]), to(d["w"]), to(d["bias"]), to(d["y"])
  sc = torch.tensor([scale], dtype=torch.float32, device=device)
  logits = capi.text_cls_fwd(h, c, w, bias)
  loss, dl = capi.softmax_xent_dense(logits, y, grad_scale_dev=sc, want_grad=want_grad)
  out = dict(logits=logits.cpu(), loss=loss.cpu(), dlogits=None)
  if want_grad:
    dw, db = to(d["g0w"]).clone(), to(d["g0b"]).clone()
    dh, dc = capi.text_cls_bwd(h, c, w, dl, dw, db)
    out.update(dlogits=dl.cpu(), dw=dw.cpu(), dbias=db.cpu(), dh=dh.cpu(), dc=None if dc is None else dc.cpu())
  torch.cuda.synchronize()
  return out


def check_head(case, scale, got, log=print):
  """Every stage of `got` against the oracle, teacher-forced stage by stage. Returns the failures."""
  d = head_inputs(case)
  fails = []

  def hold(q, t, ref):
    ok, worst = head_within(t, ref, "%s x%g %s" % (case, scale, q), log)
    if not ok:
      fails.append("%s x%g: %s err/bound %.3e" % (case, scale, q, worst))

  hold("logits", got["logits"], head_fwd_oracle(d["h"], d["c"], d["w"], d["bias"]))
  x = xent_oracle(got["logits"], d["y"], scale)
  hold("loss", got["loss"][0], x["loss"])
  hold("dlogits", got["dlogits"], x["dlogits"])
  b = head_bwd_oracle(d["h"], d["c"], d["w"], got["dlogits"], d["g0w"], d["g0b"])
  hold("dw", got["dw"], b["dw"])
  hold("dbias", got["dbias"], b["dbias"])
  ds = got["dh"] if got["dc"] is None else torch.cat([got["dh"], got["dc"]], dim=1)
  hold("dhT|dcT", ds, b["ds"])
  return fails
