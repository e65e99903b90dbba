"""Helper of tests/test_lnlstm_paths_gpu.py and tests/test_lnlstm_oracle_cpu.py (not a test module): the case
table that reaches every kernel instance of os2s_lnlstm_layer_fwd / os2s_lnlstm_layer_bwd, a float64 oracle of
the LayerNorm-LSTM recurrence alone (it takes gx, not x), the device run and the comparison of the two.

Oracle. forward_oracle() is the cell of csrc/lnlstm.hip:3-11 / include/os2s.h in float64: R plainly, R_b with a
bf16 round exactly where the kernels store bf16 (the h fed to the next step's product, y, the saved xhat; the
pre-activations, the carried c, s_hat, rstd, hT, cT stay fp32 on the device and unrounded here).
backward_oracle() is teacher-forced on what the kernel itself saved (xhat, s_hat, rstd as read back from the
device) plus dy, wh, ln, c0 and the mask, so the forward's rounding stays out of the backward bound; R_b rounds
dgx, which is also what the product of the step before reads. tests/test_lnlstm_oracle_cpu.py holds the
backward oracle against autograd of the forward oracle.

compare(): every output elementwise on live rows,
    |got - R_b| <= 4 n_q + 2^-7 |R_b|
n_q = max |R_b.q - R.q| of the case (noise_floor(): oracle alone, on the CPU; for the backward outputs the
teacher is the forward R_b). Exact: y and dgx rows at or past a sample's length are zero; the guard columns of
the strided run keep their sentinel and a contiguous rerun gives the same bits; a rerun is bit-identical, dln
included; without dropout a T-step call equals T one-step calls chained through h0 / c0 -> hT / cT; the mask of
the keep < 1 case is read from capi.dropout_mask at the same seed and indices and equals the host restatement
of the counter hash that the CPU tests use.

Kernel instances per case, read off the host code (lnlstm.hip: cell<NCH> with NCH = 1 up to H = 512, 2 up to
1024, 4 above; product backward rows8 = ceil(H/32) ceil(B/32) < 128). pf = lnlstm_prod_fwd_kernel, cf<N> =
lnlstm_cell_fwd_kernel<N>, pb<R> = lnlstm_prod_bwd_kernel<R>, cb<N> = lnlstm_cell_bwd_kernel<N>:
  h8           pf, cf<1>, pb<8>, cb<1>; H = 8: the K - 8 clamp of tile_gemm_prefetch is 0, lanes 1..63 of the cell
               wave idle; lengths 0 and T + 3 (the clamps)
  t1_h24       T = 1: no product backward launch at all, no c_{t-1} from s_hat; K = 24, K % 16 == 8
  b33_h24      second batch tile of both product launches holding one sample; strided y / dy with guard columns
  rows32_h72   pb<32> (3 x 43 = 129 >= 128) with H % 32 = 8 (the j0 + l31 < H row guard) and H % 64 != 0
  h520         cf<2>, cb<2>: lanes 1..63 own one chunk, lane 0 two
  h1032        cf<4>, cb<4>; pf two rounds (K = 1032 > 8 waves x 8 x 16), pb<8> three rounds (4128 > 2 x 2048)
  h2048        the top of the contract: every lane owns four chunks; pb<8> four rounds
  keep07_h40   keep 0.7 (seeded mask by (b, t, unit)), ragged
  state_h24    h0 / c0 given, hT / cT read, ragged

Measured on the MI355X when this file was written (the tests compute their own n_q), per case: n_q, then the
largest err / bound per output (0: bit-identical to R_b); largest of all 0.29 (rows32_h72 y):
  h8          n_q  y 1.9e-03 xhat 7.4e-03 s_hat 7.9e-04 rstd 9.3e-04 hT 3.0e-04 cT 8.4e-04 dgx 3.7e-03 dln 2.7e-03
              e/b  y 0.0e+00 xhat 0.0e+00 s_hat 7.7e-05 rstd 1.8e-05 hT 2.7e-05 cT 7.0e-05 dgx 0.0e+00 dln 5.0e-05
  t1_h24      n_q  y 1.7e-03 xhat 6.4e-03 s_hat 0.0e+00 rstd 0.0e+00 hT 0.0e+00 cT 0.0e+00 dgx 3.7e-03 dln 0.0e+00
              e/b  y 0.0e+00 xhat 0.0e+00 s_hat 6.6e-04 rstd 1.2e-05 hT 1.7e-03 cT 1.7e-03 dgx 2.1e-03 dln 5.2e-04
  b33_h24     n_q  y 2.0e-03 xhat 8.2e-03 s_hat 1.1e-03 rstd 2.5e-04 hT 5.8e-04 cT 1.0e-03 dgx 1.6e-02 dln 2.1e-03
              e/b  y 0.0e+00 xhat 0.0e+00 s_hat 5.3e-05 rstd 1.7e-05 hT 6.4e-05 cT 5.7e-05 dgx 0.0e+00 dln 6.9e-05
  rows32_h72  n_q  y 2.3e-03 xhat 1.5e-02 s_hat 1.6e-03 rstd 1.8e-04 hT 9.9e-04 cT 1.8e-03 dgx 2.2e-02 dln 1.1e-02
              e/b  y 2.9e-01 xhat 1.2e-01 s_hat 4.5e-02 rstd 4.6e-03 hT 4.6e-02 cT 4.5e-02 dgx 2.2e-02 dln 4.6e-03
  h520        n_q  y 2.0e-03 xhat 7.8e-03 s_hat 8.8e-04 rstd 7.8e-06 hT 5.2e-04 cT 8.5e-04 dgx 7.1e-03 dln 5.7e-04
              e/b  y 0.0e+00 xhat 0.0e+00 s_hat 4.2e-05 rstd 1.4e-05 hT 3.2e-05 cT 4.7e-05 dgx 0.0e+00 dln 8.2e-05
  h1032       n_q  y 2.0e-03 xhat 1.3e-02 s_hat 1.1e-03 rstd 1.5e-05 hT 4.6e-04 cT 1.4e-03 dgx 9.4e-03 dln 1.1e-03
              e/b  y 0.0e+00 xhat 0.0e+00 s_hat 5.1e-05 rstd 1.3e-05 hT 6.1e-05 cT 4.0e-05 dgx 1.3e-02 dln 9.5e-05
  h2048       n_q  y 2.0e-03 xhat 8.4e-03 s_hat 8.1e-04 rstd 6.0e-06 hT 4.5e-04 cT 9.4e-04 dgx 1.4e-02 dln 8.8e-04
              e/b  y 0.0e+00 xhat 0.0e+00 s_hat 5.6e-05 rstd 1.3e-05 hT 7.0e-05 cT 5.3e-05 dgx 0.0e+00 dln 8.1e-05
  keep07_h40  n_q  y 2.0e-03 xhat 7.8e-03 s_hat 1.1e-03 rstd 1.7e-04 hT 4.4e-04 cT 1.2e-03 dgx 5.6e-03 dln 2.2e-03
              e/b  y 0.0e+00 xhat 0.0e+00 s_hat 7.1e-05 rstd 1.4e-05 hT 4.9e-05 cT 4.3e-05 dgx 2.7e-03 dln 3.4e-04
  state_h24   n_q  y 2.2e-03 xhat 8.2e-03 s_hat 1.5e-03 rstd 2.6e-04 hT 7.6e-04 cT 1.3e-03 dgx 3.8e-03 dln 5.7e-04
              e/b  y 0.0e+00 xhat 0.0e+00 s_hat 4.0e-05 rstd 1.6e-05 hT 4.4e-05 cT 5.1e-05 dgx 0.0e+00 dln 6.8e-05"""
import functools
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
  sys.path.insert(0, REPO)

RAGGED = "ragged"
# name: B, T, H, lens, strided, keep, initial state given
CASES = {
    "h8": (5, 7, 8, [7, 1, 4, 0, 10], False, 1.0, False),
    "t1_h24": (3, 1, 24, None, False, 1.0, False),
    "b33_h24": (33, 4, 24, RAGGED, True, 1.0, False),
    "rows32_h72": (1345, 3, 72, RAGGED, False, 1.0, False),
    "h520": (2, 2, 520, RAGGED, False, 1.0, False),
    "h1032": (3, 3, 1032, RAGGED, False, 1.0, False),
    "h2048": (2, 2, 2048, RAGGED, False, 1.0, False),
    "keep07_h40": (4, 5, 40, RAGGED, False, 0.7, False),
    "state_h24": (3, 4, 24, RAGGED, False, 1.0, True),
}
FORGET_BIAS = 1.0
EPS = 1e-12
SENTINEL = -7.0
GUARD = 8
FWD_OUT = ("y", "xhat", "s_hat", "rstd", "hT", "cT")
BWD_OUT = ("dgx", "dln")
MUTATIONS = ("no_state_ln", "carry_unnormalised", "no_forget_bias", "gate_order_ifjo", "unbiased_variance",
             "swap_gamma_beta_gates", "no_keep_scale", "mask_by_live_row")
_GOLD = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def spec(case):
  B, T, H, lens, strided, keep, state = CASES[case]
  return dict(B=B, T=T, H=H, lens=lens, strided=strided, keep=keep, state=state)


def rb(x):
  """bf16 round of a float64 tensor (round to nearest even, as f2bf)."""
  return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _id(x):
  return x


def host_mask(seed, n_elems, keep):
  """The keep mask of dropout_bits8 (csrc/os2s_common.hpp) for elements 0 .. n_elems - 1, restated on the host:
  bool [n_elems]."""
  assert n_elems % 4 == 0
  thr = int(np.float32(keep) * np.float32(65536.0))
  with np.errstate(over="ignore"):
    z = np.arange(n_elems // 4, dtype=np.uint64) * np.uint64(_GOLD) + np.uint64(seed & _M64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
  u = np.stack([(z >> np.uint64(16 * e)) & np.uint64(0xffff) for e in range(4)], axis=1).astype(np.int64)
  return torch.from_numpy((u < thr).reshape(-1))


@functools.lru_cache(maxsize=None)
def build_inputs(case):
  """Inputs of one case from a seeded CPU generator: gx, dy ~ N(0,1) and wh ~ U(+-1/sqrt(H)) rounded to bf16, ln
  = gamma (1 + 0.1 N) / beta (0.1 N) rows fp32, so that every LayerNorm row has a variance of order 1. CPU tensors;
  callers must not modify them."""
  s = spec(case)
  B, T, H = s["B"], s["T"], s["H"]
  g = torch.Generator().manual_seed(sum(map(ord, "lnlstm-" + case)))
  lens = s["lens"]
  if lens == RAGGED:
    lens = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    lens[0], lens[1] = T, 1
  elif lens is not None:
    lens = torch.tensor(lens, dtype=torch.int32)
  gx = torch.randn(B, T, 4 * H, generator=g).to(torch.bfloat16)
  wh = ((torch.rand(4 * H, H, generator=g) * 2.0 - 1.0) / math.sqrt(H)).to(torch.bfloat16)
  ln = 0.1 * torch.randn(10, H, generator=g)
  ln[0::2] += 1.0
  dy = torch.randn(B, T, H, generator=g).to(torch.bfloat16)
  h0 = c0 = None
  if s["state"]:
    h0, c0 = 0.5 * torch.randn(B, H, generator=g), 0.5 * torch.randn(B, H, generator=g)
  seed = 0x5eed0000 + sum(map(ord, case))
  mask = None
  if s["keep"] < 1.0:
    mask = host_mask(seed, B * T * H, s["keep"]).view(B, T, H)
  return dict(lens=lens, gx=gx, wh=wh, ln=ln.float(), dy=dy, h0=h0, c0=c0, seed=seed, keep=s["keep"], mask=mask)


def eff_lens(lens, B, T):
  return torch.full((B,), T, dtype=torch.int64) if lens is None else lens.to(torch.int64).clamp(0, T)


def live_steps(case):
  s = spec(case)
  ln = eff_lens(build_inputs(case)["lens"], s["B"], s["T"])
  return torch.arange(s["T"])[None, :] < ln[:, None]


def _sig(x):
  return 1.0 / (1.0 + torch.exp(-x))


def layer_norm(x, gamma, beta, unbiased=False):
  """tf.contrib.layers.layer_norm(begin_norm_axis=1) of [B,H]: (gamma xhat + beta, xhat, rstd [B])."""
  H = x.shape[1]
  d = x - x.mean(1, keepdim=True)
  var = (d * d).sum(1, keepdim=True) / (H - 1 if unbiased else H)
  rstd = 1.0 / torch.sqrt(var + EPS)
  xhat = d * rstd
  return gamma * xhat + beta, xhat, rstd[:, 0]


def forward_oracle(gx, wh, ln, lens, mask=None, keep=1.0, h0=None, c0=None, forget_bias=FORGET_BIAS, rounded=False,
                   mutate=None, dtype=torch.float64):
  """The recurrence in float64 (differentiable: no in-place writes). gx [B,T,4H], wh [4H,H], ln [10,H], lens [B]
  | None, mask bool [B,T,H] | None. Returns dict(y [B,T,H], xhat [B,T,4H], s_hat [B,T,H], rstd [B,T,5], hT, cT);
  rows of finished steps are zero. dtype=torch.float32 (unrounded only): the same arithmetic in fp32, from which
  the fixture test takes its round-off bound."""
  assert dtype == torch.float64 or not rounded
  gx, wh, ln = gx.to(dtype), wh.to(dtype), ln.to(dtype)
  B, T, _ = gx.shape
  H = wh.shape[1]
  lnv = eff_lens(lens, B, T)
  rd = rb if rounded else _id
  gam, bet = ln[0::2], ln[1::2]
  if mutate == "swap_gamma_beta_gates":
    perm = [2, 1, 0, 3, 4]                      # the input gate gets the forget gate's pair and back
    gam, bet = gam[perm], bet[perm]
  role = (0, 2, 1, 3) if mutate == "gate_order_ifjo" else (0, 1, 2, 3)   # block of a holding i, j, f, o
  fb = 0.0 if mutate == "no_forget_bias" else forget_bias
  unb = mutate == "unbiased_variance"
  h = torch.zeros(B, H, dtype=dtype) if h0 is None else h0.to(dtype)
  c = torch.zeros(B, H, dtype=dtype) if c0 is None else c0.to(dtype)
  mk_all = None
  if mask is not None:
    mk_all = mask.to(dtype)
    if mutate == "mask_by_live_row":            # rows counted over live steps only instead of b T + t
      live = (torch.arange(T)[None, :] < lnv[:, None]).reshape(-1)
      packed = mask.reshape(B * T, H)[: int(live.sum())].to(dtype)
      mk_all = torch.zeros(B * T, H, dtype=dtype)
      mk_all[live] = packed
      mk_all = mk_all.view(B, T, H)
    if mutate != "no_keep_scale":
      mk_all = mk_all / keep
  ys, xhs, shs, rss = [], [], [], []
  zero = torch.zeros((), dtype=dtype)
  for t in range(T):
    act = (t < lnv)[:, None]
    a = (gx[:, t] + rd(h) @ wh.t()).view(B, 4, H)
    n, xh, rs = [None] * 4, [None] * 4, [None] * 5
    for g in range(4):
      n[g], xh[g], rs[g] = layer_norm(a[:, role[g]], gam[g], bet[g], unb)
    cand = torch.tanh(n[1])
    if mk_all is not None:
      cand = cand * mk_all[:, t]
    ct = c * _sig(n[2] + fb) + _sig(n[0]) * cand
    if mutate == "no_state_ln":
      cn, sh, rs[4] = ct, ct, torch.ones(B, dtype=dtype)
    else:
      cn, sh, rs[4] = layer_norm(ct, gam[4], bet[4], unb)
    hn = torch.tanh(cn) * _sig(n[3])
    h = torch.where(act, hn, h)
    c = torch.where(act, ct if mutate == "carry_unnormalised" else cn, c)
    xcat = torch.cat([xh[role.index(k)] for k in range(4)], dim=1)      # saved in the block order of a
    ys.append(torch.where(act, rd(hn), zero))
    xhs.append(torch.where(act, rd(xcat), zero))
    shs.append(torch.where(act, sh, zero))
    rss.append(torch.where(act, torch.stack([rs[role.index(k)] for k in range(4)] + [rs[4]], dim=1), zero))
  return dict(y=torch.stack(ys, 1), xhat=torch.stack(xhs, 1), s_hat=torch.stack(shs, 1), rstd=torch.stack(rss, 1),
              hT=h, cT=c)


def backward_oracle(xhat, s_hat, rstd, dy, wh, ln, lens, mask=None, keep=1.0, c0=None, forget_bias=FORGET_BIAS,
                    rounded=False, dtype=torch.float64):
  """Backward through time in float64, teacher-forced on the saved xhat / s_hat / rstd. Returns dict(dgx
  [B,T,4H] = d a, zero on finished steps, dln [10,H])."""
  xhat, s_hat, rstd, dy, wh, ln = (v.to(dtype) for v in (xhat, s_hat, rstd, dy, wh, ln))
  B, T, H = dy.shape
  lnv = eff_lens(lens, B, T)
  rd = rb if rounded else _id
  gam, bet = ln[0::2], ln[1::2]
  dgx = torch.zeros(B, T, 4 * H, dtype=dtype)
  dln = torch.zeros(10, H, dtype=dtype)
  dcc = torch.zeros(B, H, dtype=dtype)
  dg_next = torch.zeros(B, 4 * H, dtype=dtype)
  zero = torch.zeros((), dtype=dtype)
  for t in range(T - 1, -1, -1):
    act = (t < lnv)[:, None]
    dh = dy[:, t] + dg_next @ wh
    xh, sh, rs = xhat[:, t].view(B, 4, H), s_hat[:, t], rstd[:, t]
    n = gam[None, :4] * xh + bet[None, :4]
    ig, tj, fg, og = _sig(n[:, 0]), torch.tanh(n[:, 1]), _sig(n[:, 2] + forget_bias), _sig(n[:, 3])
    tc = torch.tanh(gam[4] * sh + bet[4])
    if t > 0:
      cprev = gam[4] * s_hat[:, t - 1] + bet[4]
    else:
      cprev = torch.zeros(B, H, dtype=dtype) if c0 is None else c0.to(dtype)
    dc = dh * og * (1.0 - tc * tc) + dcc
    ds = dc * gam[4]
    dct = rs[:, 4:5] * (ds - ds.mean(1, keepdim=True) - sh * (ds * sh).mean(1, keepdim=True))
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


_FWD_CACHE = {}


def reference_fwd(case, rounded, mask=None):
  """Forward oracle of a case, computed once (callers must not modify it). mask: the device's own mask of the
  keep < 1 case (default: the host restatement)."""
  key = (case, rounded, mask is not None)
  if key not in _FWD_CACHE:
    d = build_inputs(case)
    with torch.no_grad():
      _FWD_CACHE[key] = forward_oracle(d["gx"], d["wh"], d["ln"], d["lens"], d["mask"] if mask is None else mask,
                                       d["keep"], d["h0"], d["c0"], rounded=rounded)
  return _FWD_CACHE[key]


def reference_bwd(case, saved, rounded, mask=None):
  d = build_inputs(case)
  with torch.no_grad():
    return backward_oracle(saved["xhat"], saved["s_hat"], saved["rstd"], d["dy"], d["wh"], d["ln"], d["lens"],
                           d["mask"] if mask is None else mask, d["keep"], d["c0"], rounded=rounded)


def _live(case, q, t):
  """Live rows of a per-step output, zeros elsewhere (never a product with the mask); hT / cT / dln whole."""
  t = t.double()
  if q in ("hT", "cT", "dln"):
    return t
  return torch.where(live_steps(case)[:, :, None], t, torch.zeros((), dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def noise_floor(case):
  """n_q[q] = max|R_b.q - R.q| of the case: what the bf16 stores of the recurrence cost. Oracle alone; the
  backward is teacher-forced on the forward R_b."""
  R, Rb = reference_fwd(case, False), reference_fwd(case, True)
  G, Gb = reference_bwd(case, Rb, False), reference_bwd(case, Rb, True)
  a, b = dict(R, **G), dict(Rb, **Gb)
  return {q: float((_live(case, q, b[q]) - _live(case, q, a[q])).abs().max()) for q in FWD_OUT + BWD_OUT}


def within(case, got, ref, nq, log=None):
  """[(output, ok, max err, max err / bound)] of `got` against `ref` under 4 n_q + 2^-7 |ref|."""
  out = []
  for q in FWD_OUT + BWD_OUT:
    if q not in got:
      continue
    a, r = _live(case, q, got[q]), _live(case, q, ref[q])
    err = (a - r).abs()
    bound = 4.0 * nq[q] + 2.0 ** -7 * r.abs()
    ok = bool((err <= bound).all())                  # a NaN fails
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), err))
    out.append((q, ok, float(torch.nan_to_num(err, nan=float("inf")).max()),
                float(torch.nan_to_num(ratio, nan=float("inf")).max())))
    if log:
      log("  %-4s %s %s vs R_b (n_q %.3e): max err %.3e, max err/bound %.3e" % (("ok" if ok else "FAIL", case, q, nq[q])
                                                                                + out[-1][2:]))
  return out


# ------------------------------------------------------------------------------------------ device
def run_gpu(case, device, strided=None):
  """Forward and backward of one case through capi.lnlstm_layer_{fwd,bwd}. Returns CPU tensors dict(y, xhat,
  s_hat, rstd, hT, cT, dgx, dln[, wide_y, wide_dy])."""
  from openseq2seq_amd import capi
  s = spec(case)
  B, T, H = s["B"], s["T"], s["H"]
  d = build_inputs(case)
  strided = s["strided"] if strided is None else strided
  dev = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in d.items()}
  y, dy = None, dev["dy"]
  if strided:
    wy = torch.full((B, T, GUARD + H + GUARD), SENTINEL, dtype=torch.bfloat16, device=device)
    wdy = torch.full_like(wy, SENTINEL)
    y, dy = wy[:, :, GUARD:GUARD + H], wdy[:, :, GUARD:GUARD + H]
    dy.copy_(dev["dy"])
  fw = capi.lnlstm_layer_fwd(dev["gx"], dev["wh"], dev["ln"], dev["lens"], H, FORGET_BIAS, d["keep"], d["seed"],
                             dev["h0"], dev["c0"], y=y, save=True, want_state=True)
  torch.cuda.synchronize()
  dgx, dln = capi.lnlstm_layer_bwd(dev["wh"].t().contiguous(), dev["ln"], dev["lens"], dy, fw["xhat"], fw["s_hat"],
                                   fw["rstd"], H, FORGET_BIAS, d["keep"], d["seed"], dev["c0"])
  torch.cuda.synchronize()
  out = {k: v.cpu().contiguous() for k, v in fw.items()}
  out.update(dgx=dgx.cpu(), dln=dln.cpu())
  if strided:
    out.update(wide_y=wy.cpu(), wide_dy=wdy.cpu())
  return out


def run_gpu_chained(case, device):
  """The forward as T one-step calls chained through h0 / c0 -> hT / cT (no dropout: a one-step call indexes its
  mask with T = 1). Returns CPU dict(y, xhat, s_hat, rstd, hT, cT)."""
  from openseq2seq_amd import capi
  s = spec(case)
  B, T, H = s["B"], s["T"], s["H"]
  d = build_inputs(case)
  assert d["keep"] == 1.0
  dev = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in d.items()}
  h, c = dev["h0"], dev["c0"]
  parts = []
  for t in range(T):
    lens_t = None if dev["lens"] is None else (dev["lens"] > t).to(torch.int32)
    fw = capi.lnlstm_layer_fwd(dev["gx"][:, t:t + 1].contiguous(), dev["wh"], dev["ln"], lens_t, H, FORGET_BIAS, 1.0, 0,
                               h, c, save=True, want_state=True)
    h, c = fw["hT"], fw["cT"]
    parts.append(fw)
  torch.cuda.synchronize()
  out = {k: torch.cat([p[k] for p in parts], dim=1).cpu() for k in ("y", "xhat", "s_hat", "rstd")}
  out.update(hT=h.cpu(), cT=c.cpu())
  return out


def _bits(t):
  return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
  return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def check_case(case, device, log=print):
  """Device runs of one case and every assertion on them; returns the failures (empty: pass)."""
  from openseq2seq_amd import capi
  s = spec(case)
  B, T, H = s["B"], s["T"], s["H"]
  d = build_inputs(case)
  fails = []

  def check(ok, what):
    log("  %-4s %s %s" % ("ok" if ok else "FAIL", case, what))
    if not ok:
      fails.append("%s: %s" % (case, what))

  got = run_gpu(case, device)
  mask = None
  if d["keep"] < 1.0:
    mask = capi.dropout_mask(d["seed"], B * T * H, d["keep"], device).cpu().view(B, T, H)
    check(torch.equal(mask, d["mask"]), "capi.dropout_mask equals the host restatement at (seed, (b T + t) H + unit)")
    frac = float(mask.double().mean())
    check(abs(frac - d["keep"]) < 0.1, "mask keeps %.3f of the elements (keep %.2f)" % (frac, d["keep"]))
  Rb = reference_fwd(case, True, mask)
  Gb = reference_bwd(case, got, True, mask)
  for q, ok, err, ratio in within(case, got, dict(Rb, **Gb), noise_floor(case), log=log):
    if not ok:
      fails.append("%s: %s max err %.3e, err/bound %.3e" % (case, q, err, ratio))
  dead = ~live_steps(case)
  if bool(dead.any()):
    for q in ("y", "dgx"):
      check(bool((got[q].double()[dead] == 0.0).all()), "%s rows of finished steps exactly zero" % q)
  if s["strided"]:
    for k in ("wide_y", "wide_dy"):
      guard = torch.cat([got[k][:, :, :GUARD], got[k][:, :, GUARD + H:]], dim=2)
      check(same_bits(guard, torch.full_like(guard, SENTINEL)), "guard columns of %s untouched" % k)
    plain = run_gpu(case, device, strided=False)
    for q in FWD_OUT + BWD_OUT:
      check(same_bits(got[q], plain[q]), "%s bit-identical to the contiguous run" % q)
  again = run_gpu(case, device)
  for q in FWD_OUT + BWD_OUT:
    check(same_bits(got[q], again[q]), "%s bit-identical on a rerun" % q)
  if d["keep"] == 1.0:
    chain = run_gpu_chained(case, device)
    for q in FWD_OUT:
      check(same_bits(got[q], chain[q]), "%s of the T-step call bit-identical to T chained one-step calls" % q)
  return fails
