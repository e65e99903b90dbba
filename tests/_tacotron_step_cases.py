"""Helper of tests/test_tacotron_step_kernels_gpu.py and tests/test_tacotron_step_oracle_cpu.py (not a test
module): the case table that reaches every dispatch class of the free-running Tacotron 2 decode step
(csrc/tacotron_infer.hip: ti_lstm_kernel twice, ti_scores_kernel, ti_context_kernel), the device run at the
capi level, a stage-wise float64 oracle and the comparison of the two.

Stage-wise: every stage of step t is recomputed in float64 from the DEVICE'S OWN inputs to that stage, read
back after the run, so the trajectory amplifies nothing and the bounds can be derived instead of tuned.
For every judged element the oracle gives the value R and a pre-rounding error bound E built from reference
quantities only:

  dot products   E = d 2^-24 sum_i |a_i| |b_i| (bf16 x bf16 is exact in fp32), d = the longest addition chain
                 of that kernel's summation tree, stated per stage next to D_* below. e4m3: one more fp32
                 rounding (the scale multiply).
  fast functions propagate E with the Lipschitz constant (sigmoid 1/4, tanh 1, relu 1), then add
                 DELTA = 2^-20 per tanh_fast / sigmoidf_ evaluation (8 fp32 ulps at 1; the kernel comment claims
                 ~1e-7). __expf in the softmax: 2^-20 relative plus |e - max e| 2^-23 for the argument scaling.
  hi / lo splits (alignments, location filter, cumulative alignments): the dropped lo x lo term and the
                 residuals of the splits are below 2^-16 relative per product.

fp32 outputs are judged |got - R| <= E, bf16 outputs bf16(R - E) <= got <= bf16(R + E). compare() logs the worst
err / E per stage (for a bf16 output err is the distance of the closest pre-rounding value, |got - R| minus
half a bf16 ulp of got); a ratio above 1 fails.

  python -m tests._tacotron_step_cases CASE      runs one case on cuda:0 and prints every figure."""
import functools
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
  sys.path.insert(0, REPO)

from oracle import attn_decoder as oad  # noqa: E402

U = 128                                # attention width of every case; L = 2 cell layers
U24, DELTA, SPLIT = 2.0 ** -24, 2.0 ** -20, 2.0 ** -16
SENT = -7.03125                        # exact in bf16 (0xC0E1) and fp32; no |h| < 1 and no probability equals it
PRENET_SEEDS = (9001, 9002)
DEFAULT = dict(B=3, S=12, H=64, M=64, P=64, nm=16, K=5, F=4, fp8=False, keep=0.5, T=2, mask_seq=False, zo=0.0)


def _c(**kw):
  d = dict(DEFAULT)
  d.update(kw)
  return d


STAGES = ("prenet", "cell0", "cell1", "q", "mh", "align", "ctx", "mel", "stop")
_CFG = dict(B=32, S=200, H=1024, M=1024, P=256, nm=80, K=32, F=32)
CASES = {
    "base": _c(T=3),
    "b17": _c(B=17, M=128, nm=8, K=1),                 # second 16-sample tile with 15 padding columns; 8 context parts
    "b32_parts4": _c(B=32, H=128, M=192, P=128, nm=24, K=32, F=32, S=40),   # B > 28: 4 parts of 3 tiles
    "b16": _c(B=16),                                   # NT = 1 at its limit
    "b29": _c(B=29, M=128),                            # B > 28 at M = 128: 4 context parts where b17 has 8
    "s1": _c(S=1), "s32": _c(S=32), "s33": _c(S=33), "s256": _c(S=256), "s257": _c(S=257), "s544": _c(S=544),
    "h512": _c(H=512), "h576": _c(H=576), "h1024": _c(H=1024),
    "p192_nm128": _c(P=192, nm=128), "p256_nm80": _c(P=256, nm=80), "keep1": _c(keep=1.0),
    # K = P + M + H classes of ti_geom()
    "k2048": _c(M=1920),                               # 32 chunks: 8x4, every slot live
    "k2112": _c(M=1984), "k2112_e4m3": _c(M=1984, fp8=True), "k2112_b20": _c(M=1984, B=20),   # 33: 9x4, 3 dead slots
    "k2112_b20_e4m3": _c(M=1984, B=20, fp8=True),
    "k2368": _c(M=2240), "k2368_e4m3": _c(M=2240, fp8=True),                                 # 37: 8x5, 3 dead slots
    "k2624": _c(M=2496), "k2624_e4m3": _c(M=2496, fp8=True),   # 41: 8x5, second round with one live chunk; 39 context tiles
    "config": _c(**_CFG), "config_e4m3": _c(fp8=True, **_CFG),
    "mask_seq_a": _c(T=6, mask_seq=True), "mask_seq_b": _c(T=6, mask_seq=True),
    # tests/test_zoneout_gpu.py holds the fused decode with zoneout to the step-wise path by whole-trajectory
    # norms only, so the blend of the fused cell is judged element-wise here
    "zoneout_blend": _c(zo=0.1),
}
TABLE = tuple(CASES)
# The forced-geometry runs use the k2112 shapes with their two steps: at step 0 the attention and state columns
# are the zero initial state, so every k-chunk but the first multiplies zeros and a chunk that is dropped or read
# twice could not show. Step 1 has every chunk live.
GEOM_SHAPES = ("k2112", "k2112_e4m3", "k2112_b20", "k2112_b20_e4m3")
# (option, value, case, stages judged): the shipped experiment switches of ti_launch_lstm_nt and of the context launch
FORCED = tuple(("tacotron_infer." + o, v, n, ("cell0", "cell1"))
               for o, v in (("rows", 32),) + tuple(("geom", g) for g in (804, 805, 904, 1103, 1203, 1602, 1603))
               for n in GEOM_SHAPES) + \
         tuple(("tacotron_infer.ctx_parts", v, "b32_parts4", STAGES) for v in (1, 2))
OPTION_DEFAULTS = {"tacotron_infer.rows": 16, "tacotron_infer.geom": 0, "tacotron_infer.ctx_parts": 0}
# attention vector scale, lowered until the largest alignment weight of the oracle trajectory is below 0.99
V_SCALE = {"s256": 0.3, "s257": 0.3, "s544": 0.4, "config": 0.3}   # (default 0.1; wider sources need a larger one to leave the uniform softmax)
SEED = {"mask_seq_a": 15, "mask_seq_b": 21}      # per-case seed (default: sum of the name's code points)
# mask-sequence cases: (scale of the stop projection, stop bias) chosen on the oracle trajectory so that the
# samples finish at different steps with every logit more than 2 away from zero (seeds and biases searched on the
# CPU) — a: lengths 3, 1, 2, decoding ends after step 3 of 6 and the rest is never run; b: lengths 1, 2 and a sample
# that never finishes
STOP = {"mask_seq_a": (40.0, -3.0), "mask_seq_b": (40.0, -45.75)}


def dims(name):
  c = CASES[name]
  return tuple(c[k] for k in ("B", "S", "H", "M", "P", "nm", "K", "F", "T"))


def spad(S):
  return (S + 31) // 32 * 32


def bf(x):
  """Round to bf16 (through fp32, as the device holds fp32 before a store), back in the dtype of x."""
  return x.float().to(torch.bfloat16).to(x.dtype)


def f32(x):
  return x.float().to(x.dtype)


def quantize_e4m3_cpu(w):
  """The dequantised matrix of capi.quantize_rows_e4m3 as tests/test_tacotron_infer_gpu.py::_oracle_params
  restates it (per-row scale absmax / 448); the device runs read the library's own bytes and scales back."""
  w = w.float()
  sc = w.abs().amax(dim=1, keepdim=True) / 448.0
  sc = torch.where(sc > 0, sc, torch.ones_like(sc))
  return ((w / sc).clamp(-448, 448).to(torch.float8_e4m3fn).float() * sc).double()


@functools.lru_cache(maxsize=None)
def build_inputs(name):
  """bf16-rounded parameters and inputs of a case from a seeded CPU generator, in the dtypes the device reads."""
  B, S, H, M, P, nm, K, F, T = dims(name)
  base = name.split("_e4m3")[0]           # an e4m3 case reads the tensors of its bf16 twin
  g = torch.Generator().manual_seed(SEED.get(base, sum(map(ord, base))))
  rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
  b16 = lambda t: t.to(torch.bfloat16)
  d = dict(name=name)
  k0 = P + M + H
  d["w0x"] = b16(rn(4 * H, k0, sc=1.4 / math.sqrt(k0)))          # [w_in | wcat0]
  d["wcat1"] = b16(rn(4 * H, 2 * H, sc=2.0 / math.sqrt(2 * H)))
  d["bias0"], d["bias1"] = rn(4 * H, sc=0.5), rn(4 * H, sc=0.5)
  d["wq"] = b16(rn(U, H, sc=1.0 / math.sqrt(H)))
  wmem = b16(rn(U, M, sc=1.0 / math.sqrt(M)))
  d["wmem"] = wmem
  d["v"] = rn(U, sc=V_SCALE.get(base, 0.1))
  d["b"] = rn(U, sc=0.1)
  d["conv_w"], d["conv_b"], d["dense_w"] = rn(K, F, sc=0.5), rn(F, sc=0.1), rn(F, U, sc=0.3)
  d["wp1"], d["bp1"] = b16(rn(P, nm, sc=1.0 / math.sqrt(nm))), rn(P, sc=0.3)
  d["wp2"], d["bp2"] = b16(rn(P, P, sc=1.0 / math.sqrt(P))), rn(P, sc=0.3)
  d["wout"] = b16(rn(nm, H + M, sc=2.0 / math.sqrt(H + M)))
  d["bout"] = rn(nm, sc=0.3)
  sscale, sbias = STOP.get(name, (1.0, 0.1))
  d["wstop"] = b16(rn(nm, sc=sscale / math.sqrt(nm)))
  d["bstop"] = torch.tensor([sbias])
  memory = b16(rn(B, S, M, sc=1.0))
  src_len = torch.randint(1, S + 1, (B,), generator=g, dtype=torch.int32)
  src_len[0] = S
  src_len[B - 1] = 1
  d["src_len"] = src_len
  values, _ = oad.prepare_memory(memory.float(), src_len)
  d["values"] = b16(values)
  d["keys"] = b16(d["values"].double() @ wmem.double().t())
  Sp, nm16 = spad(S), (nm + 15) // 16 * 16
  pv = d["values"].double() @ d["wout"].double()[:, H:].t()       # [B, S, nm] fp64, rounded once
  d["pv_t"] = torch.zeros(B, nm16, Sp, dtype=torch.bfloat16)
  d["pv_t"][:, :nm, :S] = b16(pv.transpose(1, 2))
  d["values_t"] = torch.zeros(B, M, Sp, dtype=torch.bfloat16)
  d["values_t"][:, :, :S] = d["values"].transpose(1, 2)
  assert int(src_len.min()) == 1 and int(src_len.max()) == S
  return d


def oracle_weights(name, deq=None):
  """float64 copies of what the kernels read. deq: (w0x, wcat1) dequantised from the device's own e4m3 bytes."""
  d = build_inputs(name)
  B, S, H, M, P, nm, K, F, T = dims(name)
  W = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}
  if CASES[name]["fp8"]:
    W["w0x"], W["wcat1"] = deq if deq is not None else (quantize_e4m3_cpu(d["w0x"]), quantize_e4m3_cpu(d["wcat1"]))
  W["pv"] = d["pv_t"][:, :nm, :S].double().transpose(1, 2)       # [B, S, nm]
  W["mask"] = (torch.arange(S)[None, :] < d["src_len"][:, None]).double()
  W["wck"] = W["conv_w"] @ W["dense_w"]                           # the folded location filter [K, U]
  W["wckb"] = W["conv_b"] @ W["dense_w"]
  # ad_fold_location: fp32 sums over the F filters (+ one rounding of the store)
  W["e_wck"] = (F + 1) * U24 * (W["conv_w"].abs() @ W["dense_w"].abs())
  W["e_wckb"] = (F + 1) * U24 * (W["conv_b"].abs() @ W["dense_w"].abs())
  return W


def prenet_masks(name, device):
  """Two [T + 1, B, P] float64 keep masks scaled by 1 / keep (None: dropout off). With a device: the library's
  counter-hash masks, the ones ti_tail applies (index (t B + b) P + j). Without: seeded Bernoulli stand-ins."""
  B, S, H, M, P, nm, K, F, T = dims(name)
  keep = CASES[name]["keep"]
  if keep >= 1.0:
    return None
  if device is None:
    g = torch.Generator().manual_seed(4321 + sum(map(ord, name)))
    return [(torch.rand(T + 1, B, P, generator=g) < keep).double() / keep for _ in range(2)]
  from openseq2seq_amd import capi
  return [capi.dropout_mask(sd, (T + 1) * B * P, keep, device).view(T + 1, B, P).double().cpu() / keep
          for sd in PRENET_SEEDS]


# ---- addition-chain depths, read off csrc/tacotron_infer.hip -------------------------------------------------
def lstm_geom(Kdim, forced=None):
  """(waves, chunk slots per wave) as ti_geom() / ti_launch_lstm_nt pick them; forced: ("rows", 32) or ("geom", g)."""
  if forced is not None and forced[0] == "rows":
    return 8, 5
  if forced is not None and forced[0] == "geom":
    g = int(forced[1])
    return (g // 100, g % 100) if g in (804, 904, 1203, 1103, 1603, 1602) else (8, 5)
  n = Kdim // 64
  return (8, 4) if n <= 32 else ((9, 4) if n <= 36 else (8, 5))


def d_lstm(Kdim, fp8, forced=None):
  """ti_lstm_kernel: 32 products inside one MFMA; a wave chains 2 MFMAs per live chunk slot, cpw slots per
  round of the `for (base ...)` loop; the epilogue adds the kTiWaves partial sums one after the other, then the
  bias (pre[g] = s * e_sc[g] + e_bias[g] + e_gx[g]; e_gx is an exact zero here). e4m3: s * e_sc rounds once."""
  nw, cpw = lstm_geom(Kdim, forced)
  rounds = -(-(Kdim // 64) // (nw * cpw))
  return 32 + 2 * cpw * rounds + nw + 1 + (1 if fp8 else 0)


D_P1 = 8 + 8 + 8 + 1     # ti_tail layer 1: ti_dot8 (4 dot2 of 2 products), <= kTiW1Pieces pieces added in turn, <= 8 (TPR) partials + bias
D_DOT = 16 + 6           # ti_frame_hpart / ti_scores_part q: two ti_dot8 chained (16 products) + wave_sum_dpp (6 levels)
D_STOP = 2 + 6 + 1       # ti_tail stop token: one dot2 per lane (n_mel / 2 <= 64 pairs), wave_sum_dpp, + bias
D_LOC = 32 + 3 + 5       # ti_scores_part: 3 chained MFMAs (hi.hi, lo.hi, hi.lo), + q + key, qb += bias + folded bias
D_E = 2 + 4 + 3          # v0 tanh + v1 tanh, row16_sum (4 levels), the kLocParts partial scores added in ti_alignments
D_SUM = 2 + 6 + 8 + 3    # softmax sum: <= 2 trips per thread, wave_sum_dpp, 8 wave sums; e - mx, * inv, 1 / sum


def d_p2(P):
  return 8 + P // 8 + 1  # ti_tail layer 2: ti_dot8, then P / 8 partials + bias added in turn


def d_wsum(S):
  return 32 + 2 * max(spad(S) // 32, 8)   # ti_weighted_sum: hi and lo MFMA per 32-position step, at least kTiKs steps


# ---- the stages in float64: (R, E) from the stage's inputs -----------------------------------------------------
def ref_prenet(W, name, frame, m0, m1, mut=None):
  """x_seq row from the previous frame [B, n_mel] (bf16 values). The layer-1 output is a bf16 value in LDS that
  cannot be read back: where R1 +- E1 straddles a bf16 boundary, the spread of the two roundings goes through
  |W2| into E. Returns dict(x=(R, E), edot=...)."""
  P, keep = CASES[name]["P"], CASES[name]["keep"]
  one = torch.ones(())
  m0 = one if m0 is None else m0
  m1 = one if m1 is None else m1
  w1, w2 = W["wp1"], W["wp2"]
  z1 = frame @ w1.t() + W["bp1"]
  e1 = D_P1 * U24 * (frame.abs() @ w1.abs().t() + W["bp1"].abs())
  x1 = torch.relu(z1) * m0
  e1s = e1 * m0 + U24 * x1.abs()                                   # s * ik
  x1b = bf(x1)
  spread = torch.maximum(bf(torch.relu(z1 + e1) * m0 + U24 * x1.abs()) - x1b, x1b - bf(torch.relu(z1 - e1) * m0 - U24 * x1.abs()))
  z2 = x1b @ w2.t() + W["bp2"]
  e2d = d_p2(P) * U24 * (x1b.abs() @ w2.abs().t() + W["bp2"].abs())
  e2 = e2d + spread @ w2.abs().t()
  x2 = torch.relu(z2) * m1
  return dict(x=(x2, e2 * m1 + U24 * x2.abs()), dots=[(z1, e1), (z2, e2d)], e1s=e1s)


def ref_cell(W, name, layer, xcat, c_prev, h_prev, forced=None, mut=None):
  """One LSTM cell from its input row [B, K] (bf16 values), the previous cell state (fp32 values) and, for
  the zoneout blend, the previous h (bf16 values). Gate order i, j, f, o; forget bias 1 inside the sigmoid."""
  fp8, zo = CASES[name]["fp8"], CASES[name]["zo"]
  w = W["w0x"] if layer == 0 else W["wcat1"]
  bias = W["bias0"] if layer == 0 else W["bias1"]
  H = w.shape[0] // 4
  xin = xcat
  if mut == "chunk" and layer == 0:                   # the last k-chunk never reaches the accumulators
    xin = xcat.clone()
    xin[:, -64:] = 0
  if mut == "column" and layer == 0 and xcat.shape[0] > 1:   # the last sample re-reads its neighbour's row
    xin = xcat.clone()
    xin[-1] = xin[-2]
  z = xin @ w.t() + bias
  if mut == "gates" and layer == 0:                   # gates f and g of unit 1 swapped
    z = z.clone()
    z[:, [H + 1, 2 * H + 1]] = z[:, [2 * H + 1, H + 1]]
  ez = d_lstm(w.shape[1], fp8, forced) * U24 * (xcat.abs() @ w.abs().t() + bias.abs())
  hv, cn = oad.lstm_cell(xin, c_prev, w, bias, 1.0)
  if mut == "gates" and layer == 0:
    zi, zg, zf, zo_ = z.chunk(4, -1)
    cn = c_prev * torch.sigmoid(zf + 1.0) + torch.sigmoid(zi) * torch.tanh(zg)
    hv = torch.tanh(cn) * torch.sigmoid(zo_)
  zi, zg, zf, zo_ = z.chunk(4, -1)
  ei, eg, ef, eo = ez.chunk(4, -1)
  ef = ef + U24 * (zf.abs() + 1.0)                    # pre[2] + forget_bias
  i, gg, f, o = torch.sigmoid(zi), torch.tanh(zg), torch.sigmoid(zf + 1.0), torch.sigmoid(zo_)
  Ei, Eg, Ef, Eo = ei / 4 + DELTA, eg + DELTA, ef / 4 + DELTA, eo / 4 + DELTA
  e_cn = c_prev.abs() * Ef + gg.abs() * Ei + i * Eg + Ei * Eg + 3 * U24 * ((c_prev * f).abs() + (i * gg).abs())
  tc = torch.tanh(cn)
  e_t = e_cn + DELTA
  e_h = o * e_t + tc.abs() * Eo + e_t * Eo + U24 * hv.abs()
  c_st, e_c, h_st, e_hs = cn, e_cn, hv, e_h
  if zo > 0:                                           # zoneout_state mode 2: p old + (1 - p) new in fp32
    p = float(torch.tensor(zo, dtype=torch.float32))
    q = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(zo, dtype=torch.float32))
    c_st = p * c_prev + q * cn
    e_c = q * e_cn + 3 * U24 * ((p * c_prev).abs() + (q * cn).abs())
    h_st = p * h_prev + q * hv
    e_hs = q * e_h + 3 * U24 * ((p * h_prev).abs() + (q * hv).abs())
  return dict(c=(c_st, e_c), h_state=(h_st, e_hs), h_out=(hv, e_h), dots=[(z, ez)], z=z)


def ref_scores(W, name, y, cum, mut=None):
  """Query projection, location-sensitive scores and softmax from the cell output [B, H] (bf16 values) and
  the cumulative alignments [B, S] (fp32 values): q [B, U], mh [B, n_mel], align [B, S]."""
  B, S, H, M, P, nm, K, F, T = dims(name)
  wq, woh = W["wq"], W["wout"][:, :H]
  q = y @ wq.t()
  e_q = D_DOT * U24 * (y.abs() @ wq.abs().t())
  mh = y @ woh.t()
  e_mh = D_DOT * U24 * (y.abs() @ woh.abs().t())
  cin = cum
  if mut == "tap":                                    # every tap reads one position to the right
    cin = torch.cat([cum[:, 1:], torch.zeros_like(cum[:, :1])], 1)
  loc = oad.location_features(cin, W["conv_w"], W["conv_b"], W["dense_w"])          # [B, S, U]
  pl = (K - 1) // 2
  win = torch.nn.functional.pad(cum.abs(), (pl, K - 1 - pl)).unfold(1, K, 1)      # [B, S, K]
  a_loc = win @ W["wck"].abs()
  e_loc = (D_LOC * U24 + SPLIT) * a_loc + win @ W["e_wck"] + W["e_wckb"]
  keys = W["keys"]
  x = keys + q[:, None, :] + loc + W["b"]
  e_x = e_q[:, None, :] + e_loc + D_LOC * U24 * (keys.abs() + q.abs()[:, None, :] + W["wckb"].abs() + W["b"].abs())
  v = W["v"]
  th = torch.tanh(x)
  e = (v * th).sum(-1)
  e_e = (v.abs() * (e_x + DELTA)).sum(-1) + D_E * U24 * (v * th).abs().sum(-1)
  mask = W["mask"]
  a = oad.masked_softmax(e, mask)
  em = e.masked_fill(mask == 0, float("-inf"))
  gap = torch.where(mask > 0, (em - em.max(-1, keepdim=True).values).abs(), torch.zeros_like(e))
  lin = (e_e + DELTA + gap * (2.0 ** -23 + U24)) * mask
  rel = lin + (a * lin).sum(-1, keepdim=True) + (lin + lin.max(-1, keepdim=True).values) ** 2
  e_a = a * (rel + D_SUM * U24)
  return dict(q=(q, e_q), mh=(mh, e_mh), align=(a, e_a), dots=[(q, e_q), (mh, e_mh)], e=e)


def ref_context(W, name, al):
  """Context [B, M] from the alignment row [B, S] (fp32 values) and the values."""
  S = CASES[name]["S"]
  vals = W["values"]
  r = (al[:, :, None] * vals).sum(1)
  a = (al.abs()[:, :, None] * vals.abs()).sum(1)
  e = (d_wsum(S) * U24 + SPLIT) * a
  return dict(ctx=(r, e), dots=[(r, e)])


def ref_frame(W, name, y, al, pv=None, mut=None):
  """Frame [B, n_mel] = W_out[:, :H] y + sum_s a[s] PV[s] + b, PV the bf16 table the kernel reads (pv_t)."""
  B, S, H, M, P, nm, K, F, T = dims(name)
  pv = W["pv"] if pv is None else pv
  woh = W["wout"][:, :H]
  mh = y @ woh.t()
  e_mh = D_DOT * U24 * (y.abs() @ woh.abs().t())
  mc = (al[:, :, None] * pv).sum(1)
  e_mc = (d_wsum(S) * U24 + SPLIT) * (al.abs()[:, :, None] * pv.abs()).sum(1)
  bo = W["bout"]
  if mut == "bias":
    bo = bo.clone()
    bo[-1] = 0
  r = mh + bo + mc
  return dict(mel=(r, e_mh + e_mc + 2 * U24 * (mh.abs() + W["bout"].abs() + mc.abs())), dots=[(mc, e_mc)])


def ref_stop(W, name, mel):
  """Stop logit [B] from the stored frame (bf16 values); the stop projection's output is a bf16 tensor."""
  ws = W["wstop"]
  r = mel @ ws + W["bstop"]
  e = D_STOP * U24 * (mel.abs() @ ws.abs() + W["bstop"].abs())
  return dict(stop=(r, e), dots=[(r, e)])


def stop_rule(stop, mask_seq):
  """The reference's bookkeeping (dynamic_decode + TacotronHelper) on a [B, T'] logit trajectory:
  (steps run, finished [B], lengths [B], state[1])."""
  B, T = stop.shape
  fin = torch.zeros(B, dtype=torch.bool)
  ln = torch.zeros(B, dtype=torch.int32)
  for t in range(T):
    ln += (~fin).to(torch.int32)
    if mask_seq:
      fin |= stop[:, t] > 0
    if bool(fin.all()):
      return t + 1, fin, ln, t + 1
  return T, fin, ln, 0


# ---- the oracle chained over T steps: the CPU trajectory and the fabricated "device" result -----------------------
def chain(name, exact=False, mut=None, device=None, deq=None):
  """The stage oracle chained from zero state. exact=False: every value rounded as the device stores it (bf16
  / fp32), returned in the layout and dtypes of run_gpu() — a fabricated device result, with `mut` one of the
  kernel mistakes of MUTATIONS built in. exact=True: float64 throughout apart from the bf16 stores, with keys
  and PV unrounded (what oracle.tacotron.decoder_infer computes). Also returns the input-condition figures."""
  B, S, H, M, P, nm, K, F, T = dims(name)
  c = CASES[name]
  W = oracle_weights(name, deq)
  pv = None
  if exact:
    W = dict(W)
    W["keys"] = W["values"] @ W["wmem"].t()
    pv = W["values"] @ W["wout"][:, H:].t()
  r32 = (lambda x: x) if exact else f32
  masks = prenet_masks(name, device)
  mk = lambda i, t: None if masks is None else masks[i][min(t, T)]
  z = lambda *s: torch.zeros(*s, dtype=torch.float64)
  G = dict(x_seq=z(B, T + 1, P), mel=z(B, T, nm), stop=z(B, T), y_top=z(B, T, H), ctx=z(B, T, M), align=z(B, T, S),
           q_seq=z(B, T, U), cat0=z(B, T + 1, M + H), cat1=z(B, T + 1, 2 * H), c0=z(B, T, H), c1=z(B, T, H),
           cum=z(B, T + 1, S), mh=z(B, nm))
  filled = ("x_seq", "mel", "stop", "y_top", "ctx", "align", "q_seq", "c0", "c1")
  for k in filled:
    G[k] += SENT
  for k in ("cat0", "cat1", "cum"):
    G[k][:, 1:] = SENT
  for k in ("c0", "c1"):
    G[k][:, 0] = 0
  cond = dict(dots={}, gates=[[], []], amax=0.0)

  def note(stage, dots):
    for r, e in dots:
      cond["dots"].setdefault(stage, []).append((float(e.max()), float(r.pow(2).mean().sqrt())))

  frame = z(B, nm)
  n_run = T
  for t in range(T + 1):
    tm = t + 1 if mut == "mask" else t
    pr = ref_prenet(W, name, frame, mk(0, tm), mk(1, tm))
    note("prenet", pr["dots"])
    G["x_seq"][:, t] = bf(pr["x"][0])
    if t == T or t == n_run:
      break
    zero = z(B, H)
    c0 = ref_cell(W, name, 0, torch.cat([G["x_seq"][:, t], G["cat0"][:, t]], 1), G["c0"][:, t - 1] if t else zero,
                  G["cat0"][:, t, M:], mut=mut)
    note("cell0", c0["dots"])
    cond["gates"][0].append(c0["z"])
    G["c0"][:, t] = r32(c0["c"][0])
    G["cat0"][:, t + 1, M:] = bf(c0["h_state"][0])
    G["cat1"][:, t, :H] = bf(c0["h_out"][0])
    c1 = ref_cell(W, name, 1, G["cat1"][:, t], G["c1"][:, t - 1] if t else zero, G["cat1"][:, t, H:], mut=mut)
    note("cell1", c1["dots"])
    cond["gates"][1].append(c1["z"])
    G["c1"][:, t] = r32(c1["c"][0])
    G["cat1"][:, t + 1, H:] = bf(c1["h_state"][0])
    G["y_top"][:, t] = bf(c1["h_out"][0])
    sc = ref_scores(W, name, G["y_top"][:, t], G["cum"][:, t], mut=mut)
    note("q", sc["dots"])
    G["q_seq"][:, t] = r32(sc["q"][0])
    G["mh"] = r32(sc["mh"][0])
    al = r32(sc["align"][0])
    G["align"][:, t] = al
    G["cum"][:, t + 1] = r32(G["cum"][:, t] + al)
    many = build_inputs(name)["src_len"] > 1
    if bool(many.any()):
      cond["amax"] = max(cond["amax"], float(al[many].max()))
    cx = ref_context(W, name, al)
    note("ctx", cx["dots"])
    cb = bf(cx["ctx"][0])
    if mut == "ctxcol":
      cb[:, M - 1] = cb[:, M - 2]
    G["ctx"][:, t] = cb
    G["cat0"][:, t + 1, :M] = cb
    fr = ref_frame(W, name, G["y_top"][:, t], sc["align"][0] if exact else al, pv=pv, mut=mut)
    note("mel", fr["dots"])
    frame = bf(fr["mel"][0])
    G["mel"][:, t] = frame
    st = ref_stop(W, name, frame)
    note("stop", st["dots"])
    G["stop"][:, t] = bf(st["stop"][0])
    n_run = stop_rule(G["stop"][:, :t + 1], c["mask_seq"])[3] or T
    if mut == "past" and t == 0 and S > 1:
      G["align"][B - 1, 0, S - 1] = 1e-3               # the last sample has one source position
  steps, fin, ln, s1 = stop_rule(G["stop"][:, :n_run], c["mask_seq"])
  G["state"] = torch.cat([torch.tensor([0, s1, int(fin.sum()), 0], dtype=torch.int32), fin.to(torch.int32), ln])
  if not exact:
    for k in ("x_seq", "mel", "y_top", "ctx", "cat0", "cat1"):
      G[k] = G[k].to(torch.bfloat16)
    for k in ("stop", "align", "q_seq", "c0", "c1", "cum", "mh"):
      G[k] = G[k].float()
  G["cond"] = cond
  G["n_run"] = n_run
  return G


MUTATIONS = ("chunk", "gates", "column", "tap", "ctxcol", "bias", "mask", "past")


def check_inputs(name):
  """Conditions on the oracle trajectory without which a pass proves nothing; returns the violations."""
  B, S, H, M, P, nm, K, F, T = dims(name)
  G = chain(name)
  cond = G["cond"]
  bad = []
  for stage, figs in cond["dots"].items():
    for e, rms in figs:
      if rms > 0 and not e <= 2.0 ** -10 * rms:
        bad.append("%s: %s: dot allowance E %.3e above 2^-10 rms(R) = %.3e" % (name, stage, e, 2.0 ** -10 * rms))
  for l in range(2):
    rms = float(torch.cat(cond["gates"][l]).pow(2).mean().sqrt())
    if not 0.3 <= rms <= 3.0:
      bad.append("%s: gate pre-activations of layer %d have rms %.3f outside [0.3, 3]" % (name, l, rms))
  if S > 1 and not cond["amax"] < 0.99:
    bad.append("%s: largest alignment weight %.4f >= 0.99" % (name, cond["amax"]))
  sl = build_inputs(name)["src_len"].tolist()
  if 1 not in sl or S not in sl:
    bad.append("%s: src_len holds no 1 or no S" % name)
  if CASES[name]["mask_seq"]:
    st = G["stop"][:, :G["n_run"]].double()
    ulp = 2.0 ** (torch.floor(torch.log2(st.abs().clamp_min(1e-30))) - 7)
    if not bool((st.abs() >= 4 * ulp).all()) or float(st.abs().min()) == 0.0:
      bad.append("%s: a stop logit within 4 bf16 ulps of zero" % name)
    if len(set(G["state"][4 + B:].tolist())) < 2:
      bad.append("%s: the samples do not finish at different steps: %s" % (name, G["state"][4 + B:].tolist()))
  return bad


# ---- the device run ----------------------------------------------------------------------------------------------
def run_gpu(name, device, split=False):
  """One decode of T steps through capi.AttnDecoder + capi.TacotronInfer, every buffer the kernels write filled
  with SENT first; CPU copies of everything compared. split: steps(0, 1) then steps(1, T)."""
  from openseq2seq_amd import capi
  B, S, H, M, P, nm, K, F, T = dims(name)
  c = CASES[name]
  d = build_inputs(name)
  dv = lambda k: d[k].to(device)
  both = torch.full((B, T, H + M), SENT, dtype=torch.bfloat16, device=device)
  zo = dict(zoneout_prob=c["zo"], zoneout_mode=capi.ZONEOUT_BLEND) if c["zo"] > 0 else {}
  loop = capi.AttnDecoder(B, T, S, 2, H, M, U, 2, device, use_bias=True, loc_k=K, loc_f=F, forget_bias=1.0,
                          save=False, y_top=both[:, :, :H], ctx=both[:, :, H:], **zo)
  w0x = dv("w0x")
  wcat0, wcat1 = w0x[:, P:].contiguous(), dv("wcat1")
  loop.set_params([wcat0, wcat1], dv("wq"), dv("v"), bias=[None, dv("bias1")], b=dv("b"), conv_w=dv("conv_w"),
                  conv_b=dv("conv_b"), dense_w=dv("dense_w"))
  deq = None
  w = {"w0x": w0x, "w0x8": None}
  if c["fp8"]:
    q0, q1, q0x = capi.quantize_rows_e4m3(wcat0), capi.quantize_rows_e4m3(wcat1), capi.quantize_rows_e4m3(w0x)
    loop.set_fp8_weights([q0, q1])
    w["w0x8"] = q0x
    de = lambda q: q[0].cpu().view(torch.float8_e4m3fn).double() * q[1].cpu().double()[:, None]
    deq = (de(q0x), de(q1))
  for k in ("bias0", "wp1", "bp1", "wp2", "bp2", "bout", "wstop", "bstop", "pv_t", "values_t"):
    w[k] = dv(k)
  w["wout_h"] = d["wout"][:, :H].contiguous().to(device)
  loop.set_inputs(torch.zeros(8, dtype=torch.bfloat16, device=device), dv("keys"), dv("values"), dv("src_len"), None)
  fused = capi.TacotronInfer(loop, P, nm, w, c["mask_seq"], c["keep"], PRENET_SEEDS)
  assert fused.supported(), "%s: os2s_tacotron_infer_supported refuses the case" % name
  for t in (fused.x_seq, fused.mel, fused.stop, fused.mh, loop.align_seq, loop.q_seq):
    t.fill_(SENT)
  for t in loop.cat + loop.c_seq + [loop.cum_seq]:
    t[:, 1:] = SENT
  if split:
    fused.steps(0, 1)
    fused.steps(1, T)
  else:
    fused.steps(0, T)
  torch.cuda.synchronize()
  cp = lambda t: t.cpu().clone()
  got = dict(x_seq=cp(fused.x_seq), mel=cp(fused.mel), stop=cp(fused.stop), mh=cp(fused.mh), state=cp(fused.state),
             y_top=cp(loop.y_top).contiguous(), ctx=cp(loop.ctx).contiguous(), align=cp(loop.align_seq),
             q_seq=cp(loop.q_seq), cat0=cp(loop.cat[0]), cat1=cp(loop.cat[1]), c0=cp(loop.c_seq[0]),
             c1=cp(loop.c_seq[1]), cum=cp(loop.cum_seq), deq=deq)
  return got


BITS = ("x_seq", "mel", "stop", "mh", "state", "y_top", "ctx", "align", "q_seq", "cat0", "cat1", "c0", "c1", "cum")


def _bits(t):
  return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def same_bits(a, b):
  return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def compare_runs(name, a, b, what, log=print):
  fails = []
  for k in BITS:
    ok = same_bits(a[k], b[k])
    log("  %-4s %s: %s" % ("ok" if ok else "FAIL", what, k))
    if not ok:
      fails.append("%s: %s: %s differs" % (name, what, k))
  return fails


def _ulp_bf16(x):
  return 2.0 ** (torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def compare(name, got, log=print, device=None, forced=None, stages=STAGES, ratios=None):
  """Every assertion on one device (or fabricated) result; returns the failures and logs every figure judged.
  device: where the pre-net masks come from (None: the stand-in masks of the CPU checks). forced: the
  tacotron_infer.rows / geom setting the run was made under. stages: the stages judged. ratios: dict that
  receives the worst err / E per stage."""
  B, S, H, M, P, nm, K, F, T = dims(name)
  c = CASES[name]
  d = build_inputs(name)
  W = oracle_weights(name, got.get("deq"))
  masks = prenet_masks(name, device)
  mk = lambda i, t: None if masks is None else masks[i][t]
  fails = []
  worst = {}

  def check(ok, what, *figs):
    log("  %-4s %s %s" % ("ok" if ok else "FAIL", what, " ".join("%.3e" % f for f in figs)))
    if not ok:
      fails.append("%s: %s %s" % (name, what, " ".join("%.3e" % f for f in figs)))

  def judge(stage, what, g, RE, t):
    """g: the device tensor (bf16 or fp32). fp32: |g - R| <= E. bf16: bf16(R - E) <= g <= bf16(R + E)."""
    R, E = RE
    gd = g.double()
    if g.dtype == torch.bfloat16:
      ok = bool(((gd >= bf(R - E)) & (gd <= bf(R + E))).all())
      err = ((gd - R).abs() - 0.5 * _ulp_bf16(gd)).clamp_min(0)
    else:
      ok = bool(((gd - R).abs() <= E).all())
      err = (gd - R).abs()
    ratio = float((err / E.clamp_min(1e-300)).max()) if err.numel() else 0.0
    worst[stage] = max(worst.get(stage, 0.0), ratio)
    check(ok, "t=%d %s: max|got - R|, max E, worst err/E" % (t, what), float((gd - R).abs().max()), float(E.max()), ratio)

  st = got["state"]
  n_run = int(st[1]) if int(st[1]) else T
  # ---- sentinel: rows of steps that were run hold no sentinel, the others keep it bit for bit ---------------------
  sent = lambda t: (t.double() == SENT)
  for k, rows_run in (("x_seq", n_run + 1), ("mel", n_run), ("stop", n_run), ("y_top", n_run), ("ctx", n_run),
                      ("align", n_run), ("q_seq", n_run), ("c0", n_run), ("c1", n_run), ("cat0", n_run + 1),
                      ("cum", n_run + 1)):
    t = got[k]
    lo = 1 if k in ("cat0", "cum") else 0           # row 0: the zero initial state, never written
    check(not bool(sent(t[:, lo:rows_run]).any()), "%s: no sentinel left in rows of run steps" % k)
    check(bool(sent(t[:, rows_run:]).all()), "%s: rows of steps not run keep the sentinel" % k)
  c1t = got["cat1"]
  check(not bool(sent(c1t[:, :n_run, :H]).any()) and not bool(sent(c1t[:, 1:n_run + 1, H:]).any()),
        "cat1: no sentinel left in rows of run steps")
  check(bool(sent(c1t[:, n_run:, :H]).all()) and bool(sent(c1t[:, n_run + 1:, H:]).all()),
        "cat1: rows of steps not run keep the sentinel")
  check(float(got["cat0"][:, 0].abs().max()) == 0.0 and float(c1t[:, 0, H:].abs().max()) == 0.0
        and float(got["cum"][:, 0].abs().max()) == 0.0, "initial rows still zero")
  if "mh" in stages:
    check(not bool(sent(got["mh"]).any()), "mh: no sentinel left")
  # ---- exact -------------------------------------------------------------------------------------------------------
  al = got["align"][:, :n_run].double()
  past = (W["mask"] == 0)[:, None, :].expand(B, n_run, S)
  check(float(al[past].abs().sum()) == 0.0 if bool(past.any()) else True, "align past src_len zero")
  rows = float((al.sum(-1) - 1.0).abs().max())
  check(rows <= 1e-6, "live alignment rows sum to 1 within 1e-6", rows)
  cum = got["cum"]
  step = float((cum[:, 1:n_run + 1] - (cum[:, :n_run] + got["align"][:, :n_run])).abs().max())
  check(step <= 1e-6, "cum[t+1] = cum[t] + align[t]", step)
  if c["zo"] == 0:
    check(same_bits(got["cat0"][:, 1:n_run + 1, M:], c1t[:, :n_run, :H]), "both copies of h0 bit-equal")
    check(same_bits(got["y_top"][:, :n_run], c1t[:, 1:n_run + 1, H:]), "both copies of h1 bit-equal")
  check(same_bits(got["ctx"][:, :n_run], got["cat0"][:, 1:n_run + 1, :M]), "both copies of the context bit-equal")
  steps, fin, ln, s1 = stop_rule(got["stop"][:, :n_run].double(), c["mask_seq"])
  check(steps == n_run and int(st[1]) == s1, "state[1] follows the rule on the device's stop logits", float(st[1]), float(s1))
  check(torch.equal(st[4:4 + B], fin.to(torch.int32)) and int(st[2]) == int(fin.sum()), "finished flags follow the rule")
  check(torch.equal(st[4 + B:4 + 2 * B], ln), "lengths follow the rule")
  # ---- stage by stage against the oracle -----------------------------------------------------------------------------
  D = {k: (v.double() if torch.is_tensor(v) else v) for k, v in got.items()}
  zero = torch.zeros(B, H, dtype=torch.float64)
  for t in range(n_run + 1):
    if "prenet" in stages and t <= T:
      frame = D["mel"][:, t - 1] if t else torch.zeros(B, nm, dtype=torch.float64)
      pr = ref_prenet(W, name, frame, mk(0, t), mk(1, t))
      judge("prenet", "pre-net x_seq", got["x_seq"][:, t], pr["x"], t)
    if t == n_run:
      break
    if "cell0" in stages:
      r = ref_cell(W, name, 0, torch.cat([D["x_seq"][:, t], D["cat0"][:, t]], 1), D["c0"][:, t - 1] if t else zero,
                   D["cat0"][:, t, M:], forced=forced)
      judge("cell0", "cell 0 c", got["c0"][:, t], r["c"], t)
      judge("cell0", "cell 0 h (state)", got["cat0"][:, t + 1, M:], r["h_state"], t)
      judge("cell0", "cell 0 h (output)", got["cat1"][:, t, :H], r["h_out"], t)
    if "cell1" in stages:
      r = ref_cell(W, name, 1, D["cat1"][:, t], D["c1"][:, t - 1] if t else zero, D["cat1"][:, t, H:], forced=forced)
      judge("cell1", "cell 1 c", got["c1"][:, t], r["c"], t)
      judge("cell1", "cell 1 h (state)", got["cat1"][:, t + 1, H:], r["h_state"], t)
      judge("cell1", "cell 1 h (output)", got["y_top"][:, t], r["h_out"], t)
    if "q" in stages or "align" in stages or "mh" in stages:
      r = ref_scores(W, name, D["y_top"][:, t], D["cum"][:, t])
      if "q" in stages:
        judge("q", "query projection q_seq", got["q_seq"][:, t], r["q"], t)
      if "mh" in stages and t == n_run - 1:
        judge("mh", "W_out[:, :H] h1 (mh, last step)", got["mh"], r["mh"], t)
      if "align" in stages:
        judge("align", "alignments", got["align"][:, t], r["align"], t)
    if "ctx" in stages:
      judge("ctx", "context", got["ctx"][:, t], ref_context(W, name, D["align"][:, t])["ctx"], t)
    if "mel" in stages:
      judge("mel", "frame", got["mel"][:, t], ref_frame(W, name, D["y_top"][:, t], D["align"][:, t])["mel"], t)
    if "stop" in stages:
      R, E = ref_stop(W, name, D["mel"][:, t])["stop"]
      judge("stop", "stop logit", got["stop"][:, t].to(torch.bfloat16), (R, E), t)
      check(same_bits(got["stop"][:, t], got["stop"][:, t].to(torch.bfloat16).float()), "t=%d stop logit is a bf16 value" % t)
  log("  worst err/E per stage: " + " ".join("%s %.3f" % (k, worst[k]) for k in STAGES if k in worst))
  if ratios is not None:
    for k, v in worst.items():
      ratios[k] = max(ratios.get(k, 0.0), v)
  return fails


def check_case(name, device, log=print, ratios=None):
  """The full run of one case: device result against the oracle, a second run and a split run bit for bit."""
  got = run_gpu(name, device)
  fails = compare(name, got, log=log, device=device, ratios=ratios)
  fails += compare_runs(name, got, run_gpu(name, device), "second run bit-identical", log=log)
  fails += compare_runs(name, got, run_gpu(name, device, split=True), "steps(0,1) + steps(1,T) = steps(0,T)", log=log)
  return fails


def check_forced(option, value, name, stages, device, log=print, ratios=None):
  """One run under a forced launch geometry, judged against the oracle with that geometry's summation depth; the
  option is restored whatever happens."""
  from openseq2seq_amd import _lib
  old = _lib.get_option(option)
  try:
    _lib.set_option(option, value)
    got = run_gpu(name, device)
  finally:
    _lib.set_option(option, old)
  forced = (option.split(".")[1], value) if option != "tacotron_infer.ctx_parts" else None
  return compare(name, got, log=log, device=device, forced=forced, stages=stages, ratios=ratios)


def main(argv):
  if len(argv) != 2 or argv[1] not in CASES:
    print("usage: python -m tests._tacotron_step_cases {%s}" % ",".join(sorted(CASES)))
    return 2
  import __graft_entry__ as entry
  from openseq2seq_amd import _lib
  if not os.path.exists(_lib.LIB_PATH):
    entry.build()
  assert torch.cuda.is_available(), "needs a GPU"
  fails = check_case(argv[1], torch.device("cuda:0"))
  for f in fails:
    print("MISMATCH", f)
  return 1 if fails else 0


if __name__ == "__main__":
  sys.exit(main(sys.argv))
