"""Helper of tests/test_bn_kernels_gpu.py and tests/test_bn_oracle_cpu.py (not a test module): the case
table that reaches every kernel, instantiation and tiling class of csrc/batchnorm.hip, a float64 oracle per
STAGE, the rounding bounds and compare().

Teacher forcing. Every kernel is checked alone: its inputs are bf16 / fp32 tensors made on the host or the
outputs the backend itself gave for the previous stage, and the oracle evaluates the same formula in float64
on exactly those tensors. No bound absorbs an upstream kernel's rounding; each follows from
    u32 = 2^-24   unit roundoff of fp32
    ubf = 2^-8    unit roundoff of bf16 round-to-nearest-even
    a sum of n fp32 terms in any order, fused or not, errs by at most (n - 1) u32 sum|terms|
(the derivations stand next to the code of each stage below; none was tuned on a device).

A backend (the device in test_bn_kernels_gpu.py, the fp32 torch emulations in test_bn_oracle_cpu.py) gives
    stats(y2d) -> partial [ceil(rows / 128), 2, C]
    finalize(partial, count, gamma, beta, eps, momentum, training, moving_mean, moving_var, want_stats)
        -> dict(mean, rstd, scale, shift, moving_mean, moving_var)      and finalize_multi(list of those)
    dropout_mask(seed, shape, keep) -> bool
    act_fwd(ys, scales, shifts, lens, act, keep, seed) -> out
    reduce(dout, out, ys, means, rstds, lens, act, keep, seed, n) -> dz, partial [ceil(rows / n), 1 + J, C]
    bwd_finalize(partial, q, count, pre_dgamma, pre_dbeta, accumulate, mean, rstd) -> dict(dgamma, dbeta, c1, c2)
        (mean / rstd given: the raw entry point)                        and bwd_finalize_multi(...)
    apply(dz, y, gamma, mean, rstd, c1, c2, lens, margin, dz_to_len) -> dy
all on CPU tensors. check_case() walks one case through the six stages, check_finalize_handmade() feeds the
two finalize stages hand-made partials at the part counts where their loops change shape.

Rows that must not be read (y at t >= len for the forward; dout, out, y at t >= len for the reduce; dz at
t >= len under dz_to_len; dz, y at t >= len + margin for the apply) hold `poison` (NaN on the device) in
every run that has a length vector, and a rerun on the clean tensors must give the same bits.

Classes reached (kernel, instantiation, tiling, entry point):
  bn_stats            G = 1 / 3 (idle threads) / 5 / 8 / 33 / 48 / 256 with grid.y = 2 (one live group); one
                      row lane of 256 down to one row per lane; a row tail, a whole tile, a single-row tensor
                      (check_finalize_handmade, nparts = 1); 4x-unrolled loop (C = 8, 24: RL >= 85 never enters it; C = 264, 384 do)
  bn_finalize         single and multi (J = 1, 11, 16); nparts 1 .. 263: tail only, the 4x loop alone, both;
                      training / eval, gamma / beta null, mean_out / rstd_out null, moving_* null, count = 1,
                      the variance clamp; C = 40 (partial block), 64, 200 (3 full + 8), every case's own C
  bn_act_fwd          <true> (J = 1) and <false> (J = 2 .. 12); all four activations; keep = 1 and < 1;
                      out_len null, all T, ragged with 0; G = 1, 3, 5, 8, 24, 32, 33; cursor multi-wrap (RL > T)
  bn_act_bwd_reduce   <1,4> (J = 1), <4,2> (J = 2, 3, 4), <12,1> (J = 5, 12); rows per workgroup 8 .. 1024 with
                      1- and 2-row tile tails; os2s_bn_act_bwd_num_parts under every tiling
  bn_bwd_finalize     single, multi, raw; accumulate 0 / 1; dgamma / dbeta null; nparts as above (second trip of
                      fin_sum_pair at 129, 263 and with the device's own 132 partials)
  bn_bwd_apply        dense, ragged (margin 0, 5, 1000 > T), ragged_dz; gamma null; the same tilings
Not reached: the non-default tilings at more than 33 channel groups (c2056 runs the defaults only: 9 channel
blocks); tensors of 2^31 bytes and more (block_rsrc's 32-bit offsets are per workgroup, so no size changes
their class; the row index is 64-bit); B * T = 0 (the entry points return before a launch); the conv epilogues
that emit partials (tests/test_conv1d_gpu.py) and token_bn_* (transformer_norm.hip).

Measured on the MI355X, largest error / bound over all cases, tilings and hand-made part counts (the GPU test
prints them as BN-RATIO lines; 0: bit-identical to the rounded oracle):
  stats         sum 7.3e-3   sumsq 5.4e-2
  finalize      mean 0   moving_mean 0.59   moving_var 0.61   rstd 0.27   scale 0.46   shift 0.70
                variance under cancellation 2.5e-6
  act_fwd       out 0.995 (a bf16 tie: ubf |ref| is the rounding's own worst case); +0 rows and elements exact
  reduce        dz exact for none / relu / relu20, 0.97 for tanh; partial[0] 7.8e-3; partial[1+j] 0.19
  bwd_finalize  dgamma, dbeta, c1, c2 0.5 (half an ulp: correctly rounded)
  bwd_apply     dy 0.996; +0 rows exact
No bound of the issue had to be widened. Two were completed where the stated form cannot hold: with
accumulate = 1 dgamma / dbeta round twice (the fp32 sum, then the fp32 addition), so their bound is 1 ulp of the
result + 1 ulp of the sum; the raw finalize's fp64 slack is carried through rstd (x - mean sd). The first run
found bn_act_bwd_reduce storing -0 in dz for a negative dout wherever no gradient passes (dout * 0): the kernel
now selects +0 there, as the rows past the length already were."""
import math
import os
import re
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
  sys.path.insert(0, REPO)

U32 = 2.0 ** -24
UBF = 2.0 ** -8
ACT_ID = {"none": 0, "relu": 1, "tanh": 2, "relu20": 3}
EPS, MOM, SEED = 1e-3, 0.9, 1234567
STATS_ROWS = 128          # kStatsRowsPerBlock
RELU_CAP = 20.0           # kReluCap
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

# bn.<kernel>.groups / .rows of the three tiled kernels, their defaults (g_tiling) and the tilings of the sweep
KERNELS = ("act_fwd", "act_bwd_reduce", "bwd_apply")
DEFAULT_TILING = ((32, 32), (32, 64), (32, 64))
TILINGS = ((8, 8), (24, 40), (256, 1024), (32, 1024))
TILED_CASES = ("c8", "c264", "rows1050")

CASES = {
    # C8 = 1: G = 1, RL = 256, every thread a row lane
    "c8": dict(B=3, T=50, C=8, J=1, act="relu", keep=1.0, lens=[50, 31, 17]),
    # G = 3, RL = 85: thread 255 idles; T < RL; lengths contain 0 and T; reduce <4,2> with J = 2
    "c24": dict(B=11, T=7, C=24, J=2, act="none", keep=0.8, lens=[7, 0, 3, 7, 1, 0, 5, 2, 7, 4, 6]),
    # top of reduce <4,2>; finalize block with 40 of 64 channels; input 1 has mean 8, std 0.25 (cancellation)
    "c40": dict(B=2, T=77, C=40, J=4, act="tanh", keep=0.9, lens=[77, 50], cancel=1),
    # bottom of reduce <12,1> (3 of the 4 loads of its second group out of range); C8 = 33: last channel block
    # with one live group; 130 rows: a 2-row tile tail for the forward and the backward
    "c264": dict(B=2, T=65, C=264, J=5, act="relu", keep=0.7, lens=[65, 41]),
    # kMaxBnInputs; 129 rows: a 1-row tile tail everywhere (stats included)
    "c384": dict(B=1, T=129, C=384, J=12, act="relu20", keep=0.8, lens=[100]),
    # bn_stats grid.y = 2 with one live group (C8 = 257)
    "c2056": dict(B=2, T=33, C=2056, J=1, act="relu20", keep=1.0, lens=[33, 20]),
    # rows a whole number of tiles, all lengths = T / no length vector
    "c64_lens_T": dict(B=4, T=64, C=64, J=3, act="relu", keep=1.0, lens=[64, 64, 64, 64]),
    "c64_no_lens": dict(B=4, T=64, C=64, J=3, act="relu", keep=1.0, lens=None),
    # 1,050 rows: 132 partials at bn.act_bwd_reduce.rows = 8 (second trip of fin_sum_pair), several utterances
    # per cursor step at bn.act_fwd.rows = 1024 (RL = 256 > T)
    "rows1050": dict(B=150, T=7, C=8, J=1, act="relu", keep=0.8, lens="random"),
}

FIN_NPARTS = (1, 15, 16, 17, 48, 49, 64, 65, 127, 128, 129, 263)
FIN_C = (40, 64, 200)


def f32(v):
  return torch.tensor(float(v), dtype=F32)


def ulp32(x):
  """Spacing of fp32 at |x| (x float64)."""
  a = x.abs().to(F32)
  return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).to(F64)


def live_rows(lens, B, T, margin=0):
  """[B, T, 1] bool: t < len[b] + margin (all rows without a length vector)."""
  if lens is None:
    return torch.ones(B, T, 1, dtype=torch.bool)
  return (torch.arange(T)[None, :] < (lens.long()[:, None] + margin))[:, :, None]


def tiles(x2d, n):
  """[rows, C] -> [ceil(rows / n), n, C], zero padded."""
  rows, C = x2d.shape
  npart = -(-rows // n)
  pad = x2d.new_zeros(npart * n, C)
  pad[:rows] = x2d
  return pad.view(npart, n, C)


def make_inputs(name, **over):
  s = dict(CASES[name])
  s.update(over)
  B, T, C, J, act = s["B"], s["T"], s["C"], s["J"], s["act"]
  g = torch.Generator().manual_seed(sum(map(ord, name)) + 17 * J)
  ys = []
  for j in range(J):
    if j == s.get("cancel"):
      y = torch.randn(B, T, C, generator=g) * 0.25 + 8.0
    else:
      y = torch.randn(B, T, C, generator=g) * (1 + 0.25 * j) + 0.3 * j
    ys.append(y.to(BF16))
  # relu20: the pre-activation is a sum of J normalised inputs, std ~ 12 puts ~5 % of it above the cap
  gs = 12.0 / math.sqrt(J) if act == "relu20" else 1.0
  s["gammas"] = [(torch.rand(C, generator=g) + 0.5) * gs for _ in range(J)]
  s["betas"] = [torch.randn(C, generator=g) * 0.1 for _ in range(J)]
  s["mm"] = [torch.randn(C, generator=g) * 0.5 for _ in range(J)]
  s["mv"] = [torch.rand(C, generator=g) + 0.5 for _ in range(J)]
  s["ys"] = ys
  s["dout"] = torch.randn(B, T, C, generator=g).to(BF16)
  s["pre"] = [torch.randn(2, C, generator=g) for _ in range(J)]
  lens = s["lens"]
  if isinstance(lens, str):
    lens = torch.randint(0, T + 1, (B,), generator=g)
    lens[0], lens[1] = T, 0
  s["lens"] = None if lens is None else torch.as_tensor(lens, dtype=torch.int32)
  return s


def check_inputs(name, **over):
  """Host-only conditions on a case's inputs; for relu20 the fraction of outputs at the cap (float64 BatchNorm
  of the inputs): between 0.2 % and 20 %, or the cap's two sides are not both exercised."""
  R = make_inputs(name, **over)
  if R["act"] != "relu20":
    return None
  v = 0
  for y, ga, be in zip(R["ys"], R["gammas"], R["betas"]):
    x = y.double().reshape(-1, R["C"])
    m, var = x.mean(0), x.var(0, unbiased=False)
    v = v + (x - m) / torch.sqrt(var + EPS) * ga.double() + be.double()
  frac = float((v >= RELU_CAP).double().mean())
  assert 0.002 < frac < 0.2, (name, frac)
  return frac


# ---------------------------------------------------------------------------------------------------------
# compare()
# ---------------------------------------------------------------------------------------------------------
class _Checks:
  def __init__(self):
    self.ratios, self.fails = {}, []

  def within(self, name, got, ref, bound):
    """|got - ref| <= bound elementwise (a NaN fails); the ratio of an element with bound 0 is 0 or inf."""
    got = got.to(F64)
    ref, bound = ref.to(F64).expand_as(got), bound.to(F64).expand_as(got)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf))
    ratio = torch.where(torch.isnan(ratio), math.inf, ratio)
    r = float(ratio.max()) if ratio.numel() else 0.0
    self.ratios[name] = max(self.ratios.get(name, 0.0), r)
    if bool(bad.any()):
      i = int(torch.where(bad.reshape(-1), ratio.reshape(-1), -1.0).argmax())
      self.fails.append("%s: %d of %d outside the bound; worst at flat index %d: got %.9g want %.9g bound %.3g" % (
          name, int(bad.sum()), bad.numel(), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
          float(bound.reshape(-1)[i])))

  def bits(self, name, got, ref, mask=None):
    """Bit-identical (where mask holds)."""
    it = {2: torch.int16, 4: torch.int32}[got.element_size()]
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = got.contiguous().view(it) != ref.contiguous().view(it)
    if mask is not None:
      bad = bad & mask.expand_as(bad)
    self.ratios.setdefault(name, 0.0)
    if bool(bad.any()):
      i = int(bad.reshape(-1).to(torch.int8).argmax())
      self.ratios[name] = math.inf
      self.fails.append("%s: %d of %d differ in bits; first at flat index %d: got %r want %r" % (
          name, int(bad.sum()), bad.numel(), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i])))


def _cmp_stats(got, inp, chk):
  # partial[p, 0 / 1, c] = sum / sum of squares over rows [128 p, 128 p + 128). A bf16 value and the square of
  # one (16 significand bits) are exact in fp32, so only the <= 128-term sums round: 128 u32 sum|terms|.
  x = tiles(inp["y"].double(), STATS_ROWS)
  p = got["partial"]
  chk.within("sum", p[:, 0], x.sum(1), STATS_ROWS * U32 * x.abs().sum(1))
  chk.within("sumsq", p[:, 1], (x * x).sum(1), STATS_ROWS * U32 * (x * x).sum(1))


def _cmp_finalize(got, inp, chk):
  # The kernel sums the partials in fp64 (any order: ~nparts 2^-53 relative to sum|p|, far below an fp32 ulp),
  # forms m, v = max(q / count - m^2, 0) and the Bessel-corrected v in fp64 and rounds each to fp32 once. The
  # oracle does the same and keeps the fp32-rounded values as its reference:
  #   mean, new moving_var        2 ulp (one for a flipped rounding of the fp64 value, one for the fp32 update
  #                               a * momentum + b * (1 - momentum): two roundings relative to |a| + |b|, which
  #                               for the variances, both >= 0, is the result itself)
  #   new moving_mean             2 ulp of |a momentum| + |b (1 - momentum)|: the two terms may differ in sign
  #   rstd, scale                 4 ulp: rsqrtf (1 ulp) of a once-rounded argument, one product for scale
  #   shift = beta - mean g rstd  4 u32 (|beta| + |mean g rstd|)
  eps, mom = f32(inp["eps"]).double(), f32(inp["momentum"])
  om, mom = (f32(1.0) - mom).double(), mom.double()
  C = got["scale"].numel()
  g = inp["gamma"].double() if inp["gamma"] is not None else torch.ones(C, dtype=F64)
  b = inp["beta"].double() if inp["beta"] is not None else torch.zeros(C, dtype=F64)
  mm, mv = inp["moving_mean"], inp["moving_var"]
  if inp["training"]:
    p, count = inp["partial"].double(), float(inp["count"])
    m = p[:, 0].sum(0) / count
    v = (p[:, 1].sum(0) / count - m * m).clamp_min(0.0)
    mean, var = m.float().double(), v.float().double()
    mean_bound = 2 * ulp32(mean)
    if mm is not None:
      unb = (v * count / (count - 1.0) if count > 1 else v).float().double()
      a, c = mm.double() * mom, mean * om
      chk.within("moving_mean", got["moving_mean"], a + c, 2 * ulp32(a.abs() + c.abs()))
      ref = mv.double() * mom + unb * om
      chk.within("moving_var", got["moving_var"], ref, 2 * ulp32(ref))
  else:
    mean, var = mm.double(), mv.double()
    mean_bound = torch.zeros(C, dtype=F64)
    chk.bits("moving_mean", got["moving_mean"], mm)
    chk.bits("moving_var", got["moving_var"], mv)
  rstd = 1.0 / torch.sqrt(var + eps)
  if got.get("mean") is not None:
    chk.within("mean", got["mean"], mean, mean_bound)
    chk.within("rstd", got["rstd"], rstd, 4 * ulp32(rstd))
  chk.within("scale", got["scale"], g * rstd, 4 * ulp32(g * rstd))
  t = mean * g * rstd
  chk.within("shift", got["shift"], b - t, 4 * U32 * (b.abs() + t.abs()))


def _act(v, act):
  if act == "relu":
    return v.clamp_min(0.0)
  if act == "tanh":
    return torch.tanh(v)
  if act == "relu20":
    return v.clamp(0.0, RELU_CAP)
  return v


def _cmp_act_fwd(got, inp, chk):
  # v = sum_j (y_j sc_j + sh_j): J fused (or 2J unfused) operations and J - 1 additions, each rounding relative
  # to a partial sum of at most sum_j (|y_j sc_j| + |sh_j|): delta = (2J + 2) u32 of that. Every activation is
  # 1-Lipschitz (tanhf adds 2^-21), the product with fl(1 / keep) adds 2 u32 |ref| <= delta / keep / 2, and the
  # bf16 store rounds the perturbed value: ubf (|ref| + 1.5 delta / keep). Together below ubf |ref| + 2 delta / keep.
  out = got["out"]
  B, T, C = out.shape
  live = live_rows(inp["lens"], B, T)
  J = len(inp["ys"])
  v = torch.zeros(B, T, C, dtype=F64)
  mag = torch.zeros(B, T, C, dtype=F64)
  for y, sc, sh in zip(inp["ys"], inp["scales"], inp["shifts"]):
    t = torch.where(live, y.double(), 0.0) * sc.double()
    v += t + sh.double()
    mag += t.abs() + sh.double().abs()
  delta = (2 * J + 2) * U32 * mag
  inv = 1.0 / float(f32(inp["keep"]))
  kept = inp["mask"] & live
  ref = torch.where(kept, _act(v, inp["act"]) * inv, 0.0)
  bound = UBF * ref.abs() + 2 * delta * inv + (2.0 ** -21 * inv if inp["act"] == "tanh" else 0.0)
  chk.within("out", out, ref, torch.where(kept, bound, 0.0))
  chk.bits("out: +0 where dropped or t >= len", out, torch.zeros_like(out), ~kept)


def _cmp_reduce(got, inp, chk):
  dz, P = got["dz"], got["partial"]
  B, T, C = dz.shape
  n, act = inp["n"], inp["act"]
  live = live_rows(inp["lens"], B, T)
  kept = inp["mask"] & live
  keep32 = f32(inp["keep"])
  inv32 = f32(1.0) / keep32
  o = inp["out"].float()
  if act != "tanh":
    # act' is 0 or 1, taken from the STORED output: dz = bf16(fp32(dout) * fp32(1 / keep)) where it is 1 (one
    # IEEE product, one RNE rounding), +0 elsewhere; relu20: 0 < out < bf16(20 * fl(1 / keep))
    cap = (f32(RELU_CAP) * inv32).to(BF16).float()
    passes = {"none": kept, "relu": kept & (o > 0), "relu20": kept & (o > 0) & (o < cap)}[act]
    val = (inp["dout"].float() * inv32).to(BF16)
    chk.bits("dz", dz, torch.where(passes, val, torch.zeros_like(val)))
  else:
    # th = out keep, 1 - th^2, dout / keep * that: the roundings before the bf16 store stay below 4 u32 |dout| / keep
    th = torch.where(kept, o.double() * keep32.double(), 0.0)
    d = torch.where(kept, inp["dout"].double(), 0.0)
    ref = d * inv32.double() * (1.0 - th * th)
    chk.within("dz", dz, ref, UBF * ref.abs() + 4 * U32 * d.abs() * inv32.double())
  # partial[p, 0] = sum of the device's own dz over the tile's n rows: n u32 sum|dz|.
  # partial[p, 1 + j] = rstd (sum dz y - mean sum dz) = sum dz xhat: dz y is exact in fp32, the two n-term sums
  # and the three closing operations give (n + 4) u32 rstd (sum|dz y| + |mean| sum|dz|).
  D = tiles(dz.double().reshape(-1, C), n)
  Dabs = D.abs().sum(1)
  chk.within("partial[0]", P[:, 0], D.sum(1), n * U32 * Dabs)
  for j, (y, mean, rstd) in enumerate(zip(inp["ys"], inp["means"], inp["rstds"])):
    DY = D * tiles(torch.where(live, y.double(), 0.0).reshape(-1, C), n)
    mean, rstd = mean.double(), rstd.double()
    ref = rstd * (DY.sum(1) - mean * D.sum(1))
    chk.within("partial[1+j]", P[:, 1 + j], ref, (n + 4) * U32 * rstd * (DY.abs().sum(1) + mean.abs() * Dabs))


def _cmp_bwd_finalize(got, inp, chk):
  # fp64 sums (2^-50 sum|partials| covers any order over <= 263 parts), one rounding to fp32: 1 ulp; with
  # accumulate the rounded sum is added to the old value in fp32: 1 ulp of the sum + 1 ulp of the result.
  # raw: sx = rstd (sum dz y - mean sum dz) in fp64, as the kernel forms it.
  p, count = inp["partial"].double(), float(inp["count"])
  sd, sx = p[:, 0].sum(0), p[:, inp["q"]].sum(0)
  ad, ax = 2.0 ** -50 * p[:, 0].abs().sum(0), 2.0 ** -50 * p[:, inp["q"]].abs().sum(0)
  if inp.get("mean") is not None:
    mean, rstd = inp["mean"].double(), inp["rstd"].double()
    sx, ax = rstd * (sx - mean * sd), rstd * (ax + mean.abs() * ad)
  for name, s, a, pre in (("dgamma", sx, ax, inp["pre_dgamma"]), ("dbeta", sd, ad, inp["pre_dbeta"])):
    if pre is None:
      assert got[name] is None
    elif inp["accumulate"]:
      ref = pre.double() + s
      chk.within(name, got[name], ref, ulp32(ref) + ulp32(s) + a)
    else:
      chk.within(name, got[name], s, ulp32(s) + a)
  chk.within("c1", got["c1"], sd / count, ulp32(sd / count) + ad / count)
  chk.within("c2", got["c2"], sx / count, ulp32(sx / count) + ax / count)


def _cmp_apply(got, inp, chk):
  # dy = gamma rstd (dz - c1 - xhat c2) = A dz + Bq y + Cc, A = gamma rstd, Bq = -gamma rstd^2 c2,
  # Cc = gamma rstd (mean rstd c2 - c1): at most 6 roundings on each of the four terms before the bf16 store.
  # Rows t >= len + margin are +0; under dz_to_len dz counts as 0 at t >= len whatever it holds.
  dy = got["dy"]
  B, T, C = dy.shape
  rows_kept = live_rows(inp["lens"], B, T, inp["margin"])
  rows_dz = live_rows(inp["lens"], B, T, 0) if inp["dz_to_len"] else rows_kept
  d = torch.where(rows_dz, inp["dz"].double(), 0.0)
  y = torch.where(rows_kept, inp["y"].double(), 0.0)
  g = inp["gamma"].double() if inp["gamma"] is not None else torch.ones(C, dtype=F64)
  rs, mean, c1, c2 = (inp[k].double() for k in ("rstd", "mean", "c1", "c2"))
  t0, t1, t2, t3 = g * rs * d, -g * rs * rs * c2 * y, g * rs * rs * mean * c2, -g * rs * c1
  ref = torch.where(rows_kept, t0 + t1 + t2 + t3, 0.0)
  bound = UBF * ref.abs() + 6 * U32 * (t0.abs() + t1.abs() + t2.abs() + t3.abs())
  chk.within("dy", dy, ref, torch.where(rows_kept, bound, 0.0))
  chk.bits("dy: +0 at t >= len + margin", dy, torch.zeros_like(dy), ~rows_kept)


_STAGES = {"stats": _cmp_stats, "finalize": _cmp_finalize, "act_fwd": _cmp_act_fwd, "reduce": _cmp_reduce,
           "bwd_finalize": _cmp_bwd_finalize, "bwd_apply": _cmp_apply}
STAGES = tuple(_STAGES)


def compare(stage, got, inp):
  """One stage's outputs `got` against the float64 oracle of its inputs `inp`:
  ({output: largest error / bound}, [a line per output that breaks its bound])."""
  chk = _Checks()
  _STAGES[stage](got, inp, chk)
  return chk.ratios, chk.fails


# ---------------------------------------------------------------------------------------------------------
# the walks
# ---------------------------------------------------------------------------------------------------------
class _Run:
  def __init__(self, name, log):
    self.name, self.log, self.ratios, self.fails = name, log, {}, []

  def cmp(self, stage, got, inp, tag=""):
    ratios, fails = compare(stage, got, inp)
    for k, v in ratios.items():
      key = "%s.%s" % (stage, k)
      self.ratios[key] = max(self.ratios.get(key, 0.0), v)
    self.fails.extend("%s %s %s %s" % (self.name, stage, tag, f) for f in fails)

  def same(self, what, a, b, mask=None):
    chk = _Checks()
    chk.bits(what, a, b, mask)
    self.fails.extend("%s %s" % (self.name, f) for f in chk.fails)

  def within(self, stage, name, got, ref, bound):
    chk = _Checks()
    chk.within(name, got, ref, bound)
    key = "%s.%s" % (stage, name)
    self.ratios[key] = max(self.ratios.get(key, 0.0), chk.ratios[name])
    self.fails.extend("%s %s %s" % (self.name, stage, f) for f in chk.fails)

  def report(self):
    for k in sorted(self.ratios):
      self.log("BN-RATIO %-22s %-34s %.3g" % (self.name, k, self.ratios[k]))
    for f in self.fails:
      self.log("BN-FAIL " + f)


def check_case(name, be, log=print, poison=math.nan, n=DEFAULT_TILING[1][1], tag=None, **over):
  """Walks case `name` through the six stages on backend `be` (n = rows per workgroup of the reduce tiling in
  force). Returns dict(fails, ratios, out, dz, dys, dense, nparts): fails is empty iff every output kept its bound; dense
  holds the inputs of the dense apply launches that gave dys."""
  R = make_inputs(name, **over)
  B, T, C, J, act, keep, lens = (R[k] for k in ("B", "T", "C", "J", "act", "keep", "lens"))
  rows = B * T
  run = _Run(tag or name, log)
  ys = R["ys"]

  def dead(x, margin=0):
    """x with the rows t >= len + margin replaced by the poison."""
    if lens is None:
      return x
    return torch.where(live_rows(lens, B, T, margin), x, torch.full_like(x, poison))

  # ---- 1, 2: statistics -----------------------------------------------------------------------------------
  fin = []
  for j in range(J):
    y2 = ys[j].reshape(rows, C)
    part = be.stats(y2)
    run.cmp("stats", dict(partial=part), dict(y=y2), "j=%d" % j)
    inp = dict(partial=part, count=rows, gamma=R["gammas"][j], beta=R["betas"][j], eps=EPS, momentum=MOM,
               training=True, moving_mean=R["mm"][j], moving_var=R["mv"][j])
    o = be.finalize(**inp)
    run.cmp("finalize", o, inp, "j=%d" % j)
    fin.append(o)
    if j == R.get("cancel"):
      # momentum 0 leaves fl32(Bessel-corrected batch variance) in moving_var: the device's variance, against
      # the float64 variance of the bf16 inputs within the bound propagated from stage 1,
      # (dq + 2 |m| ds + ds^2 / count) / count, scaled by count / (count - 1), plus the store's ulp
      x = tiles(y2.double(), STATS_ROWS)
      ds = (STATS_ROWS * U32 * x.abs().sum(1)).sum(0)
      dq = (STATS_ROWS * U32 * (x * x).sum(1)).sum(0)
      xx = y2.double()
      m = xx.mean(0)
      unb = ((xx * xx).mean(0) - m * m) * rows / (rows - 1.0)
      o0 = be.finalize(**dict(inp, momentum=0.0, moving_mean=torch.zeros(C), moving_var=torch.zeros(C)))
      bound = (dq + 2 * m.abs() * ds + ds * ds / rows) / rows * rows / (rows - 1.0) + ulp32(unb)
      run.within("finalize", "variance under cancellation", o0["moving_var"], unb, bound)
      assert float((m * m / unb).min()) > 500.0          # the case does cancel: m^2 / v ~ 1000
  scales, shifts = [o["scale"] for o in fin], [o["shift"] for o in fin]
  means, rstds = [o["mean"] for o in fin], [o["rstd"] for o in fin]

  # ---- 3: forward apply -------------------------------------------------------------------------------------
  if keep < 1.0:
    mask = be.dropout_mask(SEED, (B, T, C), keep)
    frac = float(mask.double().mean())
    assert abs(frac - keep) < 5 * math.sqrt(keep * (1 - keep) / mask.numel()), frac
  else:
    mask = torch.ones(B, T, C, dtype=torch.bool)
  ys_p = [dead(y) for y in ys]
  out = be.act_fwd(ys_p, scales, shifts, lens, act, keep, SEED)
  run.cmp("act_fwd", dict(out=out), dict(ys=ys_p, scales=scales, shifts=shifts, lens=lens, act=act, keep=keep, mask=mask))
  if lens is not None:
    run.same("act_fwd: out unchanged by the rows t >= len", out, be.act_fwd(ys, scales, shifts, lens, act, keep, SEED))

  # ---- 4: backward reduce -----------------------------------------------------------------------------------
  dout_p, out_p = dead(R["dout"]), dead(out)
  dz, part = be.reduce(dout_p, out_p, ys_p, means, rstds, lens, act, keep, SEED, n)
  assert part.shape == (-(-rows // n), 1 + J, C), part.shape
  run.cmp("reduce", dict(dz=dz, partial=part), dict(dout=dout_p, out=out_p, ys=ys_p, means=means, rstds=rstds,
                                                    lens=lens, act=act, keep=keep, mask=mask, n=n))
  if lens is not None:
    dz2, part2 = be.reduce(R["dout"], out, ys, means, rstds, lens, act, keep, SEED, n)
    run.same("reduce: dz unchanged by the rows t >= len", dz, dz2)
    run.same("reduce: partial unchanged by the rows t >= len", part, part2)

  # ---- 5: backward finalize (accumulate alternates; input 2 has no dgamma / dbeta) ---------------------------
  bf = []
  for j in range(J):
    pre = (None, None) if j == 2 else (R["pre"][j][0], R["pre"][j][1])
    inp = dict(partial=part, q=1 + j, count=rows, pre_dgamma=pre[0], pre_dbeta=pre[1], accumulate=j % 2)
    o = be.bwd_finalize(**inp)
    run.cmp("bwd_finalize", o, inp, "j=%d" % j)
    bf.append(o)
  # raw entry point: (sum dz, sum dz y) per tile, formed on the host from the device's dz
  jr = R.get("cancel", 0)
  live = live_rows(lens, B, T)
  Dt = tiles(dz.double().reshape(rows, C), n)
  Yt = tiles(torch.where(live, ys[jr].double(), 0.0).reshape(rows, C), n)
  rawp = torch.stack([Dt.sum(1), (Dt * Yt).sum(1)], 1).float().contiguous()
  inp = dict(partial=rawp, q=1, count=rows, pre_dgamma=R["pre"][jr][0], pre_dbeta=R["pre"][jr][1], accumulate=1,
             mean=means[jr], rstd=rstds[jr])
  run.cmp("bwd_finalize", be.bwd_finalize(**inp), inp, "raw j=%d" % jr)

  # ---- 6: backward apply --------------------------------------------------------------------------------------
  dys, dense = [], []
  zero = torch.zeros(B, T, C, dtype=BF16)
  for j in range(J):
    base = dict(y=ys[j], gamma=R["gammas"][j], mean=means[j], rstd=rstds[j], c1=bf[j]["c1"], c2=bf[j]["c2"])
    inp = dict(base, dz=dz, lens=None, margin=0, dz_to_len=False)
    dy = be.apply(**inp)
    run.cmp("bwd_apply", dict(dy=dy), inp, "dense j=%d" % j)
    dys.append(dy)
    dense.append(inp)
    if j == 0:
      inp = dict(inp, gamma=None)
      run.cmp("bwd_apply", dict(dy=be.apply(**inp)), inp, "dense, gamma null")
    if lens is None or j not in (0, J - 1):
      continue
    for margin in (0, 5, 1000):
      inp = dict(base, dz=dead(dz, margin), y=dead(ys[j], margin), lens=lens, margin=margin, dz_to_len=False)
      dyr = be.apply(**inp)
      run.cmp("bwd_apply", dict(dy=dyr), inp, "ragged j=%d margin=%d" % (j, margin))
      run.same("bwd_apply: ragged margin %d = dense on the kept rows, +0 beyond" % margin, dyr,
               torch.where(live_rows(lens, B, T, margin), dy, zero))
      if margin == 5:
        # dz defined up to len only: rows [len, len + margin) are Bq y + Cc whatever dz holds there
        inp = dict(inp, dz=dead(dz, 0), dz_to_len=True)
        dyz = be.apply(**inp)
        run.cmp("bwd_apply", dict(dy=dyz), inp, "ragged_dz j=%d" % j)
        run.same("bwd_apply: ragged_dz = ragged on a dz that is zero past len", dyz, dyr)
  run.report()
  return dict(fails=run.fails, ratios=run.ratios, out=out, dz=dz, dys=dys, dense=dense, nparts=part.shape[0])


def handmade_partials(nparts, C, J=16):
  """[J, nparts, 2, C] (sum, sumsq) of 128-row tiles of x ~ N(0.3, 1) (the last tile holds 91 rows) and the
  row count. Channel 3: q / count = m^2 (1 - 1e-4), a negative variance for the clamp."""
  g = torch.Generator().manual_seed(1000 * nparts + C)
  count = nparts * STATS_ROWS - 37
  s = torch.randn(J, nparts, C, generator=g) * math.sqrt(STATS_ROWS) + 0.3 * STATS_ROWS
  q = STATS_ROWS * 1.09 + torch.randn(J, nparts, C, generator=g) * math.sqrt(2.0 * STATS_ROWS)
  m = s[:, :, 3].double().sum(1) / count
  q[:, :, 3] = (m * m * (1 - 1e-4) * count / nparts).float()[:, None]
  return torch.stack([s, q], 2).contiguous(), count


def check_finalize_handmade(nparts, C, be, log=print):
  """Stages 2 and 5 on hand-made partials [nparts, ., C]: every option of the single entry points, the multi
  entry points bit-identical to the single launches, the raw backward finalize."""
  run = _Run("fin[%d,%d]" % (nparts, C), log)
  g = torch.Generator().manual_seed(7 * nparts + C)
  P, count = handmade_partials(nparts, C)
  J = P.shape[0]
  vec = lambda scale=1.0, shift=0.0: [torch.randn(C, generator=g) * scale + shift for _ in range(J)]
  gam, bet, mm = vec(0.3, 1.0), vec(0.1), vec(0.5)
  mv = [v.abs() + 0.5 for v in vec()]
  base = [dict(partial=P[j], count=count, gamma=gam[j], beta=bet[j], eps=EPS, momentum=MOM, training=True,
               moving_mean=mm[j], moving_var=mv[j]) for j in range(J)]
  single = []
  for j in range(J):
    o = be.finalize(**base[j])
    run.cmp("finalize", o, base[j], "training j=%d" % j)
    single.append(o)
  assert bool((P[0].double()[:, 1].sum(0) / count - (P[0].double()[:, 0].sum(0) / count) ** 2)[3] < 0)
  variants = [dict(gamma=None, beta=None), dict(gamma=None), dict(want_stats=False),
              dict(moving_mean=None, moving_var=None), dict(training=False, partial=None),
              dict(training=False, partial=None, gamma=None, beta=None, want_stats=False)]
  if nparts == 1:
    # count = 1: one row; its square rounds in fp32, so q - m^2 lands on either side of zero (the clamp)
    x = torch.randn(C, generator=g) * 3
    variants.append(dict(partial=torch.stack([x, x * x])[None].contiguous(), count=1))
    # and bn_stats of a single-row tensor, its partials finalized with count = 1 (variance exactly 0)
    x = x.to(BF16)[None]
    part = be.stats(x)
    run.cmp("stats", dict(partial=part), dict(y=x), "single row")
    variants.append(dict(partial=part, count=1))
  for var in variants:
    inp = dict(base[0], **var)
    want_stats = inp.pop("want_stats", True)
    o = be.finalize(want_stats=want_stats, **inp)
    assert want_stats or o["mean"] is None
    run.cmp("finalize", o, inp, " ".join("%s=%s" % (k, "null" if v is None else v) for k, v in var.items()
                                         if not torch.is_tensor(v)))
  for Jm in (1, 11, 16):
    for training in (True, False):
      items = [dict(base[j], training=training) for j in range(Jm)]
      for j, o in enumerate(be.finalize_multi(items)):
        ref = single[j] if training else be.finalize(**items[j])
        for k in ("mean", "rstd", "scale", "shift", "moving_mean", "moving_var"):
          run.same("finalize_multi J=%d training=%d j=%d %s" % (Jm, training, j, k), o[k], ref[k])
  # ---- backward -----------------------------------------------------------------------------------------------
  Jb = {40: 5, 64: 12, 200: 1}.get(C, 3)
  Pb = torch.randn(nparts, 1 + Jb, C, generator=g) * 10
  pre = [torch.randn(2, C, generator=g) * 30 for _ in range(Jb)]
  for acc in (0, 1):
    singles = []
    for j in range(Jb):
      null = j == 1
      inp = dict(partial=Pb, q=1 + j, count=count, pre_dgamma=None if null else pre[j][0],
                 pre_dbeta=None if null else pre[j][1], accumulate=acc)
      o = be.bwd_finalize(**inp)
      run.cmp("bwd_finalize", o, inp, "accumulate=%d j=%d" % (acc, j))
      singles.append(o)
    multi = be.bwd_finalize_multi(Pb, count, [None if j == 1 else pre[j][0] for j in range(Jb)],
                                  [None if j == 1 else pre[j][1] for j in range(Jb)], acc)
    for j in range(Jb):
      for k in ("dgamma", "dbeta", "c1", "c2"):
        if singles[j][k] is None:
          assert multi[j][k] is None
        else:
          run.same("bwd_finalize_multi accumulate=%d j=%d %s" % (acc, j, k), multi[j][k], singles[j][k])
    # raw: planes (sum dz, sum dz y) with a mean that makes sum dz y - mean sum dz cancel
    rawp = Pb[:, :2].contiguous()
    rawp[:, 1] = rawp[:, 0] * 2.0 + rawp[:, 1] * 0.01
    inp = dict(partial=rawp, q=1, count=count, pre_dgamma=pre[0][0], pre_dbeta=pre[0][1], accumulate=acc,
               mean=torch.full((C,), 2.0) + 0.01 * torch.randn(C, generator=g), rstd=torch.rand(C, generator=g) + 0.5)
    run.cmp("bwd_finalize", be.bwd_finalize(**inp), inp, "raw accumulate=%d" % acc)
    inp = dict(inp, pre_dgamma=None, pre_dbeta=None)
    run.cmp("bwd_finalize", be.bwd_finalize(**inp), inp, "raw null accumulate=%d" % acc)
  run.report()
  return dict(fails=run.fails, ratios=run.ratios)


def tiling_initialiser():
  """The g_tiling initialiser of csrc/batchnorm.hip as ((groups, rows), ...)."""
  src = open(os.path.join(REPO, "openseq2seq_amd", "csrc", "batchnorm.hip")).read()
  m = re.search(r"static int g_tiling\[3\]\[2\]\s*=\s*\{([^;]*)\};", src)
  v = [int(x) for x in re.findall(r"\d+", m.group(1))]
  return tuple((v[2 * i], v[2 * i + 1]) for i in range(3))
