"""CPU proof that the bounds of tests/_bn_cases.py can fail and are not too tight: compare() accepts two fp32
torch emulations of every kernel of csrc/batchnorm.hip (tile-ordered sums, bf16 stores; the second sums in
reverse order and leaves y * sc + sh unfused) and rejects eleven wrong kernels. No GPU."""
import math

import pytest
import torch

import _bn_cases as bc
from _bn_cases import BF16, F32, f32, live_rows, tiles


class Emu:
  """fp32 emulation of the kernels as the header states them. reverse: the other summation order, unfused
  products. mutant: one of MUTANTS."""

  def __init__(self, reverse=False, mutant=None):
    self.reverse, self.mutant = reverse, mutant

  def _seqsum(self, x, live_count=None):
    """Sequential fp32 sum over dim 1 of [np, n, C]; drop_last_row: each tile omits its last row."""
    npart, n, C = x.shape
    if self.mutant == "drop_last_row":
      x = x.clone()
      for p in range(npart):
        x[p, min(n, live_count - p * n) - 1] = 0
    s = torch.zeros(npart, C, dtype=F32)
    for r in (reversed(range(n)) if self.reverse else range(n)):
      s = s + x[:, r]
    return s

  def _fma(self, a, b, c):
    if self.reverse:
      return a * b + c
    return (a.double() * b.double() + c.double()).float()

  def stats(self, y2d):
    x = tiles(y2d.float(), bc.STATS_ROWS)
    return torch.stack([self._seqsum(x, y2d.shape[0]), self._seqsum(x * x, y2d.shape[0])], 1)

  def finalize(self, partial, count, gamma, beta, eps, momentum, training, moving_mean, moving_var, want_stats=True):
    C = (gamma if gamma is not None else moving_mean if moving_mean is not None else partial[0, 0]).numel()
    eps, mom = f32(eps), f32(momentum)
    nmm, nmv = moving_mean, moving_var
    if training:
      p = partial.double().flip(0) if self.reverse else partial.double()
      m = p[:, 0].sum(0) / count
      v = (p[:, 1].sum(0) / count - m * m).clamp_min(0.0)
      mean, var = m.float(), v.float()
      if moving_mean is not None:
        unb = v * count / (count - 1.0) if count > 1 and self.mutant != "no_bessel" else v
        nmm = moving_mean * mom + mean * (f32(1.0) - mom)
        nmv = moving_var * mom + unb.float() * (f32(1.0) - mom)
    else:
      mean, var = moving_mean.clone(), moving_var.clone()
    rstd = torch.rsqrt(var + eps)
    g = gamma if gamma is not None else torch.ones(C)
    b = beta if beta is not None else torch.zeros(C)
    scale = g * rstd
    shift = b + mean * scale if self.mutant == "shift_plus" else b - mean * g * rstd
    return dict(mean=mean if want_stats else None, rstd=rstd if want_stats else None, scale=scale, shift=shift,
                moving_mean=nmm, moving_var=nmv)

  def finalize_multi(self, items):
    return [self.finalize(**it) for it in items]

  def dropout_mask(self, seed, shape, keep):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < keep

  def act_fwd(self, ys, scales, shifts, lens, act, keep, seed):
    B, T, C = ys[0].shape
    live = live_rows(lens, B, T)
    js = list(range(len(ys)))
    if self.mutant == "skip_last_input" and len(ys) == 5:
      js = js[:-1]
    v = torch.zeros(B, T, C, dtype=F32)
    for j in (reversed(js) if self.reverse else js):
      v = v + self._fma(torch.where(live, ys[j].float(), 0.0), scales[j], shifts[j])
    inv = f32(1.0) / f32(keep)
    if act == "relu20" and self.mutant == "cap_after_scale":
      a = (v.clamp_min(0.0) * inv).clamp_max(bc.RELU_CAP)
    else:
      a = bc._act(v, act)
      if keep < 1.0:
        a = a * inv
    if keep < 1.0:
      a = torch.where(self.dropout_mask(seed, (B, T, C), keep), a, 0.0)
    return torch.where(live, a, 0.0).to(BF16)

  def reduce(self, dout, out, ys, means, rstds, lens, act, keep, seed, n):
    B, T, C = dout.shape
    live = live_rows(lens, B, T)
    kept = live & self.dropout_mask(seed, (B, T, C), keep) if keep < 1.0 else live.expand(B, T, C)
    keep32 = f32(keep)
    inv = f32(1.0) / keep32
    ov = out.float()
    scaled = dout.float() * inv if keep < 1.0 else dout.float()
    if act == "tanh":
      th = ov if self.mutant == "tanh_no_keep" else ov * keep32
      dzv = torch.where(kept, scaled * (1.0 - th * th), 0.0)
    else:
      cap = (f32(bc.RELU_CAP) * inv).to(BF16).float()
      passes = {"none": kept, "relu": kept & (ov > 0), "relu20": kept & (ov > 0) & (ov < cap)}[act]
      dzv = torch.where(passes, scaled, 0.0)
    dz = dzv.to(BF16)
    rows = B * T
    D = tiles(dz.float().reshape(rows, C), n)
    sd = self._seqsum(D, rows)
    planes = [sd]
    for j, y in enumerate(ys):
      sx = self._seqsum(D * tiles(torch.where(live, y.float(), 0.0).reshape(rows, C), n), rows)
      if self.mutant == "no_mean_sd":
        sx = rstds[j] * sx
      else:
        sx = rstds[j] * (sx - means[j] * sd)
      if self.mutant == "skip_last_input" and len(ys) == 5 and j == 4:
        sx = torch.zeros_like(sx)
      planes.append(sx)
    return dz, torch.stack(planes, 1)

  def bwd_finalize(self, partial, q, count, pre_dgamma, pre_dbeta, accumulate, mean=None, rstd=None):
    p = partial.double().flip(0) if self.reverse else partial.double()
    sd, sx = p[:, 0].sum(0), p[:, q].sum(0)
    if mean is not None:
      sx = rstd.double() * (sx - mean.double() * sd)
    acc = accumulate and self.mutant != "accumulate_ignored"
    old = lambda t: t if acc else torch.zeros_like(t)
    return dict(dgamma=None if pre_dgamma is None else old(pre_dgamma) + sx.float(),
                dbeta=None if pre_dbeta is None else old(pre_dbeta) + sd.float(),
                c1=(sd / count).float(), c2=(sx / count).float())

  def bwd_finalize_multi(self, partial, count, pres_dg, pres_db, accumulate):
    return [self.bwd_finalize(partial, 1 + j, count, pres_dg[j], pres_db[j], accumulate) for j in range(len(pres_dg))]

  def apply(self, dz, y, gamma, mean, rstd, c1, c2, lens, margin, dz_to_len):
    B, T, C = dz.shape
    rows_kept = live_rows(lens, B, T, margin)
    rows_dz = live_rows(lens, B, T, 0) if dz_to_len and self.mutant != "dz_to_len_reads_dz" else rows_kept
    g = gamma if gamma is not None else torch.ones(C)
    A = g * rstd
    Bq = -g * rstd * rstd * c2
    Cc = g * rstd * (mean * rstd * c2 - (0.0 if self.mutant == "cc_no_c1" else c1))
    d = torch.where(rows_dz, dz.float(), 0.0)
    yv = torch.where(rows_kept, y.float(), 0.0)
    v = self._fma(A, d, self._fma(Bq, yv, Cc.expand(B, T, C)))
    written = live_rows(lens, B, T, 0) if self.mutant == "margin_ignored" else rows_kept
    return torch.where(written, v, 0.0).to(BF16)


# mutant: (stage whose compare() must reject it, overrides that make every geometry reach the mutated code)
MUTANTS = {
    "no_bessel": ("finalize", {}),                                   # moving variance without n / (n - 1)
    "shift_plus": ("finalize", {}),                                  # shift = beta + mean * scale
    "cap_after_scale": ("act_fwd", dict(act="relu20", keep=0.8)),    # min(relu(v) / keep, 20)
    "tanh_no_keep": ("reduce", dict(act="tanh", keep=0.9)),          # tanh' from out, not out * keep
    "drop_last_row": ("stats", {}),                                  # a tile omits its last row (reduce as well)
    "no_mean_sd": ("reduce", {}),                                    # sum dz xhat without mean * sum dz
    "cc_no_c1": ("bwd_apply", {}),                                   # Cc without the c1 term
    "margin_ignored": ("bwd_apply", {}),                             # rows >= len zeroed
    "dz_to_len_reads_dz": ("bwd_apply", {}),                         # dz_to_len reads dz at t >= len
    "accumulate_ignored": ("bwd_finalize", {}),                      # dgamma / dbeta overwritten
    "skip_last_input": ("act_fwd", dict(J=5)),                       # the last of J = 5 inputs skipped
}
MUTANT_CASES = ("c24", "c40", "c264")
quiet = lambda *a: None


@pytest.mark.parametrize("name", list(bc.CASES))
def test_inputs(name):
  frac = bc.check_inputs(name)
  assert (frac is not None) == (bc.CASES[name]["act"] == "relu20")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", list(bc.CASES))
def test_accepts_emulation(name, reverse):
  res = bc.check_case(name, Emu(reverse=reverse), log=quiet)
  assert not res["fails"], "\n".join(res["fails"])
  assert set(k.split(".")[0] for k in res["ratios"]) == set(bc.STAGES)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", bc.TILED_CASES)
def test_accepts_emulation_other_tile_rows(name, reverse):
  for _, n in bc.TILINGS:
    res = bc.check_case(name, Emu(reverse=reverse), log=quiet, n=n)
    assert not res["fails"], "\n".join(res["fails"])


@pytest.mark.parametrize("name", MUTANT_CASES)
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_rejects_mutant(mutant, name):
  stage, over = MUTANTS[mutant]
  if "act" in over:
    bc.check_inputs(name, **over)
  # a finite poison: the mutants that read a forbidden row are rejected by the bound, not by a NaN
  res = bc.check_case(name, Emu(mutant=mutant), log=quiet, poison=1.5, **over)
  hits = [f for f in res["fails"] if " %s " % stage in f]
  assert hits, (mutant, name, res["fails"])
  if mutant == "drop_last_row":
    assert any(" reduce " in f and "partial" in f for f in res["fails"])
  if mutant == "skip_last_input":
    assert any(" reduce " in f and "partial[1+j]" in f for f in res["fails"])
  # and the unmutated emulation passes on the same inputs
  res = bc.check_case(name, Emu(), log=quiet, poison=1.5, **over)
  assert not res["fails"], "\n".join(res["fails"])


@pytest.mark.parametrize("nparts", bc.FIN_NPARTS)
def test_finalize_handmade(nparts):
  for C in bc.FIN_C:
    for reverse in (False, True):
      res = bc.check_finalize_handmade(nparts, C, Emu(reverse=reverse), log=quiet)
      assert not res["fails"], "\n".join(res["fails"])
    for mutant in ("no_bessel", "shift_plus", "accumulate_ignored"):
      res = bc.check_finalize_handmade(nparts, C, Emu(mutant=mutant), log=quiet)
      assert any(" %s " % MUTANTS[mutant][0] in f for f in res["fails"]), (mutant, nparts, C)


def test_tiling_defaults_match_the_source():
  """The GPU test restores these after every tiling run: they must be the g_tiling initialiser."""
  assert bc.tiling_initialiser() == bc.DEFAULT_TILING


def test_compare_flags_nan_and_negative_zero():
  x = torch.ones(4, dtype=BF16)
  chk = bc._Checks()
  chk.within("x", torch.tensor([1.0, math.nan]), torch.ones(2), torch.ones(2))
  chk.bits("z", torch.tensor([0.0, -0.0], dtype=BF16), torch.zeros(2, dtype=BF16))
  assert len(chk.fails) == 2 and x.dtype == BF16
