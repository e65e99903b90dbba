"""CPU proof that the bounds of tests/_dw_cases.py can fail and are not too tight: compare() accepts two fp32 torch
emulations of every operation of csrc/depthwise.hip on every case of the table (taps summed in order with bf16
stores, the matrix-core class with hi + lo bf16 taps and a bf16 rounding in front of the fused epilogue; the second
sums in reverse order, unfused) and rejects the wrong kernels of MUTANTS. The dispatcher's class arithmetic, written
out again in _dw_cases.py, is checked to reach every class with the table. No GPU."""
import functools

import pytest
import torch

import _dw_cases as dc
from _dw_cases import BF16, F32, f32, mask_rows, row_tiles, tap_rows


class Emu:
  """fp32 emulation of the kernels as the header states them. reverse: the other summation order, unfused products.
  mutant: one of MUTANTS."""

  def __init__(self, reverse=False, mutant=None):
    self.reverse, self.mutant = reverse, mutant

  def num_parts(self, B, tout, K):
    return dc.num_parts(B, tout, K)

  def _fma(self, a, b, c):
    if self.reverse:
      return a * b + c
    return (a.double() * b.double() + c.double()).float()

  def _rows(self, x, in_len, K, stride, dil, padl, tout):
    xm = x.float() if self.mutant == "read_dead_rows" else mask_rows(x.float(), in_len)
    if self.mutant == "pad_off_by_one":
      padl += 1
    return tap_rows(xm, K, stride, 1 if self.mutant == "dil_taps" else dil, padl, tout)

  def _conv(self, rows, w, flip, cls):
    K = w.shape[0]
    w = w.flip(0) if flip and self.mutant != "no_flip" else w
    ks = list(range(K - 1 if self.mutant == "drop_last_tap" else K))
    ks = ks[::-1] if self.reverse else ks
    acc = torch.zeros_like(rows(0))
    if cls[0] == "mfma":
      hi = w.to(BF16).float()
      lo = (w - hi).to(BF16).float()
      for k in ks:
        acc = self._fma(rows(k), hi[k], acc)
        if self.mutant != "no_lo":
          acc = self._fma(rows(k), lo[k], acc)
    else:
      for k in ks:
        acc = self._fma(rows(k), w[k], acc)
    return acc

  def _drops_row(self, cls, op):
    return self.mutant == "drop_row_%s_%s" % (op, cls[0])

  def fwd(self, x, w, in_len, out_len, tout, stride, dil, pad_left, flip, variant):
    K = w.shape[0]
    cls = dc.fwd_class(K, stride, dil, variant)
    y = self._conv(self._rows(x, in_len, K, stride, dil, pad_left, tout), w, flip, cls).to(BF16)
    if self._drops_row(cls, "fwd"):
      tile = dc.fwd_tile(cls, K)
      y[:, tile - 1::tile] = 0
    if self.mutant == "skip_last_group":
      y[..., -8:] = 0
    return y

  def wgrad(self, x, dy, dw0, in_len, stride, dil, pad_left, variant, det):
    K = dw0.shape[0]
    cls = dc.wgrad_class(K, stride, dil, variant)
    rows = self._rows(x, in_len, K, stride, dil, pad_left, dy.shape[1])
    d = dy.float()
    if self._drops_row(cls, "wgrad"):
      d = d.clone()
      tile = dc.wgrad_tile(cls)
      d[:, tile - 1::tile] = 0
    S = torch.zeros(K, dy.shape[2], dtype=F32)
    for k in range(K - 1 if self.mutant == "drop_last_tap" else K):
      t = rows(k) * d                           # bf16 x bf16: exact
      S[k] = (t.flip(0, 1) if self.reverse else t).sum((0, 1))
    if self.mutant == "skip_last_group":
      S[:, -8:] = 0
    return S if self.mutant == "dw_overwrite" else dw0 + S

  def fused(self, dz, w, addend, alias, mask_ref, stat_ref, out_len, pad_left, mask_scale):
    K = w.shape[0]
    B, tout, C = mask_ref.shape
    cls = dc.fwd_class(K, 1, 1, -1)
    conv = self._conv(self._rows(dz, None, K, 1, 1, pad_left, tout), w, 1, cls).to(BF16).float()
    ad = addend.float() if addend is not None else torch.zeros(())
    m = mask_ref.float()
    passes = m >= 0 if self.mutant == "mask_ge" else m > 0
    scale = f32(1.0) if self.mutant == "no_mask_scale" else f32(mask_scale)
    if self.mutant == "addend_after_mask":
      v = torch.where(passes, conv * scale, 0.0) + ad
    else:
      v = torch.where(passes, (conv + ad) * scale, 0.0)
    dx = v.to(BF16)
    Tt = dc.dm_geom(K)["tile"]
    ntt = dc.ceil_div(tout, Tt)
    src = v if self.mutant == "stats_unrounded" else dx.float()
    order = (lambda t: t.flip(1)) if self.reverse else (lambda t: t)
    stats = torch.stack([order(row_tiles(src, Tt)).sum(1), order(row_tiles(src * stat_ref.float(), Tt)).sum(1)], 1)
    if self.mutant == "dead_tile_stats" and out_len is not None:
      raw = row_tiles(conv + ad, Tt).sum(1)
      dead = (torch.arange(ntt)[None, :] * Tt >= out_len[:, None]).reshape(-1)
      stats[dead, 0] = raw[dead]
    if self.mutant == "part_index":             # tile-major instead of sample-major
      stats = stats.view(B, ntt, 2, C).transpose(0, 1).reshape(B * ntt, 2, C).contiguous()
    return dx, stats


def _quiet(*a):
  pass


@pytest.mark.parametrize("reverse", (False, True), ids=("in_order", "reverse"))
@pytest.mark.parametrize("op", ("fwd", "wgrad", "fused"))
def test_emulations_inside_every_bound(op, reverse):
  fails = []
  for name, s in dc.CASES.items():
    if s["op"] == op:
      fails += dc.check_case(name, Emu(reverse), log=_quiet)["fails"]
  assert not fails, "\n".join(fails[:20])


# (mutant, operation, the cases tried): compare() must reject it on at least one of them
def _cases(op, pred=lambda s, g: True):
  return [n for n, s in dc.CASES.items() if s["op"] == op and pred(s, dc.geometry(n))]


_cls0 = lambda c: (lambda s, g: g["cls"][0] == c)
MUTANTS = [
    ("no_lo", "fwd", lambda: _cases("fwd", lambda s, g: s["init"] == "split")),
    ("no_lo", "fused", lambda: _cases("fused")),
    ("no_flip", "fwd", lambda: _cases("fwd", lambda s, g: s["flip"] == 1)),
    ("no_flip", "fused", lambda: _cases("fused")),
    ("pad_off_by_one", "fwd", lambda: _cases("fwd")),
    ("pad_off_by_one", "wgrad", lambda: _cases("wgrad")),
    ("pad_off_by_one", "fused", lambda: _cases("fused")),
    ("drop_last_tap", "fwd", lambda: _cases("fwd")),
    ("drop_last_tap", "wgrad", lambda: _cases("wgrad")),
    ("read_dead_rows", "fwd", lambda: _cases("fwd", lambda s, g: s["ragged"])),
    ("read_dead_rows", "wgrad", lambda: _cases("wgrad", lambda s, g: s["ragged"])),
    ("drop_row_fwd_generic", "fwd", lambda: _cases("fwd", _cls0("generic"))),          # 128 steps
    ("drop_row_fwd_win", "fwd", lambda: _cases("fwd", _cls0("win"))),                  # 256
    ("drop_row_fwd_mfma", "fwd", lambda: _cases("fwd", _cls0("mfma"))),                # 32 nseg
    ("drop_row_wgrad_generic", "wgrad", lambda: _cases("wgrad", _cls0("generic"))),
    ("drop_row_wgrad_win", "wgrad", lambda: _cases("wgrad", _cls0("win"))),
    ("drop_row_wgrad_mfma", "wgrad", lambda: _cases("wgrad", _cls0("mfma"))),          # 928
    ("skip_last_group", "fwd", lambda: _cases("fwd")),
    ("skip_last_group", "wgrad", lambda: _cases("wgrad")),
    ("dil_taps", "fwd", lambda: _cases("fwd", lambda s, g: s["d"] > 1)),
    ("dil_taps", "wgrad", lambda: _cases("wgrad", lambda s, g: s["d"] > 1)),
    ("dw_overwrite", "wgrad", lambda: _cases("wgrad")),
    ("stats_unrounded", "fused", lambda: _cases("fused")),
    ("addend_after_mask", "fused", lambda: _cases("fused", lambda s, g: s["addend"] != "none")),
    ("no_mask_scale", "fused", lambda: _cases("fused", lambda s, g: s["scale"] != 1.0)),
    ("mask_ge", "fused", lambda: _cases("fused")),
    ("part_index", "fused", lambda: _cases("fused", lambda s, g: s["B"] * dc.ceil_div(s["T"], dc.fwd_tile(g["cls"], s["K"])) > s["B"])),
    ("dead_tile_stats", "fused", lambda: _cases("fused", lambda s, g: s["ragged"])),
]


@pytest.mark.parametrize("mutant,op,cases", MUTANTS, ids=["%s-%s" % m[:2] for m in MUTANTS])
def test_mutant_is_rejected(mutant, op, cases):
  names = cases()
  assert names
  rejected = []
  for name in names:
    if dc.check_case(name, Emu(mutant=mutant), log=_quiet)["fails"]:
      rejected.append(name)
      break
  assert rejected, "%s passes every one of %d cases" % (mutant, len(names))


def test_mutants_rejected_on_every_case_where_they_act():
  """The mutants whose effect does not depend on the data are rejected wherever they apply: a row dropped at the
  end of a tile at 128, 256, 32 nseg and 928 steps needs a case that HAS that row."""
  for mutant, op, cls0, tile in (("drop_row_fwd_generic", "fwd", "generic", lambda s, g: 128),
                                 ("drop_row_fwd_win", "fwd", "win", lambda s, g: 256),
                                 ("drop_row_fwd_mfma", "fwd", "mfma", lambda s, g: dc.dm_geom(s["K"])["tile"]),
                                 ("drop_row_wgrad_mfma", "wgrad", "mfma", lambda s, g: 928)):
    names = _cases(op, lambda s, g: g["cls"][0] == cls0 and s["T"] >= tile(s, g) and not s["olen"])
    assert len(names) >= 2, mutant
    for name in names[:3]:
      assert dc.check_case(name, Emu(mutant=mutant), log=_quiet)["fails"], (mutant, name)


# ---------------------------------------------------------------------------------------------------------
# the dispatcher's classes, from the formulas
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reached():
  out = set()
  for name, s in dc.CASES.items():
    out.add((s["op"],) + tuple(dc.geometry(name)["cls"]))
  return out


def test_every_dispatch_class_is_reached():
  need = set()
  for jt in range(3, 9):
    need |= {("fwd", "mfma", jt), ("fused", "mfma", jt), ("wgrad", "mfma", jt - 1)}
  need |= {("fwd", "win", d) for d in (1, 2, 4)}
  need |= {("fwd", "generic", "blocked"), ("fwd", "generic", "loop")}
  need |= {("wgrad", "win", 1, 8), ("wgrad", "win", 1, 2), ("wgrad", "win", 1, 1), ("wgrad", "win", 2, 4),
           ("wgrad", "win", 2, 2), ("wgrad", "win", 4, 8), ("wgrad", "win", 4, 4)}
  need |= {("wgrad", "generic", "blocked", n) for n in (4, 3, 1)}
  need |= {("wgrad", "generic", "loop", why) for why in ("nseg0", "cells", "dil3", "stride")}
  assert not need - _reached(), sorted(need - _reached())
  # the cases the issue names land where it says
  assert dc.wgrad_class(65, 1, 4) == ("generic", "loop", "nseg0") == dc.wgrad_class(129, 1, 2)
  assert dc.wgrad_class(257, 1, 1) == ("generic", "loop", "cells")
  assert [dc.wgrad_class(K, 1, 1, 0)[2] for K in (2, 33, 75, 129)] == [4, 4, 3, 1]
  assert [dc.wgrad_class(K, 1, d)[2] for K, d in ((39, 2), (87, 2), (20, 4), (64, 4))] == [4, 2, 8, 4]
  assert [dc.fwd_class(K, 1, 1) for K in (1, 97, 257)] == [("win", 1)] * 3
  assert [dc.fwd_class(K, 1, 1, 1) for K in (2, 33, 96)] == [("win", 1)] * 3
  assert dc.fwd_class(7, 1, 3) == dc.fwd_class(9, 2, 2) == ("generic", "loop")


def test_dead_tile_paths_are_reached():
  """Per kernel family: a tile skipped because it starts at or past out_len, a tile zero-filled because its whole
  input window lies past in_len (only where no out_len skips it first), a sample of length 0 and one of length 1;
  fused: a dead tile next to a live one of the same sample, and a whole dead sample."""
  hit = set()
  for name, s in dc.CASES.items():
    R = dc.make_inputs(name)
    cls0 = R["cls"][0]
    if s["op"] == "fwd" and R["in_len"] is not None and s["s"] == 1:
      Tt = dc.fwd_tile(R["cls"], s["K"])
      for b in range(s["B"]):
        hit.add((cls0, "len", min(int(R["in_len"][b]), 2)))
        for t0 in range(0, R["tout"], Tt):
          if R["out_len"] is not None and t0 >= int(R["out_len"][b]):
            hit.add((cls0, "skip"))
          elif t0 - R["padl"] >= int(R["in_len"][b]):
            hit.add((cls0, "zero-fill", "first" if t0 == 0 else "later"))
    if s["op"] == "wgrad" and R["in_len"] is not None and s["s"] == 1:
      Tt = dc.wgrad_tile(R["cls"])
      for b in range(s["B"]):
        if any(t0 - R["padl"] >= int(R["in_len"][b]) for t0 in range(0, R["tout"], Tt)):
          hit.add(("wgrad", cls0, "no contribution"))
    if s["op"] == "fused" and R["out_len"] is not None:
      Tt = dc.dm_geom(s["K"])["tile"]
      for b in range(s["B"]):
        dead = [t0 >= int(R["out_len"][b]) for t0 in range(0, R["tout"], Tt)]
        hit.add(("fused", "whole sample dead" if all(dead) else "dead after live" if any(dead) else "live"))
  need = {(c, "skip") for c in ("mfma", "win", "generic")}
  need |= {(c, "zero-fill", w) for c in ("mfma", "win") for w in ("first", "later")}
  need |= {(c, "len", n) for c in ("mfma", "win", "generic") for n in (0, 1, 2)}
  need |= {("wgrad", c, "no contribution") for c in ("mfma", "win", "generic")}
  need |= {("fused", "whole sample dead"), ("fused", "dead after live"), ("fused", "live")}
  assert not need - hit, sorted(need - hit)


def test_class_edges_sit_where_the_table_puts_them():
  # Jt = ceil((31 + K) / 16) and NT = (K + 30) / 16 change at 17|18 .. 81|82; nseg and the tile length with Jt
  edges = [K for K in range(2, 96) if dc.dm_geom(K)["Jt"] != dc.dm_geom(K + 1)["Jt"]]
  assert edges == [17, 33, 49, 65, 81] == [K for K in range(2, 96) if dc.mfma_wgrad_nt(K) != dc.mfma_wgrad_nt(K + 1)]
  assert all(K in dc.MF_K and K + 1 in dc.MF_K for K in edges) and {2, 96} <= set(dc.MF_K)
  assert [dc.dm_geom(K)["tile"] for K in (2, 18, 34, 50, 66, 82)] == [992, 992, 960, 960, 928, 928]
  assert [dc.dm_geom(K)["Jt"] for K in dc.FUSED_K] == [3, 4, 5, 6, 7, 8]
  for K in range(2, 97):
    g = dc.dm_geom(K)
    assert g["nchunk"] <= 128 and g["plane_bytes"] == 2176 and 32 * (g["nseg"] - 1) + 16 * g["Jt"] <= 1024
    assert g["nchunk"] * 8 <= 2 * 512                                   # kIt = 2 items per thread stage the window
    assert dc.ceil_div(g["tile"], 4) * 4 <= 2 * 512                     # and store it: the depth of the partial sums


def _last_supported(cls_of):
  K = 1
  while cls_of(K + 1) != ("unsupported",):
    K += 1
  assert all(cls_of(k) == ("unsupported",) for k in range(K + 1, K + 40))
  return K


def test_lds_limits():
  """The largest supported / smallest unsupported K of each 160 KB check."""
  # generic forward (variant 0) and what the default dispatch leaves to it
  assert _last_supported(lambda K: dc.fwd_class(K, 1, 1, 0)) == 233 == dc.UNSUPPORTED["fwd"]["K"] - 1
  assert dc.generic_fwd_lds(233, 1, 1) <= dc.LDS_MAX < dc.generic_fwd_lds(234, 1, 1)
  # register-window forward: the K at which the dispatcher hands over to the generic kernel, whose tile is too large
  for dil, last in ((1, 329), (2, 244), (4, 161)):
    assert dc.win_fwd_lds(last, dil) <= dc.LDS_MAX < dc.win_fwd_lds(last + 1, dil)
    assert _last_supported(lambda K: dc.fwd_class(K, 1, dil)) == last
  # generic weight gradient
  assert _last_supported(lambda K: dc.wgrad_class(K, 1, 1)) == 313 == dc.UNSUPPORTED["wgrad"]["K"] - 1
  assert dc.generic_wgrad_lds(313, 1, 1) <= dc.LDS_MAX < dc.generic_wgrad_lds(314, 1, 1)
  # checks that cannot fail: the matrix-core kernels and the register-window weight gradient
  assert max(dc.mfma_fwd_lds(K) for K in range(2, 97)) <= 80 * 1024 and dc.MFMA_WGRAD_LDS <= 80 * 1024
  assert min(dc.mfma_fwd_lds(K) for K in range(2, 97)) >= 512 * 16 * 4     # the fused store's reduction fits
  worst = max(dc.win_wgrad_geom(K, d)[2] for d in (1, 2, 4) for K in range(1, 400) if dc.win_wgrad_geom(K, d)[1] >= 1)
  assert worst == 102400
  # the LDS reductions that reuse tile memory fit their tiles
  for K in range(1, 257):
    nseg = dc.generic_wgrad_nseg(K)
    assert nseg * dc.ceil_div(K, 8) * 8 * 64 * 4 <= dc.generic_wgrad_lds(K, 1, 1)
  assert 8 * 16 * 112 * 4 + 96 * 16 * 4 <= dc.MFMA_WGRAD_LDS
  for name, key in (("fwd", "fwd"), ("wgrad", "wgrad")):
    u = dc.UNSUPPORTED[key]
    cls_of = dc.fwd_class if key == "fwd" else dc.wgrad_class
    assert cls_of(u["K"], u["stride"], u["dil"], u["variant"]) == ("unsupported",)
