"""Every kernel, instantiation, tiling and entry point of csrc/batchnorm.hip alone against the float64 oracle of
its own inputs (tests/_bn_cases.py: the case table, the bounds and their derivations). Every output is a view
into the middle of a larger allocation whose guard rows must keep their sentinel; rows a kernel may not read hold
NaN. Each test prints its largest error / bound per stage and output (BN-RATIO lines)."""
import contextlib
import functools
import math

import pytest
import torch

import _bn_cases as bc
from _bn_cases import ACT_ID, BF16, F32

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
FILL = 7.0          # what an output holds before the launch (a kernel that skips a store leaves it)


class Device:
  """The backend of _bn_cases.check_case on the GPU: CPU tensors in, CPU tensors out."""

  def __init__(self, dev):
    self.dev, self.fails = dev, []

  def up(self, t, dtype=None):
    if t is None:
      return None
    assert dtype is None or t.dtype == dtype, (t.dtype, dtype)
    return t.contiguous().to(self.dev)

  def guarded(self, shape, dtype, init=None):
    n = math.prod(shape)
    g = max(64, 2 * shape[-1])        # two rows before and after: 16-byte aligned for bf16 rows of C % 8 == 0
    buf = torch.full((g + n + g,), SENTINEL, dtype=dtype, device=self.dev)
    view = buf[g:g + n].view(shape)
    if init is None:
      view.fill_(FILL)
    else:
      view.copy_(init.to(self.dev))
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return (buf, g, n), view

  def down(self, what, guard, view):
    buf, g, n = guard
    host = buf.cpu()
    if not (bool((host[:g] == SENTINEL).all()) and bool((host[g + n:] == SENTINEL).all())):
      self.fails.append("%s: a guard row lost its sentinel" % what)
    return host[g:g + n].view(view.shape).clone()

  # ---- stages -------------------------------------------------------------------------------------------------
  def stats(self, y2d):
    from openseq2seq_amd import _lib, capi
    rows, C = y2d.shape
    n = int(_lib.C.os2s_bn_stats_num_parts(rows))
    assert n == -(-rows // bc.STATS_ROWS)
    gd, part = self.guarded((n, 2, C), F32)
    _lib.C.os2s_bn_stats(capi._stream(), capi._ptr(self.up(y2d, BF16), BF16), rows, C, capi._ptr(part, F32))
    return self.down("bn_stats partial", gd, part)

  def _finalize_item(self, partial, count, gamma, beta, eps, momentum, training, moving_mean, moving_var,
                     want_stats=True):
    C = (gamma if gamma is not None else moving_mean if moving_mean is not None else partial[0, 0]).numel()
    it, guards = dict(partial=self.up(partial, F32), gamma=self.up(gamma, F32), beta=self.up(beta, F32)), {}
    for k, init in (("moving_mean", moving_mean), ("moving_var", moving_var), ("mean_out", None), ("rstd_out", None),
                    ("scale_out", None), ("shift_out", None)):
      if (k.startswith("moving") and init is None) or (k in ("mean_out", "rstd_out") and not want_stats):
        it[k] = None
      else:
        guards[k], it[k] = self.guarded((C,), F32, init)
    return it, guards

  def _finalize_result(self, what, it, guards):
    o = {k: (self.down("%s %s" % (what, k), guards[k], it[k]) if it[k] is not None else None)
         for k in ("moving_mean", "moving_var", "mean_out", "rstd_out", "scale_out", "shift_out")}
    return dict(mean=o["mean_out"], rstd=o["rstd_out"], scale=o["scale_out"], shift=o["shift_out"],
                moving_mean=o["moving_mean"], moving_var=o["moving_var"])

  def finalize(self, **kw):
    from openseq2seq_amd import capi
    it, guards = self._finalize_item(**kw)
    capi.bn_finalize(it["partial"], kw["count"], it["gamma"], it["beta"], kw["eps"], kw["momentum"], kw["training"],
                     it["moving_mean"], it["moving_var"], it["mean_out"], it["rstd_out"], it["scale_out"],
                     it["shift_out"])
    return self._finalize_result("bn_finalize", it, guards)

  def finalize_multi(self, items):
    from openseq2seq_amd import capi
    built = [self._finalize_item(**kw) for kw in items]
    capi.bn_finalize_multi([it for it, _ in built], items[0]["count"], items[0]["eps"], items[0]["momentum"],
                           items[0]["training"])
    return [self._finalize_result("bn_finalize_multi", it, guards) for it, guards in built]

  def dropout_mask(self, seed, shape, keep):
    from openseq2seq_amd import capi
    return capi.dropout_mask(seed, math.prod(shape), keep, self.dev).reshape(shape).cpu()

  def lens(self, lens):
    return None if lens is None else lens.to(torch.int32).to(self.dev)

  def act_fwd(self, ys, scales, shifts, lens, act, keep, seed):
    from openseq2seq_amd import capi
    gd, out = self.guarded(tuple(ys[0].shape), BF16)
    capi.bn_act_fwd([self.up(y, BF16) for y in ys], [self.up(s, F32) for s in scales],
                    [self.up(s, F32) for s in shifts], out, self.lens(lens), ACT_ID[act], keep, seed)
    return self.down("bn_act_fwd out", gd, out)

  def reduce(self, dout, out, ys, means, rstds, lens, act, keep, seed, n):
    from openseq2seq_amd import capi
    B, T, C = dout.shape
    nparts = capi.bn_act_bwd_num_parts(B * T)
    assert nparts == -(-(B * T) // n), (nparts, n)         # follows the reduce tiling in force
    gz, dz = self.guarded((B, T, C), BF16)
    gp, part = self.guarded((nparts, 1 + len(ys), C), F32)
    capi.bn_act_bwd_reduce(self.up(dout, BF16), self.up(out, BF16), [self.up(y, BF16) for y in ys],
                           [self.up(m, F32) for m in means], [self.up(r, F32) for r in rstds], dz, part,
                           self.lens(lens), ACT_ID[act], keep, seed)
    return self.down("bn_act_bwd_reduce dz", gz, dz), self.down("bn_act_bwd_reduce partial", gp, part)

  def bwd_finalize(self, partial, q, count, pre_dgamma, pre_dbeta, accumulate, mean=None, rstd=None):
    from openseq2seq_amd import capi
    C = partial.shape[2]
    g, t = {}, {}
    for k, init in (("dgamma", pre_dgamma), ("dbeta", pre_dbeta), ("c1", None), ("c2", None)):
      g[k], t[k] = (None, None) if (k[0] == "d" and init is None) else self.guarded((C,), F32, init)
    if mean is None:
      capi.bn_bwd_finalize(self.up(partial, F32), q, count, t["dgamma"], t["dbeta"], bool(accumulate), t["c1"], t["c2"])
    else:
      assert q == 1 and partial.shape[1] == 2
      capi.bn_bwd_finalize_raw(self.up(partial, F32), count, self.up(mean, F32), self.up(rstd, F32), t["dgamma"],
                               t["dbeta"], bool(accumulate), t["c1"], t["c2"])
    return {k: (None if t[k] is None else self.down("bn_bwd_finalize %s" % k, g[k], t[k])) for k in t}

  def bwd_finalize_multi(self, partial, count, pres_dg, pres_db, accumulate):
    from openseq2seq_amd import capi
    J, C = len(pres_dg), partial.shape[2]
    gs = [[(None, None) if p is None else self.guarded((C,), F32, p) for p in pres] for pres in (pres_dg, pres_db)]
    g1, c1 = self.guarded((J, C), F32)
    g2, c2 = self.guarded((J, C), F32)
    capi.bn_bwd_finalize_multi(self.up(partial, F32), count, [t for _, t in gs[0]], [t for _, t in gs[1]],
                               bool(accumulate), c1, c2)
    c1, c2 = self.down("bn_bwd_finalize_multi c1", g1, c1), self.down("bn_bwd_finalize_multi c2", g2, c2)
    get = lambda gt, k: None if gt[1] is None else self.down("bn_bwd_finalize_multi %s" % k, gt[0], gt[1])
    return [dict(dgamma=get(gs[0][j], "dgamma"), dbeta=get(gs[1][j], "dbeta"), c1=c1[j], c2=c2[j]) for j in range(J)]

  def apply(self, dz, y, gamma, mean, rstd, c1, c2, lens, margin, dz_to_len):
    from openseq2seq_amd import capi
    gd, dy = self.guarded(tuple(dz.shape), BF16)
    capi.bn_bwd_apply(self.up(dz, BF16), self.up(y, BF16), self.up(gamma, F32), self.up(mean, F32),
                      self.up(rstd, F32), self.up(c1, F32), self.up(c2, F32), dy, out_len=self.lens(lens),
                      margin=margin, dz_to_len=dz_to_len)
    return self.down("bn_bwd_apply dy", gd, dy)


@contextlib.contextmanager
def tiling(t):
  """bn.<kernel>.groups / .rows of the three tiled kernels; the defaults come back whatever happens."""
  from openseq2seq_amd import _lib
  try:
    for k in bc.KERNELS:
      _lib.set_option("bn.%s.groups" % k, t[0])
      _lib.set_option("bn.%s.rows" % k, t[1])
    yield
  finally:
    for k, (g, r) in zip(bc.KERNELS, bc.DEFAULT_TILING):
      _lib.set_option("bn.%s.groups" % k, g)
      _lib.set_option("bn.%s.rows" % k, r)


def _run(name, dev, n=bc.DEFAULT_TILING[1][1], tag=None):
  bc.check_inputs(name)                      # host-only conditions first (the relu20 cap fraction)
  be = Device(dev)
  res = bc.check_case(name, be, n=n, tag=tag)
  res["fails"] = res["fails"] + ["%s %s" % (tag or name, f) for f in be.fails]
  return res


@functools.lru_cache(maxsize=None)
def _default(name, dev):
  return _run(name, dev)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_case(cuda, name):
  res = _default(name, cuda)
  assert not res["fails"], "\n".join(res["fails"])


@pytest.mark.parametrize("t", bc.TILINGS, ids=lambda t: "g%d_r%d" % t)
@pytest.mark.parametrize("name", bc.TILED_CASES)
def test_tiling(cuda, name, t):
  from openseq2seq_amd import capi
  ref = _default(name, cuda)
  R = bc.make_inputs(name)
  rows = R["B"] * R["T"]
  with tiling(t):
    assert capi.bn_act_bwd_num_parts(rows) == -(-rows // t[1])
    res = _run(name, cuda, n=t[1], tag="%s@g%d_r%d" % ((name,) + t))
    be = Device(cuda)
    dys = [be.apply(**inp) for inp in ref["dense"]]       # the default run's dz, c1, c2 under this tiling
  assert capi.bn_act_bwd_num_parts(rows) == -(-rows // bc.DEFAULT_TILING[1][1])
  assert not res["fails"], "\n".join(res["fails"])
  assert not be.fails, be.fails
  # element-wise outputs do not depend on the tiling (dy: on the same c1 / c2; this run's own come from partials
  # summed over other tiles and differ in the last bits)
  assert torch.equal(res["out"].view(torch.int16), ref["out"].view(torch.int16))
  assert torch.equal(res["dz"].view(torch.int16), ref["dz"].view(torch.int16))
  assert len(dys) == len(ref["dys"])
  for j, (a, b) in enumerate(zip(dys, ref["dys"])):
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), j
  if name == "rows1050" and t[1] == 8:
    assert res["nparts"] == 132               # the device's own partials reach the second trip of fin_sum_pair


@pytest.mark.parametrize("nparts", bc.FIN_NPARTS)
def test_finalize_handmade(cuda, nparts):
  fails = []
  for C in bc.FIN_C:
    be = Device(cuda)
    res = bc.check_finalize_handmade(nparts, C, be)
    fails += res["fails"] + be.fails
  assert not fails, "\n".join(fails)
