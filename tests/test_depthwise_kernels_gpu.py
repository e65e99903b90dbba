"""Every kernel and dispatch class of csrc/depthwise.hip alone against the float64 oracle of its own inputs
(tests/_dw_cases.py: the case table, the bounds and their derivations). dw and dx are views into the middle of a
larger allocation whose guard rows must keep their sentinel; rows of x a kernel may not read hold NaN. Each case
prints its largest error / bound per output, the last test one DW-RATIO line per stage over all cases."""
import math

import pytest
import torch

import _dw_cases as dc
from _dw_cases import BF16, F32

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
FILL = 7.0          # what an output holds before the launch (a kernel that skips a store leaves it)
RATIOS = {}


class Device:
  """The backend of _dw_cases.check_case on the GPU: CPU tensors in, CPU tensors out."""

  def __init__(self, dev):
    self.dev, self.fails = dev, []

  def up(self, t, dtype):
    if t is None:
      return None
    assert t.dtype == dtype, (t.dtype, dtype)
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

  def num_parts(self, B, tout, K):
    from openseq2seq_amd import _lib
    return int(_lib.C.os2s_depthwise_dgrad_bnact_num_parts(B, tout, K))

  def fwd(self, x, w, in_len, out_len, tout, stride, dil, pad_left, flip, variant):
    from openseq2seq_amd import _lib, capi
    try:
      _lib.set_option("depthwise.variant", variant)
      y = capi.depthwise_conv1d_fwd(self.up(x, BF16), self.up(w, F32), stride=stride, dil=dil, pad_left=pad_left,
                                    tout=tout, in_len=self.up(in_len, torch.int32),
                                    out_len=self.up(out_len, torch.int32), flip=bool(flip))
    finally:
      _lib.set_option("depthwise.variant", -1)
    return y.cpu()

  def wgrad(self, x, dy, dw0, in_len, stride, dil, pad_left, variant, det):
    from openseq2seq_amd import _lib, capi
    gd, dw = self.guarded(tuple(dw0.shape), F32, dw0)
    was = capi.deterministic()
    try:
      _lib.set_option("depthwise.variant", variant)
      capi.set_deterministic(det)
      capi.depthwise_conv1d_wgrad(self.up(x, BF16), self.up(dy, BF16), dw, stride=stride, dil=dil, pad_left=pad_left,
                                  in_len=self.up(in_len, torch.int32))
    finally:
      capi.set_deterministic(was)
      _lib.set_option("depthwise.variant", -1)
    return self.down("depthwise_conv1d_wgrad dw", gd, dw)

  def fused(self, dz, w, addend, alias, mask_ref, stat_ref, out_len, pad_left, mask_scale):
    from openseq2seq_amd import capi
    gd, dx = self.guarded(tuple(mask_ref.shape), BF16, addend if alias else None)
    ad = dx if alias else self.up(addend, BF16)
    stats = capi.depthwise_dgrad_bnact(self.up(dz, BF16), self.up(w, F32), dx, pad_left=pad_left,
                                       out_len=self.up(out_len, torch.int32), mask_ref=self.up(mask_ref, BF16),
                                       mask_scale=mask_scale, stat_ref=self.up(stat_ref, BF16), addend=ad)
    return self.down("depthwise_dgrad_bnact dx", gd, dx), stats.cpu()


def _names(op):
  return [n for n, s in dc.CASES.items() if s["op"] == op]


def _case(name, dev):
  be = Device(dev)
  res = dc.check_case(name, be)
  for k, v in res["ratios"].items():
    RATIOS[k] = max(RATIOS.get(k, 0.0), v)
  fails = res["fails"] + ["%s %s" % (name, f) for f in be.fails]
  assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", _names("fwd"))
def test_forward(cuda, name):
  _case(name, cuda)


@pytest.mark.parametrize("name", _names("wgrad"))
def test_weight_gradient(cuda, name):
  _case(name, cuda)


@pytest.mark.parametrize("name", _names("fused"))
def test_fused_data_gradient(cuda, name):
  _case(name, cuda)


def test_unsupported_tiles_raise_and_launch_nothing(cuda):
  """The smallest K whose generic tile exceeds 160 KB: the binding raises and the output keeps what it held."""
  from openseq2seq_amd import _lib, capi
  B, T, C = 2, 37, 8
  x = torch.zeros(B, T, C, dtype=BF16, device=cuda)
  for op in ("fwd", "wgrad"):
    u = dc.UNSUPPORTED[op]
    K = u["K"]
    pad = dc.same_padding(T, K, 1, 1)[1]
    try:
      _lib.set_option("depthwise.variant", u["variant"])
      with pytest.raises(_lib.Os2sError):
        if op == "fwd":
          out = torch.full((B, T, C), FILL, dtype=BF16, device=cuda)
          w = torch.ones(K, C, dtype=F32, device=cuda)
          _lib.C.os2s_depthwise_conv1d_fwd(capi._stream(), capi._ptr(x, BF16), capi._ptr(w, F32), capi._ptr(out, BF16),
                                           None, None, B, T, T, C, K, 1, 1, pad, 0)
        else:
          out = torch.full((K, C), FILL, dtype=F32, device=cuda)
          capi.depthwise_conv1d_wgrad(x, x, out, pad_left=pad)
    finally:
      _lib.set_option("depthwise.variant", -1)
    torch.cuda.synchronize()
    assert bool((out == FILL).all()), op


def test_zz_report(cuda):
  """One line per stage: the largest error / bound over all cases of this run."""
  stages = {}
  for k, v in RATIOS.items():
    stages.setdefault(k.split(".")[0], []).append("%s %.3g" % (k.split(".", 1)[1], v))
  for st in sorted(stages):
    print("DW-RATIO %-6s %s" % (st, "   ".join(sorted(stages[st]))))
  assert all(v <= 1.0 for v in RATIOS.values()), RATIOS
