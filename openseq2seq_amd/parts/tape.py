"""The reverse-mode engine every model family is built on: Tape, Act and their helpers.

There is no graph compiler here: a layer object owns its parameters, `forward` enqueues the kernels and records one
backward closure on a Tape; `Tape.backward` replays them in reverse. `Act` is an activation tensor with its valid
lengths and (in training) its gradient. Side-stream ordering is parts/streams.py; the layers that record closures
are parts/cnns, parts/rnns, parts/transformer, parts/tacotron.
"""
import os

import torch

from .. import capi
from . import streams
from .streams import _current_stream_obj, on_side_stream

# how many small Dense weight gradients (Transformer: the 1024 x 1024 projections, 16 tiles each) share one launch
SMALL_WGRAD_GROUP = int(os.environ.get("OS2S_SMALL_WGRAD_GROUP", "3"))
# Round 6: convolution weight gradients of same-shape layers CAN be collected until they cover this many units of the
# ping-pong kernel (128 co x 128 ci x 4 taps each; 256 CUs) and go out as one launch (Tape.defer_conv_wgrad,
# os2s_conv1d_wgrad_grouped_ws). Alone on the GPU the grouped launches save the reduction splits of the 256 - 640
# channel layers; in the Jasper step — where the weight gradients run next to the data-gradient chain — holding them
# back costs what it saves: 37.15 / 37.31 ms without, 37.1 - 37.3 at 64 - 128 units, 37.4 - 38.0 at 160 - 192
# (same box, interleaved). 0 (default) = every layer alone, as in rounds 2 - 5.
CONV_WGRAD_UNIT_BUDGET = int(os.environ.get("OS2S_CONV_WGRAD_UNIT_BUDGET", "0"))


class Tape(object):
  """Reverse-mode tape. `record(fn, params)` also notes which parameters the closure writes
  gradients of. A parameter is FINAL once every closure that lists it has run; after each
  closure `on_done(w)` tells the data-parallel reducer the watermark w: every parameter at a flat
  offset >= w is final (parameters no closure lists receive no gradient), so complete gradient
  buckets above it can be all-reduced while the rest of backward runs. Variables are created in
  forward order, so the watermark normally falls with every closure; a variable used out of
  creation order (a tied embedding, say) only delays it."""

  def __init__(self, on_done=None):
    self.ops = []
    self.on_done = on_done
    # True: backward() leaves the closures (and the activations they hold) to the caller, who drops them AFTER it has
    # enqueued what follows the pass — releasing a step's few thousand tensors takes the host ~0.5 ms, during which
    # the GPU (which has caught up with the host by the end of backward) would wait for the optimizer launch
    self.defer_free = False
    self._deferred_side = True
    self._begin_pass()

  def _begin_pass(self):
    # the held-back (grouped) weight gradients and, with a gradient reducer, the closures still to run per parameter
    self._deferred, self._pending = [], None
    self._cdeferred, self._ckey = [], None

  def record(self, fn, params=()):
    self.ops.append((fn, params))

  def backward(self):
    # Re-entrant: a closure may run another tape's backward pass (a nested pass gets the zeroed scratch arena
    # of its own depth — capi.zero_arena_enter — and its own deferred-gradient list; `current_tape()` is the
    # innermost pass). Work parked on the side streams since the last join must have landed first.
    depth = len(_TAPE_STACK)
    streams.join_side_streams()
    capi.zero_arena_enter(depth)   # the previous pass's statistic partials at this depth are dead: one fill
    _TAPE_STACK.append(self)
    self._begin_pass()
    try:
      if self.on_done is None:
        for fn, _ in reversed(self.ops):
          fn()
        self.flush_deferred()
        self.flush_conv_wgrads()
      else:
        pending, by_id = {}, {}
        for _, params in self.ops:
          for p in params:
            pending[id(p)] = pending.get(id(p), 0) + 1
            by_id[id(p)] = p
        self._pending = pending
        order = sorted(by_id.values(), key=lambda p: -p.offset)
        ptr = 0

        def advance():
          nonlocal ptr
          moved = False
          while ptr < len(order) and pending[id(order[ptr])] == 0:
            ptr += 1
            moved = True
          if moved:
            self.on_done(order[ptr - 1].offset)

        for fn, params in reversed(self.ops):
          fn()
          if params:
            for p in params:
              pending[id(p)] -= 1
            advance()
        if self._deferred or self._cdeferred:
          self.flush_deferred()
          self.flush_conv_wgrads()
          advance()
    finally:
      _TAPE_STACK.pop()
      capi.zero_arena_leave(depth)
    if not self.defer_free:
      self.ops = []
    streams.join_side_streams()

  # ---- deferred (grouped) weight gradients -----------------------------------------------------
  def defer_wgrad(self, param, item, group=None, unit_budget=None, side=True):
    """A Dense weight gradient too small to fill the chip alone is held back until `group` of them — or, with
    `unit_budget`, enough of them to cover that many 256 x 256 output tiles — can go out in one launch
    (capi.gemm_wgrad_grouped: at most 16 per launch). Until then `param` does not count as final for the
    gradient reducer. Optional keys of `item`: `after` — a callable run behind the grouped launch, on its stream (a
    folded one-tap separable layer splits its product into two variables' gradients there); `also` — further
    parameters that become final with that launch."""
    # one grouped launch has ONE row count (os2s_gemm_wgrad_grouped takes a single M): a layer fed by
    # another number of packed rows (the enc-dec attention's k/v projection of the SOURCE tokens among
    # target-row layers) starts a new group
    if self._deferred and self._deferred[0][1]["x"].shape[0] != item["x"].shape[0]:
      self.flush_deferred()
    self._deferred.append((param, item))
    self._deferred_side = side        # False: the grouped launch stays on the current stream (serial profiles)
    if self._pending is not None:
      for q in (param,) + tuple(item.get("also", ())):
        if id(q) in self._pending:
          self._pending[id(q)] += 1
    if unit_budget is not None:
      units = sum(((it["dy"].shape[1] + 255) // 256) * ((it["x"].shape[1] + 255) // 256) for _, it in self._deferred)
      if units >= unit_budget or len(self._deferred) >= 16:
        self.flush_deferred()
    elif len(self._deferred) >= (group if group is not None else SMALL_WGRAD_GROUP):
      self.flush_deferred()

  def defer_conv_wgrad(self, param, key, item, units, launch_kw):
    """The weight gradient of a convolution layer is held back while layers of the SAME shape over the same batch
    follow (the `repeat` sub-blocks of a Jasper block: 12 - 150 units of work each for 256 CUs): they go out as one
    launch of the ping-pong kernel (capi.conv1d_wgrad_grouped, at most 8) once CONV_WGRAD_UNIT_BUDGET units are
    collected, when a layer of another shape arrives, or at the end of the pass. `param` is not final for the
    gradient reducer until then."""
    if self._cdeferred and self._ckey != key:
      self.flush_conv_wgrads()
    self._ckey, self._ckw = key, launch_kw
    self._cdeferred.append((param, item))
    if self._pending is not None and id(param) in self._pending:
      self._pending[id(param)] += 1
    if units * len(self._cdeferred) >= CONV_WGRAD_UNIT_BUDGET or len(self._cdeferred) >= 8:
      self.flush_conv_wgrads()

  def flush_conv_wgrads(self):
    if not self._cdeferred:
      return
    items = [it for _, it in self._cdeferred]
    with on_side_stream(items[0]["x"].device, *([it["x"] for it in items] + [it["dy"] for it in items])):
      capi.conv1d_wgrad_grouped(items, **self._ckw)
    if self._pending is not None:
      for p, _ in self._cdeferred:
        if id(p) in self._pending:
          self._pending[id(p)] -= 1
    self._cdeferred, self._ckey = [], None

  def flush_deferred(self):
    if not self._deferred:
      return
    items = [it for _, it in self._deferred]

    def launch():
      capi.gemm_wgrad_grouped(items, accumulate=True)
      for it in items:
        if "after" in it:       # behind the launch, on its stream (a folded one-tap separable layer splits its dw)
          it["after"]()
    if self._deferred_side:
      with on_side_stream(items[0]["x"].device, *([it["x"] for it in items] + [it["dy"] for it in items] +
                                                  [it["dw"] for it in items if "after" in it])):
        launch()
    else:
      launch()
    if self._pending is not None:
      for p, it in self._deferred:
        for q in (p,) + tuple(it.get("also", ())):
          if id(q) in self._pending:
            self._pending[id(q)] -= 1
    self._deferred = []


_TAPE_STACK = []


def backward_interleaved(tapes, main_streams):
  """Tape.backward for several tapes of the SAME structure (the halves of one batch) on several streams: closure i
  of every tape is issued before closure i + 1 of any, each on its tape's stream — the kernels of one half that keep
  the matrix pipes idle (LayerNorm, attention, dropout, embedding) run under the other half's GEMMs. The caller has
  set the side-key override (streams.set_side_key_override): parameter-gradient launches of all tapes queue on one side
  stream. Single-process only (no gradient reducer watermark)."""
  depth = len(_TAPE_STACK)
  streams.join_side_streams()
  capi.zero_arena_enter(depth)
  for t in tapes:
    assert t.on_done is None
    t._begin_pass()
  outer = torch.cuda.current_stream()
  try:
    n = max(len(t.ops) for t in tapes)
    for i in range(n):
      for t, st in zip(tapes, main_streams):
        if i < len(t.ops):
          fn = t.ops[len(t.ops) - 1 - i][0]
          _TAPE_STACK.append(t)
          torch.cuda.set_stream(st)
          try:
            fn()
          finally:
            _TAPE_STACK.pop()
    for t, st in zip(tapes, main_streams):
      _TAPE_STACK.append(t)
      torch.cuda.set_stream(st)
      try:
        t.flush_deferred()
        t.flush_conv_wgrads()
      finally:
        _TAPE_STACK.pop()
  finally:
    torch.cuda.set_stream(outer)
    capi.zero_arena_leave(depth)
  for t in tapes:
    t.ops = []
  for st in main_streams:
    outer.wait_stream(st)
  streams.join_side_streams()


def current_tape():
  """The tape whose backward pass is running — the innermost one (None outside Tape.backward)."""
  return _TAPE_STACK[-1] if _TAPE_STACK else None


class Act(object):
  """An activation tensor + its valid lengths + (optionally) its gradient."""
  __slots__ = ("data", "lens", "grad", "grad_init", "requires_grad", "res_grad", "mask_scale",
               "grad_masked", "bias_part", "bn_y", "bn_scale", "grad_event", "bn_full_rows")

  def __init__(self, data, lens=None, requires_grad=True):
    self.data, self.lens = data, lens
    self.grad, self.grad_init = None, False
    self.requires_grad = requires_grad
    self.res_grad = None   # gradient arriving through a residual connection (pre-norm blocks)
    # set by a ReLU (+ dropout) Dense layer on its OUTPUT: the consumer's data-gradient GEMM may
    # apply (data > 0) * mask_scale in its epilogue (and leave the bias-gradient partials in
    # bias_part); it then sets grad_masked and the producer skips its own activation backward
    self.mask_scale = None
    self.grad_masked = False
    self.bias_part = None
    # set by conv_bn_actv on the output of a single-input conv + BatchNorm + ReLU (+ dropout) layer: the
    # convolution output y. The data gradient of the NEXT layer's main convolution — the last
    # contribution to this activation's gradient — then applies the ReLU / dropout backward and leaves
    # the BatchNorm-backward partials (sum dz, sum dz * y) in bias_part (capi.conv1d_dgrad_bnact)
    self.bn_y = None
    self.bn_scale = 1.0
    # the producer's backward reads EVERY row of the finalised gradient (separable layers: their BatchNorm-backward
    # apply pass is not ragged): only a consumer that defines all rows may finalise it
    self.bn_full_rows = False
    # set by a data-gradient contribution enqueued on the SIDE stream (dense_residual.backward_end): the next
    # writer or reader of the gradient on another stream waits for it first
    self.grad_event = None

  def wait_grad(self):
    if self.grad_event is not None:
      _current_stream_obj().wait_event(self.grad_event)
      self.grad_event = None

  def grad_buffer(self):
    # a gradient that already carries its producer's activation backward takes no more addends
    assert not self.grad_masked, "a second consumer wrote to an activation whose gradient was finalised"
    if self.grad_event is not None:
      self.wait_grad()
    if self.grad is None:
      self.grad = torch.empty_like(self.data)
      self.grad_init = False
    return self.grad


def accumulate_grad(x, g):
  """x.grad (+)= g for an Act consumed by several ops."""
  if not x.requires_grad:
    return
  if x.grad_init and x.grad is not None:
    capi.add_bf16(x.grad, g, out=x.grad)
  else:
    x.grad, x.grad_init = g, True


def reshape_act(x, shape, tape, lens=None):
  """A view of an Act with another shape ([B,T,C] <-> [B*T,C]); gradients flow back."""
  v = Act(x.data.view(*shape), lens, requires_grad=x.requires_grad)
  if tape is not None and x.requires_grad:
    def backward():
      if v.grad is not None:
        accumulate_grad(x, v.grad.reshape(x.data.shape))
      v.grad = None
    tape.record(backward)
  return v
