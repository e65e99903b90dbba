"""Side streams: where work that may overlap the main stream is enqueued.

Parameter-gradient kernels (nothing in the rest of a backward pass reads their result) and the dense-residual chains
run next to the main stream's kernels; `on_side_stream` forks onto a side stream, `join_side_streams` makes the
current stream wait for them. The reverse-mode tape that joins at both ends of a pass is parts/tape.py.

Every name here has this module as its only home: other modules reach the state and the functions as
`streams.<name>` (a rebinding of `streams.join_side_streams` takes effect everywhere).
"""
import os

import torch

from .. import capi

_SIDE_STREAMS = {}

# A/B knob: 0 = the dense-residual chains share the weight-gradient side stream (FIFO behind its backlog)
DRES_OWN_STREAM = os.environ.get("OS2S_DRES_OWN_STREAM", "1") != "0"

_SIDE_STREAM_ENABLED = True
# set while two half-batches of ONE step run on two main streams (backward_interleaved): both share the side streams
# of the step's own stream — parameter gradients accumulate into the same buffers, one FIFO keeps them in order
_SIDE_KEY_OVERRIDE = None


def set_side_key_override(key):
  """`key` (a raw stream handle) replaces the current stream in the side streams' cache key until None is set:
  the half-batches of one step (tape.backward_interleaved) run on streams of their own and share the side streams of
  the step's stream."""
  global _SIDE_KEY_OVERRIDE
  _SIDE_KEY_OVERRIDE = key


def set_side_stream_enabled(on):
  """Per-model switch (config key `os2s_side_stream`, set at the start of every train step): with False
  every `on_side_stream` body runs on the current stream. Returns the previous setting (the caller
  restores it when its step is over)."""
  global _SIDE_STREAM_ENABLED
  prev, _SIDE_STREAM_ENABLED = _SIDE_STREAM_ENABLED, bool(on)
  return prev


def _side_stream(device, which=0):
  """Side stream for work that may overlap the main stream inside one backward closure
  (OS2S_WGRAD_STREAM=0 or the model's `os2s_side_stream: False` keeps everything on one stream).
  which: 0 = the parameter-gradient stream (nothing on the main stream waits for it before the end of the pass),
  1 = the stream of side work the main stream DOES wait for (the dense-residual chains): a stream is a FIFO, a
  chain queued behind a backlog of weight-gradient kernels would stall the main stream until the backlog drained."""
  if not _SIDE_STREAM_ENABLED or os.environ.get("OS2S_WGRAD_STREAM", "1") == "0" or device.type != "cuda":
    return None
  if which == 1 and not DRES_OWN_STREAM:
    which = 0
  base = _SIDE_KEY_OVERRIDE if _SIDE_KEY_OVERRIDE is not None else capi._stream().value
  key = (device.index, base) if not which else (device.index, base, which)
  st = _SIDE_STREAMS.get(key)
  if st is None:
    # OS2S_SIDE_PRIO (experiment): stream priority of the side stream (HIP: lower number = higher
    # priority; the main stream has 0)
    prio = int(os.environ.get("OS2S_DRES_PRIO" if which else "OS2S_SIDE_PRIO", "0"))
    st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=device, priority=prio)
  return st


_STREAM_OBJ = {}       # raw stream handle -> torch.cuda.Stream (torch.cuda.current_stream() builds a new object: 7 us)
_FORK_EVENT = {}       # side stream -> the event its forks are ordered by (re-recorded per use: a wait captures the
                       # record that precedes it)


def _current_stream_obj():
  raw = capi._stream().value
  st = _STREAM_OBJ.get(raw)
  if st is None:
    st = _STREAM_OBJ[raw] = torch.cuda.current_stream()
  return st


class on_side_stream(object):
  """`with on_side_stream(device, *operands):` enqueues the body on the side stream, ordered
  after everything the current stream has enqueued so far. For parameter-gradient kernels:
  nothing in the rest of backward reads their result, the main stream re-joins at the end of
  `Tape.backward` and the gradient reducer waits for the side stream itself. `operands` are the
  tensors the body reads that the main stream's closures release afterwards (their memory is kept
  until the side stream is done). With OS2S_WGRAD_STREAM=0 the body runs on the current stream.
  (Host cost matters here — QuartzNet's step is bound by the Python thread, and this context is entered ~250 times
  per step: cached stream objects, one re-recorded event per side stream and torch.cuda.set_stream instead of
  current_stream() / wait_stream() / the torch.cuda.stream context manager: ~35 -> ~10 us per use.)"""

  def __init__(self, device, *operands, which=0):
    self.side = _side_stream(device, which)
    self.operands = operands
    self.main = None

  def __enter__(self):
    if self.side is not None:
      self.main = _current_stream_obj()
      ev = _FORK_EVENT.get(self.side)
      if ev is None:
        ev = _FORK_EVENT[self.side] = torch.cuda.Event()
      ev.record(self.main)
      self.side.wait_event(ev)
      torch.cuda.set_stream(self.side)
    return self

  def __exit__(self, *exc):
    if self.side is not None:
      torch.cuda.set_stream(self.main)
      for t in self.operands:
        if t is not None:
          t.record_stream(self.side)
    return False

  def hand_over(self, *tensors):
    """Tensors ALLOCATED inside the body (side-stream allocations) that the main stream consumes
    after it has joined: their memory must not be recycled for later side-stream allocations while
    main-stream kernels still use them."""
    if self.side is not None:
      for t in tensors:
        if t is not None:
          t.record_stream(self.main)


def side_streams():
  return list(_SIDE_STREAMS.values())


_JOIN_EVENT = {}


def join_side_streams():
  """The current stream waits for everything enqueued on the side streams so far."""
  if _SIDE_STREAMS:
    cur = _current_stream_obj()
    for st in _SIDE_STREAMS.values():
      ev = _JOIN_EVENT.get(st)
      if ev is None:
        ev = _JOIN_EVENT[st] = torch.cuda.Event()
      ev.record(st)
      cur.wait_event(ev)
