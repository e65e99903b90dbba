"""capi._ZeroArena (the per-backward-pass zeroed scratch for BatchNorm-backward statistic partials):
every slice handed out reads as zeros, slices of one pass never overlap, and reset() re-zeroes what the
previous pass dirtied. Host logic only (CPU tensors)."""
import torch


def test_zero_arena_hands_out_disjoint_zeroed_slices():
  from openseq2seq_amd.capi import _ZeroArena
  dev = torch.device("cpu")
  arena = _ZeroArena()
  arena.reset()                                   # nothing known yet: a no-op
  shapes = [(7, 2, 24), (3, 2, 1024), (1, 2, 8)]
  first = [arena.take(s, dev) for s in shapes]    # before the first reset: plain zero tensors
  assert arena.buf is None and all(float(t.abs().sum()) == 0.0 and tuple(t.shape) == s for t, s in zip(first, shapes))
  arena.reset()                                   # sized to the demand of that pass
  assert arena.buf is not None and arena.buf.numel() >= sum(t.numel() for t in first)
  for rounds in range(2):
    got = [arena.take(s, dev) for s in shapes]
    for t, s in zip(got, shapes):
      assert tuple(t.shape) == s and float(t.abs().sum()) == 0.0
      assert t.data_ptr() >= arena.buf.data_ptr() and t.data_ptr() < arena.buf.data_ptr() + arena.buf.numel() * 4
    spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * 4) for t in got)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))     # disjoint
    for t in got:
      t.fill_(3.0)                                                  # a pass writes its partials
    arena.reset()
  # a pass that needs more than the buffer holds falls back to fresh zeros and grows the buffer next time
  big = arena.take((64, 2, 4096), dev)
  assert float(big.abs().sum()) == 0.0
  arena.reset()
  assert arena.buf.numel() >= big.numel()


def test_tape_backward_nests_with_an_arena_per_depth():
  """Tape.backward is re-entrant (product hygiene): a pass started from inside a closure of
  another one takes its zeroed scratch from the arena of ITS depth — the outer pass's partials stay as they
  are — and current_tape() is the innermost pass."""
  from openseq2seq_amd.parts import streams, tape as cb
  from openseq2seq_amd import capi
  dev = torch.device("cpu")
  saved = streams.join_side_streams
  streams.join_side_streams = lambda: None
  seen = []
  try:
    for rounds in range(3):          # round 0 teaches the arenas their demand, later rounds hand out arena slices
      held = {}
      inner = cb.Tape()

      def inner_op():
        seen.append(("inner", cb.current_tape() is inner))
        t = capi._zero_arena.take((4, 2, 16), dev)
        assert float(t.abs().sum()) == 0.0
        t.fill_(7.0)
        held["inner"] = t
      inner.record(inner_op)
      outer = cb.Tape()

      def outer_first():            # runs LAST (reverse order): the partials written before the nested pass survive
        seen.append(("outer_first", cb.current_tape() is outer))
        assert float(held["outer"].sum()) == 5.0 * held["outer"].numel()
        if rounds:
          a = held["outer"].data_ptr()
          b = held["inner"].data_ptr()
          assert abs(a - b) >= held["outer"].numel() * 4 or capi._zero_arenas[0].buf is not capi._zero_arenas[1].buf

      def outer_last():             # runs FIRST: takes scratch, writes it, then a nested pass runs
        t = capi._zero_arena.take((6, 2, 16), dev)
        assert float(t.abs().sum()) == 0.0
        t.fill_(5.0)
        held["outer"] = t
        inner.backward()
        assert cb.current_tape() is outer and capi._zero_arena is capi._zero_arenas[0]
      outer.record(outer_first)
      outer.record(outer_last)
      outer.backward()
      assert cb.current_tape() is None and capi._zero_arena is capi._zero_arenas[0]
    assert len(capi._zero_arenas) >= 2 and capi._zero_arenas[1].buf is not None
    assert all(ok for _, ok in seen) and len(seen) == 6
    # a failing closure unwinds the stack
    bad = cb.Tape()
    bad.record(lambda: 1 / 0)
    try:
      bad.backward()
    except ZeroDivisionError:
      pass
    assert cb.current_tape() is None and capi._zero_arena is capi._zero_arenas[0]
  finally:
    streams.join_side_streams = saved
