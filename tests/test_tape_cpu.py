"""Where the reverse-mode engine lives: parts/tape.py (Tape, Act), parts/streams.py (side streams),
parts/activations.py (activation ids); parts/cnns/conv_blocks.py keeps the CNN layers and re-exports the engine's
classes and functions for the callers that reach them through it."""

# module-level state and A/B knobs: a second binding under another module name would diverge silently
ONE_HOME = {
    "streams": ("_SIDE_STREAMS", "_JOIN_EVENT", "_STREAM_OBJ", "_FORK_EVENT", "_SIDE_STREAM_ENABLED",
                "_SIDE_KEY_OVERRIDE", "DRES_OWN_STREAM"),
    "tape": ("_TAPE_STACK", "SMALL_WGRAD_GROUP", "CONV_WGRAD_UNIT_BUDGET"),
    "conv_blocks": ("_FWD_SIDE_BUSY", "_WGRAD_RR", "FUSE_BN_BWD", "GROUP_WGRAD", "GROUP_POINTWISE_WGRAD",
                    "POINTWISE_WGRAD_GROUP", "GROUP_WGRAD_PP", "DRES_FWD_SIDE", "WGRAD_STREAMS", "DRES_FUSE_BN_BWD",
                    "SEP_FUSE_BN_BWD", "FOLD_SEP_K1"),
    "activations": ("ACT_IDS",),
}


def test_engine_modules_one_home_per_global_and_fresh_tape_flushes():
  from openseq2seq_amd.parts import activations, streams, tape
  from openseq2seq_amd.parts.cnns import conv_blocks
  mods = {"streams": streams, "tape": tape, "conv_blocks": conv_blocks, "activations": activations}
  # the re-exports are the same objects (bench.py patches conv_blocks.Tape.backward: an attribute of the one class)
  assert conv_blocks.Tape is tape.Tape and conv_blocks.Act is tape.Act
  assert conv_blocks.on_side_stream is streams.on_side_stream
  assert conv_blocks.current_tape is tape.current_tape and conv_blocks.act_id is activations.act_id
  for home, names in ONE_HOME.items():
    for name in names:
      assert [k for k, m in sorted(mods.items()) if hasattr(m, name)] == [home], name
  # a tape that never ran a pass holds nothing back
  t = tape.Tape()
  assert t.flush_deferred() is None and t.flush_conv_wgrads() is None
  assert t._deferred == [] and t._cdeferred == [] and t._pending is None and t.ops == []
  streams.set_side_key_override(7)
  assert streams._SIDE_KEY_OVERRIDE == 7
  streams.set_side_key_override(None)
  assert streams._SIDE_KEY_OVERRIDE is None
