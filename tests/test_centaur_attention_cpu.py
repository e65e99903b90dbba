"""CPU side of the dense wide-head attention: the two entry points are declared, exported and bound from the header,
the layer names the shapes the kernel is built for and refuses the rest, and the padding bias follows the ids."""
import pytest
import torch


def test_entry_points_are_declared_and_exported():
  from openseq2seq_amd import _lib
  decls = _lib.declarations()
  for name in ("os2s_attention_wide_fwd", "os2s_attention_wide_bwd"):
    assert name in decls and decls[name][2], name          # a launch: int result, a stream argument
    assert hasattr(_lib.lib(), name), name
  assert len(decls["os2s_attention_wide_fwd"][1]) == 23 and len(decls["os2s_attention_wide_bwd"][1]) == 25


def test_shape_check_names_the_supported_set():
  from openseq2seq_amd import capi
  from openseq2seq_amd.parts.centaur import attention as catt
  assert capi.ATTENTION_WIDE_HEAD_DIMS == (32, 64, 128, 256, 512) and capi.ATTENTION_WIDE_MAX_KEYS == 512
  for hidden, heads in ((512, 1), (512, 2), (256, 1), (128, 4), (64, 2)):
    assert catt.check_shape(hidden, heads, 184) == hidden // heads
  for hidden, heads, S in ((1024, 1, 8), (48, 1, 8), (64, 4, 8), (512, 1, 520), (512, 1, 20)):
    with pytest.raises(NotImplementedError):
      catt.check_shape(hidden, heads, S)
  with pytest.raises(ValueError):
    catt.check_shape(512, 3, 8)


def test_padding_bias_follows_the_ids_not_the_lengths():
  from openseq2seq_amd.parts.centaur import padding_bias
  ids = torch.tensor([[3, 0, 4, 0], [1, 2, 3, 4]])
  kb = padding_bias(ids)
  assert kb.dtype is torch.float32
  assert kb.tolist() == [[0.0, -1e9, 0.0, -1e9], [0.0, 0.0, 0.0, 0.0]]
