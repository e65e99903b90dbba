"""The TensorBoard event file format of openseq2seq_amd/utils/summary.py: record framing and crcs, the four protobuf
messages, TensorFlow's histogram encoding and bucket table. No GPU."""
import os
import struct
import sys

import numpy as np
import pytest

from openseq2seq_amd.utils import summary as S
from openseq2seq_amd.utils.tensor_bundle import crc32c, mask_crc, unmask_crc

DBL_MAX = sys.float_info.max


def test_crc32c_and_mask():
  crc = crc32c(b"123456789")
  assert crc == 0xE3069283
  masked = (((crc >> 15) | (crc << 17)) + 0xa282ead8) % (1 << 32)
  assert mask_crc(crc) == masked
  assert unmask_crc(masked) == crc


def test_hand_assembled_record_round_trips(tmp_path):
  # Event{wall_time = 1.5, step = 3, summary{value{tag "a", simple_value 0.25}}}, byte by byte
  value = b"\x0a\x01a" + b"\x15" + struct.pack("<f", 0.25)
  summary = b"\x0a" + bytes([len(value)]) + value
  event = b"\x09" + struct.pack("<d", 1.5) + b"\x10\x03" + b"\x2a" + bytes([len(summary)]) + summary
  header = struct.pack("<Q", len(event))
  record = header + struct.pack("<I", mask_crc(crc32c(header))) + event + struct.pack("<I", mask_crc(crc32c(event)))
  assert S.encode_event(1.5, step=3, values=[S._encode_value("a", simple_value=0.25)]) == event
  assert S.encode_record(event) == record
  path = tmp_path / "events.out.tfevents.0.host"
  path.write_bytes(record)
  assert S.read_events(str(path)) == [(1.5, 3, {"a": 0.25})]


def _example_counts():
  lim = S.bucket_limits()
  vals = np.array([0.05] * 3 + [-0.05] * 2)
  counts = np.bincount(np.searchsorted(lim, vals, side="right"), minlength=S.NUM_BUCKETS)
  stats = {"min": -0.05, "max": 0.05, "num": 5.0, "sum": 0.05, "sum_squares": 5 * 0.0025}
  return stats, counts


def _write_example(tmp_path):
  w = S.EventFileWriter(str(tmp_path))
  w.add_scalars(7, {"train_loss": 2.5}, wall_time=123.0)
  w.add_histograms(7, {"Loss_Optimization/variables/w_0": _example_counts()}, wall_time=124.0)
  w.flush()
  w.close()
  return w.path


def test_file_reads_back(tmp_path):
  path = _write_example(tmp_path)
  assert os.path.basename(path).startswith("events.out.tfevents.")
  assert S.event_files(str(tmp_path)) == [path]
  ev = S.read_events(path)
  assert len(ev) == 3
  assert ev[0][1] == 0 and ev[0][2] == {}
  assert ev[1] == (123.0, 7, {"train_loss": 2.5})
  wall, step, vals = ev[2]
  h = vals["Loss_Optimization/variables/w_0"]
  lim = S.bucket_limits()
  assert (wall, step) == (124.0, 7)
  assert (h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]) == (-0.05, 0.05, 5.0, 0.05, 5 * 0.0025)
  assert h["bucket_limit"] == [lim[515], lim[516], lim[1034], lim[1035], DBL_MAX]
  assert h["bucket"] == [0.0, 2.0, 0.0, 3.0, 0.0]


def _proto_classes():
  """Event / Summary / HistogramProto built at run time from the field numbers, sharing no code with the writer."""
  pytest.importorskip("google.protobuf")
  from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
  F = descriptor_pb2.FieldDescriptorProto
  fd = descriptor_pb2.FileDescriptorProto()
  fd.name, fd.package, fd.syntax = "os2s_test_event.proto", "os2s_test", "proto3"

  def msg(name, fields):
    m = fd.message_type.add()
    m.name = name
    for fname, num, ftype, label, tname in fields:
      f = m.field.add()
      f.name, f.number, f.type, f.label = fname, num, ftype, label
      if tname:
        f.type_name = ".os2s_test." + tname
    return m

  O, R = F.LABEL_OPTIONAL, F.LABEL_REPEATED
  msg("HistogramProto", [("min", 1, F.TYPE_DOUBLE, O, None), ("max", 2, F.TYPE_DOUBLE, O, None),
                         ("num", 3, F.TYPE_DOUBLE, O, None), ("sum", 4, F.TYPE_DOUBLE, O, None),
                         ("sum_squares", 5, F.TYPE_DOUBLE, O, None), ("bucket_limit", 6, F.TYPE_DOUBLE, R, None),
                         ("bucket", 7, F.TYPE_DOUBLE, R, None)])
  msg("Value", [("tag", 1, F.TYPE_STRING, O, None), ("simple_value", 2, F.TYPE_FLOAT, O, None),
                ("histo", 5, F.TYPE_MESSAGE, O, "HistogramProto")])
  msg("Summary", [("value", 1, F.TYPE_MESSAGE, R, "Value")])
  msg("Event", [("wall_time", 1, F.TYPE_DOUBLE, O, None), ("step", 2, F.TYPE_INT64, O, None),
                ("file_version", 3, F.TYPE_STRING, O, None), ("summary", 5, F.TYPE_MESSAGE, O, "Summary")])
  pool = descriptor_pool.DescriptorPool()
  pool.Add(fd)
  desc = pool.FindMessageTypeByName("os2s_test.Event")
  if hasattr(message_factory, "GetMessageClass"):
    return message_factory.GetMessageClass(desc)
  return message_factory.MessageFactory(pool).GetPrototype(desc)


def test_file_decodes_through_protobuf(tmp_path):
  Event = _proto_classes()
  path = _write_example(tmp_path)
  buf = open(path, "rb").read()
  events, pos = [], 0
  while pos < len(buf):
    (ln,) = struct.unpack_from("<Q", buf, pos)
    e = Event()
    e.ParseFromString(buf[pos + 12:pos + 12 + ln])
    events.append(e)
    pos += 12 + ln + 4
  assert len(events) == 3
  assert events[0].file_version == "brain.Event:2" and events[0].wall_time > 0
  assert events[1].step == 7 and events[1].wall_time == 123.0
  assert [(v.tag, v.simple_value) for v in events[1].summary.value] == [("train_loss", 2.5)]
  (v,) = events[2].summary.value
  lim = S.bucket_limits()
  assert v.tag == "Loss_Optimization/variables/w_0"
  assert (v.histo.min, v.histo.max, v.histo.num, v.histo.sum) == (-0.05, 0.05, 5.0, 0.05)
  assert list(v.histo.bucket_limit) == [lim[515], lim[516], lim[1034], lim[1035], DBL_MAX]
  assert list(v.histo.bucket) == [0.0, 2.0, 0.0, 3.0, 0.0]


def test_histogram_pairs():
  lim = S.bucket_limits()
  _, counts = _example_counts()
  assert S.histogram_pairs(counts) == [(lim[515], 0.0), (lim[516], 2.0), (lim[1034], 0.0), (lim[1035], 3.0),
                                       (DBL_MAX, 0.0)]
  one = np.zeros(S.NUM_BUCKETS, np.uint32)
  one[S.ZERO_BUCKET] = 64 * 4096                      # a constant tensor of zeros: one bucket
  assert S.histogram_pairs(one) == [(0.0, 0.0), (1e-12, float(64 * 4096)), (DBL_MAX, 0.0)]
  first = np.zeros(S.NUM_BUCKETS, np.uint32)
  first[0], first[-1] = 1, 2                          # no empty run at either end
  assert S.histogram_pairs(first) == [(-DBL_MAX, 1.0), (lim[1549], 0.0), (DBL_MAX, 2.0)]


@pytest.mark.parametrize("where", ["data", "length"])
def test_flipped_byte_raises(tmp_path, where):
  path = _write_example(tmp_path)
  buf = bytearray(open(path, "rb").read())
  (ln0,) = struct.unpack_from("<Q", buf, 0)
  second = 12 + ln0 + 4                               # start of the second record
  buf[second + (12 + 3 if where == "data" else 0)] ^= 0x01
  open(path, "wb").write(bytes(buf))
  with pytest.raises(ValueError, match="corrupted record " + where):
    S.read_events(path)


def test_bucket_table():
  lim = S.bucket_limits()
  assert lim.shape == (1551,) and lim.dtype == np.float64
  assert lim[776] == 1e-12 and lim[775] == 0.0
  assert lim[0] == -DBL_MAX and lim[-1] == DBL_MAX
  assert np.all(np.diff(lim) > 0)
  assert np.array_equal(lim[1:775], -lim[776:1550][::-1])
  finite = lim[1:-1]
  finite = finite[finite != 0.0]
  assert finite.size == 1548
  with np.errstate(over="ignore"):
    assert not np.any(finite.astype(np.float32).astype(np.float64) == finite)
  assert np.searchsorted(lim, [0.0, -0.0], side="right").tolist() == [776, 776]


def test_logical_count_is_the_leading_prefix():
  """Device padding is left out of a summary only where the logical elements are a leading prefix."""
  from openseq2seq_amd.optimizers.flat_params import Param
  from openseq2seq_amd.optimizers.summaries import logical_count
  assert logical_count(Param("dense/kernel", (1, 40, 16), "conv", 0.0, logical_out=33)) == 33 * 16
  assert logical_count(Param("dense/bias", (40,), "vector", 0.0, logical_out=33)) == 33
  assert logical_count(Param("conv/kernel", (3, 40, 16), "conv", 0.0, logical_out=33)) == 3 * 40 * 16
  assert logical_count(Param("plain", (5, 7), "dense", 0.0)) == 35
  wx = Param("rnn/wx_0", (1, 64, 16), "conv", 0.0)
  wx.logical_in = 13                                   # zero columns inside every row: not a prefix
  assert logical_count(wx) == 64 * 16


def test_tag_table_and_helpers():
  assert S.tag("gradient_norm", "a/b/kernel:0") == "Loss_Optimization/gradient_norm/a/b/kernel_0"
  assert S.tag("learning_rate") == "learning_rate"
  r = S.eval_scalars({"loss": 2.0, "name": "x", "samples": 3}, is_wkt=True)
  import math
  assert r == {"eval_loss": 2.0, "samples": 3.0, "ppl": math.exp(2.0), "bpc": math.exp(2.0 / math.log(2))}
  larc = S.larc_scalars({"larc_eta": 0.002}, 0.1, 2.0, 0.5)
  u = 0.002 * 2.0 / (0.1 * (0.5 + 1e-7))
  assert larc == {"larc_clip_on": 1.0, "larc_grad_update": u, "larc_final_lr": 0.1 * u}
