"""TensorBoard event files without TensorFlow or protobuf: what the reference's tf.summary.FileWriter leaves in
`logdir` (`events.out.tfevents.<time>.<host>`), written and read back with the record framing and the four
protobuf messages involved spelled out here.

Record (tensorflow/core/lib/io/record_writer.cc):
  uint64 length (little endian) | uint32 masked crc32c of those 8 bytes | data | uint32 masked crc32c of data
Messages (field numbers):
  Event          1 wall_time (double)  2 step (int64)  3 file_version (string)  5 summary (Summary)
  Summary        1 value (repeated Summary.Value)
  Summary.Value  1 tag (string)  2 simple_value (float)  5 histo (HistogramProto)
  HistogramProto 1 min  2 max  3 num  4 sum  5 sum_squares (doubles)
                 6 bucket_limit  7 bucket (packed repeated doubles)

Not written (out of scope): image summaries (attention / spectrogram plots), audio summaries, the graph_def and the
sampled transcripts of print_samples_steps.
"""
from __future__ import absolute_import, division, print_function

import math
import os
import socket
import struct
import sys
import time

import numpy as np

from .tensor_bundle import crc32c, mask_crc, unmask_crc, _varint, _proto_fields, _signed64

DBL_MAX = sys.float_info.max
NUM_BUCKETS = 1551
ZERO_BUCKET = 776          # +0.0 and -0.0: the first limit greater than 0 is limits[776] = 1e-12
STAT_FIELDS = ("min", "max", "num", "sum", "sum_squares", "nonfinite")

# ---- the tag strings, in one place ------------------------------------------------------------------------------
# `{var}` is the store's variable name (the reference's) with ':' replaced by '_' (optimizers.py:315), so
# "ForwardPass/.../kernel:0" appears as ".../kernel_0".
# NOTE on OPT_PREFIX: in TF 1 tf.summary.* prefixes the tag with the enclosing NAME scope, and optimize_loss opens
# variable_scope("Loss_Optimization") at optimizers.py:177 — after the learning_rate summary of :175, before every
# other one. That reading could not be checked against a TensorFlow run; if it is wrong, this line is the fix.
OPT_PREFIX = "Loss_Optimization/"
TAGS = {
    "train_loss": "train_loss",                                          # models/model.py:526-532
    "epoch": "epoch",
    "global_step_sec": "global_step/sec",                                # StepCounterHook of MonitoredTrainingSession
    "learning_rate": "learning_rate",                                    # optimizers.py:175
    "loss_scale": OPT_PREFIX + "loss_scale",                             # :202
    "global_gradient_norm": OPT_PREFIX + "global_gradient_norm",         # :293
    "global_clipped_gradient_norm": OPT_PREFIX + "global_clipped_gradient_norm",   # :327
    "gradients": OPT_PREFIX + "gradients/{var}",                         # :318 (histogram)
    "gradient_norm": OPT_PREFIX + "gradient_norm/{var}",                 # :320
    "variables": OPT_PREFIX + "variables/{var}",                         # :322 (histogram)
    "variable_norm": OPT_PREFIX + "variable_norm/{var}",                 # :324
    "larc_clip_on": OPT_PREFIX + "larc_clip_on/{var}",                   # :360 (clip mode only)
    "larc_grad_update": OPT_PREFIX + "larc_grad_update/{var}",           # :373
    "larc_final_lr": OPT_PREFIX + "larc_final_lr/{var}",                 # :375
    "eval_loss": "eval_loss",                                            # utils/hooks.py:219-245
}


def tag(kind, var=None):
  t = TAGS[kind]
  return t.format(var=var.replace(":", "_")) if var is not None else t


# ---- TensorFlow's default histogram buckets -----------------------------------------------------------------------
_LIMITS = None


def bucket_limits():
  """The 1551 bucket limits of tensorflow/core/lib/histogram/histogram.cc (float64, ascending): 1e-12 * 1.1^k by
  REPEATED multiplication while < 1e20 (774 values), mirrored, with 0 in the middle and -+DBL_MAX at the ends.
  bucket(v) = np.searchsorted(limits, v, side="right")."""
  global _LIMITS
  if _LIMITS is None:
    pos = []
    v = 1e-12
    while v < 1e20:
      pos.append(v)
      v *= 1.1
    lim = np.array([-DBL_MAX] + [-p for p in reversed(pos)] + [0.0] + pos + [DBL_MAX], np.float64)
    assert lim.size == NUM_BUCKETS
    lim.setflags(write=False)
    _LIMITS = lim
  return _LIMITS


# ---- protobuf encoding ----------------------------------------------------------------------------------------------
def _key(field, wire_type):
  return _varint((field << 3) | wire_type)


def _f_double(field, v):
  return _key(field, 1) + struct.pack("<d", float(v))


def _f_bytes(field, b):
  return _key(field, 2) + _varint(len(b)) + bytes(b)


def histogram_pairs(counts):
  """(limit, count) pairs of Histogram::EncodeToProto(preserve_zero_buckets = false): a non-empty bucket gives its
  pair, a maximal run of empty buckets gives ONE pair (limit of the run's last bucket, 0)."""
  counts = np.asarray(counts)
  assert counts.shape == (NUM_BUCKETS,)
  limits = bucket_limits()
  nz = counts != 0
  # keep bucket i when it is non-empty, or empty and the last of its run (the next one is non-empty or missing)
  keep = nz | np.append(nz[1:], True)
  idx = np.nonzero(keep)[0]
  return [(float(limits[i]), float(counts[i])) for i in idx]


def encode_histogram(stats, counts):
  """HistogramProto bytes. stats: mapping (or sequence in STAT_FIELDS order) with min, max, num, sum, sum_squares;
  counts: the 1551 bucket counts."""
  if not isinstance(stats, dict):
    stats = dict(zip(STAT_FIELDS, stats))
  pairs = histogram_pairs(counts)
  out = b"".join(_f_double(i + 1, stats[k]) for i, k in enumerate(STAT_FIELDS[:5]))
  out += _f_bytes(6, struct.pack("<%dd" % len(pairs), *[p[0] for p in pairs]))
  out += _f_bytes(7, struct.pack("<%dd" % len(pairs), *[p[1] for p in pairs]))
  return out


def _encode_value(tag_, simple_value=None, histo=None):
  out = _f_bytes(1, tag_.encode("utf-8"))
  if simple_value is not None:
    out += _key(2, 5) + struct.pack("<f", _as_float32(simple_value))
  if histo is not None:
    out += _f_bytes(5, histo)
  return out


def _as_float32(v):
  with np.errstate(over="ignore"):
    return float(np.float32(v))


def encode_event(wall_time, step=None, file_version=None, values=()):
  """Event bytes; values: encoded Summary.Value messages."""
  out = _f_double(1, wall_time)
  if step is not None:
    out += _key(2, 0) + _varint(int(step))
  if file_version is not None:
    out += _f_bytes(3, file_version.encode("utf-8"))
  if values:
    out += _f_bytes(5, b"".join(_f_bytes(1, v) for v in values))
  return out


def encode_record(data):
  header = struct.pack("<Q", len(data))
  return (header + struct.pack("<I", mask_crc(crc32c(header))) + bytes(data)
          + struct.pack("<I", mask_crc(crc32c(data))))


# ---- writer -----------------------------------------------------------------------------------------------------------
class EventFileWriter(object):
  """tf.summary.FileWriter's file: `logdir/events.out.tfevents.<int(time)>.<hostname>`, first record
  Event{wall_time, file_version: "brain.Event:2"}."""

  def __init__(self, logdir, filename_suffix=""):
    os.makedirs(logdir, exist_ok=True)
    self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s%s"
                             % (int(time.time()), socket.gethostname(), filename_suffix))
    self._f = open(self.path, "ab")
    self._write(encode_event(time.time(), file_version="brain.Event:2"))
    self.flush()

  def _write(self, event):
    self._f.write(encode_record(event))

  def add_scalars(self, step, scalars, wall_time=None):
    """One Event with a simple_value per tag; scalars: {tag: number} (insertion order is kept)."""
    if not scalars:
      return
    vals = [_encode_value(t, simple_value=v) for t, v in scalars.items()]
    self._write(encode_event(time.time() if wall_time is None else wall_time, step=step, values=vals))

  def add_histograms(self, step, histograms, wall_time=None):
    """One Event with a histogram per tag; histograms: {tag: (stats, counts)} as for encode_histogram."""
    if not histograms:
      return
    vals = [_encode_value(t, histo=encode_histogram(s, c)) for t, (s, c) in histograms.items()]
    self._write(encode_event(time.time() if wall_time is None else wall_time, step=step, values=vals))

  def flush(self):
    if self._f is not None:
      self._f.flush()

  def close(self):
    if self._f is not None:
      self._f.flush()
      self._f.close()
      self._f = None


# ---- reader -----------------------------------------------------------------------------------------------------------
def read_records(path):
  """The data of every record of an event file; both crcs of every record are checked (ValueError)."""
  buf = open(path, "rb").read()
  pos, n = 0, len(buf)
  while pos < n:
    if pos + 12 > n:
      raise ValueError("%s: truncated record header at byte %d" % (path, pos))
    header = buf[pos:pos + 8]
    if unmask_crc(struct.unpack_from("<I", buf, pos + 8)[0]) != crc32c(header):
      raise ValueError("%s: corrupted record length at byte %d" % (path, pos))
    ln = struct.unpack("<Q", header)[0]
    pos += 12
    if pos + ln + 4 > n:
      raise ValueError("%s: truncated record at byte %d" % (path, pos))
    data = buf[pos:pos + ln]
    if unmask_crc(struct.unpack_from("<I", buf, pos + ln)[0]) != crc32c(data):
      raise ValueError("%s: corrupted record data at byte %d" % (path, pos))
    pos += ln + 4
    yield data


def _double(bits):
  return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _packed_doubles(v):
  b = bytes(v)
  return list(struct.unpack("<%dd" % (len(b) // 8), b))


def _decode_histogram(buf):
  h = {"min": 0.0, "max": 0.0, "num": 0.0, "sum": 0.0, "sum_squares": 0.0, "bucket_limit": [], "bucket": []}
  names = {1: "min", 2: "max", 3: "num", 4: "sum", 5: "sum_squares"}
  for field, wt, v in _proto_fields(buf):
    if field in names and wt == 1:
      h[names[field]] = _double(v)
    elif field in (6, 7):
      key = "bucket_limit" if field == 6 else "bucket"
      h[key] += _packed_doubles(v) if wt == 2 else [_double(v)]
  return h


def read_events(path):
  """[(wall_time, step, {tag: float | histogram dict})] of an event file, the file_version record included (step 0,
  no values). A histogram dict has min, max, num, sum, sum_squares, bucket_limit and bucket."""
  out = []
  for data in read_records(path):
    wall_time, step, values = 0.0, 0, {}
    for field, wt, v in _proto_fields(memoryview(data)):
      if field == 1 and wt == 1:
        wall_time = _double(v)
      elif field == 2 and wt == 0:
        step = _signed64(v)
      elif field == 5 and wt == 2:
        for f2, w2, val in _proto_fields(v):
          if f2 != 1 or w2 != 2:
            continue
          name, content = None, None
          for f3, w3, x in _proto_fields(val):
            if f3 == 1 and w3 == 2:
              name = bytes(x).decode("utf-8")
            elif f3 == 2 and w3 == 5:
              content = struct.unpack("<f", struct.pack("<I", x))[0]
            elif f3 == 5 and w3 == 2:
              content = _decode_histogram(x)
          if name is not None:
            values[name] = content
    out.append((wall_time, step, values))
  return out


def event_files(logdir):
  if not os.path.isdir(logdir):
    return []
  return sorted(os.path.join(logdir, f) for f in os.listdir(logdir) if f.startswith("events.out.tfevents."))


# ---- the host side of the training summaries ----------------------------------------------------------------------
def larc_scalars(larc_params, lr, v_norm, g_norm):
  """optimizers.py:351-376 for one variable: {kind: value} of larc_clip_on (clip mode only), larc_grad_update and
  larc_final_lr."""
  eta = larc_params['larc_eta']
  mode = larc_params.get('larc_mode', 'clip')
  min_update = larc_params.get('min_update', 1e-7)
  eps = larc_params.get('epsilon', 1e-7)
  out = {}
  if mode == 'clip':
    denom = lr * (g_norm + eps)
    u = max(eta * v_norm / denom if denom != 0.0 else float("inf"), min_update)
    out["larc_clip_on"] = 1.0 if u < 1.0 else 0.0
    u = min(u, 1.0)
  else:
    u = max(eta * v_norm / (g_norm + eps), min_update)
  out["larc_grad_update"] = u
  out["larc_final_lr"] = lr * u
  return out


def eval_scalars(results, is_wkt=False):
  """utils/hooks.py:219-245: eval_loss and every number the evaluation returned; for the WikiText data layer also
  ppl = exp(loss) and bpc, which the reference writes as exp(loss / log(2)) (hooks.py:225) — reproduced as it is."""
  out = {}
  for k, v in results.items():
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
      continue
    out[TAGS["eval_loss"] if k in ("loss", "eval_loss") else k] = float(v)
  loss = out.get(TAGS["eval_loss"])
  if is_wkt and loss is not None:
    try:
      out["ppl"] = math.exp(loss)
      out["bpc"] = math.exp(loss / math.log(2))
    except OverflowError:
      out["ppl"] = out["bpc"] = float("inf")
  return out
