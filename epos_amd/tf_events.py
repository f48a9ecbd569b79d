"""TensorBoard event files without TensorFlow: scalar summaries only.

An event file is a TFRecord file (the framing of epos_amd/tfrecord.py: write_records /
read_records) whose records are serialized ``Event`` messages of tensorflow/core/util/event.proto:

    Event   { double wall_time = 1; int64 step = 2;
              oneof what { string file_version = 3; Summary summary = 5; } }
    Summary { repeated Value value = 1; }
    Value   { string tag = 1; float simple_value = 2; }

The first record carries file_version "brain.Event:2", as TensorFlow's writer puts it; every
following one a summary. The file name is events.out.tfevents.<time>.<host>, the pattern
TensorBoard looks for.

PARITY UNPINNED against TensorFlow, like the other TF formats of this build: TensorFlow is not
available, so the writer is checked against this module's reader and, where google.protobuf is
installed, against Google's runtime on a descriptor built from the lines above
(tests/test_eval_host.py).
"""
import os
import socket
import struct
import time

from epos_amd import tfrecord
from epos_amd.tfrecord import _enc_ld, _enc_varint, _fields

FILE_VERSION = 'brain.Event:2'


def _enc_event(wall_time, step, file_version=None, scalars=None):
  out = b'\x09' + struct.pack('<d', float(wall_time))              # 1: double
  if step:
    out += b'\x10' + _enc_varint(int(step))                        # 2: int64
  if file_version is not None:
    out += _enc_ld(3, file_version.encode('utf-8'))
  if scalars is not None:
    values = b''.join(
        _enc_ld(1, _enc_ld(1, tag.encode('utf-8')) + b'\x15' + struct.pack('<f', float(v)))
        for tag, v in scalars)
    out += _enc_ld(5, values)
  return out


def encode_events(scalars, step, wall_time=None):
  """The records of an event file holding `scalars` ([(tag, value)] or {tag: value}) at
  `step`: the version record, then one Event with all the values."""
  wall_time = time.time() if wall_time is None else wall_time
  if scalars is None:                        # the version record alone (EventWriter)
    return [_enc_event(wall_time, 0, file_version=FILE_VERSION)]
  if isinstance(scalars, dict):
    scalars = list(scalars.items())
  return [_enc_event(wall_time, 0, file_version=FILE_VERSION),
          _enc_event(wall_time, step, scalars=scalars)]


def write_scalars(log_dir, scalars, step, wall_time=None):
  """Writes a new event file into log_dir and returns its path."""
  wall_time = time.time() if wall_time is None else wall_time
  os.makedirs(log_dir, exist_ok=True)
  base = os.path.join(log_dir, 'events.out.tfevents.%010d.%s' % (
      int(wall_time), socket.gethostname()))
  path, n = base, 0
  while os.path.exists(path):                # two files within one second: keep both
    n += 1
    path = '%s.%d' % (base, n)
  tfrecord.write_records(path, encode_events(scalars, step, wall_time))
  return path


class EventWriter(object):
  """One event file in log_dir that grows: the version record now, then one Event per add()
  (a training run's scalars at its log steps)."""

  def __init__(self, log_dir, wall_time=None):
    wall_time = time.time() if wall_time is None else wall_time
    self.path = write_scalars(log_dir, None, 0, wall_time)

  def add(self, scalars, step, wall_time=None):
    wall_time = time.time() if wall_time is None else wall_time
    if isinstance(scalars, dict):
      scalars = list(scalars.items())
    tfrecord.write_records(self.path, [_enc_event(wall_time, step, scalars=scalars)],
                           append=True)


def decode_event(data):
  """Serialized Event -> dict(wall_time, step, file_version or None, scalars [(tag, value)])."""
  ev = {'wall_time': 0.0, 'step': 0, 'file_version': None, 'scalars': []}
  for num, wt, val in _fields(data):
    if num == 1 and wt == 1:
      ev['wall_time'] = struct.unpack('<d', val)[0]
    elif num == 2 and wt == 0:
      ev['step'] = val - (1 << 64) if val >> 63 else val
    elif num == 3 and wt == 2:
      ev['file_version'] = bytes(val).decode('utf-8')
    elif num == 5 and wt == 2:
      for n, w, value in _fields(val):
        if n != 1 or w != 2:
          continue
        tag, simple = None, None
        for m, x, v in _fields(value):
          if m == 1 and x == 2:
            tag = bytes(v).decode('utf-8')
          elif m == 2 and x == 5:
            simple = struct.unpack('<f', v)[0]
        if tag is not None and simple is not None:
          ev['scalars'].append((tag, simple))
  return ev


def read_events(path, verify_crc=True):
  """Every Event of an event file, in order (decode_event)."""
  return [decode_event(rec) for rec in tfrecord.read_records(path, verify_crc)]
