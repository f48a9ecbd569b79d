"""Host side of eval.py: the mIoU rule, the TensorBoard event writer, the skip logic of
last_evaluation.json, the binding of the evaluation symbols, and the command line."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import eval_ref      # noqa: E402


# ---------------------------------------------------------------- mIoU ---
def test_miou_on_hand_computed_matrices():
  from epos_amd import eval_utils
  # rows = ground truth. class 0: diagonal 5, row 5+1+0 = 6, column 5+2+0 = 7, union 6+7-5 = 8
  #                      class 1: diagonal 3, row 2+3+1 = 6, column 1+3+0 = 4, union 6+4-3 = 7
  #                      class 2: diagonal 4, row 0+0+4 = 4, column 0+1+4 = 5, union 4+5-4 = 5
  # IoU = 5/8, 3/7, 4/5; fg mean = (3/7 + 4/5) / 2 = 43/70; all = (5/8 + 3/7 + 4/5) / 3
  cm = [[5, 1, 0], [2, 3, 1], [0, 0, 4]]
  for fn in (eval_ref.miou, eval_utils.miou_from_confusion):
    all_, fg = fn(cm)
    assert fg == pytest.approx(43.0 / 70.0, abs=1e-15)
    assert all_ == pytest.approx((5.0 / 8 + 3.0 / 7 + 4.0 / 5) / 3, abs=1e-15)
    # class 2 never occurs (union 0): left out, not counted as 0
    all_, fg = fn([[5, 1, 0], [2, 3, 0], [0, 0, 0]])
    assert fg == pytest.approx(3.0 / 6, abs=1e-15)            # 3 / (5 + 4 - 3)
    assert all_ == pytest.approx((5.0 / 8 + 0.5) / 2, abs=1e-15)
    # background only: no foreground class -> (0, 0)
    assert fn([[9, 0, 0], [0, 0, 0], [0, 0, 0]]) == (0.0, 0.0)
    assert fn([[0]]) == (0.0, 0.0)
    # background absent (row and column 0 empty): its IoU counts as 1.0
    all_, fg = fn([[0, 0, 0], [0, 2, 2], [0, 0, 4]])           # IoU 2/4 and 4/6
    assert fg == pytest.approx((0.5 + 4.0 / 6) / 2, abs=1e-15)
    assert all_ == pytest.approx((0.5 + 4.0 / 6 + 1.0) / 3, abs=1e-15)


def test_confusion_reference_rules():
  cm, bad = eval_ref.confusion([0, 1, 255, 2, 1, 7, 1], [1, 1, 9, 2, -1, 0, 3], 3, 255)
  assert cm.tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 1]] and bad == 3
  cm, bad = eval_ref.confusion([0, 1, 1], [0, 0, 1], 2, 1)   # the ignore rule wins
  assert cm.tolist() == [[1, 0], [0, 0]] and bad == 0


# ---------------------------------------------------------------- event files ---
SCALARS = [('eval/obj_cls_miou_all', 0.625), ('eval/obj_cls_miou_fg', 1.0 / 3.0),
           ('eval/frag_acc', 0.0), ('eval/frag_acc_seg', 1.0)]


def test_event_file_round_trip_and_crc(tmp_path):
  from epos_amd import tf_events, tfrecord
  path = tf_events.write_scalars(str(tmp_path), SCALARS, 123456, wall_time=1700000000.25)
  assert re.match(r'events\.out\.tfevents\.1700000000\.', os.path.basename(path))
  records = list(tfrecord.read_records(path, verify_crc=True))   # raises on a bad CRC
  assert len(records) == 2
  first, second = tf_events.read_events(path)
  assert first == {'wall_time': 1700000000.25, 'step': 0, 'file_version': 'brain.Event:2',
                   'scalars': []}
  assert second['step'] == 123456 and second['file_version'] is None
  assert second['wall_time'] == 1700000000.25
  assert [t for t, _ in second['scalars']] == [t for t, _ in SCALARS]
  assert [v for _, v in second['scalars']] == [float(np.float32(v)) for _, v in SCALARS]
  # a second file in the same second does not overwrite the first
  other = tf_events.write_scalars(str(tmp_path), SCALARS[:1], 1, wall_time=1700000000.25)
  assert other != path and len(tf_events.read_events(path)) == 2
  # a flipped byte fails the CRC check
  raw = bytearray(open(path, 'rb').read())
  raw[20] ^= 1
  bad = tmp_path / 'bad'
  bad.write_bytes(bytes(raw))
  with pytest.raises(IOError):
    tf_events.read_events(str(bad))


def _google_event_class():
  """Event / Summary of tensorflow/core/util/event.proto and framework/summary.proto (public
  field numbers), declared at run time for Google's protobuf library."""
  from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
  fd = descriptor_pb2.FileDescriptorProto(name='epos_test_event.proto', package='epostest',
                                          syntax='proto3')
  T = descriptor_pb2.FieldDescriptorProto
  val = fd.message_type.add(name='Value')
  val.field.add(name='tag', number=1, type=T.TYPE_STRING, label=T.LABEL_OPTIONAL)
  val.field.add(name='simple_value', number=2, type=T.TYPE_FLOAT, label=T.LABEL_OPTIONAL)
  summ = fd.message_type.add(name='Summary')
  summ.field.add(name='value', number=1, type=T.TYPE_MESSAGE, label=T.LABEL_REPEATED,
                 type_name='.epostest.Value')
  ev = fd.message_type.add(name='Event')
  ev.field.add(name='wall_time', number=1, type=T.TYPE_DOUBLE, label=T.LABEL_OPTIONAL)
  ev.field.add(name='step', number=2, type=T.TYPE_INT64, label=T.LABEL_OPTIONAL)
  ev.field.add(name='file_version', number=3, type=T.TYPE_STRING, label=T.LABEL_OPTIONAL)
  ev.field.add(name='summary', number=5, type=T.TYPE_MESSAGE, label=T.LABEL_OPTIONAL,
               type_name='.epostest.Summary')
  ev.oneof_decl.add(name='what')
  for f in ev.field[2:]:
    f.oneof_index = 0
  pool = descriptor_pool.DescriptorPool()
  pool.Add(fd)
  return message_factory.GetMessageClass(pool.FindMessageTypeByName('epostest.Event'))


def test_event_wire_format_against_googles_protobuf_library():
  pytest.importorskip('google.protobuf')
  from epos_amd import tf_events
  Event = _google_event_class()
  version, summary = tf_events.encode_events(SCALARS, 77, wall_time=12.5)
  ev = Event.FromString(version)
  assert ev.WhichOneof('what') == 'file_version' and ev.file_version == 'brain.Event:2'
  assert ev.wall_time == 12.5 and ev.step == 0
  ev = Event.FromString(summary)
  assert ev.WhichOneof('what') == 'summary' and ev.step == 77 and ev.wall_time == 12.5
  assert [(v.tag, v.simple_value) for v in ev.summary.value] == [
      (t, float(np.float32(x))) for t, x in SCALARS]
  # the other direction: what protobuf serialises, this module's reader decodes
  g = Event(wall_time=3.0, step=-4)
  g.summary.value.add(tag='a/b', simple_value=0.25)
  got = tf_events.decode_event(g.SerializeToString())
  assert got == {'wall_time': 3.0, 'step': -4, 'file_version': None, 'scalars': [('a/b', 0.25)]}


# ---------------------------------------------------------------- last_evaluation.json ---
def test_skip_logic_is_a_function_of_file_checkpoint_time_and_interval():
  from epos_amd.eval_utils import skip_reason
  last = json.dumps({'time': 1000.0, 'checkpoint_path': '/m/train/model.ckpt-10'})
  assert skip_reason(None, '/m/train/model.ckpt-10', 1001.0, 3600) is None     # no file yet
  same = skip_reason(last, '/m/train/model.ckpt-10', 99999.0, 0)
  assert same == 'Skipping evaluation (checkpoint /m/train/model.ckpt-10 has been evaluated).'
  soon = skip_reason(last, '/m/train/model.ckpt-20', 1500.0, 3600)
  assert soon == 'Skipping evaluation (only 500.0 s from the last evaluation).'
  assert skip_reason(last, '/m/train/model.ckpt-20', 4600.0, 3600) is None     # interval passed
  assert skip_reason(last, '/m/train/model.ckpt-20', 1000.0, 0) is None        # interval 0
  # random weights have no checkpoint path: a second run of the same model is "the same"
  none = json.dumps({'time': 1000.0, 'checkpoint_path': None})
  assert 'checkpoint None has been evaluated' in skip_reason(none, None, 1e9, 0)


# ---------------------------------------------------------------- binding ---
def test_eval_symbols_are_declared_and_bound():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  nargs = {'epos_eval_lds_max_cls': 0, 'epos_eval_confusion': 8, 'epos_eval_frag_hits': 10}
  for name, n in nargs.items():
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is ctypes.c_int and len(argtypes) == n, name
    decl = re.search(r'\bint %s\s*\(([^)]*)\)\s*;' % name, header)
    assert decl, name
    params = decl.group(1).strip()
    assert (0 if params == 'void' else params.count(',') + 1) == n, name
  lib = _lib.load()
  assert 1 <= lib.epos_eval_lds_max_cls() < 256       # both regimes exist below the class limit
  assert lib.epos_abi_version() == 7


def test_table_is_plain_aligned_text():
  from epos_amd.eval_utils import format_table
  txt = format_table(np.array([[5, 1, 0], [2, 1234, 1], [0, 0, 4]]))
  rows = txt.rstrip('\n').split('\n')
  assert len(rows) == 4 and len(set(len(r) for r in rows)) == 1
  assert [int(x) for x in rows[0].split()] == [0, 1, 2]
  assert [[int(x) for x in r.split()] for r in rows[1:]] == [
      [0, 5, 1, 0], [1, 2, 1234, 1], [2, 0, 0, 4]]


# ---------------------------------------------------------------- command line ---
@pytest.fixture
def eval_module():
  import importlib
  return importlib.import_module('eval')


def test_eval_cli_defaults(eval_module, tmp_path, monkeypatch):
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  args, model_dir = eval_module.prepare(['--model=m', '--dataset', 'lm', '--master', 'x'])
  assert model_dir == os.path.join(str(tmp_path), 'm')
  assert args.eval_crop_size == '640,480' and args.eval_max_height_before_crop == 480
  assert args.eval_interval_secs == 3600 and args.eval_tfrecord_names is None
  assert args.batch_size == 1 and args.eval_frag_labels is None
  assert args.precision == 'fp32' and args.num_frags == 64 and args.synthetic == 0
  assert not hasattr(args, 'fitting_method') and not hasattr(args, 'infer_crop_size')
  from epos_amd import cli
  assert cli.crop_size(args.eval_crop_size) == (640, 480)
  # params.yml overrides the defaults
  (tmp_path / 'm').mkdir()
  (tmp_path / 'm' / 'params.yml').write_text('eval_crop_size: "128,96"\nnum_frags: 32\n')
  args, _ = eval_module.prepare(['--model=m', '--dataset', 'lm'])
  assert args.eval_crop_size == '128,96' and args.num_frags == 32


def test_eval_cli_needs_dataset_and_bop_path(eval_module, tmp_path, monkeypatch):
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.delenv('BOP_PATH', raising=False)
  with pytest.raises(ValueError, match=r'needs --dataset and \$BOP_PATH \(object models\)'):
    eval_module.prepare(['--model=m', '--dataset', 'lm'])
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  with pytest.raises(ValueError, match=r'needs --dataset and \$BOP_PATH \(object models\)'):
    eval_module.prepare(['--model=m'])


def test_eval_cli_refuses_unsupported_common_flags(eval_module, tmp_path, monkeypatch):
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  with pytest.raises(NotImplementedError, match='upsample_logits'):
    eval_module.prepare(['--model=m', '--dataset', 'lm', '--upsample_logits', 'true'])
  (tmp_path / 'm').mkdir()
  (tmp_path / 'm' / 'params.yml').write_text('frag_cls_agnostic: true\n')
  with pytest.raises(NotImplementedError, match='frag_cls_agnostic'):
    eval_module.prepare(['--model=m', '--dataset', 'lm'])
