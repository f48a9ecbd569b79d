"""epos_amd/_call.py on the host: the helpers compare t.device with a given device, so CPU tensors
exercise every check. The expectations for flat, rows, out and workspace were fixed by running
these cases against loss._flat, SegmentationEval._flat, loss._rows, loss._out and
loss._workspace before the helpers moved."""
import contextlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from epos_amd import _call                                # noqa: E402
from epos_amd._lib import EposError                       # noqa: E402

CPU = torch.device('cpu')
META = torch.device('meta')                               # "another device" without a GPU


# ------------------------------------------------------------------------ ptr ---
def test_ptr_of_none_is_null():
  assert _call.ptr(None) is None
  assert _call.ptr(None, 5) is None


@pytest.mark.parametrize('dtype,size', [(torch.float32, 4), (torch.int64, 8)])
def test_ptr_offsets_count_elements(dtype, size):
  t = torch.zeros(16, dtype=dtype)
  assert _call.ptr(t).value == t.data_ptr()
  assert _call.ptr(t, 3).value == t.data_ptr() + 3 * size


def test_ptr_passes_a_view_through():
  t = torch.zeros(4, 6)
  v = t.t()[2:]                                           # non-contiguous, offset 2 elements
  assert not v.is_contiguous()
  assert _call.ptr(v).value == v.data_ptr() == t.data_ptr() + 2 * 4


# ----------------------------------------------------------------------- flat ---
@pytest.mark.parametrize('where', ['the losses', 'the evaluation'])
def test_flat_refusals(where):
  t = torch.zeros(2, 3, dtype=torch.float32)
  with pytest.raises(EposError) as e:
    _call.flat(t, META, torch.float32, 6, 'x', where)
  assert str(e.value) == 'x is on cpu, %s on meta' % where
  with pytest.raises(TypeError) as e:
    _call.flat(t, CPU, torch.int32, 6, 'x', where)
  assert str(e.value) == 'x must be torch.int32, got torch.float32'
  with pytest.raises(ValueError) as e:
    _call.flat(t, CPU, torch.float32, 7, 'x', where)
  assert str(e.value) == 'x holds 6 values, expected 7'


def test_flat_accepts():
  t = torch.arange(6, dtype=torch.float32).reshape(2, 3)
  f = _call.flat(t, CPU, torch.float32, 6, 'x', 'the losses')
  assert f.shape == (6,) and f.data_ptr() == t.data_ptr()          # dense already: a view
  assert _call.flat(t, CPU, torch.float32, None, 'x', 'the evaluation').shape == (6,)
  d = _call.flat(t.t(), CPU, torch.float32, None, 'x', 'the evaluation')
  assert d.is_contiguous() and d.data_ptr() != t.data_ptr()
  assert d.tolist() == [0.0, 3.0, 1.0, 4.0, 2.0, 5.0]


# ----------------------------------------------------------------------- rows ---
def test_rows_takes_a_slice_of_a_wider_buffer_as_a_view():
  buf = torch.zeros(2, 5, 8)
  v, ld = _call.rows(buf[..., :3], 3)
  assert (tuple(v.shape), ld) == ((10, 3), 8) and v.data_ptr() == buf.data_ptr()
  v, ld = _call.rows(buf, 8)                                       # dense: stride = width
  assert (tuple(v.shape), ld) == ((10, 8), 8) and v.data_ptr() == buf.data_ptr()


def test_rows_of_a_single_row():
  buf = torch.zeros(1, 8)
  v, ld = _call.rows(buf[:, :3], 3)
  assert (tuple(v.shape), ld) == ((1, 3), 3) and v.data_ptr() == buf.data_ptr()


def test_rows_makes_a_transposed_input_dense():
  t = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()      # [4, 3], stride (1, 4)
  v, ld = _call.rows(t, 3)
  assert (tuple(v.shape), ld) == ((4, 3), 3)
  assert v.is_contiguous() and v.data_ptr() != t.data_ptr() and v.equal(t)
  gaps = torch.zeros(2, 3, 8)[:, :2, :3]                           # rows no constant stride apart
  v, ld = _call.rows(gaps, 3)
  assert (tuple(v.shape), ld) == ((4, 3), 3) and v.data_ptr() != gaps.data_ptr()


# ------------------------------------------------------------------------ out ---
def test_out_allocates_for_none():
  t = _call.out(None, CPU, torch.float64, (2, 3), 'o')
  assert t.shape == (2, 3) and t.dtype == torch.float64 and t.device == CPU


def test_out_by_shape():
  ok = torch.zeros(2, 3)
  assert _call.out(ok, CPU, torch.float32, (2, 3), 'o') is ok
  for bad, dev, dtype in ((torch.zeros(3, 2), CPU, torch.float32),          # shape
                          (torch.zeros(3, 2).t(), CPU, torch.float32),      # not contiguous
                          (ok, CPU, torch.float64), (ok, META, torch.float32)):
    with pytest.raises(ValueError) as e:
      _call.out(bad, dev, dtype, (2, 3), 'o')
    assert str(e.value) == 'o must be a contiguous %s tensor of shape (2, 3) on %s' % (dtype, dev)


def test_out_flat():
  for ok in (torch.zeros(6), torch.zeros(3, 2), torch.zeros(4, 6)[1:2]):
    assert _call.out(ok, CPU, torch.float32, (2, 3), 'o', flat=True) is ok
  for bad in (torch.zeros(7), torch.zeros(3, 2).t(), torch.zeros(6, dtype=torch.int32)):
    with pytest.raises(ValueError) as e:
      _call.out(bad, CPU, torch.float32, (2, 3), 'o', flat=True)
    assert str(e.value) == ('o must be a contiguous torch.float32 tensor of shape (2, 3) on cpu')


def test_out_rows():
  for ok in (torch.zeros(5, 3), torch.zeros(2, 5, 8)[..., :3], torch.zeros(3, 5).t()[:, :3]):
    assert _call.out(ok, CPU, torch.float32, (10, 3), 'o', rows=True) is ok   # rows() judges it
  for bad in (torch.zeros(5, 4), torch.zeros(5, 3, dtype=torch.float64)):
    with pytest.raises(ValueError) as e:
      _call.out(bad, CPU, torch.float32, (10, 3), 'o', rows=True)
    assert str(e.value) == 'o must be a torch.float32 tensor of shape [..., 3] on cpu'


# ------------------------------------------------------------------ workspace ---
@pytest.mark.parametrize('nbytes,dtype,numel', [
    (0, None, 1), (1, None, 1), (8, None, 1), (9, None, 2), (64, None, 8),
    (9, torch.float32, 3), (12, torch.float32, 3), (0, torch.float32, 1)])
def test_workspace_allocates_the_bytes_rounded_up(nbytes, dtype, numel):
  t = _call.workspace(None, CPU, nbytes, dtype)
  assert t.shape == (numel,) and t.dtype == (dtype or torch.int64) and t.device == CPU


def test_workspace_given():
  ws = torch.zeros(4, dtype=torch.int64)                           # 32 bytes
  assert _call.workspace(ws, CPU, 32) is ws                        # the exact size
  assert _call.workspace(ws, CPU, 32, torch.int64) is ws
  assert _call.workspace(torch.zeros(8, dtype=torch.float32), CPU, 32) is not None   # any dtype
  with pytest.raises(ValueError) as e:
    _call.workspace(ws, CPU, 33)                                   # one byte short
  assert str(e.value) == 'workspace must be a contiguous tensor of at least 33 bytes on cpu'
  with pytest.raises(ValueError) as e:
    _call.workspace(ws, CPU, 32, torch.float32)
  assert str(e.value) == ('workspace must be a contiguous torch.float32 tensor of at least 32 '
                          'bytes on cpu')
  for bad, dev in ((torch.zeros(8, dtype=torch.int64)[::2], CPU), (ws, META)):
    with pytest.raises(ValueError):
      _call.workspace(bad, dev, 32)


# ---------------------------------------------------------------------- dense ---
# The texts of the call sites that go through dense(); they refuse a host tensor first, so the
# messages are produced through the helper. loss_grads' out[k] and decoder_train's absmax slots
# word theirs differently and keep their checks inline.
def test_dense_messages_of_its_call_sites():
  f32, f64 = torch.zeros(6), torch.zeros(2, 3, dtype=torch.float64)
  _call.dense(f32, CPU, torch.float32, 'grad', numel=6, name='float32')
  _call.dense(f64, CPU, torch.float64, 'sums', numel=6)
  _call.dense(f32, CPU, torch.float32, 'gamma', shape=(6,), name='float32')
  with pytest.raises(ValueError) as e:                             # heads_train.momentum_step
    _call.dense(f32, CPU, torch.float32, 'grad', numel=7, name='float32')
  assert str(e.value) == 'grad must be a contiguous float32 tensor of 7 values on cpu'
  with pytest.raises(ValueError) as e:                             # loss.loss_values
    _call.dense(f64, CPU, torch.float64, 'scales', numel=9)
  assert str(e.value) == 'scales must be a contiguous torch.float64 tensor of 9 values on cpu'
  with pytest.raises(ValueError) as e:                             # decoder_train, bn
    _call.dense(f32, CPU, torch.float32, 'moving_mean', shape=(5,), name='float32')
  assert str(e.value) == 'moving_mean must be a contiguous float32 tensor of shape (5,) on cpu'


@pytest.mark.parametrize('t,device,dtype', [
    (torch.zeros(3, 2).t(), CPU, torch.float32),                   # not contiguous
    (torch.zeros(2, 3), META, torch.float32),                      # another device
    (torch.zeros(2, 3), CPU, torch.float64),                       # another dtype
    (torch.zeros(3, 2), CPU, torch.float32)])                      # another shape
def test_dense_refuses(t, device, dtype):
  with pytest.raises(ValueError):
    _call.dense(t, device, dtype, 'x', shape=(2, 3))
  if tuple(t.shape) != (2, 3) or not t.is_contiguous():
    return
  with pytest.raises(ValueError):
    _call.dense(t, device, dtype, 'x', numel=6)


# --------------------------------------------------------------------- launch ---
class _Kept(object):
  def __init__(self):
    self.recorded = []

  def record_stream(self, stream):
    self.recorded.append(stream)


class _Stream(object):
  cuda_stream = 0x1234


@pytest.fixture
def no_device(monkeypatch):
  """launch() as product code builds it, with torch's current stream and device guard replaced:
  the bookkeeping runs without a device."""
  stream, entered = _Stream(), []

  @contextlib.contextmanager
  def guard(device):
    entered.append(device)
    yield
    entered.append('left')
  monkeypatch.setattr(torch.cuda, 'current_stream', lambda device=None: stream)
  monkeypatch.setattr(torch.cuda, 'device', guard)
  return stream, entered


def test_launch_records_what_it_keeps_once(no_device):
  stream, entered = no_device
  a, b = _Kept(), _Kept()
  with _call.launch('dev') as q:
    assert q.stream is stream and q.handle.value == 0x1234 and entered == ['dev']
    q.keep(a, None)
    q.keep(None, b)
    assert a.recorded == [] and b.recorded == []
  assert a.recorded == [stream] and b.recorded == [stream] and entered == ['dev', 'left']


def test_launch_records_when_the_body_raises(no_device):
  stream, entered = no_device
  a = _Kept()
  with pytest.raises(KeyError):
    with _call.launch('dev') as q:
      q.keep(a)
      raise KeyError('refused')
  assert a.recorded == [stream] and entered[0] == 'dev'


def test_need_device():
  with pytest.raises(EposError) as e:
    _call.need_device(torch.zeros(1), 'x needs a HIP device (there is no CPU fallback)')
  assert str(e.value) == 'x needs a HIP device (there is no CPU fallback)'
  if not torch.cuda.is_available():
    with pytest.raises(EposError):
      _call.need_device(None, 'y')
