"""The depthwise 3x3 kernel in every launch regime against float64, plus the sparse-head
softmax (epos_softmax_slots_f32) and the uint8 frame cast (epos_u8_to_f32).

The regimes -- generic / sliding-window kernel, one or two rows per thread, channel slices
or row bands, slice unit, slice widths, dilation residues -- are chosen on the host
(epos_amd/csrc/layers.hip, epos_depthwise3x3_f32); tests/helpers/dw_regimes.py restates that
choice and holds the shape table, and tests/test_depthwise_regimes.py checks without a GPU
that the table reaches each of them. Everything here runs the PRODUCT library (_lib.load(),
which honours EPOS_HIP_LIB: a variant build is tested by pointing it there)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import dw_check as dc
from helpers import dw_regimes as dr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELU = [(0, 0), (1, 0), (0, 1)]


@pytest.fixture(scope='module')
def lib():
  from epos_amd import _lib
  assert torch.cuda.is_available(), 'GPU tests need a HIP device'
  return _lib.load()


def _p(t, off=0):
  return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _id(s):
  r = dr.shape_regime(s)
  if r.kernel == 'generic':
    return '%s-generic' % s.name
  return '%s-rows%d-mode%d' % (s.name, r.rows, r.mode)


# ------------------------------------------------------------ depthwise vs fp64 ---
@pytest.mark.parametrize('s', dr.SHAPES, ids=_id)
def test_depthwise_regime_against_fp64(lib, s):
  """Each (relu_in, relu_out) variant within 2^-20 (conv(|x|, |w|) + |bias|) of float64 per
  element; nothing written outside the output (padding columns, the row behind it)."""
  prob = dc.problem(s)
  refs = dc.reference(s, *prob)
  for relu_in, relu_out in RELU:
    dc.check_fp32(lib, s, relu_in, relu_out, prob, refs)


H2_SHAPES = ['c728_r1_ld736_b2', 'c728_r2_ld736_tiny', 'c128_r3_b3_band', 'c264_r5_b3',
             'c728_r12_rate_gt_wo', 's2_c256']


@pytest.mark.parametrize('s', [s for s in dr.SHAPES if s.name in H2_SHAPES], ids=_id)
def test_depthwise_fp16_pair_output_against_fp64(lib, s):
  """y_h2 with two absmax slots, the second holding the larger bound: the scale is that of
  max(x_amax, x_amax2). Decoded, the pairs are the fp32 launch's values to 2^-22 relative
  (above 2^-26 of the bound) and fp64's within the fp32 bound plus that term."""
  x, w9c, bias = dc.problem(s)
  relu_in, relu_out = 1, 0
  amax = float(np.abs(x).max())
  slot = torch.zeros(64, dtype=torch.int32, device='cuda')
  slot2 = torch.zeros(64, dtype=torch.int32, device='cuda')
  slot[3] = int(np.float32(amax / 64).view(np.int32))      # too small: its scale overflows
  slot2[17] = int(np.float32(amax).view(np.int32))
  gain = float(np.abs(w9c.astype(np.float64)).sum(0).max())
  bias0 = float(np.abs(bias).max())
  refs, tol = dc.reference(s, x, w9c, bias)
  y32 = dc.check_fp32(lib, s, relu_in, relu_out, (x, w9c, bias), (refs, tol)).astype(np.float64)
  out = dc.launch(lib, s, x, w9c, bias, relu_in, relu_out, h2=(slot, slot2, gain, bias0))
  ho, wo = y32.shape[1:3]
  raw = out.view(np.float16).reshape(s.b, ho, wo, s.c // 4, 2, 4)
  hi16, mid16 = raw[..., 0, :].astype(np.float64), raw[..., 1, :].astype(np.float64)
  bound = gain * amax + bias0
  sc = 2.0 ** (14 - np.floor(np.log2(bound)))
  dec = ((hi16 + mid16 / 2048.0) / sc).reshape(s.b, ho, wo, s.c)
  big = np.abs(y32) >= 2.0 ** -26 * bound
  d = np.abs(dec - y32)
  assert (d[big] <= 2.0 ** -22 * np.abs(y32)[big]).all(), 'pairs vs the fp32 launch'
  assert (d[~big] <= 2.0 ** -49 * bound).all(), 'pairs vs the fp32 launch (small values)'
  ref = dc.expected(refs, relu_in, relu_out)
  assert (np.abs(dec - ref) <= tol + 2.0 ** -22 * np.abs(y32) + 2.0 ** -49 * bound).all()


# ----------------------------------------------- the same values in every regime ---
_CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, 'tests'))
from epos_amd import _lib
from helpers import dw_check
for name, y in dw_check.switch_outputs(_lib.load()).items():
  np.save(os.path.join(%(out)r, name + '.npy'), y)
print('ok')
'''


@pytest.fixture(scope='module')
def default_switch_outputs(lib):
  return dc.switch_outputs(lib)


@pytest.mark.parametrize('env', dr.SWITCHES, ids=lambda e: '%s=%s' % next(iter(e.items())))
def test_depthwise_switches_give_equal_values(env, default_switch_outputs, tmp_path,
                                              gpu_children):
  """Every s1 regime computes an output by the same fma chain (bias, then ky, then kx), so
  the process-wide switches (read once per process: a child each, which also checks fp64)
  give the default run's values exactly. Compared with ==: a skipped tap and a zero tap may
  leave zeros of different sign."""
  script = _CHILD % {'root': ROOT, 'out': str(tmp_path)}
  r = subprocess.run([sys.executable, '-c', script], env=dict(os.environ, **env),
                     capture_output=True, text=True, timeout=300)
  assert r.returncode == 0 and 'ok' in r.stdout, r.stdout + r.stderr
  for s in dr.SWITCH_SHAPES:
    got = np.load(str(tmp_path / (s.name + '.npy')))
    want = default_switch_outputs[s.name]
    assert got.shape == want.shape
    neq = ~(got == want)
    assert not neq.any(), '%s: %d values differ, first at %s' % (
        s.name, neq.sum(), np.argwhere(neq)[0])


# ------------------------------------------------------------ sparse-head softmax ---
SLOTS = [(0, 2), (1, 1), (1, 4), (0, 5)]      # (image, obj_id): both images, objects 1-5 gapped


def _softmax_kernel(f, off):
  """The rule of epos_softmax_slots_f32: F = 64 on a 16-byte aligned X takes the
  16-lanes-per-group kernel, everything else the generic one."""
  return 'slots64' if f == 64 and (4 * off) % 16 == 0 else 'generic'


@pytest.mark.parametrize('f,off', [
    pytest.param(f, off, id='F%d-off%d-%s' % (f, off, _softmax_kernel(f, off)))
    for f, off in [(1, 0), (7, 0), (32, 0), (63, 0), (64, 0), (64, 1)]])
def test_softmax_slots_against_fp64(lib, f, off):
  from epos_amd import _lib
  kernel = _softmax_kernel(f, off)
  b, o, p = 2, 5, 203
  rng = np.random.RandomState(f * 10 + off)
  x = (rng.standard_normal((b, p, o, f)) * 3).astype(np.float32)
  x[0, 7, 1] = np.where(np.arange(f) % 2, 80.0, -80.0)   # slot (0, 2): logits of +-80
  x[1, 8, 3] = -80.0
  x[1, 8, 3, f // 2] = 80.0
  x[1, 11, 0] = 1.25                                      # slot (1, 1): an exact tie
  x[0, 12, 4, : (f + 1) // 2] = 2.5                       # slot (0, 5): a tied maximum
  # one group more than the tensor, so that the view at `off` floats stays inside
  buf = torch.full((x.size + f,), 123.0, device='cuda')
  buf[off:off + x.size] = torch.from_numpy(x.ravel()).cuda()
  slots = torch.tensor(SLOTS, dtype=torch.int32, device='cuda')
  _lib.check(lib.epos_softmax_slots_f32(_p(buf, off), _p(slots), len(SLOTS), p, o, f, None),
             'softmax_slots (%s kernel)' % kernel, lib=lib)
  torch.cuda.synchronize()
  got = buf.cpu().numpy()
  assert (got[:off] == 123.0).all() and (got[off + x.size:] == 123.0).all()
  got = got[off:off + x.size].reshape(b, p, o, f)
  ref = torch.softmax(torch.from_numpy(x).double(), dim=-1).numpy()
  for img in range(b):
    for obj in range(1, o + 1):
      g, xs = got[img, :, obj - 1], x[img, :, obj - 1]
      if (img, obj) in SLOTS:
        np.testing.assert_allclose(g, ref[img, :, obj - 1], rtol=2e-6, atol=1e-7,
                                   err_msg='%s kernel, slot %s' % (kernel, (img, obj)))
        sums = g.astype(np.float64).sum(-1)
        assert (np.abs(sums - 1) <= 64 * 2.0 ** -24).all(), (kernel, (img, obj))
      else:
        assert np.array_equal(g.view(np.uint32), xs.view(np.uint32)), (kernel, (img, obj))


# ---------------------------------------------------------------- uint8 -> fp32 ---
@pytest.mark.parametrize('src', ['device', 'pinned'])
@pytest.mark.parametrize('n', [16, 17, 31, 4096 + 5, 3 * 480 * 640])
def test_u8_to_f32_is_exact(lib, n, src):
  """The cast of infer.py's frames: 16 values per thread, a scalar tail for n % 16; from
  device memory and from a pinned host tensor (the zero-copy path of net.set_images)."""
  from epos_amd import _lib
  rng = np.random.RandomState(n)
  x = rng.randint(0, 256, n).astype(np.uint8)
  x[:2] = (0, 255)
  x[-2:] = (255, 1)
  X = torch.from_numpy(x)
  X = X.cuda() if src == 'device' else X.pin_memory()
  assert X.data_ptr() % 16 == 0
  pad = 37
  Y = torch.full((n + pad,), dc.SENTINEL, dtype=torch.int32, device='cuda')
  _lib.check(lib.epos_u8_to_f32(_p(X), _p(Y), n, None), 'u8_to_f32', lib=lib)
  torch.cuda.synchronize()
  y = Y.cpu().numpy()
  assert np.array_equal(y[:n].view(np.float32), x.astype(np.float32))
  assert (y[n:] == dc.SENTINEL).all()


def test_u8_to_f32_refuses_misaligned_buffers(lib):
  """The host check rejects a base that is not 16-byte aligned before anything launches."""
  X = torch.zeros(64, dtype=torch.uint8, device='cuda')
  Y = torch.zeros(64, device='cuda')
  assert lib.epos_u8_to_f32(_p(X, 1), _p(Y), 32, None) < 0
  assert lib.epos_u8_to_f32(_p(X), _p(Y, 1), 32, None) < 0
  torch.cuda.synchronize()
  assert (Y.cpu() == 0).all()
