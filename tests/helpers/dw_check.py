"""One depthwise 3x3 problem of tests/helpers/dw_regimes.py run through
epos_depthwise3x3_f32 and checked against float64 (shared by tests/test_gpu_depthwise.py
and the child processes it starts under the EPOS_DW_* switches)."""
import ctypes
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from helpers import dw_regimes as dr

SENTINEL = 0x7fa5a5a5          # a NaN bit pattern no computed value has
EPS32 = 2.0 ** -20             # per-element bound: 9 fmas + the bias, in units of the sums


def _p(t, off=0):
  return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def problem(s):
  rng = np.random.RandomState(zlib.crc32(s.name.encode()) & 0x7fffffff)
  x = rng.standard_normal((s.b, s.hi, s.wi, s.c)).astype(np.float32)
  w9c = (rng.standard_normal((9, s.c)) * 0.5).astype(np.float32)
  bias = rng.standard_normal(s.c).astype(np.float32)
  return x, w9c, bias


def reference(s, x, w9c, bias):
  """fp64 outputs by relu_in (0, 1) and the per-element error bound
  2^-20 (conv(|x|, |w|) + |bias|), which covers every (relu_in, relu_out) variant: ReLU is
  1-Lipschitz and |relu(x)| <= |x|."""
  pad = s.rate if s.stride == 1 else 1      # SAME, resp. fixed_padding + VALID
  w = torch.from_numpy(w9c).double().t().reshape(s.c, 1, 3, 3)
  xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).contiguous()
  b64 = torch.from_numpy(bias).double()

  def conv(v, k, bb):
    return F.conv2d(v, k, bb, stride=s.stride, padding=pad, dilation=s.rate,
                    groups=s.c).permute(0, 2, 3, 1).contiguous().numpy()
  refs = {0: conv(xt, w, b64), 1: conv(F.relu(xt), w, b64)}
  return refs, EPS32 * conv(xt.abs(), w.abs(), b64.abs())


def expected(refs, relu_in, relu_out):
  r = refs[relu_in]
  return np.maximum(r, 0) if relu_out else r


def launch(lib, s, x, w9c, bias, relu_in, relu_out, h2=None):
  """Runs the kernel; returns Y's (b, ho, wo, ldy) float32 view. X's padding columns hold
  NaN (a read of them would show in the output); Y starts as SENTINEL everywhere, with one
  spare image row of ldy-float pixels behind the output, and the padding columns and spare
  row are checked untouched. h2 = (slot, slot2, gain, bias0): fp16-pair output."""
  from epos_amd import _lib
  ho, wo = dr.out_size(s.hi, s.wi, s.stride)
  nx = s.b * s.hi * s.wi * s.ldx
  ny = s.b * ho * wo * s.ldy
  spare = (wo + 1) * s.ldy
  Xb = torch.full((s.off + nx,), float('nan'), device='cuda')
  Xb[s.off:].view(s.b, s.hi, s.wi, s.ldx)[..., :s.c] = torch.from_numpy(x).cuda()
  Yb = torch.full((s.off + ny + spare,), SENTINEL, dtype=torch.int32, device='cuda')
  # the mirror's alignment assumption: the caching allocator hands out line-aligned blocks
  assert Xb.data_ptr() % 128 == 0 and Yb.data_ptr() % 128 == 0
  Wd, Bd = torch.from_numpy(w9c).cuda(), torch.from_numpy(bias).cuda()
  args = _lib.DepthwiseArgs(X=_p(Xb, s.off), ldx=s.ldx, w9c=_p(Wd), bias=_p(Bd),
                            Y=_p(Yb, s.off), ldy=s.ldy, B=s.b, Hi=s.hi, Wi=s.wi, Ho=ho, Wo=wo,
                            C=s.c, stride=s.stride, rate=s.rate, relu_in=relu_in,
                            relu_out=relu_out)
  if h2 is not None:
    slot, slot2, gain, bias0 = h2
    args.y_h2, args.x_amax, args.x_amax2 = 1, _p(slot), _p(slot2)
    args.gain, args.bias0 = gain, bias0
  _lib.check(lib.epos_depthwise3x3_f32(ctypes.byref(args), None), 'depthwise', lib=lib)
  torch.cuda.synchronize()
  raw = Yb.cpu().numpy()
  assert (raw[:s.off] == SENTINEL).all() and (raw[s.off + ny:] == SENTINEL).all(), \
      'write past the output'
  out = raw[s.off:s.off + ny].reshape(s.b, ho, wo, s.ldy)
  assert (out[..., s.c:] == SENTINEL).all(), 'write into the padding columns'
  return np.ascontiguousarray(out[..., :s.c]).view(np.float32)


def check_fp32(lib, s, relu_in, relu_out, prob=None, refs=None):
  """One launch checked against fp64 and for stray writes; returns the fp32 output.
  prob = problem(s), refs = reference(s, *prob) when the caller has them already."""
  x, w9c, bias = prob or problem(s)
  y = launch(lib, s, x, w9c, bias, relu_in, relu_out)
  refs, tol = refs or reference(s, x, w9c, bias)
  ref = expected(refs, relu_in, relu_out)
  bad = ~(np.abs(y.astype(np.float64) - ref) <= tol)
  assert not bad.any(), '%s relu_in=%d relu_out=%d: %d elements off, first at %s (%r vs %r)' % (
      s.name, relu_in, relu_out, bad.sum(), np.argwhere(bad)[0], y[bad][0], ref[bad][0])
  return y


def switch_outputs(lib):
  """fp64-checked outputs of the switch problems (one relu variant each), by name."""
  variants = [(0, 0), (1, 0), (0, 1)]
  return {s.name: check_fp32(lib, s, *variants[i % 3])
          for i, s in enumerate(dr.SWITCH_SHAPES)}
