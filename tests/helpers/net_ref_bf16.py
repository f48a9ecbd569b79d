"""Test oracle for the bf16 plan (EposNet(precision='bf16')): oracle/net_ref.py's primitives,
wrapped (not edited) so that the torch restatement rounds to bf16 exactly where the plan stores a
bf16 value, and takes bf16 weights where the plan does. Run under
net_ref.precision(torch.float64), everything between two rounding points is carried out in
double; the difference to a plain float64 run is then the bf16 error the mode's definition
allows, and the GPU plan is held to a multiple of it.

Storage points of the plan ("bf16 mode"), as the wrappers restate them:
  * every conv / depthwise conv / 1x1 GEMM reads bf16: conv2d_raw and depthwise_raw round their
    input (rounding is idempotent, so a value that was already stored rounds to itself) --
    except the image-pooling 1x1, which reads the fp32 mean;
  * a GEMM's epilogue adds its residual before it rounds: add() keeps the fused operand (the
    batch-norm output of the layer that owns the residual) unrounded and rounds the other one;
    the ResNet unit whose conv3 is the decoder tap stores conv3 first (separate add + ReLU);
  * resize, max-pool, subsample, concat and the global mean read bf16 (the image-pooling
    broadcast reads the fp32 1x1 output);
  * weights: BN folded in float32 (as weights.fold_bn / Bf16Mode._weights), rounded to bf16,
    re-expressed in the unfolded checkpoint (w' = bf16(w * scale) / scale in float64); the logits
    weights rounded as they are; depthwise and image-pooling weights stay fp32;
  * the logits are not rounded (fp32 heads).
"""
import contextlib

import numpy as np
import torch

from oracle import net_ref

from helpers.bf16_ref import bf16_round

_TAP_CONV3 = '/block1/unit_2/bottleneck_v1/conv3'      # stored before its add (net.py keep_conv3)


def R(x):
  """bf16 round to nearest even of a float tensor (via float32), in x's dtype."""
  u = x.float().contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
  nan = (u & 0x7fffffff) > 0x7f800000
  r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
  r = torch.where(nan, u | 0x400000, r)
  r = r & 0xffffffff
  r = torch.where(r >= 2 ** 31, r - 2 ** 32, r).to(torch.int32)
  return r.view(torch.float32).to(x.dtype)


def bf16_checkpoint(wts):
  """The checkpoint whose float64 forward multiplies by the plan's bf16 weights."""
  out = dict(wts)
  for key, w in wts.items():
    if not key.endswith('/weights') or key.startswith('image_pooling'):
      continue
    scope = key[:-len('/weights')]
    if key.startswith('logits/'):
      out[key] = bf16_round(w.astype(np.float32)).astype(np.float64)
      continue
    if scope + '/BatchNorm/gamma' not in wts:
      continue
    eps = 1e-3 if scope.startswith('xception') else 1e-5
    g = wts[scope + '/BatchNorm/gamma'].astype(np.float64)
    v = wts[scope + '/BatchNorm/moving_variance'].astype(np.float64)
    scale = (g / np.sqrt(v + eps)).astype(np.float32)
    folded = bf16_round(w.astype(np.float32) * scale).astype(np.float64)
    out[key] = folded / scale.astype(np.float64)
  return out


@contextlib.contextmanager
def emulate_bf16():
  """Inside: net_ref (and helpers that call its primitives through the module) round to bf16
  at the plan's storage points."""
  nr = net_ref
  orig = {k: getattr(nr, k) for k in ('conv2d_raw', 'depthwise_raw', 'batch_norm', 'add',
                                      'concat', 'resize_bilinear_align_corners',
                                      'max_pool_3x3_s2_same', 'subsample', 'aspp')}

  def conv2d_raw(x, w, stride=1, rate=1, padding='SAME', scope=None):
    if scope != 'image_pooling':
      x = R(x)
    return orig['conv2d_raw'](x, w, stride, rate, padding, scope)

  def depthwise_raw(x, w, stride=1, rate=1, padding='SAME', scope=None):
    return orig['depthwise_raw'](R(x), w, stride, rate, padding, scope)

  def batch_norm(x, wts, scope, eps):
    y = orig['batch_norm'](x, wts, scope, eps)
    y._bf16_bn_scope = scope
    return y

  def fused(t):
    s = getattr(t, '_bf16_bn_scope', None)
    if s is None:
      return False
    return s.endswith('separable_conv3_pointwise') or (
        s.endswith('/conv3') and not s.endswith(_TAP_CONV3))

  def add(a, b):
    return orig['add'](a if fused(a) else R(a), b if fused(b) else R(b))

  def concat(ts):
    return orig['concat']([R(t) for t in ts])

  def resize(x, size_hw):
    if (int(x.shape[2]), int(x.shape[3])) != (1, 1):     # the image-pooling broadcast: fp32
      x = R(x)
    return orig['resize_bilinear_align_corners'](x, size_hw)

  def max_pool(x):
    return orig['max_pool_3x3_s2_same'](R(x))

  def subsample(x, factor):
    return orig['subsample'](R(x), factor)

  def aspp(features, wts, atrous_rates, end_points):
    return orig['aspp'](R(features), wts, atrous_rates, end_points)

  patched = {'conv2d_raw': conv2d_raw, 'depthwise_raw': depthwise_raw,
             'batch_norm': batch_norm, 'add': add, 'concat': concat,
             'resize_bilinear_align_corners': resize, 'max_pool_3x3_s2_same': max_pool,
             'subsample': subsample, 'aspp': aspp}
  try:
    for k, f in patched.items():
      setattr(nr, k, f)
    yield
  finally:
    for k, f in orig.items():
      setattr(nr, k, f)
