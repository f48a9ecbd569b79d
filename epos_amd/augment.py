"""The reference's training-time image augmentations on the device (csrc/augment.hip;
include/epos_hip.h, "Augmentation"; DESIGN.md, "Losses", "Augmentation").

  parse      the reference's data_augmentations flag ("a string containing a dictionary in the
             YAML format", train.py:156-159) -> an ordered list of (name, params), validated.
  draw       the drawn values of image b of training step `step`: a counter-based draw keyed
             by (seed, step, b), so a resumed run draws what an uninterrupted one would.
  Augmenter  .ops(step, B): the table epos_augment_f32 takes; .apply(images, step): in place
             on a float32 device tensor [B,H,W,3], enqueued on the current stream.

The ops run in the order of the mapping, as datagen.py:636 iterates it. Unlike the reference,
which skips a name it does not know, parse refuses it: a typo must not switch augmentation off.
Pinned to tests/helpers/augment_ref.py (numpy, fp64) and, for the JPEG round trip, to PIL;
parity with TensorFlow's image ops, cv2.GaussianBlur, cv2.randn's stream and libjpeg's integer
DCT is unpinned (docs/next_rows.md). There is no CPU fallback.
"""
import ctypes

import numpy as np

from epos_amd import _call as C
from epos_amd import _lib

NONE, BRIGHTNESS, CONTRAST, SATURATION, HUE, BLUR, NOISE, JPEG = range(8)
MAX_OPS = 8
MAX_BLUR_RADIUS = 32

# name -> (kind, the reference's parameter keys)
OPS = {
    'random_adjust_brightness': (BRIGHTNESS, ('min_delta', 'max_delta')),
    'random_adjust_contrast': (CONTRAST, ('min_delta', 'max_delta')),
    'random_adjust_saturation': (SATURATION, ('min_delta', 'max_delta')),
    'random_adjust_hue': (HUE, ('max_delta',)),
    'random_blur': (BLUR, ('max_sigma',)),
    'random_gaussian_noise': (NOISE, ('max_sigma',)),
    'jpeg_artifacts': (JPEG, ('min_quality',)),
}

# EposAugmentOp
OP_DTYPE = np.dtype([('kind', np.int32), ('a', np.float32), ('b', np.float32),
                     ('key_lo', np.uint32), ('key_hi', np.uint32)])


def blur_radius(sigma):
  """(ksize - 1) / 2 with ksize = round_half_even(8 sigma + 1) | 1, what
  cv2.GaussianBlur(img, (0, 0), sigma) takes for a float32 image; sigma as a float32."""
  return ((int(round(float(np.float32(sigma)) * 8.0 + 1.0)) | 1) - 1) // 2


def parse(spec):
  """data_augmentations as the flag or params.yml gives it -> [(name, {key: value})] in the
  order of the mapping. None, '', 'None' and {} mean no augmentation. A value that is not a
  mapping raises NotImplementedError; an unknown name, a missing key, min > max, a max_sigma
  whose blur radius exceeds 32 and a min_quality outside [1, 99] raise ValueError."""
  if spec is None or (isinstance(spec, (str, list, dict)) and len(spec) == 0) or spec == 'None':
    return []
  if isinstance(spec, str):
    import yaml
    spec = yaml.safe_load(spec)
    if spec is None:
      return []
  if not isinstance(spec, dict):
    raise NotImplementedError(
        'data_augmentations=%r: expected a mapping {name: {parameter: value}} in the YAML '
        'format' % (spec,))
  if len(spec) > MAX_OPS:
    raise ValueError('data_augmentations: %d entries, at most %d' % (len(spec), MAX_OPS))
  out = []
  for name, params in spec.items():
    if name not in OPS:
      raise ValueError('data_augmentations: unknown augmentation %r (known: %s)' % (
          name, ', '.join(sorted(OPS))))
    keys = OPS[name][1]
    if not isinstance(params, dict):
      raise ValueError('data_augmentations: %s needs a mapping with %s' % (
          name, ', '.join(keys)))
    vals = {}
    for k in keys:
      if k not in params:
        raise ValueError('data_augmentations: %s lacks %s' % (name, k))
      try:
        vals[k] = float(params[k])
      except (TypeError, ValueError):
        raise ValueError('data_augmentations: %s: %s=%r is not a number' % (
            name, k, params[k]))
      if not np.isfinite(vals[k]):
        raise ValueError('data_augmentations: %s: %s=%r is not finite' % (name, k, params[k]))
    unknown = sorted(set(params) - set(keys))
    if unknown:
      raise ValueError('data_augmentations: %s does not take %s' % (name, ', '.join(unknown)))
    if 'min_delta' in vals and vals['min_delta'] > vals['max_delta']:
      raise ValueError('data_augmentations: %s: min_delta %g > max_delta %g' % (
          name, vals['min_delta'], vals['max_delta']))
    if name == 'random_adjust_hue' and vals['max_delta'] < 0:
      raise ValueError('data_augmentations: %s: max_delta %g < 0' % (name, vals['max_delta']))
    if 'max_sigma' in vals and vals['max_sigma'] < 0:
      raise ValueError('data_augmentations: %s: max_sigma %g < 0' % (name, vals['max_sigma']))
    if name == 'random_blur' and blur_radius(vals['max_sigma']) > MAX_BLUR_RADIUS:
      raise ValueError('data_augmentations: %s: max_sigma %g gives a blur radius of %d, at '
                       'most %d' % (name, vals['max_sigma'], blur_radius(vals['max_sigma']),
                                    MAX_BLUR_RADIUS))
    if name == 'jpeg_artifacts':
      q = vals['min_quality']
      if q != int(q) or not 1 <= q <= 99:
        raise ValueError('data_augmentations: %s: min_quality %g must be an integer in '
                         '[1, 99]' % (name, q))
      vals['min_quality'] = int(q)
    out.append((name, vals))
  return out


def draw(ops, seed, step, b):
  """The drawn values of image b of training step `step`: one EposAugmentOp record per entry
  of ops (parse's list), in its order. Uniform in [min_delta, max_delta]; [-max_delta,
  max_delta] for hue; [0, max_sigma] for the sigmas; an integer in [min_quality, 100) for
  JPEG; two uint32 for the noise key. A numpy Philox generator keyed by (seed, step, b), as
  tfrecord.crop_offsets keys its draw: TensorFlow's and Python's random streams cannot be
  reproduced, the distributions are the reference's."""
  rng = np.random.Generator(np.random.Philox(key=[
      int(seed) & 0xffffffffffffffff,
      ((int(step) & 0xffffffff) << 32) | (int(b) & 0xffffffff)]))
  table = np.zeros(len(ops), OP_DTYPE)
  for rec, (name, p) in zip(table, ops):
    kind = OPS[name][0]
    rec['kind'] = kind
    if kind in (BRIGHTNESS, CONTRAST, SATURATION):
      rec['a'] = _inside(rng.uniform(p['min_delta'], p['max_delta']), p['min_delta'],
                         p['max_delta'])
    elif kind == HUE:
      rec['a'] = _inside(rng.uniform(-p['max_delta'], p['max_delta']), -p['max_delta'],
                         p['max_delta'])
    elif kind in (BLUR, NOISE):
      rec['a'] = _inside(rng.uniform(0.0, p['max_sigma']), 0.0, p['max_sigma'])
      if kind == NOISE:
        rec['key_lo'], rec['key_hi'] = (int(v) for v in rng.integers(0, 1 << 32, 2,
                                                                     dtype=np.uint64))
    else:
      rec['a'] = int(rng.integers(p['min_quality'], 100))
  return table


def _inside(x, lo, hi):
  """x as a float32 that lies inside [lo, hi] (rounding to float32 may step over an end)."""
  v = np.float32(x)
  if v < lo:
    v = np.nextafter(v, np.float32(np.inf), dtype=np.float32)
  if v > hi:
    v = np.nextafter(v, np.float32(-np.inf), dtype=np.float32)
  return v


class Augmenter(object):
  """spec: what parse takes (or its list). apply(images, step) augments a batch in place."""

  def __init__(self, spec, seed=0, device=None):
    self.entries = spec if isinstance(spec, list) else parse(spec)
    self.seed = int(seed)
    self.device = device
    self._work = None

  @property
  def names(self):
    return [name for name, _ in self.entries]

  def ops(self, step, B):
    """The table of training step `step`: EposAugmentOp records [B, n_ops]."""
    table = np.zeros((B, len(self.entries)), OP_DTYPE)
    for b in range(B):
      table[b] = draw(self.entries, self.seed, step, b)
    return table

  def apply(self, images, step):
    """images: float32 device tensor [B,H,W,3] in [0,255], contiguous; augmented in place with
    the draws of training step `step`. Enqueues on the current stream; does not synchronise."""
    B = int(images.shape[0])
    self._work = apply_ops(images, self.ops(step, B), self._work)
    return images


def apply_ops(images, table, workspace=None):
  """epos_augment_f32 on images (float32 device tensor [B,H,W,3], contiguous, in place) with
  table = EposAugmentOp records [B, n_ops]. workspace: an int64 device tensor to reuse when it
  is large enough. Returns the workspace used. Enqueues on the current stream."""
  import torch
  lib = _lib.load()
  C.need_device(images, 'augmentation needs a HIP device (there is no CPU fallback)')
  if images.dtype != torch.float32 or images.dim() != 4 or images.shape[3] != 3 or \
      not images.is_contiguous():
    raise ValueError('images must be a contiguous float32 tensor [B,H,W,3], got %s %s' % (
        images.dtype, tuple(images.shape)))
  B, h, w = (int(v) for v in images.shape[:3])
  table = np.ascontiguousarray(table, OP_DTYPE)
  if table.ndim != 2 or table.shape[0] != B:
    raise ValueError('the op table must be [B=%d, n_ops], got %s' % (B, table.shape))
  n_ops = int(table.shape[1])
  dev = images.device
  nbytes = _lib.check(lib.epos_augment_workspace_bytes(B, h, w), 'epos_augment_workspace_bytes')
  ws = workspace
  if ws is None or ws.device != dev or ws.numel() * ws.element_size() < nbytes:
    ws = C.workspace(None, dev, nbytes)     # a small or foreign one is replaced, not refused
  with C.launch(dev) as q:
    q.keep(ws)
    _lib.check(lib.epos_augment_f32(
        C.ptr(images), B, h, w, ctypes.c_void_p(table.ctypes.data), n_ops, C.ptr(ws), q.handle),
               'epos_augment_f32')
  return ws
