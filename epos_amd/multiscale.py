"""Multi-scale inference (``image_pyramid`` + ``merge_method``, model.py:515-626) for MI355X.

``MultiScaleNet`` holds one ``EposNet`` plan per scale of the pyramid, each at its own input
size, and runs them one after the other on the caller's stream:

  1. for every scale s != 1.0 the full-size image is resized to
     (scale_dimension(H, s), scale_dimension(W, s)) by ``tf.image.resize_bilinear
     (align_corners=True)`` (model.py:569-573, misc.py:94-107) into that plan's input buffer;
  2. the plan runs WITHOUT its softmax / argmax post-ops (the raw logits). For s != 1.0 the
     reference hands get_logits crop_size = [scaled_height, scaled_width] (model.py:572,581),
     which the decoder reads as [width, height] (model.py:355-356): its two inputs are resized
     to (scale_dimension(w_s, 1/4), scale_dimension(h_s, 1/4)) -- 120x90 for a 360x480 input --
     and the plan's decoder does the same (EposNet(decoder_hw=...));
  3. per head one epos_resize_merge_f32 launch resizes the logits of every scale to the merged
     size (Lh, Lw) = scale_dimension((H, W), max(1, max(P)) / 4) (model.py:559-562, 590-594)
     and merges them elementwise: reduce_max or reduce_mean over the scales (model.py:608-625).
     The reference keys the per-scale logits by 'logits_%.2f' % scale (model.py:603-606): scales
     that print alike share one entry, which holds the LAST of them at the position of the
     first. Only those scales get a plan (``merged_scales``);
  4. the object / fragment softmaxes and the argmax of ``predict`` (model.py:677-683) run on the
     merged heads.

The whole forward is one linear sequence of launches (no parallel branches): each scale's plan
fills the GPU on its own. DESIGN.md, "multi-scale mode".
"""
import math

import torch

from epos_amd import _lib
from epos_amd._call import ptr as _ptr
from epos_amd import net as _net
from epos_amd import weights as W

MAX_SCALES = 8                     # epos_resize_merge_f32: 1 <= S <= 8
MERGE_METHODS = {'max': _lib.MERGE_MAX, 'avg': _lib.MERGE_MEAN}   # common.py:140-141


def normalize_pyramid(image_pyramid):
  """The pyramid as a list of floats, or None for single-scale inference (None or [1.0]).
  ValueError for an empty list, more than MAX_SCALES scales or a scale that is not a positive
  finite number."""
  if image_pyramid is None:
    return None
  try:
    scales = [float(s) for s in image_pyramid]
  except (TypeError, ValueError):
    raise ValueError('image_pyramid must be a list of numbers (got %r).' % (image_pyramid,))
  if not scales:
    raise ValueError('image_pyramid must not be empty.')
  if len(scales) > MAX_SCALES:
    raise ValueError('image_pyramid: at most %d scales (got %d).' % (MAX_SCALES, len(scales)))
  for s in scales:
    if not (math.isfinite(s) and s > 0):
      raise ValueError('image_pyramid: scales must be positive (got %r).' % (s,))
  if scales == [1.0]:
    return None
  return scales


def check_merge_method(merge_method):
  if merge_method not in MERGE_METHODS:
    raise ValueError('Unsupported merge_method: %r (max or avg, common.py:140-141).'
                     % (merge_method,))
  return merge_method


def merged_scales(scales):
  """The scales whose logits the reference merges, in merge order: its per-scale dict is keyed
  by 'logits_%.2f' % scale (model.py:603-606), so a later scale overwrites an earlier one that
  prints alike and keeps that one's position."""
  entries = {}
  for s in scales:
    entries['%.2f' % s] = s
  return list(entries.values())


def decoder_size(height, width, scale):
  """The decoder size of the plan at `scale` (None: the stride-4 map of its input). For
  s != 1.0 the reference passes crop_size = [scaled_height, scaled_width] (model.py:572,581)
  to a decoder that reads crop_size as [width, height] (model.py:355-356)."""
  if scale == 1.0:
    return None
  h, w = _net.scale_dimension(height, scale), _net.scale_dimension(width, scale)
  return _net.scale_dimension(w, 0.25), _net.scale_dimension(h, 0.25)


def merged_size(height, width, scales):
  """(Lh, Lw): the size of the merged logits (model.py:559-562): decoder stride 4 of the
  image at max(1, max(P)), over the whole pyramid as given."""
  s = max(1.0, max(scales)) / 4
  return _net.scale_dimension(height, s), _net.scale_dimension(width, s)


def scale_sizes(height, width, scales):
  """The input size of each scale's plan (model.py:569-573)."""
  return [(height, width) if s == 1.0 else
          (_net.scale_dimension(height, s), _net.scale_dimension(width, s)) for s in scales]


class MultiScaleNet(object):
  """The multi-scale forward plan. Same surface as ``EposNet`` for ``model.predict`` and
  ``EposPipeline``: forward / outputs / set_images / capture_graph, out_h / out_w (the merged
  size), B / H / W, num_objs / num_frags, flops, algorithmic_bytes()."""

  def __init__(self, checkpoint, batch, height, width, num_objs, num_frags=64,
               image_pyramid=(1.0,), merge_method='max', model_variant='xception_65',
               encoder_output_stride=8, decoder_output_stride=4, atrous_rates=(12, 24, 36),
               multi_grid=None, device='cuda:0', dry_run=False, precision='fp32'):
    pyramid = normalize_pyramid(image_pyramid) or [1.0]
    self.merge_method = check_merge_method(merge_method)
    self.pyramid = pyramid                   # as given: it sets the merged size
    scales = merged_scales(pyramid)          # one plan per merged entry
    self.scales = scales
    self.dry_run = bool(dry_run)
    self.precision = precision
    self.B, self.H, self.W = batch, height, width
    self.num_objs, self.num_frags = num_objs, num_frags
    self.sizes = scale_sizes(height, width, scales)
    self.nets = [_net.EposNet(checkpoint, batch, h, w, num_objs, num_frags,
                              model_variant=model_variant,
                              encoder_output_stride=encoder_output_stride,
                              decoder_output_stride=decoder_output_stride,
                              atrous_rates=atrous_rates, multi_grid=multi_grid, device=device,
                              dry_run=dry_run, precision=precision,
                              decoder_hw=decoder_size(height, width, s))
                 for s, (h, w) in zip(scales, self.sizes)]
    self.lib = None if self.dry_run else _lib.load()
    self.dev = self.nets[0].dev
    self.out_h, self.out_w = merged_size(height, width, pyramid)
    self._graph = None
    self._images_u8 = None       # device staging for uint8 frames (set_images)
    # the full-size fp32 image: the 1.0 plan's own input buffer when the pyramid has one
    if 1.0 in scales:
      self.images = self.nets[scales.index(1.0)].images
    else:
      self.images = torch.empty(batch, height, width, 3, dtype=torch.float32, device=self.dev)
    B, Lh, Lw = batch, self.out_h, self.out_w
    self.channels = dict(sorted(W.outputs_to_num_channels(num_objs, num_frags).items()))
    self.logits = {name: torch.empty(B, Lh, Lw, ch, dtype=torch.float32, device=self.dev)
                   for name, ch in self.channels.items()}
    self.obj_label = torch.empty(B, Lh, Lw, dtype=torch.int64, device=self.dev)
    self.ops = []                # (name, callable(stream)), in launch order
    self.merge_bytes = 0         # algorithmic bytes of the resize / merge launches
    self._build()

  # the fp16-pair bookkeeping as infer.py prints it: the layers of every scale's plan
  h2_layers = property(lambda self: [l for n in self.nets for l in n.h2_layers])
  h2_refused = property(lambda self: [l for n in self.nets for l in n.h2_refused])
  flops = property(lambda self: sum(n.flops for n in self.nets))

  def _resize_merge(self, name, srcs, Y, Ho, Wo, C, merge):
    """Appends one epos_resize_merge_f32 launch; srcs = [(tensor, ldx, Hi, Wi)]."""
    self.merge_bytes += 4 * (sum(self.B * hi * wi * C for _, _, hi, wi in srcs) +
                             self.B * Ho * Wo * C)
    if self.dry_run:
      self.ops.append((name, None))
      return
    arr = (_lib.ResizeSrc * len(srcs))(*[_lib.ResizeSrc(_ptr(x), ld, hi, wi)
                                         for x, ld, hi, wi in srcs])
    fn, lib = self.lib.epos_resize_merge_f32, self.lib
    args = (arr, len(srcs), _ptr(Y), Y.shape[-1], self.B, Ho, Wo, C, merge)

    def run(stream):
      _lib.check(fn(*(args + (stream,))), name, lib)
    self.ops.append((name, run))

  def _build(self):
    # structure record of the multi-scale part (tests/test_multiscale_host.py)
    self.trace = {'image_pyramid': list(self.pyramid), 'scales': list(self.scales),
                  'merge_method': self.merge_method, 'merged_hw': [self.out_h, self.out_w],
                  'per_scale': [], 'logits_resize': []}
    for s, net, (h, w) in zip(self.scales, self.nets, self.sizes):
      if s != 1.0:                                            # model.py:569-573
        self._resize_merge('scale_%g/resize_input' % s, [(self.images, 3, self.H, self.W)],
                           net.images, h, w, 3, _lib.MERGE_MAX)
      self.ops.append(('scale_%g/plan' % s, lambda st, net=net: net.run_plan(with_post=False)))
      self.trace['per_scale'].append({
          'scale': s, 'input_hw': [h, w],
          'input_expr': 'resize(input,%dx%d)' % (h, w) if s != 1.0 else 'input',
          'logits_hw': [net.out_h, net.out_w], 'layers': net.trace_layers})
      self.trace['logits_resize'] += [                        # model.py:590-594
          {'output': name, 'from_hw': [net.out_h, net.out_w],
           'to_hw': [self.out_h, self.out_w]} for name in self.channels]
    merge = MERGE_METHODS[self.merge_method]
    for name, ch in self.channels.items():                   # model.py:608-625
      self._resize_merge('merge/' + name,
                         [(n.logits[name], ch, n.out_h, n.out_w) for n in self.nets],
                         self.logits[name], self.out_h, self.out_w, ch, merge)
    self.trace['merge'] = {
        name: {'keys': ['logits_%.2f' % s for s in self.scales],
               'sources': [[n.out_h, n.out_w] for n in self.nets],
               'target': [self.out_h, self.out_w], 'channels': ch}
        for name, ch in self.channels.items()}
    # predict's post-ops on the merged heads (model.py:677-683)
    m = self.B * self.out_h * self.out_w
    O, F = self.num_objs, self.num_frags
    obj, frag = self.logits[W.PRED_OBJ_CONF], self.logits[W.PRED_FRAG_CONF]
    if self.dry_run:
      return
    lib = self.lib
    post = [('softmax_obj', lib.epos_softmax_groups_f32, (_ptr(obj), m, O + 1)),
            ('softmax_frag', lib.epos_softmax_groups_f32, (_ptr(frag), m * O, F)),
            ('argmax', lib.epos_argmax_i64, (_ptr(obj), O + 1, _ptr(self.obj_label), m, O + 1))]
    for name, fn, args in post:
      self.ops.append((name, _net.EposNet._call(name, fn, args)))

  def algorithmic_bytes(self, dense_heads=True):
    """The plans' bytes (EposNet.algorithmic_bytes) plus the input resizes and the merges:
    every source read once, every output written once."""
    return sum(n.algorithmic_bytes(dense_heads) for n in self.nets) + self.merge_bytes

  # ----------------------------------------------------------- running ---
  _stream = _net.EposNet._stream
  # images: float32 or uint8 [B,H,W,3] into the full-size buffer (EposNet's own upload path,
  # on this object's B / H / W / images / staging buffer)
  set_images = _net.EposNet.set_images

  def run_plan(self, with_post=True, sparse=False):
    if sparse:
      raise ValueError('sparse heads are not available with an image pyramid.')
    if self.dry_run:
      raise _lib.EposError('a dry-run plan cannot be launched.')
    s = self._stream()
    for name, fn in self.ops:
      if with_post or name not in ('softmax_obj', 'softmax_frag', 'argmax'):
        fn(s)

  def capture_graph(self, sparse=False):
    """Captures the whole multi-scale forward into one hipGraph (linear: no branches)."""
    if sparse:
      raise ValueError('sparse heads are not available with an image pyramid.')
    torch.cuda.synchronize(self.dev)
    side = _net._capture_stream(self.dev)
    with torch.cuda.stream(side):
      self.run_plan()                      # warm-up outside capture
    torch.cuda.synchronize(self.dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
      self.run_plan()
    self._graph = g
    return g

  def forward(self, images=None, use_graph=False, sparse=False):
    """Runs the multi-scale forward on the current stream and returns the prediction dict of
    ``model.predict`` on the merged logits (views of this plan's buffers, valid until the next
    forward)."""
    if sparse:
      raise ValueError('sparse heads are not available with an image pyramid.')
    if images is not None:
      self.set_images(images)
    if use_graph:
      if self._graph is None:
        self.capture_graph()
      self._graph.replay()
    else:
      self.run_plan()
    return self.outputs()

  def set_weights(self, variables, check=True):
    raise NotImplementedError('set_weights: multi-scale nets are not supported (as in '
                              'trainer)')

  def outputs(self):
    """The prediction dict of the LAST run (no launch)."""
    B, h, w = self.B, self.out_h, self.out_w
    O, F = self.num_objs, self.num_frags
    return {
        W.PRED_OBJ_CONF: self.logits[W.PRED_OBJ_CONF],
        W.PRED_OBJ_LABEL: self.obj_label,
        W.PRED_FRAG_CONF: self.logits[W.PRED_FRAG_CONF].view(B, h, w, O, F),
        W.PRED_FRAG_LOC: self.logits[W.PRED_FRAG_LOC].view(B, h, w, O, F, 3),
    }
