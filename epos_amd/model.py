"""Operator-level mirror of ``epos_lib/model.py`` for MI355X.

``predict`` has the reference's name, argument meaning and result keys
(model.py:629-687); the graph-building half of the reference API (training) is out of
scope. The forward pass itself is the static HIP plan of ``epos_amd.net.EposNet``, or with an
``image_pyramid`` the plans of ``epos_amd.multiscale.MultiScaleNet`` (multi_scale_logits,
model.py:515-626).
"""
import collections

from epos_amd import multiscale as _ms
from epos_amd import net as _net
from epos_amd import weights as W

PRED_OBJ_CONF = W.PRED_OBJ_CONF      # common.py:24-27
PRED_OBJ_LABEL = W.PRED_OBJ_LABEL
PRED_FRAG_CONF = W.PRED_FRAG_CONF
PRED_FRAG_LOC = W.PRED_FRAG_LOC


class ModelOptions(collections.namedtuple('ModelOptions', [
    'outputs_to_num_channels', 'crop_size', 'atrous_rates',
    'encoder_output_stride', 'decoder_output_stride', 'model_variant',
    'multi_grid', 'add_image_level_feature', 'aspp_with_batch_norm',
    'aspp_with_separable_conv', 'decoder_use_separable_conv',
    'logits_kernel_size', 'merge_method'])):
  """Immutable network configuration (common.py:206-290). Only the values EPOS
  ships as defaults are supported (common.py:96-154, infer.py:586-591), plus merge_method
  (common.py:140-141, 270) for multi-scale inference."""
  __slots__ = ()

  def __new__(cls, outputs_to_num_channels, crop_size=None,
              atrous_rates=(12, 24, 36), encoder_output_stride=8,
              decoder_output_stride=(4,), model_variant='xception_65',
              multi_grid=None, merge_method='max'):
    _ms.check_merge_method(merge_method)          # common.py:140-141: 'max' | 'avg'
    return super(ModelOptions, cls).__new__(
        cls, outputs_to_num_channels, crop_size, tuple(atrous_rates),
        encoder_output_stride, tuple(decoder_output_stride), model_variant,
        multi_grid, True, True, True, True, 1, merge_method)


def get_outputs_to_num_channels(num_objs, num_frags):
  """common.py:189-203."""
  return W.outputs_to_num_channels(num_objs, num_frags)


_NETS = {}


def get_net(checkpoint, batch, height, width, num_objs, num_frags,
            model_options=None, device='cuda:0', instance=0, precision='fp32',
            image_pyramid=None):
  """Returns (and caches) the HIP plan for this checkpoint and input shape.
  ``instance`` distinguishes independent plans (own activation buffers) of the
  same network, e.g. the two halves of a double-buffered pipeline. ``precision``: 'fp32'
  (default) or 'bf16' (EposNet); plans of the two precisions are cached separately.
  ``image_pyramid``: None or [1.0] -> the single-scale EposNet; any other pyramid -> a
  MultiScaleNet merging with ``model_options.merge_method``, cached per pyramid and method."""
  mo = model_options or ModelOptions(
      get_outputs_to_num_channels(num_objs, num_frags))
  scales = _ms.normalize_pyramid(image_pyramid)
  key = (id(checkpoint), batch, height, width, num_objs, num_frags,
         mo.model_variant, mo.atrous_rates, mo.encoder_output_stride,
         mo.decoder_output_stride, tuple(mo.multi_grid or ()), str(device),
         instance, precision)
  if scales is not None:
    key += ('pyramid', tuple(scales), _ms.check_merge_method(mo.merge_method))
  if key not in _NETS:
    if len(mo.decoder_output_stride) != 1:
      raise ValueError('one decoder stage only (common.py:127-132).')
    if scales is not None:
      _NETS[key] = _ms.MultiScaleNet(
          checkpoint, batch, height, width, num_objs, num_frags, image_pyramid=scales,
          merge_method=mo.merge_method, model_variant=mo.model_variant,
          encoder_output_stride=mo.encoder_output_stride,
          decoder_output_stride=mo.decoder_output_stride[0],
          atrous_rates=mo.atrous_rates, multi_grid=mo.multi_grid, device=device,
          precision=precision)
      return _NETS[key]
    _NETS[key] = _net.EposNet(
        checkpoint, batch, height, width, num_objs, num_frags,
        model_variant=mo.model_variant,
        encoder_output_stride=mo.encoder_output_stride,
        decoder_output_stride=mo.decoder_output_stride[0],
        atrous_rates=mo.atrous_rates, multi_grid=mo.multi_grid, device=device,
        precision=precision)
  return _NETS[key]


def predict(images, model_options, checkpoint, upsample_logits=False,
            image_pyramid=None, num_objs=None, num_frags=None,
            frag_cls_agnostic=False, frag_loc_agnostic=False, device='cuda:0',
            use_graph=False, precision='fp32'):
  """model.py:629-687. images: float32 [B,H,W,3] in [0,255] (numpy or tensor).

  image_pyramid (common.py:96-98): None / [1.0] = single scale; otherwise the logits of every
  scale are resized to the stride-4 map of the largest scale (>= 1) and merged with
  ``model_options.merge_method`` ('max' or 'avg') before the softmaxes (model.py:515-626).

  Returns {pred_obj_conf f32[B,h,w,O+1], pred_obj_label i64[B,h,w],
  pred_frag_conf f32[B,h,w,O,F], pred_frag_loc f32[B,h,w,O,F,3]} as device
  tensors (views of the plan's buffers)."""
  if upsample_logits:
    raise NotImplementedError('upsample_logits=True (default False, '
                              'common.py:152-154) is out of scope.')
  if frag_cls_agnostic or frag_loc_agnostic:
    raise NotImplementedError('class-agnostic fragment heads are out of scope.')
  b, h, w = images.shape[0], images.shape[1], images.shape[2]
  net = get_net(checkpoint, b, h, w, num_objs, num_frags, model_options, device,
                precision=precision, image_pyramid=image_pyramid)
  return net.forward(images, use_graph=use_graph)
