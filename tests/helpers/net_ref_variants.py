"""Test oracle for the backbones oracle/net_ref.py does not cover -- xception_41, xception_71,
resnet_v1_50, resnet_v1_50_beta, resnet_v1_101 (feature.py:118-129) -- assembled from
net_ref's own pieces (xception_65(..., net=, blocks=), resnet_v1_101_beta(..., net=, blocks=),
bottleneck, _resnet_conv, max_pool_3x3_s2_same, aspp, decoder, conv2d_raw and its structure
trace). What is restated here is data: the block tables, the root, the decoder tap and the
preprocessing of each variant. xception_65 / resnet_v1_101_beta go through the same code and
give net_ref's results.
"""
import numpy as np
import torch

from oracle import net_ref

MEAN_RGB = [123.15, 115.90, 103.06]   # feature.py:154


def _xception_blocks(entry, middle_units, multi_grid):
  """net_xception.py block tables: (scope, depths, skip, act_in_sep, units, stride, rates)."""
  mg = list(multi_grid) if multi_grid else [1, 1, 1]
  one = [1, 1, 1]
  return ([(s, d, 'conv', False, 1, st, one) for s, d, st in entry] +
          [('middle_flow/block1', [728, 728, 728], 'sum', False, middle_units, 1, one),
           ('exit_flow/block1', [728, 1024, 1024], 'conv', False, 1, 2, one),
           ('exit_flow/block2', [1536, 1536, 2048], 'none', True, 1, 1, mg)])


_ENTRY_3 = [('entry_flow/block1', [128] * 3, 2), ('entry_flow/block2', [256] * 3, 2),
            ('entry_flow/block3', [728] * 3, 2)]
_ENTRY_5 = [('entry_flow/block1', [128] * 3, 2), ('entry_flow/block2', [256] * 3, 1),
            ('entry_flow/block3', [256] * 3, 2), ('entry_flow/block4', [728] * 3, 1),
            ('entry_flow/block5', [728] * 3, 2)]


def _resnet_blocks(block3_units, multi_grid):
  """net_resnet_v1_beta.py block tables: (scope, [(depth, bottleneck, stride, unit_rate)])."""
  mg = list(multi_grid) if multi_grid else [1, 1, 1]

  def block(scope, base, units, stride):
    return (scope, [(base * 4, base, 1, 1)] * (units - 1) + [(base * 4, base, stride, 1)])
  return [block('block1', 64, 3, 2), block('block2', 128, 4, 2),
          block('block3', 256, block3_units, 2),
          ('block4', [(2048, 512, 1, r) for r in mg])]


_XTAP = '%s/entry_flow/%s/unit_1/xception_module/separable_conv2_pointwise'
_RTAP = '%s/block1/unit_2/bottleneck_v1/conv3'

# variant -> (family, scope, blocks(multi_grid), root, preprocess, decoder tap)
VARIANTS = {
    'xception_41': ('xception', 'xception_41', lambda mg: _xception_blocks(_ENTRY_3, 8, mg),
                    None, 'unit_range', _XTAP % ('xception_41', 'block2')),
    'xception_65': ('xception', 'xception_65', lambda mg: _xception_blocks(_ENTRY_3, 16, mg),
                    None, 'unit_range', _XTAP % ('xception_65', 'block2')),
    'xception_71': ('xception', 'xception_71', lambda mg: _xception_blocks(_ENTRY_5, 16, mg),
                    None, 'unit_range', _XTAP % ('xception_71', 'block3')),
    'resnet_v1_50': ('resnet', 'resnet_v1_50', lambda mg: _resnet_blocks(6, mg), 'conv7',
                     'sub_mean', _RTAP % 'resnet_v1_50'),
    'resnet_v1_50_beta': ('resnet', 'resnet_v1_50', lambda mg: _resnet_blocks(6, mg), 'beta',
                          'unit_range', _RTAP % 'resnet_v1_50'),
    'resnet_v1_101': ('resnet', 'resnet_v1_101', lambda mg: _resnet_blocks(23, mg), 'conv7',
                      'sub_mean', _RTAP % 'resnet_v1_101'),
    'resnet_v1_101_beta': ('resnet', 'resnet_v1_101', lambda mg: _resnet_blocks(23, mg),
                           'beta', 'unit_range', _RTAP % 'resnet_v1_101'),
}


def resnet_v1_conv7(x, wts, output_stride, net, blocks):
  """net_resnet_v1_beta.py:115-204 with the default root (one 7x7 stride-2 conv2d_same 'conv1',
  :168-173) + slim stack_blocks_dense, the loop of net_ref.resnet_v1_101_beta."""
  end_points = {}
  assert output_stride % 4 == 0
  output_stride //= 4
  x = net_ref._resnet_conv(x, wts, net + '/conv1', 7, 2, 1, True)
  end_points[net + '/conv1'] = x
  x = net_ref.max_pool_3x3_s2_same(x)
  end_points[net + '/pool1'] = x
  current_stride, rate = 1, 1
  for bscope, units in blocks:
    for u, (depth, db, stride, unit_rate) in enumerate(units):
      scope = '%s/%s/unit_%d/bottleneck_v1' % (net, bscope, u + 1)
      if current_stride == output_stride:
        x = net_ref.bottleneck(x, wts, scope, depth, db, 1, rate * unit_rate, end_points)
        rate *= stride
      else:
        x = net_ref.bottleneck(x, wts, scope, depth, db, stride, unit_rate, end_points)
        current_stride *= stride
  assert current_stride == output_stride
  return x, end_points


def preprocess(x, mode):
  """feature.py:157-185 on NCHW input: 'unit_range' (2/255) x - 1, 'sub_mean' x - MEAN_RGB
  (float32 constants; channels past 3 keep their value)."""
  if mode == 'unit_range':
    y = (2.0 / 255.0) * x - 1.0
    return net_ref._tag(y, 'preprocess(input)')
  mean = np.zeros(x.shape[1], np.float32)
  mean[:3] = MEAN_RGB
  y = x - net_ref._t(mean).view(1, -1, 1, 1)
  return net_ref._tag(y, 'submean(input)')


def logits(images, wts, num_objs, num_frags, model_variant, encoder_output_stride=8,
           decoder_output_stride=(4,), atrous_rates=(12, 24, 36), multi_grid=None,
           crop_size_wh=None):
  """net_ref.logits (model.py:461-514) for every variant of VARIANTS."""
  family, scope, blocks, root, pre, tap = VARIANTS[model_variant]
  x = torch.as_tensor(np.asarray(images), dtype=torch.float32).to(net_ref.DTYPE)
  if net_ref.DEVICE:
    x = x.to(net_ref.DEVICE)
  x = x.permute(0, 3, 1, 2).contiguous()
  if crop_size_wh is None:
    crop_size_wh = (x.shape[3], x.shape[2])
  net_ref._tag(x, 'input')
  x = preprocess(x, pre)
  if family == 'xception':
    feats, end_points = net_ref.xception_65(x, wts, encoder_output_stride, net=scope,
                                            blocks=blocks(multi_grid))
  elif root == 'beta':
    feats, end_points = net_ref.resnet_v1_101_beta(x, wts, encoder_output_stride, net=scope,
                                                   blocks=blocks(multi_grid))
  else:
    feats, end_points = resnet_v1_conv7(x, wts, encoder_output_stride, scope,
                                        blocks(multi_grid))
  end_points['encoder'] = feats
  feats = net_ref.aspp(feats, wts, atrous_rates, end_points)
  feats = net_ref.decoder(feats, end_points[tap], wts, crop_size_wh, decoder_output_stride,
                          end_points)
  num_channels = {net_ref.PRED_OBJ_CONF: num_objs + 1,
                  net_ref.PRED_FRAG_CONF: num_objs * num_frags,
                  net_ref.PRED_FRAG_LOC: num_objs * num_frags * 3}
  out = {}
  for name in sorted(num_channels):                           # model.py:503
    y = net_ref.conv2d_raw(feats, wts['logits/%s/weights' % name], scope='logits/' + name)
    e = net_ref._e(y) if net_ref.TRACE is not None else None
    y = y + net_ref._t(wts['logits/%s/biases' % name]).view(1, -1, 1, 1)
    if net_ref.TRACE is not None:
      net_ref.TRACE.layers[-1]['bias'] = True
      net_ref._tag(y, e)
    out[name] = y
  return out, end_points


def predict(images, wts, num_objs, num_frags=64, **kw):
  """net_ref.predict (model.py:629-687) for every variant of VARIANTS."""
  O, F = num_objs, num_frags
  with torch.no_grad():
    lg, end_points = logits(images, wts, num_objs, num_frags, **kw)
    b, _, h, w = lg[net_ref.PRED_OBJ_CONF].shape
    obj = lg[net_ref.PRED_OBJ_CONF].permute(0, 2, 3, 1)
    frag = lg[net_ref.PRED_FRAG_CONF].permute(0, 2, 3, 1).reshape(b, h, w, O, F)
    loc = lg[net_ref.PRED_FRAG_LOC].permute(0, 2, 3, 1).reshape(b, h, w, O, F, 3)
    obj_conf = torch.softmax(obj, dim=-1)
    frag_conf = torch.softmax(frag, dim=-1)
    if net_ref.TRACE is not None:
      eo, ef, el = (net_ref._e(lg[k]) for k in (net_ref.PRED_OBJ_CONF, net_ref.PRED_FRAG_CONF,
                                                 net_ref.PRED_FRAG_LOC))
      net_ref.TRACE.outputs = {
          net_ref.PRED_OBJ_CONF: {'expr': 'softmax(%s)' % eo, 'shape': [b, h, w, O + 1]},
          net_ref.PRED_OBJ_LABEL: {'expr': 'argmax(softmax(%s))' % eo, 'shape': [b, h, w]},
          net_ref.PRED_FRAG_CONF: {'expr': 'softmax(reshape(%s,%s))' % (ef, [O, F]),
                                   'shape': [b, h, w, O, F]},
          net_ref.PRED_FRAG_LOC: {'expr': 'reshape(%s,%s)' % (el, [O, F, 3]),
                                  'shape': [b, h, w, O, F, 3]}}
    if net_ref.DEVICE == 'meta':
      return None
    return {
        net_ref.PRED_OBJ_CONF: obj_conf.numpy(),
        net_ref.PRED_OBJ_LABEL: torch.argmax(obj_conf, dim=3).numpy(),
        net_ref.PRED_FRAG_CONF: frag_conf.numpy(),
        net_ref.PRED_FRAG_LOC: loc.contiguous().numpy(),
        '_logits': {k: v.permute(0, 2, 3, 1).contiguous().numpy() for k, v in lg.items()},
        '_end_points': end_points,
    }
