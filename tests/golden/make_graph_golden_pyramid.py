#!/usr/bin/env python
"""Writes tests/golden/pyramid_graph_c2_xception65_640x480_o21.json: what the REFERENCE's own
multi-scale inference builds (model.predict -> multi_scale_logits, model.py:515-626) for C2
(xception_65, 640x480, 21 objects x 64 fragments) with image_pyramid=[0.75, 1.0, 1.25] and
merge_method='max', recorded by tests/golden/tf_recorder.py through make_graph_golden.build's
imports (see there).

Run in the build container only (needs the reference checkout make_graph_golden.py reads):

    python tests/golden/make_graph_golden_pyramid.py [--out DIR]

The recorder lacks what only the merge uses; the stand-ins live here (tf_recorder.py stays as
it is): tf.expand_dims on axis 4 ('expand(x)'), tf.concat on axis 4 ('stack(a,b,...)'),
tf.reduce_max / tf.reduce_mean over axis 4 ('reduce_max(...)' / 'reduce_mean(...)'). The
recorder's variable_scope already re-enters a scope under tf.AUTO_REUSE, so every scale
records the same layer scopes again. The fixture holds, per scale in pyramid order, the image
the network sees (its expression and size) and the layers get_logits recorded; every
misc.resize_bilinear of a logits tensor (from -> to); per output the keys of the per-scale
dict the reference merges ('logits_%.2f' % scale, model.py:605-606) and the merged expression;
and predict's output expressions.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_graph_golden as M   # noqa: E402
import tf_recorder as R         # noqa: E402

NAME = 'c2_xception65_640x480_o21'
PYRAMID = [0.75, 1.0, 1.25]
MERGE = 'max'
WIDTH, HEIGHT, OBJS, FRAGS = 640, 480, 21, 64


def _install_merge_ops(tf):
  concat, reduce_mean = tf.concat, tf.reduce_mean

  def expand_dims(x, axis=None, name=None):
    assert axis == 4 and len(x.shape) == 4
    return R.Tensor(list(x.shape) + [1], 'expand(%s)' % x.expr)

  def concat_(values, axis, name='concat'):
    if axis != 4:
      return concat(values, axis, name)
    for v in values:
      assert list(v.shape[:4]) == list(values[0].shape[:4]), [list(t.shape) for t in values]
    return R.Tensor(list(values[0].shape[:4]) + [sum(v.shape[4] for v in values)],
                    'stack(%s)' % ','.join(v.expr for v in values))

  def reduce_(op, orig):
    def fn(x, axis=None, keepdims=None, name=None, **kw):
      if axis == 4:
        assert not keepdims and len(x.shape) == 5
        return R.Tensor(list(x.shape[:4]), '%s(%s)' % (op, x.expr))
      assert orig is not None, (op, axis)
      return orig(x, axis=axis, keepdims=keepdims, name=name, **kw)
    return fn

  tf.expand_dims, tf.concat = expand_dims, concat_
  tf.reduce_max = reduce_('reduce_max', None)
  tf.reduce_mean = reduce_('reduce_mean', reduce_mean)


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=HERE, help='directory the fixture is written to')
  args = ap.parse_args(argv)
  tf = R.install()
  _install_merge_ops(tf)
  sys.path.insert(0, os.path.join(M.REFERENCE, 'external', 'slim'))
  sys.path.insert(0, M.REFERENCE)
  import nets.resnet_utils as slim_resnet_utils          # pylint: disable=import-error
  nets_mod = R._Loose('tensorflow.contrib.slim.nets')
  nets_mod.resnet_utils = slim_resnet_utils
  sys.modules['tensorflow.contrib.slim.nets'] = nets_mod
  sys.modules['tensorflow.contrib.slim.nets.resnet_utils'] = slim_resnet_utils
  sys.modules['tensorflow'].contrib.slim.nets = nets_mod
  from epos_lib import common, misc, model               # pylint: disable=import-error
  M.common, M.model = common, model
  M.HERE = args.out                                      # where build() writes
  common.FLAGS.image_pyramid = PYRAMID
  common.FLAGS.merge_method = MERGE

  scales, resizes, merged = [], [], {}
  get_logits, resize, msl = model.get_logits, misc.resize_bilinear, model.multi_scale_logits

  def get_logits_(images, model_options, **kw):
    first = len(R.REC.layers)
    out = get_logits(images=images, model_options=model_options, **kw)
    scales.append({'input_expr': images.expr,
                   'input_hw': [int(images.shape[1]), int(images.shape[2])],
                   'layers': R.REC.layers[first:]})
    return out

  def resize_(images, shape, output_dtype='float32'):
    if images.expr.startswith('L:logits/'):
      resizes.append({'output': images.expr[len('L:logits/'):],
                      'from_hw': [int(images.shape[1]), int(images.shape[2])],
                      'to_hw': [int(shape[0]), int(shape[1])]})
    return resize(images, shape, output_dtype)

  def multi_scale_logits_(*a, **kw):
    out = msl(*a, **kw)
    for k, d in sorted(out.items()):
      merged[k] = {'keys': [n for n in d if n != model.MERGED_LOGITS_SCOPE],
                   'expr': d[model.MERGED_LOGITS_SCOPE].expr,
                   'shape': list(d[model.MERGED_LOGITS_SCOPE].shape)}
    return out

  model.get_logits, misc.resize_bilinear = get_logits_, resize_
  model.multi_scale_logits = multi_scale_logits_
  # build() writes graph_<name>.json: a name of its own, so that the single-scale fixture of
  # the same configuration is not touched, removed once read
  src = os.path.join(args.out, 'graph_pyramid_%s.json' % NAME)
  dst = os.path.join(args.out, 'pyramid_graph_%s.json' % NAME)
  try:
    M.build('pyramid_' + NAME, 'xception_65', WIDTH, HEIGHT, OBJS, FRAGS)
  finally:
    if os.path.exists(src):
      with open(src) as f:
        doc = json.load(f)
      os.remove(src)
  assert len(scales) == len(PYRAMID)
  for s, rec in zip(PYRAMID, scales):
    rec['scale'] = s
  doc['config'].update({'image_pyramid': PYRAMID, 'merge_method': MERGE})
  doc.pop('layers')
  doc.update({'per_scale': scales, 'logits_resize': resizes, 'merge': merged})
  with open(dst, 'w') as f:
    json.dump(doc, f, indent=0, separators=(',', ':'))
    f.write('\n')
  print('->', dst)


if __name__ == '__main__':
  main()
