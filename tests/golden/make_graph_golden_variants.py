#!/usr/bin/env python
"""Writes tests/golden/variant_graph_*.json: the graphs the REFERENCE's own code builds for the
backbones beyond xception_65 / resnet_v1_101_beta that share its ASPP, decoder and heads --
xception_41, xception_71, resnet_v1_50_beta, resnet_v1_50 and resnet_v1_101 -- at 640x480 with
21 objects x 64 fragments (resnet_v1_50 also with multi_grid 1,2,4), recorded by
make_graph_golden.build (which it imports; see there).

Run in the build container only (needs the reference checkout make_graph_golden.py reads):

    python tests/golden/make_graph_golden_variants.py [--out DIR]

resnet_v1_50 / resnet_v1_101 preprocess with _preprocess_subtract_imagenet_mean
(feature.py:157-165): tf.reshape of a Python list, tf.shape, tf.zeros, tf.concat of
constants and `tensor - constant`. The stand-ins for those live here (tf_recorder.py stays as
it is): a constant is a _Const, and `input - _Const` is written `submean(input)` when the
constant is exactly the ImageNet mean RGB the build subtracts (weights.MEAN_RGB, zeros for
channels past 3) and `sub(input,const(...))` otherwise -- so the fixture pins which of the two
preprocessing functions _PREPROCESS_FN picked, and with which constants.

make_graph_golden.build writes graph_<name>.json; each result is renamed to the prefix
variant_graph_ so that the graph_*.json glob of tests/test_graph_trace.py (whose oracle refuses
these variants) does not collect it.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_graph_golden as M   # noqa: E402
import tf_recorder as R         # noqa: E402

MEAN_RGB = (123.15, 115.90, 103.06)   # = epos_amd.weights.MEAN_RGB

CONFIGS = [  # (name, model_variant, width, height, num_objs, num_frags, multi_grid)
    ('xception41_640x480_o21', 'xception_41', 640, 480, 21, 64, None),
    ('xception71_640x480_o21', 'xception_71', 640, 480, 21, 64, None),
    ('resnet50beta_640x480_o21', 'resnet_v1_50_beta', 640, 480, 21, 64, None),
    ('resnet50_640x480_o21', 'resnet_v1_50', 640, 480, 21, 64, None),
    ('resnet50_640x480_o21_mg124', 'resnet_v1_50', 640, 480, 21, 64, [1, 2, 4]),
    ('resnet101_640x480_o21', 'resnet_v1_101', 640, 480, 21, 64, None),
]


class _Const(object):
  """A constant tensor: shape and flat values (row-major)."""

  def __init__(self, shape, values):
    self.shape = R.Shape(shape)
    self.values = [float(v) for v in values]


def _fmt(values):
  return ','.join('%.9g' % v for v in values)


def _install_constant_ops(tf):
  reshape, concat = tf.reshape, tf.concat

  def reshape_(tensor, shape_, name=None):
    if isinstance(tensor, (list, tuple)):
      n = 1
      for s in shape_:
        n *= int(s)
      assert n == len(tensor), (tensor, shape_)
      return _Const([int(s) for s in shape_], tensor)
    return reshape(tensor, shape_, name)

  def zeros(shape_, dtype=None, name=None):
    n = 1
    for s in shape_:
      n *= int(s)
    return _Const([int(s) for s in shape_], [0.0] * n)

  def concat_(values, axis, name='concat'):
    if all(isinstance(v, _Const) for v in values):
      # along the last axis of [1, 1, 1, c] constants: the flat values concatenate
      assert axis == 3 and all(list(v.shape[:3]) == [1, 1, 1] for v in values)
      return _Const([1, 1, 1, sum(v.shape[3] for v in values)],
                    [x for v in values for x in v.values])
    return concat(values, axis, name)

  tf.reshape, tf.zeros, tf.concat = reshape_, zeros, concat_
  sub = R.Tensor.__sub__

  def sub_(self, other):
    if isinstance(other, _Const):
      assert list(other.shape[:3]) == [1, 1, 1] and other.shape[3] == self.shape[3]
      mean = [float('%.9g' % v) for v in MEAN_RGB] + [0.0] * (other.shape[3] - 3)
      if [float('%.9g' % v) for v in other.values] == mean:
        return R.Tensor(self.shape, 'submean(%s)' % self.expr)
      return R.Tensor(self.shape, 'sub(%s,const(%s))' % (self.expr, _fmt(other.values)))
    return sub(self, other)
  R.Tensor.__sub__ = sub_


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=HERE, help='directory the fixtures are written to')
  args = ap.parse_args(argv)
  tf = R.install()
  _install_constant_ops(tf)
  sys.path.insert(0, os.path.join(M.REFERENCE, 'external', 'slim'))
  sys.path.insert(0, M.REFERENCE)
  import nets.resnet_utils as slim_resnet_utils          # pylint: disable=import-error
  nets_mod = R._Loose('tensorflow.contrib.slim.nets')
  nets_mod.resnet_utils = slim_resnet_utils
  sys.modules['tensorflow.contrib.slim.nets'] = nets_mod
  sys.modules['tensorflow.contrib.slim.nets.resnet_utils'] = slim_resnet_utils
  sys.modules['tensorflow'].contrib.slim.nets = nets_mod
  from epos_lib import common, model                     # pylint: disable=import-error
  M.common, M.model = common, model
  M.HERE = args.out                                      # where build() writes
  for name, variant, w, h, objs, frags, mg in CONFIGS:
    src = os.path.join(args.out, 'graph_%s.json' % name)
    dst = os.path.join(args.out, 'variant_graph_%s.json' % name)
    try:
      M.build(name, variant, w, h, objs, frags, multi_grid=mg)
    finally:
      if os.path.exists(src):
        os.replace(src, dst)
    print('->', dst)


if __name__ == '__main__':
  main()
