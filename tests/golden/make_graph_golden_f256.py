#!/usr/bin/env python
"""Writes tests/golden/f256_graph_c2_xception65_640x480_o21.json: the graph the REFERENCE's
own code builds for the C2 network (xception_65, 640x480, 21 objects) with 256 fragments per
object, recorded by make_graph_golden.build (which it imports; see there).

Run in the build container only (needs the reference checkout make_graph_golden.py reads):

    python tests/golden/make_graph_golden_f256.py

make_graph_golden.build writes graph_<name>.json; the result is renamed to the prefix f256_
so that the graph_*.json glob of tests/test_graph_trace.py does not collect it.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_graph_golden as M   # noqa: E402
import tf_recorder as R         # noqa: E402


def main():
  R.install()
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
  name = 'c2_xception65_640x480_o21_f256'
  M.build(name, 'xception_65', 640, 480, 21, 256)
  src = os.path.join(HERE, 'graph_%s.json' % name)
  dst = os.path.join(HERE, 'f256_graph_c2_xception65_640x480_o21.json')
  os.replace(src, dst)
  print('->', dst)


if __name__ == '__main__':
  main()
