#!/usr/bin/env python
"""Generates tests/golden/knn_frags.npz from the REAL reference.

Run where the reference lies (EPOS_REFERENCE, default /root/reference):

    python tests/golden/make_knn_golden.py

Imports ``epos_lib.datagen_utils`` from where it lies, with the import-time-only dependencies
(tensorflow, bop_toolkit_lib) stubbed, and records FragmentFieldGenerator.assign_to_frags_py
(datagen_utils.py:161-199) for seeded fragment centres, sizes and float32 points at knn_frags =
1, 2, 3, 4. The fixture is data (inputs and recorded outputs); no reference source travels.

The inputs are asserted tie-free: among each point's first k+1 neighbours the relative gap
between consecutive distances is at least MIN_GAP, so the order does not depend on how a
distance is rounded (cKDTree compares its own sums; the kernel sums dx^2 + dy^2 + dz^2 in that
order).
"""
import os
import sys
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get('EPOS_REFERENCE', '/root/reference')
NUM_FRAGS, NUM_POINTS, SEED, KNNS = 16, 500, 11, (1, 2, 3, 4)
MIN_GAP = 1e-9


def import_reference():
  for name in ['tensorflow', 'bop_toolkit_lib', 'bop_toolkit_lib.transform']:
    sys.modules[name] = mock.MagicMock()
  sys.path.insert(0, REFERENCE)
  from epos_lib import datagen_utils  # pylint: disable=import-error
  return datagen_utils


def inputs():
  rng = np.random.RandomState(SEED)
  centers = rng.uniform(-80, 80, (NUM_FRAGS, 3))
  sizes = rng.uniform(5, 40, NUM_FRAGS)
  xyz = rng.uniform(-90, 90, (NUM_POINTS, 3)).astype(np.float32)
  return centers, sizes, xyz


def smallest_gap(centers, xyz, k):
  """The smallest relative gap between consecutive distances among the first k+1 neighbours."""
  d = np.sqrt(((xyz.astype(np.float64)[:, None, :] - centers[None]) ** 2).sum(axis=2))
  d = np.sort(d, axis=1)[:, :k + 1]
  return float(((d[:, 1:] - d[:, :-1]) / d[:, 1:]).min())


def generate():
  datagen_utils = import_reference()
  centers, sizes, xyz = inputs()
  gap = smallest_gap(centers, xyz, max(KNNS))
  assert gap >= MIN_GAP, gap
  out = {'centers': centers, 'sizes': sizes, 'xyz': xyz}
  for k in KNNS:
    gen = datagen_utils.FragmentFieldGenerator({1: centers}, {1: sizes}, None, knn_frags=k)
    ids, coords, weights = gen.assign_to_frags_py(1, xyz)
    assert ids.shape == (NUM_POINTS, k) and ids.dtype == np.int32
    assert coords.shape == (NUM_POINTS, k, 3) and coords.dtype == np.float32
    assert weights.shape == (NUM_POINTS, k) and (weights == 1).all()
    out['ids_k%d' % k], out['coords_k%d' % k] = ids, coords
  return out, gap


def main():
  out, gap = generate()
  path = os.path.join(HERE, 'knn_frags.npz')
  np.savez_compressed(path, **out)
  print('wrote %s (%d bytes), smallest relative gap %.3g' % (path, os.path.getsize(path), gap))


if __name__ == '__main__':
  main()
