"""Host side of the device-ordered correspondences: the numpy restatement of the stage
(tests/helpers/order_ref.py) against cases worked out by hand, corresp.confidence_order, the
path choice of infer.py, and the new C symbols."""
import itertools
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import order_ref  # noqa: E402


def _coords(px, W):
  px = np.asarray(px, np.int64)
  xy = np.stack([(px % W + 0.5) * 4.0, (px // W + 0.5) * 4.0], 1)
  xyz = np.stack([px * 1.0, px * 2.0, px * 3.0], 1)
  return xy, xyz


def test_order_ref_hand_cases():
  W = 4
  # (a) one slot, a tie, always_sort: conf .5 .9 .5 .7 .9 -> rows 1 4 3 0 2
  px = [0, 1, 5, 6, 9]
  xy, xyz = _coords(px, W)
  conf = np.array([.5, .9, .5, .7, .9], np.float32)
  r = order_ref.order_stage(conf, xy, xyz, [0, 5], 5, None, True)
  assert r['slot_base_out'].tolist() == [0, 5]
  assert r['src_row'].tolist() == [1, 4, 3, 0, 2]
  # image rows of the kept rows: px 1, 9, 6, 0, 5 -> rows 0 2 1 0 1
  assert r['yorder'].tolist() == [0, 3, 2, 4, 1]
  assert r['ypos'].tolist() == [0, 4, 2, 1, 3]
  assert np.array_equal(r['coord_2d'], xy[[1, 4, 3, 0, 2]])
  assert np.array_equal(r['coord_3d'], xyz[[1, 4, 3, 0, 2]])
  # (b) the same rows, no PROSAC, K = 5 = n (and K = 7 > n): identity
  for K in (5, 7):
    r = order_ref.order_stage(conf, xy, xyz, [0, 5], 5, K, False)
    assert not r['applied'][0]
    assert r['src_row'].tolist() == [0, 1, 2, 3, 4]
    assert r['yorder'].tolist() == [0, 1, 2, 3, 4] and r['ypos'].tolist() == [0, 1, 2, 3, 4]
    assert r['slot_base_out'].tolist() == [0, 5]
  # (c) two slots + an empty one, no PROSAC, K = 2: slot 0 (3 rows) is cut to its two best,
  # slot 1 is empty, slot 2 (2 rows) stays as it is
  conf = np.array([.2, .8, .8, .1, .3], np.float32)
  r = order_ref.order_stage(conf, xy, xyz, [0, 3, 3, 5], 5, 2, False)
  assert r['applied'].tolist() == [True, False, False]
  assert r['slot_base_out'].tolist() == [0, 2, 2, 4]
  assert r['src_row'].tolist() == [1, 2, 0, 1]
  assert r['yorder'].tolist() == [0, 1, 0, 1] and r['ypos'].tolist() == [0, 1, 0, 1]
  assert np.array_equal(r['coord_2d'], xy[[1, 2, 3, 4]])
  # (d) bounds beyond the capacity are clamped: capacity 4 leaves slot 2 one row
  r = order_ref.order_stage(conf, xy, xyz, [0, 3, 3, 5], 4, None, True)
  assert r['slot_base_out'].tolist() == [0, 3, 3, 4]
  assert r['src_row'].tolist() == [1, 2, 0, 0]


def test_order_ref_yorder_is_the_stable_sort_by_y():
  rng = np.random.default_rng(3)
  for n, K, always in [(1, None, 1), (50, 20, 0), (300, None, 1), (300, 299, 0)]:
    W = 16
    px = np.sort(rng.integers(0, W * 12, n))
    xy, xyz = _coords(px, W)
    conf = rng.choice(np.linspace(.1, .9, 7), n).astype(np.float32)
    r = order_ref.order_stage(conf, xy, xyz, [0, n], n, K, always)
    y = r['coord_2d'][:, 1]
    assert np.array_equal(r['yorder'], np.argsort(y, kind='stable'))
    assert np.array_equal(r['ypos'][r['yorder']], np.arange(len(y)))
    # ... and equals the order by (first original row with the same y, position), the key
    # the kernel builds (the original rows are in raster order: y is non-decreasing)
    y0 = xy[:, 1]
    group = np.searchsorted(y0, y0[r['src_row']], 'left')
    assert np.array_equal(r['yorder'], np.argsort(group, kind='stable'))


def test_confidence_order_is_descending_with_ascending_ties():
  from epos_amd import corresp
  rng = np.random.default_rng(5)
  for vals in (np.linspace(.05, .95, 4), rng.uniform(.01, 1, 500)):
    conf = rng.choice(vals, 700).astype(np.float32)
    perm = corresp.confidence_order(conf)
    assert sorted(perm.tolist()) == list(range(700))
    c = conf[perm]
    assert (c[:-1] >= c[1:]).all()
    same = c[:-1] == c[1:]
    assert (perm[1:][same] > perm[:-1][same]).all()
    assert np.array_equal(perm, order_ref.confidence_order(conf))


def test_fitting_path_choice():
  import infer
  for prosac, K, surf, on_dev in itertools.product((False, True), (None, 200), (False, True),
                                                   (False, True)):
    operator, ordered = infer.fitting_path(prosac, K, surf, on_dev)
    assert operator == (surf or not on_dev)
    assert ordered == ((prosac or K is not None) and not operator)
  args = infer.build_parser().parse_args(['--model', 'm'])
  assert args.order_on_device is True
  assert infer.fitting_path(args.use_prosac, args.max_correspondences, args.project_to_surface,
                            args.order_on_device) == (False, False)
  args = infer.build_parser().parse_args(['--model', 'm', '--order_on_device', 'false'])
  assert args.order_on_device is False


def test_order_symbols_are_declared_and_bound():
  from epos_amd import _lib
  with open(os.path.join(ROOT, 'include', 'epos_hip.h')) as f:
    header = f.read()
  for name, nargs in [('epos_corr_order_tile_rows', 0), ('epos_corr_order_workspace_bytes', 2),
                      ('epos_corr_order_by_conf', 18), ('epos_find6d_poses_device_ordered', 18)]:
    assert re.search(r'\b%s\s*\(' % name, header), name
    assert name in _lib.SYMBOLS, name
    assert len(_lib.SYMBOLS[name][1]) == nargs
  assert '#define EPOS_ABI_VERSION 7' in header
  # the plain device entry is still there, two arguments shorter
  assert len(_lib.SYMBOLS['epos_find6d_poses_device'][1]) == 16
