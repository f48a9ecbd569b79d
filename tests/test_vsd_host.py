"""VSD on the host: the binding, the numpy definition against an independent formulation, the
error and recall arithmetic, the pixel window, the depth readers and the parts of eval_poses.py
that need no device."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from epos_amd import bop_io, pose_error, vsd      # noqa: E402
from tests.helpers import vsd_ref                 # noqa: E402


# ------------------------------------------------------------------ binding ---
def test_vsd_symbols_declared_and_bound():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  for name, n_args in (('epos_vsd_max_taus', 0), ('epos_vsd_row_bands', 0),
                       ('epos_vsd_counts', 14)):
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
    assert m, name
    params = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).strip()
    declared = 0 if params == 'void' else params.count(',') + 1
    assert declared == n_args == len(_lib.SYMBOLS[name][1]), name
  assert re.search(r'#define\s+EPOS_ABI_VERSION\s+7\b', header)
  lib = _lib.load()
  assert lib.epos_abi_version() == 7
  assert lib.epos_vsd_max_taus() == 16 and lib.epos_vsd_row_bands() >= 1
  # the record of the header, field by field
  assert ctypes.sizeof(_lib.VsdPair) == 72 == vsd.PAIR_DTYPE.itemsize
  assert [n for n, _ in _lib.VsdPair._fields_] == list(vsd.PAIR_DTYPE.names)
  for name, _ in _lib.VsdPair._fields_:
    assert getattr(_lib.VsdPair, name).offset == vsd.PAIR_DTYPE.fields[name][1], name
  assert _lib.VsdPair.fx.offset == 32 and _lib.VsdPair.diameter.offset == 64
  struct = re.search(r'typedef struct EposVsdPair \{(.*?)\} EposVsdPair;', header, re.S).group(1)
  struct = re.sub(r'/\*.*?\*/', '', struct, flags=re.S)
  fields = [f.strip() for decl in struct.split(';') if decl.strip()
            for f in decl.strip().split(None, 1)[1].split(',')]
  assert fields == list(vsd.PAIR_DTYPE.names)


def test_constants():
  assert vsd.VSD_DELTA == 15.0
  assert len(vsd.VSD_TAUS) == len(vsd.VSD_THRESHOLDS) == 10
  assert vsd.VSD_TAUS[0] == 0.05 and vsd.VSD_TAUS[-1] == 0.5
  assert vsd.VSD_TAUS == pytest.approx(np.linspace(0.05, 0.5, 10))
  assert vsd.VSD_THRESHOLDS == vsd.VSD_TAUS
  # the default chunk: 12 bytes per pixel and instance within the budget, and < 2^31 pixels
  n = vsd.default_max_instances(480, 640)
  assert n == (1 << 30) // (12 * 480 * 640) and n * 480 * 640 < 2 ** 31
  assert vsd.default_max_instances(4, 4, budget=1 << 40) * 16 < 2 ** 31
  assert vsd.default_max_instances(4000, 4000) == 5
  assert vsd.default_max_instances(30000, 30000) == 2


# ------------------------------------------------------------------ errors ---
def test_vsd_from_counts_by_hand():
  #         mask_g vis_g mask_e vis_e inter uni  ge(0.05) ge(0.5)
  rows = [[100, 80, 90, 70, 50, 100, 20, 5],
          [10, 0, 12, 0, 0, 0, 0, 0],            # nothing visible: 1.0
          [0, 0, 0, 0, 0, 0, 0, 0],              # nothing rendered: 1.0
          [40, 40, 40, 40, 40, 40, 0, 0],        # identical: 0.0
          [40, 40, 0, 0, 0, 40, 0, 0],           # no estimate: 1.0
          [40, 30, 40, 30, 30, 30, 30, 0]]
  got = vsd.vsd_from_counts(np.array(rows, np.int64))
  assert got.shape == (6, 2) and got.dtype == np.float64
  assert got.tolist() == [[(20 + 50) / 100.0, (5 + 50) / 100.0], [1.0, 1.0], [1.0, 1.0],
                          [0.0, 0.0], [1.0, 1.0], [1.0, 0.0]]
  assert vsd.visib_fract(np.array(rows, np.int64)).tolist() == [0.8, 0.0, 0.0, 1.0, 1.0, 0.75]
  assert vsd.vsd_from_counts(np.zeros((0, 16), np.int64)).shape == (0, 10)


def test_recalls_vsd_and_ar_by_hand():
  taus, ths = (0.1, 0.2), (0.3, 0.5)
  # object 1, one image: two estimates with EQUAL scores (file order breaks the tie) and two
  # ground truths; object 2: one estimate, two ground truths
  e1 = np.array([[[0.25, 0.10], [0.20, 0.45]],      # estimate 0 against gt 0, gt 1: per tau
                 [[0.10, 0.60], [0.40, 0.20]]])
  e2 = np.array([[[0.30, 0.29], [0.9, 0.9]]])
  groups = [{'obj_id': 1, 'scores': [0.5, 0.5], 'vsd': e1},
            {'obj_id': 2, 'scores': [0.9], 'vsd': e2}]
  r = vsd.recalls_vsd(groups, taus=taus, thresholds=ths)
  # tau 0, theta .3: est 0 takes gt 1 (.20 < .25), est 1 takes gt 0 (.10): 2 of 2
  # tau 0, theta .5: the same: 2
  # tau 1, theta .3: est 0 takes gt 0 (.10); est 1: gt 1 .20 < .3: 2
  # tau 1, theta .5: est 0 takes gt 0 (.10); est 1 takes gt 1 (.20): 2
  assert r['per_object'][1]['recall_vsd'] == [[1.0, 1.0], [1.0, 1.0]]
  # object 2: .30 is not < .3 (strict); .30 < .5; .29 < .3; .29 < .5: of two targets
  assert r['per_object'][2]['recall_vsd'] == [[0.0, 0.5], [0.5, 0.5]]
  assert r['per_object'][2]['ar_vsd'] == pytest.approx(1.5 / 4)
  assert r['overall']['targets'] == 4
  assert r['overall']['recall_vsd'] == [[0.5, 0.75], [0.75, 0.75]]
  assert r['overall']['ar_vsd'] == pytest.approx(2.75 / 4)
  # the greedy order matters: with the higher score on estimate 1 it takes gt 0 first
  groups[0]['scores'] = [0.5, 0.6]
  e1b = np.array([[[0.10, 0.1], [0.60, 0.6]], [[0.05, 0.1], [0.20, 0.6]]])
  r2 = vsd.recalls_vsd([{'obj_id': 1, 'scores': [0.5, 0.6]}], [e1b], taus=taus, thresholds=ths)
  # tau 0: est 1 takes gt 0 (.05); est 0 is left with gt 1 at .60: 1 of 2 at both thresholds
  assert r2['overall']['recall_vsd'][0] == [0.5, 0.5]
  assert vsd.ar(0.3, 0.6, 0.9) == pytest.approx(0.6)
  assert vsd.ar(1.0, 1.0, 1.0) == 1.0
  # the same pooling as pose_error.recalls: targets agree on the same groups
  for g, e in zip(groups, (e1, e2)):
    g['errors'] = np.zeros(e.shape[:2] + (4,))
  pe = pose_error.recalls(groups, {1: 100.0, 2: 100.0}, {1: 1, 2: 1}, 640)
  assert pe['overall']['targets'] == r['overall']['targets']
  with pytest.raises(ValueError):
    vsd.recalls_vsd([{'obj_id': 1, 'scores': [1.0], 'vsd': np.zeros((1, 2, 3))}], taus=taus)
  # an object without ground truth or without estimates
  r3 = vsd.recalls_vsd([{'obj_id': 4, 'scores': [], 'vsd': np.zeros((0, 2, 10))},
                        {'obj_id': 5, 'scores': [1.0], 'vsd': np.zeros((1, 0, 10))}])
  assert r3['per_object'][4]['ar_vsd'] == 0.0 and r3['per_object'][4]['targets'] == 2
  assert r3['per_object'][5]['targets'] == 0 and r3['overall']['ar_vsd'] == 0.0
  assert np.shape(r3['overall']['recall_vsd']) == (10, 10)


# ------------------------------------------------------------------ window ---
def test_window_contains_every_projected_vertex():
  rng = np.random.RandomState(3)
  h, w, near = 480, 640, 10.0
  K = np.array([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]])
  n_tight = 0
  for _ in range(400):
    pts = rng.uniform(-1, 1, (50, 3)) * rng.uniform(10, 150, 3)
    R = pose_error.axis_rotation(rng.uniform(0, np.pi), rng.randn(3))
    t = np.array([rng.uniform(-500, 500), rng.uniform(-400, 400), rng.uniform(-100, 1500)])
    x0, y0, x1, y1 = vsd.window(vsd.bbox_corners(pts), R, t, K, h, w, near)
    assert 0 <= x0 <= x1 <= w and 0 <= y0 <= y1 <= h
    P = pts.dot(R.T) + t
    front = P[:, 2] >= near
    u = K[0, 0] * P[front, 0] / P[front, 2] + K[0, 2]
    v = K[1, 1] * P[front, 1] / P[front, 2] + K[1, 2]
    px, py = np.floor(u), np.floor(v)
    inside = (px >= 0) & (px < w) & (py >= 0) & (py < h)
    # every pixel of the image a vertex falls into is in the window, with a pixel to spare
    assert (px[inside] >= x0).all() and (px[inside] < x1).all()
    assert (py[inside] >= y0).all() and (py[inside] < y1).all()
    if (x0, y0, x1, y1) != (0, 0, w, h):
      n_tight += 1
      assert (px[inside] - 1 >= x0).all() or x0 == 0
      assert (px[inside] + 1 < x1).all() or x1 == w
  assert n_tight > 100                      # the check is not about full images only


def test_window_full_image_and_clipping():
  h, w, near = 40, 48, 10.0
  K = np.array([[60.0, 0.0, 24.0], [0.0, 60.0, 20.0], [0.0, 0.0, 1.0]])
  box = vsd.bbox_corners(np.array([[-5.0, -4.0, -3.0], [5.0, 4.0, 3.0]]))
  assert box.shape == (8, 3) and len(set(map(tuple, box))) == 8
  I = np.eye(3)
  # a corner nearer than `near` (12 - 3 = 9 < 10): the full image
  assert vsd.window(box, I, [0, 0, 12.0], K, h, w, near) == (0, 0, w, h)
  assert vsd.window(box, I, [0, 0, -200.0], K, h, w, near) == (0, 0, w, h)
  assert vsd.window(box, I, [0, 0, np.nan], K, h, w, near) == (0, 0, w, h)
  # exactly at `near` is in front
  x0, y0, x1, y1 = vsd.window(box, I, [0, 0, 13.0], K, h, w, near)
  assert (x0, y0, x1, y1) == (0, 0, w, h) or (x0 >= 0 and x1 <= w)
  # in front: u in 24 +- 60 * 5 / 97 = [20.9, 27.09] -> pixels 20..27, one more each side
  assert vsd.window(box, I, [0, 0, 100.0], K, h, w, near) == (19, 16, 29, 24)
  # beside the image: empty and valid
  x0, y0, x1, y1 = vsd.window(box, I, [500.0, 0, 100.0], K, h, w, near)
  assert x0 == x1 == w and 0 <= y0 <= y1 <= h
  x0, y0, x1, y1 = vsd.window(box, I, [-500.0, -500.0, 100.0], K, h, w, near)
  assert (x0, x1, y0, y1) == (0, 0, 0, 0)
  # the union of two windows; an empty one is ignored
  assert vsd.union((3, 4, 10, 12), (5, 1, 20, 6)) == (3, 1, 20, 12)
  assert vsd.union((0, 0, 0, 0), (5, 1, 20, 6)) == (5, 1, 20, 6)
  assert vsd.union((5, 1, 20, 6), (48, 3, 48, 9)) == (5, 1, 20, 6)


# ------------------------------------------------------------------ depth IO ---
def test_depth_io(tmp_path):
  rng = np.random.RandomState(0)
  d = rng.randint(0, 65536, (5, 7)).astype(np.uint16)
  d[0, 0], d[0, 1] = 0, 65535
  png = str(tmp_path / 'd.png')
  bop_io.save_depth_png(png, d)
  got = bop_io.load_depth(png)
  assert got.dtype == np.float32 and got.shape == (5, 7)
  assert (got == d.astype(np.float32)).all()
  assert (bop_io.load_depth(png, 0.1) == d.astype(np.float32) * np.float32(0.1)).all()
  f = rng.uniform(0, 2000, (4, 3)).astype(np.float32)
  np.save(str(tmp_path / 'f.npy'), f)
  assert (bop_io.load_depth(str(tmp_path / 'f.npy')) == f).all()
  np.save(str(tmp_path / 'u.npy'), d)
  got = bop_io.load_depth(str(tmp_path / 'u.npy'), 0.5)
  assert got.dtype == np.float32 and (got == d.astype(np.float32) * np.float32(0.5)).all()
  np.save(str(tmp_path / 'bad.npy'), np.zeros((2, 2, 3)))
  with pytest.raises(ValueError):
    bop_io.load_depth(str(tmp_path / 'bad.npy'))
  cam = {'3': {'cam_K': [572.4, 0.0, 325.3, 0.0, 573.6, 242.0, 0.0, 0.0, 1.0],
               'depth_scale': 0.1},
         '17': {'cam_K': list(range(9))}}
  with open(str(tmp_path / 'scene_camera.json'), 'w') as fh:
    json.dump(cam, fh)
  sc = bop_io.load_scene_camera(str(tmp_path / 'scene_camera.json'))
  assert sorted(sc) == [3, 17] and sc[3]['depth_scale'] == 0.1 and sc[17]['depth_scale'] == 1.0
  assert sc[3]['cam_K'].shape == (3, 3) and sc[3]['cam_K'][1, 2] == 242.0
  assert bop_io.depth_path('/b', 'tudl', 'test', 2, 31) == '/b/tudl/test/000002/depth/000031.png'
  assert bop_io.scene_camera_path('/b', 'tudl', 'test', 2) == \
      '/b/tudl/test/000002/scene_camera.json'


# ------------------------------------------------------------------ the definition ---
def _three_distance_images(depth_test, depth_gt, depth_est, K, delta, taus, diameter):
  """An independent formulation: three distance images, boolean masks (as the published
  description of VSD reads), on whole images."""
  h, w = depth_test.shape
  xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
  ray = np.sqrt(((xs - K[0, 2]) / K[0, 0]) ** 2 + ((ys - K[1, 2]) / K[1, 1]) ** 2 + 1.0)
  dist_test, dist_gt, dist_est = (np.asarray(d, np.float64) * ray
                                  for d in (depth_test, depth_gt, depth_est))
  valid = np.asarray(depth_test) > 0

  def visible(dist_model, mask):
    return mask & (~valid | (dist_model - dist_test <= delta))
  mask_gt, mask_est = np.asarray(depth_gt) > 0, np.asarray(depth_est) > 0
  visib_gt = visible(dist_gt, mask_gt)
  visib_est = visible(dist_est, mask_est) | (visib_gt & mask_est)
  visib_inter, visib_union = visib_gt & visib_est, visib_gt | visib_est
  dists = np.abs(dist_gt - dist_est)[visib_inter] / diameter
  return [int(mask_gt.sum()), int(visib_gt.sum()), int(mask_est.sum()), int(visib_est.sum()),
          int(visib_inter.sum()), int(visib_union.sum())] + [int((dists >= t).sum())
                                                             for t in taus]


@pytest.mark.parametrize('seed', range(4))
def test_reference_against_three_distance_images(seed):
  rng = np.random.RandomState(seed)
  h, w, delta, diameter = 23, 31, 15.0, 96.0
  taus = vsd.VSD_TAUS
  K = np.array([[64.0, 0.0, 15.5], [0.0, 32.0, 11.5], [0.0, 0.0, 1.0]])

  def blob(cx, cy, r, z):
    ys, xs = np.mgrid[:h, :w]
    inside = (xs - cx) ** 2 + (ys - cy) ** 2 < r * r
    return np.where(inside, z + np.round(rng.uniform(-10, 10, (h, w)) * 8) / 8, 0.0)
  gt = blob(14, 10, 8, 600.0).astype(np.float32)
  est = blob(17, 12, 8, 604.0).astype(np.float32)
  test = np.where(rng.rand(h, w) < 0.2, 0.0,
                  np.where(rng.rand(h, w) < 0.3, 500.0, 640.0) +
                  np.round(rng.uniform(-5, 5, (h, w)) * 8) / 8).astype(np.float32)
  # keep away from the <= and >= boundaries, where the two formulations may round apart
  xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
  ray = np.sqrt(((xs - K[0, 2]) / K[0, 0]) ** 2 + ((ys - K[1, 2]) / K[1, 1]) ** 2 + 1.0)
  for model in (gt, est):
    assert (np.abs((model - test) * ray - delta)[(model > 0) & (test > 0)] > 1e-6).all()
  d = np.abs(gt.astype(np.float64) - est) * ray / diameter
  both = (gt > 0) & (est > 0)
  assert all((np.abs(d[both] - t) > 1e-9).all() for t in taus)
  pair = {'image': 0, 'gt_inst': 0, 'est_inst': 1, 'x0': 0, 'y0': 0, 'x1': w, 'y1': h,
          'fx': K[0, 0], 'fy': K[1, 1], 'cx': K[0, 2], 'cy': K[1, 2], 'diameter': diameter}
  got = vsd_ref.counts(test[None], np.stack([gt, est]), pair, delta, taus)
  exp = _three_distance_images(test, gt, est, K, delta, taus, diameter)
  assert got.dtype == np.int64 and got.tolist() == exp
  assert got[4] > 20 and got[5] > got[4] and got[1] < got[0] and 0 < got[6 + 1] <= got[4]
  # no estimate: est_inst = -1 is an all-background rendering
  got = vsd_ref.counts(test[None], np.stack([gt, est]), dict(pair, est_inst=-1), delta, taus)
  assert got.tolist() == _three_distance_images(test, gt, np.zeros_like(gt), K, delta, taus,
                                                diameter)
  # a window that contains both renderings changes nothing; an empty one counts nothing
  ys_, xs_ = np.nonzero((gt > 0) | (est > 0))
  tight = dict(pair, x0=int(xs_.min()), x1=int(xs_.max()) + 1, y0=int(ys_.min()),
               y1=int(ys_.max()) + 1)
  assert vsd_ref.counts(test[None], np.stack([gt, est]), tight, delta, taus).tolist() == exp
  assert not vsd_ref.counts(test[None], np.stack([gt, est]), dict(pair, x1=0), delta, taus).any()


# ------------------------------------------------------------------ eval_poses.py ---
def _frames_json(directory, depth=False):
  K = [[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]]
  pose = {'obj_id': 2, 'R': np.eye(3).reshape(-1).tolist(), 't': [0.0, 0.0, 500.0]}
  meta = [{'path': 'not_there_%d.npy' % i, 'scene_id': 3, 'im_id': i, 'K': K,
           'targets': {'2': 1}, 'gt_poses': [pose]} for i in range(2)]
  if depth:
    meta[0]['depth_path'] = 'depth_0.npy'
    np.save(os.path.join(directory, 'depth_0.npy'), np.zeros((4, 4), np.float32))
  with open(os.path.join(directory, 'frames.json'), 'w') as f:
    json.dump(meta, f)


def test_eval_poses_vsd_flags_and_refusals(tmp_path, monkeypatch):
  import eval_poses
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  base = ['--model', 'm', '--dataset', 'tudl']
  args, _ = eval_poses.prepare(base + ['--frames', 'x'])
  assert args.vsd is False and args.depth_split is None and args.vsd_delta == 15.0
  assert args.min_visib_fract == 0.0 and args.vsd_max_instances is None
  args, _ = eval_poses.prepare(base + ['--infer_tfrecord_names', 'a', '--vsd', 'true',
                                       '--depth_split', 'test', '--vsd_delta', '20',
                                       '--min_visib_fract', '0.1', '--vsd_max_instances', '8'])
  assert args.vsd is True and args.depth_split == 'test' and args.vsd_delta == 20.0
  assert args.min_visib_fract == 0.1 and args.vsd_max_instances == 8
  # TFRecord frames carry no depth: without --depth_split there is no source
  with pytest.raises(ValueError, match='--vsd needs the test depth'):
    eval_poses.prepare(base + ['--infer_tfrecord_names', 'a', '--vsd', 'true'])
  with pytest.raises(ValueError, match='--min_visib_fract needs the test depth'):
    eval_poses.prepare(base + ['--infer_tfrecord_names', 'a', '--min_visib_fract', '0.1'])
  with pytest.raises(ValueError, match='min_visib_fract must be'):
    eval_poses.prepare(base + ['--frames', 'x', '--min_visib_fract', '1.5'])
  # frames.json entries without depth_path: an error that names the frame, before any device
  # or result file is touched
  _frames_json(str(tmp_path))
  with pytest.raises(ValueError, match='scene 3 image 0 has no test depth'):
    eval_poses.main(base + ['--frames', str(tmp_path), '--vsd', 'true'])
  with pytest.raises(ValueError, match='scene 3 image 0 has no test depth'):
    eval_poses.main(base + ['--frames', str(tmp_path), '--min_visib_fract', '0.1'])
  _frames_json(str(tmp_path), depth=True)               # the second frame still has none
  with pytest.raises(ValueError, match='scene 3 image 1 has no test depth'):
    eval_poses.main(base + ['--frames', str(tmp_path), '--vsd', 'true'])
  # --depth_split: a scene folder without scene_camera.json, then without the depth image
  with pytest.raises(ValueError, match='no scene_camera.json for scene 3'):
    eval_poses.main(base + ['--frames', str(tmp_path), '--vsd', 'true', '--depth_split', 'test'])
  scene = tmp_path / 'tudl' / 'test' / '000003'
  os.makedirs(str(scene / 'depth'))
  with open(str(scene / 'scene_camera.json'), 'w') as f:
    json.dump({'0': {'cam_K': list(range(9)), 'depth_scale': 1.0}}, f)
  with pytest.raises(ValueError, match='scene 3 image 0 has no test depth'):
    eval_poses.main(base + ['--frames', str(tmp_path), '--vsd', 'true', '--depth_split', 'test'])
  # without the new flags nothing asks for depth: the run gets as far as the missing results
  with pytest.raises(ValueError, match='no pose estimates'):
    eval_poses.main(base + ['--frames', str(tmp_path)])


def test_depth_sources_and_lazy_frames(tmp_path, monkeypatch):
  import eval_poses
  from epos_amd import cli
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  _frames_json(str(tmp_path), depth=True)
  meta = json.load(open(str(tmp_path / 'frames.json')))
  meta[1]['depth_path'], meta[1]['depth_scale'] = 'depth_1.png', 0.5
  json.dump(meta, open(str(tmp_path / 'frames.json'), 'w'))
  bop_io.save_depth_png(str(tmp_path / 'depth_1.png'), np.full((4, 6), 1000, np.uint16))
  meta = cli.read_frames_json(str(tmp_path))
  frames = cli.load_frames(None, str(tmp_path), 0, '640,480', 480, 0, 0, pixels=False,
                           meta=meta)[0]
  args, _ = eval_poses.prepare(['--model', 'm', '--dataset', 'tudl', '--frames', str(tmp_path),
                                '--vsd', 'true'])
  src = eval_poses.depth_sources(args, frames, meta)
  assert [s[1] for s in src] == [1.0, 0.5] and src[1][2] is frames[1].K
  lazy = eval_poses.DepthFrames(src, keep=1)
  assert len(lazy) == 2 and lazy[1][0].shape == (4, 6) and (lazy[1][0] == 500.0).all()
  assert lazy[0][0].shape == (4, 4) and len(lazy._cache) == 1
  # --depth_split: the scene's camera and scale, the BOP path template
  scene = tmp_path / 'tudl' / 'val' / '000003'
  os.makedirs(str(scene / 'depth'))
  cam_K = [500.0, 0.0, 3.0, 0.0, 510.0, 2.0, 0.0, 0.0, 1.0]
  with open(str(scene / 'scene_camera.json'), 'w') as f:
    json.dump({str(i): {'cam_K': cam_K, 'depth_scale': 0.1} for i in range(2)}, f)
  for i in range(2):
    bop_io.save_depth_png(str(scene / 'depth' / ('%06d.png' % i)),
                          np.full((4, 6), 100 * (i + 1), np.uint16))
  args.depth_split = 'val'
  src = eval_poses.depth_sources(args, frames, meta)
  assert src[1][0] == str(scene / 'depth' / '000001.png') and src[1][1] == 0.1
  assert src[0][2].tolist() == np.reshape(cam_K, (3, 3)).tolist()
  depth, K = eval_poses.DepthFrames(src)[1]
  assert (depth == np.float32(200) * np.float32(0.1)).all() and K[1, 1] == 510.0


def test_build_groups_drops_invisible_targets(tmp_path):
  import eval_poses
  from epos_amd import cli
  K = [[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]]
  pose = {'obj_id': 2, 'R': np.eye(3).reshape(-1).tolist(), 't': [0.0, 0.0, 500.0]}
  meta = [{'path': 'x', 'scene_id': 3, 'im_id': 0, 'K': K, 'targets': {'2': 3},
           'gt_poses': [pose, dict(pose, t=[1.0, 0, 500.0]), dict(pose, t=[2.0, 0, 500.0])]}]
  with open(str(tmp_path / 'frames.json'), 'w') as f:
    json.dump(meta, f)
  frames = cli.load_frames(None, str(tmp_path), 0, '640,480', 480, 0, 0, pixels=False)[0]
  results = [{'scene_id': 3, 'im_id': 0, 'obj_id': 2, 'score': s, 'R': np.eye(3),
              't': np.zeros((3, 1))} for s in (0.1, 0.9, 0.5)]
  groups, ignored = eval_poses.build_groups(frames, results)
  assert ignored == 0 and len(groups[0]['ests']) == 3 and len(groups[0]['gts']) == 3
  assert groups[0]['frame_index'] == 0
  # the instance count shrinks before the n-best cut
  groups, ignored = eval_poses.build_groups(frames, results, {(0, 2): {1}})
  assert ignored == 1 and [e['score'] for e in groups[0]['ests']] == [0.9, 0.5]
  assert [float(g['t'][0, 0]) for g in groups[0]['gts']] == [0.0, 2.0]
  groups, ignored = eval_poses.build_groups(frames, results, {(0, 2): {0, 1, 2}})
  assert ignored == 3 and groups[0]['ests'] == [] and groups[0]['gts'] == []
