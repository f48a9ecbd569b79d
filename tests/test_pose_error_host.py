"""Host side of the pose-error stage: the numpy restatement of the definitions against the
textbook formulation, the symmetry sets, matching and recall on hand-computed cases, the
binding, and the parts of eval_poses.py that need no device."""
import ctypes
import json
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from epos_amd import pose_error as pe                      # noqa: E402
from tests.helpers import pose_error_ref as ref            # noqa: E402

CAM = (1066.778, 1067.487, 312.9869, 241.3109)


def _rot(axis, angle):
  from scipy.spatial.transform import Rotation
  a = np.asarray(axis, np.float64)
  return Rotation.from_rotvec(a / np.linalg.norm(a) * angle).as_matrix()


def _pair(seed, n_verts, syms, t_scale=8.0):
  rng = np.random.RandomState(seed)
  X = rng.uniform(-60, 60, (n_verts, 3))
  R_g = _rot(rng.randn(3), rng.uniform(0, 3))
  t_g = np.array([rng.uniform(-80, 80), rng.uniform(-60, 60), rng.uniform(500, 900)])
  R_e = _rot(rng.randn(3), 0.08).dot(R_g)
  t_e = t_g + rng.randn(3) * t_scale
  return X, syms, R_e, t_e, R_g, t_g, CAM


# ------------------------------------------------------------------ definitions ---
@pytest.mark.parametrize('n_verts', [1, 5, 255, 256, 257, 700])
@pytest.mark.parametrize('sym', ['none', 'disc', 'cont'])
def test_elementwise_definition_equals_published_formula(n_verts, sym):
  info = {'none': {}, 'disc': {'symmetries_discrete': [_sym4(_rot([0, 0, 1], math.pi), [0, 0, 0])]},
          'cont': {'symmetries_continuous': [{'axis': [0, 0, 1], 'offset': [1, 2, 3]}]}}[sym]
  syms = pe.symmetry_transformations(info, 0.2 if sym == 'cont' else 0.01)
  args = _pair(n_verts, n_verts, syms)
  a, b = ref.errors(*args), ref.errors_plain(*args)
  assert np.isfinite(a).all() and (a > 0).all()
  np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)


def test_adi_nearest_neighbours_against_kdtree():
  from scipy.spatial import cKDTree
  X, syms, R_e, t_e, R_g, t_g, cam = _pair(3, 600, pe.symmetry_transformations({}))
  E = R_e.dot(X.T).T + t_e
  G = R_g.dot(X.T).T + t_g
  d, _ = cKDTree(E).query(G, k=1)
  got = ref.errors(X, syms, R_e, t_e, R_g, t_g, cam)
  np.testing.assert_allclose(got[3], d.mean(), rtol=1e-12)
  assert got[3] <= got[2]                       # ADI never exceeds ADD


def test_fixed_sum_shape():
  # 1e16 and then 256 strides of ones: the ones of one residue are summed before they meet
  # the big term only in this shape
  t = np.ones(600)
  t[0] = 2.0 ** 53
  p = np.zeros(256)
  for v in range(600):
    p[v % 256] = p[v % 256] + t[v]
  s = 128
  while s:
    for j in range(s):
      p[j] = p[j] + p[j + s]
    s //= 2
  assert ref.fixed_sum(t) == p[0]
  assert ref.fixed_sum([3.5]) == 3.5 and ref.fixed_sum(np.arange(257.0)) == 257 * 128.0


def test_special_cases_of_the_definition():
  syms = pe.symmetry_transformations({'symmetries_continuous': [
      {'axis': [0, 1, 0], 'offset': [0, 0, 0]}]})
  X, _, R_e, t_e, R_g, t_g, cam = _pair(5, 100, syms)
  assert (ref.errors(X, syms, R_g, t_g, R_g, t_g, cam) == 0).all()
  # behind the camera: MSPD +inf, MSSD finite
  e = ref.errors(X, syms, R_g, t_g * [1, 1, -1], R_g, t_g, cam)
  assert e[1] == np.inf and np.isfinite(e[[0, 2, 3]]).all()
  assert np.isnan(ref.errors(X, syms, R_e, t_e, R_g, t_g, cam, want_adi=False)[3])


# ------------------------------------------------------------------ symmetry sets ---
def _sym4(R, t):
  m = np.eye(4)
  m[:3, :3], m[:3, 3] = R, t
  return m.reshape(-1).tolist()


DISC = [_sym4(_rot([0, 0, 1], math.pi), [2.0, -4.0, 0.0]),
        _sym4(_rot([1, 0, 0], math.pi), [0.0, 0.0, 6.0])]
CONT = [{'axis': [0, 0, 1], 'offset': [1.0, -2.0, 0.5]}]


@pytest.mark.parametrize('info,count', [
    ({}, 1),
    ({'symmetries_discrete': DISC}, 3),
    ({'symmetries_continuous': CONT}, 315),
    ({'symmetries_discrete': DISC[:1], 'symmetries_continuous': CONT}, 630),
])
def test_symmetry_sets(info, count):
  s = pe.symmetry_transformations(info)
  assert s.shape == (count, 12) and s.dtype == np.float64
  assert s[0].tolist() == np.eye(3).reshape(-1).tolist() + [0.0, 0.0, 0.0]    # exactly
  R = s[:, :9].reshape(-1, 3, 3)
  np.testing.assert_allclose(np.einsum('nij,nkj->nik', R, R), np.broadcast_to(np.eye(3), R.shape),
                             atol=1e-14)
  np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=1e-14)


def test_continuous_symmetry_matrices_and_offset():
  n = int(math.ceil(math.pi / 0.01))
  assert n == 315
  s = pe.symmetry_transformations({'symmetries_continuous': CONT})
  off = np.array(CONT[0]['offset'])
  for i in (0, 1, 157, 314):
    np.testing.assert_allclose(s[i, :9].reshape(3, 3), _rot([0, 0, 1], i * 2 * math.pi / n),
                               atol=1e-14)
  # the axis passes through the offset: points on it stay fixed
  for lam in (-30.0, 0.0, 12.5):
    p = off + lam * np.array([0.0, 0.0, 1.0])
    moved = s[:, :9].reshape(-1, 3, 3).dot(p) + s[:, 9:]
    np.testing.assert_allclose(moved, np.broadcast_to(p, moved.shape), atol=1e-12)
  # a point off the axis keeps its distance to it and does move
  q = off + np.array([10.0, 0.0, 3.0])
  moved = s[:, :9].reshape(-1, 3, 3).dot(q) + s[:, 9:]
  np.testing.assert_allclose(np.linalg.norm((moved - off)[:, :2], axis=1), 10.0, atol=1e-12)
  assert np.linalg.norm(moved[157] - q) > 19.9
  # a coarser step
  assert len(pe.symmetry_transformations({'symmetries_continuous': CONT}, 0.5)) == 7


def test_combined_set_is_continuous_after_discrete():
  s = pe.symmetry_transformations({'symmetries_discrete': DISC[:1],
                                   'symmetries_continuous': CONT}, 0.5)
  assert len(s) == 14
  d = np.asarray(DISC[0]).reshape(4, 4)
  c = pe.symmetry_transformations({'symmetries_continuous': CONT}, 0.5)
  for i in range(7):
    Rc, tc = c[i, :9].reshape(3, 3), c[i, 9:]
    np.testing.assert_allclose(s[2 * i], c[i], atol=0)                  # c o identity
    np.testing.assert_allclose(s[2 * i + 1, :9].reshape(3, 3), Rc.dot(d[:3, :3]), atol=1e-15)
    np.testing.assert_allclose(s[2 * i + 1, 9:], Rc.dot(d[:3, 3]) + tc, atol=1e-14)


def test_load_models_info(tmp_path):
  p = tmp_path / 'models_info.json'
  p.write_text(json.dumps({'1': {'diameter': 10.5}, '12': {'diameter': 3.0,
                                                         'symmetries_continuous': CONT}}))
  info = pe.load_models_info(str(p))
  assert sorted(info) == [1, 12] and info[12]['symmetries_continuous'] == CONT
  assert pe.models_info_path('/b', 'ycbv') == '/b/ycbv/models_eval/models_info.json'


def test_rotation_and_translation_error():
  R = _rot([1, 2, 3], 0.7)
  assert pe.rotation_error(R, R) == pytest.approx(0.0, abs=1e-7)
  assert pe.rotation_error(_rot([0, 1, 0], 0.25).dot(R), R) == pytest.approx(0.25, abs=1e-12)
  assert pe.rotation_error(_rot([0, 1, 0], math.pi).dot(R), R) == pytest.approx(math.pi)
  assert pe.translation_error([1, 2, 3], [[4], [6], [3]]) == 5.0


# ------------------------------------------------------------------ matching and recall ---
def test_match_greedy_order_matters():
  # the better-scored estimate takes ground truth 1 (3 < 4); the other one is then left with
  # ground truth 0 at 60: one hit, where an optimal assignment would find two
  err = [[4.0, 3.0], [60.0, 2.0]]
  assert pe.match([0.9, 0.8], err, 5.0).tolist() == [1, -1]
  assert pe.match([0.8, 0.9], err, 5.0).tolist() == [0, 1]      # the other order: two hits
  assert pe.match([0.9, 0.8], err, 61.0).tolist() == [1, 0]
  assert pe.match([0.9, 0.8], err, 3.0).tolist() == [-1, 1]


def test_match_tie_threshold_and_surplus():
  # equal scores: file order
  assert pe.match([0.5, 0.5], [[20.0], [1.0]], 25.0).tolist() == [0, -1]
  assert pe.match([0.5, 0.5], [[1.0], [20.0]], 25.0).tolist() == [0, -1]
  # an error equal to the threshold is no hit
  assert pe.match([1.0], [[10.0]], 10.0).tolist() == [-1]
  assert pe.match([1.0], [[10.0]], np.nextafter(10.0, 11.0)).tolist() == [0]
  # more estimates than ground truths; equal errors go to the lowest ground-truth index
  assert pe.match([0.1, 0.3, 0.2], [[1.0, 1.0]] * 3, 2.0).tolist() == [-1, 0, 1]
  # non-finite errors, no ground truth, no estimate
  assert pe.match([1.0, 0.5], [[np.inf], [np.nan]], 1e300).tolist() == [-1, -1]
  assert pe.match([1.0], np.zeros((1, 0)), 5.0).tolist() == [-1]
  assert pe.match([], np.zeros((0, 2)), 5.0).tolist() == []


def _cols(e, mspd=None, add=None, adi=None):
  e = np.asarray(e, np.float64)
  return np.stack([e, e if mspd is None else np.asarray(mspd, np.float64),
                   e if add is None else np.asarray(add, np.float64),
                   e if adi is None else np.asarray(adi, np.float64)], axis=-1)


def test_recalls_by_hand():
  groups = [
      # object 1 (diameter 100, no symmetry), two instances: one hit at every threshold
      {'obj_id': 1, 'scores': [0.9, 0.8], 'errors': _cols([[4.0, 3.0], [60.0, 2.0]])},
      # an error of exactly 10: no hit at 5 and 10 (mm, px), a hit from 15 on; ADD 10 = 0.1 d
      {'obj_id': 1, 'scores': [0.7], 'errors': _cols([[10.0]])},
      # a non-finite estimate
      {'obj_id': 1, 'scores': [0.7], 'errors': _cols([[np.inf]])},
      # object 2 (diameter 50, symmetric): three estimates for one instance
      {'obj_id': 2, 'scores': [0.9, 0.8, 0.7],
       'errors': _cols([[100.0], [2.0], [1.0]], mspd=[[100.0], [7.0], [100.0]],
                       add=[[100.0]] * 3, adi=[[100.0], [4.0], [100.0]])},
      # no estimate for an instance
      {'obj_id': 2, 'scores': [], 'errors': np.zeros((0, 1, 4))},
  ]
  r = pe.recalls(groups, {1: 100.0, 2: 50.0}, {1: 1, 2: 315}, image_width=640)
  o1, o2, al = r['per_object'][1], r['per_object'][2], r['overall']
  assert (o1['targets'], o1['estimates']) == (4, 4)
  assert o1['recall_mssd'] == [0.25, 0.25] + [0.5] * 8 and o1['recall_mspd'] == o1['recall_mssd']
  assert o1['ar_mssd'] == pytest.approx(0.45) and o1['ar_mspd'] == pytest.approx(0.45)
  assert o1['add_s_recall'] == 0.25 and o1['add_s_error'] == 'add'
  assert (o2['targets'], o2['estimates']) == (2, 3)
  assert o2['recall_mssd'] == [0.5] * 10 and o2['recall_mspd'] == [0.0] + [0.5] * 9
  assert o2['ar_mssd'] == pytest.approx(0.5) and o2['ar_mspd'] == pytest.approx(0.45)
  assert o2['add_s_recall'] == 0.5 and o2['add_s_error'] == 'adi'
  assert (al['targets'], al['estimates']) == (6, 7)
  assert al['recall_mssd'] == pytest.approx([2 / 6.0] * 2 + [0.5] * 8)
  assert al['recall_mspd'] == pytest.approx([1 / 6.0, 2 / 6.0] + [0.5] * 8)
  assert al['ar_mssd'] == pytest.approx((4 / 6.0 + 4.0) / 10)
  assert al['ar_mspd'] == pytest.approx(0.45)
  assert al['add_s_recall'] == pytest.approx(2 / 6.0)
  assert al['mean_ar_mssd_mspd'] == pytest.approx(((4 / 6.0 + 4.0) / 10 + 0.45) / 2)
  # the pixel thresholds scale with the image width: at 1280 the error of 7 px is below 10 px
  r2 = pe.recalls(groups[3:4], {2: 50.0}, {2: 315}, image_width=1280)
  assert r2['overall']['recall_mspd'] == [1.0] * 10
  th = pe.thresholds(50.0, 1280)
  assert th['mspd'] == [10.0 * k for k in range(1, 11)] and th['add'] == 5.0
  assert th['mssd'] == pytest.approx([2.5 * k for k in range(1, 11)])


# ------------------------------------------------------------------ binding ---
def test_pose_error_symbols_declared_and_bound():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  for name, n_args in (('epos_pose_error_group_syms', 0), ('epos_pose_error_adi_tile', 0),
                       ('epos_pose_errors_f64', 10)):
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
    assert m, name
    params = m.group(1).strip()
    declared = 0 if params == 'void' else params.count(',') + 1
    assert declared == n_args == len(_lib.SYMBOLS[name][1]), name
  assert re.search(r'#define\s+EPOS_ABI_VERSION\s+7\b', header)
  lib = _lib.load()
  assert lib.epos_abi_version() == 7
  assert lib.epos_pose_error_group_syms() >= 1 and lib.epos_pose_error_adi_tile() >= 1
  # the record of the header, field by field
  assert ctypes.sizeof(_lib.PosePair) == 240 == pe.PAIR_DTYPE.itemsize
  for name, _ in _lib.PosePair._fields_:
    np_name = {'fx': 'cam'}.get(name, name)
    if name in ('fy', 'cx', 'cy'):
      continue
    assert getattr(_lib.PosePair, name).offset == pe.PAIR_DTYPE.fields[np_name][1], name
  assert _lib.PosePair.cy.offset == 232


# ------------------------------------------------------------------ eval_poses.py ---
def _frames_json(directory, gt=True):
  K = [[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]]
  pose = {'obj_id': 2, 'R': np.eye(3).reshape(-1).tolist(), 't': [0.0, 0.0, 500.0]}
  meta = [{'path': 'not_there_%d.npy' % i, 'scene_id': 3, 'im_id': i, 'K': K,
           'targets': {'2': 2}} for i in range(2)]
  if gt:
    for m in meta:
      m['gt_poses'] = [pose, dict(pose, t=[50.0, 0.0, 600.0])]
  with open(os.path.join(directory, 'frames.json'), 'w') as f:
    json.dump(meta, f)


def test_eval_poses_parser_and_refusals(tmp_path, monkeypatch):
  import eval_poses
  from epos_amd import cli
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  flags = {a.dest for a in eval_poses.build_parser()._actions}
  assert {'model', 'dataset', 'infer_tfrecord_names', 'frames', 'infer_name', 'result_path',
          'adi', 'synthetic', 'infer_crop_size'} <= flags
  args, model_dir = eval_poses.prepare(['--model', 'm', '--dataset', 'tudl', '--frames', 'x',
                                        '--infer_name', 'run', '--adi', 'false'])
  assert args.adi is False and model_dir == str(tmp_path / 'm')
  assert eval_poses.result_path(args, model_dir) == str(
      tmp_path / 'm' / 'infer' / 'estimated-poses_run.csv')
  assert eval_poses.prepare(['--model', 'm', '--dataset', 'tudl', '--frames', 'x'])[0].adi
  with pytest.raises(ValueError, match='no ground-truth poses'):
    eval_poses.prepare(['--model', 'm', '--dataset', 'tudl', '--synthetic', '4'])
  with pytest.raises(ValueError, match='dataset'):
    eval_poses.prepare(['--model', 'm', '--frames', 'x'])
  with pytest.raises(ValueError, match='No input files'):
    eval_poses.prepare(['--model', 'm', '--dataset', 'tudl'])
  # params.yml overrides flag defaults, as for eval.py
  os.makedirs(str(tmp_path / 'm'))
  (tmp_path / 'm' / 'params.yml').write_text('dataset: ycbv\ninfer_crop_size: [720, 540]\n')
  args, _ = eval_poses.prepare(['--model', 'm', '--frames', 'x'])
  assert args.dataset == 'ycbv' and cli.crop_size(args.infer_crop_size) == (720, 540)
  # frames without ground truth are refused before anything touches a device
  _frames_json(str(tmp_path), gt=False)
  with pytest.raises(ValueError, match='ground-truth poses'):
    eval_poses.main(['--model', 'm', '--frames', str(tmp_path)])


def test_eval_poses_reads_frames_json_without_images(tmp_path):
  import eval_poses
  from epos_amd import cli
  _frames_json(str(tmp_path))
  frames = cli.load_frames(None, str(tmp_path), 0, '640,480', 480, 0, 0, pixels=False)[0]
  assert [f.im_id for f in frames] == [0, 1] and frames[0].scene_id == 3
  assert frames[0].targets == {2: 2} and len(frames[1].gt_poses) == 2
  assert frames[0].K[0, 2] == 320.0 and os.listdir(str(tmp_path)) == ['frames.json']
  # the two best-scored estimates per (image, object) are kept, ties in file order; estimates
  # of other objects or images are counted as ignored
  def est(im, obj, score):
    return {'scene_id': 3, 'im_id': im, 'obj_id': obj, 'score': score, 'R': np.eye(3),
            't': np.zeros((3, 1))}
  results = [est(0, 2, 0.2), est(0, 2, 0.9), est(0, 2, 0.2), est(0, 5, 1.0), est(7, 2, 1.0),
             est(1, 2, 0.4)]
  groups, ignored = eval_poses.build_groups(frames, results)
  assert ignored == 3 and [len(g['ests']) for g in groups] == [2, 1]
  assert [e is results[i] for e, i in zip(groups[0]['ests'], (1, 0))] == [True, True]
  assert all(len(g['gts']) == 2 and g['obj_id'] == 2 for g in groups)
