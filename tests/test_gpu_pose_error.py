"""The pose-error kernels (csrc/pose_error.hip) against tests/helpers/pose_error_ref.py, bit for
bit: every shape regime, special inputs, determinism, the launcher's argument checks, and
eval_poses.py over them."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import mesh_cases, pose_error_ref as ref      # noqa: E402

pytestmark = pytest.mark.gpu

CAM = (1066.778, 1067.487, 312.9869, 241.3109)
E_INVALID = -1
SENTINEL = 123.25


def _lib():
  from epos_amd import _lib as binding
  return binding.load()


def _pe():
  from epos_amd import pose_error
  return pose_error


def _p(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _rot(axis, angle):
  return _pe().axis_rotation(angle, axis)


def sym_set(n, seed=0):
  """n rigid transforms, the identity first: rotations about an axis through an offset."""
  rng = np.random.RandomState(1000 + seed)
  axis, off = rng.randn(3), rng.uniform(-5, 5, 3)
  out = []
  for i in range(n):
    R = _rot(axis, i * 2 * math.pi / n)
    out.append(np.concatenate([R.reshape(9), off - R.dot(off)]))
  return np.stack(out)


class Pool(object):
  """Objects (n_verts, symmetry count or set) pooled as the launcher takes them. A few unused
  vertices and symmetries in front keep every base non-zero."""

  def __init__(self, shapes, seed=0, pad=(5, 3)):
    rng = np.random.RandomState(seed)
    self.verts, self.syms, self.objs = [rng.uniform(-9, 9, (pad[0], 3))], [sym_set(pad[1])], []
    nv, ns = pad
    for k, (n_verts, n_sym) in enumerate(shapes):
      X = rng.uniform(-60, 60, (n_verts, 3)) * rng.uniform(0.3, 1.0, 3)
      S = sym_set(n_sym, seed + k) if isinstance(n_sym, int) else np.asarray(n_sym, np.float64)
      n_sym = len(S)
      self.objs.append((nv, n_verts, ns, n_sym, X, S))
      self.verts.append(X)
      self.syms.append(S)
      nv += n_verts
      ns += n_sym
    self.verts, self.syms = np.concatenate(self.verts), np.concatenate(self.syms)
    self.d_verts = torch.from_numpy(self.verts).cuda()
    self.d_syms = torch.from_numpy(self.syms).cuda()

  def pair(self, obj, R_e, t_e, R_g, t_g, cam=CAM):
    rec = np.zeros(1, _pe().PAIR_DTYPE)[0]
    rec['vert_base'], rec['n_verts'], rec['sym_base'], rec['n_sym'] = self.objs[obj][:4]
    rec['R_e'], rec['t_e'] = np.reshape(R_e, 9), np.reshape(t_e, 3)
    rec['R_g'], rec['t_g'] = np.reshape(R_g, 9), np.reshape(t_g, 3)
    rec['cam'] = cam
    return rec

  def random_pair(self, obj, rng, angle=0.08, shift=8.0):
    R_g = _rot(rng.randn(3), rng.uniform(0, 3))
    t_g = np.array([rng.uniform(-80, 80), rng.uniform(-60, 60), rng.uniform(500, 900)])
    return self.pair(obj, _rot(rng.randn(3), angle).dot(R_g), t_g + rng.randn(3) * shift, R_g, t_g)

  def ref(self, rec, want_adi=True):
    for base, n_verts, sbase, n_sym, X, S in self.objs:
      if base == rec['vert_base'] and sbase == rec['sym_base']:
        return ref.errors(X, S, rec['R_e'], rec['t_e'], rec['R_g'], rec['t_g'], rec['cam'],
                          want_adi)
    raise KeyError

  def launch(self, recs, want_adi=True, err=None, rc_only=False, n_pairs=None,
             totals=None):
    tab = np.array(recs, _pe().PAIR_DTYPE)
    n = len(tab) if n_pairs is None else n_pairs
    dev = torch.empty((max(1, len(tab)) * 240,), dtype=torch.uint8, device='cuda')
    if err is None:
      err = torch.full((max(1, len(tab)), 4), SENTINEL, dtype=torch.float64, device='cuda')
    nv, ns = totals or (len(self.verts), len(self.syms))
    rc = _lib().epos_pose_errors_f64(
        _p(self.d_verts), nv, _p(self.d_syms), ns, ctypes.c_void_p(tab.ctypes.data), _p(dev), n,
        int(want_adi), _p(err), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()                       # `tab` is read by the copy until here
    if rc_only:
      return rc, err.cpu().numpy()
    assert rc == 0, _lib().epos_last_error()
    return err.cpu().numpy()[:len(tab)]


def assert_same_bytes(got, exp):
  got, exp = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(exp, np.float64)
  assert got.shape == exp.shape
  assert got.tobytes() == exp.tobytes(), (got, exp, got - exp)


def _regimes():
  lib = _lib()
  return lib.epos_pose_error_group_syms(), lib.epos_pose_error_adi_tile()


N_VERTS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 'tile-1', 'tile', 'tile+1', '2tile+1']
N_SYM = [1, 2, 7, 315, 'group-1', 'group', 'group+1', '2group+1']


@pytest.mark.parametrize('n_sym', N_SYM)
@pytest.mark.parametrize('n_verts', N_VERTS)
def test_errors_match_reference_bit_for_bit(n_verts, n_sym):
  group, tile = _regimes()
  n_verts = {'tile-1': tile - 1, 'tile': tile, 'tile+1': tile + 1,
             '2tile+1': 2 * tile + 1}.get(n_verts, n_verts)
  n_sym = {'group-1': group - 1, 'group': group, 'group+1': group + 1,
           '2group+1': 2 * group + 1}.get(n_sym, n_sym)
  assert n_verts >= 1 and n_sym >= 1
  pool = Pool([(n_verts, n_sym)], seed=n_verts * 7 + n_sym)
  rng = np.random.RandomState(n_verts + 31 * n_sym)
  recs = [pool.random_pair(0, rng) for _ in range(3)]
  got = pool.launch(recs)
  exp = np.stack([pool.ref(r) for r in recs])
  assert np.isfinite(exp).all() and (exp[:, :3] > 0).all()
  assert_same_bytes(got, exp)
  assert_same_bytes(pool.launch(recs[:1]), exp[:1])              # n_pairs = 1


@pytest.fixture(scope='module')
def mixed():
  """70 pairs over five objects of different sizes and symmetry counts, and their reference."""
  group, tile = _regimes()
  pool = Pool([(1000, 315), (65, 1), (2 * tile + 1, 2), (1, group + 1), (257, 7)], seed=4)
  rng = np.random.RandomState(11)
  recs = [pool.random_pair(i % 5, rng, angle=0.02 + 0.05 * (i % 7), shift=1.0 + i)
          for i in range(70)]
  return pool, recs, np.stack([pool.ref(r) for r in recs])


def test_mixed_table_of_70_pairs(mixed):
  pool, recs, exp = mixed
  got = pool.launch(recs)
  assert_same_bytes(got, exp)
  assert_same_bytes(pool.launch(recs), got)                      # the same launch twice
  rows = np.concatenate([pool.launch([r]) for r in recs])        # 70 single-pair launches
  assert_same_bytes(rows, got)
  order = np.random.RandomState(0).permutation(70)               # and in another order
  assert_same_bytes(pool.launch([recs[i] for i in order]), got[order])


def test_want_adi_zero_leaves_column_three(mixed):
  pool, recs, exp = mixed
  got = pool.launch(recs, want_adi=False)
  assert_same_bytes(got[:, :3], exp[:, :3])
  assert (got[:, 3] == SENTINEL).all()


def test_special_inputs():
  pe = _pe()
  cont = pe.symmetry_transformations({'symmetries_continuous': [
      {'axis': [0, 0, 1], 'offset': [1.0, -2.0, 0.5]}]})
  four = sym_set(4, 77)
  # object 2: a real continuous set; object 3: duplicated symmetries, which tie
  pool = Pool([(300, 1), (300, four), (300, cont), (300, four[[0, 1, 1, 0, 3, 3, 2, 1, 0, 2]])],
              seed=9)
  rng = np.random.RandomState(2)
  base = pool.random_pair(2, rng)
  R_g, t_g = base['R_g'].reshape(3, 3), base['t_g'].copy()
  X = pool.objs[2][4]
  diameter = max(np.linalg.norm(X - x, axis=1).max() for x in X)
  recs, kinds = [], []
  for obj in (0, 1, 2, 3):                          # estimate = ground truth: exactly 0
    recs.append(pool.pair(obj, R_g, t_g, R_g, t_g))
    kinds.append('same')
  for k in (1, 100, 314):                           # estimate = ground truth o symmetry k
    R_e, t_e = ref.compose(R_g, t_g, cont[k])
    recs.append(pool.pair(2, R_e, t_e, R_g, t_g))
    kinds.append('sym')
  recs.append(pool.random_pair(3, rng))             # duplicated symmetries
  kinds.append('dup')
  far = pool.random_pair(2, rng)                    # translations of 1e6 mm
  far['t_g'] = [2.0e5, -1.0e5, 1.0e6]
  far['t_e'] = far['t_g'] + np.array([3.0, -2.0, 40.0])
  recs.append(far)
  kinds.append('far')
  behind = pool.random_pair(1, rng)                 # the estimate behind the camera
  behind['t_e'] = behind['t_g'] * [1, 1, -1]
  recs.append(behind)
  kinds.append('behind')
  gt_behind = pool.random_pair(1, rng)              # ... and the ground truth
  gt_behind['t_g'] = gt_behind['t_e'] * [1, 1, -1]
  recs.append(gt_behind)
  kinds.append('behind')
  straddle = pool.random_pair(0, rng)               # some vertices at Z <= 0, some in front
  straddle['t_e'] = [0.0, 0.0, 5.0]
  recs.append(straddle)
  kinds.append('behind')
  got = pool.launch(recs)
  exp = np.stack([pool.ref(r) for r in recs])
  assert_same_bytes(got, exp)
  for row, kind in zip(got, kinds):
    if kind == 'same':
      assert (row == 0).all()
    elif kind == 'sym':
      assert 0 <= row[0] <= 1e-9 * diameter and 0 <= row[1] <= 1e-9 * diameter
      assert row[2] > 0.1                           # ADD does see the rotation about the axis
    elif kind == 'behind':
      assert row[1] == np.inf and np.isfinite(row[[0, 2, 3]]).all()
    else:
      assert np.isfinite(row).all() and (row > 0).all()
  # the duplicates change nothing: the same pair over the set without them
  dup = recs[7]
  assert_same_bytes(got[7], ref.errors(pool.objs[3][4], four, dup['R_e'], dup['t_e'], dup['R_g'],
                                       dup['t_g'], dup['cam']))


def test_refusals_come_before_any_launch():
  """Return codes only: ordinary argument checks, nothing is launched or copied."""
  pool = Pool([(40, 3), (10, 1)], seed=1)
  rng = np.random.RandomState(0)
  good = pool.random_pair(0, rng)
  nv, ns = len(pool.verts), len(pool.syms)

  def changed(**kw):
    rec = good.copy()
    for k, v in kw.items():
      rec[k] = v
    return rec
  bad = [changed(n_verts=0), changed(n_verts=-4), changed(n_sym=0), changed(n_sym=-1),
         changed(vert_base=-1), changed(vert_base=nv), changed(vert_base=nv - 39),
         changed(sym_base=-1), changed(sym_base=ns - 2), changed(vert_base=2 ** 31 - 1),
         changed(n_verts=2 ** 31 - 1), changed(n_sym=2 ** 31 - 1)]
  for rec in bad:
    for recs in ([rec], [good, rec], [rec, good]):
      rc, err = pool.launch(recs, rc_only=True)
      assert rc == E_INVALID, rec
      assert (err == SENTINEL).all()
  assert b'epos_pose_errors_f64' in _lib().epos_last_error()
  assert pool.launch([good], rc_only=True, n_pairs=-1)[0] == E_INVALID
  assert pool.launch([good], rc_only=True, totals=(nv, 5))[0] == E_INVALID
  assert pool.launch([good], rc_only=True, totals=(44, ns))[0] == E_INVALID
  rc, err = pool.launch([good], rc_only=True, n_pairs=0)           # nothing to do
  assert rc == 0 and (err == SENTINEL).all()
  lib = _lib()
  assert lib.epos_pose_errors_f64(None, 0, None, 0, None, None, 0, 1, None, None) == 0
  assert lib.epos_pose_errors_f64(None, nv, None, ns, None, None, 1, 1, None, None) == E_INVALID
  # the ranges that just fit are accepted
  edge = changed(vert_base=nv - 40, sym_base=ns - 3)
  rc, err = pool.launch([edge], rc_only=True)
  assert rc == 0 and np.isfinite(err[0]).all()


# ------------------------------------------------------------------ public interface ---
def _diameter(pts):
  return float(max(np.linalg.norm(pts - p, axis=1).max() for p in pts))


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
  """$BOP_PATH/tudl/models_eval with three small meshes (object 2 with a continuous, object 3
  with a discrete symmetry), a frames.json with ground-truth poses and no image files, and a
  hand-made result CSV under $TF_MODELS_PATH/m/infer/."""
  from epos_amd import bop_io, ply
  pe = _pe()
  root = tmp_path_factory.mktemp('pose_eval')
  bop, models_dir, frames_dir = root / 'bop', root / 'models', root / 'frames'
  eval_models = bop / 'tudl' / 'models_eval'
  os.makedirs(str(eval_models))
  os.makedirs(str(models_dir / 'm' / 'infer'))
  os.makedirs(str(frames_dir))
  meshes = {1: mesh_cases.icosphere(1, 40.0, (1.0, 0.7, 0.5)),
            2: mesh_cases.icosphere(2, 30.0, (1.0, 1.0, 1.6)),
            3: mesh_cases.soup(3, 70, 90)}
  info = {}
  for o, (verts, faces) in meshes.items():
    ply.save_ply(ply.model_path(str(bop), 'tudl', o, 'eval'), verts, faces)
  models = ply.load_models(str(bop), 'tudl', 'eval', obj_ids=[1, 2, 3])
  for o in meshes:
    info[str(o)] = {'diameter': _diameter(models[o]['pts'])}
  info['2']['symmetries_continuous'] = [{'axis': [0, 0, 1], 'offset': [0, 0, 0]}]
  m = np.eye(4)
  m[:3, :3] = _rot([0, 0, 1], math.pi)
  info['3']['symmetries_discrete'] = [m.reshape(-1).tolist()]
  with open(str(eval_models / 'models_info.json'), 'w') as f:
    json.dump(info, f)
  syms = {o: pe.symmetry_transformations(info[str(o)]) for o in meshes}

  rng = np.random.RandomState(5)

  def gt(o):
    return {'obj_id': o, 'R': _rot(rng.randn(3), rng.uniform(0, 3)),
            't': np.array([rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(500, 800)])}
  K = [np.array([[600.0, 0, 320.0], [0, 610.0, 240.0], [0, 0, 1]]),
       np.array([[580.0, 0, 300.0], [0, 585.0, 250.0], [0, 0, 1]])]
  frames = [{'scene_id': 2, 'im_id': 10, 'K': K[0], 'targets': {1: 2, 2: 1},
             'gt': [gt(1), gt(2), gt(1)]},
            {'scene_id': 2, 'im_id': 11, 'K': K[1], 'targets': {2: 1, 3: 2},
             'gt': [gt(3), gt(2), gt(3)]}]
  with open(str(frames_dir / 'frames.json'), 'w') as f:
    json.dump([{'path': 'im_%d.png' % fr['im_id'], 'scene_id': fr['scene_id'],
                'im_id': fr['im_id'], 'K': fr['K'].tolist(),
                'targets': {str(k): v for k, v in fr['targets'].items()},
                'gt_poses': [{'obj_id': g['obj_id'], 'R': g['R'].reshape(-1).tolist(),
                              't': g['t'].tolist()} for g in fr['gt']]} for fr in frames], f)

  def est(fr, o, score, R, t):
    return {'scene_id': fr['scene_id'], 'im_id': fr['im_id'], 'obj_id': o, 'score': score,
            'R': np.asarray(R).reshape(3, 3), 't': np.asarray(t).reshape(3, 1), 'time': 0.1}

  def nudged(g, angle, shift):
    return _rot([1, 2, 3], angle).dot(g['R']), g['t'] + np.array(shift)
  f0, f1 = frames
  g = f0['gt']
  sym_R, sym_t = ref.compose(g[1]['R'], g[1]['t'], syms[2][123])
  results = [
      est(f0, 1, 0.1, *nudged(g[0], 1.0, [90.0, 0, 0])),       # wrong, and cut: third of two
      est(f0, 1, 0.9, g[0]['R'], g[0]['t']),                   # exact
      est(f0, 1, 0.8, *nudged(g[2], 0.01, [0.3, -0.2, 0.5])),  # slightly perturbed
      est(f0, 2, 0.7, sym_R, sym_t),                           # symmetric-equivalent
      est(f1, 2, 0.95, f1['gt'][1]['R'], [np.nan, 0.0, 600.0]),    # non-finite, best-scored
      est(f1, 2, 0.6, f1['gt'][1]['R'], f1['gt'][1]['t']),     # exact but cut: second of one
      est(f1, 3, 0.5, *nudged(f1['gt'][2], 0.02, [1.0, 1.0, -2.0])),
      est(f1, 3, 0.4, *nudged(f1['gt'][0], 2.0, [0, 150.0, 0])),   # wrong
      est(f1, 1, 0.9, g[0]['R'], g[0]['t']),                   # no target in this image
  ]
  bop_io.save_bop_results(str(models_dir / 'm' / 'infer' / 'estimated-poses.csv'), results)
  return {'bop': str(bop), 'models_dir': str(models_dir), 'frames_dir': str(frames_dir),
          'models': models, 'syms': syms, 'info': info, 'frames': frames, 'results': results}


def _expected_groups(ds, kept):
  """kept: per group (frame index, object, indices into results in score order)."""
  groups = []
  for fi, o, idx in kept:
    fr = ds['frames'][fi]
    gts = [g for g in fr['gt'] if g['obj_id'] == o]
    cam = (fr['K'][0, 0], fr['K'][1, 1], fr['K'][0, 2], fr['K'][1, 2])
    err = np.zeros((len(idx), len(gts), 4))
    for a, i in enumerate(idx):
      e = ds['results'][i]
      for b, g in enumerate(gts):
        if not (np.isfinite(e['R']).all() and np.isfinite(e['t']).all()):
          err[a, b] = np.inf
        else:
          err[a, b] = ref.errors(ds['models'][o]['pts'], ds['syms'][o], e['R'], e['t'], g['R'],
                                 g['t'], cam)
    groups.append({'obj_id': o, 'scores': [ds['results'][i]['score'] for i in idx],
                   'errors': err})
  return groups


def test_eval_poses_end_to_end(dataset, monkeypatch):
  import eval_poses
  pe = _pe()
  ds = dataset
  monkeypatch.setenv('BOP_PATH', ds['bop'])
  monkeypatch.setenv('TF_MODELS_PATH', ds['models_dir'])
  assert os.listdir(ds['frames_dir']) == ['frames.json']          # no image files
  scores = eval_poses.main(['--model', 'm', '--dataset', 'tudl', '--frames', ds['frames_dir']])
  out = os.path.join(ds['models_dir'], 'm', 'eval')
  assert json.load(open(os.path.join(out, 'pose_scores.json'))) == json.loads(json.dumps(scores))
  groups = _expected_groups(ds, [(0, 1, [1, 2]), (0, 2, [3]), (1, 2, [4]), (1, 3, [6, 7])])
  diam = {o: ds['info'][str(o)]['diameter'] for o in (1, 2, 3)}
  exp = pe.recalls(groups, diam, {1: 1, 2: 315, 3: 2}, image_width=640)
  assert scores['overall'] == exp['overall']
  assert scores['per_object'] == {str(o): r for o, r in exp['per_object'].items()}
  assert scores['n_symmetries'] == {'1': 1, '2': 315, '3': 2}
  assert scores['counts'] == {
      'frames': 2, 'estimates_in_file': 9, 'estimates_scored': 6, 'estimates_ignored': 3,
      'targets': 6, 'pairs': 2 * 2 + 1 + 1 + 2 * 2, 'non_finite_pairs': 1}
  # by hand: object 1 -- both instances found at every threshold; object 2 -- the symmetric
  # equivalent is a hit, the non-finite estimate is none; object 3 -- one of two
  po = scores['per_object']
  assert po['1']['recall_mssd'] == [1.0] * 10 and po['1']['add_s_recall'] == 1.0
  assert po['2']['recall_mssd'] == [0.5] * 10 and po['2']['recall_mspd'] == [0.5] * 10
  assert po['2']['add_s_recall'] == 0.5 and po['2']['add_s_error'] == 'adi'
  assert po['3']['recall_mssd'][-1] == 0.5 and po['3']['targets'] == 2
  assert scores['overall']['mean_ar_mssd_mspd'] == (
      scores['overall']['ar_mssd'] + scores['overall']['ar_mspd']) / 2
  rows = open(os.path.join(out, 'pose_errors.csv')).read().strip().split('\n')
  assert rows[0].startswith('scene_id,im_id,obj_id') and len(rows) == 1 + 10
  first = [float(v) for v in rows[1].split(',')[6:]]              # the exact estimate
  assert first[:4] == [0.0] * 4 and first[5] == 0.0 and first[4] < 1e-7
  # --infer_name and --adi false: other file names, no ADD(-S) figure for symmetric objects
  src = os.path.join(ds['models_dir'], 'm', 'infer', 'estimated-poses.csv')
  dst = os.path.join(ds['models_dir'], 'm', 'infer', 'estimated-poses_run2.csv')
  with open(dst, 'w') as f:
    f.write(open(src).read())
  s2 = eval_poses.main(['--model', 'm', '--dataset', 'tudl', '--frames', ds['frames_dir'],
                        '--infer_name', 'run2', '--adi', 'false'])
  assert os.path.exists(os.path.join(out, 'pose_scores_run2.json'))
  assert os.path.exists(os.path.join(out, 'pose_errors_run2.csv'))
  assert s2['overall']['ar_mssd'] == scores['overall']['ar_mssd']
  assert s2['per_object']['1']['add_s_recall'] == 1.0
  assert s2['per_object']['2']['add_s_recall'] is None and s2['overall']['add_s_recall'] is None


def test_pose_error_eval_class(dataset):
  pe = _pe()
  ds = dataset
  info = {int(k): v for k, v in ds['info'].items()}
  ev = pe.PoseErrorEval(ds['models'], info, 'cuda:0', chunk_pairs=4)   # two launches
  assert [ev.n_sym(o) for o in (1, 2, 3)] == [1, 315, 2]
  rng = np.random.RandomState(1)
  pairs, exp = [], []
  for i in range(9):
    o = 1 + i % 3
    R_g = _rot(rng.randn(3), rng.uniform(0, 3))
    t_g = np.array([rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(500, 800)])
    R_e, t_e = _rot(rng.randn(3), 0.05).dot(R_g), t_g + rng.randn(3) * 3
    if i == 4:
      t_e = t_e * np.array([1.0, np.inf, 1.0])
    K = np.array([[600.0 + i, 0, 320.0], [0, 610.0, 240.0], [0, 0, 1]])
    pairs.append({'obj_id': o, 'R_e': R_e, 't_e': t_e.reshape(3, 1), 'R_g': R_g, 't_g': t_g,
                  'K': K})
    if i == 4:
      exp.append([np.inf] * 6)
    else:
      four = ref.errors(ds['models'][o]['pts'], ds['syms'][o], R_e, t_e, R_g, t_g,
                        (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
      exp.append(list(four) + [pe.rotation_error(R_e, R_g), pe.translation_error(t_e, t_g)])
  got = ev.errors(pairs)
  assert got.shape == (9, 6)
  assert_same_bytes(got, np.array(exp))
  assert abs(got[0, 4] - 0.05) < 1e-9
  no_adi = ev.errors(pairs, want_adi=False)
  assert_same_bytes(no_adi[:, [0, 1, 2, 4, 5]], got[:, [0, 1, 2, 4, 5]])
  assert np.isnan(no_adi[[0, 1, 2, 3, 5, 6, 7, 8], 3]).all() and no_adi[4, 3] == np.inf
  assert ev.errors([]).shape == (0, 6)
