"""The VSD kernel (csrc/vsd.hip) against tests/helpers/vsd_ref.py, exactly: every image and
window regime, special inputs, ties, determinism, the launcher's argument checks, VsdEval over
the renderer, and eval_poses.py --vsd over both depth sources."""
import ctypes
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import mesh_cases, vsd_ref as ref      # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID = -1
SENTINEL = -77
CAM = (61.5, 59.25, 30.75, 3.5)


def _lib():
  from epos_amd import _lib as binding
  return binding.load()


def _vsd():
  from epos_amd import vsd
  return vsd


def _p(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def rec(image, gt, est, win, cam=CAM, diameter=80.0):
  r = np.zeros(1, _vsd().PAIR_DTYPE)[0]
  r['image'], r['gt_inst'], r['est_inst'] = image, gt, est
  r['x0'], r['y0'], r['x1'], r['y1'] = win
  r['fx'], r['fy'], r['cx'], r['cy'] = cam
  r['diameter'] = diameter
  return r


def launch(depth_test, depth_model, recs, delta=15.0, taus=None, rc_only=False, n_pairs=None,
           shape=None, nulls=()):
  """One epos_vsd_counts call; counts start as SENTINEL. shape: (n_images, n_inst, h, w) told
  to the launcher instead of the arrays' own."""
  taus = np.ascontiguousarray(_vsd().VSD_TAUS if taus is None else taus, np.float64)
  tab = np.array(recs, _vsd().PAIR_DTYPE)
  n = len(tab) if n_pairs is None else n_pairs
  d_test = torch.from_numpy(np.ascontiguousarray(depth_test, np.float32)).cuda()
  d_model = torch.from_numpy(np.ascontiguousarray(depth_model, np.float32)).cuda()
  n_img, n_inst, h, w = shape or (d_test.shape[0], d_model.shape[0]) + tuple(d_test.shape[1:])
  dev = torch.empty((max(1, len(tab)) * 72,), dtype=torch.uint8, device='cuda')
  counts = torch.full((max(1, len(tab)), 6 + max(1, len(taus))), SENTINEL, dtype=torch.int64,
                      device='cuda')
  ptrs = {'test': _p(d_test), 'model': _p(d_model), 'pairs': ctypes.c_void_p(tab.ctypes.data),
          'dev': _p(dev), 'taus': ctypes.c_void_p(taus.ctypes.data), 'counts': _p(counts)}
  for k in nulls:
    ptrs[k] = None
  rc = _lib().epos_vsd_counts(
      ptrs['test'], n_img, ptrs['model'], n_inst, h, w, ptrs['pairs'], ptrs['dev'], n,
      float(delta), ptrs['taus'], len(taus), ptrs['counts'],
      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  torch.cuda.synchronize()                         # `tab` is read by the copy until here
  if rc_only:
    return rc, counts.cpu().numpy()
  assert rc == 0, _lib().epos_last_error()
  return counts.cpu().numpy()[:len(tab)]


def scene(h, w, n_images=2, n_inst=3, seed=0):
  """Synthetic depth maps: renderings with a background of 0 and depths in 400..700 mm, test
  images that are in places missing (0, negative, NaN), in front of, behind and right at the
  renderings."""
  rng = np.random.RandomState(seed)
  model = np.where(rng.rand(n_inst, h, w) < 0.35, 0.0,
                   rng.uniform(400, 700, (n_inst, h, w))).astype(np.float32)
  model[1:] = np.where(rng.rand(n_inst - 1, h, w) < 0.5, model[:1] + rng.uniform(
      -30, 30, (n_inst - 1, h, w)).astype(np.float32), model[1:]) * (model[1:] > 0)
  test = rng.uniform(380, 720, (n_images, h, w)).astype(np.float32)
  near = rng.rand(n_images, h, w) < 0.4
  test = np.where(near, model[rng.randint(0, n_inst, (n_images, h, w)),
                              np.arange(h)[None, :, None], np.arange(w)[None, None, :]] +
                  rng.uniform(-25, 25, (n_images, h, w)), test).astype(np.float32)
  kind = rng.rand(n_images, h, w)
  test[kind < 0.08] = 0.0
  test[(kind >= 0.08) & (kind < 0.12)] = -5.0
  test[(kind >= 0.12) & (kind < 0.16)] = np.nan
  return test, model


def windows(h, w, bands):
  """Full, empty, one column, one row, unaligned offsets, fewer rows than row bands, more."""
  wins = [(0, 0, w, h), (0, 0, 0, 0), (w, h, w, h), (w // 2, 0, w // 2, h),
          (w - 1, 0, w, h), (0, h - 1, w, h), (0, 0, w, 1), (0, 0, 1, 1)]
  if w > 2 and h > 2:
    wins += [(1, 1, w - 1, h - 1), (w // 3, h // 3, w - w // 4, h - h // 4)]
  if w > 66:
    wins += [(3, 0, 67, h), (1, 0, 66, 1), (65, 0, w, h), (63, 1, 65, 2)]
  if h > 1:
    wins.append((0, 1, w, min(h, 1 + max(1, bands - 1))))
  return wins


SIZES = [(1, 1), (7, 5), (63, 3), (64, 4), (65, 3), (130, 9), (257, 2), (40, 70)]


@pytest.mark.parametrize('n_taus', [1, 10, 16])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_counts_equal_reference(size, n_taus):
  w, h = size
  bands = _lib().epos_vsd_row_bands()
  if size == (40, 70):
    assert h > 2 * bands             # a wavefront walks more than two rows of the window
  test, model = scene(h, w, seed=w * 131 + h)
  taus = np.linspace(0.02, 0.6, n_taus) if n_taus > 1 else np.array([0.1])
  recs = []
  for k, win in enumerate(windows(h, w, bands)):
    recs.append(rec(k % 2, k % 3, (k + 1) % 3, win, diameter=60.0 + k))
    recs.append(rec(1 - k % 2, 2 - k % 3, -1 if k % 2 else 2 - k % 3, win,
                    cam=(w * 1.1, w * 0.9, w / 2.0 + 0.25, h / 2.0)))
  got = launch(test, model, recs, taus=taus)
  exp = ref.counts_table(test, model, recs, 15.0, taus)
  assert got.dtype == np.int64 and got.shape == exp.shape == (len(recs), 6 + n_taus)
  assert (got == exp).all(), (got, exp)
  if w * h > 100:
    full = exp[0]                                     # the full window sees every regime
    assert full[1] < full[0] and full[4] > 0 and full[5] > full[4] and full[3] < full[2]
    assert full[6] > 0 and (np.diff(exp[:, 6:], axis=1) <= 0).all()
  assert (launch(test, model, recs[:1], taus=taus) == exp[:1]).all()        # n_pairs = 1


def test_seventy_pairs_share_images_and_instances():
  w, h = 130, 9
  test, model = scene(h, w, n_images=3, n_inst=5, seed=7)
  rng = np.random.RandomState(1)
  recs = []
  for i in range(70):
    x0, y0 = rng.randint(0, w), rng.randint(0, h)
    win = (x0, y0, rng.randint(x0, w + 1), rng.randint(y0, h + 1)) if i % 5 else (0, 0, w, h)
    # many pairs on image 2 and ground truth 4; every seventh without an estimate
    recs.append(rec(2 if i % 3 else i % 3, 4 if i % 2 else i % 5, -1 if i % 7 == 0 else i % 5,
                    win, diameter=50.0 + i))
  got = launch(test, model, recs)
  exp = ref.counts_table(test, model, recs, 15.0, _vsd().VSD_TAUS)
  assert (got == exp).all()
  assert got.tobytes() == launch(test, model, recs).tobytes()           # the same call twice
  rows = np.concatenate([launch(test, model, [r]) for r in recs[:12]])    # single-pair calls
  assert (rows == got[:12]).all()
  order = rng.permutation(70)
  assert (launch(test, model, [recs[i] for i in order]) == got[order]).all()
  for i in range(0, 70, 7):                        # no estimate: nothing of it is counted
    assert got[i, 2] == got[i, 3] == got[i, 4] == 0 and got[i, 5] == got[i, 1]
    assert (got[i, 6:] == 0).all()


def test_tight_and_full_windows_agree():
  w, h = 130, 41
  test, model = scene(h, w, n_images=1, n_inst=2, seed=3)
  model[:, :7] = 0                                 # nothing outside rows 7..29, columns 33..101
  model[:, 30:] = 0
  model[:, :, :33] = 0
  model[:, :, 102:] = 0
  tight, full = rec(0, 0, 1, (33, 7, 102, 30)), rec(0, 0, 1, (0, 0, w, h))
  got = launch(test, model, [tight, full])
  assert (got[0] == got[1]).all() and got[0, 4] > 100
  assert (got == ref.counts_table(test, model, [tight, full], 15.0, _vsd().VSD_TAUS)).all()


def test_special_inputs():
  w, h = 65, 3
  zeros = np.zeros((h, w), np.float32)
  gt = np.full((h, w), 500.0, np.float32)
  est = np.full((h, w), 520.0, np.float32)
  model = np.stack([gt, est, zeros])
  tests = np.stack([zeros,                                   # all missing: 0
                    np.full((h, w), -3.0, np.float32),       # negative
                    np.full((h, w), np.nan, np.float32),     # NaN
                    np.full((h, w), 100.0, np.float32),      # everything occluded
                    np.full((h, w), 9000.0, np.float32)])    # a far background
  full = (0, 0, w, h)
  recs = [rec(0, 0, 1, full), rec(1, 0, 1, full), rec(2, 0, 1, full),   # missing -> visible
          rec(3, 0, 1, full),                                # ground truth fully occluded
          rec(4, 2, 2, full),                                # both renderings empty
          rec(4, 0, 2, full), rec(4, 0, -1, full),           # estimate empty / absent
          rec(4, 2, 0, full),                                # ground truth empty
          rec(4, 0, 0, full)]                                # estimate = ground truth
  got = launch(tests, model, recs)
  exp = ref.counts_table(tests, model, recs, 15.0, _vsd().VSD_TAUS)
  assert (got == exp).all()
  n = w * h
  for i in (0, 1, 2):
    assert got[i, :6].tolist() == [n] * 6 and got[i, 6] == n     # 20 mm / 80 mm = 0.25 and up
    assert got[i, 6 + 4] == n and got[i, 6 + 5] == 0             # tau 0.25 is reached, 0.30 not
  assert got[3].tolist() == [n, 0, n, 0, 0, 0] + [0] * 10
  assert got[4].tolist() == [0] * 16
  assert got[5].tolist() == got[6].tolist() == [n, n, 0, 0, 0, n] + [0] * 10
  assert got[7].tolist() == [0, 0, n, n, 0, n] + [0] * 10
  assert got[8].tolist() == [n, n, n, n, n, n] + [0] * 10
  v = _vsd().vsd_from_counts(got)
  assert v[3].tolist() == [1.0] * 10 and v[4].tolist() == [1.0] * 10
  assert v[5].tolist() == [1.0] * 10 and v[8].tolist() == [0.0] * 10
  assert v[0].tolist() == [1.0] * 5 + [0.0] * 5
  assert _vsd().visib_fract(got)[[0, 3, 4]].tolist() == [1.0, 0.0, 0.0]


def test_exact_ties_count():
  """dg - dt == delta is visible, d == tau counts: on the principal ray (x + .5 == cx, y + .5
  == cy) s is exactly 1, so the distances are the depths themselves."""
  w, h = 7, 5
  cam = (50.0, 50.0, 3.5, 2.5)                     # the ray of pixel (3, 2)
  gt, est, test = (np.zeros((h, w), np.float32) for _ in range(3))
  gt[2, 3], est[2, 3] = 100.0, 105.0
  test[2, 3] = 85.0                                # dg - dt == 15 == delta; de - dt == 20
  model = np.stack([gt, est])
  pair = rec(0, 0, 1, (0, 0, w, h), cam=cam, diameter=100.0)
  got = launch(test[None], model, [pair], delta=15.0, taus=[0.05])
  assert (got == ref.counts_table(test[None], model, [pair], 15.0, [0.05])).all()
  # the ground truth is visible by the tie, the estimate through it; 5 / 100 >= 0.05
  assert got[0].tolist() == [1, 1, 1, 1, 1, 1, 1]
  # one step of fp32 nearer and the ground truth is hidden (and with it the estimate)
  test[2, 3] = np.nextafter(np.float32(85.0), np.float32(0))
  got = launch(test[None], model, [pair], delta=15.0, taus=[0.05])
  assert got[0].tolist() == [1, 0, 1, 0, 0, 0, 0]
  # a tau just above the tie is not reached
  test[2, 3] = 85.0
  got = launch(test[None], model, [pair], delta=15.0, taus=[np.nextafter(0.05, 1.0), 0.05])
  assert got[0].tolist() == [1, 1, 1, 1, 1, 1, 0, 1]


def test_refusals_come_before_any_launch():
  """Return codes only: ordinary argument checks, nothing is launched, copied or cleared."""
  w, h = 20, 10
  test, model = scene(h, w, seed=5)                # 2 images, 3 instances
  full = (0, 0, w, h)
  good = rec(1, 2, 0, full)

  def changed(**kw):
    r = good.copy()
    for k, v in kw.items():
      r[k] = v
    return r
  bad = [changed(image=-1), changed(image=2), changed(gt_inst=-1), changed(gt_inst=3),
         changed(est_inst=-2), changed(est_inst=3), changed(image=2 ** 31 - 1),
         changed(x0=-1), changed(x1=w + 1), changed(y0=-1), changed(y1=h + 1),
         changed(x0=5, x1=4), changed(y0=6, y1=2), changed(x0=w + 1, x1=w + 1),
         changed(diameter=0.0), changed(diameter=-1.0), changed(diameter=np.nan),
         changed(diameter=np.inf), changed(fx=0.0), changed(fy=0.0), changed(fx=np.nan),
         changed(fy=np.inf), changed(fx=-np.inf)]
  for r in bad:
    for recs in ([r], [good, r], [r, good]):
      rc, counts = launch(test, model, recs, rc_only=True)
      assert rc == E_INVALID, r
      assert (counts == SENTINEL).all()
  assert b'epos_vsd_counts' in _lib().epos_last_error()
  for kw in ({'n_pairs': -1}, {'taus': np.zeros(17)}, {'delta': np.nan}, {'delta': np.inf},
             {'shape': (2, 2 ** 31 // (h * w) + 1, h, w)}, {'shape': (2, 1 << 20, 1 << 6, 1 << 5)},
             {'nulls': ('test',)}, {'nulls': ('model',)}, {'nulls': ('pairs',)},
             {'nulls': ('dev',)}, {'nulls': ('taus',)}, {'nulls': ('counts',)}):
    rc, counts = launch(test, model, [good], rc_only=True, **kw)
    assert rc == E_INVALID, kw
    assert (counts == SENTINEL).all()
  lib = _lib()
  tau = np.array([0.1])
  one = ctypes.c_void_p(tau.ctypes.data)
  assert lib.epos_vsd_counts(None, 0, None, 0, 0, 0, None, None, 1, 15.0, one, 0, None,
                             None) == E_INVALID                          # n_taus = 0
  # nothing to do
  rc, counts = launch(test, model, [good], rc_only=True, n_pairs=0)
  assert rc == 0 and (counts == SENTINEL).all()
  assert lib.epos_vsd_counts(None, 0, None, 0, 0, 0, None, None, 0, 15.0, None, 1, None,
                             None) == 0
  # the edges that just fit are accepted: the last indices, an empty window at the corner,
  # est_inst = -1, a negative focal length, 16 taus
  edge = [changed(image=1, gt_inst=2, est_inst=2, x0=w, x1=w, y0=h, y1=h),
          changed(est_inst=-1), changed(fx=-50.0)]
  taus = np.linspace(0.01, 0.9, 16)
  rc, counts = launch(test, model, edge, rc_only=True, taus=taus)
  assert rc == 0 and (counts == ref.counts_table(test, model, edge, 15.0, taus)).all()


# ------------------------------------------------------------------ VsdEval ---
W, H = 48, 40
K0 = np.array([[110.0, 0.0, 24.3], [0.0, 112.0, 19.6], [0.0, 0.0, 1.0]])
K1 = np.array([[100.0, 0.0, 22.0], [0.0, 100.0, 21.0], [0.0, 0.0, 1.0]])


def _rot(axis, angle):
  from epos_amd import pose_error
  return pose_error.axis_rotation(angle, axis)


def _meshes():
  return {1: mesh_cases.icosphere(1, 40.0, (1.0, 0.7, 0.5)),
          2: mesh_cases.icosphere(2, 30.0, (1.0, 1.0, 1.6))}


def _diameter(pts):
  return float(max(np.linalg.norm(pts - p, axis=1).max() for p in pts))


def _render(ev, obj_id, R, t, K):
  return ev.renderer.render_instances([obj_id], np.reshape(R, (1, 3, 3)), np.reshape(t, (1, 3)),
                                      K, size=(W, H), outputs=('depth',))['depth'][0].cpu().numpy()


def _nearest(depths):
  d = np.stack(depths)
  return np.where((d > 0).any(axis=0), np.where(d > 0, d, np.inf).min(axis=0), 0.0)


def _expected(ev, depth, K, obj_id, gt, est, diameter, delta=15.0):
  """Counts of one pair by the reference on downloaded renderings, full-image window."""
  dg = _render(ev, obj_id, gt[0], gt[1], K)
  finite = est is not None and np.isfinite(est[0]).all() and np.isfinite(est[1]).all()
  model = np.stack([dg, _render(ev, obj_id, est[0], est[1], K) if finite else np.zeros_like(dg)])
  pair = rec(0, 0, 1 if finite else -1, (0, 0, W, H), cam=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]),
             diameter=diameter)
  return ref.counts(depth[None], model, pair, delta, _vsd().VSD_TAUS)


@pytest.fixture(scope='module')
def world():
  """Two icospheres, three frames of 48 x 40 with ground truths, and test depth images made of
  the downloaded ground-truth renderings, an occluding rectangle and a hole of zeros."""
  vsd = _vsd()
  meshes = _meshes()
  models = {o: {'pts': v, 'faces': f} for o, (v, f) in meshes.items()}
  info = {o: {'diameter': _diameter(v)} for o, (v, f) in meshes.items()}
  ev = vsd.VsdEval(models, info, 'cuda:0')
  rng = np.random.RandomState(8)

  def gt(o, x, y, z):
    return {'obj_id': o, 'R': _rot(rng.randn(3), rng.uniform(0, 3)), 't': np.array([x, y, z])}
  frames = [{'K': K0, 'gt': [gt(1, -45.0, -20.0, 420.0), gt(2, 40.0, 25.0, 380.0),
                             gt(1, 30.0, -35.0, 520.0)]},
            {'K': K1, 'gt': [gt(2, -10.0, 5.0, 330.0), gt(1, 60.0, 40.0, 450.0)]},
            {'K': K0, 'gt': [gt(2, 0.0, 0.0, 400.0)]}]
  for fi, fr in enumerate(frames):
    rend = [_render(ev, g['obj_id'], g['R'], g['t'], fr['K']) for g in fr['gt']]
    assert all((r > 0).sum() > 40 for r in rend)
    depth = _nearest(rend)
    depth[depth == 0] = 900.0                           # a background wall
    depth[H // 2 - 2:H // 2 + 3, 5:W - 5] = 0.0         # a hole: no measurement
    if fi == 0:
      # an occluder over the whole of ground truth 1 (object 2), chosen from its own mask
      ys, xs = np.nonzero(rend[1] > 0)
      depth[ys.min():ys.max() + 1, xs.min():xs.max() + 1] = 200.0
    if fi == 1:
      depth[:, :W // 2 - 4] = np.minimum(depth[:, :W // 2 - 4], 250.0)    # a partial occluder
    fr['depth'] = np.round(depth).astype(np.float32)    # whole mm: a 16-bit PNG holds them
  return {'ev': ev, 'models': models, 'info': info, 'frames': frames, 'meshes': meshes}


def _nudged(g, angle, shift):
  return _rot([1, 2, 3], angle).dot(g['R']), g['t'] + np.array(shift)


def test_vsd_eval_end_to_end(world):
  vsd = _vsd()
  ev, frames = world['ev'], world['frames']
  fdepth = [(fr['depth'], fr['K']) for fr in frames]
  pairs, exp = [], []

  def add(fi, gi, est):
    g = frames[fi]['gt'][gi]
    pairs.append({'frame': fi, 'obj_id': g['obj_id'], 'R_g': g['R'], 't_g': g['t'],
                  'R_e': None if est is None else est[0],
                  't_e': None if est is None else np.reshape(est[1], (3, 1))})
    exp.append(_expected(ev, frames[fi]['depth'], frames[fi]['K'], g['obj_id'],
                         (g['R'], g['t']), est, world['info'][g['obj_id']]['diameter']))
  f0, f1 = frames[0]['gt'], frames[1]['gt']
  add(0, 0, (f0[0]['R'], f0[0]['t']))                   # exact
  add(0, 0, _nudged(f0[0], 0.2, [6.0, -4.0, 12.0]))     # the same ground truth, another estimate
  add(0, 1, _nudged(f0[1], 0.1, [3.0, 3.0, 5.0]))       # covered ground truth
  add(0, 2, _nudged(f0[2], 0.3, [-8.0, 2.0, -20.0]))
  add(0, 2, None)                                       # ground truth only
  add(1, 0, _nudged(f1[0], 0.05, [1.0, 1.0, 2.0]))
  add(1, 1, _nudged(f1[1], 0.5, [300.0, 0.0, 0.0]))     # an estimate outside the image
  add(1, 1, (f1[1]['R'], np.array([0.0, 0.0, -400.0])))    # behind the camera: full window
  add(2, 0, _nudged(frames[2]['gt'][0], 0.1, [2.0, 0.0, 30.0]))
  add(2, 0, (frames[2]['gt'][0]['R'], np.array([np.nan, 0.0, 400.0])))     # non-finite
  exp = np.stack(exp)
  got_vsd, got_fract = ev.errors(fdepth, pairs)
  assert got_vsd.shape == (len(pairs), 10) and got_fract.shape == (len(pairs),)
  assert (got_vsd == vsd.vsd_from_counts(exp)).all()
  assert (got_fract == vsd.visib_fract(exp)).all()
  assert (ev.counts(fdepth, pairs) == exp).all()
  # what the scene was built for
  assert (got_vsd[0] == 0.0).all() and got_fract[0] > 0.5
  assert 0.0 < got_vsd[1, 0] and got_vsd[1, -1] < got_vsd[1, 0]
  assert got_fract[2] == 0.0 and (got_vsd[2] == 1.0).all()          # covered
  assert (got_vsd[4] == 1.0).all() and got_fract[4] == got_fract[3]
  assert (got_vsd[6] == 1.0).all() and (got_vsd[9] == 1.0).all() and got_fract[9] > 0.5
  assert 0.0 < got_fract[5] < 1.0                                     # partly occluded
  # chunking: two instances per chunk, and everything in one, give the same
  for cap in (2, 3, 10 ** 6):
    small = vsd.VsdEval(world['models'], world['info'], 'cuda:0', max_instances=cap)
    chunks, skipped = small.plan(fdepth, pairs)
    assert not skipped and all(len(c['inst']) <= cap for c in chunks)
    assert (len(chunks) > 4) if cap == 2 else True
    v, f = small.errors(fdepth, pairs)
    assert v.tobytes() == got_vsd.tobytes() and f.tobytes() == got_fract.tobytes()
  chunks, _ = ev.plan(fdepth, pairs)
  assert len(chunks) == 1 and len(chunks[0]['inst']) == 6 + 7 and chunks[0]['frames'] == [0, 1, 2]
  # full-image windows give the same counts as the host windows
  full = ev.table(chunks[0], full_windows=True)
  assert (full['x1'] == W).all() and (ev.table(chunks[0])['x1'] < W).any()
  # a non-finite ground truth or camera never reaches the device
  bad = [dict(pairs[0], t_g=np.array([0.0, np.inf, 400.0])), dict(pairs[0])]
  v, f = ev.errors(fdepth, bad)
  assert (v[0] == 1.0).all() and f[0] == 0.0 and (v[1] == got_vsd[0]).all()
  v, f = ev.errors([(frames[0]['depth'], K0 * np.nan)], [dict(pairs[0], frame=0)])
  assert (v == 1.0).all() and (f == 0.0).all()
  v, f = ev.errors(fdepth, [])
  assert v.shape == (0, 10) and f.shape == (0,)
  with pytest.raises(ValueError):
    vsd.VsdEval(world['models'], world['info'], 'cuda:0', max_instances=1)


# ------------------------------------------------------------------ eval_poses.py ---
@pytest.fixture(scope='module')
def dataset(world, tmp_path_factory):
  """$BOP_PATH/tudl with models_eval and test/000002/{depth/*.png, scene_camera.json}, a
  frames directory with depth .npy files, one without any depth, and a result CSV."""
  from epos_amd import bop_io, ply
  root = tmp_path_factory.mktemp('vsd_eval')
  bop, models_dir = root / 'bop', root / 'models'
  frames_dir, plain_dir = root / 'frames', root / 'frames_plain'
  eval_models = bop / 'tudl' / 'models_eval'
  scene_dir = bop / 'tudl' / 'test' / '000002'
  for d in (eval_models, scene_dir / 'depth', models_dir / 'm' / 'infer', frames_dir, plain_dir):
    os.makedirs(str(d))
  for o, (verts, faces) in world['meshes'].items():
    ply.save_ply(ply.model_path(str(bop), 'tudl', o, 'eval'), verts, faces)
  # the models as the script will load them (fp32 vertices in the file)
  models = ply.load_models(str(bop), 'tudl', 'eval', obj_ids=[1, 2])
  info = {str(o): {'diameter': _diameter(models[o]['pts'])} for o in models}
  with open(str(eval_models / 'models_info.json'), 'w') as f:
    json.dump(info, f)
  frames = world['frames']
  meta, cams = [], {}
  for i, fr in enumerate(frames):
    im_id = 10 + i
    targets = {}
    for g in fr['gt']:
      targets[str(g['obj_id'])] = targets.get(str(g['obj_id']), 0) + 1
    meta.append({'path': 'im_%d.png' % im_id, 'scene_id': 2, 'im_id': im_id,
                 'K': fr['K'].tolist(), 'targets': targets,
                 'gt_poses': [{'obj_id': g['obj_id'], 'R': g['R'].reshape(-1).tolist(),
                               't': g['t'].tolist()} for g in fr['gt']]})
    # frames.json route: float32 mm in a .npy; --depth_split route: tenths of a mm in a PNG
    np.save(str(frames_dir / ('depth_%d.npy' % im_id)), fr['depth'])
    bop_io.save_depth_png(str(scene_dir / 'depth' / ('%06d.png' % im_id)),
                          (fr['depth'] * 10).astype(np.uint16))
    cams[str(im_id)] = {'cam_K': fr['K'].reshape(-1).tolist(), 'depth_scale': 0.1}
  with open(str(scene_dir / 'scene_camera.json'), 'w') as f:
    json.dump(cams, f)
  with open(str(plain_dir / 'frames.json'), 'w') as f:
    json.dump(meta, f)
  with open(str(frames_dir / 'frames.json'), 'w') as f:
    json.dump([dict(m, depth_path='depth_%d.npy' % m['im_id']) for m in meta], f)

  def est(fi, o, score, R, t):
    return {'scene_id': 2, 'im_id': 10 + fi, 'obj_id': o, 'score': score,
            'R': np.asarray(R).reshape(3, 3), 't': np.asarray(t).reshape(3, 1), 'time': 0.1}
  f0, f1, f2 = (fr['gt'] for fr in frames)
  results = [
      est(0, 1, 0.9, f0[0]['R'], f0[0]['t']),                         # exact
      est(0, 1, 0.8, *_nudged(f0[2], 0.1, [4.0, -3.0, 9.0])),         # slightly off
      est(0, 1, 0.1, *_nudged(f0[0], 1.0, [90.0, 0, 0])),             # cut: third of two
      est(0, 2, 0.7, *_nudged(f0[1], 0.05, [1.0, 1.0, 2.0])),         # the covered instance
      est(1, 2, 0.6, *_nudged(f1[0], 0.3, [10.0, 5.0, 25.0])),
      est(1, 1, 0.5, f1[1]['R'], [np.nan, 0.0, 450.0]),               # non-finite
      est(2, 2, 0.4, *_nudged(f2[0], 0.02, [0.5, 0.5, 1.0])),
  ]
  bop_io.save_bop_results(str(models_dir / 'm' / 'infer' / 'estimated-poses.csv'), results)
  return {'bop': str(bop), 'models_dir': str(models_dir), 'frames_dir': str(frames_dir),
          'plain_dir': str(plain_dir), 'models': models, 'info': info, 'frames': frames,
          'results': bop_io.load_bop_results(
              str(models_dir / 'm' / 'infer' / 'estimated-poses.csv'))}


def _expected_groups(ds, kept, delta=15.0, skip_gt=()):
  """kept: per group (frame index, object, indices into results in score order). The errors
  by the reference, on renderings of the models and poses as the script reads them."""
  vsd = _vsd()
  ev = vsd.VsdEval(ds['models'], {int(k): v for k, v in ds['info'].items()}, 'cuda:0')
  groups, rows = [], []
  for fi, o, idx in kept:
    fr = ds['frames'][fi]
    gts = [g for k, g in enumerate(g_ for g_ in fr['gt'] if g_['obj_id'] == o)
           if (fi, o, k) not in skip_gt]
    err = np.ones((len(idx), len(gts), 10))
    for a, i in enumerate(idx):
      e = ds['results'][i]
      for b, g in enumerate(gts):
        # frames.json stores the ground truth as json numbers: they round-trip exactly
        c = _expected(ev, fr['depth'], fr['K'], o, (g['R'], g['t']), (e['R'], e['t'][:, 0]),
                      ds['info'][str(o)]['diameter'], delta)
        err[a, b] = vsd.vsd_from_counts(c[None])[0]
        rows.append((10 + fi, o, a, b, err[a, b], vsd.visib_fract(c[None])[0]))
    groups.append({'obj_id': o, 'scores': [ds['results'][i]['score'] for i in idx], 'vsd': err})
  return groups, rows


KEPT = [(0, 1, [0, 1]), (0, 2, [3]), (1, 1, [5]), (1, 2, [4]), (2, 2, [6])]


def _check_scores(ds, scores, kept=KEPT, skip_gt=()):
  vsd = _vsd()
  groups, rows = _expected_groups(ds, kept, skip_gt=skip_gt)
  exp = vsd.recalls_vsd(groups)
  for got, want in [(scores['overall'], exp['overall'])] + [
      (scores['per_object'][str(o)], exp['per_object'][o]) for o in exp['per_object']]:
    assert got['recall_vsd'] == want['recall_vsd'] and got['ar_vsd'] == want['ar_vsd']
    assert np.shape(got['recall_vsd']) == (10, 10)
    assert got['targets'] == want['targets']
    assert got['ar'] == (got['ar_vsd'] + got['ar_mssd'] + got['ar_mspd']) / 3.0
    assert got['mean_ar_mssd_mspd'] == (got['ar_mssd'] + got['ar_mspd']) / 2
  assert scores['thresholds']['vsd_taus'] == list(vsd.VSD_TAUS)
  assert scores['thresholds']['vsd_thresholds'] == list(vsd.VSD_THRESHOLDS)
  assert scores['vsd_delta'] == 15.0
  return rows


@pytest.mark.parametrize('source', ['frames_json', 'depth_split'])
def test_eval_poses_vsd(dataset, monkeypatch, capsys, source):
  import eval_poses
  ds = dataset
  monkeypatch.setenv('BOP_PATH', ds['bop'])
  monkeypatch.setenv('TF_MODELS_PATH', ds['models_dir'])
  argv = ['--model', 'm', '--dataset', 'tudl', '--vsd', 'true', '--infer_name', source]
  # --depth_split does not need depth entries in frames.json: the plain directory will do
  argv += (['--frames', ds['frames_dir']] if source == 'frames_json' else
           ['--frames', ds['plain_dir'], '--depth_split', 'test'])
  infer_dir = os.path.join(ds['models_dir'], 'm', 'infer')
  shutil.copy(os.path.join(infer_dir, 'estimated-poses.csv'),
              os.path.join(infer_dir, 'estimated-poses_%s.csv' % source))
  scores = eval_poses.main(argv)
  printed = capsys.readouterr().out
  assert 'AR_VSD=%.4f' % scores['overall']['ar_vsd'] in printed
  assert 'AR=%.4f' % scores['overall']['ar'] in printed and 'AR_MSSD=' in printed
  out = os.path.join(ds['models_dir'], 'm', 'eval')
  assert json.load(open(os.path.join(out, 'pose_scores_%s.json' % source))) == \
      json.loads(json.dumps(scores))
  rows = _check_scores(ds, scores)
  assert 'targets_dropped_by_visibility' not in scores['counts']
  assert scores['counts']['targets'] == 6 and scores['counts']['pairs'] == 4 + 1 + 1 + 1 + 1
  # by hand: object 1 -- the exact estimate is a hit everywhere, the non-finite one never
  assert scores['per_object']['1']['recall_vsd'][0][0] >= 1.0 / 3
  assert 0.0 < scores['overall']['ar_vsd'] < 1.0
  lines = open(os.path.join(out, 'pose_errors_%s.csv' % source)).read().strip().split('\n')
  head = lines[0].split(',')
  assert head[:6] == ['scene_id', 'im_id', 'obj_id', 'est_rank', 'gt_index', 'score']
  assert head[6:12] == ['mssd', 'mspd', 'add', 'adi', 're', 'te']
  assert head[12:] == ['vsd_%.2f' % (0.05 * k) for k in range(1, 11)] + ['gt_visib_fract']
  assert len(lines) == 1 + len(rows)
  for line, (im_id, o, a, b, err, fract) in zip(lines[1:], rows):
    cells = line.split(',')
    assert [int(c) for c in cells[:5]] == [2, im_id, o, a, b]
    assert [float(c) for c in cells[12:22]] == err.tolist() and float(cells[22]) == fract
  first = [float(c) for c in lines[1].split(',')[12:]]
  assert first[:10] == [0.0] * 10 and first[10] > 0.5                # the exact estimate


def test_eval_poses_min_visib_fract(dataset, monkeypatch):
  import eval_poses
  ds = dataset
  monkeypatch.setenv('BOP_PATH', ds['bop'])
  monkeypatch.setenv('TF_MODELS_PATH', ds['models_dir'])
  # the reference's own counts say which instance is below the bound: the covered one alone
  vsd = _vsd()
  ev = vsd.VsdEval(ds['models'], {int(k): v for k, v in ds['info'].items()}, 'cuda:0')
  low = []
  for fi, fr in enumerate(ds['frames']):
    seen = {}
    for g in fr['gt']:
      k = seen.get(g['obj_id'], 0)
      seen[g['obj_id']] = k + 1
      c = _expected(ev, fr['depth'], fr['K'], g['obj_id'], (g['R'], g['t']), None,
                    ds['info'][str(g['obj_id'])]['diameter'])
      assert c[0] > 40
      if c[1] < 0.1 * c[0]:
        low.append((fi, g['obj_id'], k))
      else:
        assert c[1] >= 0.2 * c[0]                       # nothing sits near the bound
  assert low == [(0, 2, 0)]
  scores = eval_poses.main(['--model', 'm', '--dataset', 'tudl', '--frames', ds['frames_dir'],
                            '--vsd', 'true', '--min_visib_fract', '0.1', '--infer_name', 'vis',
                            '--result_path', os.path.join(ds['models_dir'], 'm', 'infer',
                                                          'estimated-poses.csv')])
  assert scores['counts']['targets_dropped_by_visibility'] == 1
  assert scores['min_visib_fract'] == 0.1
  assert scores['counts']['targets'] == 5 and scores['per_object']['2']['targets'] == 2
  # its estimate is no longer scored: the instance count of (image 10, object 2) is 0
  assert scores['counts']['estimates_scored'] == 5 and scores['counts']['pairs'] == 4 + 1 + 1 + 1
  _check_scores(ds, scores, [(0, 1, [0, 1]), (0, 2, []), (1, 1, [5]), (1, 2, [4]), (2, 2, [6])],
                skip_gt={(0, 2, 0)})
  # without --vsd the bound still applies, and no VSD figure appears
  s2 = eval_poses.main(['--model', 'm', '--dataset', 'tudl', '--frames', ds['plain_dir'],
                        '--depth_split', 'test', '--min_visib_fract', '0.1', '--infer_name',
                        'vis2', '--result_path', scores['result_path']])
  assert s2['counts']['targets_dropped_by_visibility'] == 1 and s2['counts']['targets'] == 5
  assert 'ar_vsd' not in s2['overall'] and 'vsd_taus' not in s2['thresholds']
  assert s2['overall']['ar_mssd'] == scores['overall']['ar_mssd']


def test_eval_poses_without_the_flag_ignores_depth(dataset, monkeypatch):
  """Without --vsd the files are byte for byte those of a folder that holds no depth at all."""
  import eval_poses
  ds = dataset
  monkeypatch.setenv('BOP_PATH', ds['bop'])
  monkeypatch.setenv('TF_MODELS_PATH', ds['models_dir'])
  out = os.path.join(ds['models_dir'], 'm', 'eval')

  def run(frames_dir):
    eval_poses.main(['--model', 'm', '--dataset', 'tudl', '--frames', frames_dir])
    return (open(os.path.join(out, 'pose_scores.json'), 'rb').read(),
            open(os.path.join(out, 'pose_errors.csv'), 'rb').read())
  with_depth, plain = run(ds['frames_dir']), run(ds['plain_dir'])
  assert with_depth == plain
  scores = json.loads(plain[0].decode())
  assert 'ar_vsd' not in scores['overall'] and 'vsd_delta' not in scores
  assert sorted(scores['thresholds']) == ['add_s_x_diameter', 'max_sym_disc_step',
                                          'mspd_px', 'mspd_px_at_width_640', 'mssd_x_diameter']
  assert plain[1].decode().split('\n')[0].endswith(',re,te')
