"""The device-side ordering stage (csrc/corresp_order.hip) through the C ABI, bit for bit
against its numpy restatement (tests/helpers/order_ref.py) in every launch regime, and the
ordered fitting entry against the host entry given the same confidence-ordered rows."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import fit_scenes, order_ref  # noqa: E402

pytestmark = pytest.mark.gpu

W = 160                   # head-map width of the synthetic rows (640 / 4)
GUARD = 32                # guard elements behind every output buffer


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr())


def _lib():
  from epos_amd import _lib as L
  return L, L.load()


def tile_rows():
  return _lib()[1].epos_corr_order_tile_rows()


def make_slot(rng, n, conf='random', rows='random'):
  """n rows in raster order, several rows per pixel, as epos_corr_fill writes them: (conf f32,
  px_id i64, coord_2d, coord_3d). The masked pixels lie in a band of the head map narrower
  than W and px_id is the index among the MASKED pixels (corresp.py:92), so px_id // W is not
  the image row: the row order has to come from coord_2d y."""
  band = 23                                            # masked columns 40 .. 62 of W = 160
  if rows == 'one_row':
    cell = 7 * band + np.sort(rng.integers(0, band, n))
  elif rows == 'row_each':
    cell = np.arange(n, dtype=np.int64) * band + rng.integers(0, band, n)
  else:
    cell = np.sort(rng.integers(0, band * max(2, min(120, n // 3 + 2)), n))
  cell = cell.astype(np.int64)
  x, y = 40 + cell % band, cell // band
  px = np.unique(cell, return_inverse=True)[1].astype(np.int64)     # dense masked-pixel index
  if conf == 'equal':
    c = np.full(n, 0.37)
  elif conf == 'three':
    c = rng.choice([0.2, 0.21, 0.9], n)
  elif conf == 'increasing':
    c = np.linspace(0.01, 0.99, n) if n > 1 else np.full(n, 0.5)
  elif conf == 'decreasing':
    c = np.linspace(0.99, 0.01, n) if n > 1 else np.full(n, 0.5)
  else:
    c = rng.uniform(1e-4, 1.0, n)
  xy = np.stack([(x + 0.5) * 4.0, (y + 0.5) * 4.0], 1)
  xyz = rng.uniform(-80, 80, (n, 3))
  return c.astype(np.float32), px, xy, xyz


def pool(slots, capacity=None):
  """Pooled arrays of `capacity` rows (default: the total) and slot_base; rows beyond the
  capacity are dropped from the arrays but stay in slot_base (an overflowed fill)."""
  ns = [len(s[0]) for s in slots]
  slot_base = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
  cap = int(slot_base[-1]) if capacity is None else capacity
  cat = [np.concatenate([s[i] for s in slots]) if slots else None for i in range(4)]
  out = []
  for a, tail, dt in zip(cat, [(), (), (2,), (3,)], [np.float32, np.int64, np.float64, np.float64]):
    full = np.zeros((cap,) + tail, dt)
    if a is not None:
      m = min(cap, len(a))
      full[:m] = a[:m]
    out.append(full)
  return out, slot_base, cap


def run_stage(arrays, slot_base, cap, K, always):
  """The C call on buffers sized exactly for the expected rows + GUARD sentinel elements;
  returns the outputs as numpy arrays after checking the guards."""
  L, lib = _lib()
  conf, px, xy, xyz = arrays
  exp = order_ref.order_stage(conf, xy, xyz, slot_base, cap, K, always)
  n_out = int(exp['slot_base_out'][-1])
  S = len(slot_base) - 1
  d = 'cuda:0'
  dev = [torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in (conf, px, xy, xyz)]
  sb = torch.from_numpy(slot_base).to(d)

  def guarded(n, dt, fill):
    return torch.full((n + GUARD,), fill, dtype=dt, device=d)
  sbo = guarded(S + 1, torch.int64, -77)
  c2 = guarded(2 * n_out, torch.float64, -77.0)
  c3 = guarded(3 * n_out, torch.float64, -77.0)
  src, yo, yp = (guarded(n_out, torch.int32, -77) for _ in range(3))
  wbytes = lib.epos_corr_order_workspace_bytes(S, cap)
  assert wbytes >= 0
  work = torch.full((wbytes + GUARD,), 0x5a, dtype=torch.uint8, device=d)
  rc = lib.epos_corr_order_by_conf(
      _ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), _ptr(sb), S, cap, W,
      K if K is not None else 0, int(always), _ptr(work), _ptr(sbo), _ptr(c2), _ptr(c3),
      _ptr(src), _ptr(yo), _ptr(yp), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  L.check(rc, 'epos_corr_order_by_conf')
  torch.cuda.synchronize()
  got = {}
  for name, buf, n in [('slot_base_out', sbo, S + 1), ('coord_2d', c2, 2 * n_out),
                       ('coord_3d', c3, 3 * n_out), ('src_row', src, n_out),
                       ('yorder', yo, n_out), ('ypos', yp, n_out), ('work', work, wbytes)]:
    h = buf.cpu().numpy()
    assert (h[n:] == (0x5a if name == 'work' else -77)).all(), 'guard behind ' + name
    got[name] = h[:n]
  return got, exp


def check_case(slots, K, always, capacity=None):
  arrays, slot_base, cap = pool(slots, capacity)
  got, exp = run_stage(arrays, slot_base, cap, K, always)
  for name in ('slot_base_out', 'src_row', 'yorder', 'ypos'):
    assert np.array_equal(got[name], exp[name]), (name, K, always)
  for name in ('coord_2d', 'coord_3d'):          # gathered doubles: byte-equal
    assert got[name].tobytes() == exp[name].ravel().tobytes(), (name, K, always)
  # slots left in their order have identity permutations
  for s, applied in enumerate(exp['applied']):
    lo, hi = exp['slot_base_out'][s], exp['slot_base_out'][s + 1]
    if not applied:
      assert np.array_equal(got['src_row'][lo:hi], np.arange(hi - lo))
      assert np.array_equal(got['yorder'][lo:hi], np.arange(hi - lo))
  return exp


def k_values(n):
  return [None] + [k for k in (1, n - 1, n, n + 1) if k > 0]


@pytest.mark.parametrize('always', [0, 1])
def test_slot_sizes_and_caps(always):
  """One slot of every size around the wavefront and the in-LDS limit T, and of about 4 T rows
  (three merge passes, an odd run left over), with every cap around the size."""
  T = tile_rows()
  rng = np.random.default_rng(11 + always)
  for n in [0, 1, 5, 63, 64, 65, 257, T - 1, T, T + 1, 4 * T + 3]:
    slot = make_slot(rng, n)
    for K in k_values(n):
      check_case([slot], K, always)


@pytest.mark.parametrize('always', [0, 1])
def test_five_slots_with_empty_ones(always):
  T = tile_rows()
  rng = np.random.default_rng(21)
  slots = [make_slot(rng, n) for n in (0, 300, 0, T + 50, 0)]
  for K in (None, 100, 300):
    exp = check_case(slots, K, always)
    assert exp['slot_base_out'][1] == 0 and exp['slot_base_out'][-1] == exp['slot_base_out'][-2]
  check_case([make_slot(rng, 0) for _ in range(5)], 10, always)


@pytest.mark.parametrize('always', [0, 1])
@pytest.mark.parametrize('conf', ['equal', 'three', 'increasing', 'decreasing'])
def test_confidence_patterns(conf, always):
  T = tile_rows()
  rng = np.random.default_rng(31)
  for n in (257, 2 * T + 5):
    slot = make_slot(rng, n, conf=conf)
    for K in (None, n // 2):
      check_case([slot], K, always)


@pytest.mark.parametrize('always', [0, 1])
@pytest.mark.parametrize('rows', ['one_row', 'row_each'])
def test_image_row_patterns(rows, always):
  T = tile_rows()
  rng = np.random.default_rng(41)
  for n in (150, T + 9):
    slot = make_slot(rng, n, rows=rows)
    for K in (None, n - 40):
      check_case([slot], K, always)


@pytest.mark.parametrize('always', [0, 1])
def test_total_equal_to_capacity_and_overflow(always):
  rng = np.random.default_rng(51)
  slots = [make_slot(rng, n) for n in (300, 500, 400)]
  for K in (None, 350):
    check_case(slots, K, always, capacity=1200)          # pooled total == capacity
    # slot_base[S] = 1200 > capacity: slot 2 is cut to the 200 rows below it
    exp = check_case(slots, K, always, capacity=1000)
    assert exp['slot_base_out'][-1] == (1000 if K is None else 300 + 350 + 200)
    # ... and a slot that STARTS beyond the capacity is empty
    exp = check_case(slots, K, always, capacity=700)
    assert exp['slot_base_out'][-1] == exp['slot_base_out'][-2]


def test_argument_checks():
  L, lib = _lib()
  assert lib.epos_corr_order_workspace_bytes(-1, 10) < 0
  assert lib.epos_corr_order_workspace_bytes(3, -1) < 0
  z = torch.zeros(64, dtype=torch.int64, device='cuda:0')
  p = _ptr(z)
  args = lambda S, cap, conf: (conf, p, p, p, p, S, cap, W, 0, 1, p, p, p, p, p, p, p, None)   # noqa: E731
  assert lib.epos_corr_order_by_conf(*args(-1, 4, p)) == -1
  assert lib.epos_corr_order_by_conf(*args(1, -4, p)) == -1
  assert lib.epos_corr_order_by_conf(*args(1, 4, None)) == -1
  # capacity 0: every bound is 0, nothing else is touched
  sbo = torch.full((4,), 9, dtype=torch.int64, device='cuda:0')
  rc = lib.epos_corr_order_by_conf(None, None, None, None, p, 3, 0, W, 0, 1, None, _ptr(sbo),
                                   None, None, None, None, None, None)
  assert rc == 0
  torch.cuda.synchronize()
  assert sbo.cpu().tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------
# fitting level
# ---------------------------------------------------------------------------------------------
def _scenes():
  rng = np.random.default_rng(7)
  out = []
  for n_inst, tz in [(1, 700.0), (1, 900.0), (2, 800.0)]:
    inst = []
    for i in range(n_inst):
      inst.append((fit_scenes.rand_rot(rng),
                   np.array([-60.0 + 150.0 * i + 40.0 * (n_inst == 1), 10.0 * i, tz])))
    xy, xyz, _, _ = fit_scenes.dense_scene(rng, inst)
    cell = (np.rint(xy[:, 1] / 4 - 0.5) * W + np.rint(xy[:, 0] / 4 - 0.5)).astype(np.int64)
    assert (np.diff(cell) >= 0).all()                  # raster order
    px = np.unique(cell, return_inverse=True)[1].astype(np.int64)   # index among masked pixels
    # few distinct confidences: ties everywhere
    conf = rng.choice(np.linspace(0.05, 0.95, 19), len(px)).astype(np.float32)
    out.append(((conf, px, xy, xyz), n_inst))
  return out


@pytest.fixture(scope='module')
def scenes():
  return _scenes()


def _fit_ordered(L, lib, scene_ids, scenes, K, prosac, max_k, seeds, yorder_only=False):
  from epos_amd import fitting
  d = 'cuda:0'
  slots = [scenes[i][0] for i in scene_ids]
  arrays, slot_base, cap = pool(slots)
  S = len(slots)
  dev = [torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in arrays]
  sb = torch.from_numpy(slot_base).to(d)
  sbo = torch.zeros(S + 1, dtype=torch.int64, device=d)
  c2 = torch.zeros(max(cap, 1), 2, dtype=torch.float64, device=d)
  c3 = torch.zeros(max(cap, 1), 3, dtype=torch.float64, device=d)
  src, yo, yp = (torch.zeros(max(cap, 1), dtype=torch.int32, device=d) for _ in range(3))
  work = torch.empty(lib.epos_corr_order_workspace_bytes(S, cap), dtype=torch.uint8, device=d)
  st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  L.check(lib.epos_corr_order_by_conf(
      _ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), _ptr(sb), S, cap, W,
      K or 0, int(prosac), _ptr(work), _ptr(sbo), _ptr(c2), _ptr(c3), _ptr(src), _ptr(yo),
      _ptr(yp), st), 'epos_corr_order_by_conf')
  fit = fitting.fit_params(use_prosac=prosac)
  wants = [scenes[i][1] for i in scene_ids]
  Ks = torch.from_numpy(np.tile(fit_scenes.K_YCBV.reshape(1, 9), (S, 1))).to(d)
  mm = torch.tensor(wants, dtype=torch.int32, device=d)
  sd = torch.tensor(seeds, dtype=torch.int64, device=d)
  fwork = torch.empty(lib.epos_fit_workspace_bytes(S, cap, ctypes.byref(fit), max_k),
                      dtype=torch.uint8, device=d)
  poses = torch.zeros(S, max_k, 12, dtype=torch.float64, device=d)
  scores = torch.zeros(S, max_k, dtype=torch.float64, device=d)
  nm = torch.zeros(S, dtype=torch.int32, device=d)
  labels = torch.full((max(cap, 1),), -5, dtype=torch.int32, device=d)
  rc = lib.epos_find6d_poses_device_ordered(
      _ptr(c2), _ptr(c3), _ptr(sbo), S, cap, _ptr(Ks), _ptr(mm), _ptr(sd), ctypes.byref(fit),
      max_k, _ptr(fwork), _ptr(poses), _ptr(scores), _ptr(nm), _ptr(labels), st, _ptr(yo),
      None if yorder_only else _ptr(yp))
  torch.cuda.synchronize()
  if yorder_only:
    return rc
  L.check(rc, 'epos_find6d_poses_device_ordered')
  return (poses.cpu().numpy(), scores.cpu().numpy(), nm.cpu().numpy(), labels.cpu().numpy(),
          sbo.cpu().numpy(), src.cpu().numpy())


def _fit_host(L, lib, scene, K, prosac, max_k, seed):
  """The host entry on the rows in confidence order (it builds yorder / ypos itself)."""
  from epos_amd import fitting
  (conf, px, xy, xyz), want = scene
  n = len(conf)
  apply = prosac or (K and n > K)
  perm = order_ref.confidence_order(conf) if apply else np.arange(n)
  perm = perm[:min(n, K) if K else n]
  a, b = np.ascontiguousarray(xy[perm]), np.ascontiguousarray(xyz[perm])
  fit = fitting.fit_params(use_prosac=prosac, max_model_number=want)
  poses = np.zeros((max_k, 12))
  scores = np.zeros(max_k)
  labels = np.full(len(perm), -5, np.int32)
  vp = ctypes.c_void_p
  Kd = np.ascontiguousarray(fit_scenes.K_YCBV.reshape(9))
  k = L.check(lib.epos_find6d_poses(
      a.ctypes.data_as(vp), b.ctypes.data_as(vp), len(perm), Kd.ctypes.data_as(vp),
      ctypes.byref(fit), seed, poses.ctypes.data_as(vp), labels.ctypes.data_as(vp),
      scores.ctypes.data_as(vp), max_k), 'epos_find6d_poses')
  return k, poses, scores, labels, perm


@pytest.mark.parametrize('prosac,K', [(1, None), (1, 900), (0, 900)])
@pytest.mark.parametrize('scene_ids', [(0,), (2,), (0, 1, 2)])
def test_ordered_device_entry_equals_host_entry(scenes, scene_ids, prosac, K):
  """epos_corr_order_by_conf + epos_find6d_poses_device_ordered, one slot and three slots per
  call, against epos_find6d_poses on the same confidence-ordered rows: poses, scores,
  num_models and labels (in original rows, through src_row) bit for bit."""
  L, lib = _lib()
  max_k = max(scenes[i][1] for i in scene_ids)
  seeds = [1000 + 17 * i for i in scene_ids]
  assert all(len(scenes[i][0][0]) > 900 for i in scene_ids)       # K truncates every slot
  poses, scores, nm, labels, sbo, src = _fit_ordered(L, lib, scene_ids, scenes, K, prosac,
                                                     max_k, seeds)
  found = 0
  for s, i in enumerate(scene_ids):
    k, hp, hs, hl, perm = _fit_host(L, lib, scenes[i], K, prosac, max_k, seeds[s])
    lo, hi = int(sbo[s]), int(sbo[s + 1])
    assert hi - lo == len(perm)
    assert np.array_equal(src[lo:hi], perm)
    assert nm[s] == k
    found += k
    assert poses[s, :k].tobytes() == hp[:k].tobytes()
    assert scores[s, :k].tobytes() == hs[:k].tobytes()
    n = len(scenes[i][0][0])
    by_row_dev, by_row_host = np.full(n, -9), np.full(n, -9)
    by_row_dev[src[lo:hi]] = labels[lo:hi]
    by_row_host[perm] = hl
    assert np.array_equal(by_row_dev, by_row_host)
  assert found >= len(scene_ids)


def test_ordered_entry_wants_both_permutations_or_neither(scenes):
  L, lib = _lib()
  rc = _fit_ordered(L, lib, (0,), scenes, None, 1, 1, [5], yorder_only=True)
  assert rc == -1                                                   # EPOS_E_INVALID
  assert b'both or neither' in lib.epos_last_error()
