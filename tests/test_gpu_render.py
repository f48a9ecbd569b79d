"""The mesh renderer's kernels (csrc/render.hip) against tests/helpers/render_ref.py, bit for
bit: keys, depth, face, local_pos, colour and every ground-truth field; the Renderer class; the
launchers' argument checks; the --vis_renderer command line."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import mesh_cases, render_ref as rr      # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(37, 29), (160, 120)]            # (w, h): odd and narrower than a wave; several rows
NAMES = ('depth', 'face', 'local_pos', 'color')


def _K(fx, fy, cx, cy):
  return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _rot(axis, angle):
  axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
  a, b, c = axis
  S = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]])
  return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


class Scene(object):
  """Models {obj_id: (verts, faces[, colors])} in a device Renderer, and the reference's
  images of (object, pose, K) instances, computed once per distinct instance."""

  def __init__(self, models):
    from epos_amd import render
    self.models = {}
    self.ren = render.Renderer('cuda:0')
    for o, m in sorted(models.items()):
      model = {'pts': m[0], 'faces': m[1]}
      if len(m) > 2:
        model['colors'] = m[2]
      self.models[o] = (np.asarray(m[0], np.float64), np.asarray(m[1], np.int32),
                        rr.vertex_colors(model))
      self.ren.add_model(o, model)
    self._ref = {}

  def ref(self, o, R, t, K, size):
    key = (o, np.asarray(R).tobytes(), np.asarray(t).tobytes(), np.asarray(K).tobytes(), size)
    if key not in self._ref:
      v, f, c = self.models[o]
      self._ref[key] = rr.render(v, f, c, R, t, K[0, 0], K[1, 1], K[0, 2], K[1, 2],
                                 size[1], size[0])
    return self._ref[key]

  def check(self, objs, Rs, ts, Ks, size):
    """Renders the instances in one call and compares every image with the reference's.
    Returns the reference outputs."""
    got = self.ren.render_instances(objs, np.stack(Rs), np.stack(ts), np.stack(Ks), size=size)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    refs = []
    for i, o in enumerate(objs):
      exp = self.ref(o, Rs[i], ts[i], Ks[i], size)
      assert got['keys'][i].view(np.uint64).tobytes() == exp['keys'].tobytes(), (i, o, 'keys')
      for name in NAMES:
        assert got[name][i].dtype == exp[name].dtype
        assert got[name][i].tobytes() == exp[name].tobytes(), (i, o, name)
      refs.append(exp)
    return refs


def _tri(*pts):
  return np.asarray(pts, np.float64), np.array([[0, 1, 2]], np.int32)


# single triangles, all seen with R = I, t = 0 through K(100, 100, cx, cy): u = 100 X / Z + cx
TRIANGLES = {
    1: _tri((-10, -8, 100), (12, -6, 110), (-2, 9, 95)),                 # inside the image
    2: _tri((-3e6, -3e6, 100), (3e6, -3e6, 100), (0, 4e6, 100)),         # far larger than it
    3: _tri((500, 500, 100), (520, 500, 100), (510, 520, 100)),          # off-screen
    4: _tri((-10, -8, 5), (12, -6, 6), (-2, 9, 7)),                      # behind near
    5: _tri((-10, -8, 100), (12, -6, 9.5), (-2, 9, 95)),                 # straddles near
    6: _tri((-10, -8, 100), (0, 0, 100), (10, 8, 100)),                  # zero area
    7: (np.array([(-10, -8, 100), (12, -6, 110), (-2, 9, 95)], np.float64),
        np.array([[0, 1, 2], [0, 1, 2]], np.int32)),                     # coplanar twins
    8: (np.array([(-10, -8, 100), (12, -6, 110), (-2, 9, 95)], np.float64),
        np.array([[2, 1, 0], [0, 1, 2]], np.int32)),                     # twins, other winding
}


@pytest.fixture(scope='module')
def triangles():
  return Scene(TRIANGLES)


@pytest.fixture(scope='module')
def meshes():
  sphere1 = mesh_cases.icosphere(1)
  sphere2 = mesh_cases.icosphere(2)
  rng = np.random.RandomState(4)
  colours = rng.randint(0, 256, (len(sphere2[0]), 3)).astype(np.float64)
  return Scene({1: sphere1, 2: sphere2 + (colours,), 3: mesh_cases.grid4097(),
                4: mesh_cases.with_slivers(*sphere1),
                5: mesh_cases.with_duplicate(*sphere2, which=131),   # a face the test pose shows
                6: mesh_cases.with_zero_area(*mesh_cases.soup(3))})


@pytest.mark.parametrize('size', SIZES)
def test_single_triangles(triangles, size):
  w, h = size
  K = _K(100.0, 100.0, w / 2.0 + 0.25, h / 2.0 - 0.125)
  objs = sorted(TRIANGLES)
  n = len(objs)
  refs = triangles.check(objs, [np.eye(3)] * n, [np.zeros(3)] * n, [K] * n, size)
  covered = {o: int((r['depth'] > 0).sum()) for o, r in zip(objs, refs)}
  assert 0 < covered[1] < w * h
  assert covered[2] == w * h                        # the whole image, by the cooperative path
  assert covered[3] == covered[4] == covered[5] == covered[6] == 0
  # its snapped coordinates need the wide (128-bit) edge functions
  tri = rr._setup(TRIANGLES[2][0], [0, 1, 2], np.eye(3), np.zeros(3), 100.0, 100.0,
                  K[0, 2], K[1, 2], h, w, rr.NEAR)
  assert tri is not None and tri.wide
  assert covered[7] == covered[8] == covered[1]
  # identical triangles give equal depth bits: the lowest face index wins everywhere
  assert set(np.unique(refs[objs.index(7)]['face'])) == {-1, 0}


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('obj', [1, 2, 3, 4, 5, 6])
def test_meshes(meshes, obj, size):
  w, h = size
  K = _K(1.9 * w, 1.9 * w, w / 2.0 - 0.3, h / 2.0 + 0.2)
  R = _rot([1, 2, 3], 0.7) if obj != 3 else _rot([1, 0.2, 0], 0.5)
  ref, = meshes.check([obj], [R], [np.array([3.0, -2.0, 400.0])], [K], size)
  assert (ref['depth'] > 0).sum() > (w * h) // 40
  if obj == 5:                                      # the duplicated face never wins
    assert (ref['face'] != len(meshes.models[5][1]) - 1).all() and (ref['face'] == 131).any()


def test_lane_and_wavefront_paths_meet_at_the_threshold(triangles):
  """Right triangles whose clipped boxes hold one sample fewer than the lane limit, exactly
  the limit (still the lane's), and more (the wavefront's), in one mesh; K makes u = X + cx."""
  from epos_amd import _lib
  limit = _lib.load().epos_render_lane_max_pixels()
  assert limit == 256
  boxes = [(15, 17), (16, 16), (16, 17), (64, 5), (3, 80)]        # 255, 256, 272, 320, 240
  verts, faces, x = [], [], 2.0
  for i, (bw, bh) in enumerate(boxes):
    verts += [(x, 3.0, 100.0), (x + bw, 3.0, 100.0), (x, 3.0 + bh, 100.0)]
    faces.append((3 * i, 3 * i + 1, 3 * i + 2))
    x += bw + 1
  verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int32)
  w, h = 160, 120
  counts = []
  for f in faces:
    t = rr._setup(verts, f, np.eye(3), np.zeros(3), 100.0, 100.0, 0.0, 0.0, h, w, rr.NEAR)
    counts.append((t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1))
  assert counts == [limit - 1, limit, limit + 16, 320, 240]
  scene = Scene({1: (verts, faces)})
  ref, = scene.check([1], [np.eye(3)], [np.zeros(3)], [_K(100.0, 100.0, 0.0, 0.0)], (w, h))
  assert set(np.unique(ref['face'])) == {-1, 0, 1, 2, 3, 4}


def _large_mesh():
  """icosphere(5), 20 480 faces, with four oversized triangles: at face indices 300 and 5 000
  (first pass of the face loop: workgroups 1 and 19, in the latter its third wavefront) and two at the end
  (indices 20 482 and 20 483: the second pass, which starts at face 16 384)."""
  verts, faces = mesh_cases.icosphere(5)
  n = len(verts)
  big = np.array([(-200, 150, -70), (200, 150, -70), (0, 5, 80),          # cuts into the sphere
                  (-200, -150, -60), (200, -150, -60), (0, -5, -50),      # in front, upper half
                  (-200, -200, 60), (200, -200, 60), (0, 250, 60),        # behind everything
                  (-30, -200, -45), (-5, 200, -45), (-60, 200, -45)],     # a band in front
                 np.float64)
  tri = np.arange(n, n + 12, dtype=np.int32).reshape(4, 3)
  faces = np.insert(faces, [300, 4999], tri[:2], axis=0)
  faces = np.concatenate([faces, tri[2:]]).astype(np.int32)
  assert len(faces) == 20484 and (faces[300] == tri[0]).all() and (faces[5000] == tri[1]).all()
  return np.concatenate([verts, big]), faces, (300, 5000, 20482, 20483)


def test_mesh_beyond_one_pass_of_the_face_loop():
  """More faces than one pass of the raster kernel's face loop covers (64 workgroups x 256
  lanes = 16 384), with wavefront-walked triangles in both passes and in wavefronts other than
  a workgroup's first."""
  verts, faces, large = _large_mesh()
  w, h = SIZES[0]
  scene = Scene({1: (verts, faces)})
  K = _K(1.9 * w, 1.9 * w, w / 2.0 - 0.3, h / 2.0 + 0.2)
  t = np.array([3.0, -2.0, 400.0])
  ref, = scene.check([1], [np.eye(3)], [t], [K], (w, h))
  limit = 256
  for f in large:
    tri = rr._setup(verts, faces[f], np.eye(3), t, K[0, 0], K[1, 1], K[0, 2], K[1, 2], h, w,
                    rr.NEAR)
    assert (tri.x1 - tri.x0 + 1) * (tri.y1 - tri.y0 + 1) > limit, f
    assert (ref['face'] == f).any(), f                # each of them is seen somewhere
  small = ref['face'][~np.isin(ref['face'], large + (-1,))]
  assert (small >= 16384).any() and (small < 16384).any()


def _mixed_instances(n):
  rng = np.random.RandomState(n)
  objs = [(1, 2, 4, 5)[i % 4] for i in range(n)]
  Rs = [_rot(rng.normal(size=3), rng.uniform(0, 3)) for _ in range(n)]
  ts = [np.array([rng.uniform(-40, 40), rng.uniform(-30, 30), rng.uniform(250, 500)])
        for _ in range(n)]
  Ks = [_K(rng.uniform(150, 260), rng.uniform(150, 260), rng.uniform(60, 100),
           rng.uniform(40, 80)) for _ in range(n)]
  if n > 1:
    ts[n // 2] = np.array([5000.0, 0.0, 300.0])     # out of sight: no pixel
  return objs, Rs, ts, Ks


@pytest.mark.parametrize('n', [1, 3, 17])
def test_instances_and_launch_order(meshes, n):
  objs, Rs, ts, Ks = _mixed_instances(n)
  refs = meshes.check(objs, Rs, ts, Ks, (160, 120))
  seen = [bool((r['depth'] > 0).any()) for r in refs]
  assert seen == [n == 1 or i != n // 2 for i in range(n)]
  # the same instances in another order: every image is the one of its instance
  order = np.random.RandomState(1).permutation(n)
  meshes.check([objs[i] for i in order], [Rs[i] for i in order], [ts[i] for i in order],
               [Ks[i] for i in order], (160, 120))


def test_renderer_class(meshes):
  from epos_amd import render
  from epos_amd._lib import EposError
  R, t = _rot([0, 1, 1], 1.1), np.array([4.0, 6.0, 350.0])
  ren = meshes.ren
  ren.init(160, 120)
  ren.render_object(2, R.flatten().tolist(), t.tolist(), 200.0, 210.0, 80.0, 60.0)
  exp = meshes.ref(2, R, t, _K(200.0, 210.0, 80.0, 60.0), (160, 120))
  assert ren.get_depth_image(2).tobytes() == exp['depth'].tobytes()
  assert ren.get_color_image(2).tobytes() == exp['color'].tobytes()
  assert ren.get_local_pos_image(2).tobytes() == exp['local_pos'].tobytes()
  assert ren.get_color_image(2).shape == (120, 160, 3) and (exp['color'] > 0).any()
  batched = ren.render_instances([2], R[None], t[None], _K(200.0, 210.0, 80.0, 60.0))
  assert batched['depth'][0].cpu().numpy().tobytes() == ren.get_depth_image(2).tobytes()
  # the workspace of a size is carved once: a call with fewer instances or other outputs, and
  # a call at another size in between, leave it where it is
  three = ren.render_instances([2, 1, 2], np.stack([R] * 3), np.stack([t] * 3), np.eye(3))
  where = three['depth'].data_ptr()
  ren.render_instances([1], R[None], t[None], np.eye(3), size=(41, 23), outputs=('color',))
  again = ren.render_instances([1], R[None], t[None], np.eye(3), outputs=('depth',))
  assert again['depth'].data_ptr() == where and set(again) == {'depth', 'keys'}
  assert set(ren._work[(23, 41)]) == {'color', 'keys'}    # a size no other test uses
  with pytest.raises(EposError, match='no faces'):
    render.Renderer('cuda:0').add_model(1, {'pts': np.zeros((4, 3))})
  with pytest.raises(EposError, match='not added'):
    ren.render_instances([99], R[None], t[None], np.eye(3))
  with pytest.raises(EposError, match='not been rendered'):
    ren.get_depth_image(1)


# ---------------------------------------------------------------- epos_gt_fields ---
@pytest.fixture(scope='module')
def field_inputs():
  """Three overlapping instances (objects 2, 1, 2) at 37x29, rendered by the reference."""
  verts, faces = mesh_cases.icosphere(1, 30.0)
  ts = [np.array([0.0, 0.0, 300.0]), np.array([14.0, 5.0, 340.0]), np.array([-9.0, 6.0, 280.0])]
  outs = [rr.render(verts, faces, None, _rot([1, 1, 0], 0.3 * i), t, 100.0, 100.0, 18.0, 14.0,
                    29, 37) for i, t in enumerate(ts)]
  depth = np.stack([o['depth'] for o in outs])
  local = np.stack([o['local_pos'] for o in outs])
  assert ((depth > 0).sum(axis=0) >= 2).any()
  masks = np.random.RandomState(0).rand(3, 29, 37) < 0.8
  return depth, local, masks, [2, 1, 2]


def _centres(F, seed=0):
  rng = np.random.RandomState(seed + F)
  c = rng.uniform(-30, 30, (2, F, 3))
  if F > 1:                                         # two equal centres on the side the camera
    c[:, F // 2] = c[:, 1] = [0.0, 0.0, -30.0]      # sees: the lower index wins
  return c, rng.uniform(4, 15, (2, F))


@pytest.mark.parametrize('with_masks', [True, False])
@pytest.mark.parametrize('F', [1, 64, 256])
def test_gt_fields(field_inputs, F, with_masks):
  from epos_amd import render
  depth, local, masks, obj_ids = field_inputs
  centers, sizes = _centres(F)
  m = masks if with_masks else None
  exp = rr.gt_fields(depth, local, m, obj_ids, centers, sizes)
  got = render.gt_fields_device(
      torch.from_numpy(depth).cuda(), torch.from_numpy(local).cuda(), obj_ids, centers, sizes,
      None if m is None else torch.from_numpy(m.astype(np.uint8)).cuda())
  torch.cuda.synchronize()
  for k, v in exp.items():
    g = got[k].cpu().numpy()
    assert g.dtype == v.dtype and g.tobytes() == v.tobytes(), k
  assert len(np.unique(exp['instance'])) == 4       # background and all three instances
  if F > 1:
    assert (exp['frag_label'] != F // 2).all() and (exp['frag_label'] == 1).any()
  if not with_masks:                                # nearest wins where instances overlap
    both = (depth[0] > 0) & (depth[2] > 0)
    assert (exp['instance'][both] == 2).all() and both.any()


def test_gt_fields_without_instances():
  from epos_amd import render
  centers, sizes = _centres(64)
  got = render.gt_fields_device(torch.zeros((0, 29, 37), device='cuda'),
                                torch.zeros((0, 29, 37, 3), device='cuda'), [], centers, sizes)
  torch.cuda.synchronize()
  assert (got['instance'].cpu().numpy() == -1).all()
  for k in ('obj_label', 'frag_label', 'frag_loc', 'frag_weight'):
    assert (got[k].cpu().numpy() == 0).all()


def test_host_helpers_over_the_kernels(meshes):
  """make_masks_exclusive, gt_label_map and FragmentFieldGenerator against the reference's
  maps of the same renderings."""
  from epos_amd import render
  objs, w, h = [2, 1, 2], 80, 60
  K = _K(150.0, 150.0, 40.0, 30.0)
  Rs = [np.eye(3), _rot([0, 1, 0], 0.4), _rot([1, 0, 0], 0.9)]
  ts = [np.array([0.0, 0.0, 400.0]), np.array([30.0, 5.0, 450.0]), np.array([-25.0, 10.0, 350.0])]
  refs = [meshes.ref(o, R, t, K, (w, h)) for o, R, t in zip(objs, Rs, ts)]
  depth = np.stack([r['depth'] for r in refs])
  local = np.stack([r['local_pos'] for r in refs])
  masks = np.random.RandomState(2).rand(3, h, w) < 0.7
  centers, sizes = _centres(64)
  frag_c = {1: centers[0], 2: centers[1]}
  frag_s = {1: sizes[0], 2: sizes[1]}
  exp = rr.gt_fields(depth, local, masks, objs, centers, sizes)
  excl = render.make_masks_exclusive(meshes.ren, K, objs, np.stack(Rs), np.stack(ts), masks)
  assert excl.dtype == bool
  assert np.array_equal(excl, exp['instance'][None] == np.arange(3).reshape(3, 1, 1))
  assert np.array_equal(
      render.gt_label_map(meshes.ren, K, objs, np.stack(Rs), np.stack(ts), (w, h), masks),
      exp['obj_label'])
  nomask = rr.gt_fields(depth, local, None, objs, centers, sizes)
  assert np.array_equal(
      render.gt_label_map(meshes.ren, K, objs, np.stack(Rs), np.stack(ts), (w, h)),
      nomask['obj_label'])
  gen = render.FragmentFieldGenerator(frag_c, frag_s, meshes.ren)
  ids, coords, weights = gen.construct_frag_fields(w, h, K, objs, np.stack(Rs), np.stack(ts),
                                                   masks)
  assert ids.shape == (h, w, 1) and coords.shape == (h, w, 1, 3) and weights.shape == (h, w, 1)
  assert ids[..., 0].tobytes() == exp['frag_label'].tobytes()
  assert coords[:, :, 0].tobytes() == exp['frag_loc'].tobytes()
  assert weights[..., 0].tobytes() == exp['frag_weight'].tobytes()


# ---------------------------------------------------------------- argument checks ---
def test_render_launchers_refuse_invalid_arguments():
  """Return codes only: every refusal happens before anything is launched."""
  from epos_amd import _lib
  lib = _lib.load()
  dev = 'cuda:0'
  verts = torch.zeros((3, 3), dtype=torch.float64, device=dev)
  faces = torch.zeros((1, 3), dtype=torch.int32, device=dev)
  cols = torch.zeros((3, 3), dtype=torch.uint8, device=dev)
  insts = torch.zeros((1, 144), dtype=torch.uint8, device=dev)
  keys = torch.zeros((1, 4, 4), dtype=torch.int64, device=dev)
  depth = torch.zeros((1, 4, 4), dtype=torch.float32, device=dev)
  local = torch.zeros((1, 4, 4, 3), dtype=torch.float32, device=dev)
  ids = torch.ones((1,), dtype=torch.int32, device=dev)
  cen = torch.zeros((1, 257, 3), dtype=torch.float64, device=dev)
  siz = torch.ones((1, 257), dtype=torch.float64, device=dev)
  color = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=dev)
  p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
  s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  E = -1                                            # EPOS_E_INVALID

  def raster(v=p(verts), f=p(faces), i=p(insts), n=1, h=4, w=4, near=10.0, k=p(keys), nv=3,
             nf=1):
    return lib.epos_render_raster(v, nv, f, nf, i, n, h, w, near, k, s)
  assert raster() == 0
  for kw in (dict(v=None), dict(f=None), dict(i=None), dict(k=None), dict(n=-1), dict(h=-1),
             dict(w=-1), dict(nv=-1), dict(nf=-1), dict(near=0.0), dict(near=-1.0),
             dict(near=float('nan')), dict(h=40000)):
    assert raster(**kw) == E, kw
  assert b'epos_render_raster' in lib.epos_last_error()
  assert raster(n=0, k=None, i=None) == 0           # nothing to do

  def resolve(k=p(keys), v=p(verts), f=p(faces), c=p(cols), i=p(insts), n=1, h=4, w=4,
              near=10.0, out=p(color)):
    return lib.epos_render_resolve(k, v, 3, f, 1, c, i, n, h, w, near, p(depth), None, None,
                                   out, s)
  assert resolve() == 0
  for kw in (dict(k=None), dict(v=None), dict(f=None), dict(i=None), dict(c=None), dict(n=-1),
             dict(h=-1), dict(w=-1), dict(near=0.0)):
    assert resolve(**kw) == E, kw
  assert resolve(c=None, out=None) == 0             # colours are needed for the colour image only

  def fields(d=p(depth), l=p(local), o=p(ids), c=p(cen), z=p(siz), n=1, h=4, w=4, O=1, F=64):
    return lib.epos_gt_fields(d, l, None, o, n, h, w, c, z, O, F, None, None, None, None,
                              None, s)
  assert fields() == 0
  for kw in (dict(d=None), dict(l=None), dict(o=None), dict(c=None), dict(z=None), dict(n=-1),
             dict(h=-1), dict(w=-1), dict(O=0), dict(F=0), dict(F=257)):
    assert fields(**kw) == E, kw
  assert fields(F=256) == 0
  torch.cuda.synchronize()


# ---------------------------------------------------------------- command line ---
def test_infer_cli_mesh_renderer(tmp_path, gpu_children):
  """--vis with --vis_renderer mesh: the grid gains the "gt obj labels" tile, the four
  ground-truth fragment images are written, and the poses are those of the splat run, whose
  grid is byte for byte the one of a run without the flag."""
  from PIL import Image
  from epos_amd import ply, synthetic, vis
  store = synthetic.ModelStore(3, 64, seed=0)          # the store infer.py --synthetic builds
  bop = tmp_path / 'bop'
  (bop / 'lm' / 'models_eval').mkdir(parents=True)
  for o in store.dp_model['obj_ids']:
    v, f = mesh_cases.icosphere(1, 1.0, scale=store.radii[o])
    ply.save_ply(ply.model_path(str(bop), 'lm', o, 'eval'), v, f)
  fdir = tmp_path / 'frames'
  fdir.mkdir()
  np.save(str(fdir / 'a.npy'), synthetic.image(0, 96, 128).astype(np.uint8))
  K = [[150.0, 0.0, 64.0], [0.0, 150.0, 48.0], [0.0, 0.0, 1.0]]
  gt = [{'obj_id': 1, 'R': np.eye(3).tolist(), 't': [0.0, 0.0, 500.0]},
        {'obj_id': 2, 'R': _rot([0, 1, 0], 0.5).tolist(), 't': [60.0, 20.0, 600.0]}]
  (fdir / 'frames.json').write_text(json.dumps(
      [{'path': 'a.npy', 'im_id': 1, 'scene_id': 1, 'K': K, 'targets': {'1': 1, '2': 1},
        'gt_poses': gt}]))
  runs = {'mesh': ['--vis_renderer', 'mesh', '--vis_gt_frag_fields', 'true'],
          'splat': ['--vis_renderer', 'splat'], 'default': []}
  csv, grid = {}, {}
  for name, extra in runs.items():
    d = tmp_path / name
    (d / 'toy').mkdir(parents=True)
    (d / 'toy' / 'params.yml').write_text('infer_crop_size: "128,96"\n')
    out = subprocess.run(
        ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'infer.py'),
         '--model=toy', '--synthetic', '1', '--frames', str(fdir), '--num_objs', '3',
         '--dataset', 'lm', '--vis', 'true'] + extra,
        env=dict(os.environ, TF_MODELS_PATH=str(d), BOP_PATH=str(bop)), capture_output=True,
        text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = (d / 'toy' / 'infer' / 'estimated-poses.csv').read_text().strip().split('\n')
    csv[name] = '\n'.join(','.join(r.split(',')[:-1]) for r in rows)   # last column: time
    grid[name] = (d / 'toy' / 'vis' / '000000_grid.jpg').read_bytes()
  assert csv['mesh'] == csv['splat'] == csv['default']
  assert grid['splat'] == grid['default']
  vdir = tmp_path / 'mesh' / 'toy' / 'vis'
  for key in ('labels', 'coords', 'reconst', 'weights'):
    im = Image.open(str(vdir / ('000000_gt_frag_%s.png' % key)))
    assert im.size == (32, 24)                      # the output resolution, stride 4
  assert np.asarray(Image.open(str(vdir / '000000_gt_frag_weights.png'))).max() == 255
  # input, gt poses, pred poses, gt obj labels, predicted obj labels: 2 x 3 tiles, not 2 x 2
  tw, th = vis.TILE_SIZE
  assert Image.open(str(vdir / '000000_grid.jpg')).size == (3 * tw, 2 * th)
  assert Image.open(str(tmp_path / 'splat' / 'toy' / 'vis' / '000000_grid.jpg')).size == (
      2 * tw, 2 * th)
  assert not list((tmp_path / 'splat' / 'toy' / 'vis').glob('*_gt_frag_*'))
