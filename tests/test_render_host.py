"""The numpy restatement of the mesh renderer (tests/helpers/render_ref.py) against facts that
do not depend on it -- watertight coverage, the analytic depth of a sphere, a k-d tree, a
line-by-line mask loop -- and the host-side pieces around the kernels: instance masks from
TFRecords, the command-line wiring, the declared symbols."""
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import mesh_cases, render_ref as rr      # noqa: E402

H, W = 120, 160
FX = FY = 300.0
CX, CY = 80.0, 60.0


def _rot(axis, angle):
  axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
  a, b, c = axis
  K = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]])
  return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _pose_with_vertex_on_pixel_centre(verts):
  """Identity rotation; the translation puts vertex 0 at depth 512 and its projection exactly
  on the sample point of pixel (90, 50): every quantity is a small dyadic number, so the
  snapped coordinate is exactly 256 * 90 + 128."""
  z = 512.0
  fx = fy = 256.0
  want = np.array([(90.5 - CX) * z / fx, (50.5 - CY) * z / fy, z])
  return np.eye(3), want - verts[0], fx, fy


POSES = [(_rot([1, 2, 3], 0.7), np.array([3.0, -2.0, 400.0])),
         (_rot([0, 1, 0], 2.1), np.array([-25.0, 14.0, 300.0]))]


@pytest.mark.parametrize('subdiv', [1, 3])
def test_closed_convex_mesh_is_covered_exactly_twice(subdiv):
  """A closed convex mesh: every ray through a sample point enters once and leaves once, so
  over both windings a pixel is covered by exactly 0 or 2 triangles -- 1 would be a crack or
  a lost edge pixel, 3+ a double hit on a shared edge or vertex."""
  verts, faces = mesh_cases.icosphere(subdiv)
  # dyadic vertices make the third pose's vertex land exactly on a pixel centre
  verts = np.round(verts * 64.0) / 64.0
  R3, t3, fx3, fy3 = _pose_with_vertex_on_pixel_centre(verts)
  for R, t, fx, fy in [(POSES[0][0], POSES[0][1], FX, FY), (POSES[1][0], POSES[1][1], FX, FY),
                       (R3, t3, fx3, fy3)]:
    keys, cover = rr.raster(verts, faces, R, t, fx, fy, CX, CY, H, W, count=True)
    assert set(np.unique(cover)) == {0, 2}
    assert np.array_equal(cover == 2, keys != rr.BACKGROUND)
    assert (cover == 2).sum() > 500
  # the third pose: vertex 0 snaps onto the sample point of pixel (90, 50), which is covered
  tri = rr._setup(verts, [0, 0, 0], R3, t3, fx3, fy3, CX, CY, H, W, rr.NEAR)
  assert (tri.x[0], tri.y[0]) == (256 * 90 + 128, 256 * 50 + 128)
  assert cover[50, 90] == 2


def test_icosphere_depth_against_the_analytic_sphere():
  """Depth of an icosphere of radius r (vertices on the sphere) against the ray-sphere depth.

  The polyhedron is inscribed, so along a pixel's ray the mesh is met no earlier than the
  sphere, and every mesh-covered pixel is sphere-covered. How much later: a face is a chord
  plane of a cap whose half-angle is at most theta, the angular circumradius of the largest
  face, so the whole mesh lies outside the concentric sphere of radius r - s, with the sagitta
  s = r (1 - cos(theta)). A ray that enters the sphere at incidence cosine c reaches radius
  r - s after the path length
      L = r c - sqrt(r^2 c^2 - 2 r s + s^2) = s / c + s^2 (1 - c^2) / (2 r c^3) + O(s^3),
  and has met the mesh by then. (Inside the sphere the radial descent per unit length,
  -(p . d) / |p|, starts at c and shrinks, which is why L exceeds s / c.) The camera z moves by
  L times the z component of the unit ray direction, which is below 1. Hence, to first order
  in s / r,
      0 <= z_mesh - z_sphere <= s / c;
  the exact bound is L d_z. The second-order term is at most s^2 0.75 / (2 r 0.125) = 0.0025
  here (s = 0.18, r = 40, c = 0.5), 0.7 % of s / c, and d_z >= 0.994 over this silhouette takes
  up to 0.6 % off: the exact bound is within a percent of s / c either way. The assertion is the
  first-order bound as it stands, without that margin; only the fp32 rounding of the depth
  (2^-24 relative: 3e-5 at z = 400, eps = 1e-4) is added at both ends.
  Pixels with c < 0.5 are left out; orthographically those are the outer annulus of area
  1 - 0.75 = 25 % of the silhouette. At distance 400 with r = 40 the perspective silhouette
  is slightly smaller than the disc of radius r, and the share stays under the 30 % cap."""
  r, dist = 40.0, 400.0
  verts, faces = mesh_cases.icosphere(3, r)
  t = np.array([3.0, -2.0, dist])
  out = rr.render(verts, faces, None, np.eye(3), t, FX, FY, CX, CY, H, W)
  ys, xs = np.mgrid[0:H, 0:W]
  d = np.stack([(xs + 0.5 - CX) / FX, (ys + 0.5 - CY) / FY, np.ones((H, W))], axis=-1)
  dn = d / np.linalg.norm(d, axis=-1, keepdims=True)
  b = dn @ t
  disc = b * b - (t @ t - r * r)
  sphere = disc > 0
  lam = b - np.sqrt(np.where(sphere, disc, 0.0))
  hit = lam[..., None] * dn
  z_sphere = hit[..., 2]
  cos_inc = -np.einsum('ijk,ijk->ij', (hit - t) / r, dn)
  mesh = out['depth'] > 0
  assert not (mesh & ~sphere).any()                   # inscribed: a subset
  tri = verts[faces]
  centre = tri.mean(axis=1)
  centre /= np.linalg.norm(centre, axis=1, keepdims=True)
  cos_theta = min(float(np.min(np.einsum('fk,fvk->fv', centre, tri / r))), 1.0)
  s = r * (1.0 - cos_theta)
  use = mesh & (cos_inc >= 0.5)
  left_out = 1.0 - use.sum() / float(sphere.sum())
  print('sagitta %.4f, pixels %d, left out %.3f' % (s, use.sum(), left_out))
  assert left_out <= 0.30
  diff = out['depth'].astype(np.float64)[use] - z_sphere[use]
  eps = 1e-4
  print('z_mesh - z_sphere: min %.6f max %.6f' % (diff.min(), diff.max()))
  assert (diff >= -eps).all()
  assert (diff <= s / cos_inc[use] + eps).all()


def test_nearest_fragment_against_a_kd_tree():
  spatial = pytest.importorskip('scipy.spatial')
  rng = np.random.RandomState(3)
  centers = rng.uniform(-50, 50, (64, 3))
  sizes = rng.uniform(5, 20, 64)
  xyz = rng.uniform(-60, 60, (2000, 3)).astype(np.float32)
  lab, loc = rr.nearest_fragment(xyz, centers, sizes)
  _, ids = spatial.cKDTree(centers).query(xyz.astype(np.float64), k=1)
  assert np.array_equal(lab, ids.astype(np.int32))
  back = centers[lab] + loc.astype(np.float64) * sizes[lab][:, None]
  # loc is one fp32 rounding of (xyz - centre) / size: |error| <= 2^-24 |loc| size per axis
  tol = 2.0 ** -23 * (np.abs(loc) * sizes[lab][:, None]) + 1e-12
  assert (np.abs(back - xyz.astype(np.float64)) <= tol).all()


def _exclusive_by_the_reference_loop(masks, depths):
  """The loop of datagen_utils.make_masks_exclusive_py, statement by statement, over given
  per-instance depth images (what its renderer calls return)."""
  num_gts, height, width = masks.shape
  masks = masks.copy()
  avail = np.ones([height, width], bool)
  for gt_id in range(num_gts)[::-1]:
    depth = depths[gt_id].astype(np.float32)
    obj_mask = np.logical_and(np.logical_and(masks[gt_id], avail), depth > 0)
    avail = np.logical_and(np.logical_not(obj_mask), avail)
    masks[gt_id] = obj_mask
  return masks


def test_masks_exclusive_against_the_reference_loop():
  verts, faces = mesh_cases.icosphere(1, 30.0)
  obj_ids = [2, 1, 2]
  ts = [np.array([0.0, 0.0, 300.0]), np.array([20.0, 5.0, 340.0]), np.array([-15.0, 10.0, 280.0])]
  h, w = 60, 80
  outs = [rr.render(verts, faces, None, np.eye(3), t, 150.0, 150.0, 40.0, 30.0, h, w) for t in ts]
  depth = np.stack([o['depth'] for o in outs])
  local = np.stack([o['local_pos'] for o in outs])
  rng = np.random.RandomState(0)
  masks = rng.rand(3, h, w) < 0.8                   # loose masks: not every rendered pixel
  exp = _exclusive_by_the_reference_loop(masks, depth)
  got = rr.gt_fields(depth, local, masks, obj_ids, np.zeros((2, 1, 3)), np.ones((2, 1)))
  mine = got['instance'][None] == np.arange(3).reshape(3, 1, 1)
  assert np.array_equal(mine, exp)
  assert (exp.sum(axis=0) <= 1).all() and (exp.sum(axis=0) == 1).any()
  assert (depth[0] > 0)[exp[2]].any()               # instances do overlap
  # the label map in the reduce_sum form of datagen.py:590-604
  label = np.sum(exp.astype(np.int32) * np.asarray(obj_ids).reshape(3, 1, 1), axis=0)
  assert np.array_equal(got['obj_label'], label)


def _png(arr):
  from PIL import Image
  buf = io.BytesIO()
  Image.fromarray(arr).save(buf, format='PNG')
  return buf.getvalue()


def test_decode_instance_masks(tmp_path):
  from epos_amd import frames, tfrecord
  rng = np.random.RandomState(5)
  h0, w0 = 96, 128
  masks = (rng.rand(3, h0, w0) < 0.5)
  feats = {'image/encoded': [_png(np.zeros((h0, w0, 3), np.uint8))],
           'image/height': [h0], 'image/width': [w0], 'image/scene_id': [1], 'image/im_id': [2],
           'image/camera/fx': [200.0], 'image/camera/fy': [200.0],
           'image/camera/cx': [64.0], 'image/camera/cy': [48.0],
           'image/object/id': [1, 7, 2], 'image/object/visibility': [1.0, 1.0, 1.0],
           'image/object/mask': [_png(m.astype(np.uint8) * 255) for m in masks]}
  path = str(tmp_path / 'm.tfrecord')
  tfrecord.write_records(path, [tfrecord.encode_example(feats)])
  back = tfrecord.parse_example(next(tfrecord.read_records(path)))
  # identity: no resize, full crop, output = input size
  geo = (h0, w0, h0, w0, h0, w0)
  same = tfrecord.decode_instance_masks(back, geo, (0, 0), (w0, h0))
  assert same.dtype == bool and np.array_equal(same, masks)
  # shrink 96 -> 48 rows, crop 40x56 at (3, 5), output stride 4; instances 0 and 2 kept
  geo = (h0, w0, 48, 64, 40, 56)
  got = tfrecord.decode_instance_masks(back, geo, (3, 5), (14, 10), keep=[0, 2])
  assert got.shape == (2, 10, 14)

  def idx(n_in, n_out):
    return [int(np.floor(np.float32(d) * (np.float32(n_in - 1) / np.float32(n_out - 1)) +
                         np.float32(0.5))) for d in range(n_out)]
  r1, c1 = idx(h0, 48), idx(w0, 64)
  r2, c2 = idx(40, 10), idx(56, 14)
  assert r1[-1] == h0 - 1 and c1[-1] == w0 - 1      # align_corners: last maps to last
  assert r2[-1] == 39 and c2[-1] == 55
  for j, i in enumerate([0, 2]):
    for y in (0, 4, 9):
      for x in (0, 6, 13):
        assert got[j, y, x] == masks[i, r1[3 + r2[y]], c1[5 + c2[x]]]
  # the frame scanner fills the lazy masks only when the record has the feature
  fr = frames.scan_tfrecords([path], (w0, h0), h0, [1, 2])
  assert len(fr) == 1 and len(fr[0].gt_poses or [1, 2]) == 2
  lazy = fr[0].gt_masks((w0, h0))
  assert np.array_equal(lazy, masks[[0, 2]])
  del feats['image/object/mask']
  tfrecord.write_records(path, [tfrecord.encode_example(feats)])
  assert frames.scan_tfrecords([path], (w0, h0), h0, [1, 2])[0].gt_masks((w0, h0)) is None
  plain = frames.Frame(0, 1, np.eye(3), {}, None)
  assert plain.gt_masks((4, 4)) is None


def test_mesh_renderer_flag_needs_a_dataset(tmp_path, monkeypatch):
  import infer
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  with pytest.raises(ValueError, match='--vis_renderer mesh needs --dataset'):
    infer.main(['--model', 'm', '--synthetic', '1', '--vis', 'true', '--vis_renderer', 'mesh'])
  monkeypatch.delenv('BOP_PATH')
  with pytest.raises(ValueError, match='--vis_renderer mesh needs --dataset'):
    infer.main(['--model', 'm', '--synthetic', '1', '--vis', 'true', '--vis_renderer', 'mesh',
                '--dataset', 'lm'])


def test_splat_still_refuses_gt_frag_fields(tmp_path, monkeypatch):
  import infer
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  assert infer.build_parser().parse_args(['--model', 'm']).vis_renderer == 'splat'
  for extra in ([], ['--vis_renderer', 'splat']):
    with pytest.raises(NotImplementedError):
      infer.main(['--model', 'm', '--synthetic', '1', '--vis', 'true',
                  '--vis_gt_frag_fields', 'true'] + extra)


def test_render_symbols_are_declared_and_bound():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  lib = _lib.load()
  for name in ('epos_render_lane_max_pixels', 'epos_render_raster', 'epos_render_resolve',
               'epos_gt_fields'):
    assert name in _lib.SYMBOLS and name + '(' in header
    assert getattr(lib, name).argtypes is not None or name.endswith('max_pixels')
  assert lib.epos_render_lane_max_pixels() >= 64
  assert lib.epos_abi_version() == 7


def test_vis_takes_a_renderer_and_gt_fields(tmp_path):
  """visualize(renderer=, gt_fields=): the pose tiles come from the renderer's colour images
  (saturating add, 0.3 / 0.7 blend), the label tile and the four fragment images from the
  maps; without them the call is the old one."""
  from PIL import Image
  from epos_amd import synthetic, vis

  class FakeRenderer(object):
    def has_object(self, o):
      return o == 1

    def render_instances(self, obj_ids, Rs, ts, K, size=None, outputs=()):
      import torch
      w, h = size
      col = np.zeros((len(obj_ids), h, w, 3), np.uint8)
      col[:, :h // 2] = 200
      return {'color': torch.from_numpy(col)}

  store = synthetic.ModelStore(2, 8, seed=0)
  h, w = 48, 64
  rgb = np.full((h, w, 3), 100.0, np.float32)
  poses = [{'obj_id': 1, 'R': np.eye(3), 't': np.array([0, 0, 500.0])}] * 2 + [
      {'obj_id': 2, 'R': np.eye(3), 't': np.array([0, 0, 500.0])}]
  over = vis.overlay_object_poses(rgb, np.eye(3), poses, store, renderer=FakeRenderer())
  assert (over[:h // 2] == int(0.3 * 100 + 0.7 * 255)).all()      # 200 + 200 saturates
  assert (over[h // 2:] == 30).all()
  oh, ow = 12, 16
  pred = {'pred_obj_label': np.zeros((oh, ow), np.int64)}
  obj = np.zeros((oh, ow), np.int32)
  obj[2:8, 3:9] = 1
  rng = np.random.RandomState(0)
  fields = {'obj_label': obj, 'frag_label': rng.randint(0, 8, (oh, ow)).astype(np.int32) * (obj > 0),
            'frag_loc': rng.uniform(-1, 1, (oh, ow, 3)).astype(np.float32) * (obj > 0)[..., None],
            'frag_weight': (obj > 0).astype(np.float32)}
  flags = {'vis_gt_frag_fields': True}
  a = vis.visualize(rgb, np.eye(3), pred, [], 3, store, str(tmp_path / 'a'), gt_poses=poses,
                    flags=flags, renderer=FakeRenderer(), gt_fields=fields)
  names = sorted(os.path.basename(p) for p in a)
  assert names == ['000003_grid.jpg', '000003_gt_frag_coords.png', '000003_gt_frag_labels.png',
                   '000003_gt_frag_reconst.png', '000003_gt_frag_weights.png']
  wts = np.asarray(Image.open(str(tmp_path / 'a' / '000003_gt_frag_weights.png')))
  assert np.array_equal(wts > 0, obj > 0)
  b = vis.visualize(rgb, np.eye(3), pred, [], 3, store, str(tmp_path / 'b'), gt_poses=poses)
  ga, gb = Image.open(a[-1]).size, Image.open(b[-1]).size
  # input, gt poses, pred poses, [gt obj labels], predicted obj labels: 5 tiles vs 4
  assert ga == (3 * vis.TILE_SIZE[0], 2 * vis.TILE_SIZE[1])
  assert gb == (2 * vis.TILE_SIZE[0], 2 * vis.TILE_SIZE[1])
