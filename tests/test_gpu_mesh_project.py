"""epos_project_rows_to_mesh_f64 (csrc/mesh_project.hip) through the C ABI: the indexed
closest-point query against the exhaustive sweep kernel and the numpy oracle, bit for bit;
the pooled launch (slots, empty slots, capacity); the tie rule; the pruning."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import mesh_cases, mesh_query_ref      # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Table(object):
  """A device mesh table over {obj_id: (verts, faces)}."""

  def __init__(self, meshes, num_objs):
    from epos_amd import _lib, mesh_index
    self.lib = _lib.load()
    self.meshes = meshes
    self.table = mesh_index.MeshTable(
        {o: {'pts': v, 'faces': f} for o, (v, f) in meshes.items()}, num_objs, 'cuda:0')

  def run(self, rows, counts, objs, capacity=None, S=None):
    """rows f64[N,3] (the buffer, N may exceed capacity); slot s holds counts[s] rows of object
    objs[s]. Returns (rows after the call, face_idx, visited)."""
    from epos_amd import _lib
    n = len(rows)
    capacity = n if capacity is None else capacity
    S = len(counts) if S is None else S
    buf = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).cuda()
    base = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).cuda()
    slots = torch.tensor([[0, o] for o in objs] or [[0, 0]], dtype=torch.int32).cuda()
    face = torch.full((max(n, 1),), -7, dtype=torch.int32).cuda()
    vis = torch.full((max(n, 1),), -7, dtype=torch.int32).cuda()
    t = self.table
    _lib.check(self.lib.epos_project_rows_to_mesh_f64(
        _ptr(buf), _ptr(base), _ptr(slots), S, capacity, _ptr(t.recs_dev), t.num_objs,
        _ptr(t.geom_dev), _ptr(t.fid_dev), _ptr(face), _ptr(vis),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'project_rows')
    torch.cuda.synchronize()
    return buf.cpu().numpy(), face.cpu().numpy()[:n], vis.cpu().numpy()[:n]


def sweep(pts, mesh):
  from epos_amd import corresp
  return corresp.project_pts_to_model(pts, mesh[0], mesh[1], return_faces=True)


def points(mesh, n, seed=5, centre=False):
  """The special queries of the host tests plus random ones, n in all."""
  pts = mesh_cases.queries(mesh[0], mesh[1], n_random=40, centre=centre)
  rng = np.random.RandomState(seed)
  lo, hi = mesh[0].min(axis=0), mesh[0].max(axis=0)
  more = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), (n - len(pts), 3))
  return np.concatenate([pts, more])


@pytest.fixture(scope='module')
def world():
  sphere = mesh_cases.icosphere(3)
  meshes = {1: mesh_cases.soup(), 2: sphere, 3: mesh_cases.with_duplicate(*sphere),
            5: mesh_cases.grid4097(), 6: mesh_cases.with_zero_area(*mesh_cases.soup(3)),
            7: mesh_cases.with_slivers(*mesh_cases.icosphere(1))}
  return Table(meshes, 7)                    # object 4 has no mesh


@pytest.mark.parametrize('obj', [1, 2, 6, 7])
def test_entry_equals_the_sweep_kernel(world, obj):
  mesh = world.meshes[obj]
  pts = points(mesh, 300)
  exp, exp_f = sweep(pts, mesh)
  got, got_f, vis = world.run(pts, [300], [obj])
  assert got.tobytes() == exp.tobytes()
  assert np.array_equal(got_f, exp_f)
  ix = world.table.index[obj]
  assert (vis >= 1).all() and (vis <= ix['nleaf'] + ix['nalways']).all()


def test_entry_equals_the_oracle(world):
  from oracle import project_ref
  mesh = world.meshes[1]
  pts = mesh_cases.queries(mesh[0], mesh[1], n_random=35)
  assert len(pts) == 60
  exp, exp_f = project_ref.project_pts_to_model(pts, mesh[0], mesh[1])
  got, got_f, _ = world.run(pts, [60], [1])
  assert got.tobytes() == exp.tobytes()
  assert np.array_equal(got_f, exp_f)


@pytest.mark.parametrize('counts,objs', [((1, 64, 65), (2, 1, 2)), ((65, 0, 1), (1, 2, 2)),
                                         ((0, 64, 0, 1), (1, 2, 1, 1))])
def test_pooled_launch(world, counts, objs):
  rng = np.random.RandomState(11)
  rows = rng.uniform(-60, 60, (sum(counts), 3))
  got, got_f, _ = world.run(rows, counts, objs)
  lo = 0
  for n, obj in zip(counts, objs):
    if n:
      exp, exp_f = sweep(rows[lo:lo + n], world.meshes[obj])
      assert got[lo:lo + n].tobytes() == exp.tobytes()
      assert np.array_equal(got_f[lo:lo + n], exp_f)
    lo += n


def test_no_slots_and_no_capacity(world):
  rows = np.full((8, 3), SENTINEL)
  for kw in (dict(S=0), dict(capacity=0)):
    got, got_f, vis = world.run(rows, [8], [1], **kw)
    assert (got == SENTINEL).all() and (got_f == -7).all() and (vis == -7).all()


def test_rows_beyond_capacity_stay(world):
  """slot_base says 40 + 60 rows, the buffers hold capacity = 70: rows 0..69 are projected (the
  second slot's first 30 among them), rows 70.. of the allocation are not touched."""
  rng = np.random.RandomState(12)
  rows = np.concatenate([rng.uniform(-60, 60, (70, 3)), np.full((30, 3), SENTINEL)])
  got, got_f, vis = world.run(rows, [40, 60], [2, 1], capacity=70)
  assert (got[70:] == SENTINEL).all() and (got_f[70:] == -7).all() and (vis[70:] == -7).all()
  for lo, hi, obj in ((0, 40, 2), (40, 70, 1)):
    exp, exp_f = sweep(rows[lo:hi], world.meshes[obj])
    assert got[lo:hi].tobytes() == exp.tobytes()
    assert np.array_equal(got_f[lo:hi], exp_f)


def test_object_without_mesh_leaves_rows(world):
  """The kernel's guard behind the Python layer's refusal (MeshProjector.check_slots)."""
  rows = np.full((5, 3), SENTINEL)
  got, _, _ = world.run(rows, [5], [4])
  assert (got == SENTINEL).all()


def test_tie_rule(world):
  """Equidistant faces: the duplicated face (queries on and above it) and the sphere's centre
  resolve to the face the sweep reports, the lowest index."""
  mesh = world.meshes[3]
  dup = mesh[0][mesh[1][-1]]
  pts = np.concatenate([dup, dup.mean(axis=0)[None] * np.array([[1.0], [1.05], [0.9]]),
                        np.zeros((1, 3))])
  exp, exp_f = sweep(pts, mesh)
  got, got_f, _ = world.run(pts, [len(pts)], [3])
  assert np.array_equal(got_f, exp_f) and got.tobytes() == exp.tobytes()
  assert (got_f != len(mesh[1]) - 1).all() and (got_f == 100).any()
  c_exp, c_f = sweep(np.zeros((1, 3)), world.meshes[2])
  c_got, c_gf, _ = world.run(np.zeros((1, 3)), [1], [2])
  assert c_gf[0] == c_f[0] and c_got.tobytes() == c_exp.tobytes()


@pytest.mark.parametrize('obj', [2, 5])
def test_pruning(world, obj):
  """Near-surface queries sweep at most a quarter of the leaves on average, and exactly the
  blocks the numpy model of the traversal sweeps (the order is deterministic: ascending
  bound, ties by child number, every bound computed with the same float64 operations)."""
  mesh = world.meshes[obj]
  ix = world.table.index[obj]
  pts = mesh_cases.near_surface(mesh[0], mesh[1], n=100)
  exp, exp_f, exp_vis = mesh_query_ref.project(ix, pts)
  got, got_f, vis = world.run(pts, [len(pts)], [obj])
  assert got.tobytes() == exp.tobytes() and np.array_equal(got_f, exp_f)
  assert ix['nalways'] == 0
  assert vis.mean() <= ix['nleaf'] / 4.0, (vis.mean(), ix['nleaf'])
  assert np.array_equal(vis, exp_vis)
