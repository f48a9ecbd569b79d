"""The mesh index of the fused project_to_surface stage, on the host: builder invariants, the
numpy model of the indexed query (tests/helpers/mesh_query_ref.py) against the exhaustive
sweep oracle (oracle/project_ref.py) bit for bit, the pruning the index must deliver, and the
command-line routing."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from epos_amd import mesh_index                        # noqa: E402
from oracle import project_ref                         # noqa: E402
from tests.helpers import mesh_cases, mesh_query_ref   # noqa: E402

LEAF = mesh_index.LEAF


def _meshes():
  sphere = mesh_cases.icosphere(3)
  return {
      'soup': mesh_cases.soup(),
      'sphere': sphere,
      'duplicate': mesh_cases.with_duplicate(*sphere),
      'zero_area': mesh_cases.with_zero_area(*mesh_cases.soup(3)),
      'slivers': mesh_cases.with_slivers(*mesh_cases.icosphere(1)),
      'grid4097': mesh_cases.grid4097(),
  }


MESHES = _meshes()


@pytest.fixture(scope='module')
def indices():
  return {k: mesh_index.build(*m) for k, m in MESHES.items()}


@pytest.mark.parametrize('name', sorted(MESHES))
def test_builder_invariants(indices, name):
  verts, faces = MESHES[name]
  ix = indices[name]
  nf = len(faces)
  assert ix['nf'] == nf
  # every face in exactly one leaf or on the always-swept list
  tree_ids = ix['fid'][:ix['nleaf'] * LEAF]
  always_ids = ix['fid'][ix['nleaf'] * LEAF:]
  assert len(always_ids) == ix['nalways'] * LEAF
  placed = np.concatenate([tree_ids[tree_ids >= 0], always_ids[always_ids >= 0]])
  assert np.array_equal(np.sort(placed), np.arange(nf))
  assert np.array_equal(tree_ids[tree_ids >= 0], ix['order'])
  assert np.array_equal(always_ids[always_ids >= 0], ix['always'])
  # the triangle blocks hold the faces' own vertices, untouched
  tri = ix['tri'].reshape(-1, 9, LEAF)
  for blk, lane in ((0, 0), (len(tri) - 1, 0)):
    f = ix['fid'][blk * LEAF + lane]
    assert tri[blk, :, lane].tobytes() == verts[faces[f]].reshape(9).tobytes()
  # level 0 boxes contain the vertices of their leaf's faces; every upper box its children
  lo = [ix['leaf_lo']]; hi = [ix['leaf_hi']]
  for leaf in range(ix['nleaf']):
    ids = tree_ids[leaf * LEAF:(leaf + 1) * LEAF]
    v = verts[faces[ids[ids >= 0]]].reshape(-1, 3)
    assert (v >= lo[0][leaf]).all() and (v <= hi[0][leaf]).all()
  assert ix['count'][0] == ix['nleaf']
  for level in range(ix['top'] + 1 if ix['nleaf'] else 0):
    n = ix['count'][level]
    g = ix['boxes'][level].reshape(-1, 6, LEAF)
    assert len(g) == (n + LEAF - 1) // LEAF
    blo = g[:, 0:3, :].transpose(0, 2, 1).reshape(-1, 3)[:n]
    bhi = g[:, 3:6, :].transpose(0, 2, 1).reshape(-1, 3)[:n]
    if level == 0:
      assert blo.tobytes() == lo[0].tobytes() and bhi.tobytes() == hi[0].tobytes()
    else:
      for i in range(n):
        kids = slice(i * LEAF, (i + 1) * LEAF)
        assert (lo[level - 1][kids] >= blo[i]).all() and (hi[level - 1][kids] <= bhi[i]).all()
    lo.append(blo); hi.append(bhi)
  if ix['nleaf']:
    assert ix['count'][ix['top']] <= LEAF
    assert all(c == 0 for c in ix['count'][ix['top'] + 1:])
  # deterministic
  again = mesh_index.build(verts, faces)
  for key in ('tri', 'fid', 'order', 'always', 'near_lo', 'near_hi'):
    assert again[key].tobytes() == ix[key].tobytes(), key
  assert all(a.tobytes() == b.tobytes() for a, b in zip(again['boxes'], ix['boxes']))


def test_index_shapes(indices):
  """The structural conditions the query tests rely on."""
  assert indices['sphere']['nleaf'] == 20 and indices['sphere']['top'] == 0
  assert indices['grid4097']['nleaf'] == 65 and indices['grid4097']['top'] == 1     # 3rd level
  assert indices['sphere']['nalways'] == 0 and len(indices['sphere']['always']) == 0
  assert indices['grid4097']['nalways'] == 0 and len(indices['grid4097']['always']) == 0
  # the degenerate faces and the slivers are where the argument sends them
  nf = indices['zero_area']['nf']
  assert set(range(nf - 3, nf)) <= set(indices['zero_area']['always'].tolist())
  nf = indices['slivers']['nf']
  assert {nf - 2, nf - 1} <= set(indices['slivers']['always'].tolist())       # 1e-8, 1e-12


def test_table_offsets():
  models = {2: dict(zip(('pts', 'faces'), MESHES['soup'])),
            4: dict(zip(('pts', 'faces'), MESHES['grid4097'])),
            9: dict(zip(('pts', 'faces'), MESHES['soup']))}       # beyond num_objs: ignored
  table = mesh_index.MeshTable(models, 5)
  assert table.obj_ids == [2, 4]
  assert not table.has_mesh(1) and table.has_mesh(4) and not table.has_mesh(9)
  assert ctypes.sizeof(table.recs) == 5 * 128
  goff = foff = 0
  for obj in (1, 2, 3, 4, 5):
    r = table.recs[obj - 1]
    if obj not in (2, 4):
      assert r.nf == 0
      continue
    ix = mesh_index.build(models[obj]['pts'], models[obj]['faces'])
    assert (r.nf, r.nleaf, r.nalways, r.top) == (ix['nf'], ix['nleaf'], ix['nalways'], ix['top'])
    assert (r.tri_off, r.fid_off) == (goff, foff)
    assert table.geom[r.tri_off:r.tri_off + len(ix['tri'])].tobytes() == ix['tri'].tobytes()
    assert table.fid[r.fid_off:r.fid_off + len(ix['fid'])].tobytes() == ix['fid'].tobytes()
    goff += len(ix['tri']); foff += len(ix['fid'])
    for level, bx in enumerate(ix['boxes']):
      assert r.box_off[level] == goff and r.count[level] == ix['count'][level]
      assert table.geom[goff:goff + len(bx)].tobytes() == bx.tobytes()
      goff += len(bx)
    assert list(r.near_lo) == list(ix['near_lo']) and list(r.near_hi) == list(ix['near_hi'])
  assert goff == len(table.geom) and foff == len(table.fid)


QUERY_ARGS = {
    'soup': dict(n_random=60), 'sphere': dict(n_random=40, centre=True),
    'duplicate': dict(n_random=20, centre=True), 'zero_area': dict(n_random=60),
    'slivers': dict(n_random=60), 'grid4097': dict(n_random=14),
}


def _queries(name):
  verts, faces = MESHES[name]
  pts = mesh_cases.queries(verts, faces, **QUERY_ARGS[name])
  if name == 'duplicate':           # on and near the duplicated face: both copies tie
    dup = verts[faces[-1]]
    pts = np.concatenate([pts, dup.mean(axis=0)[None] * np.array([[1.0], [1.05], [0.9]]), dup])
  if name == 'slivers':             # next to the slivers, where they are the closest faces
    pts = np.concatenate([pts, verts[-9:] + np.array([0.5, 0.1, -0.2])])
  assert len(pts) <= 100
  return pts


@pytest.mark.parametrize('name', sorted(MESHES))
def test_tree_query_equals_the_sweep(indices, name):
  verts, faces = MESHES[name]
  pts = _queries(name)
  with np.errstate(all='ignore'):
    exp, exp_f = project_ref.project_pts_to_model(pts, verts, faces)
  got, got_f, visited = mesh_query_ref.project(indices[name], pts)
  assert got.tobytes() == exp.tobytes()
  assert np.array_equal(got_f, exp_f)
  ix = indices[name]
  blocks = ix['nleaf'] + ix['nalways']
  assert (visited >= 1).all() and (visited <= blocks).all()
  far = ~(np.all(pts >= ix['near_lo'], axis=1) & np.all(pts <= ix['near_hi'], axis=1))
  assert far.sum() == 1 and (visited[far] == blocks).all()      # the far-field query sweeps all
  if name == 'duplicate':
    assert (exp_f != len(faces) - 1).all()                      # the copy never wins a tie
    assert (exp_f == 100).any()
  if name == 'sphere':
    centre = len(pts) - 2
    assert np.array_equal(pts[centre], np.zeros(3))
    assert got_f[centre] == exp_f[centre]


@pytest.mark.parametrize('name', ['sphere', 'grid4097'])
def test_index_prunes(indices, name):
  """Near-surface queries sweep at most a quarter of the leaves on average. The model has room:
  3.21 of 20 leaves on the sphere (cap 5), 7.57 of 65 on the 4097-face mesh (cap 16.25)."""
  verts, faces = MESHES[name]
  ix = indices[name]
  pts = mesh_cases.near_surface(verts, faces, n=100)
  _, _, visited = mesh_query_ref.project(ix, pts)
  assert ix['nalways'] == 0
  assert visited.min() >= 1
  assert visited.mean() <= ix['nleaf'] / 4.0, (visited.mean(), ix['nleaf'])


def test_fitting_path_with_surface_on_device():
  import infer
  for prosac, K, surf, on_dev, surf_dev in itertools.product(
      (False, True), (None, 200), (False, True), (False, True), (False, True)):
    operator, ordered = infer.fitting_path(prosac, K, surf, on_dev, surf_dev)
    assert operator == ((surf and not surf_dev) or not on_dev)
    assert ordered == ((prosac or K is not None) and not operator)
    if not surf_dev:
      assert (operator, ordered) == infer.fitting_path(prosac, K, surf, on_dev)
  args = infer.build_parser().parse_args(['--model', 'm'])
  assert args.surface_on_device is False
  args = infer.build_parser().parse_args(['--model', 'm', '--surface_on_device', 'true'])
  assert args.surface_on_device is True


def test_symbol_declared_and_bound():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  declared = set(re.findall(r'\b(epos_[a-z0-9_]+)\s*\(', header))
  assert 'epos_project_rows_to_mesh_f64' in declared
  assert 'epos_project_rows_to_mesh_f64' in _lib.SYMBOLS
  assert len(_lib.SYMBOLS['epos_project_rows_to_mesh_f64'][1]) == 12
  assert 'EPOS_ABI_VERSION 7' in re.sub(r'\s+', ' ', header)
