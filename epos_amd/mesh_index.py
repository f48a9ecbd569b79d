"""Host-side spatial index of a triangle mesh for the indexed closest-point query
(csrc/mesh_project.hip, ``epos_project_rows_to_mesh_f64``): numpy only, deterministic, built
once per pipeline. DESIGN.md, "Mesh index", holds the argument that a query through this
index returns what the exhaustive sweep returns, bit for bit; the constants below are the
thresholds that argument derives.

Structure of one mesh: the faces that qualify for the tree, sorted by the Morton code of
their centroid (ties by face index); a leaf = 64 consecutive sorted faces; level 0 of the
boxes bounds the leaves and node i of level l+1 covers nodes 64i .. 64i+63 of level l, up to
a top level of at most 64 nodes. A face's box is its vertex box grown by
``face_margin``; a node's box is the union of its children's. Faces that do not qualify are
kept in further blocks of 64 that every query sweeps.
"""
import ctypes

import numpy as np

from epos_amd import _lib

LEAF = 64                   # faces per leaf = children per node = lanes of a wavefront
MAX_LEVELS = 4              # box levels of EposMeshRec (enough for 2^30 faces)
TRI_BLOCK = 9 * LEAF        # doubles of a triangle block: [k][lane], k = ax ay az bx .. cz
BOX_GROUP = 6 * LEAF        # doubles of a box group: [k][lane], k = lo xyz, hi xyz

# Near field: the mesh's box grown by NEAR_EXTENTS times its longest side on every side.
# Queries outside sweep every leaf (the error bound of the pruning argument needs
# |query - vertex| <= D = the diagonal of this box).
NEAR_EXTENTS = 1.0
# A face enters the tree iff |ab x ac|^2 >= QUALITY * D * L^3 (L = its longest edge), i.e.
# (2 area / L^2)^2 >= QUALITY * D / L: then the closest point computed for any near-field
# query lies in the face's vertex box grown by L / 8.
QUALITY = 2.0 ** -17
MARGIN_EDGE = 1.0 / 8       # box margin: this fraction of the face's longest edge ...
MARGIN_ABS = 2.0 ** -40     # ... plus this fraction of the largest |coordinate| in reach


def _morton(cells):
  """cells uint64[n,3] (21 bits each) -> uint64[n] with the bits interleaved (x lowest)."""
  code = np.zeros(len(cells), np.uint64)
  for bit in range(21):
    for k in range(3):
      code |= ((cells[:, k] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + k)
  return code


def _group_boxes(lo, hi):
  """Boxes of the next level: union over runs of 64."""
  n = len(lo)
  g = (n + LEAF - 1) // LEAF
  plo = np.full((g * LEAF, 3), np.inf); phi = np.full((g * LEAF, 3), -np.inf)
  plo[:n] = lo; phi[:n] = hi
  return plo.reshape(g, LEAF, 3).min(axis=1), phi.reshape(g, LEAF, 3).max(axis=1)


def _pack_groups(lo, hi):
  """[n,3] boxes -> ceil(n / 64) groups of 6 x 64 doubles (unused places 0)."""
  n = len(lo)
  g = (n + LEAF - 1) // LEAF
  out = np.zeros((g * LEAF, 6))
  out[:n, :3] = lo; out[:n, 3:] = hi
  return np.ascontiguousarray(out.reshape(g, LEAF, 6).transpose(0, 2, 1)).reshape(-1)


def _pack_triangles(tris, ids):
  """tris [n,9], ids [n] -> blocks of 9 x 64 doubles and 64 face ids (-1 = empty place)."""
  n = len(ids)
  g = (n + LEAF - 1) // LEAF
  t = np.zeros((g * LEAF, 9)); f = np.full(g * LEAF, -1, np.int32)
  t[:n] = tris; f[:n] = ids
  return np.ascontiguousarray(t.reshape(g, LEAF, 9).transpose(0, 2, 1)).reshape(-1), f


def build(verts, faces):
  """Index of one mesh (verts [V,3], faces [F,3]) as a dict of flat arrays:
  nf, nleaf, nalways (blocks), top, count[4], tri f64 (tree leaves, then the always-swept
  blocks), fid int32, boxes [top+1 arrays of box groups], near_lo / near_hi, and for
  inspection order (tree faces as sorted), always (face ids), leaf_lo / leaf_hi."""
  verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
  faces = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
  nf = len(faces)
  if nf < 1 or nf >= 1 << 30:
    raise ValueError('a mesh needs between 1 and 2^30 - 1 faces')
  if faces.min() < 0 or faces.max() >= len(verts):
    raise ValueError('face refers to a vertex that does not exist')
  tris = verts[faces].reshape(nf, 9)
  a, b, c = tris[:, 0:3], tris[:, 3:6], tris[:, 6:9]
  finite = np.isfinite(tris).all(axis=1)
  used = tris[finite].reshape(-1, 3)
  if len(used):
    mlo, mhi = used.min(axis=0), used.max(axis=0)
    grow = NEAR_EXTENTS * float((mhi - mlo).max())
    near_lo, near_hi = mlo - grow, mhi + grow
    reach = float(np.sqrt(((near_hi - near_lo) ** 2).sum()))          # D
    largest = float(max(np.abs(near_lo).max(), np.abs(near_hi).max()))
  else:                                 # nothing finite: no tree, every query is far
    mlo = mhi = np.zeros(3)
    near_lo, near_hi = np.full(3, np.inf), np.full(3, -np.inf)
    reach = largest = 0.0
  with np.errstate(all='ignore'):
    ab, ac, bc = b - a, c - a, c - b
    edge = np.sqrt(np.maximum(np.maximum((ab * ab).sum(1), (ac * ac).sum(1)),
                              (bc * bc).sum(1)))
    cr = np.cross(ab, ac)
    area2 = (cr * cr).sum(1)                                           # (2 area)^2
    in_tree = finite & (area2 > 0.0) & (area2 >= QUALITY * reach * edge ** 3)
  ids = np.arange(nf)
  tree, always = ids[in_tree], ids[~in_tree]
  # Morton order of the centroids on a 2^21 grid over the mesh box, ties by face index
  cent = (a[tree] + b[tree] + c[tree]) / 3.0
  side = np.where(mhi > mlo, mhi - mlo, 1.0)
  cells = np.clip(np.floor((cent - mlo) / side * (2 ** 21 - 1)), 0, 2 ** 21 - 1)
  order = tree[np.lexsort((tree, _morton(cells.astype(np.uint64))))]
  margin = (MARGIN_EDGE * edge[order] + MARGIN_ABS * largest)[:, None]
  t = tris[order].reshape(-1, 3, 3)
  flo, fhi = t.min(axis=1) - margin, t.max(axis=1) + margin
  lo, hi = _group_boxes(flo, fhi) if len(order) else (np.zeros((0, 3)), np.zeros((0, 3)))
  leaf_lo, leaf_hi = lo, hi
  boxes, count = [], [0] * MAX_LEVELS
  level = 0
  while len(lo):
    if level >= MAX_LEVELS:
      raise ValueError('mesh too large for a %d-level index' % MAX_LEVELS)
    boxes.append(_pack_groups(lo, hi))
    count[level] = len(lo)
    if len(lo) <= LEAF:
      break
    lo, hi = _group_boxes(lo, hi)
    level += 1
  tri_t, fid_t = _pack_triangles(tris[order], order)
  tri_a, fid_a = _pack_triangles(tris[always], always)
  return {
      'nf': nf, 'nleaf': len(leaf_lo), 'nalways': len(fid_a) // LEAF,
      'top': max(len(boxes) - 1, 0), 'count': count,
      'tri': np.concatenate([tri_t, tri_a]), 'fid': np.concatenate([fid_t, fid_a]),
      'boxes': boxes, 'near_lo': near_lo, 'near_hi': near_hi,
      'order': order.astype(np.int32), 'always': always.astype(np.int32),
      'leaf_lo': leaf_lo, 'leaf_hi': leaf_hi,
  }


class MeshTable(object):
  """The indices of the objects of ``models`` ({obj_id: {'pts', 'faces'}}) concatenated:
  geom (f64), fid (int32) and one EposMeshRec per obj_id - 1 (nf = 0: no mesh). With a
  device the three arrays are uploaded once (geom_dev, fid_dev, recs_dev); device=None keeps
  the host arrays only."""

  def __init__(self, models, num_objs, device=None):
    self.num_objs = int(num_objs)
    self.recs = (_lib.MeshRec * max(self.num_objs, 1))()
    self.index = {}
    geom, fid = [], []
    goff = foff = 0
    for obj_id in sorted(models):
      if not 1 <= obj_id <= self.num_objs:
        continue
      ix = build(models[obj_id]['pts'], models[obj_id]['faces'])
      self.index[obj_id] = ix
      r = self.recs[obj_id - 1]
      r.tri_off, r.fid_off = goff, foff
      geom.append(ix['tri']); goff += len(ix['tri'])
      fid.append(ix['fid']); foff += len(ix['fid'])
      for l, bx in enumerate(ix['boxes']):
        r.box_off[l] = goff
        r.count[l] = ix['count'][l]
        geom.append(bx); goff += len(bx)
      r.nf, r.nleaf, r.nalways, r.top = ix['nf'], ix['nleaf'], ix['nalways'], ix['top']
      for k in range(3):
        r.near_lo[k], r.near_hi[k] = ix['near_lo'][k], ix['near_hi'][k]
    self.geom = np.concatenate(geom) if geom else np.zeros(1)
    self.fid = np.concatenate(fid) if fid else np.full(1, -1, np.int32)
    self.obj_ids = sorted(self.index)
    if device is not None:
      import torch
      self.geom_dev = torch.from_numpy(self.geom).to(device)
      self.fid_dev = torch.from_numpy(self.fid).to(device)
      raw = np.frombuffer(bytes(self.recs), np.uint8).copy()
      self.recs_dev = torch.from_numpy(raw).to(device)

  def has_mesh(self, obj_id):
    return obj_id in self.index


assert ctypes.sizeof(_lib.MeshRec) == 128
