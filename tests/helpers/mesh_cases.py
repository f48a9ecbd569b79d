"""Meshes and query points of the mesh-index tests (CPU model and GPU kernel share them)."""
import numpy as np


def soup(seed=0, nv=60, nf=90):
  """Random triangle soup, as _toy_mesh of test_gpu_corresp_fit.py."""
  rng = np.random.RandomState(seed)
  verts = rng.uniform(-50, 50, (nv, 3))
  faces = np.stack([rng.choice(nv, 3, replace=False) for _ in range(nf)]).astype(np.int32)
  return verts, faces


def icosphere(subdiv=3, radius=40.0, scale=(1.0, 1.0, 1.0)):
  """20 * 4^subdiv faces (subdiv 3: 1280), vertices on the ellipsoid radius * scale."""
  t = (1.0 + 5.0 ** 0.5) / 2.0
  v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t),
       (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
  verts = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
  faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4),
           (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8),
           (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
  for _ in range(subdiv):
    mid, out = {}, []

    def midpoint(i, j):
      key = (min(i, j), max(i, j))
      if key not in mid:
        m = verts[i] + verts[j]
        verts.append(m / np.linalg.norm(m))
        mid[key] = len(verts) - 1
      return mid[key]
    for a, b, c in faces:
      ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
      out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    faces = out
  return (np.asarray(verts) * radius * np.asarray(scale, np.float64),
          np.asarray(faces, np.int32))


def with_duplicate(verts, faces, which=100):
  """The mesh plus a second copy of face `which` at the end (tie rule: the lower index wins)."""
  return verts, np.concatenate([faces, faces[which:which + 1]]).astype(np.int32)


def with_zero_area(verts, faces):
  """Plus faces of exactly zero area: a repeated vertex, three equal vertices, and three
  distinct collinear vertices (the midpoint of an edge is added as a vertex)."""
  mid = 0.5 * (verts[faces[0, 0]] + verts[faces[0, 1]])
  v = np.concatenate([verts, mid[None], 2.0 * verts[faces[0, 1]][None] - verts[faces[0, 0]][None]])
  n = len(verts)
  extra = [(faces[0, 0], faces[0, 0], faces[0, 1]), (faces[1, 2],) * 3,
           (faces[0, 0], faces[0, 1], n + 1)]
  return v, np.concatenate([faces, np.asarray(extra, np.int32)]).astype(np.int32)


def with_slivers(verts, faces, aspects=(1e-3, 1e-8, 1e-12)):
  """Plus one sliver per aspect ratio (height / base) standing next to the mesh."""
  v, f = [verts], [faces]
  n = len(verts)
  for i, asp in enumerate(aspects):
    base = np.array([45.0 + 3 * i, -10.0, 5.0 * i])
    v.append(np.stack([base, base + [0.0, 20.0, 0.0], base + [20.0 * asp, 9.0, 0.0]]))
    f.append(np.array([[n, n + 1, n + 2]], np.int32))
    n += 3
  return np.concatenate(v), np.concatenate(f).astype(np.int32)


def grid4097(nx=64, ny=32):
  """A bumpy height field of 2 * 64 * 32 = 4096 faces plus one more: 4097 faces, 65 leaves,
  hence a third level in the index."""
  xs, ys = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64))
  z = 4.0 * np.sin(0.37 * xs) * np.cos(0.29 * ys)
  verts = np.stack([2.0 * xs.ravel() - nx, 2.0 * ys.ravel() - ny, z.ravel()], axis=1)
  idx = lambda i, j: j * (nx + 1) + i      # noqa: E731
  faces = []
  for j in range(ny):
    for i in range(nx):
      faces += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)),
                (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
  n = len(verts)
  verts = np.concatenate([verts, [[-nx, -ny - 3.0, 1.0], [-nx + 2.0, -ny - 3.0, 0.0],
                                  [-nx + 1.0, -ny - 1.5, 2.0]]])
  faces.append((n, n + 1, n + 2))
  return verts, np.asarray(faces, np.int32)


def queries(verts, faces, n_random=60, seed=1, centre=False, far=True):
  """Query points (at most 100): random ones inside and outside the mesh box, points exactly
  on vertices, edge midpoints, face centroids, optionally the centre, and one point beyond
  the far-field limit of the index."""
  rng = np.random.RandomState(seed)
  lo, hi = verts.min(axis=0), verts.max(axis=0)
  ext = float((hi - lo).max())
  pts = [rng.uniform(lo - 0.3 * ext, hi + 0.3 * ext, (n_random, 3))]
  fs = faces[rng.choice(len(faces), 8, replace=False)]
  pts.append(verts[fs[:, 0]])
  pts.append(0.5 * (verts[fs[:, 0]] + verts[fs[:, 1]]))
  pts.append((verts[fs[:, 0]] + verts[fs[:, 1]] + verts[fs[:, 2]]) / 3.0)
  if centre:
    pts.append(np.zeros((1, 3)))
  if far:
    pts.append((hi + 5.0 * ext)[None])
  return np.concatenate(pts)


def near_surface(verts, faces, n=60, seed=2, offset=0.02):
  """Points within `offset` x the longest side of the mesh of random faces' interiors."""
  rng = np.random.RandomState(seed)
  fs = faces[rng.choice(len(faces), n)]
  w = rng.dirichlet([1.0, 1.0, 1.0], n)
  p = (w[:, :1] * verts[fs[:, 0]] + w[:, 1:2] * verts[fs[:, 1]] + w[:, 2:] * verts[fs[:, 2]])
  ext = float((verts.max(axis=0) - verts.min(axis=0)).max())
  return p + rng.uniform(-offset, offset, (n, 3)) * ext
