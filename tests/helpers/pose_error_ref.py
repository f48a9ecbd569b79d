"""The pose errors of include/epos_hip.h, "Pose errors", in element-wise numpy: every product
and sum is written out, so that the operation order is the definition's (no dot, no matmul:
a BLAS may fuse or reorder). csrc/pose_error.hip equals `errors` bit for bit. `errors_plain`
is the textbook formulation (R.dot(pts.T)), which agrees to rounding."""
import numpy as np

PARTS = 256


def compose(Rg, tg, sym):
  """R' = R_g R_s, t' = R_g t_s + t_g of one symmetry (12 numbers): each element
  (a0 b0 + a1 b1) + a2 b2, t_g added last."""
  Rg = np.asarray(Rg, np.float64).reshape(3, 3)
  tg = np.asarray(tg, np.float64).reshape(3)
  Rs, ts = np.asarray(sym[:9], np.float64).reshape(3, 3), np.asarray(sym[9:12], np.float64)
  R, t = np.empty((3, 3)), np.empty(3)
  for i in range(3):
    for j in range(3):
      R[i, j] = (Rg[i, 0] * Rs[0, j] + Rg[i, 1] * Rs[1, j]) + Rg[i, 2] * Rs[2, j]
    t[i] = ((Rg[i, 0] * ts[0] + Rg[i, 1] * ts[1]) + Rg[i, 2] * ts[2]) + tg[i]
  return R, t


def transform(R, t, X):
  """(x, y, z) arrays of R X_v + t, each row ((r0 x + r1 y) + r2 z) + t."""
  R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
  x, y, z = X[:, 0], X[:, 1], X[:, 2]
  return [((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)]


def fixed_sum(terms):
  """The header's sum shape: 256 strided left-to-right partial sums, then a halving tree."""
  terms = np.asarray(terms, np.float64)
  rows = -(-len(terms) // PARTS)
  pad = np.zeros(rows * PARTS)
  pad[:len(terms)] = terms                     # p + 0.0 == p
  pad = pad.reshape(rows, PARTS)
  p = np.zeros(PARTS)
  for r in range(rows):
    p = p + pad[r]
  s = PARTS // 2
  while s >= 1:
    p[:s] = p[:s] + p[s:2 * s]
    s //= 2
  return p[0]


def errors(X, syms, R_e, t_e, R_g, t_g, cam, want_adi=True):
  """(mssd, mspd, add, adi) of one pair; X f64 [n,3], syms f64 [S,12], cam = (fx, fy, cx, cy).
  adi is nan without want_adi."""
  X = np.asarray(X, np.float64).reshape(-1, 3)
  syms = np.asarray(syms, np.float64).reshape(-1, 12)
  fx, fy, cx, cy = [np.float64(v) for v in cam]
  ex, ey, ez = transform(R_e, t_e, X)
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    ue, ve = (fx * ex) / ez + cx, (fy * ey) / ez + cy
  best3 = best2 = np.inf
  for k in range(len(syms)):
    R, t = compose(R_g, t_g, syms[k])
    gx, gy, gz = transform(R, t, X)
    dx, dy, dz = ex - gx, ey - gy, ez - gz
    d3 = (dx * dx + dy * dy) + dz * dz
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
      ug, vg = (fx * gx) / gz + cx, (fy * gy) / gz + cy
      du, dv = ue - ug, ve - vg
      d2 = np.where((ez <= 0.0) | (gz <= 0.0), np.inf, du * du + dv * dv)
    best3 = min(best3, d3.max())
    best2 = min(best2, d2.max())
    if k == 0:
      add = fixed_sum(np.sqrt(d3)) / np.float64(len(X))
      adi = np.nan
      if want_adi:
        nearest = np.empty(len(X))
        for v0 in range(0, len(X), 512):        # [w, v] blocks of squared distances
          sl = slice(v0, v0 + 512)
          ax, ay, az = (ex[:, None] - gx[None, sl], ey[:, None] - gy[None, sl],
                        ez[:, None] - gz[None, sl])
          nearest[sl] = ((ax * ax + ay * ay) + az * az).min(axis=0)
        adi = fixed_sum(np.sqrt(nearest)) / np.float64(len(X))
  return np.array([np.sqrt(best3), np.sqrt(best2), add, adi])


def errors_plain(X, syms, R_e, t_e, R_g, t_g, cam, want_adi=True):
  """The published formulas with matrix products (Hodan et al. 2020, section 2.2)."""
  X = np.asarray(X, np.float64).reshape(-1, 3)
  K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1.0]])
  R_e, R_g = np.asarray(R_e).reshape(3, 3), np.asarray(R_g).reshape(3, 3)
  t_e, t_g = np.asarray(t_e).reshape(3, 1), np.asarray(t_g).reshape(3, 1)

  def project(P):
    uvw = K.dot(P)
    return uvw[:2] / uvw[2:]
  E = R_e.dot(X.T) + t_e
  mssd, mspd = [], []
  for s in np.asarray(syms, np.float64).reshape(-1, 12):
    Rs, ts = s[:9].reshape(3, 3), s[9:].reshape(3, 1)
    G = R_g.dot(Rs.dot(X.T) + ts) + t_g
    mssd.append(np.linalg.norm(E - G, axis=0).max())
    bad = (E[2] <= 0) | (G[2] <= 0)
    with np.errstate(divide='ignore', invalid='ignore'):
      d = np.linalg.norm(project(E) - project(G), axis=0)
    mspd.append(np.where(bad, np.inf, d).max())
  s0 = np.asarray(syms, np.float64).reshape(-1, 12)[0]
  G = R_g.dot(s0[:9].reshape(3, 3).dot(X.T) + s0[9:].reshape(3, 1)) + t_g
  add = np.linalg.norm(E - G, axis=0).mean()
  adi = np.nan
  if want_adi:
    adi = np.mean([np.linalg.norm(E - G[:, v:v + 1], axis=0).min() for v in range(X.shape[0])])
  return np.array([min(mssd), min(mspd), add, adi])
