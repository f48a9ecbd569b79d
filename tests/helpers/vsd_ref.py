"""The VSD counts of include/epos_hip.h, "VSD", restated in element-wise numpy: fp64, the same
operations in the same order, integer counts. csrc/vsd.hip must equal this exactly."""
import numpy as np


def counts(depth_test, depth_model, pair, delta, taus):
  """depth_test f32 [n_images,h,w], depth_model f32 [n_inst,h,w], pair a record or dict with
  image, gt_inst, est_inst, x0, y0, x1, y1, fx, fy, cx, cy, diameter -> i64 [6 + n_taus]."""
  g = lambda k: pair[k]            # noqa: E731
  x0, y0, x1, y1 = int(g('x0')), int(g('y0')), int(g('x1')), int(g('y1'))
  taus = np.asarray(taus, np.float64)
  out = np.zeros(6 + len(taus), np.int64)
  if x1 <= x0 or y1 <= y0:
    return out
  win = (slice(y0, y1), slice(x0, x1))
  zt = np.asarray(depth_test[int(g('image'))], np.float32)[win].astype(np.float64)
  zg = np.asarray(depth_model[int(g('gt_inst'))], np.float32)[win].astype(np.float64)
  if int(g('est_inst')) < 0:
    ze = np.zeros_like(zg)
  else:
    ze = np.asarray(depth_model[int(g('est_inst'))], np.float32)[win].astype(np.float64)
  fx, fy, cx, cy = (np.float64(g(k)) for k in ('fx', 'fy', 'cx', 'cy'))
  diameter = np.float64(g('diameter'))
  delta = np.float64(delta)
  xs = np.arange(x0, x1, dtype=np.float64)[None, :]
  ys = np.arange(y0, y1, dtype=np.float64)[:, None]
  with np.errstate(invalid='ignore', over='ignore'):
    missing = ~(zt > 0)
    rx = ((xs + 0.5) - cx) / fx
    ry = ((ys + 0.5) - cy) / fy
    s = np.sqrt((rx * rx + ry * ry) + 1.0)
    dt, dg, de = zt * s, zg * s, ze * s
    mask_g, mask_e = zg > 0, ze > 0
    vis_g = mask_g & (missing | (dg - dt <= delta))
    vis_e = mask_e & (missing | (de - dt <= delta) | vis_g)
    inter, uni = vis_g & vis_e, vis_g | vis_e
    d = np.abs(dg - de) / diameter
  out[:6] = [mask_g.sum(), vis_g.sum(), mask_e.sum(), vis_e.sum(), inter.sum(), uni.sum()]
  for k, tau in enumerate(taus):
    out[6 + k] = int((inter & (d >= tau)).sum())
  return out


def counts_table(depth_test, depth_model, pairs, delta, taus):
  """i64 [n_pairs, 6 + n_taus]."""
  if not len(pairs):
    return np.zeros((0, 6 + len(taus)), np.int64)
  return np.stack([counts(depth_test, depth_model, p, delta, taus) for p in pairs])
