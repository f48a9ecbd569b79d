"""Numpy restatement of the device-side ordering stage (epos_corr_order_by_conf,
include/epos_hip.h): confidence order, the rule for when it applies, truncation,
slot_base_out, src_row and the row-order permutation yorder / ypos of the kept rows.
Written from the stage's specification, slot by slot, with numpy's stable sorts."""
import numpy as np


def confidence_order(conf):
  """conf descending, ties by ascending row."""
  return np.argsort(-np.asarray(conf), kind='stable')


def slot_rows(slot_base, capacity):
  """[(first pooled row, rows)] per slot, bounds clamped to [0, capacity]."""
  sb = np.clip(np.asarray(slot_base, np.int64), 0, capacity)
  return [(int(sb[s]), int(max(sb[s + 1] - sb[s], 0))) for s in range(len(sb) - 1)]


def order_stage(conf, coord_2d, coord_3d, slot_base, capacity, max_corr, always_sort):
  """Returns dict(slot_base_out i64[S+1], coord_2d f64[N',2], coord_3d f64[N',3],
  src_row i32[N'], yorder i32[N'], ypos i32[N'], applied bool[S])."""
  K = int(max_corr) if max_corr is not None and max_corr > 0 else 0
  base_out, c2, c3, src, yorder, ypos, applied = [0], [], [], [], [], [], []
  for lo, n in slot_rows(slot_base, capacity):
    apply = bool(always_sort) or (K > 0 and n > K)
    perm = confidence_order(conf[lo:lo + n]) if apply else np.arange(n)
    keep = perm[:min(n, K) if K > 0 else n]
    xy = coord_2d[lo:lo + n][keep]
    yo = np.argsort(xy[:, 1], kind='stable')       # the host entry's std::stable_sort by y
    yp = np.empty_like(yo)
    yp[yo] = np.arange(len(yo))
    applied.append(apply)
    base_out.append(base_out[-1] + len(keep))
    c2.append(xy)
    c3.append(coord_3d[lo:lo + n][keep])
    src.append(keep)
    yorder.append(yo)
    ypos.append(yp)
  cat = lambda parts, dt, tail: (np.concatenate(parts).astype(dt) if parts     # noqa: E731
                                 else np.zeros((0,) + tail, dt))
  return {'slot_base_out': np.asarray(base_out, np.int64),
          'coord_2d': cat(c2, np.float64, (2,)).reshape(-1, 2),
          'coord_3d': cat(c3, np.float64, (3,)).reshape(-1, 3),
          'src_row': cat(src, np.int32, ()), 'yorder': cat(yorder, np.int32, ()),
          'ypos': cat(ypos, np.int32, ()), 'applied': np.asarray(applied, bool)}
