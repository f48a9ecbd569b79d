"""VSD (Visible Surface Discrepancy) of estimated against ground-truth poses: the pixel counts
on the device (csrc/vsd.hip) over depth renderings of the mesh renderer (epos_amd/render.py),
the errors, the visible fraction of every ground-truth instance, and the recalls AR_VSD and
AR = (AR_VSD + AR_MSSD + AR_MSPD) / 3 on the host.

The reference leaves pose scoring to ``bop_toolkit`` (an empty submodule there). Everything
here is THIS BUILD'S DEFINITION after the published BOP'19 formulas, written out in
include/epos_hip.h, "VSD": parity with bop_toolkit's numbers is unpinned, the ray of a pixel
goes through x + .5, y + .5 -- the sample point of this build's renderer, not necessarily
bop_toolkit's -- and tests/helpers/vsd_ref.py restates the counts in numpy, exactly.

There is no CPU fallback: without the library or a device VsdEval raises EposError.
``window``, ``vsd_from_counts``, ``visib_fract`` and ``recalls_vsd`` are plain numpy.
"""
import ctypes

import numpy as np

from epos_amd import _call as C
from epos_amd import _lib, pose_error

VSD_DELTA = 15.0                                          # mm, the visibility tolerance
VSD_TAUS = tuple(0.05 * k for k in range(1, 11))          # x object diameter
VSD_THRESHOLDS = tuple(0.05 * k for k in range(1, 11))    # an estimate is correct below these
N_FIXED = 6                                               # counters in front of the per-tau ones
MEMORY_BUDGET = 1 << 30          # bytes of renderer workspace (keys + depth) one chunk may take
BYTES_PER_PIXEL = 12             # i64 key + f32 depth per pixel and instance

# EposVsdPair as a numpy record (72 bytes)
PAIR_DTYPE = np.dtype([('image', '<i4'), ('gt_inst', '<i4'), ('est_inst', '<i4'),
                       ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'),
                       ('reserved0', '<i4'), ('fx', '<f8'), ('fy', '<f8'), ('cx', '<f8'),
                       ('cy', '<f8'), ('diameter', '<f8')])
assert PAIR_DTYPE.itemsize == ctypes.sizeof(_lib.VsdPair) == 72


def bbox_corners(pts):
  """The eight corners [8,3] of the axis-aligned box of a model's vertices."""
  pts = np.asarray(pts, np.float64).reshape(-1, 3)
  lo, hi = pts.min(axis=0), pts.max(axis=0)
  return np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]]
                   for i in (0, 1) for j in (0, 1) for k in (0, 1)])


def window(model_bbox_corners, R, t, K, h, w, near):
  """A conservative pixel window (x0, y0, x1, y1), x0 <= x < x1, of one instance: the bounding
  rectangle of the eight projected corners of the model's box, widened by one pixel and
  clipped to the image. The rectangle only bounds the rendering when the whole box is in front
  of the camera, so the window is the FULL IMAGE whenever a corner has Zc < near (or anything
  is not finite). Correctness never depends on the window being tight."""
  full = (0, 0, int(w), int(h))
  K = np.asarray(K, np.float64).reshape(3, 3)
  P = np.asarray(model_bbox_corners, np.float64).reshape(-1, 3).dot(
      np.asarray(R, np.float64).reshape(3, 3).T) + np.asarray(t, np.float64).reshape(1, 3)
  if not (np.isfinite(P).all() and np.isfinite(K).all()) or (P[:, 2] < near).any():
    return full
  u = K[0, 0] * P[:, 0] / P[:, 2] + K[0, 2]
  v = K[1, 1] * P[:, 1] / P[:, 2] + K[1, 2]
  if not (np.isfinite(u).all() and np.isfinite(v).all()) or \
      max(np.abs(u).max(), np.abs(v).max()) > 1e9:
    return full
  x0 = min(max(int(np.floor(u.min())) - 1, 0), int(w))
  y0 = min(max(int(np.floor(v.min())) - 1, 0), int(h))
  x1 = max(min(int(np.floor(u.max())) + 2, int(w)), x0)
  y1 = max(min(int(np.floor(v.max())) + 2, int(h)), y0)
  return x0, y0, x1, y1


def union(a, b):
  """The smallest window holding both; an empty window holds nothing and is ignored."""
  if a[2] <= a[0] or a[3] <= a[1]:
    return tuple(b)
  if b[2] <= b[0] or b[3] <= b[1]:
    return tuple(a)
  return min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3])


def _rows(counts):
  c = np.asarray(counts, np.int64)
  if c.ndim != 2 or c.shape[1] <= N_FIXED:
    raise ValueError('counts must be [n, 6 + n_taus], got %s' % (c.shape,))
  return c


def vsd_from_counts(counts):
  """i64 [n, 6 + n_taus] -> f64 [n, n_taus]: (ge_k + (uni - inter)) / uni, 1.0 where uni == 0
  (nothing of either rendering is visible)."""
  c = _rows(counts)
  inter, uni = c[:, 4].astype(np.float64), c[:, 5].astype(np.float64)
  out = np.ones((len(c), c.shape[1] - N_FIXED))
  ok = c[:, 5] > 0
  out[ok] = (c[ok, N_FIXED:].astype(np.float64) + (uni[ok] - inter[ok])[:, None]) / \
      uni[ok][:, None]
  return out


def visib_fract(counts):
  """#vis_g / #mask_g of every row, 0 where the ground-truth rendering is empty."""
  c = _rows(counts)
  out = np.zeros(len(c))
  ok = c[:, 0] > 0
  out[ok] = c[ok, 1].astype(np.float64) / c[ok, 0].astype(np.float64)
  return out


def default_max_instances(h, w, budget=MEMORY_BUDGET):
  """Instances (ground truths + estimates) of one chunk at image size (h, w): what the
  renderer's workspace of 12 bytes per pixel and instance (i64 keys + f32 depth) fits into
  `budget` bytes, and n_inst * h * w < 2^31 (epos_vsd_counts)."""
  px = max(1, int(h) * int(w))
  return max(2, min(int(budget) // (BYTES_PER_PIXEL * px), (2 ** 31 - 1) // px))


class VsdEval(object):
  """A render.Renderer with the `models` ({obj_id: {'pts', 'faces'}}, the 'eval' models) and
  the diameters of `models_info`. max_instances: instances per chunk (None: derived from the
  image size, default_max_instances)."""

  def __init__(self, models, models_info, device=None, max_instances=None):
    from epos_amd import cli
    C.need_device(None, 'VSD needs a HIP device (there is no CPU fallback)')
    self.lib = _lib.load()
    self.renderer = cli.eval_renderer(models, device)
    self.device = self.renderer.device
    if max_instances is not None and int(max_instances) < 2:
      raise ValueError('max_instances must be >= 2 (a ground truth and its estimate)')
    self.max_instances = None if max_instances is None else int(max_instances)
    self.corners, self.diameters = {}, {}
    for o in sorted(models):
      self.corners[o] = bbox_corners(models[o]['pts'])
      if 'diameter' in models_info.get(o, {}):
        self.diameters[o] = float(models_info[o]['diameter'])
    if not self.corners:
      raise ValueError('no object models')

  @staticmethod
  def _finite(*arrays):
    return all(np.isfinite(np.asarray(a, np.float64)).all() for a in arrays)

  def plan(self, frames, pairs):
    """Chunks of the pairs that can reach the device. Returns (chunks, skipped): a chunk is
    {'size': (h, w), 'frames': [frame index], 'inst': [(obj_id, R, t, K)], 'rows': [(pair
    index, image, gt_inst, est_inst, window, K, diameter)]}; `skipped` the pairs whose ground
    truth or camera is not finite."""
    by_size, skipped = {}, []
    for i, p in enumerate(pairs):
      depth, K = frames[p['frame']]
      if int(p['obj_id']) not in self.diameters:
        raise ValueError('models_info gives no diameter for object %d' % int(p['obj_id']))
      if not self._finite(K, p['R_g'], p['t_g']):
        skipped.append(i)
        continue
      by_size.setdefault(tuple(np.shape(depth)), []).append(i)
    chunks = []
    for (h, w), idx in sorted(by_size.items()):
      # never more than epos_vsd_counts takes: n_inst * h * w < 2^31
      cap = max(2, min(self.max_instances or default_max_instances(h, w),
                       (2 ** 31 - 1) // max(1, h * w)))
      chunk = None
      for i in sorted(idx, key=lambda j: pairs[j]['frame']):
        p = pairs[i]
        K = np.asarray(frames[p['frame']][1], np.float64).reshape(3, 3)
        o = int(p['obj_id'])
        has_est = p.get('R_e') is not None and self._finite(p['R_e'], p['t_e'])
        keys = [(p['frame'], o, np.asarray(p['R_g'], np.float64).tobytes(),
                 np.asarray(p['t_g'], np.float64).tobytes())]
        poses = [(p['R_g'], p['t_g'])]
        if has_est:
          keys.append((p['frame'], o, np.asarray(p['R_e'], np.float64).tobytes(),
                       np.asarray(p['t_e'], np.float64).tobytes()))
          poses.append((p['R_e'], p['t_e']))
        new = 0 if chunk is None else sum(k not in chunk['index'] for k in set(keys))
        if chunk is None or len(chunk['inst']) + new > cap:
          chunk = {'size': (h, w), 'frames': [], 'inst': [], 'rows': [], 'index': {},
                   'image': {}}
          chunks.append(chunk)
        if p['frame'] not in chunk['image']:
          chunk['image'][p['frame']] = len(chunk['frames'])
          chunk['frames'].append(p['frame'])
        slots, win = [], (0, 0, 0, 0)
        for key, (R, t) in zip(keys, poses):
          if key not in chunk['index']:
            chunk['index'][key] = len(chunk['inst'])
            chunk['inst'].append((o, np.asarray(R, np.float64).reshape(3, 3),
                                  np.asarray(t, np.float64).reshape(3), K))
          slots.append(chunk['index'][key])
          win = union(win, window(self.corners[o], R, t, K, h, w, self.renderer.near))
        chunk['rows'].append((i, chunk['image'][p['frame']], slots[0],
                              slots[1] if has_est else -1, win, K, self.diameters[o]))
    return chunks, skipped

  def table(self, chunk, full_windows=False):
    """The EposVsdPair records of a chunk (PAIR_DTYPE)."""
    h, w = chunk['size']
    tab = np.zeros(len(chunk['rows']), PAIR_DTYPE)
    for r, (_, image, gt, est, win, K, diameter) in enumerate(chunk['rows']):
      tab[r]['image'], tab[r]['gt_inst'], tab[r]['est_inst'] = image, gt, est
      tab[r]['x0'], tab[r]['y0'], tab[r]['x1'], tab[r]['y1'] = \
          (0, 0, w, h) if full_windows else win
      tab[r]['fx'], tab[r]['fy'], tab[r]['cx'], tab[r]['cy'] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
      tab[r]['diameter'] = diameter
    return tab

  def render(self, chunk):
    """depth f32 [n_inst,h,w] of a chunk's instances (the renderer's workspace)."""
    h, w = chunk['size']
    inst = chunk['inst']
    return self.renderer.render_instances(
        [o for o, _, _, _ in inst], np.stack([R for _, R, _, _ in inst]),
        np.stack([t for _, _, t, _ in inst]), np.stack([K for _, _, _, K in inst]),
        size=(w, h), outputs=('depth',))['depth']

  def upload_depth(self, frames, chunk):
    """The test depth images of a chunk, f32 [n_images,h,w] on the device (one upload)."""
    import torch
    h, w = chunk['size']
    host = torch.empty((len(chunk['frames']), h, w), dtype=torch.float32, pin_memory=True)
    for k, fi in enumerate(chunk['frames']):
      host[k].numpy()[:] = np.asarray(frames[fi][0], np.float32)
    return host, host.to(self.device, non_blocking=True)

  def enqueue_counts(self, depth_test, depth_model, tab, delta, taus, counts):
    """One epos_vsd_counts call on the current stream into counts i64 [len(tab), 6 + n_taus].
    Returns what has to stay alive until the stream has been synchronised."""
    import torch
    n = len(tab)
    host = torch.empty((max(n, 1) * PAIR_DTYPE.itemsize,), dtype=torch.uint8, pin_memory=True)
    host.numpy()[:n * PAIR_DTYPE.itemsize] = np.ascontiguousarray(tab).view(np.uint8).reshape(-1)
    dev = torch.empty(host.shape, dtype=torch.uint8, device=self.device)
    taus = np.ascontiguousarray(taus, np.float64)
    n_img, h, w = depth_test.shape
    with C.launch(self.device) as q:
      _lib.check(self.lib.epos_vsd_counts(
          C.ptr(depth_test), n_img, C.ptr(depth_model), depth_model.shape[0], h, w,
          C.ptr(host), C.ptr(dev), n, float(delta), ctypes.c_void_p(taus.ctypes.data), len(taus),
          C.ptr(counts), q.handle), 'epos_vsd_counts')
    return host, dev

  def counts(self, frames, pairs, delta=VSD_DELTA, taus=VSD_TAUS):
    """i64 [n_pairs, 6 + n_taus]: per chunk one render_instances call, one upload of the
    chunk's test depth and one epos_vsd_counts call; one download at the end. The rows of
    pairs that never reach the device stay 0. Only the pinned pair tables (72 bytes a pair) stay
    alive until that download -- the library's copy reads them outside torch's bookkeeping; a
    chunk's depth images, pinned and on the device, are let go as soon as the chunk is enqueued
    (torch's allocators hand such memory out again in stream order), so the footprint is one
    chunk's, not the dataset's."""
    import torch
    n_c = N_FIXED + len(taus)
    chunks, _ = self.plan(frames, pairs)
    out = np.zeros((len(pairs), n_c), np.int64)
    n_rows = sum(len(c['rows']) for c in chunks)
    if not n_rows:
      return out
    dev_counts = torch.empty((n_rows, n_c), dtype=torch.int64, device=self.device)
    tables, order, r0 = [], [], 0
    for chunk in chunks:
      host_depth, depth_test = self.upload_depth(frames, chunk)
      tab = self.table(chunk)
      tables.append(self.enqueue_counts(depth_test, self.render(chunk), tab, delta, taus,
                                        dev_counts[r0:r0 + len(tab)]))
      del host_depth, depth_test
      order += [row[0] for row in chunk['rows']]
      r0 += len(tab)
    out[np.asarray(order, np.int64)] = dev_counts.cpu().numpy()      # synchronises
    del tables
    return out

  def errors(self, frames, pairs, delta=VSD_DELTA, taus=VSD_TAUS):
    """frames: [(depth_mm f32 [h,w], K [3,3])]; pairs: [{frame (index), obj_id, R_g, t_g, R_e,
    t_e}], R_e = None for a ground-truth-only query. Returns (vsd f64 [n_pairs, n_taus],
    gt_visib_fract f64 [n_pairs]). A pair with a non-finite estimate gets VSD 1.0 at every tau
    (its estimate is not rendered); one with a non-finite ground truth or K never reaches the
    device and gets VSD 1.0 and fraction 0."""
    c = self.counts(frames, pairs, delta, taus)
    return vsd_from_counts(c), visib_fract(c)


# ------------------------------------------------------------------ recall ---
def recalls_vsd(groups, vsd_errors=None, taus=VSD_TAUS, thresholds=VSD_THRESHOLDS):
  """groups: [{obj_id, scores [n_est], vsd [n_est, n_gt, n_taus]}] (or the vsd arrays given
  apart, one per group, in `vsd_errors`), one per (image, object), already cut to the top
  estimates. For every tau k and every threshold theta the estimates are matched with
  pose_error.match (strictly below theta); recall = matches / ground-truth instances, pooled
  over the groups of an object and over all of them as in pose_error.recalls. ar_vsd is the
  mean over the len(taus) x len(thresholds) combinations."""
  objs = sorted(set(int(g['obj_id']) for g in groups))
  tp = {o: np.zeros((len(taus), len(thresholds)), np.int64) for o in objs}
  n_gt = dict.fromkeys(objs, 0)
  for gi, g in enumerate(groups):
    o = int(g['obj_id'])
    err = np.asarray(g['vsd'] if vsd_errors is None else vsd_errors[gi], np.float64)
    scores = np.asarray(g['scores'], np.float64).reshape(-1)
    if err.ndim != 3 or err.shape[0] != len(scores) or err.shape[2] != len(taus):
      raise ValueError('vsd must be [n_est, n_gt, n_taus], got %s for %d scores' % (
          err.shape, len(scores)))
    n_gt[o] += err.shape[1]
    if not len(scores) or not err.shape[1]:
      continue
    for k in range(len(taus)):
      for j, theta in enumerate(thresholds):
        tp[o][k, j] += int((pose_error.match(scores, err[:, :, k], theta) >= 0).sum())

  def summary(ids):
    n = sum(n_gt[o] for o in ids)
    hits = sum(tp[o] for o in ids)
    rec = [[float(hits[k, j]) / n if n else 0.0 for j in range(len(thresholds))]
           for k in range(len(taus))]
    return {'targets': int(n), 'recall_vsd': rec, 'ar_vsd': float(np.mean(rec))}
  return {'per_object': {o: summary([o]) for o in objs}, 'overall': summary(objs)}


def ar(ar_vsd, ar_mssd, ar_mspd):
  """BOP'19's AR of one object or of a dataset."""
  return (ar_vsd + ar_mssd + ar_mspd) / 3.0
