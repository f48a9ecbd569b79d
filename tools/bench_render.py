"""Times the mesh renderer (epos_amd/render.py) on the device, warm, with HIP events: the median
of repeated launches of the raster and the resolve pass for 1, 8 and 32 instances of an
icosphere of 20 480 faces at 640 x 480, the same at 160 x 120 followed by epos_gt_fields at 64
and 256 fragments, and beside them the numpy point splat of vis.overlay_object_poses on the
same poses (the host-side way --vis draws poses by default).

    python tools/bench_render.py [--repeats 30] [--out profiles/r15/render.txt]

A second workload gives the time spent in triangles above the lane limit (the ones a whole
wavefront walks): the same sphere standing on a square plate of two triangles, 400 mm a side,
against the sphere alone on the same poses; the share is the difference of the two raster
times over the time with the plate. Beside it: the share of bounding-box samples that belong
to such triangles, computed on the host from the projected boxes.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def icosphere(subdiv, radius):
  t = (1.0 + 5.0 ** 0.5) / 2.0
  verts = [np.asarray(v, np.float64) / np.linalg.norm(v) for v in [
      (-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t),
      (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]]
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
  return np.asarray(verts) * radius, np.asarray(faces, np.int32)


def poses(n, seed=0):
  rng = np.random.RandomState(seed)
  Rs, ts = [], []
  for _ in range(n):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    Rs.append(np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]))
    ts.append([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(500, 900)])
  return np.stack(Rs), np.asarray(ts)


def median_ms(fn, repeats, warmup=5):
  import torch
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
  return float(np.median(times))


def wavefront_share(verts, faces, Rs, ts, K, w, h, limit):
  """Share of clipped bounding-box samples in triangles above the lane limit."""
  total = large = 0
  for R, t in zip(Rs, ts):
    cam = verts @ R.T + t
    uv = cam[:, :2] / cam[:, 2:3] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    tri = uv[faces]
    lo = np.clip(np.ceil(tri.min(axis=1) - 0.5), 0, [w, h])
    hi = np.clip(np.floor(tri.max(axis=1) - 0.5) + 1, 0, [w, h])
    box = np.prod(np.maximum(hi - lo, 0), axis=1)
    total += box.sum()
    large += box[box > limit].sum()
  return large / total if total else 0.0


def main():
  import torch
  from epos_amd import _lib, render, vis
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=30)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  lib = _lib.load()
  limit = lib.epos_render_lane_max_pixels()
  verts, faces = icosphere(5, 60.0)
  ren = render.Renderer('cuda:0')
  ren.add_model(1, {'pts': verts, 'faces': faces})
  plate = np.array([(-200, -200, -60), (200, -200, -60), (200, 200, -60), (-200, 200, -60)],
                   np.float64)
  nv = len(verts)
  verts2 = np.concatenate([verts, plate])
  faces2 = np.concatenate([faces, [[nv, nv + 1, nv + 2], [nv, nv + 2, nv + 3]]]).astype(np.int32)
  ren.add_model(2, {'pts': verts2, 'faces': faces2})
  lines = ['mesh renderer, icosphere of %d faces, median of %d warm launches (HIP events)' % (
      len(faces), args.repeats)]

  def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None

  class Store(object):
    frag_centers = {1: verts[:64]}
    models = {1: {'pts': verts}}

  for (w, h), K in (((640, 480), np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1.0]])),
                    ((160, 120), np.array([[143.1, 0, 81.3], [0, 143.4, 60.5], [0, 0, 1.0]]))):
    for n in (1, 8, 32):
      Rs, ts = poses(n)
      objs = [1] * n
      both = median_ms(lambda: ren.render_instances(objs, Rs, ts, K, size=(w, h)), args.repeats)
      out = ren.render_instances(objs, Rs, ts, K, size=(w, h))
      vd, fd, cd = ren._upload()
      insts = torch.from_numpy(ren.instance_table(objs, Rs, ts, K).view(np.uint8)).cuda()
      s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
      keys = out['keys']
      raster = median_ms(lambda: lib.epos_render_raster(
          ptr(vd), ren._nv, ptr(fd), ren._nf, ptr(insts), n, h, w, ren.near, ptr(keys), s),
                         args.repeats)
      resolve = median_ms(lambda: lib.epos_render_resolve(
          ptr(keys), ptr(vd), ren._nv, ptr(fd), ren._nf, ptr(cd), ptr(insts), n, h, w, ren.near,
          ptr(out['depth']), ptr(out['face']), ptr(out['local_pos']), ptr(out['color']), s),
                          args.repeats)
      share = wavefront_share(verts, faces, Rs, ts, K, w, h, limit)
      covered = float((out['depth'] > 0).float().mean())
      line = ('%dx%d, %2d instances: render_instances %.3f ms (with the table upload); raster '
              '%.3f ms, resolve %.3f ms; covered %.1f %% of the pixels; box samples in '
              'wavefront-walked triangles %.1f %%' % (w, h, n, both, raster, resolve,
                                                      100 * covered, 100 * share))
      if (w, h) == (160, 120):
        for F in (64, 256):
          rng = np.random.RandomState(F)
          c, z = rng.uniform(-60, 60, (1, F, 3)), rng.uniform(5, 20, (1, F))
          ms = median_ms(lambda: render.gt_fields_device(out['depth'], out['local_pos'], objs,
                                                         c, z), args.repeats)
          line += '; gt_fields F=%d %.3f ms (with its uploads)' % (F, ms)
      else:
        rgb = np.zeros((h, w, 3), np.uint8)
        ps = [{'obj_id': 1, 'R': R, 't': t} for R, t in zip(Rs, ts)]
        splat = []
        for _ in range(4):                            # the first call is the warm-up
          t0 = time.perf_counter()
          vis.overlay_object_poses(rgb, K, ps, Store())
          splat.append(1e3 * (time.perf_counter() - t0))
        line += '; numpy splat of the same poses on the host %.1f ms (median of 3, warm)' % (
            float(np.median(splat[1:])))
        insts2 = torch.from_numpy(ren.instance_table([2] * n, Rs, ts, K).view(np.uint8)).cuda()
        plated = median_ms(lambda: lib.epos_render_raster(
            ptr(vd), ren._nv, ptr(fd), ren._nf, ptr(insts2), n, h, w, ren.near, ptr(keys), s),
                           args.repeats)
        line += ('; with the plate: raster %.3f ms, of it in wavefront-walked triangles %.1f %% '
                 '(box samples in them %.1f %%)' % (
                     plated, 100 * max(plated - raster, 0.0) / plated,
                     100 * wavefront_share(verts2, faces2, Rs, ts, K, w, h, limit)))
      print(line, flush=True)
      lines.append(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
