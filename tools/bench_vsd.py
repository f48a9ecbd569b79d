"""Times the VSD stage (csrc/vsd.hip, epos_amd/vsd.py) on the device, warm, with HIP events, next
to the vectorised numpy formulation of the same counts on the host.

    python tools/bench_vsd.py [--frames 200] [--per_frame 5] [--repeats 5] [--host_pairs 20]
        [--out profiles/r18/vsd.txt] [--bands 2,4,16]

A YCB-V-shaped load from a seed: 21 ellipsoidal meshes of 1 280 faces (semi-axes 25 .. 90 mm),
--frames images of 640 x 480 with the YCB-V camera, --per_frame ground-truth instances each at
0.6 .. 1.1 m, one estimate per ground truth up to 0.1 rad and a few millimetres off; the test
depth of a frame is the nearest ground-truth rendering over a wall at 1.5 m, plus three
clutter rectangles at 0.4 .. 0.9 m and 5 % of pixels without a measurement.

  (a) the render: render_instances(outputs=('depth',)) of every chunk, between two HIP events;
  (b) epos_vsd_counts of every chunk (table upload from pinned memory, counter clear, one
      kernel) with the host windows of vsd.window and (c) with full-image windows; per chunk
      the median of --repeats warm calls, summed over the chunks;
  (d) the whole VsdEval.errors call -- planning and tables on the host, uploads, renders,
      counts, one download -- on a host clock around a synchronised call;
  (e) the host: the same formulas in vectorised numpy over whole images, on renderings that
      have already been downloaded, for --host_pairs pairs; the total for all pairs is
      EXTRAPOLATED from their mean and is named so.
The kernel reads 12 bytes per window pixel and pair (three fp32 maps); the achieved rate is
those bytes over the time of (b) or (c), next to the 8 TB/s HBM3E peak of the MI355X data
sheet. Pixels that several pairs share come from the caches, so the rate is no HBM figure.

--bands: also time (b) and (c) with the kernel compiled for other numbers of workgroups per
pair (-DEPOS_VSD_BANDS=n; the default is what epos_vsd_row_bands() / 4 reports). Each variant
is a library of its own, built with --build_bands on a machine with hipcc and timed in a child
process; a variant whose library is missing is reported as not measured. A child that exits
with anything but 0 (or runs into its time limit) ends the whole run there: the lines gathered
so far are written to --out and nothing more is started on the device.
"""
import argparse
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_render import icosphere      # noqa: E402

O, W, H = 21, 640, 480
CAM = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]])
HBM_PEAK = 8.0e12


def variant_path(bands):
  from epos_amd import build
  return os.path.join(build.LIB_DIR, 'libepos_hip_vsdb%d.so' % bands)


def load(seed, n_frames, per_frame):
  """(models, models_info, frames [{gt: [(obj, R, t)], est: [(R, t)]}]) of the seeded load."""
  from epos_amd import pose_error as pe
  rng = np.random.RandomState(seed)
  unit, faces = icosphere(3, 1.0)
  models, info = {}, {}
  for o in range(1, O + 1):
    axes = rng.uniform(25, 90, 3)
    models[o] = {'pts': unit * axes, 'faces': faces}
    info[o] = {'diameter': 2.0 * float(axes.max())}
  frames = []
  for _ in range(n_frames):
    gt, est = [], []
    for _ in range(per_frame):
      R = pe.axis_rotation(rng.uniform(0, math.pi), rng.randn(3))
      t = np.array([rng.uniform(-200, 200), rng.uniform(-150, 150), rng.uniform(600, 1100)])
      gt.append((int(rng.randint(1, O + 1)), R, t))
      est.append((pe.axis_rotation(rng.uniform(0, 0.1), rng.randn(3)).dot(R),
                  t + rng.randn(3) * 5.0))
    frames.append({'gt': gt, 'est': est})
  return models, info, frames


def test_depth(ev, frames, seed):
  """The test depth images f32 [n,H,W]: nearest ground-truth rendering, wall, clutter, holes."""
  import torch
  rng = np.random.RandomState(seed + 1)
  out = np.empty((len(frames), H, W), np.float32)
  for i, fr in enumerate(frames):
    d = ev.renderer.render_instances(
        [o for o, _, _ in fr['gt']], np.stack([R for _, R, _ in fr['gt']]),
        np.stack([t for _, _, t in fr['gt']]), CAM, size=(W, H), outputs=('depth',))['depth']
    d = torch.where(d > 0, d, torch.full_like(d, 1500.0)).min(dim=0).values.cpu().numpy()
    for _ in range(3):
      x, y = rng.randint(0, W - 80), rng.randint(0, H - 80)
      d[y:y + rng.randint(20, 80), x:x + rng.randint(20, 80)] = rng.uniform(400, 900)
    d[rng.rand(H, W) < 0.05] = 0.0
    out[i] = d
  return out


def host_counts(depth, dg, de, K, delta, taus, diameter):
  """The counts of one pair over the whole image, vectorised numpy."""
  xs, ys = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
  s = np.sqrt(((xs - K[0, 2]) / K[0, 0]) ** 2 + ((ys - K[1, 2]) / K[1, 1]) ** 2 + 1.0)
  dt, dg, de = depth * s, dg * s, de * s
  missing, mg, me = ~(depth > 0), dg > 0, de > 0
  vg = mg & (missing | (dg - dt <= delta))
  ve = me & (missing | (de - dt <= delta) | vg)
  inter = vg & ve
  d = np.abs(dg - de)[inter] / diameter
  return np.array([mg.sum(), vg.sum(), me.sum(), ve.sum(), inter.sum(), (vg | ve).sum()] +
                  [(d >= t).sum() for t in taus], np.int64)


def median_ms(fn, repeats):
  import torch
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


def kernel_times(ev, fdepth, pairs, repeats):
  """(render ms, counts ms with host windows, with full windows, window bytes, full bytes,
  counts of the host-window calls), summed over the chunks."""
  import torch
  from epos_amd import vsd
  chunks, _ = ev.plan(fdepth, pairs)
  n_c = vsd.N_FIXED + len(vsd.VSD_TAUS)
  t_render = t_win = t_full = 0.0
  b_win = b_full = 0
  rows = []
  for chunk in chunks:
    keep = ev.upload_depth(fdepth, chunk)
    t_render += median_ms(lambda: ev.render(chunk), repeats)
    model = ev.render(chunk)
    for full in (False, True):
      tab = ev.table(chunk, full_windows=full)
      counts = torch.empty((len(tab), n_c), dtype=torch.int64, device=ev.device)
      held = []
      ms = median_ms(lambda: held.append(ev.enqueue_counts(
          keep[1], model, tab, vsd.VSD_DELTA, vsd.VSD_TAUS, counts)), repeats)
      area = int(((tab['x1'] - tab['x0']).astype(np.int64) *
                  (tab['y1'] - tab['y0']).astype(np.int64)).sum())
      if full:
        t_full, b_full = t_full + ms, b_full + 12 * area
        assert (counts.cpu().numpy() == rows[-1]).all(), 'full and host windows disagree'
      else:
        t_win, b_win = t_win + ms, b_win + 12 * area
        rows.append(counts.cpu().numpy())
      del held
  return t_render, t_win, t_full, b_win, b_full, len(chunks), np.concatenate(rows)


def rate_line(tag, what, ms, nbytes, n_pairs, repeats):
  return ('(%s) epos_vsd_counts, %s: %.3f ms for all chunks (per chunk the median of %d warm '
          'calls, HIP events); %.0f bytes read per pair on average (window area x 12 B), '
          '%.1f GB/s = %.1f %% of the 8 TB/s HBM peak' % (
              tag, what, ms, repeats, nbytes / float(n_pairs), nbytes / (ms * 1e-3) / 1e9,
              100.0 * nbytes / (ms * 1e-3) / HBM_PEAK))


def write_report(path, lines):
  if path:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--frames', type=int, default=200)
  ap.add_argument('--per_frame', type=int, default=5)
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--host_pairs', type=int, default=20)
  ap.add_argument('--seed', type=int, default=0)
  ap.add_argument('--bands', default='')
  ap.add_argument('--build_bands', default='',
                  help='build the libraries of these variants (needs hipcc, no device) and exit')
  ap.add_argument('--kernel_only', action='store_true',
                  help='print the (b) and (c) lines only (the child process of --bands)')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  if args.build_bands:
    from epos_amd import build
    for b in args.build_bands.split(','):
      print(build.build_variant('vsdb%d' % int(b), ['-DEPOS_VSD_BANDS=%d' % int(b)],
                                only=['vsd.hip']))
    return
  import torch
  from epos_amd import _lib, vsd
  models, info, frames = load(args.seed, args.frames, args.per_frame)
  ev = vsd.VsdEval(models, info, 'cuda:0')
  depth = test_depth(ev, frames, args.seed)
  fdepth = [(depth[i], CAM) for i in range(len(frames))]
  pairs = [{'frame': i, 'obj_id': o, 'R_g': R, 't_g': t, 'R_e': Re, 't_e': te}
           for i, fr in enumerate(frames) for (o, R, t), (Re, te) in zip(fr['gt'], fr['est'])]
  bands = _lib.load().epos_vsd_row_bands() // 4
  t_render, t_win, t_full, b_win, b_full, n_chunks, dev_rows = kernel_times(
      ev, fdepth, pairs, args.repeats)
  kernel_lines = [
      rate_line('b', 'host windows, %d workgroups per pair' % bands, t_win, b_win, len(pairs),
                args.repeats),
      rate_line('c', 'full-image windows, %d workgroups per pair' % bands, t_full, b_full,
                len(pairs), args.repeats)]
  if args.kernel_only:
    print('\n'.join(kernel_lines), flush=True)
    return
  lines = ['VSD, %d frames of %d x %d, %d (ground truth, estimate) pairs over %d objects of %d '
           'faces, %d instances rendered in %d chunk(s), seed %d' % (
               len(frames), W, H, len(pairs), O, len(models[1]['faces']), 2 * len(pairs),
               n_chunks, args.seed),
           '(a) render_instances(depth) of every chunk: %.3f ms (per chunk the median of %d '
           'warm calls, HIP events) = %.1f us per instance' % (
               t_render, args.repeats, 1e3 * t_render / (2 * len(pairs)))] + kernel_lines
  print('\n'.join(lines), flush=True)
  for b in [int(x) for x in args.bands.split(',') if x]:
    lib = variant_path(b)
    if not os.path.exists(lib):
      lines.append('%d workgroups per pair: not measured (no library at %s)' % (
          b, os.path.relpath(lib, ROOT)))
    else:
      out = subprocess.run(
          [sys.executable, os.path.abspath(__file__), '--kernel_only', '--frames',
           str(args.frames), '--per_frame', str(args.per_frame), '--repeats', str(args.repeats),
           '--seed', str(args.seed)], env=dict(os.environ, EPOS_HIP_LIB=lib),
          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
      if out.returncode != 0:
        # whatever ended the child, nothing more is started on the device: the lines gathered
        # so far are written and the run ends here
        lines.append('%d workgroups per pair: the run failed (exit %d); stopped here' % (
            b, out.returncode))
        write_report(args.out, lines)
        raise SystemExit('bench_vsd: the %d-workgroup variant exited with %d; nothing further '
                         'was run on the device. Its output:\n%s' % (
                             b, out.returncode, out.stdout))
      lines += [ln for ln in out.stdout.split('\n') if ln.startswith('(')]   # its (b), (c)
    print(lines[-1], flush=True)

  torch.cuda.synchronize()
  ev.errors(fdepth, pairs)                                   # warm
  t0 = time.perf_counter()
  got_vsd, _ = ev.errors(fdepth, pairs)
  t_all = time.perf_counter() - t0
  assert (got_vsd == vsd.vsd_from_counts(dev_rows)).all()
  lines.append('(d) VsdEval.errors, the whole call (planning and tables on the host, %d depth '
               'uploads, renders, counts, one download): %.1f ms on a host clock, one warm '
               'call' % (len(frames), 1e3 * t_all))
  print(lines[-1], flush=True)

  idx = list(range(0, len(pairs), max(1, len(pairs) // max(1, args.host_pairs))))[:args.host_pairs]
  t_host, same = 0.0, True
  for i in idx:
    p = pairs[i]
    both = ev.renderer.render_instances(
        [p['obj_id']] * 2, np.stack([p['R_g'], p['R_e']]), np.stack([p['t_g'], p['t_e']]), CAM,
        size=(W, H), outputs=('depth',))['depth'].cpu().numpy().astype(np.float64)
    d64 = depth[p['frame']].astype(np.float64)
    t0 = time.perf_counter()
    row = host_counts(d64, both[0], both[1], CAM, vsd.VSD_DELTA, vsd.VSD_TAUS,
                      info[p['obj_id']]['diameter'])
    t_host += time.perf_counter() - t0
    same = same and (row == dev_rows[i]).all()
  scale = len(pairs) / float(len(idx))
  lines.append('(e) host numpy over whole images, %d pairs on downloaded renderings: %.3f s; '
               'EXTRAPOLATED to %d pairs: %.1f s (not run in full; the renders and downloads '
               'are not in it); counts equal to the device rows: %s' % (
                   len(idx), t_host, len(pairs), t_host * scale, same))
  lines.append('extrapolated host time / (a) + (b): %.0f' % (
      t_host * scale / ((t_render + t_win) * 1e-3)))
  print('\n'.join(lines[-2:]), flush=True)
  write_report(args.out, lines)


if __name__ == '__main__':
  main()
