"""Times the pose-error stage (csrc/pose_error.hip) on the device, warm, with HIP events, next to
the plain numpy formulation of the same errors on the host.

    python tools/bench_pose_error.py [--pairs 3000] [--repeats 5] [--host_pairs 21]
        [--out profiles/r17/pose_error.txt]

A YCB-V-shaped load from a seed: 21 objects with 2,000 .. 12,000 vertices each; symmetry sets
as that dataset's models_info.json has them in kind -- most objects none (1 element), a few a
discrete one (2 or 4 elements), three a continuous one (315 elements, one of them 630 with a
discrete symmetry on top); --pairs (estimate, ground truth) pairs spread evenly over the
objects, the estimate a few degrees and millimetres off the ground truth.

  (a) epos_pose_errors_f64 with want_adi = 0 and (b) with want_adi = 1: the whole launch
      sequence of one call over all pairs (table upload from pinned memory, four kernels)
      between two HIP events; median of --repeats warm calls.
  (c) the host: the published formulas with numpy matrix products (R.dot(pts.T)), ADI by
      blocks of the all-pairs distance matrix, for --host_pairs pairs (one per object, in
      turn); a host clock. The total for all pairs is EXTRAPOLATED from their mean per object
      -- the full run with ADI would take many minutes -- and is named so.
Point-pair operations are counted from the shapes: sum of n_sym * n_verts (each a 3-D and a
2-D distance) for MSSD / MSPD, n_verts for ADD, n_verts^2 for ADI.
"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

O = 21
CAM = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]])


def load(seed, n_pairs):
  """(models, models_info, pairs) of the seeded load."""
  from epos_amd import pose_error as pe
  rng = np.random.RandomState(seed)
  models, info = {}, {}
  half_turn = np.eye(4)
  half_turn[:3, :3] = pe.axis_rotation(math.pi, [0, 0, 1])
  quarter = [np.eye(4) for _ in range(3)]
  for k in range(3):
    quarter[k][:3, :3] = pe.axis_rotation((k + 1) * math.pi / 2, [0, 0, 1])
  for o in range(1, O + 1):
    n = int(rng.randint(2000, 12001))
    models[o] = {'pts': rng.uniform(-1, 1, (n, 3)) * rng.uniform(30, 120, 3)}
    info[o] = {'diameter': 200.0}
    if o in (1, 13, 18):
      info[o]['symmetries_continuous'] = [{'axis': [0, 0, 1], 'offset': [0, 0, 0]}]
    if o in (16, 19, 20, 18):
      info[o]['symmetries_discrete'] = [half_turn.reshape(-1).tolist()]
    if o == 21:
      info[o]['symmetries_discrete'] = [q.reshape(-1).tolist() for q in quarter]
  pairs = []
  for i in range(n_pairs):
    R_g = pe.axis_rotation(rng.uniform(0, math.pi), rng.randn(3))
    t_g = np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(600, 1200)])
    pairs.append({'obj_id': 1 + i % O, 'R_g': R_g, 't_g': t_g, 'K': CAM,
                  'R_e': pe.axis_rotation(rng.uniform(0, 0.2), rng.randn(3)).dot(R_g),
                  't_e': t_g + rng.randn(3) * 5.0})
  return models, info, pairs


def host_errors(pts, syms, p, want_adi):
  """(mssd, mspd, add, adi) of one pair: the published formulas in plain numpy."""
  K = p['K']
  X = pts.T
  E = p['R_e'].dot(X) + p['t_e'].reshape(3, 1)
  uv = K.dot(E)
  uv = uv[:2] / uv[2:]
  mssd = mspd = np.inf
  for s in syms:
    G = p['R_g'].dot(s[:9].reshape(3, 3).dot(X) + s[9:].reshape(3, 1)) + p['t_g'].reshape(3, 1)
    mssd = min(mssd, np.linalg.norm(E - G, axis=0).max())
    pg = K.dot(G)
    mspd = min(mspd, np.linalg.norm(uv - pg[:2] / pg[2:], axis=0).max())
  G = p['R_g'].dot(X) + p['t_g'].reshape(3, 1)
  add = np.linalg.norm(E - G, axis=0).mean()
  adi = np.nan
  if want_adi:
    near = np.empty(X.shape[1])
    for v0 in range(0, X.shape[1], 256):
      d = E[:, :, None] - G[:, None, v0:v0 + 256]
      near[v0:v0 + 256] = np.sqrt((d * d).sum(axis=0).min(axis=0))
    adi = near.mean()
  return np.array([mssd, mspd, add, adi])


def main():
  import torch
  from epos_amd import pose_error as pe
  ap = argparse.ArgumentParser()
  ap.add_argument('--pairs', type=int, default=3000)
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--host_pairs', type=int, default=O)
  ap.add_argument('--seed', type=int, default=0)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  models, info, pairs = load(args.seed, args.pairs)
  ev = pe.PoseErrorEval(models, info, 'cuda:0')
  tab, finite = ev.table(pairs)
  assert finite.all()
  nv = tab['n_verts'].astype(np.float64)
  ns = tab['n_sym'].astype(np.float64)
  ops_ms, ops_add, ops_adi = float((nv * ns).sum()), float(nv.sum()), float((nv * nv).sum())
  lines = ['pose errors, %d pairs over %d objects (%d .. %d vertices, %d in the pool; symmetry '
           'sets of %s elements), seed %d' % (
               len(pairs), O, min(v[1] for v in ev.objects.values()),
               max(v[1] for v in ev.objects.values()), ev.n_verts_total,
               sorted(set(v[3] for v in ev.objects.values())), args.seed),
           'point-pair operations per call: MSSD/MSPD %.4g, ADD %.4g, ADI %.4g' % (
               ops_ms, ops_add, ops_adi)]
  print('\n'.join(lines), flush=True)
  host, dev, err = ev.staging(tab)
  results = {}
  for want_adi in (0, 1):
    ev.enqueue(host, dev, err, want_adi)                     # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      ev.enqueue(host, dev, err, want_adi)
      b.record()
      b.synchronize()
      times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    results[want_adi] = err.cpu().numpy().copy()
    ops = ops_ms + ops_add + (ops_adi if want_adi else 0.0)
    line = ('(%s) device, want_adi = %d: %.3f ms per call (median of %d warm calls, HIP events; '
            'min %.3f, max %.3f) = %.4g point-pair operations/s' % (
                'ab'[want_adi], want_adi, ms, args.repeats, min(times), max(times),
                ops / (ms * 1e-3)))
    print(line, flush=True)
    lines.append(line)
    results['ms%d' % want_adi] = ms
  adi_ms = results['ms1'] - results['ms0']
  if adi_ms > 0:
    lines.append('(b) - (a), the ADI kernel alone by difference: %.3f ms = %.4g point-pair '
                 'operations/s' % (adi_ms, ops_adi / (adi_ms * 1e-3)))
    print(lines[-1], flush=True)

  # the host on one pair per object in turn, checked against the device rows
  idx = list(range(min(args.host_pairs, len(pairs))))
  t_no = t_adi = 0.0
  worst = 0.0
  for i in idx:
    p = pairs[i]
    pts = models[p['obj_id']]['pts']
    syms = pe.symmetry_transformations(info[p['obj_id']])
    t0 = time.perf_counter()
    host_errors(pts, syms, p, False)
    t1 = time.perf_counter()
    h = host_errors(pts, syms, p, True)
    t2 = time.perf_counter()
    t_no += t1 - t0
    t_adi += t2 - t1
    worst = max(worst, float(np.max(np.abs(h - results[1][i]) / np.maximum(np.abs(h), 1e-300))))
  scale = len(pairs) / float(len(idx))
  line = ('(c) host numpy, %d pairs (one per object in turn): %.3f s without ADI, %.3f s with; '
          'EXTRAPOLATED to %d pairs: %.1f s without ADI, %.1f s with (not run in full); largest '
          'relative difference to the device rows %.2e' % (
              len(idx), t_no, t_adi, len(pairs), t_no * scale, t_adi * scale, worst))
  print(line, flush=True)
  lines.append(line)
  lines.append('extrapolated host time / device time: %.0f without ADI, %.0f with' % (
      t_no * scale / (results['ms0'] * 1e-3), t_adi * scale / (results['ms1'] * 1e-3)))
  print(lines[-1], flush=True)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
