#!/usr/bin/env python
"""project_to_surface on the device: the indexed mesh query against the exhaustive sweep, and
the fused route of infer.py against the operator route ("Mesh index"). One JSON
line per measurement.

    python tools/bench_surface.py kernel [--subdiv 4,6,7] [--rows 20000] [--rounds 5]
        per-launch time of epos_project_rows_to_mesh_f64 and epos_project_to_mesh_f64 on the
        same rows, alternating, for noisy icospheres of 20 * 4^subdiv faces (4: 5120,
        6: 81920, 7: 327680); rows scattered around the surface.
    python tools/bench_surface.py infer [--frames 60] [--rounds 3] [--subdiv 5]
        images/s of `infer.py --synthetic` (C2 shape: 640x480, 21 objects), alternating: plain,
        --project_to_surface true (operator route) and the same with --surface_on_device true;
        meshes are ellipsoids of 20 * 4^subdiv faces written under a temporary BOP_PATH.
        (Random-init heads of a synthetic frame yield no correspondences: this compares the
        routes' structure, the stage itself has no rows to project there.)
    python tools/bench_surface.py pipeline [--steps 60] [--rounds 2] [--subdiv 5]
        images/s and the correspondence stage's time of EposPipeline at the C2 shape with
        planted scenes (synthetic.planted_scene: tens of thousands of rows per image), built
        without and with project_to_surface, alternating in one process.
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def icosphere(subdiv, radii=(1.0, 1.0, 1.0), noise=0.0, seed=0):
  t = (1.0 + 5.0 ** 0.5) / 2.0
  v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t),
                (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)], float)
  v /= np.linalg.norm(v, axis=1, keepdims=True)
  f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9),
                (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6),
                (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)])
  for _ in range(subdiv):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    uniq, inv = np.unique(e, axis=0, return_inverse=True)
    mid = v[uniq[:, 0]] + v[uniq[:, 1]]
    mid /= np.linalg.norm(mid, axis=1, keepdims=True)
    ab, bc, ca = inv.reshape(3, -1) + len(v)
    v = np.concatenate([v, mid])
    f = np.concatenate([np.stack([f[:, 0], ab, ca], 1), np.stack([f[:, 1], bc, ab], 1),
                        np.stack([f[:, 2], ca, bc], 1), np.stack([ab, bc, ca], 1)])
  if noise:
    edge = np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean()
    v = v * (1.0 + noise * edge * np.random.RandomState(seed).standard_normal((len(v), 1)))
  return v * np.asarray(radii, float), f.astype(np.int32)


def bench_kernel(args):
  import torch
  from epos_amd import _lib, mesh_index
  lib = _lib.load()
  ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  rng = np.random.RandomState(1)
  d = rng.standard_normal((args.rows, 3))
  d /= np.linalg.norm(d, axis=1, keepdims=True)
  rows = d * 50.0 * (1.0 + 0.05 * rng.standard_normal((args.rows, 1)))
  rows0 = torch.from_numpy(rows).cuda()
  base = torch.tensor([0, args.rows], dtype=torch.int64).cuda()
  slots = torch.tensor([[0, 1]], dtype=torch.int32).cuda()
  for subdiv in [int(s) for s in args.subdiv.split(',')]:
    verts, faces = icosphere(subdiv, (50.0, 50.0, 50.0), noise=0.2)
    t0 = time.perf_counter()
    table = mesh_index.MeshTable({1: {'pts': verts, 'faces': faces}}, 1, 'cuda:0')
    build_s = time.perf_counter() - t0
    ix = table.index[1]
    V = torch.from_numpy(verts).cuda()
    Fc = torch.from_numpy(faces).cuda()
    buf = rows0.clone()
    out = torch.empty_like(rows0)
    fa = torch.empty(args.rows, dtype=torch.int32).cuda()
    fb = torch.empty(args.rows, dtype=torch.int32).cuda()
    vis = torch.empty(args.rows, dtype=torch.int32).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def tree():
      buf.copy_(rows0)
      ev[0].record()
      _lib.check(lib.epos_project_rows_to_mesh_f64(
          ptr(buf), ptr(base), ptr(slots), 1, args.rows, ptr(table.recs_dev), 1,
          ptr(table.geom_dev), ptr(table.fid_dev), ptr(fa), ptr(vis), stream), 'tree')
      ev[1].record()
      torch.cuda.synchronize()
      return ev[0].elapsed_time(ev[1])

    def sweep():
      ev[0].record()
      _lib.check(lib.epos_project_to_mesh_f64(
          ptr(rows0), args.rows, ptr(V), len(verts), ptr(Fc), len(faces), ptr(out), ptr(fb),
          stream), 'sweep')
      ev[1].record()
      torch.cuda.synchronize()
      return ev[0].elapsed_time(ev[1])
    tree(); sweep()                                   # warm-up
    times = {'tree': [], 'sweep': []}
    for _ in range(args.rounds):
      times['tree'].append(tree())
      times['sweep'].append(sweep())
    same = bool(torch.equal(buf, out) and torch.equal(fa, fb))
    print(json.dumps({
        'measure': 'kernel', 'faces': len(faces), 'rows': args.rows, 'leaves': ix['nleaf'],
        'always_faces': int(len(ix['always'])), 'levels': ix['top'] + 1,
        'index_build_s': round(build_s, 3), 'index_mb': round(table.geom.nbytes / 1e6, 2),
        'mean_blocks_swept': round(float(vis.float().mean()), 2),
        'tree_ms': [round(t, 3) for t in times['tree']],
        'sweep_ms': [round(t, 3) for t in times['sweep']],
        'tree_ms_median': round(float(np.median(times['tree'])), 3),
        'sweep_ms_median': round(float(np.median(times['sweep'])), 3),
        'bit_equal': same}), flush=True)


def bench_infer(args):
  from epos_amd import ply, synthetic
  work = tempfile.mkdtemp(prefix='bench_surface_')
  store = synthetic.ModelStore(args.num_objs, 64, seed=0)
  os.makedirs(os.path.join(work, 'bop', 'ycbv', 'models_eval'))
  for o in store.dp_model['obj_ids']:
    v, f = icosphere(args.subdiv, store.radii[o])
    ply.save_ply(ply.model_path(os.path.join(work, 'bop'), 'ycbv', o, 'eval'), v, f)
  routes = {'plain': [],
            'operator': ['--dataset', 'ycbv', '--project_to_surface', 'true'],
            'on_device': ['--dataset', 'ycbv', '--project_to_surface', 'true',
                          '--surface_on_device', 'true']}
  for r in range(args.rounds):
    for name, extra in routes.items():
      d = os.path.join(work, '%s_%d' % (name, r))
      os.makedirs(os.path.join(d, 'c2'))
      out = subprocess.run(
          [sys.executable, os.path.join(ROOT, 'infer.py'), '--model=c2', '--synthetic',
           str(args.frames), '--num_objs', str(args.num_objs)] + extra,
          env=dict(os.environ, TF_MODELS_PATH=d, BOP_PATH=os.path.join(work, 'bop')),
          capture_output=True, text=True)
      if out.returncode:
        raise SystemExit(out.stdout[-2000:] + out.stderr[-2000:])
      m = re.search(r'inference loop ([0-9.]+) s = ([0-9.]+) images/s', out.stdout)
      plan = [l for l in out.stdout.split('\n') if 'step(s) in flight' in l][0]
      saved = re.search(r'Saved (\d+) pose estimates', out.stdout)
      print(json.dumps({'measure': 'infer', 'route': name, 'round': r, 'frames': args.frames,
                        'mesh_faces': 20 * 4 ** args.subdiv,
                        'images_per_s': float(m.group(2)), 'loop_s': float(m.group(1)),
                        'poses': int(saved.group(1)) if saved else None, 'plan': plan}),
            flush=True)


def bench_pipeline(args):
  import torch
  from epos_amd import _lib, model, pipeline, synthetic, weights
  lib = _lib.load()
  H, W_, O, F, depth = 480, 640, args.num_objs, 64, 4
  ckpt = weights.random_init(num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F))
  store = synthetic.ModelStore(O, F, seed=0)
  store.models = {}
  for o in store.dp_model['obj_ids']:
    v, f = icosphere(args.subdiv, store.radii[o])
    store.models[o] = {'pts': v, 'faces': f}
  built = {}
  for name, flag in (('plain', False), ('project_to_surface', True)):
    built[name] = [pipeline.EposPipeline(ckpt, 1, H, W_, O, F, store, capacity=1 << 20,
                                         max_instances=1, instance=j, model_options=mo, queue=2,
                                         project_to_surface=flag) for j in range(depth)]
  net = built['plain'][0].net
  pool = []
  for j in range(5):
    tg = [{o: 1 for o in synthetic.targets(j, O, 5)}]
    sc = synthetic.planted_scene(j, store, tg[0], synthetic.YCBV_K, net.out_h, net.out_w, O, F,
                                 outlier_frac=0.5, image_in_batch=0)
    dv = {}
    for key in ('obj', 'frag', 'loc'):
      off, val = sc[key][0], sc[key][1].reshape(len(sc[key][0]), -1)
      dv[key] = (torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(val)).cuda(),
                 int(val.shape[1]))
    pool.append((torch.from_numpy(synthetic.image(j, H, W_)[None]).cuda(), tg, [j], dv))

  def planter(dv):
    def plant(p):
      st = ctypes.c_void_p(p.stream.cuda_stream)
      for key, name in (('obj', weights.PRED_OBJ_CONF), ('frag', weights.PRED_FRAG_CONF),
                        ('loc', weights.PRED_FRAG_LOC)):
        off, val, width = dv[key]
        _lib.check(lib.epos_scatter_blocks_f32(
            ctypes.c_void_p(p.net.logits[name].data_ptr()), ctypes.c_void_p(off.data_ptr()),
            ctypes.c_void_p(val.data_ptr()), off.numel(), width, st), 'scatter_blocks')
    return plant
  Ks = synthetic.YCBV_K[None]

  def run(pipes, first, count, timing):
    inflight, n, corr_s, rows = [], 0, [], []

    def take(p):
      poses, rt = p.collect()
      if rt:
        corr_s.append(rt['establish_corr'])
      rows.append(int(p.last_totals[:, 1].sum()))
      return len(poses)
    for i in range(first, first + count):
      p = pipes[i % depth]
      if len(inflight) == depth * p.queue:
        n += take(inflight.pop(0))
      imgs, tg, idx, dv = pool[i % 5]
      p.launch(imgs, Ks, tg, image_ids=idx, seed=i, timing=timing, after_net=planter(dv))
      inflight.append(p)
    while inflight:
      n += take(inflight.pop(0))
    return n, corr_s, rows
  for r in range(args.rounds):
    for name, pipes in built.items():
      run(pipes, 0, 8, False)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      poses, _, rows = run(pipes, 8, args.steps, False)
      torch.cuda.synchronize()
      dt = time.perf_counter() - t0
      _, corr_s, _ = run(pipes, 8, 20, True)          # stage times from a run of their own
      print(json.dumps({'measure': 'pipeline', 'pipeline': name, 'round': r,
                        'mesh_faces': 20 * 4 ** args.subdiv, 'steps': args.steps,
                        'images_per_s': round(args.steps / dt, 1), 'poses': poses,
                        'rows_per_image': int(np.mean(rows)),
                        'establish_corr_ms': round(float(np.mean(corr_s)) * 1e3, 3)}),
            flush=True)


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('mode', choices=['kernel', 'infer', 'pipeline'])
  ap.add_argument('--subdiv', default=None)
  ap.add_argument('--rows', type=int, default=20000)
  ap.add_argument('--rounds', type=int, default=None)
  ap.add_argument('--frames', type=int, default=60)
  ap.add_argument('--steps', type=int, default=60)
  ap.add_argument('--num-objs', type=int, default=21)
  args = ap.parse_args(argv)
  if args.mode == 'kernel':
    args.subdiv = args.subdiv or '4,6,7'
    args.rounds = args.rounds or 5
    bench_kernel(args)
  elif args.mode == 'infer':
    args.subdiv = int(args.subdiv or 5)
    args.rounds = args.rounds or 3
    bench_infer(args)
  else:
    args.subdiv = int(args.subdiv or 5)
    args.rounds = args.rounds or 2
    bench_pipeline(args)


if __name__ == '__main__':
  main()
