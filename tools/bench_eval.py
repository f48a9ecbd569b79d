"""Times the evaluation reductions (csrc/eval.hip) on the device, warm, with HIP events, next to
the host route the reference takes, and eval.py end to end.

    python tools/bench_eval.py [--repeats 50] [--frames 64] [--out profiles/r16/eval_bench.txt]

At B = 1 and B = 8 images of 640 x 480 (label maps of 120 x 160), 21 objects, 64 fragments:
  (a) epos_eval_confusion on the two label maps;
  (b) epos_eval_frag_hits on the label maps and the dense [P, 21, 64] confidences;
  (c) the reference's route (eval_utils.py:56-70): download both label maps, mask the ignored
      pixels, np.unique over the stacked label pairs, add the counts into the matrix.
(a) and (b) are medians of single launches between two events; (c) is a host clock around
download + numpy, which ends synchronised by the download itself. A quarter of the pixels is
foreground, in blobs of one object, as a frame with a handful of objects has them.

End to end: eval.py as a child process on --frames of 640 x 480 noise images with five
ground-truth poses each (icosphere meshes under a temporary $BOP_PATH, random weights), at
--batch_size 1 and 8; the images/s of its closing line (forward pass, rendered ground-truth
maps and both reductions per batch; set-up excluded).
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

H, W, O, F = 120, 160, 21, 64


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


def label_maps(B, seed):
  """gt i32 [B,H,W] with blobs of objects over a quarter of the image, pred i64 [B,H,W] that
  agrees with it on most pixels."""
  rng = np.random.RandomState(seed)
  gt = np.zeros((B, H, W), np.int32)
  yy, xx = np.mgrid[:H, :W]
  for b in range(B):
    for _ in range(5):
      cy, cx, r = rng.randint(H), rng.randint(W), rng.randint(15, 30)
      gt[b][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = rng.randint(1, O + 1)
  pred = gt.astype(np.int64)
  flip = rng.rand(B, H, W) < 0.2
  pred[flip] = rng.randint(0, O + 1, int(flip.sum()))
  return gt, pred


def host_route(gt_dev, pred_dev, cm):
  """Counting on the host, image by image, on downloaded maps: the label pairs of the pixels
  that are not ignored, their distinct rows and multiplicities, added into cm."""
  gt, pred = gt_dev.cpu().numpy(), pred_dev.cpu().numpy()
  for b in range(gt.shape[0]):
    keep = gt[b] != 255
    pairs = np.column_stack((gt[b][keep], pred[b][keep]))
    cells, n = np.unique(pairs, axis=0, return_counts=True)
    np.add.at(cm, (cells[:, 0], cells[:, 1]), n)


def write_scene(root, n_frames):
  """A temporary $BOP_PATH with 21 'ycbv' meshes and a --frames directory."""
  from epos_amd import ply, synthetic
  from tools.bench_render import icosphere, poses
  bop = os.path.join(root, 'bop')
  os.makedirs(os.path.join(bop, 'ycbv', 'models_eval'))
  for o in range(1, O + 1):
    v, f = icosphere(3, 40.0 + o)
    ply.save_ply(ply.model_path(bop, 'ycbv', o, 'eval'), v, f)
  fdir = os.path.join(root, 'frames')
  os.makedirs(fdir)
  meta = []
  rng = np.random.RandomState(0)
  K = synthetic.YCBV_K
  for i in range(n_frames):
    np.save(os.path.join(fdir, '%d.npy' % i), synthetic.image(i, 480, 640).astype(np.uint8))
    Rs, ts = poses(5, seed=i)
    ids = rng.choice(np.arange(1, O + 1), 5, replace=False)
    meta.append({'path': '%d.npy' % i, 'im_id': i, 'scene_id': 1, 'K': K.reshape(-1).tolist(),
                 'targets': {str(int(o)): 1 for o in ids},
                 'gt_poses': [{'obj_id': int(o), 'R': R.reshape(-1).tolist(), 't': list(t)}
                              for o, R, t in zip(ids, Rs, ts)]})
  with open(os.path.join(fdir, 'frames.json'), 'w') as f:
    json.dump(meta, f)
  return bop, fdir


def end_to_end(n_frames, lines):
  with tempfile.TemporaryDirectory() as root:
    bop, fdir = write_scene(root, n_frames)
    for B in (1, 8):
      models = os.path.join(root, 'models_b%d' % B)
      os.makedirs(os.path.join(models, 'bench'))
      t0 = time.time()
      out = subprocess.run(
          ['timeout', '-k', '10', '400', sys.executable, os.path.join(ROOT, 'eval.py'),
           '--model=bench', '--synthetic', str(n_frames), '--frames', fdir, '--dataset', 'ycbv',
           '--num_objs', str(O), '--batch_size', str(B)],
          env=dict(os.environ, TF_MODELS_PATH=models, BOP_PATH=bop), capture_output=True,
          text=True)
      if out.returncode != 0:
        raise RuntimeError('eval.py failed (%d):\n%s' % (out.returncode, out.stdout + out.stderr))
      closing = [ln for ln in out.stdout.split('\n') if ln.startswith('eval: ')][0]
      rate = float(re.search(r'([0-9.]+) images/s', closing).group(1))
      line = ('eval.py end to end, %d frames of 640x480 with 5 ground-truth poses each, '
              '--batch_size %d: %.1f images/s in the evaluation loop (process %.1f s with '
              'set-up); %s' % (n_frames, B, rate, time.time() - t0, closing))
      print(line, flush=True)
      lines.append(line)


def main():
  import torch
  from epos_amd import _lib
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=50)
  ap.add_argument('--frames', type=int, default=64, help='frames of the end-to-end run (0: skip)')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  lib = _lib.load()
  lines = ['evaluation reductions, %dx%d maps, %d objects, %d fragments; (a), (b): median of %d '
           'warm launches (HIP events); (c): median of %d host-clock runs' % (
               W, H, O, F, args.repeats, args.repeats)]

  def ptr(t):
    return ctypes.c_void_p(t.data_ptr())
  s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  for B in (1, 8):
    gt_h, pred_h = label_maps(B, B)
    gt, pred = torch.from_numpy(gt_h).cuda(), torch.from_numpy(pred_h).cuda()
    gt_frag = torch.randint(0, F, (B, H, W), dtype=torch.int32, device='cuda')
    conf = torch.rand((B, H, W, O, F), device='cuda')
    cm = torch.zeros((O + 1, O + 1), dtype=torch.int64, device='cuda')
    bad = torch.zeros((1,), dtype=torch.int64, device='cuda')
    counts = torch.zeros((O + 1, 3), dtype=torch.int64, device='cuda')
    P = B * H * W

    def confusion():
      _lib.check(lib.epos_eval_confusion(ptr(gt), ptr(pred), P, O + 1, 255, ptr(cm), ptr(bad),
                                         s))

    def frag_hits():
      _lib.check(lib.epos_eval_frag_hits(ptr(gt), ptr(gt_frag), ptr(pred), ptr(conf), P, O, F,
                                         255, ptr(counts), s))
    a_ms = median_ms(confusion, args.repeats)
    b_ms = median_ms(frag_hits, args.repeats)
    # the device table against the host route on the same maps, before timing the latter
    cm.zero_()
    confusion()
    cm_host = np.zeros((O + 1, O + 1), np.int64)
    host_route(gt, pred, cm_host)
    assert np.array_equal(cm.cpu().numpy(), cm_host) and int(bad.cpu()[0]) == 0
    host = []
    for _ in range(args.repeats + 3):
      t0 = time.perf_counter()
      host_route(gt, pred, cm_host)
      host.append(1e3 * (time.perf_counter() - t0))
    c_ms = float(np.median(host[3:]))
    fg = float((gt_h > 0).mean())
    line = ('B=%d (%d pixels, %.0f %% foreground): (a) epos_eval_confusion %.4f ms; (b) '
            'epos_eval_frag_hits %.4f ms; (c) download + np.unique on the host %.3f ms; '
            '(c) / ((a) + (b)) = %.1f, (c) / (a) = %.1f' % (
                B, P, 100 * fg, a_ms, b_ms, c_ms, c_ms / (a_ms + b_ms), c_ms / a_ms))
    print(line, flush=True)
    lines.append(line)
  if args.frames:
    end_to_end(args.frames, lines)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
