"""Times the augmentation (csrc/augment.hip) on the device, warm, with HIP events, next to the
floor of one pass over the images, next to the same ops on the host, and inside a training step.

    python tools/bench_augment.py [--repeats 30] [--host_repeats 3]
                                  [--out profiles/r23/augment_bench.txt]

At B = 1 and B = 8 images of 640 x 480 with the seven-op chain in the reference's order
(brightness, contrast, saturation, hue, blur, noise, JPEG; tables drawn by augment.draw):
  (a) augment.apply_ops with a table drawn beforehand: the launches alone;
  (b) Augmenter.apply: the draw of the table on the host and the launches;
  (c) the yardstick: one device-to-device copy of the same buffer -- the floor of ONE pass;
      (a), (b) and (c) are timed INTERLEAVED, one call of each per round, each between its own
      two events; the medians of the rounds are reported, and per stage of (a) the time of a
      table that holds that stage's ops alone;
  (d) the host route: the same ops through numpy, scipy (the blur) and PIL (the round trip),
      one image per thread, 16 threads at most; wall clock, upload and download not counted;
  (e) B = 1: trainer.train_step with and without the augmenter, interleaved.
Before timing, one full-size image is validated against tests/helpers/augment_ref.py: the six
ops in front of the round trip to 2e-3 on [0,255], the levels entering the round trip as
tests/test_gpu_augment.py compares them, and the round trip alone by the share of equal levels
(a random image has rounding ties, where the order of a sum decides: the tests use tie-free
images and ask for equality).
"""
import argparse
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_eval import label_maps      # noqa: E402
from tests.helpers import augment_ref as R   # noqa: E402

H, W, O, F = 480, 640, 21, 64
IGNORE = 255
SPEC = {'random_adjust_brightness': {'min_delta': -0.2, 'max_delta': 0.2},
        'random_adjust_contrast': {'min_delta': 0.8, 'max_delta': 1.2},
        'random_adjust_saturation': {'min_delta': 0.8, 'max_delta': 1.2},
        'random_adjust_hue': {'max_delta': 0.02},
        'random_blur': {'max_sigma': 3.0},
        'random_gaussian_noise': {'max_sigma': 0.05},
        'jpeg_artifacts': {'min_quality': 80}}


def host_image(img, ops):
  """One image [h,w,3] float32 in [0,255] through ops on the host, in fp32 where the library
  allows it: what a numpy / scipy / PIL input pipeline would do."""
  from PIL import Image
  from scipy import ndimage
  x = img / np.float32(255)
  for op in ops:
    kind, a = int(op['kind']), np.float32(op['a'])
    if kind == R.BRIGHTNESS:
      x = np.clip(x + a, 0, 1)
    elif kind == R.CONTRAST:
      m = x.reshape(-1, 3).mean(0, dtype=np.float64).astype(np.float32)
      x = np.clip((x - m) * a + m, 0, 1)
    elif kind in (R.SATURATION, R.HUE):
      hsv = R.rgb_to_hsv(x)
      if kind == R.SATURATION:
        hsv[..., 1] = np.clip(hsv[..., 1] * a, 0, 1)
      else:
        hsv[..., 0] = np.mod(hsv[..., 0] + a, 1)
      x = np.clip(R.hsv_to_rgb(hsv), 0, 1).astype(np.float32)
    elif kind == R.BLUR:
      if R.blur_ksize(a) > 1 and a > 0:
        k = R.blur_weights(a).astype(np.float32)
        x = ndimage.correlate1d(ndimage.correlate1d(x, k, axis=1, mode='mirror'), k, axis=0,
                                mode='mirror')
    elif kind == R.NOISE:
      rng = np.random.Generator(np.random.Philox(key=[int(op['key_lo']), int(op['key_hi'])]))
      x = np.clip(x + a * rng.standard_normal(x.shape, dtype=np.float32), 0, 1)
    elif kind == R.JPEG:
      buf = io.BytesIO()
      Image.fromarray(np.minimum(np.floor(x * np.float32(255.5)), 255).astype(np.uint8)).save(
          buf, 'JPEG', quality=int(a))
      x = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB')).astype(
          np.float32) / np.float32(255)
  return x * np.float32(255)


def main():
  import torch
  from epos_amd import augment, net as enet, synthetic, trainer, weights
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=30)
  ap.add_argument('--host_repeats', type=int, default=3)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  torch.cuda.init()
  lines = ['augmentation, %dx%d, the seven-op chain (max blur sigma %.1f); (a)-(c), (e): medians '
           'of %d warm interleaved rounds (HIP events); (d): best of %d runs (wall clock)' % (
               W, H, SPEC['random_blur']['max_sigma'], args.repeats, args.host_repeats)]

  def say(line):
    print(line, flush=True)
    lines.append(line)

  def interleaved(fns):
    for fn in fns * 3:
      fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(args.repeats):
      for fn, ts in zip(fns, times):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return [float(np.median(ts)) for ts in times]

  aug = augment.Augmenter(SPEC, seed=0, device='cuda:0')
  frames = np.stack([synthetic.image(i, H, W).astype(np.float32) for i in range(8)])

  # ---- one full-size image against the helper, before anything is timed
  table = aug.ops(0, 1)
  x = torch.from_numpy(frames[:1]).cuda()
  augment.apply_ops(x, table[:, :6])
  dev = x.cpu().numpy()[0]
  before = []
  R.apply(frames[0], table[0], levels_before_jpeg=before)
  ref = R.apply(frames[0], table[0][:6])
  err = float(np.abs(dev - ref).max())
  assert err <= 2e-3, err
  near = np.abs(before[0] - np.rint(before[0])) <= 2e-3
  differ = R.to_levels(dev.astype(np.float64) / 255.0) != np.clip(np.floor(before[0]), 0, 255)
  assert not (differ & ~near).any()
  levels = np.rint(frames[0]).astype(np.int64)
  x = torch.from_numpy(levels[None].astype(np.float32)).cuda()
  q = int(table[0][6]['a'])
  jpeg_only = np.zeros((1, 1), augment.OP_DTYPE)
  jpeg_only[0, 0] = table[0][6]
  augment.apply_ops(x, jpeg_only)
  got = np.rint(x.cpu().numpy()[0]).astype(np.int64)
  want, ties = R.jpeg_round_trip(levels, q)
  same = float((got == want).mean())
  assert same >= 0.99 and np.abs(got - want).max() <= 8, (same, np.abs(got - want).max())
  say('validated at %dx%d: six ops in front of the round trip max |device - helper| = %.3g '
      '(bound 2e-3); %d of %d levels entering the round trip differ, all within 2e-3 of an '
      'integer; round trip alone at quality %d: %.4f %% of the levels equal the helper\'s, %d of '
      '%d MCUs of the helper hold a rounding tie' % (
          W, H, err, int(differ.sum()), differ.size, q, 100 * same, int((ties < 1e-6).sum()),
          ties.size))

  # ---- (a)-(d)
  stages = (('brightness', [0]), ('contrast + saturation + hue (sums, one pass)', [1, 2, 3]),
            ('blur', [4]), ('noise', [5]), ('jpeg', [6]))
  for B in (1, 8):
    imgs = torch.from_numpy(frames[:B]).cuda()
    buf, other = imgs.clone(), torch.empty_like(imgs)
    table = aug.ops(0, B)
    work = [None]

    def launches(t=table):
      work[0] = augment.apply_ops(buf, t, work[0])

    def whole():
      aug.apply(buf, 0)

    def floor():
      other.copy_(buf)

    # buf is augmented again and again: the cost of no stage depends on the values
    a_ms, b_ms, c_ms = interleaved((launches, whole, floor))
    nbytes = imgs.numel() * 4
    say('B=%d (%.1f MB): (a) apply_ops %.4f ms; (b) Augmenter.apply, draw included, %.4f ms; '
        '(c) device-to-device copy %.4f ms = %.0f GB/s read + written; (a) / (c) = %.1f; blur '
        'radii %s, qualities %s' % (
            B, nbytes / 1e6, a_ms, b_ms, c_ms, 2 * nbytes / c_ms / 1e6, a_ms / c_ms,
            [augment.blur_radius(s) for s in table['a'][:, 4]],
            [int(v) for v in table['a'][:, 6]]))
    parts = interleaved(tuple((lambda t=np.ascontiguousarray(table[:, cols]): launches(t))
                              for _, cols in stages))
    say('B=%d by stage, each alone on the [0,255] image: %s' % (
        B, '; '.join('%s %.4f ms' % (name, ms) for (name, _), ms in zip(stages, parts))))
    host_in = frames[:B]
    best = None
    with ThreadPoolExecutor(max_workers=min(16, B)) as pool:
      for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        list(pool.map(lambda b: host_image(host_in[b], table[b]), range(B)))
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    say('B=%d: (d) host route (numpy, scipy, PIL; %d threads) %.1f ms; (d) / (a) = %.0f' % (
        B, min(16, B), best, best / a_ms))
    del imgs, buf, other

  # ---- (e) inside a training step, B = 1
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  net = enet.EposNet(ckpt, 1, H, W, O, F, device='cuda:0')
  opt = trainer.Optimizer(ckpt, lr=1e-4)
  images = torch.from_numpy(synthetic.image(0, H, W)[None].astype(np.uint8)).cuda()
  gt_h, _ = label_maps(1, 1)
  gt_h[:, :6] = IGNORE
  gt = {'obj_label': torch.from_numpy(gt_h).cuda(),
        'frag_label': torch.randint(0, F, (1, H // 4, W // 4), dtype=torch.int32, device='cuda'),
        'frag_loc': torch.randn((1, H // 4, W // 4, 3), device='cuda'),
        'frag_weight': torch.ones((1, H // 4, W // 4), device='cuda')}

  def plain():
    trainer.train_step(net, images, gt, opt, 0.0)

  def augmented():
    trainer.train_step(net, images, gt, opt, 0.0, augment=aug, step=0)

  p_ms, s_ms = interleaved((plain, augmented))
  say('B=1, %dx%d: train_step %.4f ms; with the augmenter %.4f ms; augmentation adds %.4f ms '
      '(%.1f %% of the step)' % (W, H, p_ms, s_ms, s_ms - p_ms, 100.0 * (s_ms - p_ms) / p_ms))
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
