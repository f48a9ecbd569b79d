#!/usr/bin/env python
"""images/s of the end-to-end pipeline (network + correspondences + fitting) per backbone, one
JSON line each, driven the way bench.py drives the C2 line: batch 1, random-init weights with
randomised BatchNorm and logits calibrated on one frame, 4 pipelines in flight with 2 batches
queued per pipeline, a pool of 5 synthetic 640x480 frames resident in HBM, 5 target objects per
frame out of 21, hipGraph replay. bench.py --model-variant takes only xception_65 /
resnet_v1_101_beta; this tool takes every variant of epos_amd.weights.VARIANTS.

    python tools/bench_variants.py --variants xception_41,resnet_v1_50 --steps 20 --warmup 3
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epos_amd import model, pipeline, synthetic, weights   # noqa: E402


def measure(variant, args):
  B, H, W_, O, F = 1, args.height, args.width, args.num_objs, 64
  ckpt = weights.random_init(variant, num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), model_variant=variant)
  store = synthetic.ModelStore(O, F, seed=0)
  net0 = model.get_net(ckpt, 1, H, W_, O, F, mo)
  net0.forward(torch.from_numpy(synthetic.image(0, H, W_)[None]).cuda())
  torch.cuda.synchronize()
  synthetic.calibrate_logits(ckpt, net0.decoder_out[0].cpu().numpy())
  model._NETS.clear()
  del net0
  depth = 4
  pipes = [pipeline.EposPipeline(ckpt, B, H, W_, O, F, store, capacity=1 << 20,
                                 max_instances=1, instance=j, model_options=mo, queue=2)
           for j in range(depth)]
  pool = []
  for j in range(5):
    imgs = synthetic.image(j, H, W_)[None]
    tg = [{o: 1 for o in synthetic.targets(j, O, 5)}]
    pool.append((torch.from_numpy(imgs).cuda(), tg, [j]))
  Ks = synthetic.YCBV_K[None]
  for j in range(depth):                     # every plan captures its graph outside the timing
    imgs, tg, idx = pool[j]
    pipes[j].launch(imgs, Ks, tg, image_ids=idx, seed=0)
    pipes[j].collect()
  torch.cuda.synchronize()

  def run(first, count):
    inflight, n = [], 0
    for i in range(first, first + count):
      p = pipes[i % depth]
      if len(inflight) == depth * p.queue:
        n += len(inflight.pop(0).collect()[0])
      imgs, tg, idx = pool[i % 5]
      p.launch(imgs, Ks, tg, image_ids=idx, seed=i)
      inflight.append(p)
    while inflight:
      n += len(inflight.pop(0).collect()[0])
    return n
  run(0, args.warmup)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  poses = run(args.warmup, args.steps)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  out = {'metric': 'images/sec end-to-end (CNN+PnP-RANSAC), %dx%d' % (W_, H),
         'model_variant': variant, 'value': round(args.steps * B / dt, 3),
         'ms_per_step': round(dt / args.steps * 1e3, 3), 'steps': args.steps,
         'warmup': args.warmup, 'poses': poses, 'num_objs': O, 'num_frags': F,
         'plan_launches': len(pipes[0].net.ops)}
  del pipes
  model._NETS.clear()
  torch.cuda.empty_cache()
  return out


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--variants', default=','.join(sorted(weights.VARIANTS)))
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--height', type=int, default=480)
  ap.add_argument('--width', type=int, default=640)
  ap.add_argument('--num-objs', type=int, default=21)
  args = ap.parse_args(argv)
  for v in args.variants.split(','):
    weights.variant(v)
    print(json.dumps(measure(v, args)), flush=True)


if __name__ == '__main__':
  main()
