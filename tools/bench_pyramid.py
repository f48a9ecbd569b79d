#!/usr/bin/env python
"""images/s of the end-to-end pipeline per image pyramid (multi-scale inference, max merge;
DESIGN.md, "multi-scale mode"), one JSON line per run, driven as tools/bench_precision.py drives
it (C2: Xception-65, batch 1, random-init weights with randomised BatchNorm and logits
calibrated on one frame, `--depth` pipelines in flight with 2 batches queued each, 5 resident
640x480 frames, 5 targets of 21 objects, hipGraph replay). Every pyramid's pipelines are built
once; the pyramids then alternate in one process, `--rounds` times each, so that all see the
same clocks. mem_gb_per_pipeline: device memory one pipeline (its plans + buffers) holds.

    python tools/bench_pyramid.py --pyramids "1.0;0.75,1.0,1.25;0.5,0.75,1.0,1.25,1.5,1.75"
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epos_amd import model, pipeline, synthetic, weights   # noqa: E402

CONFIG = {'xception_65': 'C2', 'resnet_v1_101_beta': 'C5'}


def build(pyr, ckpt, store, mo, args):
  B, H, W_, O, F = 1, args.height, args.width, args.num_objs, 64
  torch.cuda.synchronize()
  m0 = torch.cuda.memory_allocated()
  pipes = [pipeline.EposPipeline(ckpt, B, H, W_, O, F, store, capacity=1 << 20,
                                 max_instances=1, instance=j, model_options=mo, queue=2,
                                 image_pyramid=pyr, merge_method='max')
           for j in range(args.depth)]
  torch.cuda.synchronize()
  return pipes, (torch.cuda.memory_allocated() - m0) / args.depth


def measure(pyr, pipes, mem, pool, args):
  depth = len(pipes)
  Ks = synthetic.YCBV_K[None]
  for j in range(depth):
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
  net = pipes[0].net
  return {'metric': 'images/sec end-to-end (CNN+PnP-RANSAC), %dx%d' % (args.width, args.height),
          'config': 'C2', 'image_pyramid': pyr, 'merge_method': 'max',
          'merged_hw': [net.out_h, net.out_w], 'value': round(args.steps / dt, 3),
          'ms_per_step': round(dt / args.steps * 1e3, 3), 'steps': args.steps,
          'warmup': args.warmup, 'depth': depth, 'poses': poses,
          'tflop_per_image': round(net.flops / 1e12, 4),
          'algorithmic_gb': round(net.algorithmic_bytes() / 1e9, 3),
          'merge_gb': round(getattr(net, 'merge_bytes', 0) / 1e9, 3),
          'mem_gb_per_pipeline': round(mem / 1e9, 3)}


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--pyramids', default='1.0;0.75,1.0,1.25;0.5,0.75,1.0,1.25,1.5,1.75')
  ap.add_argument('--depth', type=int, default=4)
  ap.add_argument('--rounds', type=int, default=2)
  ap.add_argument('--steps', type=int, default=60)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--height', type=int, default=480)
  ap.add_argument('--width', type=int, default=640)
  ap.add_argument('--num-objs', type=int, default=21)
  args = ap.parse_args(argv)
  H, W_, O, F = args.height, args.width, args.num_objs, 64
  ckpt = weights.random_init(num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F))
  store = synthetic.ModelStore(O, F, seed=0)
  net0 = model.get_net(ckpt, 1, H, W_, O, F, mo)        # logits calibrated on the fp32 plan
  net0.forward(torch.from_numpy(synthetic.image(0, H, W_)[None]).cuda())
  torch.cuda.synchronize()
  synthetic.calibrate_logits(ckpt, net0.decoder_out[0].cpu().numpy())
  model._NETS.clear()
  del net0
  pool = []
  for j in range(5):
    tg = [{o: 1 for o in synthetic.targets(j, O, 5)}]
    pool.append((torch.from_numpy(synthetic.image(j, H, W_)[None]).cuda(), tg, [j]))
  pyrs = [[float(s) for s in p.split(',')] for p in args.pyramids.split(';')]
  built = [build(p, ckpt, store, mo, args) for p in pyrs]
  for _ in range(args.rounds):
    for p, (pipes, mem) in zip(pyrs, built):
      print(json.dumps(measure(p, pipes, mem, pool, args)), flush=True)


if __name__ == '__main__':
  main()
