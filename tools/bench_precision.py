#!/usr/bin/env python
"""images/s of the end-to-end pipeline per numeric mode of the network (precision 'fp32' /
'bf16'), one JSON line per run, driven the way tools/bench_variants.py drives it (batch 1,
random-init weights with randomised BatchNorm and logits calibrated on one frame, 4 pipelines
in flight with 2 batches queued each, 5 resident 640x480 frames, 5 targets of 21 objects,
hipGraph replay). The precisions alternate in one process, `--rounds` times each, so that both
see the same clocks.

    python tools/bench_precision.py --variants xception_65,resnet_v1_101_beta --rounds 2
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


def measure(variant, precision, args):
  B, H, W_, O, F = 1, args.height, args.width, args.num_objs, 64
  ckpt = weights.random_init(variant, num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), model_variant=variant)
  store = synthetic.ModelStore(O, F, seed=0)
  net0 = model.get_net(ckpt, 1, H, W_, O, F, mo)        # logits calibrated on the fp32 plan
  net0.forward(torch.from_numpy(synthetic.image(0, H, W_)[None]).cuda())
  torch.cuda.synchronize()
  synthetic.calibrate_logits(ckpt, net0.decoder_out[0].cpu().numpy())
  model._NETS.clear()
  del net0
  depth = 4
  pipes = [pipeline.EposPipeline(ckpt, B, H, W_, O, F, store, capacity=1 << 20,
                                 max_instances=1, instance=j, model_options=mo, queue=2,
                                 precision=precision)
           for j in range(depth)]
  pool = []
  for j in range(5):
    tg = [{o: 1 for o in synthetic.targets(j, O, 5)}]
    pool.append((torch.from_numpy(synthetic.image(j, H, W_)[None]).cuda(), tg, [j]))
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
  out = {'metric': 'images/sec end-to-end (CNN+PnP-RANSAC), %dx%d' % (W_, H),
         'config': CONFIG.get(variant, variant), 'model_variant': variant,
         'precision': precision, 'value': round(args.steps * B / dt, 3),
         'ms_per_step': round(dt / args.steps * 1e3, 3), 'steps': args.steps,
         'warmup': args.warmup, 'poses': poses, 'plan_launches': len(net.ops),
         'algorithmic_gb': round(net.algorithmic_bytes() / 1e9, 3)}
  del pipes, net
  model._NETS.clear()
  torch.cuda.empty_cache()
  return out


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--variants', default='xception_65,resnet_v1_101_beta')
  ap.add_argument('--precisions', default='fp32,bf16')
  ap.add_argument('--rounds', type=int, default=2)
  ap.add_argument('--steps', type=int, default=60)
  ap.add_argument('--warmup', type=int, default=6)
  ap.add_argument('--height', type=int, default=480)
  ap.add_argument('--width', type=int, default=640)
  ap.add_argument('--num-objs', type=int, default=21)
  args = ap.parse_args(argv)
  for v in args.variants.split(','):
    weights.variant(v)
    for _ in range(args.rounds):
      for prec in args.precisions.split(','):
        print(json.dumps(measure(v, prec, args)), flush=True)


if __name__ == '__main__':
  main()
