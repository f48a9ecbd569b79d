"""Times the weight update of the logits layers (csrc/weight_pack.hip through
EposNet.set_weights) on the device, warm, with HIP events, next to the route the host
packers allow and next to the floor of anything that reads the weights and writes the packs.

    python tools/bench_head_update.py [--repeats 30] [--out profiles/r22/head_update_bench.txt]

At the workload's size -- K = 256, 21 objects, 64 fragments: the three layers (22, 1344 and
4032 columns) plus the 42 per-object packs of the sparse heads, 45 matrices, 2.8 M packed
weights in four layouts -- on a 640 x 480 net at B = 1:
  (a) net.set_weights(opt.params, check=False): one grouped device call;
  (b) the route without the device packer, for the same effect on the same buffers: download
      the six tensors, net_modes._fold and the three host packers per matrix, copy_ into the
      plan's tensors;
  (c) the floor: device-to-device copies of every source tensor and, from scratch tensors of
      the same sizes, into every destination.
(a), (b) and (c) are timed INTERLEAVED -- one call of each per round, each between its own two
events -- and the medians of the rounds are reported. Then one trainer.train_step against its
parts (forward_logits from its graph, net_grads, Optimizer.step), interleaved the same way: the difference is what the update adds to a step.
Before timing, the bytes (a) leaves in the plan's tensors are compared with (b)'s.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_eval import label_maps      # noqa: E402

H, W, O, F = 480, 640, 21, 64
IGNORE = 255


def main():
  import torch
  from epos_amd import net as enet, net_modes, synthetic, trainer, weights
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=30)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  torch.cuda.init()
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  net = enet.EposNet(ckpt, 1, H, W, O, F, device='cuda:0')
  mode = net.mode
  opt = trainer.Optimizer(ckpt, lr=1e-4)
  net._build_sparse_packs()
  layers = sorted(weights.outputs_to_num_channels(O, F))
  sparse = {'pred_frag_conf': (0, F), 'pred_frag_loc': (1, 3 * F)}

  def packs():
    """(layer, col0, n, (wp, bp, ws, wh)) of the 45 matrices."""
    for layer in layers:
      yield layer, 0, opt.params['logits/%s/biases' % layer].numel(), mode.packs['logits/' + layer][2]
    for layer, (kind, n) in sorted(sparse.items()):
      for o in range(O):
        yield layer, o * n, n, net._sparse_packs[o][kind]

  def device_route():
    net.set_weights(opt.params, check=False)

  def host_route():
    host = {k: v.cpu().numpy() for k, v in opt.params.items()}
    for layer, col0, n, (wp, bp, ws, wh) in packs():
      w = host['logits/%s/weights' % layer].reshape(256, -1)[:, col0:col0 + n]
      w = net_modes._fold(np.ascontiguousarray(w), np.ones(n, np.float32), 4)
      b = host['logits/%s/biases' % layer][col0:col0 + n]
      wp.copy_(torch.from_numpy(net_modes._pack(mode.pack_plain, w, np.float32)))
      ws.copy_(torch.from_numpy(net_modes._pack(mode.pack_split, w, np.uint8)))
      bp.copy_(torch.from_numpy(net_modes._bias(b, n, 128)))
      if wh is not None:
        wh.copy_(torch.from_numpy(net_modes._pack(mode.pack_h2, w, np.uint8)))

  dsts = [t for _, _, _, pack in packs() for t in pack if t is not None]
  scratch = [torch.empty_like(t) for t in dsts]
  srcs = list(opt.params.values())
  src_copy = [torch.empty_like(t) for t in srcs]
  src_bytes = sum(t.numel() * t.element_size() for t in srcs)
  dst_bytes = sum(t.numel() * t.element_size() for t in dsts)

  def floor():
    for d, s in zip(src_copy, srcs):
      d.copy_(s)
    for d, s in zip(dsts, scratch):
      d.copy_(s)

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

  # (a) against (b) on the same buffers, before timing either
  host_route()
  torch.cuda.synchronize()
  want = [t.clone() for t in dsts]
  for t in dsts:
    t.view(torch.uint8).fill_(0xA5)
  status = net.set_weights(opt.params, check=False)
  torch.cuda.synchronize()
  assert status.tolist() == [0] * 45
  for got, exp in zip(dsts, want):
    assert torch.equal(got.view(torch.uint8), exp.view(torch.uint8))
  scratch = [t.clone() for t in want]          # the floor leaves the right weights behind

  lines = ['weight update of the logits layers, K = 256, %d objects, %d fragments: 45 matrices, '
           '%.2f M weights; medians of %d warm interleaved rounds (HIP events)' % (
               O, F, sum(n for _, _, n, _ in packs()) * 256 / 1e6, args.repeats)]
  a_ms, b_ms, c_ms = interleaved((device_route, host_route, floor))
  line = ('(a) set_weights(check=False) %.4f ms; (b) download + host packers + copy_ '
          '%.2f ms; (c) device-to-device copies, %.1f MB of sources and %.1f MB of packs, '
          '%.4f ms; (b) / (a) = %.0f; (a) / (c) = %.2f' % (
              a_ms, b_ms, src_bytes / 1e6, dst_bytes / 1e6, c_ms, b_ms / a_ms, a_ms / c_ms))
  print(line, flush=True)
  lines.append(line)

  # one training step against its parts, B = 1
  images = torch.from_numpy(synthetic.image(0, H, W)[None].astype(np.uint8)).cuda()
  gt_h, _ = label_maps(1, 1)
  gt_h[:, :6] = IGNORE
  gt = {'obj_label': torch.from_numpy(gt_h).cuda(),
        'frag_label': torch.randint(0, F, (1, H // 4, W // 4), dtype=torch.int32, device='cuda'),
        'frag_loc': torch.randn((1, H // 4, W // 4, 3), device='cuda'),
        'frag_weight': torch.ones((1, H // 4, W // 4), device='cuda')}
  lr = 0.0                                      # the weights stay where they are

  def parts():
    net.forward_logits(images, use_graph=True)
    values, bad, grads = trainer.net_grads(net, gt, opt.params)
    opt.step(grads, lr)

  def step():
    trainer.train_step(net, images, gt, opt, lr)

  p_ms, s_ms = interleaved((parts, step))
  line = ('B=1, %dx%d: forward_logits + net_grads + Optimizer.step %.4f ms; '
          'train_step %.4f ms; the update adds %.4f ms (%.1f %%)' % (
              W, H, p_ms, s_ms, s_ms - p_ms, 100.0 * (s_ms - p_ms) / p_ms))
  print(line, flush=True)
  lines.append(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
