"""Times the weight gradient of decoder/decoder_conv1_pointwise (csrc/pointwise_wgrad.hip) on
the device, warm, with HIP events, next to two torch routes on the same tensors, and a training
step with the layer unfrozen next to the heads-only step.

    python tools/bench_pointwise_wgrad.py [--repeats 30] \
        [--out profiles/r25/pointwise_wgrad_bench.txt]

At the workload's shape -- M = 19200 B rows (heads of 120 x 160) for B = 1 and 8, K = N = 256 --
with A behind a ReLU and a third of G zero, as the layer has them:
  (a) epos_pointwise_wgrad_f32 on an fp32 A, and on the fp16 pairs of the same A (the plan's
      default); epos_pointwise_wgrad_close_f32 with a batch norm, by itself;
  (b) A.double().t() @ G.double(): the same arithmetic, conversions included;
  (c) A.t() @ G in fp32: the cheap route.
All are timed INTERLEAVED -- one call of each per round, each between its own two events -- and
the medians of the rounds are reported, with the fp64 rate 2 M K N / time of (a) and (b). Before
timing, (a) is compared with (b) to (M + 16) 2^-52 sum |A||G|.
Then, on a 640 x 480 net with 21 objects and 64 fragments at B = 1: trainer.train_step with
the layer trained against the logits-only step, interleaved the same way, at lr = 0.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_eval import label_maps      # noqa: E402

H, W, O, F, K, N = 480, 640, 21, 64, 256, 256
IGNORE = 255


def main():
  import torch
  from epos_amd import _lib, net as enet, synthetic, trainer, weights
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=30)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  lib = _lib.load()
  torch.cuda.init()
  lines = ['weight gradient of decoder_conv1_pointwise, K = N = %d; medians of %d warm interleaved '
           'rounds (HIP events)' % (K, args.repeats)]

  def say(line):
    print(line, flush=True)
    lines.append(line)

  def ptr(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else None
  s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

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

  Wt = 0.06 * torch.randn((K, N), device='cuda')
  gamma, mean = torch.randn(N, device='cuda'), torch.randn(N, device='cuda')
  var = 0.5 + torch.rand(N, device='cuda')
  for B in (1, 8):
    M = B * (H // 4) * (W // 4)
    A = torch.relu(torch.randn((M, K), device='cuda')) * 3
    G = 1e-3 * torch.randn((M, N), device='cuda')
    G[torch.rand((M, N), device='cuda') < 0.33] = 0.0
    # the fp16 pairs of A at the scale of its absmax, as the depthwise kernel writes them
    amax = A.abs().max()
    slot = torch.zeros(_lib.AMAX_WORDS, dtype=torch.int32, device='cuda')
    slot[0] = amax.view(torch.int32)
    e = int(amax.view(torch.int32).item()) >> 23
    scale = 2.0 ** (268 - e - 127)
    t = A * scale
    hi = t.half()
    mid = ((t - hi.float()) * 2048.0).half()
    pairs = torch.stack([hi.view(M, K // 4, 4), mid.view(M, K // 4, 4)], dim=2).contiguous()
    A_h2 = pairs.view(M, 2 * K).view(torch.float32)
    assert tuple(A_h2.shape) == (M, K)
    nbytes = lib.epos_pointwise_wgrad_workspace_bytes(M, K, N)
    ws = torch.empty((max(1, nbytes // 8),), dtype=torch.int64, device='cuda')
    S = torch.empty((K, N), dtype=torch.float64, device='cuda')
    g = torch.empty((N,), dtype=torch.float64, device='cuda')
    dW, dgamma, dbeta = (torch.empty(n, device='cuda') for n in (K * N, N, N))
    ref = [None, None]

    def wgrad_args(a, h2):
      return _lib.PointwiseWgradArgs(
          A=ptr(a), lda=K, G=ptr(G), ldg=N, M=M, K=K, N=N, a_presplit=int(h2),
          a_amax=ptr(slot) if h2 else None, S=ptr(S), g=ptr(g), workspace=ptr(ws))
    a32, a16 = wgrad_args(A, False), wgrad_args(A_h2, True)

    def kernel_f32():
      _lib.check(lib.epos_pointwise_wgrad_f32(ctypes.byref(a32), s))

    def kernel_h2():
      _lib.check(lib.epos_pointwise_wgrad_f32(ctypes.byref(a16), s))

    def closing():
      _lib.check(lib.epos_pointwise_wgrad_close_f32(
          ptr(S), ptr(g), ptr(Wt), K, N, ptr(gamma), ptr(mean), ptr(var), 1e-5, ptr(dW),
          ptr(dgamma), ptr(dbeta), s))

    def torch_f64():
      ref[0] = A.double().t() @ G.double()

    def torch_f32():
      ref[1] = A.t() @ G

    # (a) against (b) before timing either
    kernel_f32()
    torch_f64()
    bound = (M + 16) * 2.0 ** -52 * (A.double().t() @ G.double().abs())
    torch.cuda.synchronize()
    assert bool(((S - ref[0]).abs() <= bound).all()) and float(ref[0].abs().max()) > 0
    kernel_h2()
    torch.cuda.synchronize()
    assert float((S - ref[0]).abs().max()) <= 1e-5 * float(ref[0].abs().max())

    k32, k16, c_ms, t64, t32 = interleaved((kernel_f32, kernel_h2, closing, torch_f64, torch_f32))
    flop = 2.0 * M * K * N
    say('B=%d (M = %d rows, %d row ranges, %.1f MB of slabs): (a) epos_pointwise_wgrad_f32 on '
        'fp32 A %.4f ms (%.1f TFLOP/s fp64), on fp16-pair A %.4f ms (%.1f TFLOP/s); '
        'epos_pointwise_wgrad_close_f32 %.4f ms; (b) torch A.double().t() @ G.double() %.4f ms '
        '(%.1f TFLOP/s); (c) torch fp32 A.t() @ G %.4f ms; (a, pairs) / (b) = %.2f; '
        '(a, pairs) / (c) = %.2f' % (
            B, M, -(-M // lib.epos_pointwise_wgrad_range_rows(M, K, N)), nbytes / 1e6, k32,
            flop / k32 / 1e9, k16, flop / k16 / 1e9, c_ms, t64, flop / t64 / 1e9, t32,
            k16 / t64, k16 / t32))
    del A, G, A_h2, pairs, hi, mid, t, ws, ref
    torch.cuda.empty_cache()

  # a training step with the layer unfrozen against the heads-only step, B = 1
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  net = enet.EposNet(ckpt, 1, H, W, O, F, device='cuda:0')
  heads_opt = trainer.Optimizer(ckpt, lr=1e-4)
  layer_opt = trainer.Optimizer(ckpt, lr=1e-4, trainable=trainer.VARIABLES)
  images = torch.from_numpy(synthetic.image(0, H, W)[None].astype(np.uint8)).cuda()
  gt_h, _ = label_maps(1, 1)
  gt_h[:, :6] = IGNORE
  gt = {'obj_label': torch.from_numpy(gt_h).cuda(),
        'frag_label': torch.randint(0, F, (1, H // 4, W // 4), dtype=torch.int32, device='cuda'),
        'frag_loc': torch.randn((1, H // 4, W // 4, 3), device='cuda'),
        'frag_weight': torch.ones((1, H // 4, W // 4), device='cuda')}
  lr = 0.0                                      # the weights stay where they are

  def heads_step():
    trainer.train_step(net, images, gt, heads_opt, lr)

  def layer_step():
    trainer.train_step(net, images, gt, layer_opt, lr)

  def forward():
    net.forward_logits(images, use_graph=True)

  f_ms, h_ms, l_ms = interleaved((forward, heads_step, layer_step))
  say('B=1, %dx%d, presplit A = %s: forward_logits %.4f ms; train_step, logits only %.4f ms; '
      'train_step with the layer %.4f ms; the layer adds %.4f ms (%.1f %%)' % (
          W, H, net.pointwise_operand()['presplit'], f_ms, h_ms, l_ms, l_ms - h_ms,
          100.0 * (l_ms - h_ms) / h_ms))
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
