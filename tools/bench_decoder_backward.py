"""Times the backward pass through decoder_conv1 (csrc/pointwise_dgrad.hip,
csrc/depthwise_grad.hip) on the device, warm, with HIP events, next to torch routes on the same
tensors and to a device copy of the same bytes, and the whole chain from a running net next to
net_grads.

    python tools/bench_decoder_backward.py [--repeats 30] \
        [--out profiles/r28/decoder_backward_bench.txt]

At the workload's shape -- heads of 120 x 160, M = 19200 B rows for B = 1 and 8, K = N = C = 256 --
with A and X behind a ReLU and a third of G zero, as the layers have them:
  (a) epos_pointwise_dgrad_f32 (fold + GEMM) with the mask as fp16 pairs (the plan's default),
      as fp32 and without one, with the fp64 rate 2 M K N / time; torch's (G @ Wf.t()) * (A > 0)
      in fp32 and in fp64 (conversions included);
  (b) epos_depthwise_wgrad_f32 (+ its closing through epos_pointwise_wgrad_close_f32, by itself)
      and epos_depthwise_dgrad_f32, with the bytes they must move (X and D read; D and the mask
      read, dX written) over their time; torch's conv2d weight and input gradients in fp32 on
      channels-last tensors; a device copy of the same number of bytes.
All are timed INTERLEAVED -- one call of each per round, each between its own two events -- and
the medians of the rounds are reported. Before timing, (a) is compared with torch's fp64 product
and (b) with torch's fp64 gradients.
Then, on a 640 x 480 net with 21 objects and 64 fragments at B = 1 and 8, after a forward_logits:
trainer.decoder_conv1_grads against trainer.net_grads with the four layers, interleaved.
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
# profiles/r25/: the merged weight-gradient GEMM of the same 2 M K N flops, fp16-pair A
WGRAD_MS = {1: 0.084, 8: 0.42}


def main():
  import torch
  from epos_amd import _lib, net as enet, synthetic, trainer, weights
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=30)
  ap.add_argument('--batches', default='1,8')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  batches = [int(b) for b in args.batches.split(',')]
  lib = _lib.load()
  torch.cuda.init()
  lines = ['backward through decoder_conv1, K = N = C = %d; medians of %d warm interleaved rounds '
           '(HIP events)' % (K, args.repeats)]

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
  scale = (gamma.double() / torch.sqrt(var.double() + 1e-5)).float()
  Wf = Wt * scale[None, :]
  w9c = 0.3 * torch.randn((9, K), device='cuda')
  w9 = 0.3 * torch.randn((9, K), device='cuda')
  dh, dw_ = H // 4, W // 4
  for B in batches:
    M = B * dh * dw_
    A = torch.relu(torch.randn((M, K), device='cuda')) * 3
    X = torch.relu(torch.randn((B, dh, dw_, K), device='cuda')) * 3
    G = 1e-3 * torch.randn((M, N), device='cuda')
    G[torch.rand((M, N), device='cuda') < 0.33] = 0.0
    # the fp16 pairs of A at the scale of its absmax, as the depthwise kernel writes them
    e = int(A.abs().max().view(torch.int32).item()) >> 23
    t = A * 2.0 ** (268 - e - 127)
    hi = t.half()
    mid = ((t - hi.float()) * 2048.0).half()
    pairs = torch.stack([hi.view(M, K // 4, 4), mid.view(M, K // 4, 4)], dim=2).contiguous()
    A_h2 = pairs.view(M, 2 * K).view(torch.float32)
    ws = torch.empty((lib.epos_pointwise_dgrad_workspace_bytes(K, N) // 8,), dtype=torch.float64,
                     device='cuda')
    D = torch.empty((M, K), device='cuda')
    ref = [None] * 4

    def dgrad_args(mask, h2):
      return _lib.PointwiseDgradArgs(
          G=ptr(G), ldg=N, W=ptr(Wt), gamma=ptr(gamma), moving_variance=ptr(var), eps=1e-5,
          mask=ptr(mask), ldm=K, mask_h2=int(h2), M=M, K=K, N=N, D=ptr(D), ldd=K,
          workspace=ptr(ws))
    a_h2, a_f32, a_none = dgrad_args(A_h2, True), dgrad_args(A, False), dgrad_args(None, False)

    def dgrad_h2():
      _lib.check(lib.epos_pointwise_dgrad_f32(ctypes.byref(a_h2), s))

    def dgrad_f32():
      _lib.check(lib.epos_pointwise_dgrad_f32(ctypes.byref(a_f32), s))

    def dgrad_none():
      _lib.check(lib.epos_pointwise_dgrad_f32(ctypes.byref(a_none), s))

    def torch_f32():
      ref[0] = (G @ Wf.t()) * (A > 0)

    def torch_f64():
      ref[1] = (G.double() @ Wf.double().t()) * (A > 0)

    dgrad_f32()
    torch_f64()
    bound = 2.0 ** -24 * ref[1].abs() + (N + 16) * 2.0 ** -52 * (G.double().abs() @
                                                                 Wf.double().abs().t())
    torch.cuda.synchronize()
    assert bool(((D.double() - ref[1]).abs() <= bound).all()) and float(ref[1].abs().max()) > 0
    ref[1] = None
    k_h2, k_f32, k_none, t32, t64 = interleaved((dgrad_h2, dgrad_f32, dgrad_none, torch_f32,
                                                 torch_f64))
    flop = 2.0 * M * K * N
    say('B=%d (M = %d rows): (a) epos_pointwise_dgrad_f32 with a pair mask %.4f ms (%.1f TFLOP/s '
        'fp64), an fp32 mask %.4f ms (%.1f TFLOP/s), no mask %.4f ms; torch (G @ Wf.t()) * (A > 0) '
        'fp32 %.4f ms, fp64 %.4f ms (%.1f TFLOP/s); (a, pairs) / torch fp64 = %.2f; (a, pairs) / '
        'torch fp32 = %.2f; (a, pairs) / the weight-gradient GEMM of profiles/r25 (%.3f ms) = %.2f'
        % (B, M, k_h2, flop / k_h2 / 1e9, k_f32, flop / k_f32 / 1e9, k_none, t32, t64,
           flop / t64 / 1e9, k_h2 / t64, k_h2 / t32, WGRAD_MS.get(B, float('nan')),
           k_h2 / WGRAD_MS.get(B, float('nan'))))
    ref[0] = ref[1] = None

    # ---- the depthwise layer
    dims = (B, dh, dw_, K)
    nbytes = lib.epos_depthwise_wgrad_workspace_bytes(*dims)
    ws2 = torch.empty((max(1, nbytes // 8),), dtype=torch.int64, device='cuda')
    T = torch.empty((9, K), dtype=torch.float64, device='cuda')
    tsum = torch.empty((K,), dtype=torch.float64, device='cuda')
    dwo, dgo, dbo = (torch.empty(n, device='cuda') for n in (9 * K, K, K))
    dX = torch.empty(dims, device='cuda')
    wa = _lib.DepthwiseWgradArgs(X=ptr(X), ldx=K, D=ptr(D), ldd=K, B=B, H=dh, W=dw_, C=K, stride=1,
                                 rate=1, T=ptr(T), t=ptr(tsum), workspace=ptr(ws2))

    def dw_wgrad():
      _lib.check(lib.epos_depthwise_wgrad_f32(ctypes.byref(wa), s))

    def dw_close():
      _lib.check(lib.epos_pointwise_wgrad_close_f32(
          ptr(T), ptr(tsum), ptr(w9), 9, K, ptr(gamma), ptr(mean), ptr(var), 1e-5, ptr(dwo),
          ptr(dgo), ptr(dbo), s))

    def dw_dgrad():
      _lib.check(lib.epos_depthwise_dgrad_f32(ptr(D), K, ptr(w9c), ptr(X), K, ptr(dX), K, B, dh,
                                              dw_, K, 1, s))

    one = torch.empty((2, M * K), device='cuda')
    half = torch.empty((2, 3 * M * K // 2), device='cuda')

    def copy_wgrad():                     # X and D read: the bytes a copy of ONE tensor moves
      one[1].copy_(one[0])

    def copy_dgrad():                     # D and the mask read, dX written: a copy of 1.5
      half[1].copy_(half[0])

    dgrad_h2()                            # D as the chain has it
    x_nchw = X.permute(0, 3, 1, 2)        # channels-last views of the NHWC tensors
    d_nchw = D.view(dims).permute(0, 3, 1, 2)
    wt_conv = w9c.t().reshape(K, 1, 3, 3).contiguous()
    torch_ok = True

    def torch_wgrad():
      ref[2] = torch.nn.grad.conv2d_weight(x_nchw, (K, 1, 3, 3), d_nchw, padding=1, groups=K)

    def torch_dgrad():
      ref[3] = torch.nn.grad.conv2d_input((B, K, dh, dw_), wt_conv, d_nchw, padding=1, groups=K)
    try:
      dw_wgrad()
      dw_dgrad()
      want_T = torch.nn.grad.conv2d_weight(x_nchw.double(), (K, 1, 3, 3), d_nchw.double(),
                                           padding=1, groups=K).reshape(K, 9).t()
      want_dX = torch.nn.grad.conv2d_input((B, K, dh, dw_), wt_conv.double(), d_nchw.double(),
                                           padding=1, groups=K).permute(0, 2, 3, 1) * (X > 0)
      torch.cuda.synchronize()
      assert float(want_T.abs().max()) > 0 and float(want_dX.abs().max()) > 0
      assert float((T - want_T).abs().max()) <= 1e-9 * float(want_T.abs().max())
      assert float((dX.double() - want_dX).abs().max()) <= 1e-6 * float(want_dX.abs().max())
      del want_T, want_dX
      torch_wgrad()
      torch_dgrad()
      torch.cuda.synchronize()
    except (RuntimeError, AssertionError) as err:           # a conv route torch lacks here
      torch_ok = False
      say('B=%d: torch conv2d backward not measured: %s' % (B, str(err).splitlines()[0]))
    fns = [dw_wgrad, dw_close, dw_dgrad, copy_wgrad, copy_dgrad]
    if torch_ok:
      fns += [torch_wgrad, torch_dgrad]
    res = interleaved(tuple(fns))
    wg, cl, dg, cw, cd = res[:5]
    gb_w, gb_d = 2 * 4.0 * M * K / 1e9, 3 * 4.0 * M * K / 1e9
    say('B=%d: (b) epos_depthwise_wgrad_f32 %.4f ms (%d ranges, %.1f MB of slabs; %.0f GB/s of X '
        'and D), closing %.4f ms, a device copy moving as many bytes %.4f ms, ratio %.2f; '
        'epos_depthwise_dgrad_f32 %.4f ms (%.0f GB/s of D, mask and dX), a device copy moving as '
        'many bytes %.4f ms, ratio %.2f' % (
            B, wg, -(-M // lib.epos_depthwise_wgrad_range_pixels(*dims)), nbytes / 1e6,
            gb_w / wg * 1e3, cl, cw, wg / cw, dg, gb_d / dg * 1e3, cd, dg / cd))
    if torch_ok:
      say('B=%d: torch conv2d_weight fp32 %.4f ms (epos / torch = %.2f), conv2d_input fp32 %.4f ms '
          '(epos / torch = %.2f)' % (B, res[5], wg / res[5], res[6], dg / res[6]))
    del A, X, G, A_h2, pairs, hi, mid, t, D, dX, one, half, ws2, ref
    torch.cuda.empty_cache()

  # the whole chain from a running net against net_grads with the four layers
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  for B in batches:
    net = enet.EposNet(ckpt, B, H, W, O, F, device='cuda:0')
    variables = {n: torch.from_numpy(np.ascontiguousarray(ckpt[n])).cuda()
                 for n in trainer.VARIABLES}
    images = torch.from_numpy(np.stack([synthetic.image(i, H, W) for i in range(B)]).astype(
        np.uint8)).cuda()
    gt_h, _ = label_maps(B, 1)
    gt_h[:, :6] = IGNORE
    gt = {'obj_label': torch.from_numpy(gt_h).cuda(),
          'frag_label': torch.randint(0, F, (B, dh, dw_), dtype=torch.int32, device='cuda'),
          'frag_loc': torch.randn((B, dh, dw_, 3), device='cuda'),
          'frag_weight': torch.ones((B, dh, dw_), device='cuda')}
    net.forward_logits(images, use_graph=True)
    layers = tuple(weights.TRAINABLE_LAYERS)

    def four_layers():
      trainer.net_grads(net, gt, variables, layers)

    def chain():
      trainer.decoder_conv1_grads(net, gt, variables)

    n_ms, c_ms = interleaved((four_layers, chain))
    say('B=%d, %dx%d, presplit A = %s: net_grads with the four layers %.4f ms; '
        'decoder_conv1_grads %.4f ms; the three new gradients add %.4f ms (%.1f %%)' % (
            B, W, H, net.pointwise_operand()['presplit'], n_ms, c_ms, c_ms - n_ms,
            100.0 * (c_ms - n_ms) / n_ms))
    del net, variables, images, gt
    torch.cuda.empty_cache()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
