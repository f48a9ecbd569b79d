"""Times the backward pass through the decoder (csrc/resize_grad.hip and the existing gradient
kernels at the widths trainer.decoder_grads brings) on the device, warm, with HIP events.

    python tools/bench_decoder_chain.py --build-parent [--parent-rev HEAD~1]   # where git and hipcc are
    python tools/bench_decoder_chain.py [--repeats 30] [--out profiles/r30/decoder_chain_bench.txt]

At C2's sizes -- encoder 60 x 80, decoder 120 x 160, C = 256 -- for B = 1 and 8, all candidates of
a group INTERLEAVED in one process (one call of each per round, each between its own two
events), medians of the rounds:
  (a) epos_resize_bilinear_dgrad_f32 with and without the mask, next to a device copy that moves
      as many bytes (D and the mask read, dX written), and next to torch's interpolate backward
      in fp32 on channels-last tensors (which adds with floating-point atomics);
  (b) the existing kernels at their new widths, through their wrappers with an fp32 A: the
      weight-gradient GEMM at K x N = 304 x 256, 128 x 48, 256 x 48 (rows of the decoder) and
      1280 x 256 (rows of the encoder); the input gradient at K = 304; the depthwise sums and
      input gradient at C = 304;
  (c) on a 640 x 480 net with 21 objects and 64 fragments, after a forward_logits:
      trainer.decoder_conv1_grads against trainer.decoder_grads;
  (d) with the parent commit's library (--build-parent; epos_amd/lib/libepos_hip_parent.so and a
      second copy of it) swapped in under the same Python: trainer.net_grads with the four layers
      and trainer.decoder_conv1_grads -- a sha256 of every output per library, and the times of
      this build over the parent's next to parent2 over parent, the spread of the measurement.
Nothing here is a gate: the numbers are recorded.
"""
import argparse
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_eval import label_maps                      # noqa: E402
from tools.bench_knn import build_parent, parent_paths       # noqa: E402

H, W, O, F, C = 480, 640, 21, 64, 256
EH, EW, DH, DW = 60, 80, 120, 160
IGNORE = 255


def open_library(path):
  """Another build of the library with the entries it has bound as _lib.SYMBOLS binds them (the
  parent lacks the entries this change adds)."""
  from epos_amd import _lib
  lib = ctypes.CDLL(path)
  for name, (restype, argtypes) in _lib.SYMBOLS.items():
    fn = getattr(lib, name, None)
    if fn is not None:
      fn.restype = restype
      if argtypes is not None:
        fn.argtypes = argtypes
  return lib


def digest(tensors):
  h = hashlib.sha256()
  for t in tensors:
    h.update(t.detach().contiguous().cpu().numpy().tobytes())
  return h.hexdigest()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=30)
  ap.add_argument('--batches', default='1,8')
  ap.add_argument('--out', default=None)
  ap.add_argument('--build-parent', action='store_true')
  ap.add_argument('--parent-rev', default='HEAD~1')
  args = ap.parse_args()
  if args.build_parent:
    build_parent(args.parent_rev)
    return
  import torch
  from epos_amd import _lib, decoder_train as DT, net as enet, synthetic, trainer, weights
  batches = [int(b) for b in args.batches.split(',')]
  lib = _lib.load()
  torch.cuda.init()
  lines = ['backward through the decoder, encoder %dx%d, decoder %dx%d, C = %d; medians of %d warm '
           'interleaved rounds (HIP events)' % (EH, EW, DH, DW, C, args.repeats)]

  def say(line):
    print(line, flush=True)
    lines.append(line)

  def ptr(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else None
  s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

  def interleaved(fns, all_rounds=False):
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
    return times if all_rounds else [float(np.median(ts)) for ts in times]

  for B in batches:
    # ---- (a) the resize adjoint
    D = 1e-3 * torch.randn((B, DH, DW, C), device='cuda')
    Y = torch.relu(torch.randn((B, EH, EW, C), device='cuda'))
    dX = torch.empty((B, EH, EW, C), device='cuda')
    n_d, n_x = D.numel(), dX.numel()

    def adj_mask():
      _lib.check(lib.epos_resize_bilinear_dgrad_f32(ptr(D), C, ptr(Y), C, ptr(dX), C, B, EH, EW,
                                                    DH, DW, C, s))

    def adj_plain():
      _lib.check(lib.epos_resize_bilinear_dgrad_f32(ptr(D), C, None, C, ptr(dX), C, B, EH, EW,
                                                    DH, DW, C, s))
    with_mask = torch.empty((2, (n_d + 2 * n_x) // 2), device='cuda')
    without = torch.empty((2, (n_d + n_x) // 2), device='cuda')

    def copy_mask():
      with_mask[1].copy_(with_mask[0])

    def copy_plain():
      without[1].copy_(without[0])
    x_cl = torch.zeros((B, C, EH, EW), device='cuda').contiguous(
        memory_format=torch.channels_last).requires_grad_()
    y_cl = torch.nn.functional.interpolate(x_cl, size=(DH, DW), mode='bilinear',
                                           align_corners=True)
    d_cl = D.permute(0, 3, 1, 2)                          # a channels-last view of the NHWC D
    got = [None]

    def torch_adj():
      got[0] = torch.autograd.grad(y_cl, x_cl, d_cl, retain_graph=True)[0]
    adj_plain()
    torch_adj()
    torch.cuda.synchronize()
    diff = float((dX - got[0].permute(0, 2, 3, 1)).abs().max() / got[0].abs().max())
    assert diff < 1e-4, diff
    k_m, k_p, c_m, c_p, t_a = interleaved((adj_mask, adj_plain, copy_mask, copy_plain, torch_adj))
    gb_m, gb_p = 4.0 * (n_d + 2 * n_x) / 1e9, 4.0 * (n_d + n_x) / 1e9
    say('B=%d: (a) epos_resize_bilinear_dgrad_f32 with the mask %.4f ms (%.0f GB/s of D, mask and '
        'dX), a device copy moving as many bytes %.4f ms, ratio %.2f; without the mask %.4f ms '
        '(%.0f GB/s), copy %.4f ms, ratio %.2f; torch interpolate backward fp32 channels-last '
        '%.4f ms (epos / torch = %.2f; largest difference %.1e of the largest gradient)' % (
            B, k_m, gb_m / k_m * 1e3, c_m, k_m / c_m, k_p, gb_p / k_p * 1e3, c_p, k_p / c_p, t_a,
            k_p / t_a, diff))
    del with_mask, without, x_cl, y_cl, got
    torch.cuda.empty_cache()

    # ---- (b) the existing kernels at their new widths
    def wgrad_case(M, K, N):
      A = torch.relu(torch.randn((M, K), device='cuda'))
      G = 1e-3 * torch.randn((M, N), device='cuda')
      Wt = 0.06 * torch.randn((K, N), device='cuda')
      bn = (torch.randn(N, device='cuda'), torch.randn(N, device='cuda'),
            0.5 + torch.rand(N, device='cuda'))
      ws = torch.empty((DT.workspace_words(M, K, N),), dtype=torch.int64, device='cuda')
      out = {n: torch.empty(K * N if n == 'weights' else N, device='cuda')
             for n in weights.CONV_VARIABLES[True]}
      return lambda: DT.pointwise_weight_grads(A, G, Wt, bn=bn, eps=1e-5, out=out, workspace=ws)
    M_dec, M_enc = B * DH * DW, B * EH * EW
    shapes = ((M_dec, 304, 256), (M_dec, 128, 48), (M_dec, 256, 48), (M_enc, 1280, 256))
    res = interleaved(tuple(wgrad_case(*sh) for sh in shapes))
    say('B=%d: (b) pointwise_weight_grads (fp32 A, closing included) ' % B + '; '.join(
        'M=%d %dx%d %.4f ms (%.1f TFLOP/s fp64)' % (m, k, n, t, 2.0 * m * k * n / t / 1e9)
        for (m, k, n), t in zip(shapes, res)))
    K0 = 304
    G = 1e-3 * torch.randn((M_dec, C), device='cuda')
    A0 = torch.relu(torch.randn((M_dec, K0), device='cuda'))
    W0 = 0.06 * torch.randn((K0, C), device='cuda')
    bn2 = (torch.randn(C, device='cuda'), 0.5 + torch.rand(C, device='cuda'))
    D0 = torch.empty((M_dec, K0), device='cuda')
    ws0 = torch.empty((lib.epos_pointwise_dgrad_workspace_bytes(K0, C) // 8,),
                      dtype=torch.float64, device='cuda')
    X = torch.relu(torch.randn((B, DH, DW, K0), device='cuda'))
    w9 = 0.3 * torch.randn((3, 3, K0, 1), device='cuda')
    w9c = 0.3 * torch.randn((9, K0), device='cuda')
    bn3 = (torch.randn(K0, device='cuda'), torch.randn(K0, device='cuda'),
           0.5 + torch.rand(K0, device='cuda'))
    wsd = torch.empty((DT.depthwise_workspace_words(B, DH, DW, K0),), dtype=torch.int64,
                      device='cuda')
    dcat = torch.empty((B, DH, DW, K0), device='cuda')
    D4 = D0.view(B, DH, DW, K0)
    wl, wr = w9c[:, :C].contiguous(), w9c[:, C:].contiguous()

    def dgrad304():
      DT.pointwise_input_grad(G, W0, bn=bn2, eps=1e-5, relu_of=A0, out=D0, workspace=ws0)

    def dw_wgrad304():
      DT.depthwise_weight_grads(X, D4, w9, bn3, 1e-5, workspace=wsd)

    def dw_dgrad304():                                    # as the chain runs it: two slices
      DT.depthwise_input_grad(D4[..., :C], wl, out=dcat[..., :C])
      DT.depthwise_input_grad(D4[..., C:], wr, relu_of=X[..., C:], out=dcat[..., C:])
    dgrad304()
    t_dg, t_ww, t_wd = interleaved((dgrad304, dw_wgrad304, dw_dgrad304))
    say('B=%d: (b) pointwise_input_grad K=304 N=256 (fp32 mask) %.4f ms (%.1f TFLOP/s fp64); '
        'depthwise_weight_grads C=304 (closing included) %.4f ms (%.0f GB/s of X and D); '
        'depthwise_input_grad C=304 in its two slices %.4f ms (%.0f GB/s of D, the 48-wide mask '
        'and dX)' % (B, t_dg, 2.0 * M_dec * K0 * C / t_dg / 1e9, t_ww,
                     8.0 * M_dec * K0 / t_ww / 1e6, t_wd,
                     4.0 * M_dec * (2 * K0 + 48) / t_wd / 1e6))
    del D, Y, dX, G, A0, D0, X, dcat, D4, wsd
    torch.cuda.empty_cache()

  # ---- (c), (d): from a running net
  parents = [open_library(p) if os.path.exists(p) else None for p in parent_paths()]
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  layers = tuple(weights.TRAINABLE_LAYERS)
  for B in batches:
    net = enet.EposNet(ckpt, B, H, W, O, F, device='cuda:0')
    variables = {n: torch.from_numpy(np.ascontiguousarray(ckpt[n])).cuda()
                 for n in trainer.VARIABLES}
    images = torch.from_numpy(np.stack([synthetic.image(i, H, W) for i in range(B)]).astype(
        np.uint8)).cuda()
    gt_h, _ = label_maps(B, 1)
    gt_h[:, :6] = IGNORE
    gt = {'obj_label': torch.from_numpy(gt_h).cuda(),
          'frag_label': torch.randint(0, F, (B, DH, DW), dtype=torch.int32, device='cuda'),
          'frag_loc': torch.randn((B, DH, DW, 3), device='cuda'),
          'frag_weight': torch.ones((B, DH, DW), device='cuda')}
    net.forward_logits(images, use_graph=True)

    def conv1():
      return trainer.decoder_conv1_grads(net, gt, variables)

    def whole():
      return trainer.decoder_grads(net, gt, variables)
    c_ms, w_ms = interleaved((conv1, whole))
    say('B=%d, %dx%d, presplit A = %s: (c) decoder_conv1_grads %.4f ms; decoder_grads %.4f ms; '
        'the twelve new gradients and d_proj add %.4f ms (%.1f %%)' % (
            B, W, H, net.pointwise_operand()['presplit'], c_ms, w_ms, w_ms - c_ms,
            100.0 * (w_ms - c_ms) / c_ms))
    if None in parents:
      say('B=%d: (d) not measured: build the parent library first (--build-parent)' % B)
      continue

    def under(handle, fn):
      def run():
        keep, _lib._lib = _lib._lib, handle
        try:
          return fn()
        finally:
          _lib._lib = keep
      return run

    def four():
      return trainer.net_grads(net, gt, variables, layers)

    def flat(result):
      out = [result[0], result[1]] + [result[2][n] for n in sorted(result[2])]
      return out + list(result[3:])
    builds = (('parent', parents[0]), ('this', lib), ('parent2', parents[1]))
    for what, fn in (('net_grads with the four layers', four), ('decoder_conv1_grads', conv1)):
      hashes = {}
      for name, handle in builds:
        out = under(handle, fn)()
        torch.cuda.synchronize()
        hashes[name] = digest(flat(out))
      rounds = interleaved(tuple(under(handle, fn) for _, handle in builds), all_rounds=True)
      med = [float(np.median(ts)) for ts in rounds]
      ratio = lambda i: float(np.median(np.asarray(rounds[i]) / np.asarray(rounds[0])))  # noqa: E731
      say('B=%d: (d) %s: sha256 parent %s, this %s, parent2 %s -- %s; parent %.4f ms, this %.4f '
          'ms, parent2 %.4f ms; this / parent = %.3f, parent2 / parent = %.3f (medians of the '
          'per-round ratios)' % (
              B, what, hashes['parent'][:16], hashes['this'][:16], hashes['parent2'][:16],
              'EQUAL' if len(set(hashes.values())) == 1 else 'DIFFERENT', med[0], med[1], med[2],
              ratio(1), ratio(2)))
    del net, variables, images, gt
    torch.cuda.empty_cache()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
