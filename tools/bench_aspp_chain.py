"""Times the backward pass through ASPP (csrc/aspp_grad.hip and the existing gradient kernels at
the widths trainer.aspp_grads brings) on the device, warm, with HIP events.

    python tools/bench_aspp_chain.py --build-parent [--parent-rev HEAD~1]   # where git and hipcc are
    python tools/bench_aspp_chain.py [--repeats 30] [--out profiles/r31/aspp_chain_bench.txt]

At C2's sizes -- encoder 60 x 80, ec = 2048, rates 12 / 24 / 36 -- for B = 1 and 8, all candidates
of a group INTERLEAVED in one process (one call of each per round, each between its own two
events), medians of the rounds:
  (a) epos_aspp_join_dgrad_f32 in ASPP's case (three depthwise terms, one plain, the per-image
      term, the mask) in each partition built, next to a device copy of its compulsory bytes (six
      tensors of B 60 80 2048 floats);
  (b) the same against the unfused route on the same inputs: three depthwise_input_grad calls,
      torch additions of the five terms and a torch.where for the mask. THE GATE: the shipped
      partition must not be slower than that route at either batch size (exit status 1);
  (c) epos_pool_broadcast_dgrad_f32 on a 256-wide slice of a 1280-wide buffer next to a copy of
      its bytes and next to torch's sum(1);
  (d) the existing kernels at their new widths, through their wrappers with an fp32 A:
      pointwise_input_grad at K x N = 1280 x 256 and 2048 x 256, pointwise_weight_grads at 2048 x
      256 with M = rows and M = B, the depthwise sums and input gradient at C = 2048;
  (e) on a 640 x 480 net with 21 objects and 64 fragments, after a forward_logits:
      trainer.decoder_grads against trainer.aspp_grads;
  (f) with the parent commit's library (--build-parent) swapped in under the same Python:
      trainer.decoder_grads -- a sha256 of every output per library, and the times of this build
      over the parent's next to parent2 over parent, the spread of the measurement.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_decoder_chain import digest, open_library   # noqa: E402
from tools.bench_eval import label_maps                      # noqa: E402
from tools.bench_knn import build_parent, parent_paths       # noqa: E402

H, W, O, F = 480, 640, 21, 64
EH, EW, EC, DH, DW = 60, 80, 2048, 120, 160
RATES = (12, 24, 36)
IGNORE = 255


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=30)
  ap.add_argument('--batches', default='1,8')
  ap.add_argument('--groups', default='abcdef')
  ap.add_argument('--out', default=None)
  ap.add_argument('--build-parent', action='store_true')
  ap.add_argument('--parent-rev', default='HEAD~1')
  args = ap.parse_args()
  if args.build_parent:
    build_parent(args.parent_rev)
    return 0
  import torch
  from epos_amd import _lib, decoder_train as DT, net as enet, synthetic, trainer, weights
  batches = [int(b) for b in args.batches.split(',')]
  lib = _lib.load()
  torch.cuda.init()
  lines = ['backward through ASPP, encoder %dx%d, ec = %d, rates %s; medians of %d warm '
           'interleaved rounds (HIP events)' % (EH, EW, EC, RATES, args.repeats)]
  slower = []

  def say(line):
    print(line, flush=True)
    lines.append(line)

  def interleaved(fns, all_rounds=False):
    for fn in tuple(fns) * 3:
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

  def randn(*shape, scale=1.0):
    return scale * torch.randn(shape, device='cuda')

  for B in batches:
    M = B * EH * EW
    n = M * EC
    if set('ab') & set(args.groups):
      # ---- (a), (b) the join
      Ds = [randn(B, EH, EW, EC, scale=1e-3) for _ in RATES]
      w9 = [randn(9, EC, scale=0.3) for _ in RATES]
      E0 = randn(B, EH, EW, EC, scale=1e-3)
      pool = randn(B, EC, scale=1e-3)
      Y = torch.relu(randn(B, EH, EW, EC))
      out = torch.empty((B, EH, EW, EC), device='cuda')
      terms = list(zip(Ds, w9, RATES))
      partitions = ('shipped', 'pixel', 'slice32', 'slice64', 'slice32x2', 'slice32x4')

      def fused(partition):
        return lambda: DT.aspp_join_grad(depthwise=terms, plain=[E0], pooled=(pool, EH * EW),
                                         relu_of=Y, out=out, partition=partition)
      tmp = [torch.empty((B, EH, EW, EC), device='cuda') for _ in RATES]
      acc = torch.empty((B, EH, EW, EC), device='cuda')
      zero = torch.zeros((), device='cuda')
      got = [None]

      def unfused():
        for d, w, r, t in zip(Ds, w9, RATES, tmp):
          DT.depthwise_input_grad(d, w, rate=r, out=t)
        torch.add(E0, tmp[0], out=acc)
        acc.add_(tmp[1]).add_(tmp[2]).add_((pool / (EH * EW))[:, None, None, :])
        got[0] = torch.where(Y <= 0, zero, acc)
      move = torch.empty((2, 3 * n), device='cuda')          # 3 n read + 3 n written = 6 tensors

      def copy6():
        move[1].copy_(move[0])
      fused('shipped')()
      unfused()
      torch.cuda.synchronize()
      diff = float((out - got[0]).abs().max() / got[0].abs().max())
      assert diff < 1e-5, diff
      res = interleaved([fused(p) for p in partitions] + [copy6, unfused])
      gb = 6 * 4.0 * n / 1e9
      by = dict(zip(partitions, res))
      t_copy, t_un = res[-2], res[-1]
      say('B=%d: (a) epos_aspp_join_dgrad_f32 (3 depthwise + 1 plain + pool + mask, %.0f MB '
          'compulsory) ' % (B, gb * 1e3) + '; '.join(
              '%s %.4f ms (%.0f GB/s)' % (p, by[p], gb / by[p] * 1e3) for p in partitions) +
          '; a device copy moving as many bytes %.4f ms (%.0f GB/s); shipped / copy = %.2f' % (
              t_copy, gb / t_copy * 1e3, by['shipped'] / t_copy))
      # the unfused route: 3 x (D read, dX written) + add (2 r, 1 w) + 2 in-place adds (2 r, 1 w)
      # + the broadcast add (1 r, 1 w) + where (2 r, 1 w) = 19 tensor-sized transfers
      say('B=%d: (b) the unfused route (3 depthwise_input_grad, torch additions, torch.where; 19 '
          'tensor-sized transfers against 6) %.4f ms; shipped / unfused = %.3f; largest '
          'difference %.1e of the largest gradient' % (B, t_un, by['shipped'] / t_un, diff))
      if by['shipped'] > t_un:
        slower.append((B, by['shipped'], t_un))
      del Ds, E0, Y, out, tmp, acc, move, got
      torch.cuda.empty_cache()

    if 'c' in args.groups:
      # ---- (c) the broadcast's adjoint, on slice 0 of the concat's gradient
      cat = randn(B, EH * EW, 1280, scale=1e-3)
      d = cat[..., :256]
      g = torch.empty((B, 256), device='cuda')
      ws = torch.empty((max(DT.pool_workspace_bytes(B, EH * EW, 256) // 8, 1),),
                       dtype=torch.float64, device='cuda')
      move = torch.empty((2, B * EH * EW * 256 // 2), device='cuda')
      got = [None]

      def pool_k():
        DT.pool_broadcast_grad(d, out=g, workspace=ws)

      def pool_t():
        got[0] = d.sum(1)

      def pool_c():
        move[1].copy_(move[0])
      t_k, t_t, t_c = interleaved((pool_k, pool_t, pool_c))
      diff = float((g - got[0]).abs().max() / got[0].abs().max())
      say('B=%d: (c) epos_pool_broadcast_dgrad_f32 [%d,%d,256 of 1280] %.4f ms; torch sum(1) '
          '%.4f ms; a copy of its bytes %.4f ms; largest difference %.1e' % (
              B, B, EH * EW, t_k, t_t, t_c, diff))
      del cat, move

    if 'd' in args.groups:
      # ---- (d) the existing kernels at their new widths
      G = randn(M, 256, scale=1e-3)
      bn2 = (randn(256), 0.5 + torch.rand(256, device='cuda'))
      bn3 = (randn(256), randn(256), 0.5 + torch.rand(256, device='cuda'))
      wsd = torch.empty((lib.epos_pointwise_dgrad_workspace_bytes(1024, 256) // 8,),
                        dtype=torch.float64, device='cuda')
      fns, names = [], []
      for K in (1280, 2048):
        Wt, A, D = randn(K, 256, scale=0.06), torch.relu(randn(M, K)), torch.empty((M, K),
                                                                                   device='cuda')
        fns.append(lambda Wt=Wt, A=A, D=D: DT.pointwise_input_grad(
            G, Wt, bn=bn2, eps=1e-5, relu_of=A, out=D, workspace=wsd))
        names.append('pointwise_input_grad M=%d K=%d N=256 (fp32 mask)' % (M, K))
      A, Wt = torch.relu(randn(M, EC)), randn(EC, 256, scale=0.06)
      for rows in (M, B):
        ws = torch.empty((DT.workspace_words(rows, EC, 256),), dtype=torch.int64, device='cuda')
        fns.append(lambda rows=rows, ws=ws: DT.pointwise_weight_grads(
            A[:rows], G[:rows], Wt, bn=bn3, eps=1e-5, workspace=ws))
        names.append('pointwise_weight_grads M=%d 2048x256 (closing included)' % rows)
      X, D4 = A.view(B, EH, EW, EC), randn(B, EH, EW, EC, scale=1e-3)
      w33, w9c = randn(3, 3, EC, 1, scale=0.3), randn(9, EC, scale=0.3)
      bnc = (randn(EC), randn(EC), 0.5 + torch.rand(EC, device='cuda'))
      wsw = torch.empty((DT.depthwise_workspace_words(B, EH, EW, EC),), dtype=torch.int64,
                        device='cuda')
      dX = torch.empty((B, EH, EW, EC), device='cuda')
      for r in RATES:
        fns.append(lambda r=r: DT.depthwise_weight_grads(X, D4, w33, bnc, 1e-5, rate=r,
                                                         workspace=wsw))
        names.append('depthwise_weight_grads C=2048 rate %d' % r)
        fns.append(lambda r=r: DT.depthwise_input_grad(D4, w9c, rate=r, relu_of=X, out=dX))
        names.append('depthwise_input_grad C=2048 rate %d' % r)
      res = interleaved(fns)
      say('B=%d: (d) ' % B + '; '.join('%s %.4f ms' % (nm, t) for nm, t in zip(names, res)))
      del fns, A, X, D4, dX, G
      torch.cuda.empty_cache()

  # ---- (e), (f): from a running net
  if set('ef') & set(args.groups):
    parents = [open_library(p) if os.path.exists(p) else None for p in parent_paths()]
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
            'frag_label': torch.randint(0, F, (B, DH, DW), dtype=torch.int32, device='cuda'),
            'frag_loc': torch.randn((B, DH, DW, 3), device='cuda'),
            'frag_weight': torch.ones((B, DH, DW), device='cuda')}
      net.forward_logits(images, use_graph=True)

      def decoder():
        return trainer.decoder_grads(net, gt, variables)

      def aspp():
        return trainer.aspp_grads(net, gt, variables)
      if 'e' in args.groups:
        d_ms, a_ms = interleaved((decoder, aspp))
        say('B=%d, %dx%d: (e) decoder_grads %.4f ms; aspp_grads %.4f ms; the %d new gradients '
            'and d_enc add %.4f ms' % (B, W, H, d_ms, a_ms, 3 * (2 + 2 * len(RATES)),
                                       a_ms - d_ms))
      if 'f' not in args.groups:
        continue
      if None in parents:
        say('B=%d: (f) not measured: build the parent library first (--build-parent)' % B)
        continue

      def under(handle, fn):
        def run():
          keep, _lib._lib = _lib._lib, handle
          try:
            return fn()
          finally:
            _lib._lib = keep
        return run

      def flat(result):
        return [result[0], result[1]] + [result[2][n] for n in sorted(result[2])] + [result[3]]
      builds = (('parent', parents[0]), ('this', lib), ('parent2', parents[1]))
      hashes = {}
      for name, handle in builds:
        res = under(handle, decoder)()
        torch.cuda.synchronize()
        hashes[name] = digest(flat(res))
      rounds = interleaved(tuple(under(handle, decoder) for _, handle in builds), all_rounds=True)
      med = [float(np.median(ts)) for ts in rounds]
      ratio = lambda i: float(np.median(np.asarray(rounds[i]) / np.asarray(rounds[0])))  # noqa: E731
      say('B=%d: (f) decoder_grads: sha256 parent %s, this %s, parent2 %s -- %s; parent %.4f ms, '
          'this %.4f ms, parent2 %.4f ms; this / parent = %.3f, parent2 / parent = %.3f (medians '
          'of the per-round ratios)' % (
              B, hashes['parent'][:16], hashes['this'][:16], hashes['parent2'][:16],
              'EQUAL' if len(set(hashes.values())) == 1 else 'DIFFERENT', med[0], med[1], med[2],
              ratio(1), ratio(2)))
      del net, variables, images, gt
      torch.cuda.empty_cache()
  for B, t_f, t_u in slower:
    say('GATE (b) MISSED at B=%d: the shipped partition %.4f ms, the unfused route %.4f ms' % (
        B, t_f, t_u))
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')
  return 1 if slower else 0


if __name__ == '__main__':
  sys.exit(main())
