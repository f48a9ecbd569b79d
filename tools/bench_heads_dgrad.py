"""Times the logits layers' input gradient (csrc/heads_dgrad.hip) on the device, warm, with HIP
events, next to the dense route and next to the floor of anything that writes dX once.

    python tools/bench_heads_dgrad.py [--repeats 30] [--out profiles/r24/heads_dgrad_bench.txt]

At B = 1 and B = 8 images of 640 x 480 (heads of 120 x 160 = 19200 pixels), 21 objects, 64
fragments, K = 256 features, fp32:
  (a) epos_heads_dgrad_f32 with the transposition of the three weight matrices in front of it
      (three torch copies of W.t() into one buffer, as heads_train.heads_input_grad makes them);
  (b) the dense route: epos_loss_grads (415 MB of gradient per image) followed by three torch
      fp32 matmuls d_h @ W_h.t(), summed, on the same tensors;
  (c) the floor: a device memset of dX.
(a), (b) and (c) are timed INTERLEAVED -- one call of each per round, each between its own two
events -- so that a drift of the machine meets all three alike; the medians of the rounds are
reported, and the breakdown of (a) and of (b) by stage likewise.
A quarter of the pixels is foreground, in blobs of one object, as a frame with a handful of
objects has them; a band at the top carries the ignore label (tools/bench_loss.py's maps).
Before timing, (a) is compared with (b): fp64 sums against fp32 matmuls, to 1e-3 of the largest
element.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_eval import label_maps      # noqa: E402

H, W, O, F, K = 120, 160, 21, 64, 256
IGNORE = 255
WEIGHTS = (1.0, 1.0, 100.0)


def main():
  import torch
  from epos_amd import _lib
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=30)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  lib = _lib.load()
  torch.cuda.init()
  lines = ['input gradient of the logits layers, %dx%d heads, %d objects, %d fragments, K = %d; '
           'medians of %d warm interleaved rounds (HIP events)' % (W, H, O, F, K, args.repeats)]

  def ptr(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else None
  s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  P = H * W
  widths = (O + 1, O * F, O * F * 3)
  starts = (0, widths[0], widths[0] + widths[1], sum(widths))
  Ws = [0.05 * torch.randn((K, n), device='cuda') for n in widths]      # the checkpoint layout
  wt = torch.empty((sum(widths), K), device='cuda')
  for B in (1, 8):
    gt_h, _ = label_maps(B, B)
    gt_h[:, :6] = IGNORE
    t = {'gt_obj': torch.from_numpy(gt_h).cuda(),
         'gt_frag': torch.randint(0, F, (B, H, W), dtype=torch.int32, device='cuda'),
         'gt_loc': torch.randn((B, H, W, 3), device='cuda'),
         'gt_weight': torch.ones((B, H, W), device='cuda'),
         'obj': 4 * torch.randn((B, H, W, O + 1), device='cuda'),
         'frag': 4 * torch.randn((B, H, W, O, F), device='cuda'),
         'loc': torch.randn((B, H, W, O, F, 3), device='cuda')}
    lws = torch.empty((lib.epos_loss_workspace_bytes(B, P, O, F) // 8,), dtype=torch.int64,
                      device='cuda')
    sums = torch.empty((B, O + 1, 3), dtype=torch.float64, device='cuda')
    counts = torch.empty((B, O + 1, 2), dtype=torch.int64, device='cuda')
    bad = torch.empty((B,), dtype=torch.int64, device='cuda')
    values = torch.empty((4,), dtype=torch.float64, device='cuda')
    scales = torch.empty((B, 3), dtype=torch.float64, device='cuda')
    _lib.check(lib.epos_loss_terms(
        ptr(t['obj']), O + 1, ptr(t['frag']), ptr(t['loc']), ptr(t['gt_obj']), ptr(t['gt_frag']),
        ptr(t['gt_loc']), ptr(t['gt_weight']), B, P, O, F, IGNORE, ptr(lws), ptr(sums),
        ptr(counts), ptr(bad), s))
    _lib.check(lib.epos_loss_reduce(ptr(sums), ptr(counts), B, O, WEIGHTS[0], WEIGHTS[1],
                                    WEIGHTS[2], 1, ptr(values), ptr(scales), s))
    dX = torch.empty((B * P, K), device='cuda')
    d = [torch.empty_like(t[k]) for k in ('obj', 'frag', 'loc')]
    dense = [None]

    def transpose():
      for k in range(3):
        wt[starts[k]:starts[k + 1]].copy_(Ws[k].t())

    def kernel():
      _lib.check(lib.epos_heads_dgrad_f32(
          ptr(t['obj']), O + 1, ptr(t['frag']), ptr(t['loc']), ptr(t['gt_obj']),
          ptr(t['gt_frag']), ptr(t['gt_loc']), ptr(t['gt_weight']), B, P, O, F, IGNORE,
          ptr(scales), None, ptr(wt[starts[0]:]), ptr(wt[starts[1]:]), ptr(wt[starts[2]:]), K, K,
          None, 0, ptr(dX), K, s))

    def dgrad():
      transpose()
      kernel()

    def loss_grads():
      _lib.check(lib.epos_loss_grads(
          ptr(t['obj']), O + 1, ptr(t['frag']), ptr(t['loc']), ptr(t['gt_obj']),
          ptr(t['gt_frag']), ptr(t['gt_loc']), ptr(t['gt_weight']), B, P, O, F, IGNORE,
          ptr(scales), None, ptr(d[0]), O + 1, ptr(d[1]), ptr(d[2]), s))

    def matmuls():
      acc = d[0].view(B * P, widths[0]) @ Ws[0].t()
      for k in (1, 2):
        acc = acc + d[k].view(B * P, widths[k]) @ Ws[k].t()
      dense[0] = acc

    def dense_route():
      loss_grads()
      matmuls()

    def floor():
      dX.zero_()

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

    # (a) against (b) on the same tensors, before timing either
    dgrad()
    dense_route()
    torch.cuda.synchronize()
    assert int(bad.sum()) == 0
    err, ref = float((dX - dense[0]).abs().max()), float(dense[0].abs().max())
    assert ref > 0 and err <= 1e-3 * ref, (err, ref)

    # the floor last in a round: its zeros are overwritten by the next round's (a)
    a_ms, b_ms, c_ms = interleaved((dgrad, dense_route, floor))
    fg = (t['gt_obj'] > 0) & (t['gt_obj'] <= O)
    line = ('B=%d (%d pixels, %.0f %% foreground): (a) weight transposition + '
            'epos_heads_dgrad_f32 %.4f ms; (b) epos_loss_grads + three fp32 matmuls, summed '
            '%.4f ms; (c) memset of dX, %.1f MB, %.4f ms; (b) / (a) = %.2f; (a) / (c) = %.1f' % (
                B, B * P, 100.0 * int(fg.sum()) / (B * P), a_ms, b_ms,
                dX.numel() * 4 / 1e6, c_ms, b_ms / a_ms, a_ms / c_ms))
    print(line, flush=True)
    lines.append(line)
    t_ms, k_ms, g_ms, m_ms = interleaved((transpose, kernel, loss_grads, matmuls))
    line = ('B=%d breakdown: (a) transposition %.4f ms, epos_heads_dgrad_f32 alone %.4f ms; '
            '(b) epos_loss_grads %.4f ms, matmuls and sums %.4f ms' % (B, t_ms, k_ms, g_ms, m_ms))
    print(line, flush=True)
    lines.append(line)
    del t, d, dense, dX
    torch.cuda.empty_cache()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
