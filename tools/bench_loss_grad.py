"""Times the loss gradients (csrc/loss_grad.hip) on the device, warm, with HIP events, next to
the floor of anything that has to write the same bytes and next to torch's own autograd.

    python tools/bench_loss_grad.py [--repeats 50] [--torch_repeats 10] [--breakdown]
                                    [--out profiles/r20/loss_grad_bench.txt]

At B = 1 and B = 8 images of 640 x 480 (heads of 120 x 160 = 19200 pixels), 21 objects, 64
fragments -- 415 MB of gradient per image:
  (a) epos_loss_grads alone, all three heads;
  (b) epos_loss_terms + epos_loss_reduce + epos_loss_grads, one after the other on the stream;
  (c) the yardstick: hipMemsetAsync of the same three output buffers, in the same process.
      (a), (b) and (c) are timed INTERLEAVED -- one call of each per round, each between its
      own two events -- so that a drift of the machine meets all three alike; the medians of
      the rounds are reported;
  (d) torch's fp32 autograd on the device tensors: cross_entropy over the object rows, and
      over the gathered foreground rows, huber_loss on the gathered localisation values,
      backward to the three dense heads.
A quarter of the pixels is foreground, in blobs of one object, as a frame with a handful of
objects has them; a band at the top carries the ignore label (tools/bench_loss.py's maps).
--breakdown adds, per head and for all three: the launch writing that head alone, the same
launch with every pixel labelled background (zeros only, no value path), and the memset of
that head.
Before timing, (a) is compared with (d): fp32 against fp64-then-rounded, to 1e-5 relative.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_eval import label_maps      # noqa: E402

H, W, O, F = 120, 160, 21, 64
IGNORE = 255
WEIGHTS = (1.0, 1.0, 100.0)


def hip_runtime():
  """The HIP runtime torch has already mapped into this process (never a second copy)."""
  with open('/proc/self/maps') as f:
    paths = {line.split()[-1] for line in f if 'libamdhip64' in line}
  if not paths:
    raise RuntimeError('no HIP runtime is mapped: initialise torch.cuda first')
  rt = ctypes.CDLL(sorted(paths)[0])
  rt.hipMemsetAsync.restype = ctypes.c_int
  rt.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
  return rt


def torch_route(t, B):
  """The mean-over-images total loss in torch fp32 and its backward to the three heads."""
  import torch
  TF = torch.nn.functional
  total = 0.0
  for b in range(B):
    g = t['gt_obj'][b].reshape(-1).long()
    keep = g != IGNORE
    ce = TF.cross_entropy(t['obj'][b].reshape(-1, O + 1), torch.where(keep, g, 0),
                          reduction='none')
    total = total + WEIGHTS[0] * (ce * keep).mean()
    fg = torch.nonzero(keep & (g > 0)).reshape(-1)
    o, f = g[fg] - 1, t['gt_frag'][b].reshape(-1)[fg].long()
    rows = t['frag'][b].reshape(-1, O, F)[fg, o]
    total = total + WEIGHTS[1] * TF.cross_entropy(rows, f)
    pred = t['loc'][b].reshape(-1, O, F, 3)[fg, o, f]
    hub = TF.huber_loss(pred, t['gt_loc'][b].reshape(-1, 3)[fg], delta=1.0, reduction='none')
    total = total + WEIGHTS[2] * (hub * t['gt_weight'][b].reshape(-1)[fg, None]).mean()
  (total / B).backward()


def main():
  import torch
  from epos_amd import _lib
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=50)
  ap.add_argument('--torch_repeats', type=int, default=10)
  ap.add_argument('--breakdown', action='store_true')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  lib = _lib.load()
  torch.cuda.init()
  rt = hip_runtime()
  lines = ['loss gradients, %dx%d heads, %d objects, %d fragments; (a)-(c): medians of %d warm '
           'interleaved rounds (HIP events); (d): median of %d warm runs (HIP events)' % (
               W, H, O, F, args.repeats, args.torch_repeats)]

  def ptr(x):
    return ctypes.c_void_p(x.data_ptr())
  s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  P = H * W
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
    ws = torch.empty((lib.epos_loss_workspace_bytes(B, P, O, F) // 8,), dtype=torch.int64,
                     device='cuda')
    sums = torch.empty((B, O + 1, 3), dtype=torch.float64, device='cuda')
    counts = torch.empty((B, O + 1, 2), dtype=torch.int64, device='cuda')
    bad = torch.empty((B,), dtype=torch.int64, device='cuda')
    values = torch.empty((4,), dtype=torch.float64, device='cuda')
    scales = torch.empty((B, 3), dtype=torch.float64, device='cuda')
    outs = [torch.empty_like(t[k]) for k in ('obj', 'frag', 'loc')]
    out_bytes = sum(x.numel() * 4 for x in outs)

    def terms():
      _lib.check(lib.epos_loss_terms(
          ptr(t['obj']), O + 1, ptr(t['frag']), ptr(t['loc']), ptr(t['gt_obj']),
          ptr(t['gt_frag']), ptr(t['gt_loc']), ptr(t['gt_weight']), B, P, O, F, IGNORE, ptr(ws),
          ptr(sums), ptr(counts), ptr(bad), s))
      _lib.check(lib.epos_loss_reduce(ptr(sums), ptr(counts), B, O, WEIGHTS[0], WEIGHTS[1],
                                      WEIGHTS[2], 0, ptr(values), ptr(scales), s))

    def grads(need=(True, True, True), labels=None):
      d = [ptr(x) if n else None for x, n in zip(outs, need)]
      _lib.check(lib.epos_loss_grads(
          ptr(t['obj']), O + 1, ptr(t['frag']), ptr(t['loc']),
          ptr(t['gt_obj'] if labels is None else labels), ptr(t['gt_frag']), ptr(t['gt_loc']),
          ptr(t['gt_weight']), B, P, O, F, IGNORE, ptr(scales), None, d[0], O + 1, d[1], d[2], s))

    def both():
      terms()
      grads()

    def memset(need=(True, True, True)):
      for x, n in zip(outs, need):
        assert not n or rt.hipMemsetAsync(ptr(x), 0, x.numel() * 4, s) == 0

    def interleaved(fns):
      for fn in fns * 5:
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

    # (a) against (d) on the same tensors, before timing either
    for k in ('obj', 'frag', 'loc'):
      t[k].requires_grad_()
    torch_route(t, B)
    both()
    torch.cuda.synchronize()
    assert int(bad.sum()) == 0
    for k, d in zip(('obj', 'frag', 'loc'), outs):
      err = float((d - t[k].grad).abs().max())
      ref = float(t[k].grad.abs().max())
      assert err <= 1e-5 * ref, (k, err, ref)

    a_ms, b_ms, c_ms = interleaved((grads, both, memset))

    torch_ms = []
    for i in range(args.torch_repeats + 2):
      for k in ('obj', 'frag', 'loc'):
        t[k].grad = None
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      torch_route(t, B)
      b.record()
      b.synchronize()
      if i >= 2:
        torch_ms.append(a.elapsed_time(b))
    d_ms = float(np.median(torch_ms))
    fg = (t['gt_obj'] > 0) & (t['gt_obj'] <= O)
    line = ('B=%d (%d pixels, %.0f %% foreground), %.1f MB of gradient: (a) epos_loss_grads '
            '%.4f ms = %.0f GB/s written; (b) terms + reduce + grads %.4f ms; (c) hipMemsetAsync '
            'of the three buffers %.4f ms = %.0f GB/s; (a) / (c) = %.2f; (d) torch fp32 '
            'autograd, forward + backward, %.2f ms; (d) / (b) = %.1f' % (
                B, B * P, 100.0 * int(fg.sum()) / (B * P), out_bytes / 1e6, a_ms,
                out_bytes / a_ms / 1e6, b_ms, c_ms, out_bytes / c_ms / 1e6, a_ms / c_ms, d_ms,
                d_ms / b_ms))
    print(line, flush=True)
    lines.append(line)
    if args.breakdown:
      # one head at a time against the memset of that head, and the same launches with every
      # pixel background: no value path, only zeros
      background = torch.zeros_like(t['gt_obj'])
      for name, need in (('d_obj', (True, False, False)), ('d_frag', (False, True, False)),
                         ('d_loc', (False, False, True)), ('all', (True, True, True))):
        g_ms, z_ms, m_ms = interleaved((lambda: grads(need), lambda: grads(need, background),
                                        lambda: memset(need)))
        line = ('B=%d breakdown, %s: epos_loss_grads %.4f ms; with background-only labels '
                '%.4f ms; hipMemsetAsync %.4f ms' % (B, name, g_ms, z_ms, m_ms))
        print(line, flush=True)
        lines.append(line)
    del t, outs
    torch.cuda.empty_cache()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
