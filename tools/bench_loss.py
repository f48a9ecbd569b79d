"""Times the loss reduction (csrc/loss.hip) on the device, warm, with HIP events, next to the
route through the host.

    python tools/bench_loss.py [--repeats 50] [--host_repeats 3] [--out profiles/r19/loss_bench.txt]

At B = 1 and B = 8 images of 640 x 480 (heads of 120 x 160 = 19200 pixels), 21 objects, 64
fragments:
  (a) epos_loss_terms on the three dense heads and the four ground-truth maps: median of single
      calls (both launches) between two events;
  (b) the host route: download the three head tensors (413 MB per image) and the maps, and take
      the same sums in numpy fp64 (gathered rows, vectorised) -- a host clock around download +
      numpy, which ends synchronised by the download itself.
A quarter of the pixels is foreground, in blobs of one object, as a frame with a handful of
objects has them; a band at the top carries the ignore label.

The line states the bytes the call has to move, computed from the foreground share -- every
pixel's label, every counted pixel's O+1 object logits, every foreground pixel's fragment
label, weight, target, F fragment logits and 3 localisation values, and the workspace rows
written and read back -- next to the GB/s they imply, and the rate the same time would mean
had the launch read the dense heads. That the fragment heads of background, ignored and bad
pixels are not used is checked before timing: they are overwritten with NaN and the output
bytes stay the same.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_eval import label_maps, median_ms      # noqa: E402

H, W, O, F = 120, 160, 21, 64
IGNORE = 255


def host_route(t):
  """The sums of the header's rules in vectorised numpy fp64 on downloaded tensors:
  (sums [B,O+1,3], counts [B,O+1])."""
  obj, frag, loc = (t[k].cpu().numpy() for k in ('obj', 'frag', 'loc'))
  gt_obj, gt_frag = t['gt_obj'].cpu().numpy(), t['gt_frag'].cpu().numpy()
  gt_loc, gt_w = t['gt_loc'].cpu().numpy(), t['gt_weight'].cpu().numpy()
  B = gt_obj.shape[0]
  sums = np.zeros((B, O + 1, 3))
  counts = np.zeros((B, O + 1), np.int64)

  def ce(rows, target):
    rows = rows.astype(np.float64)
    m = rows.max(axis=1)
    s = np.exp(rows - m[:, None]).sum(axis=1)
    return np.log(s) + (m - rows[np.arange(len(rows)), target])
  for b in range(B):
    g = gt_obj[b].reshape(-1)
    keep = np.nonzero(g != IGNORE)[0]
    c_obj = ce(obj[b].reshape(-1, O + 1)[keep], g[keep])
    np.add.at(sums[b, :, 0], g[keep], c_obj)
    np.add.at(counts[b], g[keep], 1)
    fg = keep[g[keep] > 0]
    o, f = g[fg] - 1, gt_frag[b].reshape(-1)[fg]
    np.add.at(sums[b, :, 1], g[fg], ce(frag[b].reshape(-1, O, F)[fg, o], f))
    d = (loc[b].reshape(-1, O, F, 3)[fg, o, f].astype(np.float64) -
         gt_loc[b].reshape(-1, 3)[fg].astype(np.float64))
    hub = np.where(np.abs(d) <= 1.0, 0.5 * d * d, np.abs(d) - 0.5)
    np.add.at(sums[b, :, 2], g[fg],
              gt_w[b].reshape(-1)[fg].astype(np.float64) * ((hub[:, 0] + hub[:, 1]) + hub[:, 2]))
  return sums, counts


def main():
  import torch
  from epos_amd import _lib
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=50)
  ap.add_argument('--host_repeats', type=int, default=3)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  lib = _lib.load()
  lines = ['loss reduction, %dx%d heads, %d objects, %d fragments; (a): median of %d warm calls '
           '(HIP events); (b): median of %d host-clock runs' % (
               W, H, O, F, args.repeats, args.host_repeats)]

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
    ws_bytes = lib.epos_loss_workspace_bytes(B, P, O, F)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device='cuda')
    sums = torch.empty((B, O + 1, 3), dtype=torch.float64, device='cuda')
    counts = torch.empty((B, O + 1, 2), dtype=torch.int64, device='cuda')
    bad = torch.empty((B,), dtype=torch.int64, device='cuda')

    def terms():
      _lib.check(lib.epos_loss_terms(
          ptr(t['obj']), O + 1, ptr(t['frag']), ptr(t['loc']), ptr(t['gt_obj']),
          ptr(t['gt_frag']), ptr(t['gt_loc']), ptr(t['gt_weight']), B, P, O, F, IGNORE, ptr(ws),
          ptr(sums), ptr(counts), ptr(bad), s))
    # the device sums against the host route on the same tensors, before timing either
    terms()
    dev_sums, dev_counts = sums.cpu().numpy(), counts.cpu().numpy()
    h_sums, h_counts = host_route(t)
    assert int(bad.sum()) == 0 and np.array_equal(dev_counts[:, :, 0], h_counts)
    assert np.allclose(dev_sums, h_sums, rtol=1e-11, atol=0)
    # fragment values of pixels that are not foreground are not used: NaN there, same bytes
    fg = (t['gt_obj'] > 0) & (t['gt_obj'] <= O)
    keep_frag, keep_loc = t['frag'].clone(), t['loc'].clone()
    t['frag'][~fg] = float('nan')
    t['loc'][~fg] = float('nan')
    terms()
    assert sums.cpu().numpy().tobytes() == dev_sums.tobytes()
    t['frag'], t['loc'] = keep_frag, keep_loc
    a_ms = median_ms(terms, args.repeats)
    host = []
    for _ in range(args.host_repeats + 1):
      t0 = time.perf_counter()
      host_route(t)
      host.append(1e3 * (time.perf_counter() - t0))
    b_ms = float(np.median(host[1:]))
    n_fg = int(fg.sum())
    n_counted = int((t['gt_obj'] != IGNORE).sum())
    moved = (4 * B * P + 4 * (O + 1) * n_counted + n_fg * (4 + 4 + 12 + 4 * F + 12) +
             2 * ws_bytes + 8 * B * (5 * (O + 1) + 1))
    dense = 4 * B * P * ((O + 1) + 4 * O * F)
    line = ('B=%d (%d pixels, %.0f %% foreground): (a) epos_loss_terms %.4f ms; the call has to '
            'move %.2f MB (from the foreground share; workspace %.2f MB), i.e. %.1f GB/s; the '
            'dense heads are %.1f MB, which in that time would be %.0f GB/s; (b) download + '
            'numpy on the host %.1f ms; (b) / (a) = %.0f' % (
                B, B * P, 100.0 * n_fg / (B * P), a_ms, moved / 1e6, ws_bytes / 1e6,
                moved / a_ms / 1e6, dense / 1e6, dense / a_ms / 1e6, b_ms, b_ms / a_ms))
    print(line, flush=True)
    lines.append(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
