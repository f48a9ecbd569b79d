"""Numpy restatement of the loss sums (csrc/loss.hip; include/epos_hip.h, "Losses") and of the
per-image and dataset formulas of epos_amd/loss.py, written from that description in its order:
plain loops in fp64, no shared code with the package."""
import math

import numpy as np

NAMES = ('obj_cls_loss', 'frag_cls_loss', 'frag_loc_loss', 'total_loss')


def row_lengths(num_objs, num_frags):
  """(values per object row, values per fragment row): the row length of the cross-entropy
  tolerance."""
  return num_objs + 1, num_frags


def cross_entropy(row, target):
  """ce = log(sum_c exp(x_c - m)) + (m - x_target), m = max x, the sum in index order, in fp64
  on the fp32 values."""
  x = [float(v) for v in np.asarray(row, np.float32)]
  m = float(np.max(np.asarray(row, np.float32)))      # a NaN stays a NaN
  s = 0.0
  for v in x:
    d = v - m
    s += d if d != d else math.exp(d)
  return (math.log(s) if s == s and s > 0.0 else float('nan')) + (m - x[target])


def huber(d):
  """tf.losses.huber_loss with delta = 1 on one difference."""
  a = abs(d)
  return 0.5 * d * d if a <= 1.0 else a - 0.5


def pixel_terms(obj_row, frag_rows, loc_rows, g, f, loc, weight, num_objs, num_frags, ignore):
  """One pixel: ('ignored',) | ('bad',) | ('ok', g, ce_obj, ce_frag, hub). frag_rows [O,F] and
  loc_rows [O,F,3] are only indexed where the rules read them."""
  if g == ignore:
    return ('ignored',)
  if g < 0 or g > num_objs:
    return ('bad',)
  if g >= 1:
    w = float(np.float32(weight))
    if f < 0 or f > num_frags - 1 or not (w > 0.0 and math.isfinite(w)):
      return ('bad',)
  ce_obj = cross_entropy(obj_row, g)
  if g == 0:
    return ('ok', 0, ce_obj, 0.0, 0.0)
  ce_frag = cross_entropy(frag_rows[g - 1], f)
  hub = [huber(float(loc_rows[g - 1, f, k]) - float(loc[k])) for k in range(3)]
  return ('ok', g, ce_obj, ce_frag, w * ((hub[0] + hub[1]) + hub[2]))


def terms(obj_logits, frag_logits, frag_loc, gt_obj, gt_frag, gt_loc, gt_weight, ignore, share):
  """(sums f64 [B,O+1,3], counts i64 [B,O+1,2], bad i64 [B]) of obj_logits [B,P,O+1],
  frag_logits [B,P,O,F], frag_loc [B,P,O,F,3], gt_obj / gt_frag / gt_weight [B,P] and gt_loc
  [B,P,3]. share = pixels per share: every share is summed in pixel order from 0.0, then the
  shares of an image in share order from 0.0."""
  obj_logits = np.asarray(obj_logits, np.float32)
  frag_logits = np.asarray(frag_logits, np.float32)
  frag_loc = np.asarray(frag_loc, np.float32)
  gt_loc = np.asarray(gt_loc, np.float32)
  B, P, O1 = obj_logits.shape
  O, F = frag_logits.shape[2], frag_logits.shape[3]
  assert O1 == O + 1 and frag_loc.shape == (B, P, O, F, 3)
  sums = np.zeros((B, O1, 3), np.float64)
  counts = np.zeros((B, O1, 2), np.int64)
  bad = np.zeros((B,), np.int64)
  for b in range(B):
    for p0 in range(0, P, share):
      part = [[0.0, 0.0, 0.0] for _ in range(O1)]
      for p in range(p0, min(p0 + share, P)):
        t = pixel_terms(obj_logits[b, p], frag_logits[b, p], frag_loc[b, p], int(gt_obj[b, p]),
                        int(gt_frag[b, p]), gt_loc[b, p], gt_weight[b, p], O, F, ignore)
        if t[0] == 'ignored':
          counts[b, 0, 1] += 1
        elif t[0] == 'bad':
          bad[b] += 1
        else:
          g = t[1]
          counts[b, g, 0] += 1
          for k in range(3):
            part[g][k] += t[2 + k]
      for g in range(O1):
        for k in range(3):
          sums[b, g, k] += part[g][k]
  return sums, counts, bad


def image_losses(sums, counts, weights=(1.0, 1.0, 100.0)):
  """The reference's losses of ONE image as a batch of one (loss.py:149,224-229,298-303) from
  its sums [O+1,3] and counts [O+1,2]: the object loss is a mean over all P pixels, ignored
  ones included; the fragment losses are means over the n_fg foreground pixels (and their 3
  coordinates), 0 without foreground; the objects are added in index order."""
  w_obj, w_cls, w_loc = weights
  O1 = sums.shape[0]
  P = int(counts[:, 0].sum()) + int(counts[0, 1])
  n_fg = int(counts[1:, 0].sum())
  s = [0.0, 0.0, 0.0]
  for g in range(O1):
    s[0] += float(sums[g, 0])
    if g >= 1:
      s[1] += float(sums[g, 1])
      s[2] += float(sums[g, 2])
  out = {'obj_cls_loss': w_obj * (s[0] / P),
         'frag_cls_loss': w_cls * (s[1] / n_fg) if n_fg else 0.0,
         'frag_loc_loss': w_loc * (s[2] / (3 * n_fg)) if n_fg else 0.0}
  out['total_loss'] = (out['obj_cls_loss'] + out['frag_cls_loss']) + out['frag_loc_loss']
  return out


def dataset_losses(sums, counts, weights=(1.0, 1.0, 100.0)):
  """{'per_image', 'mean', 'pooled', 'per_object'} of sums [N,O+1,3] and counts [N,O+1,2]:
  mean = the mean over the images of each loss (added in image order); pooled = dataset sums
  over dataset counts; per_object = the pooled fragment losses and the pixel count of each
  object id."""
  w_obj, w_cls, w_loc = weights
  N, O1 = sums.shape[0], sums.shape[1]
  per_image = [image_losses(sums[i], counts[i], weights) for i in range(N)]
  mean = {}
  for name in NAMES:
    acc = 0.0
    for r in per_image:
      acc += r[name]
    mean[name] = acc / N
  tot = np.zeros((O1, 3), np.float64)
  n = np.zeros((O1,), np.int64)
  pixels = 0
  for i in range(N):
    tot += sums[i]
    n += counts[i, :, 0]
    pixels += int(counts[i, :, 0].sum()) + int(counts[i, 0, 1])
  pooled = image_losses(tot, np.stack([n, np.zeros_like(n)], axis=1), weights)
  obj_sum = 0.0
  for g in range(O1):
    obj_sum += float(tot[g, 0])
  pooled['obj_cls_loss'] = w_obj * (obj_sum / pixels)
  pooled['total_loss'] = ((pooled['obj_cls_loss'] + pooled['frag_cls_loss']) +
                          pooled['frag_loc_loss'])
  per_object = {}
  for g in range(1, O1):
    c = int(n[g])
    per_object[g] = {'frag_cls_loss': w_cls * (float(tot[g, 1]) / c) if c else 0.0,
                     'frag_loc_loss': w_loc * (float(tot[g, 2]) / (3 * c)) if c else 0.0,
                     'pixels': c}
  return {'per_image': per_image, 'mean': mean, 'pooled': pooled, 'per_object': per_object}


def ce_bound(row_len, n, ref):
  """The tolerance of a cross-entropy sum of n terms with value ref over rows of row_len
  values: one rounding per added exponential, a few ulp for exp and log in either library,
  non-negative terms throughout."""
  return (row_len + 16) * 2.0 ** -52 * (n + ref)
