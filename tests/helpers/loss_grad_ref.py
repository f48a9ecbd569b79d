"""Numpy restatement of the loss gradients and of the gradient factors (csrc/loss_grad.hip;
include/epos_hip.h, "Losses"), written from that description: plain loops in fp64, rounded to
fp32 once, no shared code with the package. The class of a pixel is loss_ref.pixel_terms'."""
import math

import numpy as np

from tests.helpers import loss_ref

MEAN, POOLED = 0, 1


def scales(counts, weights, reduction):
  """f64 [B,3] from counts i64 [B,O+1,2]: per image { w_obj / (P_b * B), w_cls / (n_b * B),
  w_loc / (3 * n_b * B) } for the mean over the images, { w_obj / sum P, w_cls / N_fg,
  w_loc / (3 N_fg) } for the pooled batch; a fragment factor without foreground is 0."""
  w_obj, w_cls, w_loc = weights
  B = counts.shape[0]
  pix = [int(counts[b, :, 0].sum()) + int(counts[b, 0, 1]) for b in range(B)]
  fg = [int(counts[b, 1:, 0].sum()) for b in range(B)]
  out = np.zeros((B, 3), np.float64)
  for b in range(B):
    if reduction == MEAN:
      d = (pix[b] * B, fg[b] * B, 3 * fg[b] * B)
    else:
      d = (sum(pix), sum(fg), 3 * sum(fg))
    out[b] = [w / n if n else 0.0 for w, n in zip((w_obj, w_cls, w_loc), d)]
  return out


def softmax_minus_one_hot(row, target):
  """[exp(x_c - m) / S - [c == target]] in fp64 on the fp32 values, m = max x, S added in
  index order."""
  x = [float(v) for v in np.asarray(row, np.float32)]
  m = float(np.max(np.asarray(row, np.float32)))      # a NaN stays a NaN
  e = []
  for v in x:
    d = v - m
    e.append(d if d != d else math.exp(d))
  s = 0.0
  for v in e:
    s += v
  if not (s == s and s > 0.0):
    return [float('nan')] * len(x)
  return [v / s - (1.0 if c == target else 0.0) for c, v in enumerate(e)]


def clamp1(d):
  """The derivative of loss_ref.huber: d inside [-1, 1], knee included, else its sign."""
  return 1.0 if d > 1.0 else -1.0 if d < -1.0 else d


def upstream_factors(upstream):
  """u_k = upstream[k] + upstream[3]; None is {0, 0, 0, 1}."""
  if upstream is None:
    return [1.0, 1.0, 1.0]
  return [float(upstream[k]) + float(upstream[3]) for k in range(3)]


def grads(c, scale, upstream=None, ignore=255, rounded=True):
  """(d_obj [B,P,O+1], d_frag [B,P,O,F], d_loc [B,P,O,F,3]) of a loss_cases case: fp32 when
  rounded (fl32 of the fp64 product, once), the fp64 values themselves otherwise."""
  obj = np.asarray(c['obj_logits'], np.float32)
  frag = np.asarray(c['frag_logits'], np.float32)
  loc = np.asarray(c['frag_loc'], np.float32)
  gt_loc = np.asarray(c['gt_loc'], np.float32)
  B, P, O1 = obj.shape
  O, F = frag.shape[2], frag.shape[3]
  u = upstream_factors(upstream)
  d_obj = np.zeros(obj.shape, np.float64)
  d_frag = np.zeros(frag.shape, np.float64)
  d_loc = np.zeros(loc.shape, np.float64)
  for b in range(B):
    s = [float(scale[b, k]) * u[k] for k in range(3)]
    for p in range(P):
      g, f = int(c['gt_obj'][b, p]), int(c['gt_frag'][b, p])
      w = c['gt_weight'][b, p]
      t = loss_ref.pixel_terms(obj[b, p], frag[b, p], loc[b, p], g, f, gt_loc[b, p], w, O, F,
                               ignore)
      if t[0] != 'ok':
        continue
      for k, v in enumerate(softmax_minus_one_hot(obj[b, p], g)):
        d_obj[b, p, k] = s[0] * v
      if g == 0:
        continue
      for k, v in enumerate(softmax_minus_one_hot(frag[b, p, g - 1], f)):
        d_frag[b, p, g - 1, k] = s[1] * v
      for k in range(3):
        d = float(loc[b, p, g - 1, f, k]) - float(gt_loc[b, p, k])
        d_loc[b, p, g - 1, f, k] = s[2] * (float(np.float32(w)) * clamp1(d))
  if not rounded:
    return d_obj, d_frag, d_loc
  with np.errstate(over='ignore', invalid='ignore'):
    return d_obj.astype(np.float32), d_frag.astype(np.float32), d_loc.astype(np.float32)


def active_masks(c, ignore=255):
  """Boolean arrays shaped like the three gradients: the elements the rules give a value.
  Every other element is +0.0."""
  B, P, O1 = c['obj_logits'].shape
  O, F = c['frag_logits'].shape[2], c['frag_logits'].shape[3]
  m_obj = np.zeros((B, P, O1), bool)
  m_frag = np.zeros((B, P, O, F), bool)
  m_loc = np.zeros((B, P, O, F, 3), bool)
  for b in range(B):
    for p in range(P):
      g, f = int(c['gt_obj'][b, p]), int(c['gt_frag'][b, p])
      w = float(np.float32(c['gt_weight'][b, p]))
      if g == ignore or g < 0 or g > O:
        continue
      if g >= 1 and (f < 0 or f > F - 1 or not (w > 0.0 and math.isfinite(w))):
        continue
      m_obj[b, p] = True
      if g >= 1:
        m_frag[b, p, g - 1] = True
        m_loc[b, p, g - 1, f] = True
  return m_obj, m_frag, m_loc


def bound(ref, s_k, row_len):
  """|got - ref| <= 2^-23 |ref| + |s_k| (row_len + 16) 2^-52 + 2^-149 for a softmax element:
  the fp64 probability differs by the order of S only, one rounding per added exponential plus
  a few ulp of exp, an absolute error of at most (row_len + 16) 2^-52 on a value <= 1; two fp32
  roundings of values that close differ by at most one ulp."""
  return 2.0 ** -23 * np.abs(ref.astype(np.float64)) + abs(s_k) * (row_len + 16) * 2.0 ** -52 + \
      2.0 ** -149
