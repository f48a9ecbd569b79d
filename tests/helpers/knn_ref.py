"""Numpy restatement of the rules of include/epos_hip.h, "k nearest fragments": the ground truth
with knn slots per pixel, the loss sums, the gradient factors, the logit gradients and the
logits layers' weight and input gradients over them. Plain loops in fp64, written from that
description; what the section leaves unchanged is imported from loss_ref, loss_grad_ref,
heads_wgrad_ref and heads_dgrad_ref. No shared code with the package."""
import math

import numpy as np

from tests.helpers import heads_dgrad_ref, heads_wgrad_ref, loss_cases, loss_grad_ref, loss_ref

MAX_KNN = 4
MEAN, POOLED = loss_grad_ref.MEAN, loss_grad_ref.POOLED
NAMES = loss_ref.NAMES


# ------------------------------------------------------------------ cases ---
def make_case(B, P, O, F, knn, seed, empty_images=(), ignore_band=True):
  """loss_cases.make_case with knn slots per pixel: gt_frag i32 [B,P,knn] (knn different
  fragments of a foreground pixel, in random order; -1 elsewhere), gt_loc f32 [B,P,knn,3] and
  gt_weight f32 [B,P,knn] (0 outside the foreground)."""
  c = loss_cases.make_case(B, P, O, F, seed, empty_images, ignore_band)
  rng = np.random.RandomState(seed + 7919)
  fg = (c['gt_obj'] >= 1) & (c['gt_obj'] <= O)
  frag = np.full((B, P, knn), -1, np.int32)
  for b in range(B):
    for p in range(P):
      if fg[b, p]:
        frag[b, p] = rng.permutation(F)[:knn]
  c['gt_frag'] = frag
  c['gt_loc'] = (1.5 * rng.randn(B, P, knn, 3)).astype(np.float32)
  c['gt_weight'] = np.where(fg[..., None], rng.uniform(0.25, 2.0, (B, P, knn)),
                            0.0).astype(np.float32)
  return c


def squeeze_case(c):
  """A knn = 1 case in the layout of loss_cases.make_case (no slot dimension)."""
  assert c['gt_frag'].shape[-1] == 1
  out = dict(c)
  out['gt_frag'] = c['gt_frag'][..., 0]
  out['gt_loc'] = c['gt_loc'][..., 0, :]
  out['gt_weight'] = c['gt_weight'][..., 0]
  return out


# ------------------------------------------------------------------ ground truth ---
def assign(xyz, centers, sizes, knn):
  """(ids i32 [n,knn], coords f32 [n,knn,3]) of points xyz f32 [n,3] against centers f64 [F,3]
  and sizes f64 [F]: slot j holds the j-th nearest centre by dx^2 + dy^2 + dz^2, summed in that
  order in fp64 on the fp32 xyz, ascending, ties to the lower index; coords = (xyz - centre) /
  size in fp64, rounded to fp32 once."""
  xyz = np.asarray(xyz, np.float32)
  centers = np.asarray(centers, np.float64)
  sizes = np.asarray(sizes, np.float64)
  n, F = xyz.shape[0], centers.shape[0]
  ids = np.zeros((n, knn), np.int32)
  coords = np.zeros((n, knn, 3), np.float32)
  for i in range(n):
    x, y, z = (float(v) for v in xyz[i])
    d2 = []
    for f in range(F):
      dx, dy, dz = x - centers[f, 0], y - centers[f, 1], z - centers[f, 2]
      d2.append((dx * dx + dy * dy) + dz * dz)
    order = sorted(range(F), key=lambda f: (d2[f], f))
    for j in range(knn):
      f = order[j]
      ids[i, j] = f
      for k, v in enumerate((x, y, z)):
        coords[i, j, k] = np.float32((v - centers[f, k]) / sizes[f])
  return ids, coords


def gt_fields(depth, local_pos, masks, obj_ids, centers, sizes, knn):
  """epos_gt_fields_knn: depth f32 [n,h,w], local_pos f32 [n,h,w,3], masks u8 [n,h,w] or None,
  centers f64 [O,F,3], sizes f64 [O,F]. Returns {obj_label i32 [h,w], instance i32 [h,w],
  frag_label i32 [h,w,knn], frag_loc f32 [h,w,knn,3], frag_weight f32 [h,w,knn]}. With masks a
  pixel goes to the last instance with mask != 0 and depth > 0, without to the nearest depth
  > 0, ties to the higher index; an instance whose id is outside 1..O takes no pixel; a pixel no
  instance takes is 0 everywhere (instance -1)."""
  n, h, w = depth.shape
  O = sizes.shape[0]
  out = {'obj_label': np.zeros((h, w), np.int32), 'instance': np.full((h, w), -1, np.int32),
         'frag_label': np.zeros((h, w, knn), np.int32),
         'frag_loc': np.zeros((h, w, knn, 3), np.float32),
         'frag_weight': np.zeros((h, w, knn), np.float32)}
  for y in range(h):
    for x in range(w):
      win, best = -1, 0.0
      for i in range(n):
        o, d = int(obj_ids[i]), depth[i, y, x]
        if not (1 <= o <= O and d > 0):
          continue
        if masks is not None:
          if masks[i, y, x]:
            win = i                           # the last one wins
        elif win < 0 or d <= best:
          win, best = i, d
      if win < 0:
        continue
      o = int(obj_ids[win])
      ids, coords = assign(local_pos[win, y, x][None], centers[o - 1], sizes[o - 1], knn)
      out['obj_label'][y, x], out['instance'][y, x] = o, win
      out['frag_label'][y, x], out['frag_loc'][y, x] = ids[0], coords[0]
      out['frag_weight'][y, x] = 1.0
  return out


# ------------------------------------------------------------------ forward ---
def pixel_class(g, fs, ws, num_objs, num_frags, ignore):
  """'ignored' | 'bad' | 'ok': the ignore rule first; a foreground pixel is bad if any slot's
  fragment is outside 0..F-1, any slot's weight is not a finite number > 0, or two slots name
  the same fragment."""
  if g == ignore:
    return 'ignored'
  if g < 0 or g > num_objs:
    return 'bad'
  if g >= 1:
    for j, f in enumerate(fs):
      w = float(np.float32(ws[j]))
      if f < 0 or f > num_frags - 1 or not (w > 0.0 and math.isfinite(w)):
        return 'bad'
      if any(int(fs[i]) == int(f) for i in range(j)):
        return 'bad'
  return 'ok'


def pixel_terms(obj_row, frag_rows, loc_rows, g, fs, locs, ws, num_objs, num_frags, ignore):
  """One pixel: ('ignored',) | ('bad',) | ('ok', g, ce_obj, ce_frag, hub); fs [knn], locs
  [knn,3], ws [knn]. ce_frag and hub are the sums over the slots in order from 0.0 of
  loss_ref's summands."""
  cls = pixel_class(g, fs, ws, num_objs, num_frags, ignore)
  if cls != 'ok':
    return (cls,)
  ce_obj = loss_ref.cross_entropy(obj_row, g)
  if g == 0:
    return ('ok', 0, ce_obj, 0.0, 0.0)
  ce_frag, hub_sum = 0.0, 0.0
  for j, f in enumerate(fs):
    f = int(f)
    ce_frag += loss_ref.cross_entropy(frag_rows[g - 1], f)
    hub = [loss_ref.huber(float(loc_rows[g - 1, f, k]) - float(locs[j][k])) for k in range(3)]
    hub_sum += float(np.float32(ws[j])) * ((hub[0] + hub[1]) + hub[2])
  return ('ok', g, ce_obj, ce_frag, hub_sum)


def terms(c, share, ignore=loss_cases.IGNORE):
  """(sums f64 [B,O+1,3], counts i64 [B,O+1,2], bad i64 [B]) of a make_case case: loss_ref.terms
  with the slots. counts count pixels."""
  obj = np.asarray(c['obj_logits'], np.float32)
  frag = np.asarray(c['frag_logits'], np.float32)
  loc = np.asarray(c['frag_loc'], np.float32)
  gt_loc = np.asarray(c['gt_loc'], np.float32)
  B, P, O1 = obj.shape
  O, F = frag.shape[2], frag.shape[3]
  sums = np.zeros((B, O1, 3), np.float64)
  counts = np.zeros((B, O1, 2), np.int64)
  bad = np.zeros((B,), np.int64)
  for b in range(B):
    for p0 in range(0, P, share):
      part = [[0.0, 0.0, 0.0] for _ in range(O1)]
      for p in range(p0, min(p0 + share, P)):
        t = pixel_terms(obj[b, p], frag[b, p], loc[b, p], int(c['gt_obj'][b, p]),
                        c['gt_frag'][b, p], gt_loc[b, p], c['gt_weight'][b, p], O, F, ignore)
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


# ------------------------------------------------------------------ reduce ---
def image_losses(sums, counts, weights=(1.0, 1.0, 100.0), knn=1):
  """loss_ref.image_losses with n_fg * knn rows in the two fragment means."""
  w_obj, w_cls, w_loc = weights
  O1 = sums.shape[0]
  P = int(counts[:, 0].sum()) + int(counts[0, 1])
  rows = int(counts[1:, 0].sum()) * knn
  s = [0.0, 0.0, 0.0]
  for g in range(O1):
    s[0] += float(sums[g, 0])
    if g >= 1:
      s[1] += float(sums[g, 1])
      s[2] += float(sums[g, 2])
  out = {'obj_cls_loss': w_obj * (s[0] / P),
         'frag_cls_loss': w_cls * (s[1] / rows) if rows else 0.0,
         'frag_loc_loss': w_loc * (s[2] / (3 * rows)) if rows else 0.0}
  out['total_loss'] = (out['obj_cls_loss'] + out['frag_cls_loss']) + out['frag_loc_loss']
  return out


def dataset_losses(sums, counts, weights=(1.0, 1.0, 100.0), knn=1):
  """loss_ref.dataset_losses with knn: 'per_image', 'mean', 'pooled', 'per_object'."""
  w_obj, w_cls, w_loc = weights
  N, O1 = sums.shape[0], sums.shape[1]
  per_image = [image_losses(sums[i], counts[i], weights, knn) for i in range(N)]
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
  pooled = image_losses(tot, np.stack([n, np.zeros_like(n)], axis=1), weights, knn)
  obj_sum = 0.0
  for g in range(O1):
    obj_sum += float(tot[g, 0])
  pooled['obj_cls_loss'] = w_obj * (obj_sum / pixels)
  pooled['total_loss'] = ((pooled['obj_cls_loss'] + pooled['frag_cls_loss']) +
                          pooled['frag_loc_loss'])
  per_object = {}
  for g in range(1, O1):
    c = int(n[g])
    per_object[g] = {'frag_cls_loss': w_cls * (float(tot[g, 1]) / (c * knn)) if c else 0.0,
                     'frag_loc_loss': w_loc * (float(tot[g, 2]) / (3 * c * knn)) if c else 0.0,
                     'pixels': c}
  return {'per_image': per_image, 'mean': mean, 'pooled': pooled, 'per_object': per_object}


def scales(counts, weights, reduction, knn=1):
  """loss_grad_ref.scales with n_b * knn in the two fragment factors."""
  w_obj, w_cls, w_loc = weights
  B = counts.shape[0]
  pix = [int(counts[b, :, 0].sum()) + int(counts[b, 0, 1]) for b in range(B)]
  fg = [int(counts[b, 1:, 0].sum()) * knn for b in range(B)]
  out = np.zeros((B, 3), np.float64)
  for b in range(B):
    if reduction == MEAN:
      d = (pix[b] * B, fg[b] * B, 3 * fg[b] * B)
    else:
      d = (sum(pix), sum(fg), 3 * sum(fg))
    out[b] = [w / n if n else 0.0 for w, n in zip((w_obj, w_cls, w_loc), d)]
  return out


# ------------------------------------------------------------------ logit gradients ---
def softmax_knn(row, targets, knn):
  """[knn * exp(x_c - m) / S - [c in targets]] in fp64 on the fp32 values, m = max x, S added
  in index order: loss_grad_ref.softmax_minus_one_hot with the factor and the set."""
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
  hot = set(int(t) for t in targets)
  return [float(knn) * (v / s) - (1.0 if c in hot else 0.0) for c, v in enumerate(e)]


def grads(c, scale, upstream=None, ignore=loss_cases.IGNORE, rounded=True):
  """(d_obj [B,P,O+1], d_frag [B,P,O,F], d_loc [B,P,O,F,3]) of a make_case case, as
  loss_grad_ref.grads."""
  obj = np.asarray(c['obj_logits'], np.float32)
  frag = np.asarray(c['frag_logits'], np.float32)
  loc = np.asarray(c['frag_loc'], np.float32)
  gt_loc = np.asarray(c['gt_loc'], np.float32)
  B, P, O1 = obj.shape
  O, F = frag.shape[2], frag.shape[3]
  knn = c['gt_frag'].shape[-1]
  u = loss_grad_ref.upstream_factors(upstream)
  d_obj = np.zeros(obj.shape, np.float64)
  d_frag = np.zeros(frag.shape, np.float64)
  d_loc = np.zeros(loc.shape, np.float64)
  for b in range(B):
    s = [float(scale[b, k]) * u[k] for k in range(3)]
    for p in range(P):
      g, fs, ws = int(c['gt_obj'][b, p]), c['gt_frag'][b, p], c['gt_weight'][b, p]
      if pixel_class(g, fs, ws, O, F, ignore) != 'ok':
        continue
      for k, v in enumerate(loss_grad_ref.softmax_minus_one_hot(obj[b, p], g)):
        d_obj[b, p, k] = s[0] * v
      if g == 0:
        continue
      for k, v in enumerate(softmax_knn(frag[b, p, g - 1], fs, knn)):
        d_frag[b, p, g - 1, k] = s[1] * v
      for j in range(knn):
        f = int(fs[j])
        for k in range(3):
          d = float(loc[b, p, g - 1, f, k]) - float(gt_loc[b, p, j, k])
          d_loc[b, p, g - 1, f, k] = s[2] * (float(np.float32(ws[j])) * loss_grad_ref.clamp1(d))
  if not rounded:
    return d_obj, d_frag, d_loc
  with np.errstate(over='ignore', invalid='ignore'):
    return d_obj.astype(np.float32), d_frag.astype(np.float32), d_loc.astype(np.float32)


def active_masks(c, ignore=loss_cases.IGNORE):
  """loss_grad_ref.active_masks with the slots: the elements the rules give a value."""
  B, P, O1 = c['obj_logits'].shape
  O, F = c['frag_logits'].shape[2], c['frag_logits'].shape[3]
  m_obj = np.zeros((B, P, O1), bool)
  m_frag = np.zeros((B, P, O, F), bool)
  m_loc = np.zeros((B, P, O, F, 3), bool)
  for b in range(B):
    for p in range(P):
      g = int(c['gt_obj'][b, p])
      if pixel_class(g, c['gt_frag'][b, p], c['gt_weight'][b, p], O, F, ignore) != 'ok':
        continue
      m_obj[b, p] = True
      if g >= 1:
        m_frag[b, p, g - 1] = True
        m_loc[b, p, g - 1, c['gt_frag'][b, p]] = True
  return m_obj, m_frag, m_loc


def softmax_bound(ref, s_k, row_len, knn):
  """loss_grad_ref.bound with the factor knn that multiplies the probability:
  2^-23 |ref| + |s| knn (row_len + 16) 2^-52 (+ 2^-149)."""
  return loss_grad_ref.bound(ref, s_k * knn, row_len)


# ------------------------------------------------------------------ weight / input gradients ---
def classes(c, ignore=loss_cases.IGNORE):
  """(cls i64 [B*P], frag i64 [B*P,knn]): heads_wgrad_ref.classes with the slots."""
  O, F = c['frag_logits'].shape[2], c['frag_logits'].shape[3]
  knn = c['gt_frag'].shape[-1]
  g = np.asarray(c['gt_obj']).reshape(-1).astype(np.int64)
  f = np.asarray(c['gt_frag']).reshape(-1, knn).astype(np.int64)
  w = np.asarray(c['gt_weight'], np.float32).reshape(-1, knn)
  cls = g.copy()
  for p in range(g.size):
    kind = pixel_class(int(g[p]), f[p], w[p], O, F, ignore)
    if kind != 'ok':
      cls[p] = -1
  return cls, f


def wgrads(A, d_obj, d_frag, d_loc, cls, frag):
  """heads_wgrad_ref.wgrads with frag [B*P,knn]: the localisation columns of a pixel are the
  three values at (g-1, f_j) of every slot. Returns (sums, abs_sums, n_terms)."""
  knn = frag.shape[1]
  sums, abs_sums, n_terms = heads_wgrad_ref.wgrads(A, d_obj, d_frag, d_loc, cls, frag[:, 0])
  if knn == 1:
    return sums, abs_sums, n_terms
  A = np.asarray(A, np.float64)
  n_pix, K = A.shape
  O, F = d_frag.shape[-2], d_frag.shape[-1]
  d_loc = np.asarray(d_loc).reshape(n_pix, O, F, 3)
  absA = np.abs(A)
  dW, db = (x.copy() for x in sums['loc'])
  aW, ab = (x.copy() for x in abs_sums['loc'])
  nt = n_terms['loc'].copy()
  dW, aW = dW.reshape(K, O, F, 3), aW.reshape(K, O, F, 3)
  db, ab, nt = db.reshape(O, F, 3), ab.reshape(O, F, 3), nt.reshape(O, F, 3)
  with np.errstate(invalid='ignore', over='ignore'):
    for g in range(1, O + 1):
      idx = np.nonzero(cls == g)[0]
      for j in range(1, knn):
        for p in idx:                          # pixel order within a slot; the bound covers it
          f = int(frag[p, j])
          v = d_loc[p, g - 1, f].astype(np.float64)
          dW[:, g - 1, f] += A[p][:, None] * v[None, :]
          db[g - 1, f] += v
          aW[:, g - 1, f] += absA[p][:, None] * np.abs(v)[None, :]
          ab[g - 1, f] += np.abs(v)
          nt[g - 1, f] += 1
  sums['loc'] = (dW.reshape(K, -1), db.reshape(-1))
  abs_sums['loc'] = (aW.reshape(K, -1), ab.reshape(-1))
  n_terms['loc'] = nt.reshape(-1)
  return sums, abs_sums, n_terms


def dgrad(d_obj, d_frag, d_loc, W_obj, W_frag, W_loc, cls, frag):
  """heads_dgrad_ref.dgrad with frag [B*P,knn]: the heads obj, frag, loc, ascending n within a
  head, so a pixel's slots are visited in ascending fragment index. Returns (sums, abs_sums,
  n_active)."""
  knn = frag.shape[1]
  if knn == 1:
    return heads_dgrad_ref.dgrad(d_obj, d_frag, d_loc, W_obj, W_frag, W_loc, cls, frag[:, 0])
  O1 = d_obj.shape[-1]
  O, F = d_frag.shape[-2], d_frag.shape[-1]
  n_pix = cls.shape[0]
  d_obj = np.asarray(d_obj).reshape(n_pix, O1)
  d_frag = np.asarray(d_frag).reshape(n_pix, O, F)
  d_loc = np.asarray(d_loc).reshape(n_pix, O, F, 3)
  Ws = [np.asarray(w, np.float64).reshape(-1, n) for w, n in (
      (W_obj, O1), (W_frag, O * F), (W_loc, O * F * 3))]
  K = Ws[0].shape[0]
  sums, abs_sums = np.zeros((n_pix, K)), np.zeros((n_pix, K))
  n_active = np.zeros((n_pix,), np.int64)
  valid = np.nonzero(cls >= 0)[0]
  fg = np.nonzero(cls >= 1)[0]
  g1 = cls[fg] - 1
  by_frag = np.sort(frag[fg], axis=1)
  with np.errstate(invalid='ignore', over='ignore'):
    def add(idx, d, rows):
      d = d.astype(np.float64)[:, None]
      sums[idx] += d * rows
      abs_sums[idx] += np.abs(d) * np.abs(rows)
      n_active[idx] += 1
    for c in range(O1):
      add(valid, d_obj[valid, c], np.broadcast_to(Ws[0][:, c], (valid.size, K)))
    for c in range(F):
      add(fg, d_frag[fg, g1, c], Ws[1][:, g1 * F + c].T)
    for a in range(knn):
      f = by_frag[:, a]
      for k in range(3):
        add(fg, d_loc[fg, g1, f, k], Ws[2][:, (g1 * F + f) * 3 + k].T)
  return sums, abs_sums, n_active
