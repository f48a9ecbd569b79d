"""Numpy restatement of the logits layers' weight gradients and of the momentum step
(csrc/heads_wgrad.hip; include/epos_hip.h, "Weight gradients"), written from that description:
fp64 sums over the ACTIVE entries of the logit gradients only, no shared code with the package."""
import math

import numpy as np

HEADS = ('obj', 'frag', 'loc')


def classes(c, ignore=255):
  """(cls i64 [B*P], frag i64 [B*P]) of a loss_cases case: cls = -1 for a pixel that contributes
  nothing (ignored or bad), 0 for background, g in 1..O for a foreground pixel of object g; the
  ignore rule first, as in include/epos_hip.h, "Losses"."""
  O, F = c['frag_logits'].shape[2], c['frag_logits'].shape[3]
  g = np.asarray(c['gt_obj']).reshape(-1).astype(np.int64)
  f = np.asarray(c['gt_frag']).reshape(-1).astype(np.int64)
  w = np.asarray(c['gt_weight'], np.float32).reshape(-1)
  cls = g.copy()
  cls[(g < 0) | (g > O)] = -1
  fg = (g >= 1) & (g <= O)
  with np.errstate(invalid='ignore'):
    bad = fg & ((f < 0) | (f > F - 1) | ~(w > 0) | ~np.isfinite(w))
  cls[bad] = -1
  cls[g == ignore] = -1
  return cls, f


def wgrads(A, d_obj, d_frag, d_loc, cls, frag):
  """The six fp64 sums of one batch and what their error bound needs. A [B*P, K] (any float
  type, taken as fp64); d_obj [..., O+1], d_frag [..., O, F], d_loc [..., O, F, 3] over the
  same B*P pixels (fp32 as epos_loss_grads writes them, or fp64); cls, frag from classes().
  Returns (sums, abs_sums, n_terms), dicts over 'obj', 'frag', 'loc' of (dW [K,N], db [N]):
    sums      dW[k,n] = sum_p A[p,k] d[p,n], db[n] = sum_p d[p,n] over the pixels for which
              column n is active (the O+1 object values of a pixel with cls >= 0; the row g-1
              and the three values at (g-1, f) of a foreground pixel), nothing else touched
    abs_sums  the same sums over |A| |d| (over |d| for db)
    n_terms   i64 [N]: the number of pixels added into column n
  Per object gathers and np.add.at: F = 256 stays cheap and an inactive NaN stays out."""
  A = np.asarray(A, np.float64)
  n_pix, K = A.shape
  O1 = d_obj.shape[-1]
  O, F = d_frag.shape[-2], d_frag.shape[-1]
  d_obj = np.asarray(d_obj).reshape(n_pix, O1)
  d_frag = np.asarray(d_frag).reshape(n_pix, O, F)
  d_loc = np.asarray(d_loc).reshape(n_pix, O, F, 3)
  absA = np.abs(A)
  sums, abs_sums, n_terms = {}, {}, {}
  with np.errstate(invalid='ignore', over='ignore'):
    idx = np.nonzero(cls >= 0)[0]
    d = d_obj[idx].astype(np.float64)
    sums['obj'] = (A[idx].T @ d, d.sum(axis=0))
    abs_sums['obj'] = (absA[idx].T @ np.abs(d), np.abs(d).sum(axis=0))
    n_terms['obj'] = np.full((O1,), idx.size, np.int64)
    dW_f, db_f = np.zeros((K, O, F)), np.zeros((O, F))
    aW_f, ab_f = np.zeros((K, O, F)), np.zeros((O, F))
    dW_l, db_l = np.zeros((K, O, F, 3)), np.zeros((O, F, 3))
    aW_l, ab_l = np.zeros((K, O, F, 3)), np.zeros((O, F, 3))
    n_f, n_l = np.zeros((O, F), np.int64), np.zeros((O, F, 3), np.int64)
    for g in range(1, O + 1):
      idx = np.nonzero(cls == g)[0]
      if not idx.size:
        continue
      d = d_frag[idx, g - 1].astype(np.float64)                  # [n, F]
      dW_f[:, g - 1], db_f[g - 1] = A[idx].T @ d, d.sum(axis=0)
      aW_f[:, g - 1], ab_f[g - 1] = absA[idx].T @ np.abs(d), np.abs(d).sum(axis=0)
      n_f[g - 1] = idx.size
      f = frag[idx]
      v = d_loc[idx, g - 1, f].astype(np.float64)                # [n, 3]
      tW, tb = np.zeros((F, K, 3)), np.zeros((F, 3))
      uW, ub = np.zeros((F, K, 3)), np.zeros((F, 3))
      np.add.at(tW, f, A[idx][:, :, None] * v[:, None, :])
      np.add.at(tb, f, v)
      np.add.at(uW, f, absA[idx][:, :, None] * np.abs(v)[:, None, :])
      np.add.at(ub, f, np.abs(v))
      dW_l[:, g - 1], db_l[g - 1] = tW.transpose(1, 0, 2), tb
      aW_l[:, g - 1], ab_l[g - 1] = uW.transpose(1, 0, 2), ub
      np.add.at(n_l[g - 1], f, 1)
  sums['frag'] = (dW_f.reshape(K, O * F), db_f.reshape(-1))
  abs_sums['frag'] = (aW_f.reshape(K, O * F), ab_f.reshape(-1))
  n_terms['frag'] = n_f.reshape(-1)
  sums['loc'] = (dW_l.reshape(K, O * F * 3), db_l.reshape(-1))
  abs_sums['loc'] = (aW_l.reshape(K, O * F * 3), ab_l.reshape(-1))
  n_terms['loc'] = n_l.reshape(-1)
  return sums, abs_sums, n_terms


def bound(ref, abs_sum, n_terms):
  """|got - ref| <= 2^-24 |ref| + (n_terms + 16) 2^-52 abs_sum + 2^-149.

  Every term A[p,k] * d[p,n] is the product of two fp32 values, exact in fp64, so the device's
  sum and the reference's are two fp64 summations of the SAME n_terms numbers in different
  orders. Any order of n additions with unit roundoff u = 2^-53 is within
  (n - 1) u / (1 - (n - 1) u) * sum |term| of the exact sum (Higham, Accuracy and Stability,
  eq. 4.4), so the two differ by at most 2 (n - 1) u abs_sum (1 + O(n u)) <= n 2^-52 abs_sum for
  the sizes used here. The device then rounds once to fp32: half an ulp, 2^-24 |value|, or half
  the smallest subnormal, 2^-150, below the normal range. |value| may exceed |ref| by the
  summation difference, which costs 2^-24 of it again: the 16 extra units of 2^-52 abs_sum
  cover that and the neglected second-order terms many times over."""
  ref = np.asarray(ref, np.float64)
  return (2.0 ** -24 * np.abs(ref) +
          (np.asarray(n_terms, np.float64) + 16.0) * 2.0 ** -52 * np.asarray(abs_sum) +
          2.0 ** -149)


def within(got, ref, abs_sum, n_terms):
  """(ok, worst): every element of the fp32 result inside bound(); a non-finite reference
  element asks for a non-finite result, nothing more. worst = max error / bound over the
  finite elements."""
  got = np.asarray(got, np.float64)
  ref = np.asarray(ref, np.float64)
  tol = bound(np.where(np.isfinite(ref), ref, 0.0),
              np.where(np.isfinite(abs_sum), abs_sum, 0.0), n_terms)
  fin = np.isfinite(ref)
  if not (np.isfinite(got) == fin).all():
    return False, math.inf
  with np.errstate(invalid='ignore'):
    err = np.abs(np.where(fin, got - ref, 0.0))
  ratio = err / tol
  return bool((err <= tol).all()), float(ratio.max()) if ratio.size else 0.0


def momentum_step(w, accum, grad, lr, momentum, weight_decay, grad_mult):
  """(w', accum') of epos_momentum_step_f32 in numpy float32, each operation rounded once:
  g = grad_mult * (grad + weight_decay * w); a' = momentum * accum + g; w' = w - lr * a'."""
  f = np.float32
  w, accum, grad = (np.asarray(x, np.float32) for x in (w, accum, grad))
  g = f(grad_mult) * (grad + f(weight_decay) * w)
  a2 = f(momentum) * accum + g
  w2 = w - f(lr) * a2
  assert g.dtype == np.float32 and a2.dtype == np.float32 and w2.dtype == np.float32
  return w2, a2
