"""Numpy restatement of the logits layers' input gradient (csrc/heads_dgrad.hip;
include/epos_hip.h, "Input gradient"), written from that description: per pixel one fp64 sum
over the ACTIVE entries of the logit gradients only, in the stated order (the heads obj, frag,
loc; ascending n within a head), and the ReLU mask. No shared code with the package."""
import math

import numpy as np


def dgrad(d_obj, d_frag, d_loc, W_obj, W_frag, W_loc, cls, frag):
  """The fp64 sums of one batch and what their error bound needs. d_obj [..., O+1], d_frag
  [..., O, F], d_loc [..., O, F, 3] over the same B*P pixels (fp32 as epos_loss_grads writes
  them, or fp64); W_h [K, N_h] (or [1,1,K,N_h]) in the checkpoint layout, any float type, taken
  as fp64; cls, frag from heads_wgrad_ref.classes(). Returns (sums, abs_sums, n_active):
    sums      f64 [B*P, K]: dX[p,k] = sum_h sum_n d_h[p,n] W_h[k,n] over the columns ACTIVE at p
              (the O+1 object values of a pixel with cls >= 0; the row g-1 and the three values
              at (g-1, f) of a foreground pixel), added one by one from 0.0 in the stated order;
              a pixel with cls < 0 keeps its +0.0 and nothing of it is read
    abs_sums  the same sums over |d| |W|
    n_active  i64 [B*P]: the number of columns added into the pixel's row
  The loops run over the column index, vectorised over the pixels: every pixel's own order is
  the stated one, and an inactive NaN stays out."""
  O1 = d_obj.shape[-1]
  O, F = d_frag.shape[-2], d_frag.shape[-1]
  n_pix = cls.shape[0]
  d_obj = np.asarray(d_obj).reshape(n_pix, O1)
  d_frag = np.asarray(d_frag).reshape(n_pix, O, F)
  d_loc = np.asarray(d_loc).reshape(n_pix, O, F, 3)
  Ws = [np.asarray(w, np.float64).reshape(-1, n) for w, n in (
      (W_obj, O1), (W_frag, O * F), (W_loc, O * F * 3))]
  K = Ws[0].shape[0]
  assert all(w.shape[0] == K for w in Ws)
  sums, abs_sums = np.zeros((n_pix, K)), np.zeros((n_pix, K))
  n_active = np.zeros((n_pix,), np.int64)
  valid = np.nonzero(cls >= 0)[0]
  fg = np.nonzero(cls >= 1)[0]
  g1, f = cls[fg] - 1, frag[fg]
  with np.errstate(invalid='ignore', over='ignore'):
    def add(idx, d, rows):                     # d [n], rows [n, K]: one column of each pixel
      d = d.astype(np.float64)[:, None]
      sums[idx] += d * rows
      abs_sums[idx] += np.abs(d) * np.abs(rows)
      n_active[idx] += 1
    for c in range(O1):
      add(valid, d_obj[valid, c], np.broadcast_to(Ws[0][:, c], (valid.size, K)))
    for c in range(F):
      add(fg, d_frag[fg, g1, c], Ws[1][:, g1 * F + c].T)
    for k in range(3):
      add(fg, d_loc[fg, g1, f, k], Ws[2][:, (g1 * F + f) * 3 + k].T)
  return sums, abs_sums, n_active


def relu_mask(dx, y):
  """dx with +0.0 wherever y <= 0 (-0.0 counts, a NaN does not)."""
  out = np.array(dx, copy=True)
  with np.errstate(invalid='ignore'):
    out[np.asarray(y) <= 0] = 0.0
  return out


def bound(ref, abs_sum, n_active):
  """|got - ref| <= 2^-24 |ref| + (n_active + 16) 2^-52 abs_sum, per element; n_active [B*P]
  is the pixel's. The reasoning is heads_wgrad_ref.bound's: exact products, two fp64 summations
  of the same n_active numbers, one rounding to fp32."""
  ref = np.asarray(ref, np.float64)
  n = np.asarray(n_active, np.float64).reshape(-1, 1)
  return 2.0 ** -24 * np.abs(ref) + (n + 16.0) * 2.0 ** -52 * np.asarray(abs_sum)


def within(got, ref, abs_sum, n_active):
  """(ok, worst): every element of the fp32 result inside bound(); a non-finite reference
  element asks for a non-finite result, nothing more. worst = max error / bound over the finite
  elements with a non-zero bound."""
  got = np.asarray(got, np.float64)
  ref = np.asarray(ref, np.float64)
  fin = np.isfinite(ref)
  tol = bound(np.where(fin, ref, 0.0), np.where(np.isfinite(abs_sum), abs_sum, 0.0), n_active)
  if not (np.isfinite(got) == fin).all():
    return False, math.inf
  with np.errstate(invalid='ignore', divide='ignore'):
    err = np.abs(np.where(fin, got - ref, 0.0))
    ratio = np.where(tol > 0, err / tol, 0.0)
  return bool((err <= tol).all()), float(ratio.max()) if ratio.size else 0.0
