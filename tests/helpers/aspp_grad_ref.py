"""Numpy restatement of the two ASPP gradient entries (csrc/aspp_grad.hip; include/epos_hip.h,
"ASPP gradients"), written from that description in fp64: the join of the branches' gradients at
the encoder output, operation for operation and to be matched bit for bit, and the adjoint of the
image-pooling broadcast with its bound. No shared code with the package."""
import math

import numpy as np


def _shifted(X, dy, dx):
  """X [B,H,W,C] read at (y + dy, x + dx), zeros outside the image."""
  B, H, W, C = X.shape
  out = np.zeros_like(X)
  ys0, ys1 = max(0, -dy), min(H, H - dy)
  xs0, xs1 = max(0, -dx), min(W, W - dx)
  if ys0 < ys1 and xs0 < xs1:
    out[:, ys0:ys1, xs0:xs1] = X[:, ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
  return out


def _valid(shape, dy, dx):
  H, W = shape
  y, x = np.arange(H)[:, None], np.arange(W)[None, :]
  return (y + dy >= 0) & (y + dy < H) & (x + dx >= 0) & (x + dx < W)


def aspp_join_ref(shape, depthwise=(), plain=(), pooled=None, Y=None, dtype=np.float32):
  """dX f32 [B,H,W,C], to be matched BIT FOR BIT. Per element one fp64 accumulator from +0.0: the
  plain terms E_j in index order; the depthwise terms (D, w9c, rate) in index order, within a
  term the taps in ascending tap = 3 ky + kx, each the exact product w9c[tap, c] * D[b, y -
  (ky-1) rate, x - (kx-1) rate, c], a tap outside the image adding +0.0 and not 0 * d; the
  per-image term Pool[b, c] / div, an fp64 division; one rounding to fp32; +0.0 where Y <= 0.
  dtype=np.float64: the same operations on fp64 inputs without the rounding -- the formula
  itself, for a comparison with autograd."""
  B, H, W, C = shape
  acc = np.zeros((B, H, W, C), np.float64)
  with np.errstate(invalid='ignore', over='ignore'):
    for E in plain:
      acc = acc + np.asarray(E, dtype).reshape(B, H, W, C).astype(np.float64)
    for D, w9c, rate in depthwise:
      D64 = np.asarray(D, dtype).astype(np.float64)
      w64 = np.asarray(w9c, dtype).astype(np.float64)
      for ky in range(3):
        for kx in range(3):
          dy, dx = -(ky - 1) * rate, -(kx - 1) * rate
          ok = _valid((H, W), dy, dx)[None, :, :, None]
          term = w64[3 * ky + kx] * _shifted(D64, dy, dx)
          acc = acc + np.where(ok, term, 0.0)
    if pooled is not None:
      pool, div = pooled
      acc = acc + (np.asarray(pool, dtype).astype(np.float64) / np.float64(div))[
          :, None, None, :]
    out = acc.astype(dtype)
  if Y is not None:
    with np.errstate(invalid='ignore'):
      out = np.where(np.asarray(Y) <= 0, dtype(0.0), out)
  return out


def pool_broadcast_ref(D):
  """(ref f64 [B,C], bound f64 [B,C]) for D [B,P,C]: the exact sum over P of the values
  (math.fsum, rounded to fp64 once) and 2^-24 |ref| + (P + 16) 2^-52 sum |D| -- the one rounding
  to fp32 and an fp64 summation of P terms in any order (Higham, eq. 4.4; the 16 extra units
  cover the second-order terms and fsum's own rounding)."""
  D = np.asarray(D).astype(np.float64)
  B, P, C = D.shape
  ref = np.array([[math.fsum(D[b, :, c]) for c in range(C)] for b in range(B)], np.float64)
  bound = 2.0 ** -24 * np.abs(ref) + (P + 16.0) * 2.0 ** -52 * np.abs(D).sum(axis=1)
  return ref, bound
