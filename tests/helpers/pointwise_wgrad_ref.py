"""Numpy restatement of the weight and batch-norm gradients of a 1x1 conv layer
(csrc/pointwise_wgrad.hip; include/epos_hip.h, "Pointwise weight gradient"), written from that
description in fp64: the fp16-pair form of A from its raw bytes, S = A^T G and g, the three
formulas, and the error bounds. No shared code with the package."""
import math

import numpy as np


# ------------------------------------------------------------ fp16 pairs ---
def h2_scale(bound):
  """(s, 1/s): the power of two s with s * bound in [2^14, 2^15), from the exponent field of the
  fp32 bound; capped at 2^126, and 1 for a bound that is not finite."""
  e = int(np.float32(bound).view(np.uint32)) >> 23
  sb = min(268 - e, 253)
  if e >= 255:
    sb = 127
  return 2.0 ** (sb - 127), 2.0 ** (127 - sb)


def slot_bound(slot, slot2=None, gain=0.0, bias=0.0):
  """The bound the 64 words of an absmax slot (or two) stand for: the largest word, as fp32 bits,
  then gain * it + bias in fp32 unless gain == 0."""
  v = int(np.asarray(slot, np.uint32).max())
  if slot2 is not None:
    v = max(v, int(np.asarray(slot2, np.uint32).max()))
  b = np.array([v], np.uint32).view(np.float32)[0]
  if gain != 0.0:
    b = np.float32(np.float32(gain) * b) + np.float32(bias)
  return np.float32(b)


def h2_split(x, s):
  """The bytes EposDepthwiseArgs.y_h2 writes for fp32 x [M, K] (K % 4 == 0) at scale s, as
  float32 [M, K] words: per four columns [hi hi hi hi | mid mid mid mid] fp16, t = x * s,
  hi = rn_fp16(t), mid = rn_fp16((t - hi) * 2^11), each step rounded in fp32."""
  x = np.asarray(x, np.float32)
  M, K = x.shape
  assert K % 4 == 0
  t = x * np.float32(s)
  hi = t.astype(np.float16)
  mid = ((t - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
  out = np.empty((M, K // 4, 2, 4), np.float16)
  out[:, :, 0, :] = hi.reshape(M, K // 4, 4)
  out[:, :, 1, :] = mid.reshape(M, K // 4, 4)
  return out.reshape(M, K * 2).view(np.float32)


def h2_values(raw, K, inv):
  """fp64 [M, K]: the values a pre-split A stands for, (hi + mid 2^-11) * inv, from its raw words
  (float32 or uint32 [M, >= K]; columns from K on are not looked at)."""
  raw = np.ascontiguousarray(np.asarray(raw)[:, :K])
  M = raw.shape[0]
  h = raw.view(np.float16).reshape(M, K // 4, 2, 4).astype(np.float64)
  return ((h[:, :, 0, :] + h[:, :, 1, :] * 2.0 ** -11) * inv).reshape(M, K)


# ------------------------------------------------------------------ sums ---
def sums(A, G):
  """(S [K,N], g [N], abs_S, abs_g): S = A^T G and the column sums of G in fp64, and the same
  sums over |A||G| and |G| for the bounds."""
  A, G = np.asarray(A, np.float64), np.asarray(G, np.float64)
  with np.errstate(invalid='ignore', over='ignore'):
    return A.T @ G, G.sum(axis=0), np.abs(A).T @ np.abs(G), np.abs(G).sum(axis=0)


def fold_scale(gamma, var, eps):
  """(scale, rstd): scale_c = fl32(gamma_c / sqrt(var_c + eps)) as fp64 values, rstd_c in fp64."""
  sd = np.sqrt(np.asarray(var, np.float32).astype(np.float64) + eps)
  scale = (np.asarray(gamma, np.float32).astype(np.float64) / sd).astype(np.float32)
  return scale.astype(np.float64), 1.0 / sd


def close(S, g, W=None, gamma=None, mean=None, var=None, eps=0.0, scale=None):
  """fp64 (dW [K,N], dgamma [N] or None, dbeta [N]): with a batch norm dW = scale S,
  dgamma = rstd (sum_k W S - mean g), dbeta = g; without (gamma None) dW = S, db = g. `scale`
  overrides the fp32-rounded scale (the autograd test differentiates through its own)."""
  S, g = np.asarray(S, np.float64), np.asarray(g, np.float64)
  if gamma is None:
    return S.copy(), None, g.copy()
  sc, rstd = fold_scale(gamma, var, eps)
  if scale is not None:
    sc = np.asarray(scale, np.float64)
  with np.errstate(invalid='ignore', over='ignore'):
    dot = (np.asarray(W, np.float64) * S).sum(axis=0)
    dgamma = rstd * (dot - np.asarray(mean, np.float64) * g)
    return sc[None, :] * S, dgamma, g.copy()


# ---------------------------------------------------------------- bounds ---
def bound(M, abs_sum):
  """|got - ref| <= (M + 16) 2^-52 abs_sum for S and g.

  Every term A[p,k] G[p,c] is the product of two values of at most 24 bits, exact in fp64, so
  the device's sum and the reference's are two fp64 summations of the SAME M numbers in
  different orders. Any order of n additions with unit roundoff u = 2^-53 is within
  (n - 1) u / (1 - (n - 1) u) sum |term| of the exact sum (Higham, Accuracy and Stability, eq.
  4.4), so the two differ by at most 2 (M - 1) u abs_sum (1 + O(M u)) <= M 2^-52 abs_sum; the 16
  extra units cover the second-order terms and the slabs' additions many times over."""
  return (float(M) + 16.0) * 2.0 ** -52 * np.asarray(abs_sum, np.float64)


def bounds_close(M, S, g, abs_S, abs_g, W=None, gamma=None, mean=None, var=None, eps=0.0):
  """Bounds of the fp32 outputs (dW, dgamma or None, dbeta) against close() of the reference's S
  and g: half an ulp of the fp32 rounding, 2^-24 |ref| (2^-149 below the normal range), plus
  bound() carried through the formula:
    dW      |scale| bound(S), and 2^-52 |ref| for the one fp64 product;
    dbeta   bound(g);
    dgamma  rstd (sum_k |W| bound(S) + |mean| bound(g)) for the inputs, and for the evaluation
            itself -- K products and K additions in some order, one more product, a difference
            and a product, each within 2^-53, on the device and in the reference --
            (K + 8) 2^-52 rstd (sum_k |W||S| + |mean||g|)."""
  S, g = np.asarray(S, np.float64), np.asarray(g, np.float64)
  bS, bg = bound(M, abs_S), bound(M, abs_g)
  dW, dgamma, dbeta = close(S, g, W, gamma, mean, var, eps)
  tiny = 2.0 ** -149
  fin = lambda a: np.where(np.isfinite(a), a, 0.0)                       # noqa: E731
  if gamma is None:
    return (2.0 ** -24 * np.abs(fin(dW)) + bS + tiny, None,
            2.0 ** -24 * np.abs(fin(dbeta)) + bg + tiny)
  sc, rstd = fold_scale(gamma, var, eps)
  absW, absm = np.abs(np.asarray(W, np.float64)), np.abs(np.asarray(mean, np.float64))
  K = S.shape[0]
  tW = (2.0 ** -24 + 2.0 ** -52) * np.abs(fin(dW)) + np.abs(sc)[None, :] * bS + tiny
  mag = (absW * np.abs(fin(S))).sum(axis=0) + absm * np.abs(fin(g))
  tg = (2.0 ** -24 * np.abs(fin(dgamma)) + rstd * ((absW * bS).sum(axis=0) + absm * bg) +
        (K + 8.0) * 2.0 ** -52 * rstd * mag + tiny)
  return tW, tg, 2.0 ** -24 * np.abs(fin(dbeta)) + bg + tiny


def within(got, ref, tol):
  """(ok, worst): every element of `got` within tol of ref; a non-finite reference element asks
  for a non-finite result, nothing more. worst = max error / tol over the finite elements."""
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  fin = np.isfinite(ref)
  if not (np.isfinite(got) == fin).all():
    return False, math.inf
  with np.errstate(invalid='ignore'):
    err = np.abs(np.where(fin, got - ref, 0.0))
  tol = np.where(fin, tol, 1.0)
  ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, math.inf, 0.0))
  return bool((err <= tol).all()), float(ratio.max()) if ratio.size else 0.0
