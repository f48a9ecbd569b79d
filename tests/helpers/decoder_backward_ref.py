"""Numpy restatement of the backward pass of the separable conv decoder_conv1
(csrc/pointwise_dgrad.hip, csrc/depthwise_grad.hip; include/epos_hip.h, "Pointwise input gradient"
and "Depthwise gradients"), written from those descriptions in fp64: the fold, D = mask (.)
(G Wf^T), the depthwise sums T and t, the depthwise input gradient, and their bounds. No shared
code with the package."""
import numpy as np


# ------------------------------------------------------------------ fold ---
def fold(W, gamma=None, var=None, eps=0.0):
  """Wf f32 [K,N]: W[k,c] * scale_c as ONE fp32 product, scale_c = fl32(gamma_c / sqrt(var_c +
  eps)) with the quotient in fp64 -- what the forward multiplies by. gamma None: Wf = W."""
  W = np.asarray(W, np.float32)
  if gamma is None:
    return W.copy()
  sd = np.sqrt(np.asarray(var, np.float32).astype(np.float64) + eps)
  scale = (np.asarray(gamma, np.float32).astype(np.float64) / sd).astype(np.float32)
  with np.errstate(invalid='ignore', over='ignore'):
    return (W * scale[None, :]).astype(np.float32)


def pair_values(raw, K):
  """fp64 [M,K]: hi + mid 2^-11 of the fp16 pairs in raw (float32 or uint32 words [M, >= K]),
  per four columns [hi hi hi hi | mid mid mid mid]: the mask a pre-split A stands for, up to
  its positive scale."""
  raw = np.ascontiguousarray(np.asarray(raw)[:, :K])
  M = raw.shape[0]
  h = raw.view(np.float16).reshape(M, K // 4, 2, 4).astype(np.float64)
  return (h[:, :, 0, :] + h[:, :, 1, :] * 2.0 ** -11).reshape(M, K)


# ------------------------------------------------------ pointwise dgrad ---
def pointwise_dgrad(G, Wf, mask=None):
  """(D f64 [M,K], abs f64 [M,K]): D[p,k] = sum_c G[p,c] Wf[k,c] in fp64, +0.0 wherever mask <= 0
  (a NaN in the mask does not count), and sum_c |G||Wf| for the bound (0 where masked)."""
  G, Wf = np.asarray(G, np.float64), np.asarray(Wf, np.float64)
  with np.errstate(invalid='ignore', over='ignore'):
    D = G @ Wf.T
    A = np.abs(G) @ np.abs(Wf).T
  if mask is not None:
    with np.errstate(invalid='ignore'):
      off = np.asarray(mask, np.float64) <= 0
    D = np.where(off, 0.0, D)
    A = np.where(off, 0.0, A)
  return D, A


def bound_pointwise_dgrad(N, ref, abs_sum):
  """2^-24 |ref| + (N + 16) 2^-52 sum_c |G||Wf|: the one rounding to fp32, and two fp64
  summations of the same N exact products in different orders (Higham, eq. 4.4: each within
  (N - 1) 2^-53 of the exact sum to first order; the 16 extra units cover the second-order
  terms). Nothing is added for results below fp32's normal range."""
  fin = lambda a: np.where(np.isfinite(a), a, 0.0)                       # noqa: E731
  return 2.0 ** -24 * np.abs(fin(ref)) + (N + 16.0) * 2.0 ** -52 * fin(abs_sum)


# ------------------------------------------------------------ depthwise ---
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
  """bool [H,W]: whether (y + dy, x + dx) lies inside the image."""
  H, W = shape
  y, x = np.arange(H)[:, None], np.arange(W)[None, :]
  return (y + dy >= 0) & (y + dy < H) & (x + dx >= 0) & (x + dx < W)


def depthwise_forward(X, w9c, bias, rate):
  """relu(sum_tap w9c[tap] X(tap) + bias) in fp64: the layer's forward with folded weights."""
  X = np.asarray(X, np.float64)
  acc = np.zeros_like(X)
  for ky in range(3):
    for kx in range(3):
      acc += np.asarray(w9c, np.float64)[3 * ky + kx] * _shifted(X, (ky - 1) * rate,
                                                                  (kx - 1) * rate)
  return np.maximum(acc + np.asarray(bias, np.float64), 0.0)


def depthwise_wgrad(X, D, rate):
  """(T f64 [9,C], t f64 [C], abs_T, abs_t): T[tap,c] = sum X(tap) D, t[c] = sum D, taps in the
  padding adding nothing, and the same sums over absolute values."""
  X, D = np.asarray(X, np.float64), np.asarray(D, np.float64)
  C = X.shape[-1]
  T, aT = np.zeros((9, C)), np.zeros((9, C))
  with np.errstate(invalid='ignore', over='ignore'):
    for ky in range(3):
      for kx in range(3):
        ok = _valid(X.shape[1:3], (ky - 1) * rate, (kx - 1) * rate)[None, :, :, None]
        xs = _shifted(X, (ky - 1) * rate, (kx - 1) * rate)
        T[3 * ky + kx] = np.where(ok, xs * D, 0.0).sum(axis=(0, 1, 2))
        aT[3 * ky + kx] = np.where(ok, np.abs(xs * D), 0.0).sum(axis=(0, 1, 2))
    return T, D.sum(axis=(0, 1, 2)), aT, np.abs(D).sum(axis=(0, 1, 2))


def bound_depthwise_wgrad(pixels, abs_sum):
  """(B H W + 16) 2^-52 sum |X||D|: two fp64 summations of the same exact products in different
  orders, as tests/helpers/pointwise_wgrad_ref.bound."""
  a = np.asarray(abs_sum, np.float64)
  return (float(pixels) + 16.0) * 2.0 ** -52 * np.where(np.isfinite(a), a, 0.0)


def depthwise_dgrad(D, w9c, rate, Y=None):
  """dX f32 [B,H,W,C], to be matched BIT FOR BIT: one fp64 accumulator from +0.0, the taps in
  ascending order, a tap whose source pixel (y - (ky-1) r, x - (kx-1) r) lies outside the image
  skipped (not added as a zero), each product exact, rounded to fp32 once; +0.0 where Y <= 0."""
  D64, w64 = np.asarray(D, np.float32).astype(np.float64), np.asarray(w9c, np.float32).astype(
      np.float64)
  acc = np.zeros_like(D64)
  with np.errstate(invalid='ignore', over='ignore'):
    for ky in range(3):
      for kx in range(3):
        dy, dx = -(ky - 1) * rate, -(kx - 1) * rate
        ok = _valid(D64.shape[1:3], dy, dx)[None, :, :, None]
        term = w64[3 * ky + kx] * _shifted(D64, dy, dx)
        acc = np.where(ok, acc + term, acc)
    out = acc.astype(np.float32)
  if Y is not None:
    with np.errstate(invalid='ignore'):
      out = np.where(np.asarray(Y) <= 0, np.float32(0.0), out)
  return out
