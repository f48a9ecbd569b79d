"""Numpy restatement of epos_resize_bilinear_dgrad_f32 (csrc/resize_grad.hip; include/epos_hip.h,
"Resize input gradient"), written from that description: the adjoint of the align-corners
bilinear resize with the forward's own fp32 coordinates (glue_ref._resize_coords_f32), the same
operations in the same stated order, and the bound. No shared code with the package."""
import numpy as np

from tests.helpers.glue_ref import _resize_coords_exact, _resize_coords_f32


def axis_taps(ni, no):
  """Per output index o of an axis ni -> no: the list of (source index, weight) of its DISTINCT
  taps, in fp64 from the forward's fp32 fraction l: [(i0, 1 - l), (i1, l)], or [(i0, 1.0)] where
  both taps name the same index (l == 0, and the clamped last coordinate)."""
  i0, i1, l = _resize_coords_f32(ni, no)
  i0 = np.minimum(i0, ni - 1)
  taps = []
  for o in range(no):
    if i0[o] == i1[o]:
      taps.append([(int(i0[o]), 1.0)])
    else:
      lo = float(np.float64(l[o]))
      taps.append([(int(i0[o]), 1.0 - lo), (int(i1[o]), lo)])
  return taps


def axis_matrix(ni, no, exact=False):
  """W f64 [no, ni]: the weight of source index i on output index o -- with the forward's fp32
  coordinates, or (exact) with the exact positions o (ni - 1) / (no - 1)."""
  Wm = np.zeros((no, ni))
  if exact:
    i0, i1, fr = _resize_coords_exact(ni, no)
    for o in range(no):
      if i0[o] == i1[o]:
        Wm[o, i0[o]] = 1.0
      else:
        Wm[o, i0[o]], Wm[o, i1[o]] = 1.0 - fr[o], fr[o]
    return Wm
  for o, taps in enumerate(axis_taps(ni, no)):
    for i, w in taps:
      Wm[o, i] = w
  return Wm


def resize_dgrad(D, hi, wi, Y=None, dtype=np.float64):
  """dX f32 [B,hi,wi,C], to be matched BIT FOR BIT: one fp64 accumulator per element from +0.0;
  the output pixels in (yo, xo) order, rows ascending, columns ascending within a row, each
  adding to the sources its taps name w = wy * wx, p = w * (double)D, acc += p, every operation
  rounded once; rounded to fp32 once; +0.0 where Y <= 0. dtype=np.longdouble: the same sum in
  extended precision, returned unrounded and unmasked together with sum |w||D| and the number of
  output pixels in every element's footprint (for the bound)."""
  D = np.asarray(D, np.float32)
  B, ho, wo, C = D.shape
  Dd = D.astype(dtype)
  ty, tx = axis_taps(hi, ho), axis_taps(wi, wo)
  acc = np.zeros((B, hi, wi, C), dtype)
  mag = np.zeros((B, hi, wi, C), dtype)
  count = np.zeros((hi, wi), np.int64)
  wide = dtype is not np.float64
  with np.errstate(invalid='ignore', over='ignore'):
    for yo in range(ho):
      for yi, wy in ty[yo]:
        for xo in range(wo):
          d = Dd[:, yo, xo, :]
          for xi, wx in tx[xo]:
            w = dtype(wy) * dtype(wx)
            acc[:, yi, xi, :] += w * d
            if wide:
              mag[:, yi, xi, :] += abs(w) * np.abs(d)
              count[yi, xi] += 1
  if wide:
    return acc, mag, count
  out = acc.astype(np.float32)
  if Y is not None:
    with np.errstate(invalid='ignore'):
      out = np.where(np.asarray(Y) <= 0, np.float32(0.0), out)
  return out


def bound(exact, mag, count):
  """2^-24 |exact| + (n + 16) 2^-52 sum |w||D|, n = the output pixels of the element's
  footprint: the one rounding to fp32, and an fp64 sum of n products, each with at most three
  roundings of its own (w, p, the addition; Higham, eq. 4.4, to first order (n + 2) 2^-53 of sum
  |w||D|; the rest of the allowance covers the second-order terms)."""
  n = np.asarray(count, np.float64)[None, :, :, None]
  fin = lambda a: np.where(np.isfinite(a), a, 0.0)                       # noqa: E731
  return (2.0 ** -24 * np.abs(fin(np.asarray(exact, np.float64))) +
          (n + 16.0) * 2.0 ** -52 * fin(np.asarray(mag, np.float64)))


def sources_of(yo, xo, hi, wi, ho, wo):
  """The distinct source pixels (yi, xi) that output pixel (yo, xo) adds to."""
  return sorted({(yi, xi) for yi, _ in axis_taps(hi, ho)[yo] for xi, _ in axis_taps(wi, wo)[xo]})
