"""numpy references and seeded inputs for the tables of tests/helpers/glue_cases.py.

Exact operations (max pool, subsample, add+relu, argmax, scatter) are plain numpy and the GPU
result must be array_equal. Resize and the means are restated in float32 IN THE KERNELS' ORDER OF
OPERATIONS (the library is built with -ffp-contract=off, so a float32 numpy expression of the same
shape gives the same bits); tests/test_glue_cases_host.py holds these restatements to derived
bounds against float64. The correspondences come from oracle/corresp_ref.py, slot by slot.
"""
import functools
import zlib

import numpy as np

from helpers import glue_cases as gc
from helpers.bf16_ref import bf16_round, bf16_round_bits

F32 = np.float32


def rng_for(kind, case):
  return np.random.RandomState(zlib.crc32(('%s/%s/%d' % (kind, case.name, case.seed)).encode())
                               & 0x7fffffff)


# --------------------------------------------------------------------------------- means ---
def mean_input(case, bf16=False):
  """[b, hw, c] float32 (bf16: already rounded to bf16 values); a third of the images carry an
  offset so that the sums do not hover around zero."""
  x = rng_for('mean', case).standard_normal((case.b, case.hw, case.c)).astype(F32)
  x[::3] += F32(1.5)
  return bf16_round(x) if bf16 else x


def partial_input(case):
  return rng_for('partial', case).standard_normal((case.b, case.blocks, case.c)).astype(F32) * \
      F32(32.0)


def mean_f32(x, phases, divisor=None):
  """The kernels' fixed order: phase p adds rows p, p + phases, ... in order (the eight-row loop
  of global_avg_pool_kernel adds its eight rows in the same order); then the `phases` partial
  sums in index order, starting from phase 0's; then one division. phases = 64
  (global_avg_pool_kernel), 32 (global_avg_pool_bf16_kernel), 16 (pool_partial_kernel, whose
  divisor is hw, not the row count)."""
  x = np.ascontiguousarray(x, F32)
  b, hw, c = x.shape
  part = np.zeros((b, phases, c), F32)
  for r0 in range(0, hw, phases):
    n = min(phases, hw - r0)
    part[:, :n] = part[:, :n] + x[:, r0:r0 + n]
  t = part[:, 0].copy()
  for i in range(1, phases):
    t = t + part[:, i]
  return (t / F32(hw if divisor is None else divisor)).astype(F32)


def mean_f64(x, divisor=None):
  x = np.asarray(x, np.float64)
  return x.sum(1) / (x.shape[1] if divisor is None else divisor)


# -------------------------------------------------------------------------------- resize ---
def resize_input(case, bf16=False):
  x = rng_for('resize', case).standard_normal((case.b, case.hi, case.wi, case.c)).astype(F32)
  return bf16_round(x) if bf16 else x


def _resize_coords_f32(ni, no):
  """resize_bilinear_kernel: s = float(ni - 1) / (no - 1) in float32 (0 for no == 1),
  f = o * s in float32, i0 = floor(f), i1 = min(ceil(f), ni - 1), l = f - i0."""
  s = F32(ni - 1) / F32(no - 1) if no > 1 else F32(0)
  f = np.arange(no, dtype=F32) * s
  i0 = np.floor(f).astype(np.int64)
  i1 = np.minimum(np.ceil(f).astype(np.int64), ni - 1)
  return i0, i1, (f - i0.astype(F32)).astype(F32)


def resize_f32(x, ho, wo):
  """float32 restatement of resize_bilinear_kernel on x [b, hi, wi, c]: returns the output and
  the four corner tensors (for the bounds)."""
  x = np.ascontiguousarray(x, F32)
  hi, wi = x.shape[1:3]
  y0, y1, ly = _resize_coords_f32(hi, ho)
  x0, x1, lx = _resize_coords_f32(wi, wo)
  ly, lx = ly[None, :, None, None], lx[None, None, :, None]
  tl, tr = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
  bl, br = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
  top = tl + (tr - tl) * lx
  bot = bl + (br - bl) * lx
  out = top + (bot - top) * ly
  assert out.dtype == F32
  return out, (tl, tr, bl, br)


def _resize_coords_exact(ni, no):
  """The exact sample positions o * (ni - 1) / (no - 1) as (cell, fraction) in integers."""
  o = np.arange(no, dtype=np.int64)
  if no == 1:
    return o * 0, np.minimum(o * 0 + 1, ni - 1) * 0, np.zeros(no)
  num, den = o * (ni - 1), no - 1
  i0 = num // den
  frac = (num % den) / den
  i1 = np.minimum(i0 + (num % den != 0), ni - 1)
  return i0, i1, frac


def resize_f64(x, ho, wo):
  """Exact-position bilinear interpolation in float64, and |tl| + |tr| + |bl| + |br|."""
  x = np.asarray(x, np.float64)
  hi, wi = x.shape[1:3]
  y0, y1, ly = _resize_coords_exact(hi, ho)
  x0, x1, lx = _resize_coords_exact(wi, wo)
  ly, lx = ly[None, :, None, None], lx[None, None, :, None]
  tl, tr = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
  bl, br = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
  top = tl + (tr - tl) * lx
  bot = bl + (br - bl) * lx
  return top + (bot - top) * ly, np.abs(tl) + np.abs(tr) + np.abs(bl) + np.abs(br)


def resize_bound(x, ho, wo):
  """The derived bound of the float32 restatement against resize_f64 (see
  tests/test_glue_cases_host.py): (2 d + 6 * 2^-24) * (|tl| + |tr| + |bl| + |br|) with
  d = 4 * 2^-24 * max(hi, wi); where float32 rounding moved the sample into the neighbouring
  cell, the magnitudes of both 2x2 cells."""
  hi, wi = x.shape[1:3]
  _, mag = resize_f64(x, ho, wo)
  _, (tl, tr, bl, br) = resize_f32(x, ho, wo)
  mag32 = (np.abs(tl) + np.abs(tr) + np.abs(bl) + np.abs(br)).astype(np.float64)
  ye, _, _ = _resize_coords_exact(hi, ho)
  xe, _, _ = _resize_coords_exact(wi, wo)
  yf, _, _ = _resize_coords_f32(hi, ho)
  xf, _, _ = _resize_coords_f32(wi, wo)
  moved = (ye != yf)[None, :, None, None] | (xe != xf)[None, None, :, None]
  d = 4 * 2.0 ** -24 * max(hi, wi)
  return (2 * d + 6 * 2.0 ** -24) * np.where(moved, mag + mag32, mag)


# ------------------------------------------------------------------- max pool, subsample ---
def pool_input(case, bf16=False):
  x = rng_for('pool', case).standard_normal((case.b, case.hi, case.wi, case.c)).astype(F32)
  if case.negative:
    x = -np.abs(x) - F32(0.25)
  return bf16_round(x) if bf16 else x


def max_pool_3x3_s2_same(x):
  """TF 'SAME' 3x3 stride-2 max pool of x [b, hi, wi, c]; padded cells never win."""
  b, hi, wi, c = x.shape
  ho, wo = (hi + 1) // 2, (wi + 1) // 2
  ty, tx = (ho - 1) * 2 + 3 - hi, (wo - 1) * 2 + 3 - wi
  py, px = max(ty, 0) // 2, max(tx, 0) // 2
  xp = np.full((b, hi + 4, wi + 4, c), -np.inf, x.dtype)
  xp[:, py:py + hi, px:px + wi] = x
  out = np.full((b, ho, wo, c), -np.inf, x.dtype)
  for ky in range(3):
    for kx in range(3):
      out = np.maximum(out, xp[:, ky:ky + 2 * ho - 1:2, kx:kx + 2 * wo - 1:2])
  return out


def sub_input(case, bf16=False):
  x = rng_for('sub', case).standard_normal((case.b, case.hi, case.wi, case.c)).astype(F32)
  return bf16_round(x) if bf16 else x


def subsample(x, factor):
  return np.ascontiguousarray(x[:, ::factor, ::factor])


# ------------------------------------------------------------------------------ add+relu ---
def add_relu_input(case, bf16=False):
  r = rng_for('add_relu', case)
  a, b = r.standard_normal(case.n).astype(F32), r.standard_normal(case.n).astype(F32)
  if case.negative:
    a, b = -np.abs(a) - F32(0.5), -np.abs(b)
  return (bf16_round(a), bf16_round(b)) if bf16 else (a, b)


def add_relu(a, b):
  return np.maximum(np.asarray(a, F32) + np.asarray(b, F32), F32(0))


def add_relu_bf16_bits(a, b):
  """One round-to-nearest-even of the fp32 sum's relu."""
  return bf16_round_bits(add_relu(a, b))


# -------------------------------------------------------------------------------- argmax ---
# rows with planted patterns (row index modulo the row count)
def argmax_input(case):
  x = (rng_for('argmax', case).standard_normal((case.p, case.c)) * 3).astype(F32)
  p, c = case.p, case.c
  if c >= 2:
    x[5 % p] = F32(1.25)                              # all tied: index 0
  if c >= 4 and p >= 16:
    x[7, :] = F32(-2.0); x[7, [c - 2, c - 1]] = F32(4.5)        # a tie at the end
    x[8, :] = F32(-1.0); x[8, [2, c - 1]] = F32(0.5)            # a tie away from index 0
    x[9, :] = -np.inf                                           # nothing but -inf: index 0
    x[10, :] = -np.inf; x[10, c // 2] = F32(-3.0e38)            # -inf at index 0, finite later
    x[11, :c - 1] = -np.inf; x[11, c - 1] = F32(0.0)            # the maximum in the last place
    x[12, 0] = np.inf; x[12, 3] = np.inf                        # +inf twice
  return x


def argmax(x):
  return np.argmax(x, axis=1).astype(np.int64)


def argmax_planted_ok(case, x, lab):
  """The planted rows are where they were meant to be (checked on the CPU)."""
  p, c = case.p, case.c
  if c >= 2 and lab[5 % p] != 0:
    return False
  if c >= 4 and p >= 16:
    return (lab[7], lab[8], lab[9], lab[10], lab[11], lab[12]) == (c - 2, 2, 0, c // 2, c - 1, 0)
  return True


# ------------------------------------------------------------------------------- softmax ---
def softmax_input(case):
  g, n = case.g, case.n
  x = (rng_for('softmax', case).standard_normal((n, g)) * 3).astype(F32)
  if n > 6:
    x[3] = np.where(np.arange(g) % 2, 80.0, -80.0)    # exp underflow next to 1
    x[4] = 1.25                                       # all tied
    x[5, :max(g // 2, 1)] = 2.5                       # a tied maximum
    x[6, g - 1] = 40.0                                # the maximum in the last lane
  return x


def softmax_f64(x):
  x = np.asarray(x, np.float64)
  e = np.exp(x - x.max(-1, keepdims=True))
  return e / e.sum(-1, keepdims=True)


# ------------------------------------------------------------------------------- scatter ---
def scatter_problem(case):
  """dst0 (float32, random), offsets (int64, blocks never overlap), src (float32)."""
  r = rng_for('scatter', case)
  nb, w, gap = case.n_blocks, case.width, case.gap
  lead = 5
  starts = lead + np.arange(nb, dtype=np.int64) * (w + gap)
  if case.order == 'desc':
    starts = starts[::-1].copy()
  elif case.order == 'shuffled':
    starts = starts[r.permutation(nb)]
  size = lead + nb * (w + gap) + 7
  dst0 = r.standard_normal(size).astype(F32)
  src = r.standard_normal(nb * w).astype(F32)
  return dst0, starts, src


def scatter(dst0, offsets, src, width):
  out = dst0.copy()
  for b, o in enumerate(offsets):
    out[o:o + width] = src[b * width:(b + 1) * width]
  return out


# ------------------------------------------------------------------------ correspondences ---
CORR_KEYS = ['px_id', 'frag_id', 'coord_2d', 'coord_3d', 'conf', 'conf_obj', 'conf_frag']
CORR_DTYPES = {'px_id': np.int64, 'frag_id': np.int64, 'coord_2d': np.float64,
               'coord_3d': np.float64, 'conf': F32, 'conf_obj': F32, 'conf_frag': F32}
CORR_WIDTH = {'px_id': 1, 'frag_id': 1, 'coord_2d': 2, 'coord_3d': 3, 'conf': 1, 'conf_obj': 1,
              'conf_frag': 1}
TAU_A = 0.85
TAU_B = 0.5
OUTPUT_SCALE = 0.25
TIE_PIXELS = (3, 40)            # raster indices (image 0 and 1, object 1) with a planted tie


def corr_num_objs(case):
  return gc.CORR_O if case.all_obj else gc.CORR_O - 1


def corr_data_key(case):
  return (case.f, case.h, case.w, bool(case.all_obj), case.seed)


def corr_problem(case):
  """Head tensors of a case: obj_confs [B, P, O + 1], frag_confs [B, P, O, F], frag_coords
  [B, P, O, F, 3] (float32), frag centers [O, F, 3] / sizes [O, F] (float64).
  Object 1: three pixels in eight masked (more than 1024 from P = 5063 on), object 3: about
  15 %; one to three fragments kept. Object 2: never
  above the threshold, some pixels exactly AT it (the test is a strict >). Object 4 (all_obj
  cases): every pixel masked, every fragment kept. At the TIE_PIXELS of object 1 (F >= 3)
  fragment 1 holds max * tau_b exactly (not kept: strict >) and fragment 2 the next float32
  above it (kept)."""
  # seeded by the data's shape alone: the offset and capacity variants of a case share its data
  r = np.random.RandomState(zlib.crc32(repr(corr_data_key(case)).encode()) & 0x7fffffff)
  B, O, F, P = gc.CORR_B, corr_num_objs(case), case.f, case.h * case.w
  obj = r.uniform(0, 1, (B, P, O + 1)).astype(F32)
  tau_a = F32(TAU_A)
  obj[:, :, 1] = F32(0.6) + F32(0.4) * obj[:, :, 1]              # object 1: 3 pixels in 8 masked
  obj[:, :, 2] = np.minimum(obj[:, :, 2], tau_a)                 # object 2: nowhere masked
  frag = (r.standard_normal((B, P, O, F)) * 3).astype(F32)
  frag = np.exp(frag - frag.max(-1, keepdims=True))
  frag = (frag / frag.sum(-1, keepdims=True)).astype(F32)
  if case.all_obj:
    obj[:, :, 4] = np.maximum(obj[:, :, 4], F32(0.9))
    frag[:, :, 3] = r.uniform(0.6, 1.0, (B, P, F)).astype(F32)
  for img in range(B):
    for p in TIE_PIXELS:
      if F >= 3 and p < P:
        obj[img, p, 1] = F32(0.95)
        row = frag[img, p, 0]
        row[:] = F32(0.01)
        row[0] = F32(0.75)
        row[1] = F32(0.75) * F32(TAU_B)
        row[2] = np.nextafter(row[1], F32(1))
  coords = r.standard_normal((B, P, O, F, 3)).astype(F32)
  centers = r.uniform(-80, 80, (O, F, 3))
  sizes = r.uniform(5, 40, (O, F))
  return obj, frag, coords, centers, sizes


def corr_reference(case):
  return _corr_reference(gc.Corr('data', *corr_data_key(case)[:3], all_obj=case.all_obj,
                                 seed=case.seed))


@functools.lru_cache(maxsize=2)
def _corr_reference(case):
  """(problem, per-slot oracle outputs, totals int32 [S, 2], slot_base int64 [S + 1], pooled
  outputs by key). totals[s] = (masked pixels, correspondences)."""
  from oracle import corresp_ref
  prob = corr_problem(case)
  obj, frag, coords, centers, sizes = prob
  B, O, F = gc.CORR_B, corr_num_objs(case), case.f
  h, w = case.h, case.w
  slots = gc.corr_slots(case)
  per_slot, totals = [], []
  for img, oid in slots:
    out = corresp_ref.establish_many_to_many(
        obj[img].reshape(h, w, O + 1), frag[img].reshape(h, w, O, F),
        coords[img].reshape(h, w, O, F, 3), [oid], [oid], {oid: centers[oid - 1]},
        {oid: sizes[oid - 1]}, OUTPUT_SCALE, TAU_A, TAU_B, True)
    res = out.get(oid)
    if res is None:
      res = {k: np.zeros((0,) + ((CORR_WIDTH[k],) if CORR_WIDTH[k] > 1 else ()), CORR_DTYPES[k])
             for k in CORR_KEYS}
    per_slot.append(res)
    masked = int((obj[img, :, oid] > F32(TAU_A)).sum())
    totals.append((masked, len(res['px_id'])))
  totals = np.asarray(totals, np.int32).reshape(len(slots), 2)
  slot_base = np.concatenate([[0], np.cumsum(totals[:, 1], dtype=np.int64)]).astype(np.int64)
  pooled = {k: np.concatenate([s[k] for s in per_slot], axis=0) for k in CORR_KEYS}
  return prob, per_slot, totals, slot_base, pooled


def corr_capacity(case, totals, slot_base):
  total = int(slot_base[-1])
  return {None: total, 'total-1': total - 1, 'slot0': int(totals[0, 1]), 'zero': 0}[
      case.capacity]
