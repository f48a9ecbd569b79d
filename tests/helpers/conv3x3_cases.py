"""Case table of the dense 3x3 convolution epos_conv3x3_f32 (include/epos_hip.h), which runs as
an implicit GEMM inside the CONV instantiations of pointwise_gemm_h2_f32 (epos_amd/csrc/
pointwise_gemm_h2.hip) and pointwise_gemm_split_f32 (pointwise_gemm_split.hip); tests/
test_gpu_conv3x3_regimes.py. In the style of tests/helpers/h2_presplit_cases.py: the cases, a
classifier of the launch regimes a case takes -- written from epos_conv3x3_f32, launch_grouped_h2
and launch_grouped_split, sharing no code with them --, the inputs of every value kind and the
fp64 expectation. Pure numpy: tests/test_conv3x3_cases_host.py checks without a GPU that the
table reaches every regime the GPU tests are written for and that no case is dead.

A problem: Y[B, Ho, Wo, Cout] = act(conv3x3(X[B, H, W, Cin], w[3, 3, Cin, Cout]) + bias), output
(y, x) reading input (y*stride + (ky-1)*rate, x*stride + (kx-1)*rate), taps outside the image
zero, Ho = (H-1)/stride + 1. X lies in a buffer of ldx columns with x_guard_rows NaN rows in
front of the first pixel and behind the last and NaN in the columns Cin..ldx of every row; Y
starts y_off floats into a sentinel-filled buffer of row pitch ldy with GUARD_BEFORE rows in
front and guard_after(M) behind. Everything a correct kernel touches lies inside its own
allocation, and so does everything a kernel with a wrong tap, row or column would touch."""
import collections
import functools

import numpy as np

from helpers import heads_cases as hc

BM = 128                           # rows of an h2 tile, and of the split kernel's large tile
H2_BK, H2_NST = 16, 5              # channels per K step and stages of the ring, h2
SP_BK, SP_NST = 16, 4              # ... and of the split kernel
SPLIT_ROWS128_FROM = 200           # 128-row tiles in the split kernel from this many tiles on
GUARD_BEFORE = hc.GUARD_BEFORE
SENTINEL_BITS = hc.SENTINEL_BITS
H2_MAX_REL_ERR = hc.H2_MAX_REL_ERR      # the project's bar for the two product GEMM kernels
KERNELS = ('h2', 'split')
KINDS = ('int', 'normal', 'relu_like')
SLOTS = ('given', 'measured', 'stale')
INT_MAX = 15                       # 'int' data: integers in [-15, 15]
BIG = 1 << 30

# what the entry point refuses before anything is launched (test_conv3x3_refusals)
REFUSALS = ('null_x', 'null_wp', 'null_y', 'cin_48', 'ldx_lt_cin', 'ldx_mod_4', 'x_unaligned',
            'stride_3', 'rate_0', 'b_0', 'no_wh_no_ws', 'm_8', 'y_amax_cout_mod_4',
            'y_amax_ldy_mod_4', 'y_amax_y_unaligned')


def _cdiv(a, b):
  return -(-a // b)


_Case = collections.namedtuple(
    '_Case', 'name b h w cin cout stride rate bias relu ldx y_off ldy slot y_amax kinds expect '
             'seed')


def Case(name, b, h, w, cin, cout, expect, stride=1, rate=1, bias=True, relu=1, ldx_pad=0,
         y_off=0, ldy_pad=0, slot='given', y_amax=False, kinds=('int', 'normal')):
  """ldx = Cin + ldx_pad; Y starts y_off floats behind a 16-byte aligned address and has row
  pitch ldy = y_off + Cout + ldy_pad; slot: what the h2 launch gets as x_amax."""
  assert slot in SLOTS and all(k in KINDS for k in kinds) and kinds and stride in (1, 2)
  assert cin % 32 == 0 and ldx_pad % 4 == 0 and rate >= 1
  c = _Case(name, b, h, w, cin, cout, stride, rate, bool(bias), int(relu), cin + ldx_pad, y_off,
            y_off + cout + ldy_pad, slot, bool(y_amax), tuple(kinds), tuple(expect), 0)
  assert not c.y_amax or vec(c), 'y_amax needs the float4 epilogue'
  return c


def by_name(table):
  d = {c.name: c for c in table}
  assert len(d) == len(table), 'duplicate case names'
  return d


def out_hw(case):
  return (case.h - 1) // case.stride + 1, (case.w - 1) // case.stride + 1


def m_of(case):
  ho, wo = out_hw(case)
  return case.b * ho * wo


# ------------------------------------------------------------------- launcher mirror ---
def kernel_taken(wh, ws, m):
  """epos_conv3x3_f32 in the product library: Wh (its bound given, or measured by the library)
  -> h2; otherwise Ws -> split; otherwise, and for M <= 8 whatever came along, refused."""
  if m <= 8:
    return None
  return 'h2' if wh else 'split' if ws else None


def tiles128(case):
  """ceil(M / 128) * ceil(N / 128): the h2 launch's workgroups (a conv never takes the narrow
  tile) and the number the split launcher chooses its row tile by."""
  return _cdiv(m_of(case), BM) * _cdiv(case.cout, 128)


def split_rows(case):
  return 128 if tiles128(case) >= SPLIT_ROWS128_FROM else 64


def k_steps(case, kernel):
  """K steps of the implicit GEMM: both kernels walk a tap in blocks of 16 channels."""
  return 9 * case.cin // (H2_BK if kernel == 'h2' else SP_BK)


def vec(case):
  """The float4 epilogue: N and ldy multiples of 4, Y 16-byte aligned (the Y buffers are
  512-byte aligned and GUARD_BEFORE = 4 rows precede the matrix)."""
  return case.cout % 4 == 0 and case.ldy % 4 == 0 and case.y_off % 4 == 0


def regime_names(case):
  s = set(KERNELS)                                       # every case runs through both kernels
  ho, wo = out_hw(case)
  m = case.b * ho * wo
  s.add('split_rows%d' % split_rows(case))
  if tiles128(case) == SPLIT_ROWS128_FROM:
    s.add('split_tiles_200')
  if case.cin in (32, 64, 96, 128, 160, 512):
    s.add('cin%d' % case.cin)
  if case.stride == 1:
    if case.rate in (1, 2, 4):
      s.add('stride1_rate%d' % case.rate)
  else:
    if case.h % 2 and case.w % 2:
      s.add('stride2_odd')
    if case.h % 2 == 0 and case.w % 2 == 0:
      s.add('stride2_even')
    if case.rate == 2:
      s.add('stride2_rate2')
  if case.rate >= case.w and case.rate >= case.h:
    s.add('rate_ge_hw')
  elif case.rate >= case.w:
    s.add('rate_ge_w')
  elif case.rate >= case.h:
    s.add('rate_ge_h')
  if case.b >= 2 and (ho * wo) % BM:
    s.add('batch_boundary_in_tile')
  if case.b == 3:
    s.add('images_3')
  s.add('ragged_m' if m % BM else 'm_multiple_of_128')
  if case.cout <= 64:
    s.add('n_le_64')
  if 128 < case.cout <= 256:
    s.add('n_two_tiles')
  if case.cout % 32:
    s.add('n_ragged')
  if vec(case):
    s.add('epilogue_vec')
  else:
    s.add('epilogue_scalar')
    s.add('epilogue_scalar_by_n' if case.cout % 4 else 'epilogue_scalar_by_alignment')
  if case.ldx > case.cin:
    s.add('ldx_padded')
    if case.ldx - case.cin in (4, 36):
      s.add('ldx_pad%d' % (case.ldx - case.cin))
  if case.y_off and case.ldy > case.y_off + case.cout:
    s.add('ldy_padded_offset')
  if not case.bias:
    s.add('bias_none')
  if not case.relu:
    s.add('relu_off')
  s.add('slot_' + case.slot)
  if case.slot == 'measured':                   # the rows measured: B*H*W, which is M at stride 1
    s.add('slot_measured_stride%d' % case.stride)
  if case.y_amax:
    s.add('y_amax')
  for k in case.kinds:
    s.add('values_' + k)
  return s


REQUIRED_REGIMES = tuple(
    ['h2', 'split', 'split_rows64', 'split_rows128', 'split_tiles_200'] +
    ['cin%d' % c for c in (32, 64, 96, 128, 160, 512)] +
    ['stride1_rate1', 'stride1_rate2', 'stride1_rate4', 'rate_ge_w', 'rate_ge_h', 'rate_ge_hw',
     'stride2_odd', 'stride2_even', 'stride2_rate2'] +
    ['batch_boundary_in_tile', 'images_3', 'ragged_m', 'm_multiple_of_128', 'n_le_64',
     'n_two_tiles', 'n_ragged'] +
    ['epilogue_vec', 'epilogue_scalar', 'epilogue_scalar_by_n', 'epilogue_scalar_by_alignment',
     'ldx_padded', 'ldx_pad4', 'ldx_pad36', 'ldy_padded_offset', 'bias_none', 'relu_off'] +
    ['slot_' + k for k in SLOTS] + ['slot_measured_stride1', 'slot_measured_stride2', 'y_amax'] +
    ['values_' + k for k in KINDS])

# Small: B*H*W <= 400 pixels, Cin <= 160, Cout <= 264 -- except the cases of SIZE_EXCEPTIONS.
# Cin = 32 .. 160 give 18, 36, 54, 72 and 90 K steps: every residue mod 5 (the h2 ring) and both
# residues mod 4 the split ring can see (a tap is a whole number of steps, so 9 Cin / 16 is
# always even); tests/test_conv3x3_cases_host.py checks this.
CASES = (
    Case('s1_r1_cin32', 2, 9, 13, 32, 64,
         ['h2', 'split', 'split_rows64', 'cin32', 'stride1_rate1', 'batch_boundary_in_tile',
          'ragged_m', 'n_le_64', 'epilogue_vec', 'slot_given', 'values_int', 'values_normal']),
    Case('s1_r2_cin64', 1, 16, 16, 64, 136,
         ['cin64', 'stride1_rate2', 'm_multiple_of_128', 'n_two_tiles', 'n_ragged',
          'values_relu_like'], rate=2, kinds=('int', 'relu_like')),
    Case('s1_r4_cin96', 1, 11, 17, 96, 40, ['cin96', 'stride1_rate4', 'bias_none', 'y_amax'],
         rate=4, bias=False, y_amax=True),
    Case('cin128_n37', 1, 9, 11, 128, 37,
         ['cin128', 'epilogue_scalar', 'epilogue_scalar_by_n', 'relu_off'], relu=0),
    Case('cin160_y_off1', 2, 7, 9, 160, 72,
         ['cin160', 'epilogue_scalar_by_alignment', 'ldx_padded', 'ldx_pad4'],
         ldx_pad=4, y_off=1, ldy_pad=1, kinds=('int', 'relu_like')),
    Case('rate_ge_w', 1, 23, 5, 32, 64, ['rate_ge_w', 'ldx_pad36'], rate=6, ldx_pad=36),
    Case('rate_ge_h', 2, 3, 40, 32, 48, ['rate_ge_h'], rate=3),
    Case('rate_ge_hw', 2, 6, 7, 64, 40, ['rate_ge_hw'], rate=7),
    Case('s2_odd_measured', 1, 15, 21, 32, 72,
         ['stride2_odd', 'slot_measured', 'slot_measured_stride2', 'ldx_padded'],
         stride=2, ldx_pad=4, slot='measured'),
    Case('s2_even_y_slice', 2, 12, 16, 64, 72, ['stride2_even', 'ldy_padded_offset'],
         stride=2, y_off=4, ldy_pad=4, relu=0),
    Case('s2_r2_stale', 1, 13, 18, 96, 40, ['stride2_rate2', 'slot_stale'], stride=2, rate=2,
         slot='stale', kinds=('int', 'relu_like')),
    Case('images_3', 3, 8, 13, 32, 136, ['images_3', 'batch_boundary_in_tile', 'y_amax'],
         rate=2, y_amax=True),
    # a self-measurement over too MANY rows or columns (NaN guard rows, 36 NaN padding columns)
    Case('s1_measured', 2, 10, 11, 64, 200, ['slot_measured_stride1', 'ldx_pad36'],
         ldx_pad=36, slot='measured', kinds=('int', 'relu_like')),
    # ---- the three cases above the size cap
    Case('rows128', 2, 80, 81, 32, 136, ['split_rows128', 'ragged_m', 'n_two_tiles'],
         kinds=('int', 'relu_like')),
    Case('tiles_200', 1, 80, 160, 32, 136, ['split_tiles_200', 'split_rows128'], rate=2,
         kinds=('int',)),
    Case('cin512', 1, 5, 7, 512, 40, ['cin512'], kinds=('int', 'normal')),
)
CASES = tuple(c._replace(seed=i) for i, c in enumerate(CASES))

SIZE_EXCEPTIONS = ('rows128', 'tiles_200', 'cin512')

# (X, Y) of the launch-history test: Y has another Cin, rate, K-step count and tile count than X
HISTORY_PAIR = ('s1_r2_cin64', 's1_r4_cin96')
STREAM_CASE = 'cin160_y_off1'
GRAPH_CASE = 's1_r4_cin96'
REFUSAL_CASE = 's1_r4_cin96'
IMAGES_CASE = 'images_3'


# ------------------------------------------------------------------------------ layout ---
def x_guard_rows(case):
  """NaN rows in front of the first pixel and behind the last: more than the farthest tap of any
  pixel reaches (rate rows and rate pixels)."""
  return case.rate * (case.w + 1) + 2


def guard_after(m):
  """Sentinel rows behind Y: the dead rows of the last 128-row tile and two more."""
  return _cdiv(m, BM) * BM - m + 2


YBuf = collections.namedtuple('YBuf', 'rows width floats off')


def y_layout(case, m=None):
  """The Y buffer: flat, [rows, ldy] + 4 floats of slack; Y starts `off` floats into it."""
  m = m_of(case) if m is None else m
  rows = GUARD_BEFORE + m + guard_after(m)
  return YBuf(rows, case.ldy, rows * case.ldy + 4, GUARD_BEFORE * case.ldy + case.y_off)


def y_index(case, m=None):
  """Flat indices [M, Cout] of Y's elements in its buffer."""
  m = m_of(case) if m is None else m
  return (y_layout(case, m).off + np.arange(m)[:, None] * case.ldy +
          np.arange(case.cout)[None, :])


def written_mask(case, m=None):
  mask = np.zeros(y_layout(case, m).floats, bool)
  mask[y_index(case, m)] = True
  return mask


# ---------------------------------------------------------------------------- reference ---
def conv_ref(x, w_hwio, bias, stride, rate, relu):
  """fp64, from the sentence in include/epos_hip.h: output (y, x) reads input
  (y*stride + (ky-1)*rate, x*stride + (kx-1)*rate), taps outside the image are zero,
  Ho = (H-1)/stride + 1. x [B, H, W, Cin], w [3, 3, Cin, Cout] -> [B, Ho, Wo, Cout]."""
  x = np.asarray(x, np.float64)
  w = np.asarray(w_hwio, np.float64)
  b, h, wd, _ = x.shape
  ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
  out = np.zeros((b, ho, wo, w.shape[3]))
  for ky in range(3):
    for kx in range(3):
      dy, dx = (ky - 1) * rate, (kx - 1) * rate
      ys = [y for y in range(ho) if 0 <= y * stride + dy < h]
      xs = [v for v in range(wo) if 0 <= v * stride + dx < wd]
      if not ys or not xs:
        continue
      iy = np.array(ys) * stride + dy
      ix = np.array(xs) * stride + dx
      out[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] += x[:, iy][:, :, ix] @ w[ky, kx]
  if bias is not None:
    out += np.asarray(bias, np.float64)
  return np.maximum(out, 0) if relu else out


def conv_ref_mag(x, w_hwio, bias, stride, rate, relu):
  """(ref, mag): mag = conv_ref(|x|, |w|, |bias|) without the ReLU = sum |x||w| + |bias|."""
  ref = conv_ref(x, w_hwio, bias, stride, rate, relu)
  mag = conv_ref(np.abs(x), np.abs(w_hwio), None if bias is None else np.abs(bias), stride, rate,
                 False)
  return ref, mag


def im2col(x, stride, rate):
  """[B*Ho*Wo, 9*Cin] in x's dtype: column (ky*3 + kx)*Cin + c, the row order of the weights."""
  b, h, wd, c = x.shape
  ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
  xp = np.zeros((b, h + 2 * rate, wd + 2 * rate, c), x.dtype)
  xp[:, rate:rate + h, rate:rate + wd] = x
  cols = [xp[:, ky * rate:ky * rate + (ho - 1) * stride + 1:stride,
             kx * rate:kx * rate + (wo - 1) * stride + 1:stride]
          for ky in range(3) for kx in range(3)]
  return np.concatenate(cols, axis=3).reshape(b * ho * wo, 9 * c)


# ------------------------------------------------------------------------------ values ---
Inputs = collections.namedtuple('Inputs', 'x w bias true_max')


@functools.lru_cache(maxsize=None)
def inputs(name, kind):
  """x fp32 [B, H, W, Cin], w fp32 [3, 3, Cin, Cout], bias fp32 [Cout] or None, max |x|.
  'int': integers in [-15, 15], x without a zero (a read of the wrong pixel cannot hide as a
  read of nothing) -- exact in both kernels: the piece products are exact, the scales powers of
  two, every sum below 2^24. 'normal': x ~ N(0, 1), w ~ N(0, 1) / sqrt(9 Cin), bias ~ N(0, 1).
  'relu_like': x = max(N(0, 1), 0).
  Where the library measures X itself (slot 'measured'), the first B*Ho*Wo pixels -- what a
  measurement over M rows instead of B*H*W would see -- stay below a quarter of max |x| and the
  last pixel holds the maximum: a bound taken from too few rows overflows the fp16 pairs."""
  case = by_name(CASES)[name]
  assert kind in case.kinds
  rng = np.random.default_rng(9000 + 8 * case.seed + KINDS.index(kind))
  shape = (case.b, case.h, case.w, case.cin)
  if kind == 'int':
    x = (rng.integers(1, INT_MAX + 1, shape) * rng.choice([-1, 1], shape)).astype(np.float32)
    w = rng.integers(-INT_MAX, INT_MAX + 1, (3, 3, case.cin, case.cout)).astype(np.float32)
    bias = rng.integers(-INT_MAX, INT_MAX + 1, case.cout).astype(np.float32)
  else:
    x = rng.standard_normal(shape).astype(np.float32)
    if kind == 'relu_like':
      x = np.maximum(x, 0)
    w = (rng.standard_normal((3, 3, case.cin, case.cout)) / np.sqrt(9 * case.cin)).astype(
        np.float32)
    bias = rng.standard_normal(case.cout).astype(np.float32)
  if case.slot == 'measured':
    flat = x.reshape(-1, case.cin)
    m = m_of(case)
    if kind == 'int':
      flat[:m] = np.clip(flat[:m], -3, 3)
      flat[-1, -1] = -INT_MAX
    else:
      flat[-1, -1] = np.float32(4) * np.abs(flat).max()
      flat[:m] *= np.float32(0.25)
  out = Inputs(x, w, bias if case.bias else None, np.float32(np.abs(x).max()))
  for a in out[:3]:
    if a is not None:
      a.setflags(write=False)
  return out


@functools.lru_cache(maxsize=None)
def expected(name, kind):
  """(ref, mag) in fp64 as [M, Cout]. Computed once."""
  case = by_name(CASES)[name]
  inp = inputs(name, kind)
  ref, mag = conv_ref_mag(inp.x, inp.w, inp.bias, case.stride, case.rate, case.relu)
  ref, mag = ref.reshape(-1, case.cout), mag.reshape(-1, case.cout)
  ref.setflags(write=False)
  mag.setflags(write=False)
  return ref, mag


@functools.lru_cache(maxsize=None)
def fp32_product_error(name, kind):
  """max |a32 @ w32 (+ bias) - ref| / mag of a float32 numpy im2col product of the same inputs:
  the yardstick of the cin512 case (K = 4608, where H2_MAX_REL_ERR has never been measured)."""
  case = by_name(CASES)[name]
  inp = inputs(name, kind)
  ref, mag = expected(name, kind)
  got = im2col(inp.x, case.stride, case.rate) @ inp.w.reshape(9 * case.cin, case.cout)
  if inp.bias is not None:
    got = got + inp.bias
  if case.relu:
    got = np.maximum(got, 0)
  assert got.dtype == np.float32
  return float((np.abs(got.astype(np.float64) - ref) / mag).max())


def slot_word(case, true_max):
  """The bit pattern the h2 launch finds in its x_amax slot; None: x_amax == NULL."""
  t = np.float32(true_max)
  if case.slot == 'measured':
    return None
  if case.slot == 'stale':
    t = t * np.float32(1024)
  return int(t.view(np.uint32))


def scale_ratio(case, true_max):
  """The power of two by which the case's slot moves the h2 scale below the one of the exact
  maximum (>= 1; heads_cases.scale_ratio restated for one slot): the factor on the bar."""
  w = slot_word(case, true_max)
  if w is None:
    return 1.0
  e_true = hc.h2_scale_exp([int(np.float32(true_max).view(np.uint32))])
  return float(2.0 ** max(e_true - hc.h2_scale_exp([w]), 0))


def x_buffer(case, kind):
  """X's whole allocation as fp32 [guard + B*H*W + guard, ldx]: NaN everywhere but in the Cin
  columns of the pixel rows. X itself starts at row x_guard_rows(case)."""
  g, n = x_guard_rows(case), case.b * case.h * case.w
  buf = np.full((g + n + g, case.ldx), np.nan, np.float32)
  buf[g:g + n, :case.cin] = inputs(case.name, kind).x.reshape(n, case.cin)
  return buf
