"""Case table of the fp16-pair GEMM on a PRE-SPLIT A operand (pointwise_gemm_h2_f32 with
EposPointwiseArgs.a_presplit, epos_amd/csrc/pointwise_gemm_h2.hip; tests/test_gpu_h2_presplit.py),
in the style of tests/helpers/heads_cases.py: the cases, a classifier of the launch regimes a
case takes -- written from launch_grouped_h2 and the kernel, sharing no code with them --, the
host-side encoder of every value kind and the fp64 expectation from the DECODED pairs, so that
the reference is exact for what the kernel was given. Pure numpy: tests/
test_h2_presplit_cases_host.py checks without a GPU that the table reaches every regime the GPU
tests are written for and that no case is dead.

A problem: C[M, N] = A[M, K] W[K, N] (+ bias) (+ R) (ReLU). A is M rows of fp16 pairs with row
pitch lda (per four k: [4 hi | 4 mid], the layout EposDepthwiseArgs.y_h2 writes); every word of
A's allocation that the kernel must not read -- columns K..lda of every row and A_NAN_ROWS rows
behind row M - 1 -- holds A_POISON_BITS, whose two fp16 halves are both NaN (and which is an
fp32 NaN for the fp32-A launches of the same problem). C starts c_off floats into a buffer of
row pitch ldc with GUARD_BEFORE sentinel rows in front and guard_after(M) behind.

"""
import collections
import functools

import numpy as np

from helpers import heads_cases as hc
from helpers import pointwise_wgrad_ref as wr

BM, BK, NST = 128, 16, 5           # rows per tile, K per step, stages of the ring
BIG = 1 << 30                      # tile limit: 128 x 64 tiles wherever the launcher offers them
GUARD_BEFORE = hc.GUARD_BEFORE
A_NAN_ROWS = hc.A_NAN_ROWS
H2_MAX_REL_ERR = hc.H2_MAX_REL_ERR      # the project's bar, shared with the dense-heads tests
SENTINEL_BITS = hc.SENTINEL_BITS
A_POISON_BITS = 0x7fc17e01         # fp16 halves 0x7e01 and 0x7fc1: both NaN; as fp32: NaN
SCALES = tuple(k for k in hc.SCALES if k)       # None (no slot) is a refusal: REFUSALS
VALUES = ('relu_like', 'signed', 'zero_rows', 'window', 'noncanonical')
CANONICAL = ('relu_like', 'signed', 'zero_rows', 'window')
HI_MAX = 2.0 ** 15 - 16            # the largest |hi| a scale that keeps its bound allows

REFUSALS = ('no_a_amax', 'sub_2', 'relu_in', 'm_8', 'mixed_kinds', 'col_sums_with_residual')


def _cdiv(a, b):
  return -(-a // b)


_Problem = collections.namedtuple(
    '_Problem', 'm n k lda ldc c_off bias res ldr relu c_stream c_amax col_sums images')


def P(m, n, k, pad_a=False, c_off=0, pad=0, bias=True, res=False, relu=0, c_stream=0,
      c_amax=False, col_sums=False, images=1):
  """pad_a: lda = K rounded up to 32 floats (the plan's pitch), which must exceed K; pad: free
  floats behind the N columns (ldc = c_off + N + pad); res: a residual with ldr = N + 4."""
  lda = _cdiv(k, 32) * 32 if pad_a else k
  assert k % 4 == 0 and (not pad_a or lda > k) and m % images == 0
  return _Problem(m, n, k, lda, c_off + n + pad, c_off, bool(bias), bool(res),
                  n + 4 if res else 0, relu, c_stream, bool(c_amax), bool(col_sums), images)


_Case = collections.namedtuple('_Case', 'name problems scale values limit shared expect seed')


def Case(name, problems, expect, scale='pow2', values='relu_like', limit=0, shared=False):
  """shared: the problems write column slices of ONE buffer (the ASPP `cat` layout: ldc = the sum
  of the N's, each problem at its own c_off) and publish into ONE c_amax slot."""
  problems = tuple(problems)
  assert scale in SCALES and values in VALUES and limit in (0, BIG) and 1 <= len(problems) <= 8
  if shared:
    width, col, out = sum(p.n for p in problems), 0, []
    for p in problems:
      assert p.c_off == 0 and p.ldc == p.n
      out.append(p._replace(ldc=width, c_off=col))
      col += p.n
    problems = tuple(out)
  return _Case(name, problems, scale, values, limit, shared, tuple(expect), 0)


def by_name(table):
  d = {c.name: c for c in table}
  assert len(d) == len(table), 'duplicate case names'
  return d


# ------------------------------------------------------------------- launcher mirror ---
def launches(case):
  """The kernel launches a case becomes: a group with residuals goes out problem by problem."""
  if len(case.problems) > 1 and any(p.res for p in case.problems):
    return [(p,) for p in case.problems]
  return [case.problems]


def launch_shape(problems, limit):
  """(tile width, workgroups, per problem (row tiles, column tiles)) of ONE launch: 128 x 64
  tiles when the launch has at most `limit` 128 x 128 tiles and no problem wants block sums."""
  wide = sum(_cdiv(p.m, BM) * _cdiv(p.n, 128) for p in problems)
  narrow = wide <= limit and not any(p.col_sums for p in problems)
  bn = 64 if narrow else 128
  t = [(_cdiv(p.m, BM), _cdiv(p.n, bn)) for p in problems]
  return bn, sum(a * b for a, b in t), t


def vec(p):
  """The float4 epilogue: rows of C (and R) 16-byte aligned, N a multiple of 4. The C buffers
  are 512-byte aligned and GUARD_BEFORE = 4 rows precede the matrix."""
  return p.ldc % 4 == 0 and p.n % 4 == 0 and p.c_off % 4 == 0 and (not p.res or p.ldr % 4 == 0)


def regime_names(case):
  s = set()
  ls = launches(case)
  if len(ls) > 1:
    s.add('group_res_serial')
  for problems in ls:
    bn, _, t = launch_shape(problems, case.limit)
    res = problems[0].res
    if len(problems) > 1:
      s.add('narrow_64_group' if bn == 64 else 'group_128')
    else:
      s.add(('narrow_64' if bn == 64 else 'single_128') + ('_res' if res else ''))
    width = 'narrow' if bn == 64 else 'wide'
    for p, (tm, tn) in zip(problems, t):
      nks = _cdiv(p.k, BK)
      if nks <= 10 or nks == 46:
        s.add('nks_%d' % nks)
      s.add('krem_%d' % (p.k % BK))
      s.add('lda_eq_k' if p.lda == p.k else 'lda_padded')
      if p.m in (9, 127, 128, 129):
        s.add('m_%d' % p.m)
      if tm >= 3:
        s.add('m_3_row_tiles')
      s.add('nq%d_%s' % (((p.n - 1) % 128) // 32 + 1, width))
      if tn > 8 and tn % 8 and tm >= 2:
        s.add('band_' + width)
      if p.n % 4:
        s.add('scalar_by_n')
      elif not vec(p):
        s.add('scalar_by_alignment')
      if p.res and not vec(p):
        s.add('scalar_res')
      if p.c_off == 0:
        s.add('c_off_0')
      else:
        s.add('c_off_aligned' if p.c_off % 4 == 0 and p.ldc % 4 == 0 else 'c_off_unaligned')
      s.add('c_stream_%d' % p.c_stream)
      s.add('bias' if p.bias else 'no_bias')
      s.add('relu' if p.relu else 'no_relu')
      if p.res and p.ldr > p.n:
        s.add('res_ldr_gt_n')
      if p.c_amax:
        s.add('c_amax_cat' if case.shared and len(problems) > 1 else 'c_amax')
      if p.col_sums:
        if p.m % 32:
          s.add('col_sums_partial_block')
        if p.images == 2 and (p.m // 2) % 32 == 0:
          s.add('col_sums_two_images')
        if sum(_cdiv(q.m, BM) * _cdiv(q.n, 128) for q in problems) <= case.limit:
          s.add('col_sums_forces_wide')
  s.add('scale_' + case.scale)
  s.add('values_' + case.values)
  return s


REQUIRED_REGIMES = tuple(
    ['single_128', 'single_128_res', 'narrow_64', 'narrow_64_res', 'narrow_64_group',
     'group_128', 'group_res_serial'] +
    ['nks_%d' % i for i in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 46)] +
    ['krem_%d' % r for r in (0, 4, 8, 12)] +
    ['lda_eq_k', 'lda_padded'] +
    ['m_9', 'm_127', 'm_128', 'm_129', 'm_3_row_tiles'] +
    ['nq%d_%s' % (q, w) for q in (1, 2, 3, 4) for w in ('wide', 'narrow')] +
    ['scalar_by_n', 'scalar_by_alignment', 'scalar_res', 'band_wide', 'band_narrow'] +
    ['c_off_0', 'c_off_aligned', 'c_off_unaligned', 'c_stream_0', 'c_stream_1'] +
    ['bias', 'no_bias', 'relu', 'no_relu', 'res_ldr_gt_n', 'c_amax', 'c_amax_cat',
     'col_sums_partial_block', 'col_sums_two_images', 'col_sums_forces_wide'] +
    ['scale_' + k for k in SCALES] + ['values_' + v for v in VALUES])

# Every case is ALSO launched with the other tile limit (and must give the same bytes), so each
# K-step count, N quarter and epilogue below runs through both the 128 x 128 and the 128 x 64
# schedule; `limit` is the shape the case is named and classified for. N = 200: one column tile
# with four live column blocks and one with three.
#
# Measured on an MI355X, worst error / bound over the table per assertion family (RECORDED, not
# asserted: the starting point of a later tightening):
#   fp64 accuracy, |got - exact| / (H2_MAX_REL_ERR * mag):        0.598 (band_narrow, K = 16);
#                                                                 0.23 .. 0.43 for K >= 32
#   col_sums, |sum - fp64 sum| / (31 * 2^-24 * sum_block |c|):    0.090 (col_sums_two_images)
#   depthwise-written pairs on padded rows (test_gpu_h2_presplit.py), fp64 accuracy: 0.475
CASES = (
    # ---- K steps 1..10 (every residue of nks mod 5 past the first wrap), M edges, N quarters
    Case('k16_m9', [P(9, 200, 16)], ['single_128', 'nks_1', 'krem_0', 'm_9', 'nq3_wide']),
    Case('k32_m127_narrow', [P(127, 200, 32, bias=False, relu=1)],
         ['narrow_64', 'nks_2', 'm_127', 'nq3_narrow', 'no_bias', 'relu', 'scale_pow2_below',
          'values_signed'], scale='pow2_below', values='signed', limit=BIG),
    Case('k48_m128_res', [P(128, 200, 48, res=True, c_stream=1)],
         ['single_128_res', 'nks_3', 'm_128', 'res_ldr_gt_n', 'c_stream_1', 'scale_stale',
          'values_zero_rows'], scale='stale', values='zero_rows'),
    Case('k64_m129_res_narrow', [P(129, 200, 64, res=True, relu=1)],
         ['narrow_64_res', 'nks_4', 'm_129', 'scale_amax2', 'values_window'],
         scale='amax2', values='window', limit=BIG),
    Case('k80_noncanonical', [P(129, 136, 80, c_off=4, pad=4)],
         ['nks_5', 'nq1_wide', 'c_off_aligned', 'scale_gain', 'values_noncanonical'],
         scale='gain', values='noncanonical'),
    Case('k96_unaligned_narrow', [P(137, 136, 96, c_off=3, pad=1)],
         ['nks_6', 'nq1_narrow', 'c_off_unaligned', 'scalar_by_alignment'], limit=BIG),
    Case('k112_padded', [P(137, 180, 112, pad_a=True)], ['nks_7', 'lda_padded', 'nq2_wide']),
    Case('k128_narrow', [P(137, 180, 128, bias=False)], ['nks_8', 'nq2_narrow'],
         values='noncanonical', limit=BIG),
    Case('k144_padded', [P(137, 256, 144, pad_a=True, relu=1)], ['nks_9', 'nq4_wide'],
         values='signed'),
    Case('k160_narrow', [P(137, 256, 160, c_stream=1)], ['nks_10', 'nq4_narrow'],
         values='window', limit=BIG),
    # ---- partial last K step: K % 16 = 4, 8, 12; the scalar epilogue by N; three row tiles
    Case('k20_n22_m300', [P(300, 22, 20, pad_a=True)],
         ['krem_4', 'm_3_row_tiles', 'scalar_by_n']),
    Case('k40_n37_res_narrow', [P(137, 37, 40, pad_a=True, res=True)],
         ['krem_8', 'scalar_res'], values='signed', limit=BIG),
    Case('k92_padded', [P(137, 100, 92, pad_a=True)], ['krem_12'], values='zero_rows'),
    Case('k728_long', [P(257, 200, 728, pad_a=True, relu=1)], ['nks_46', 'lda_padded']),
    # ---- more than eight column tiles: the band order, last band narrower than 8
    Case('band_wide', [P(129, 1100, 16)], ['band_wide']),
    Case('band_narrow', [P(129, 1100, 16)], ['band_narrow'], limit=BIG),
    # ---- output absmax, groups, block sums, the non-finite bound
    Case('c_amax_single', [P(137, 200, 48, relu=1, c_amax=True)], ['c_amax'], values='signed'),
    Case('group_wide', [P(137, 136, 80), P(200, 72, 48, pad_a=True, relu=1), P(137, 200, 80)],
         ['group_128']),
    Case('group_narrow', [P(137, 136, 80), P(200, 72, 48, pad_a=True, relu=1), P(137, 200, 80)],
         ['narrow_64_group'], values='signed', limit=BIG),
    Case('group_cat_amax', [P(137, 72, 48, c_amax=True, relu=1), P(137, 136, 80, c_amax=True),
                            P(137, 64, 112, pad_a=True, c_amax=True, relu=1)],
         ['c_amax_cat'], values='signed', limit=BIG, shared=True),
    Case('group_res', [P(137, 136, 80, res=True, relu=1), P(137, 72, 48, res=True)],
         ['group_res_serial', 'single_128_res'], values='signed'),
    Case('col_sums_partial', [P(137, 136, 48, col_sums=True, relu=1)],
         ['col_sums_partial_block'], values='signed'),
    Case('col_sums_two_images', [P(192, 136, 48, col_sums=True, images=2)],
         ['col_sums_two_images', 'col_sums_forces_wide'], limit=BIG),
    Case('scale_inf', [P(137, 200, 48)], ['scale_inf'], scale='inf'),
)
CASES = tuple(c._replace(seed=i) for i, c in enumerate(CASES))

# (X, Y) of the launch-history test: Y has another instantiation, tile width, K-step count and
# epilogue than X
HISTORY_PAIR = ('k112_padded', 'k40_n37_res_narrow')
STREAM_CASE = 'group_narrow'
GRAPH_CASE = 'k144_padded'
REFUSAL_CASE = 'k112_padded'


# ------------------------------------------------------------------------------ layout ---
def guard_after(m):
  """Sentinel rows behind the matrix: the dead rows of the last row tile and two more."""
  return _cdiv(m, BM) * BM - m + 2


Buf = collections.namedtuple('Buf', 'rows width floats problems')     # problems: (index, off, ldc)


def layout(case):
  """The C buffers of a case: flat, [rows, width] + 4 floats of slack; problem i's C starts
  `off` floats into its buffer and has row pitch ldc."""
  if case.shared:
    m = case.problems[0].m
    assert all(p.m == m for p in case.problems)
    width = case.problems[0].ldc
    rows = GUARD_BEFORE + m + guard_after(m)
    return [Buf(rows, width, rows * width + 4,
                tuple((i, GUARD_BEFORE * width + p.c_off, width)
                      for i, p in enumerate(case.problems)))]
  out = []
  for i, p in enumerate(case.problems):
    rows = GUARD_BEFORE + p.m + guard_after(p.m)
    out.append(Buf(rows, p.ldc, rows * p.ldc + 4, ((i, GUARD_BEFORE * p.ldc + p.c_off, p.ldc),)))
  return out


def places(case):
  """Per problem: (buffer index, offset of C in floats, ldc)."""
  out = [None] * len(case.problems)
  for bi, b in enumerate(layout(case)):
    for i, off, ldc in b.problems:
      out[i] = (bi, off, ldc)
  return out


def written_mask(case, bi):
  """Boolean mask over flat C buffer bi: the elements the case must write, all others must keep
  the sentinel."""
  b = layout(case)[bi]
  mask = np.zeros(b.floats, bool)
  for i, off, ldc in b.problems:
    p = case.problems[i]
    idx = off + np.arange(p.m)[:, None] * ldc + np.arange(p.n)[None, :]
    assert not mask[idx].any()
    mask[idx] = True
  return mask


def sums_rows(p):
  """Rows of a problem's col_sums buffer: ceil(M / 32) block rows and two sentinel rows; its row
  pitch is N + 4."""
  return _cdiv(p.m, 32) + 2


# ------------------------------------------------------------------------------ values ---
def encode(x, s):
  """Canonical pairs of fp32 x [M, K] at scale s, as uint32 words [M, K]."""
  with np.errstate(invalid='ignore', over='ignore'):
    return wr.h2_split(x, s).view(np.uint32)


def pairs_from(hi, mid):
  """uint32 words [M, K] of fp16 hi, mid [M, K]: per four k [4 hi | 4 mid]."""
  m, k = hi.shape
  out = np.empty((m, k // 4, 2, 4), np.float16)
  out[:, :, 0, :] = hi.reshape(m, k // 4, 4)
  out[:, :, 1, :] = mid.reshape(m, k // 4, 4)
  return out.reshape(m, 2 * k).view(np.uint32)


def halves(words):
  """(hi, mid) fp16 [M, K] of uint32 pair words [M, K]."""
  words = np.ascontiguousarray(words, np.uint32)
  m, k = words.shape
  h = words.view(np.float16).reshape(m, k // 4, 2, 4)
  return h[:, :, 0, :].reshape(m, k), h[:, :, 1, :].reshape(m, k)


def _fp32_values(kind, m, k, rng):
  """(x fp32 [M, K], max |x|) of a canonical value kind."""
  if kind == 'signed':
    x = rng.standard_normal((m, k)).astype(np.float32)
  elif kind in ('relu_like', 'zero_rows'):
    x = np.maximum(rng.standard_normal((m, k)), 0).astype(np.float32)
    if kind == 'zero_rows':
      x[[0, 5, m - 1]] = 0
      x[32:64] = 0
      assert np.abs(x).max() > 0
  else:                                   # 'window'
    # by column: the bound, -bound, bound 2^-11 (exact on even rows: mid = 0), bound 2^-20,
    # bound 2^-30 (hi an fp16 subnormal), -0.0; random 24-bit mantissas below the bound elsewhere
    # (mid negative about as often as positive, subnormal in the 2^-30 class)
    top = np.float32(2.7182817)
    man = rng.uniform(0.5, 1.0, (m, k)).astype(np.float32)
    sign = rng.choice(np.float32([-1, 1]), (m, k))
    cls = (np.arange(k) % 6)[None, :] + np.zeros((m, 1), int)
    x = np.zeros((m, k), np.float32)
    x[cls == 0] = top
    x[cls == 1] = -top
    mid_exact = (np.arange(m) % 2 == 0)[:, None] & (cls == 2)
    x[cls == 2] = (sign * man * top * np.float32(2.0 ** -11))[cls == 2]
    x[mid_exact] = top * np.float32(2.0 ** -11)
    x[cls == 3] = (sign * man * top * np.float32(2.0 ** -20))[cls == 3]
    x[cls == 4] = (sign * man * top * np.float32(2.0 ** -30))[cls == 4]
    x[cls == 5] = np.float32(-0.0)
  return x, np.float32(np.abs(x).max())


def weights(kind, k, n, rng):
  """(W fp32 [K, N], bias [N]). For 'window' A the columns of the second half of N have no weight
  on the rows that meet |x| = bound, those of the last quarter none on the 2^-11 class either:
  there sum |a||w| is made of the small elements alone, so that a flushed fp16 subnormal or a
  misread mid is no longer hidden behind the large terms."""
  w = (rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32)
  if kind == 'window':
    c = np.arange(k) % 6
    w[np.ix_(c <= 1, np.arange(n) >= n // 2)] = 0
    w[np.ix_(c == 2, np.arange(n) >= 3 * n // 4)] = 0
  return w, rng.standard_normal(n).astype(np.float32)


Inputs = collections.namedtuple(
    'Inputs', 'x words slot slot2 gain bias_a inv a64 w bias r bad_rows')


@functools.lru_cache(maxsize=None)
def inputs(name, i):
  """Problem i of case `name`: x fp32 [M, K] (None for 'noncanonical'), the pair words uint32
  [M, K], the slot word(s) with a_gain / a_bias, 1 / scale, the fp64 values the pairs stand for,
  W, bias, R and the rows that hold a non-finite element ('inf' only). Computed once."""
  case = by_name(CASES)[name]
  p = case.problems[i]
  rng = np.random.default_rng(7000 + 16 * case.seed + i)
  x = None
  if case.values == 'noncanonical':
    true_max = np.float32(2.75)
  else:
    x, true_max = _fp32_values(case.values, p.m, p.k, rng)
  slot, slot2, gain, bias_a = hc.slot_words(case, true_max)
  bound = wr.slot_bound([slot], [slot2] if slot2 is not None else None, gain, bias_a)
  s, inv = wr.h2_scale(bound)
  if case.values == 'noncanonical':
    # hi and mid drawn independently: hi over the whole range up to +-(2^15 - 16) with some
    # zeros, subnormals and both extremes; mid = j ulp(hi), j in -2047..2047 (a canonical split
    # has |j| <= 1024 and the sign the residual asks for)
    hi = np.clip(rng.standard_normal((p.m, p.k)) * 9000.0, -HI_MAX, HI_MAX).astype(np.float16)
    pick = rng.uniform(size=hi.shape)
    hi[pick < 0.04] = np.float16(HI_MAX)
    hi[(pick >= 0.04) & (pick < 0.08)] = np.float16(-HI_MAX)
    hi[(pick >= 0.08) & (pick < 0.10)] = np.float16(0)
    hi[(pick >= 0.10) & (pick < 0.12)] = np.float16(3 * 2.0 ** -24)
    ulp = np.spacing(np.abs(hi)).astype(np.float64)
    j = rng.integers(-2047, 2048, hi.shape)
    j[pick > 0.97] = 2047
    j[(pick > 0.94) & (pick <= 0.97)] = -2047
    mid64 = j * ulp
    mid = mid64.astype(np.float16)
    assert (mid.astype(np.float64) == mid64).all() and np.abs(hi).max() == HI_MAX
    words = pairs_from(hi, mid)
  else:
    if case.scale == 'inf':
      x[3, 17 % p.k] = np.inf
      x[5, 5] = np.nan
    words = encode(x, s)
  with np.errstate(invalid='ignore'):
    a64 = wr.h2_values(words, p.k, inv)
  bad = ~np.isfinite(a64).all(axis=1)
  assert bad.any() == (case.scale == 'inf')
  w, bias = weights(case.values, p.k, p.n, rng)
  r = rng.standard_normal((p.m, p.n)).astype(np.float32)
  out = Inputs(x, words, slot, slot2, gain, bias_a, inv, a64, w, bias if p.bias else None,
               r if p.res else None, bad)
  for a in out:
    if isinstance(a, np.ndarray):
      a.setflags(write=False)
  return out


@functools.lru_cache(maxsize=None)
def expected(name, i):
  """(exact, mag) in fp64: exact = A64 W64 (+ bias) (+ R), then ReLU; mag = |A64| |W64| + |bias|
  + |R|. Rows with a non-finite element of A are non-finite."""
  case = by_name(CASES)[name]
  p = case.problems[i]
  inp = inputs(name, i)
  w64 = inp.w.astype(np.float64)
  with np.errstate(invalid='ignore', over='ignore'):
    exact = inp.a64 @ w64
    mag = np.abs(inp.a64) @ np.abs(w64)
  if inp.bias is not None:
    exact = exact + inp.bias.astype(np.float64)
    mag = mag + np.abs(inp.bias).astype(np.float64)
  if inp.r is not None:
    exact = exact + inp.r.astype(np.float64)
    mag = mag + np.abs(inp.r).astype(np.float64)
  if p.relu:
    with np.errstate(invalid='ignore'):
      exact = np.where(np.isnan(exact), exact, np.maximum(exact, 0))
  exact.setflags(write=False)
  mag.setflags(write=False)
  return exact, mag


def a_buffer(case, i, presplit=True):
  """The whole allocation of problem i's A as uint32 [M + A_NAN_ROWS, lda]: pairs (or, presplit
  False, the fp32 values) in [:M, :K], A_POISON_BITS everywhere else."""
  p = case.problems[i]
  inp = inputs(case.name, i)
  buf = np.full((p.m + A_NAN_ROWS, p.lda), A_POISON_BITS, np.uint32)
  buf[:p.m, :p.k] = inp.words if presplit else inp.x.view(np.uint32)
  return buf
