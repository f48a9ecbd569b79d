"""Case tables of the two product kernels behind epos_pointwise_conv_grouped_f32 that are not the
fp16-pair kernel (epos_amd/csrc/pointwise_gemm.hip, pointwise_gemm_split.hip; tests/
test_gpu_gemm_fallback.py), in the style of tests/helpers/h2_presplit_cases.py:
  * pointwise_gemv_f32: one problem with M <= 8 and sub == 1 (the image-pooling 1x1);
  * pointwise_gemm_split_f32 (bf16 x 6): every problem with Ws that the fp16-pair kernel does not
    take (no Wh), in its {single, group} x {residual, none} x {64-row, 128-row tile} forms.
The module holds the cases, a mirror of the routing (grouped_impl, split_eligible) and of each
launcher (the GEMV's slice loops, launch_grouped_split, launch_split_rb and the kernel's
workgroup -> tile map) -- written from the sources, sharing no code with them --, the classifier
of the regimes a case takes, the buffer layout with its guards, the input generators, the fp64
expectation and the restatement of the GEMV's summation order. Pure numpy: tests/
test_gemm_fallback_cases_host.py checks without a GPU that the tables reach every regime the GPU
tests are written for and that no case is dead.

A problem: C[M, N] = act(relu_in(A)[row(m), :K] W[K, N] (+ bias) (+ R)). A has row pitch lda;
every word of its allocation that the kernels must not read -- columns K..lda of every row,
A_NAN_ROWS rows behind the last one and, under sub = 2, the rows of the Hi x Wi map that the
gather skips -- is NaN. C starts c_off floats into a buffer of row pitch ldc with GUARD_BEFORE
sentinel rows in front and guard_after(M) behind; R has NaN in columns N..ldr and in guard rows
around it, the bias vector NaN in front of and behind its N values.

Measured on an MI355X, worst error / bound per assertion family (RECORDED, not asserted: the
starting point of a later tightening):
  GEMV, fp64 accuracy, |got - exact| / ((n + 18) 2^-24 1.01 mag):   0.051 (k4_m1_n1);
        0.034 at K = 36, 0.017 at K = 448, 0.003 at K = 2048; 0.067 in the routing test
  GEMV, restated summation order: bit-equal everywhere, no element flagged in any case
  split, fp64 accuracy, |got - exact| / (H2_MAX_REL_ERR mag), 64-row tiles:
        0.386 (band_64, K = 16); 0.19 .. 0.35 in the other cases
  split, the same with 128-row tiles:   0.541 (big_band_group, K = 16), 0.505, 0.465
  split / fp32-MFMA kernel, worst errors on the same inputs (bar: 1.5):
        0.35 (k128_res), 0.38 (k728_long), 0.81 (band_64)
  M = 9 split rows against the M = 8 GEMV rows, |difference| / (sum of the two bounds): 0.061
  exact-integer inputs: bit-equal to the integer product in every case of both tables
"""
import collections
import functools

import numpy as np

from helpers import heads_cases as hc

GUARD_BEFORE = hc.GUARD_BEFORE
A_NAN_ROWS = hc.A_NAN_ROWS
SENTINEL_BITS = hc.SENTINEL_BITS
H2_MAX_REL_ERR = hc.H2_MAX_REL_ERR      # the project's bar for a GEMM against fp64, per sum |a||w|

GEMV_SLICES, GEMV_UNROLL, GEMV_MAX_M = 16, 8, 8
SP_BN, SP_BK, SP_NST = 128, 16, 4       # columns per tile, K per step, stages of the ring
SP_BIG_TILES = 200                      # 128-row tiles from this many 128 x 128 tiles on
MAX_GROUP = 8
FLAG_CAP = 0.01                         # GEMV restatement: flagged elements per case


def _cdiv(a, b):
  return -(-a // b)


_Problem = collections.namedtuple(
    '_Problem', 'm n k lda ldc c_off bias res ldr relu relu_in c_amax sub b hi wi')


def P(m, n, k, lda_pad=0, c_off=0, pad=0, bias=True, res=False, ldr_pad=4, relu=0, relu_in=0,
      c_amax=False, sub2=None):
  """lda = K + lda_pad; ldc = c_off + N + pad; res: a residual with ldr = N + ldr_pad; sub2 =
  (B, Hi, Wi): A is a B x Hi x Wi map of which every second row and column is taken (m must be
  B * ceil(Hi / 2) * ceil(Wi / 2))."""
  assert k % 4 == 0 and lda_pad % 4 == 0
  b, hi, wi = sub2 if sub2 else (0, 0, 0)
  if sub2:
    assert m == b * ((hi + 1) // 2) * ((wi + 1) // 2)
  return _Problem(m, n, k, k + lda_pad, c_off + n + pad, c_off, bool(bias), bool(res),
                  n + ldr_pad if res else 0, relu, relu_in, bool(c_amax), 2 if sub2 else 1,
                  b, hi, wi)


def out_hw(p):
  return (p.hi + 1) // 2, (p.wi + 1) // 2


def a_rows(p):
  """Rows of A's live part: the whole input map under sub = 2."""
  return p.b * p.hi * p.wi if p.sub > 1 else p.m


def gather_rows(p):
  """Row of A that output row m reads."""
  if p.sub == 1:
    return np.arange(p.m)
  ho, wo = out_hw(p)
  b, yo, xo = np.meshgrid(np.arange(p.b), np.arange(ho), np.arange(wo), indexing='ij')
  return ((b * p.hi + yo * 2) * p.wi + xo * 2).reshape(-1)


VALUES = ('signed', 'relu_like', 'integers', 'negative', 'nan_row')
_Case = collections.namedtuple('_Case', 'name kernel problems values shared extra expect seed')


def Case(name, kernel, problems, expect, values='signed', shared=False, extra=False):
  """shared: the problems write column slices of ONE buffer (ldc = the sum of the N's, each
  problem at its own c_off) and publish into ONE c_amax slot. extra (GEMV): the call also brings
  Wh, Ws and an a_amax slot, which the GEMV must ignore."""
  problems = tuple(problems)
  assert kernel in ('gemv', 'split') and values in VALUES and 1 <= len(problems) <= MAX_GROUP
  if shared:
    width, col, out = sum(p.n for p in problems), 0, []
    for p in problems:
      assert p.c_off == 0 and p.ldc == p.n
      out.append(p._replace(ldc=width, c_off=col))
      col += p.n
    problems = tuple(out)
  return _Case(name, kernel, problems, values, shared, bool(extra), tuple(expect), 0)


def by_name(table):
  d = {c.name: c for c in table}
  assert len(d) == len(table), 'duplicate case names'
  return d


# ---------------------------------------------------------------------- routing mirror ---
def route(problems, has, ref_build=False):
  """grouped_impl of pointwise_gemm.hip for problems whose weights / slots `has` names: a set out
  of {'Ws', 'Wh', 'a_amax', 'a_presplit'} (the same for every problem). Returns 'gemv', 'h2',
  'split', 'fp32_mfma' (the test build only) or 'refused'."""
  for p in problems:
    if 'a_presplit' in has and not ('Wh' in has and 'a_amax' in has and p.relu_in == 0 and
                                    p.m > GEMV_MAX_M and p.sub == 1):
      return 'refused'
    if p.c_amax and not (p.relu_in == 0 and p.m > GEMV_MAX_M and vec(p)):
      return 'refused'
    if (p.relu_in != 0) != (problems[0].relu_in != 0) or p.res != problems[0].res:
      return 'refused'
  if len(problems) == 1 and problems[0].m <= GEMV_MAX_M and problems[0].sub == 1:
    return 'gemv'
  plain = all(p.relu_in == 0 and p.m > GEMV_MAX_M for p in problems)
  if plain and 'Wh' in has:
    return 'h2'
  if plain and 'Ws' in has:
    return 'split'
  return 'fp32_mfma' if ref_build else 'refused'


# (name, problems, has, expected route on the product library): the table of the routing test
_R8 = P(8, 40, 36)
ROUTES = (
    ('m8_wp', (_R8,), (), 'gemv'),
    ('m8_wp_ws', (_R8,), ('Ws',), 'gemv'),
    ('m8_wp_wh_bound', (_R8,), ('Wh', 'a_amax'), 'gemv'),
    ('m8_relu_in', (_R8._replace(relu_in=1),), ('Ws',), 'gemv'),
    ('m9_relu_in', (_R8._replace(m=9, relu_in=1),), ('Ws',), 'refused'),
    ('m8_c_amax', (_R8._replace(c_amax=True),), ('Ws',), 'refused'),
    ('m8_in_group', (_R8, _R8), ('Ws',), 'refused'),
    ('m8_sub2', (P(8, 40, 36, sub2=(1, 3, 7)),), ('Ws',), 'refused'),
    ('m9_ws', (_R8._replace(m=9),), ('Ws',), 'split'),
    ('m9_wp_only', (_R8._replace(m=9),), (), 'refused'),
    ('presplit_without_wh', (_R8._replace(m=9),), ('Ws', 'a_amax', 'a_presplit'), 'refused'),
)
SMALL_M_REFUSALS = ('m8_in_group', 'm8_sub2')       # epos_last_error() names M <= 8


# ------------------------------------------------------------------------ GEMV mirror ---
def gemv_slice_iters(k, s):
  """(main iterations, remainder iterations) of K-slice s: quads s, s + 16, ... of K / 4, eight
  per main iteration."""
  kq, q, main, rem = k // 4, s, 0, 0
  while q + (GEMV_UNROLL - 1) * GEMV_SLICES < kq:
    q += GEMV_UNROLL * GEMV_SLICES
    main += 1
  while q < kq:
    q += GEMV_SLICES
    rem += 1
  return main, rem


def gemv_grid(p):
  """(blocks of 64 columns, rows): the column blocks cover N rounded up to 128."""
  return _cdiv(p.n, 128) * 2, p.m


def gemv_chain(k):
  """Longest fused multiply-add chain of a slice."""
  return 4 * _cdiv(k, 64)


def gemv_regimes(case):
  p, = case.problems
  s = set()
  iters = [gemv_slice_iters(p.k, i) for i in range(GEMV_SLICES)]
  for main, rem in iters:
    s.add('main_%s' % (main if main < 2 else 'ge2'))
    if main + rem:
      s.add('rem_%d' % rem if rem in (0, 1, 7) else 'rem_other')
  if len({m > 0 for m, _ in iters}) == 2:
    s.add('slices_disagree_on_main')
  if p.k == 4:
    s.add('k_4')
  if 8 <= p.k <= 60:
    s.add('k_idle_slices')
  if p.k == 2048:
    s.add('k_2048')
  if p.k % 512 == 4 and p.k > 512:
    s.add('k_past_main_multiple')
  if p.m in (1, 2, 8):
    s.add('m_%d' % p.m)
  if p.n == 1:
    s.add('n_1')
  elif p.n < 64:
    s.add('n_lt_64')
  elif p.n in (64, 128):
    s.add('n_%d' % p.n)
  elif p.n < 128:
    s.add('n_65_127')
  elif p.n % 64:
    s.add('n_3_blocks_ragged')
  else:
    s.add('n_full_blocks')
  s.add('bias' if p.bias else 'no_bias')
  s.add('res_ldr_gt_n' if p.res and p.ldr > p.n else 'no_res')
  s.add('relu' if p.relu else 'no_relu')
  s.add('relu_in' if p.relu_in else 'no_relu_in')
  s.add('lda_gt_k' if p.lda > p.k else 'lda_eq_k')
  if p.ldc > p.n and p.c_off % 4:
    s.add('ldc_gt_n_unaligned')
  if case.extra:
    s.add('extra_weights_ignored')
  s.add('values_' + case.values)
  return s


GEMV_REQUIRED = tuple(
    ['main_0', 'main_1', 'main_ge2', 'rem_0', 'rem_1', 'rem_7', 'slices_disagree_on_main',
     'k_4', 'k_idle_slices', 'k_2048', 'k_past_main_multiple', 'm_1', 'm_2', 'm_8',
     'n_1', 'n_lt_64', 'n_64', 'n_65_127', 'n_128', 'n_3_blocks_ragged',
     'bias', 'no_bias', 'res_ldr_gt_n', 'no_res', 'relu', 'no_relu', 'relu_in', 'no_relu_in',
     'lda_gt_k', 'lda_eq_k', 'ldc_gt_n_unaligned', 'extra_weights_ignored'] +
    ['values_' + v for v in VALUES])
GEMV_OPTIONAL = ('rem_other', 'n_full_blocks')

GEMV_CASES = (
    Case('k4_m1_n1', 'gemv', [P(1, 1, 4)],
         ['k_4', 'm_1', 'n_1', 'main_0', 'rem_1', 'bias', 'no_res', 'no_relu', 'no_relu_in',
          'lda_eq_k', 'values_signed']),
    Case('k36_m2_n40', 'gemv', [P(2, 40, 36, lda_pad=28, res=True, relu=1)],
         ['k_idle_slices', 'm_2', 'n_lt_64', 'lda_gt_k', 'res_ldr_gt_n', 'relu'],
         values='relu_like'),
    Case('k448_m8_n64', 'gemv', [P(8, 64, 448, bias=False, relu_in=1)],
         ['rem_7', 'm_8', 'n_64', 'no_bias', 'relu_in']),
    Case('k480_m3_n100', 'gemv', [P(3, 100, 480, c_off=3, pad=2, lda_pad=4)],
         ['main_1', 'rem_0', 'rem_7', 'slices_disagree_on_main', 'n_65_127',
          'ldc_gt_n_unaligned']),
    Case('k2048_m2_n256', 'gemv', [P(2, 256, 2048, relu=1)], ['k_2048', 'main_ge2', 'rem_0'],
         values='relu_like'),
    Case('k2052_m2_n130', 'gemv', [P(2, 130, 2052, res=True, relu_in=1, c_off=1, pad=3)],
         ['k_past_main_multiple', 'rem_1', 'n_3_blocks_ragged', 'main_ge2']),
    Case('k64_m8_n128_int', 'gemv', [P(8, 128, 64, res=True, lda_pad=8)],
         ['n_128', 'values_integers', 'rem_1'], values='integers'),
    Case('k516_m2_n70_int', 'gemv', [P(2, 70, 516, relu=1, relu_in=1, c_off=2, pad=1)],
         ['main_1', 'values_integers', 'extra_weights_ignored'], values='integers', extra=True),
    Case('negative_relu_in', 'gemv', [P(4, 70, 132, res=True, relu_in=1)],
         ['values_negative', 'relu_in'], values='negative'),
    Case('nan_row', 'gemv', [P(4, 70, 132)], ['values_nan_row'], values='nan_row'),
)
GEMV_CASES = tuple(c._replace(seed=i) for i, c in enumerate(GEMV_CASES))


# ----------------------------------------------------------------------- split mirror ---
def split_eligible(problems):
  return all(p.relu_in == 0 and p.m > GEMV_MAX_M for p in problems)


def split_launch(problems):
  """launch_grouped_split / launch_split_rb: (rows per tile, workgroups, per problem (row tiles,
  column tiles), instantiation name)."""
  tiles128 = sum(_cdiv(p.m, 128) * _cdiv(p.n, SP_BN) for p in problems)
  rows = 128 if tiles128 >= SP_BIG_TILES else 64
  t = [(_cdiv(p.m, rows), _cdiv(p.n, SP_BN)) for p in problems]
  inst = '%s_%s_%d' % ('single' if len(problems) == 1 else 'group',
                       'res' if problems[0].res else 'plain', rows)
  return rows, sum(a * b for a, b in t), t, inst


def xcd_remap(raw, total):
  """blockIdx.x -> position in the tile list: the workgroups of one XCD (blockIdx % 8) take a
  contiguous range."""
  x, idx = raw & 7, raw >> 3
  q, r = total >> 3, total & 7
  return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + idx


def split_tile(bid, tm, tn):
  """(row tile, column tile) of position bid inside a problem of tm x tn tiles: column fastest,
  in bands of 8 column tiles from 9 column tiles on."""
  if tn <= 8:
    return bid // tn, bid % tn
  per_band = tm * 8
  band = bid // per_band
  rem = bid - band * per_band
  bw = min(tn - band * 8, 8)
  return rem // bw, band * 8 + rem % bw


def vec(p):
  """The float4 epilogue: rows of C (and R) 16-byte aligned, N a multiple of 4. The C buffers
  are 512-byte aligned and GUARD_BEFORE = 4 rows precede the matrix."""
  return p.ldc % 4 == 0 and p.n % 4 == 0 and p.c_off % 4 == 0 and (not p.res or p.ldr % 4 == 0)


def split_regimes(case):
  s = set()
  rows, wgs, t, inst = split_launch(case.problems)
  s.add(inst)
  if wgs < 8:
    s.add('wgs_lt_8')
  elif wgs % 8:
    s.add('wgs_not_multiple_of_8')
  if len(case.problems) == 8:
    s.add('group_8')
  if len(case.problems) > 1 and all(len({getattr(p, f) for p in case.problems}) > 1
                                    for f in ('m', 'n', 'k')):
    s.add('group_mixed_m_n_k')
  for p, (tm, tn) in zip(case.problems, t):
    nks = _cdiv(p.k, SP_BK)
    if nks <= 10 or nks == 46:
      s.add('nks_%d' % nks)
    s.add('krem_%d' % (p.k % SP_BK))
    s.add('lda_eq_k' if p.lda == p.k else 'lda_padded')
    if p.m in (9, 63, 64, 65, 127, 128, 129):
      s.add('m_%d' % p.m)
    if tm >= 3:
      s.add('m_3_row_tiles')
    s.add('nq%d' % (((p.n - 1) % SP_BN) // 32 + 1))
    if rows == 128:                # the last column tile's fourth block: skipped when dead
      s.add('live3_128' if (tn - 1) * SP_BN + 96 >= p.n else 'live4_128')
    if tn > 8 and tn % 8 and tm >= 2:
      s.add('band_%d' % rows)
    if vec(p):
      s.add('vec')
    elif p.n % 4:
      s.add('scalar_by_n')
    elif p.ldc % 4 or p.c_off % 4:
      s.add('scalar_by_alignment')
    else:
      s.add('scalar_by_ldr')
    if p.c_off == 0:
      s.add('c_off_0')
    else:
      s.add('c_off_aligned' if p.c_off % 4 == 0 and p.ldc % 4 == 0 else 'c_off_unaligned')
    s.add('bias' if p.bias else 'no_bias')
    s.add('relu' if p.relu else 'no_relu')
    if p.res and p.ldr > p.n:
      s.add('res_ldr_gt_n')
    if p.c_amax:
      s.add('c_amax_cat' if case.shared and len(case.problems) > 1 else 'c_amax')
    if p.sub > 1:
      s.add('sub2_single' if len(case.problems) == 1 else 'sub2_group')
      if p.hi % 2 and p.wi % 2:
        s.add('sub2_odd_map')
  s.add('values_' + case.values)
  return s


SPLIT_VALUES = ('signed', 'relu_like', 'integers')
SPLIT_REQUIRED = tuple(
    ['%s_%s_%d' % (a, b, c) for a in ('single', 'group') for b in ('plain', 'res')
     for c in (64, 128)] +
    ['nks_%d' % i for i in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 46)] +
    ['krem_%d' % r for r in (0, 4, 8, 12)] +
    ['lda_eq_k', 'lda_padded'] +
    ['m_%d' % m for m in (9, 63, 64, 65, 127, 128, 129)] + ['m_3_row_tiles'] +
    ['nq%d' % q for q in (1, 2, 3, 4)] + ['live3_128', 'live4_128', 'band_64', 'band_128'] +
    ['vec', 'scalar_by_n', 'scalar_by_alignment', 'scalar_by_ldr'] +
    ['c_off_0', 'c_off_aligned', 'c_off_unaligned', 'bias', 'no_bias', 'relu', 'no_relu',
     'res_ldr_gt_n', 'c_amax', 'c_amax_cat'] +
    ['sub2_single', 'sub2_group', 'sub2_odd_map'] +
    ['group_8', 'group_mixed_m_n_k', 'wgs_lt_8', 'wgs_not_multiple_of_8'] +
    ['values_' + v for v in SPLIT_VALUES])
SPLIT_OPTIONAL = ()

_THIN = 25600                      # 200 row tiles of 128: the smallest single-column-tile launch
SPLIT_CASES = (
    # ---- K steps 1..10, M edges, N quarters: 64-row tiles
    Case('k16_m9', 'split', [P(9, 200, 16)],
         ['single_plain_64', 'nks_1', 'krem_0', 'm_9', 'nq3', 'vec', 'lda_eq_k', 'c_off_0', 'bias',
          'no_relu', 'wgs_lt_8', 'values_signed']),
    Case('k32_m63_res', 'split', [P(63, 100, 32, res=True, relu=1)],
         ['single_res_64', 'nks_2', 'm_63', 'nq4', 'res_ldr_gt_n', 'relu']),
    Case('k48_m64', 'split', [P(64, 32, 48, bias=False)], ['nks_3', 'm_64', 'nq1', 'no_bias'],
         values='relu_like'),
    Case('k64_m65_padded', 'split', [P(65, 64, 64, lda_pad=32)],
         ['nks_4', 'm_65', 'nq2', 'lda_padded']),
    Case('k80_m127', 'split', [P(127, 136, 80, c_off=4, pad=4)],
         ['nks_5', 'm_127', 'c_off_aligned', 'vec']),
    Case('k96_m128_unaligned', 'split', [P(128, 136, 96, c_off=3, pad=1)],
         ['nks_6', 'm_128', 'c_off_unaligned', 'scalar_by_alignment']),
    Case('k112_m129', 'split', [P(129, 180, 112, lda_pad=16, relu=1)], ['nks_7', 'm_129'],
         values='relu_like'),
    Case('k128_res', 'split', [P(137, 256, 128, res=True)], ['nks_8']),
    Case('k144_padded', 'split', [P(70, 72, 144, lda_pad=16)], ['nks_9']),
    Case('k160', 'split', [P(70, 72, 160, bias=False, relu=1)], ['nks_10']),
    # ---- partial last K step, the scalar epilogues, three row tiles, the long ring
    Case('k20_n22_m200', 'split', [P(200, 22, 20, lda_pad=12)],
         ['krem_4', 'm_3_row_tiles', 'scalar_by_n']),
    Case('k40_res_ldr', 'split', [P(70, 36, 40, lda_pad=24, res=True, ldr_pad=5)],
         ['krem_8', 'scalar_by_ldr']),
    Case('k92_int', 'split', [P(137, 100, 92, lda_pad=4, res=True, relu=1)],
         ['krem_12', 'values_integers'], values='integers'),
    Case('k728_long', 'split', [P(130, 136, 728, lda_pad=8, relu=1)], ['nks_46', 'krem_8'],
         values='relu_like'),
    # ---- more than eight column tiles: the band order, last band narrower than 8
    Case('band_64', 'split', [P(129, 1100, 16)], ['band_64', 'wgs_not_multiple_of_8']),
    # ---- output absmax, groups, the stride-2 gather
    Case('c_amax_single', 'split', [P(137, 200, 48, relu=1, c_amax=True)], ['c_amax']),
    Case('group_8', 'split',
         [P(9, 40, 16), P(70, 22, 20, lda_pad=4), P(64, 128, 32), P(9, 4, 4), P(65, 136, 48),
          P(30, 64, 36, bias=False, relu=1), P(129, 32, 16), P(10, 129, 64, c_off=1, pad=2)],
         ['group_plain_64', 'group_8', 'group_mixed_m_n_k']),
    Case('group_res_mixed', 'split',
         [P(137, 136, 80, res=True, relu=1), P(70, 36, 40, res=True, ldr_pad=5),
          P(9, 22, 20, res=True)], ['group_res_64', 'group_mixed_m_n_k'], values='integers'),
    Case('group_cat_amax', 'split',
         [P(137, 72, 48, c_amax=True, relu=1), P(137, 136, 80, c_amax=True),
          P(137, 64, 112, lda_pad=16, c_amax=True, relu=1)], ['c_amax_cat'], shared=True),
    Case('sub2_single_odd', 'split', [P(40, 136, 72, lda_pad=8, sub2=(2, 7, 9))],
         ['sub2_single', 'sub2_odd_map']),
    Case('sub2_group', 'split',
         [P(126, 136, 72, sub2=(2, 13, 18)), P(126, 22, 40, sub2=(2, 13, 18)),
          P(40, 260, 20, res=False, sub2=(2, 7, 9))], ['sub2_group'], values='relu_like'),
    # ---- 128-row tiles: from 200 tiles of 128 x 128 on
    Case('big_thin', 'split', [P(_THIN, 128, 16)], ['single_plain_128', 'live4_128']),
    Case('big_thin_res_live3', 'split', [P(_THIN - 3, 96, 16, res=True, relu=1)],
         ['single_res_128', 'live3_128'], values='relu_like'),
    Case('big_band_group', 'split', [P(2900, 1100, 16), P(9, 40, 36, lda_pad=4)],
         ['group_plain_128', 'band_128']),
    Case('big_group_res_int', 'split',
         [P(_THIN // 2, 100, 16, res=True), P(_THIN // 2, 128, 20, res=True, relu=1)],
         ['group_res_128'], values='integers'),
)
SPLIT_CASES = tuple(c._replace(seed=100 + i) for i, c in enumerate(SPLIT_CASES))

ALL_CASES = GEMV_CASES + SPLIT_CASES


def regime_names(case):
  return gemv_regimes(case) if case.kernel == 'gemv' else split_regimes(case)


REQUIRED_REGIMES = {'gemv': GEMV_REQUIRED, 'split': SPLIT_REQUIRED}
OPTIONAL_REGIMES = {'gemv': GEMV_OPTIONAL, 'split': SPLIT_OPTIONAL}

# launch context: (X, Y) of the launch-history tests (Y another instantiation / another kernel),
# the cases run on a non-default stream and in a captured graph
HISTORY_PAIRS = (('k480_m3_n100', 'k40_res_ldr'), ('k112_m129', 'group_res_mixed'))
STREAM_CASES = ('k2052_m2_n130', 'group_8')
GRAPH_CASES = ('k448_m8_n64', 'k144_padded')
ROW_ALONE_CASE = 'k448_m8_n64'     # row m of an M = 8 call against the same row as M = 1


# ------------------------------------------------------------------------------ layout ---
def guard_after(m):
  """Sentinel rows behind the matrix: the dead rows of a last 128-row tile and two more."""
  return _cdiv(m, 128) * 128 - m + 2


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


BIAS_GUARD = 4                     # NaN floats in front of the bias values (keeps 16 bytes)
R_GUARD_ROWS = 4                   # NaN rows in front of and behind R


def bias_buffer(p, bias):
  """[4 NaN | N values | NaN up to the next multiple of 128 and 4 more]."""
  b = np.full(BIAS_GUARD + _cdiv(p.n, 128) * 128 + 4, np.nan, np.float32)
  b[BIAS_GUARD:BIAS_GUARD + p.n] = bias
  return b


def r_buffer(p, r):
  """[R_GUARD_ROWS + M + R_GUARD_ROWS, ldr], NaN outside [M) x [N)."""
  buf = np.full((2 * R_GUARD_ROWS + p.m, p.ldr), np.nan, np.float32)
  buf[R_GUARD_ROWS:R_GUARD_ROWS + p.m, :p.n] = r
  return buf


# ------------------------------------------------------------------------------ values ---
def _int_amax(p):
  """Largest |a| of the exact-integer kind: with |w| <= 7, |bias|, |R| <= 2^15 every partial sum
  of a C element stays below 2^24 whatever the order."""
  return int(min(2 ** 20, (2 ** 24 - 2 ** 17) // (7 * p.k)))


Inputs = collections.namedtuple('Inputs', 'a w bias r')


def make_inputs(p, values, seed):
  """a fp32 [M, K] (the gathered rows, in output order), W [K, N], bias [N] or None, R [M, N] or
  None of problem p, read-only."""
  rng = np.random.default_rng(seed)
  if values == 'integers':
    top = _int_amax(p)
    a = rng.integers(-top, top + 1, (p.m, p.k)).astype(np.float32)
    a[0, 0], a[p.m - 1, p.k - 1] = top, -top
    w = rng.integers(-7, 8, (p.k, p.n)).astype(np.float32)
    bias = rng.integers(-2 ** 15, 2 ** 15 + 1, p.n).astype(np.float32)
    r = rng.integers(-2 ** 15, 2 ** 15 + 1, (p.m, p.n)).astype(np.float32)
  else:
    a = rng.standard_normal((p.m, p.k)).astype(np.float32)
    if values == 'relu_like':
      a = np.maximum(a, 0)
    elif values == 'negative':
      a = -np.abs(a) - np.float32(2.0 ** -20)
    elif values == 'nan_row':
      a[1, 5 % p.k], a[1, p.k - 3] = np.nan, np.inf
    w = (rng.standard_normal((p.k, p.n)) / np.sqrt(p.k)).astype(np.float32)
    bias = rng.standard_normal(p.n).astype(np.float32)
    r = rng.standard_normal((p.m, p.n)).astype(np.float32)
  out = Inputs(a, w, bias if p.bias else None, r if p.res else None)
  for x in out:
    if x is not None:
      x.setflags(write=False)
  return out


@functools.lru_cache(maxsize=None)
def inputs(name, i):
  """Problem i of case `name`, computed once."""
  case = by_name(ALL_CASES)[name]
  return make_inputs(case.problems[i], case.values, 9000 + 16 * case.seed + i)


def a_buffer(p, inp):
  """The whole allocation of a problem's A, fp32 [rows + A_NAN_ROWS, lda]: the values in the rows
  the problem reads, columns [:K]; NaN everywhere else (the rows a stride-2 gather skips
  included)."""
  buf = np.full((a_rows(p) + A_NAN_ROWS, p.lda), np.nan, np.float32)
  buf[gather_rows(p), :p.k] = inp.a
  return buf


def _act_in(p, a):
  with np.errstate(invalid='ignore'):
    return np.where(np.isnan(a), a, np.maximum(a, 0)) if p.relu_in else a


def expectation(p, inp):
  """(exact, mag) in fp64: exact = relu_in(A) W (+ bias) (+ R), then ReLU; mag = |relu_in(A)| |W|
  + |bias| + |R|. Rows with a non-finite element of A are non-finite."""
  a64 = _act_in(p, inp.a).astype(np.float64)
  w64 = inp.w.astype(np.float64)
  with np.errstate(invalid='ignore', over='ignore'):
    exact = a64 @ w64
    mag = np.abs(a64) @ np.abs(w64)
  for x in (inp.bias, inp.r):
    if x is not None:
      exact = exact + x.astype(np.float64)
      mag = mag + np.abs(x).astype(np.float64)
  if p.relu:
    with np.errstate(invalid='ignore'):
      exact = np.where(np.isnan(exact), exact, np.maximum(exact, 0))
  exact.setflags(write=False)
  mag.setflags(write=False)
  return exact, mag


@functools.lru_cache(maxsize=None)
def expected(name, i):
  """expectation() of problem i of case `name`, computed once."""
  return expectation(by_name(ALL_CASES)[name].problems[i], inputs(name, i))


def gemv_bound(p, mag):
  """Slice chains of at most n = 4 ceil(K / 64) fused multiply-adds, then 15 additions of
  partials, the bias and the residual, each within 2^-24 relative of a partial result that mag
  bounds (1.01: the second-order terms)."""
  return (gemv_chain(p.k) + 18) * 2.0 ** -24 * 1.01 * mag


def integer_partial_sum_bound(name, i):
  """max over the elements of sum |a||w| + |bias| + |R|: every partial sum in any order."""
  return float(expected(name, i)[1].max())


# --------------------------------------------------- the GEMV's summation order, restated ---
def _rounded_add(x64, acc32):
  """fp32(x64 + acc32) through one fp64 addition, and where that may differ from the single
  rounding the hardware does: the fp64 sum is itself rounded AND lands exactly half way between
  two fp32 numbers."""
  c = acc32.astype(np.float64)
  with np.errstate(invalid='ignore', over='ignore'):
    s = x64 + c
    bb = s - x64
    err = (x64 - (s - bb)) + (c - bb)              # two-sum: x64 + c == s + err exactly
    f = s.astype(np.float32)
    d = s - f.astype(np.float64)
    other = f.astype(np.float64) + 2.0 * d         # the fp32 neighbour s would be half way to
    half_way = (d != 0) & (other.astype(np.float32).astype(np.float64) == other)
  return f, half_way & (err != 0)


@functools.lru_cache(maxsize=None)
def gemv_restated(name):
  """gemv_restate() of a GEMV case, computed once."""
  case = by_name(GEMV_CASES)[name]
  return gemv_restate(case.problems[0], inputs(name, 0))


def gemv_restate(p, inp):
  """(value fp32 [M, N], flagged bool [M, N]) of a GEMV problem in the kernel's own order: per
  slice s one chain of fmas over quads s, s + 16, ... (the main and the remainder loop walk the
  same sequence), the 16 partials added in index order, then bias, R and ReLU. An fp32 fma is
  the exact product (fp64 holds it) plus the accumulator, rounded once; an element is flagged
  when any of its sums is one where the two roundings taken here may not be that one."""
  a64 = _act_in(p, inp.a).astype(np.float64)
  w64 = inp.w.astype(np.float64)
  kq = p.k // 4
  acc = np.zeros((p.m, GEMV_SLICES, p.n), np.float32)
  flag = np.zeros(acc.shape, bool)
  for j in range(_cdiv(kq, GEMV_SLICES)):
    quads = np.arange(GEMV_SLICES) + GEMV_SLICES * j
    live = (quads < kq)[None, :, None]
    for e in range(4):
      ks = np.minimum(quads * 4 + e, p.k - 1)
      with np.errstate(invalid='ignore', over='ignore'):
        prod = a64[:, ks][:, :, None] * w64[ks][None, :, :]
      new, fl = _rounded_add(prod, acc)
      acc = np.where(live, new, acc)
      flag |= fl & live
  v, fv = acc[:, 0], flag[:, 0]
  for s in range(1, GEMV_SLICES):
    v, fl = _rounded_add(acc[:, s].astype(np.float64), v)
    fv = fv | fl | flag[:, s]
  for x in (inp.bias, inp.r):
    if x is not None:
      v, fl = _rounded_add(np.broadcast_to(x, v.shape).astype(np.float64), v)
      fv = fv | fl
  if p.relu:
    v = np.where(v > 0, v, np.float32(0)).astype(np.float32)     # fmaxf(v, 0): NaN -> 0
  v.setflags(write=False)
  fv.setflags(write=False)
  return v, fv
