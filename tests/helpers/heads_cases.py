"""Case table of the dense-heads kernel (heads_gemm_h2_f32, epos_amd/csrc/heads_gemm_h2.hip;
tests/test_gpu_heads_regimes.py) and host-side mirrors of what its launcher and the kernel
branch on, in the style of tests/helpers/glue_cases.py: choose_range, the blockIdx -> (panel,
tile range) map, hd_tile, the store-path predicate and the scale rule of h2_scale.h. Pure
Python: tests/test_heads_cases_host.py holds the mirrors to epos_heads_gemm_plan and checks
without a GPU that the table reaches every regime the GPU tests are written for.

A case: M rows of one A [M, K = 256] with row pitch lda, starting a_off floats into its
allocation; heads = ((N, bias?), ...); pads[i] = free floats behind head i's N columns (ldc =
N + pad, or, with shared, the gap behind the head's column slice of ONE buffer whose width is
every head's ldc); c_off = floats by which every C is moved off its 16-byte aligned place;
bias_off = the same for the bias vectors; scale = how the absmax slot is filled (SCALES).
Allocations come 512-byte aligned from the caching allocator.
"""
import collections
import ctypes

import numpy as np

K = 256
BM, BN = 128, 64
CUS = 256                          # MI355X; the values in the comments below are for it
GUARD_BEFORE = 4                   # sentinel rows in front of a C matrix (4 rows: 16 B aligned)
A_NAN_ROWS = 128                   # NaN rows of A behind row M - 1
H2_MAX_REL_ERR = 4e-7              # fp16-pair GEMM against fp64, relative to sum |a||w| (+|bias|):
                                   # the bar of test_pointwise_gemm_h2_accuracy (test_gpu_h2.py)
SENTINEL_BITS = 0x7fc12345         # a NaN no arithmetic produces

SCALES = (None, 'pow2', 'pow2_below', 'stale', 'amax2', 'gain', 'inf')


def _cdiv(a, b):
  return -(-a // b)


_Case = collections.namedtuple(
    '_Case', 'name m heads expect lda pads shared c_off c_stream a_off bias_off scale seed')


def Case(name, m, heads, expect=(), lda=K, pads=None, shared=False, c_off=0, c_stream=1,
         a_off=0, bias_off=0, scale=None, seed=0):
  heads = tuple((h, True) if isinstance(h, int) else tuple(h) for h in heads)
  pads = tuple(pads) if pads is not None else (0,) * len(heads)
  assert len(pads) == len(heads) and scale in SCALES
  return _Case(name, m, heads, tuple(expect), lda, pads, shared, c_off, c_stream, a_off,
               bias_off, scale, seed)


def by_name(table):
  d = {c.name: c for c in table}
  assert len(d) == len(table), 'duplicate case names'
  return d


# --------------------------------------------------------------------- launcher mirrors ---
def choose_range(nt, panels, cus=CUS):
  """choose_range of heads_gemm_h2.hip: tiles per work item."""
  slots = cus * 2 // 8 if cus > 8 else 1
  pmax = (panels + 7) // 8
  best, best_cost = min(nt, 4), -1
  for r in range(4, 33):
    rr = min(r, nt)
    nr = _cdiv(nt, rr)
    cost = _cdiv(pmax * nr, slots) * (rr + 1)
    if best_cost < 0 or cost < best_cost:
      best_cost, best = cost, rr
    if rr == nt:
      break
  return best


def xcd_panels(panels):
  return [((x + 1) * panels >> 3) - (x * panels >> 3) for x in range(8)]


def plan_of(ns, m, cus=CUS):
  """{nt, panels, range, nr, grid blocks} as launch_heads_h2 computes them."""
  nt = sum(_cdiv(n, BN) for n in ns)
  panels = _cdiv(m, BM)
  rng = choose_range(nt, panels, cus)
  nr = _cdiv(nt, rng)
  return (nt, panels, rng, nr, 8 * max(px * nr for px in xcd_panels(panels)))


def block_item(b, nt, panels, rng, nr):
  """The kernel's work item of workgroup b: (panel, t0, t1), or None (the workgroup returns)."""
  x, k = b & 7, b >> 3
  p_lo, p_hi = (x * panels) >> 3, ((x + 1) * panels) >> 3
  px = p_hi - p_lo
  if k >= px * nr:
    return None
  r = k // px
  t0 = r * rng
  return (p_lo + (k - r * px), t0, min(t0 + rng, nt))


def tile0(ns):
  t, out = 0, []
  for n in ns:
    out.append(t)
    t += _cdiv(n, BN)
  return out + [t]


def hd_tile(ns, t):
  """hd_tile: (problem, local tile, odd 4 KB half of the 128-column stage image?)."""
  t0 = tile0(ns)
  pi = 0
  for i in range(1, len(ns)):
    if t >= t0[i]:
      pi = i
  tl = t - t0[pi]
  return pi, tl, tl & 1


def vec(n, ldc, c_off):
  """The kernel's float4 store path; c_off = C's offset in floats from a 16-byte aligned
  address."""
  return ldc % 4 == 0 and n % 4 == 0 and (4 * c_off) % 16 == 0


# ------------------------------------------------------------------------ scale mirror ---
def _bits(x):
  return int(np.float32(x).view(np.uint32))


def h2_scale_exp(words, gain=0.0, bias=0.0):
  """h2_scale_finish of h2_scale.h: log2 of the scale s for a slot whose words (bit patterns,
  both slots together) are `words`."""
  bound = np.uint32(max(words)).view(np.float32)
  if gain != 0.0:
    bound = np.float32(np.float32(gain) * bound) + np.float32(bias)
  e = _bits(bound) >> 23
  sb = min(268 - e, 253)
  if e >= 255:
    sb = 127
  return sb - 127


def slot_words(case, true_max):
  """(slot word, slot2 word or None, a_gain, a_bias) of a case whose max |A| is true_max; None
  for the slot word: measured on the device (epos_absmax_f32)."""
  t = np.float32(true_max)
  if case.scale is None:
    return None, None, 0.0, 0.0
  if case.scale in ('pow2', 'pow2_below'):
    p = np.float32(2.0 ** np.ceil(np.log2(float(t)) + 1e-9))    # the power of two above
    b = p if case.scale == 'pow2' else np.nextafter(p, np.float32(0))
    assert t <= b
    return _bits(b), None, 0.0, 0.0
  if case.scale == 'stale':
    return _bits(t * np.float32(1024)), None, 0.0, 0.0
  if case.scale == 'amax2':                      # the first slot alone would overflow fp16
    return _bits(t * np.float32(0.25)), _bits(t), 0.0, 0.0
  if case.scale == 'gain':
    return _bits(t), None, 2.0, 1.0
  return 0x7f800000, None, 0.0, 0.0              # 'inf'


def scale_ratio(case, true_max):
  """The power of two by which the case's slot moves the scale below the one of an exact
  bound (>= 1): the factor on H2_MAX_REL_ERR."""
  w, w2, gain, bias = slot_words(case, true_max)
  if w is None:
    return 1.0
  e_true = h2_scale_exp([_bits(true_max)])
  e_case = h2_scale_exp([w] + ([w2] if w2 is not None else []), gain, bias)
  return float(2.0 ** max(e_true - e_case, 0))


# ------------------------------------------------------------------------------ layout ---
Buf = collections.namedtuple('Buf', 'rows width floats heads')      # heads: (index, c_off, ldc)


def guard_after(m):
  """Sentinel rows behind the matrix: the dead rows of the last panel and two more."""
  return _cdiv(m, BM) * BM - m + 2


def layout(case):
  """The C buffers of a case: flat, [rows, width] + 4 floats of slack; head i's C starts
  c_off floats into its buffer and has row pitch ldc."""
  rows = GUARD_BEFORE + case.m + guard_after(case.m)
  if case.shared:
    width = sum(n + p for (n, _), p in zip(case.heads, case.pads))
    hs, col = [], 0
    for i, ((n, _), p) in enumerate(zip(case.heads, case.pads)):
      hs.append((i, GUARD_BEFORE * width + col + case.c_off, width))
      col += n + p
    return [Buf(rows, width, rows * width + 4, tuple(hs))]
  return [Buf(rows, n + p, rows * (n + p) + 4,
              ((i, GUARD_BEFORE * (n + p) + case.c_off, n + p),))
          for i, ((n, _), p) in enumerate(zip(case.heads, case.pads))]


def head_places(case):
  """Per head: (buffer index, c_off in floats, ldc)."""
  out = [None] * len(case.heads)
  for bi, b in enumerate(layout(case)):
    for i, off, ldc in b.heads:
      out[i] = (bi, off, ldc)
  return out


def a_floats(case):
  return case.a_off + (case.m + A_NAN_ROWS) * case.lda


def wh_bytes(n):
  return _cdiv(n, 128) * (K // 16) * 8192 + _cdiv(n, 128) * 128 * 4


PLAIN_PACK_MAX_N = 4096            # above it Wp (never read on the fp16-pair path) aliases Wh


def device_bytes(case):
  """Bytes of everything a case keeps on the device at one time: A, the slots, the weights in
  both packings, the biases and ONE set of C buffers (the two kernels' outputs are compared on
  the host)."""
  total = 4 * a_floats(case) + 2 * 64 * 4
  for n, _ in case.heads:
    total += wh_bytes(n) + 4 * (_cdiv(n, 128) * 128 + 4)
    if n <= PLAIN_PACK_MAX_N:
      total += 4 * K * _cdiv(n, 128) * 128
  return total + sum(4 * b.floats for b in layout(case))


# ------------------------------------------------------------------------------ regime ---
Regime = collections.namedtuple(
    'Regime', 'nt panels range nr blocks last_len odd_start switches paths partial '
    'vec_partial xcds_without_panel xcd_panels last_rows')


def regime(case, cus=CUS):
  ns = [n for n, _ in case.heads]
  nt, panels, rng, nr, blocks = plan_of(ns, case.m, cus)
  places = head_places(case)
  paths, partial = [], []
  for t in range(nt):
    pi, tl, _ = hd_tile(ns, t)
    paths.append('v' if vec(ns[pi], places[pi][2], places[pi][1]) else 'e')
    if ns[pi] - tl * BN < BN:
      partial.append(t)
  starts = [r * rng for r in range(nr)]
  switches = 0
  for t0 in starts:
    ps = [hd_tile(ns, t)[0] for t in range(t0, min(t0 + rng, nt))]
    switches = max(switches, sum(a != b for a, b in zip(ps, ps[1:])))
  xp = xcd_panels(panels)
  return Regime(nt, panels, rng, nr, blocks, nt - (nr - 1) * rng,
                any(hd_tile(ns, t0)[2] for t0 in starts), switches, ''.join(paths),
                tuple(partial), any(paths[t] == 'v' for t in partial),
                sum(p == 0 for p in xp), tuple(xp), case.m - (panels - 1) * BM)


STD_HEADS = ((22, True), (68, True), (640, True))        # section C's group


def regime_names(case, cus=CUS):
  """The named regimes (issue sections 4A-4D) a case is in on a device with `cus` CUs."""
  r = regime(case, cus)
  ns = [n for n, _ in case.heads]
  places = head_places(case)
  s = set()
  # A: tile-list structure
  if r.range == r.nt and r.nt <= 4:
    s.add('range_eq_nt%d' % r.nt)
  if r.range == 4 and r.last_len == 1 and r.nt in (5, 9):
    s.add('r4_last_range_one_tile_nt%d' % r.nt)
  if r.nr == 3 and r.last_len == r.range:
    s.add('three_full_ranges')
  if r.range % 2 == 1 and r.odd_start and r.nt > 256:
    s.add('odd_range_item_starts_on_odd_half')
  if r.nt > 256 and r.range > 4 and r.last_len == 1:
    s.add('long_list_last_range_one_tile')
  if len(ns) == 1:
    s.add('single_problem')
  if (len(ns) == 8 and r.nt == 8 and r.paths in ('veveveve', 'evevevev') and
      all(case.heads[i][1] != case.heads[i + 1][1] for i in range(7))):
    s.add('group8_every_tile_switches')
  for t0 in range(0, r.nt, r.range):
    if r.paths[t0:min(t0 + r.range, r.nt)] == 'evee':
      s.add('evee_in_one_range')
  if len(ns) >= 2 and tile0(ns)[1] % 2 == 1 and ns[1] > BN:
    s.add('second_problem_on_odd_tiles')
  # B: N per problem, where N alone decides the path
  plain = (not case.shared and case.c_off == 0 and not any(case.pads))
  if plain:
    for n in ns:
      if n % 4:
        s.add('elem_n%d' % n)
      else:
        s.add(('vec_partial_n%d' if n % BN else 'vec_full_n%d') % n)
  # C: rows
  if case.heads == STD_HEADS:
    s.add('m%d' % case.m)
  for k in (0, 1, 2):
    if k in r.xcd_panels:
      s.add('xcd_with_%d_panels' % k)
  if len(set(r.xcd_panels)) > 1 and min(r.xcd_panels) > 0:
    s.add('uneven_panel_split')
  if r.last_rows < BM:
    s.add('partial_last_panel')
  if r.last_rows < 32:
    s.add('last_panel_under_one_wave')
  # D: addressing and scale
  if plain:
    s.add('ldc_eq_n')
  if not case.shared and all(p == 4 for p in case.pads) and case.c_off == 0:
    s.add('ldc_n_plus_4')
  for n, (_, off, ldc) in zip(ns, places):
    if n % 4 == 0 and ldc % 4 != 0:
      s.add('elem_by_ldc')
    if n % 4 == 0 and ldc % 4 == 0 and (4 * off) % 16 != 0:
      s.add('elem_by_alignment')
  if case.shared:
    s.add('shared_buffer')
    if 'v' in r.paths:
      s.add('shared_buffer_vector_path')
  s.add('c_stream%d' % case.c_stream)
  if case.lda > K:
    s.add('lda_gt_k')
  if case.a_off == 4:
    s.add('a_16_bytes_into_allocation')
  if case.bias_off == 1 and any(b for _, b in case.heads):
    s.add('bias_offset_one_float')
  if case.scale:
    s.add('scale_' + case.scale)
  return s


REQUIRED_REGIMES = (
    # 4A
    ['range_eq_nt%d' % i for i in (1, 2, 3, 4)] +
    ['r4_last_range_one_tile_nt5', 'r4_last_range_one_tile_nt9', 'three_full_ranges',
     'odd_range_item_starts_on_odd_half', 'long_list_last_range_one_tile', 'single_problem',
     'group8_every_tile_switches', 'evee_in_one_range', 'second_problem_on_odd_tiles'] +
    # 4B
    ['elem_n%d' % n for n in (1, 3, 22, 65, 127, 129)] +
    ['vec_partial_n%d' % n for n in (4, 60, 68, 124)] +
    ['vec_full_n%d' % n for n in (64, 128, 640)] +
    # 4C
    ['m%d' % m for m in (9, 31, 33, 127, 128, 129, 255, 256, 257, 896, 1024, 1152, 1920, 2176)] +
    ['xcd_with_0_panels', 'xcd_with_1_panels', 'xcd_with_2_panels', 'uneven_panel_split',
     'partial_last_panel', 'last_panel_under_one_wave'] +
    # 4D
    ['ldc_eq_n', 'ldc_n_plus_4', 'elem_by_ldc', 'elem_by_alignment', 'shared_buffer',
     'shared_buffer_vector_path', 'c_stream0', 'c_stream1', 'lda_gt_k',
     'a_16_bytes_into_allocation', 'bias_offset_one_float'] +
    ['scale_' + k for k in SCALES if k])

NB = (64, False)                                          # a head without bias

CASES = (
    # ---- A: tile-list structure. M = 130: two panels, the second with 2 rows, six XCDs idle
    [Case('a_nt1_single', 130, [22], ['range_eq_nt1', 'single_problem', 'xcd_with_0_panels',
                                     'last_panel_under_one_wave']),
     Case('a_nt2', 130, [22, 64], ['range_eq_nt2']),
     Case('a_nt3', 130, [22, 68], ['range_eq_nt3', 'partial_last_panel']),
     Case('a_nt4_evee', 130, [22, NB, 65], ['range_eq_nt4', 'evee_in_one_range']),
     Case('a_nt4_64_192', 130, [64, 192], ['range_eq_nt4', 'second_problem_on_odd_tiles']),
     Case('a_nt5', 130, [22, 256], ['r4_last_range_one_tile_nt5']),
     Case('a_nt9', 130, [22, 512], ['r4_last_range_one_tile_nt9']),
     Case('a_nt12', 130, [128, 640], ['three_full_ranges']),
     Case('a_nt257', 130, [22, 16384], ['odd_range_item_starts_on_odd_half']),          # R 5
     Case('a_nt337_m200', 200, [22, 5376, 16128], ['long_list_last_range_one_tile']),   # R 6
     Case('a_single_n640', 130, [640], ['single_problem']),
     Case('a_group8', 130, [64, (22, False), 4, (3, False), 60, (1, False), 16, (63, False)],
          ['group8_every_tile_switches'])] +
    # ---- B: N per problem
    [Case('b_elem', 130, [1, 3, 22, 65, 127, 129],
          ['elem_n%d' % n for n in (1, 3, 22, 65, 127, 129)]),
     Case('b_vec_partial', 130, [4, 60, 68, 124],
          ['vec_partial_n%d' % n for n in (4, 60, 68, 124)]),
     Case('b_vec_full', 130, [64, 128, 640],
          ['vec_full_n%d' % n for n in (64, 128, 640)] + ['ldc_eq_n', 'c_stream1'])] +
    # ---- C: rows
    [Case('c_m%d' % m, m, STD_HEADS, ['m%d' % m], seed=m)
     for m in (9, 31, 33, 127, 128, 129, 255, 256, 257)] +
    [Case('c_m%d_p%d' % (128 * p, p), 128 * p, STD_HEADS, ['m%d' % (128 * p)] + e, seed=p)
     for p, e in ((7, ['xcd_with_0_panels', 'xcd_with_1_panels']), (8, ['xcd_with_1_panels']),
                  (9, ['xcd_with_2_panels', 'uneven_panel_split']),
                  (15, ['uneven_panel_split']), (17, ['uneven_panel_split']))] +
    # ---- D: addressing and scale
    [Case('d_ldc_n_plus_4', 130, STD_HEADS, ['ldc_n_plus_4'], pads=[4, 4, 4]),
     Case('d_elem_by_ldc', 130, [64, 68, 128], ['elem_by_ldc'], pads=[1, 1, 1]),
     Case('d_elem_by_alignment', 130, [64, 68], ['elem_by_alignment'], pads=[0, 4], c_off=1),
     Case('d_shared', 130, [22, NB, 68], ['shared_buffer', 'shared_buffer_vector_path'],
          pads=[2, 4, 4], shared=True),
     Case('d_shared_odd_width', 130, [22, 64, 68], ['shared_buffer', 'elem_by_ldc'],
          pads=[3, 4, 1], shared=True),
     Case('d_c_stream0', 130, STD_HEADS, ['c_stream0'], c_stream=0),
     Case('d_lda292', 130, STD_HEADS, ['lda_gt_k'], lda=292),
     Case('d_a_off16', 130, STD_HEADS, ['a_16_bytes_into_allocation'], a_off=4),
     Case('d_bias_off1', 130, STD_HEADS, ['bias_offset_one_float'], bias_off=1)] +
    [Case('d_scale_' + k, 130, STD_HEADS, ['scale_' + k], scale=k) for k in SCALES if k])

# (X, Y) of the history test: Y has another tile count, another number of parity flips per
# item and other store paths than X
HISTORY_PAIR = ('a_nt5', 'b_elem')


# --------------------------------------------------------------------------- arguments ---
def make_args(case, a_ptr, slot_ptr, slot2_ptr, gain, bias, head_ptrs):
  """The ctypes argument array of a case. head_ptrs[i] = (Wp, Wh, bias or None, base of the
  head's C buffer); a_ptr = the base of A's allocation. Plain integers: the plan query
  dereferences nothing."""
  from epos_amd import _lib
  args = []
  for (n, has_bias), (_, off, ldc), (wp, wh, b, cbase) in zip(case.heads, head_places(case),
                                                              head_ptrs):
    args.append(_lib.PointwiseArgs(
        A=a_ptr + 4 * case.a_off, lda=case.lda, Wp=wp,
        bias=b + 4 * case.bias_off if has_bias else None, R=None, ldr=0,
        C=cbase + 4 * off, ldc=ldc, M=case.m, N=n, K=K, relu=0, sub=1, Wh=wh,
        a_amax=slot_ptr, a_amax2=slot2_ptr, a_gain=gain, a_bias=bias,
        c_stream=case.c_stream))
  return (_lib.PointwiseArgs * len(args))(*args)


def host_args(case):
  """make_args with made-up, suitably aligned addresses (for the plan query on the host)."""
  w = slot_words(case, 12.0)
  base = 0x7f0000000000
  hp = [(base + (4 * i + 1 << 28), base + (4 * i + 2 << 28), base + (4 * i + 3 << 28),
         base + (4 * head_places(case)[i][0] + 4 << 28)) for i in range(len(case.heads))]
  return make_args(case, base, base + 0x1000, base + 0x2000 if w[1] is not None else None,
                   w[2], w[3], hp)


def query_plan(lib, args, count, cus):
  """(return value, [nt, panels, range, nr, blocks]) of epos_heads_gemm_plan."""
  out = (ctypes.c_int32 * 5)(*([-1] * 5))
  rc = lib.epos_heads_gemm_plan(args, count, cus, out)
  return rc, list(out)
