"""Host-side regime selection of epos_depthwise3x3_f32, restated in Python, and the shape
table of tests/test_gpu_depthwise.py.

`regime()` mirrors epos_amd/csrc/layers.hip:691-779 (epos_depthwise3x3_f32): the choice
between the generic kernel and the sliding-window depthwise3x3_s1_kernel, ROWS (the
threads2 < 256 * 256 rule and EPOS_DW_ROWS), the partition mode (channel slices / row
bands, EPOS_DW_MODE), the slice unit (128-byte lines only for line-aligned rows and bases),
the distinct slice widths of the FastDiv tables, nres and nrows -- and from
depthwise3x3_s1_kernel (layers.hip:226-275) which per-XCD item ranges end inside a wave and
whether a row band holds rows of two images. Pure Python: the CPU test
tests/test_depthwise_regimes.py checks that the table reaches every regime without a GPU.
"""
import collections

L = 4            # outputs per run (L of epos_depthwise3x3 in layers.hip)
WAVE = 64

Regime = collections.namedtuple(
    'Regime', 'kernel rows mode unit widths nres nrows dead_lanes band_crosses_image')


def _cdiv(a, b):
  return -(-a // b)


def out_size(hi, wi, stride):
  """SAME for stride 1, fixed_padding + VALID for stride 2: both give ceil(hi / stride)."""
  return _cdiv(hi, stride), _cdiv(wi, stride)


def regime(b, hi, wi, c, rate, stride=1, ldx=None, ldy=None, x_off=0, y_off=0,
           rows_env=None, mode_env=None):
  """Regime of one launch. x_off / y_off: byte offsets of the bases from a 128-byte line
  (the caching allocator hands out line-aligned blocks). rows_env / mode_env: the values of
  EPOS_DW_ROWS / EPOS_DW_MODE (None = unset)."""
  ldx = c if ldx is None else ldx
  ldy = c if ldy is None else ldy
  ho, wo = out_size(hi, wi, stride)
  c4n = c // 4
  if not (stride == 1 and hi == ho and wi == wo):
    return Regime('generic', None, None, None, (), None, None, None, None)
  nres = min(rate, wo)
  per_res = _cdiv(wo, rate)
  nchunk = _cdiv(per_res, L)
  rows_env = 2 if rows_env is None else rows_env
  threads2 = b * _cdiv(ho, 2) * _cdiv(wo, L) * c4n
  rows = 1 if (rows_env == 1 or (rows_env != 22 and threads2 < 256 * 256)) else 2
  nrows = _cdiv(ho, 2 * rate) * rate if rows == 2 else ho
  runs = b * nrows * nres * nchunk
  mode = 0 if (c4n >= 128 or (c4n >= 64 and c4n % 8 == 0)) else 1
  if mode_env is not None and mode_env >= 0:
    mode = mode_env
  if c4n < 8:
    mode = 1
  lines = ldx % 32 == 0 and ldy % 32 == 0 and x_off % 128 == 0 and y_off % 128 == 0 and \
      c4n >= 64
  unit = 8 if lines else 1
  nu = _cdiv(c4n, unit)
  widths = []
  slices = []
  for x in range(8):
    lo = (x * nu // 8) * unit
    hi_ = min(((x + 1) * nu // 8) * unit, c4n)
    slices.append(max(hi_ - lo, 0))
    if hi_ - lo > 0 and hi_ - lo not in widths:
      widths.append(hi_ - lo)
  assert len(widths) <= 3, widths            # the kernel has three FastDiv tables
  # items of each XCD (one item = one lane); the waves of an XCD's range are dense, so the
  # last one has dead lanes unless the count is a multiple of 64
  if mode == 0:
    items = [runs * w for w in slices]
  else:
    rows_all = b * nrows
    bands = [((x * rows_all) // 8, ((x + 1) * rows_all) // 8) for x in range(8)]
    items = [(h - l) * nres * nchunk * c4n for l, h in bands]
  dead = any(n % WAVE for n in items if n > 0)
  crosses = False
  if mode == 1:
    crosses = any(h > l and l // nrows != (h - 1) // nrows for l, h in bands)
  if mode == 1:                              # slices (and their unit) are mode 0's alone
    unit, widths = None, ()
  return Regime('s1', rows, mode, unit, tuple(sorted(widths)), nres, nrows, dead, crosses)


# One problem of the table: bases offset by x_off / y_off FLOATS (0 = as allocated).
Shape = collections.namedtuple('Shape', 'name b hi wi c rate stride ldx ldy off')


def S(name, b, hi, wi, c, rate, stride=1, ldx=None, ldy=None, off=0):
  ldx = c if ldx is None else ldx
  # Y always has padding columns (the stray-write check looks at them); it is line-aligned
  # whenever X is, so that X decides the slice unit
  if ldy is None:
    ldy = ldx + 32 if ldx % 32 == 0 else c + 4
  return Shape(name, b, hi, wi, c, rate, stride, ldx, ldy, off)


SHAPES = [
    S('c728_r1_ld736_b2', 2, 61, 83, 728, 1, ldx=736),      # ROWS 2, mode 0, unit 8, 3 widths
    S('c728_r1_dense', 1, 61, 83, 728, 1),                  # ROWS 2, mode 0, unit 1
    S('c728_r2_ld736_tiny', 1, 9, 11, 728, 2, ldx=736),     # ROWS 1, mode 0, unit 8
    S('c128_r1_b2', 2, 121, 161, 128, 1),                   # ROWS 2, mode 1
    S('c128_r3_b3_band', 3, 97, 129, 128, 3),               # ROWS 2, mode 1, bands cross images
    S('c264_r5_b3', 3, 41, 57, 264, 5),                     # ROWS 1, mode 1
    S('c1536_r12_b2', 2, 34, 45, 1536, 12),                 # ROWS 2, Ho % 24 = 10
    S('c2048_r24_rate_ge_wo', 1, 33, 45, 2048, 24),         # ROWS 2, rate >= Wo
    S('c728_r12_rate_gt_wo', 2, 10, 7, 728, 12, ldx=736),   # rate > Wo, rate > Ho
    S('c256_r1_entry_c4', 1, 135, 180, 256, 1),             # odd Ho, one line per XCD
    S('c256_r1_off4_ld256', 1, 47, 61, 256, 1, ldx=256, ldy=256, off=4),  # unaligned bases
    S('c40_r2_b3_band', 3, 29, 37, 40, 2),                  # mode 1 bands across images
    S('s2_c256', 2, 33, 47, 256, 1, stride=2),              # generic kernel, C >= 256
    S('s2_c728_ld736', 1, 31, 42, 728, 1, stride=2, ldx=736),   # generic, ldx != C
    S('s2_c64_ld72_odd', 2, 15, 21, 64, 1, stride=2, ldx=72),    # generic, odd maps
]


def shape_regime(s, **env):
  off = 4 * s.off
  return regime(s.b, s.hi, s.wi, s.c, s.rate, s.stride, s.ldx, s.ldy, off, off, **env)


# Problems run under every process-wide switch (one child process per setting)
SWITCHES = [{'EPOS_DW_ROWS': '1'}, {'EPOS_DW_ROWS': '22'}, {'EPOS_DW_MODE': '0'},
            {'EPOS_DW_MODE': '1'}, {'EPOS_DW_THREADS': '64'}]

SWITCH_SHAPES = [
    S('sw_c728_r1_ld736_b2', 2, 31, 45, 728, 1, ldx=736),   # ROWS 2, mode 0, unit 8
    S('sw_c264_r5_b3', 3, 41, 57, 264, 5),                  # ROWS 1, mode 1
    S('sw_c128_r3_b2', 2, 61, 83, 128, 3),                  # ROWS 2, mode 1
    S('sw_c728_r12_rate_gt_wo', 2, 10, 7, 728, 12, ldx=736),   # rate > Ho, Wo
    S('sw_c32_r8_tiny', 2, 5, 6, 32, 8),                    # c4n = 8, rate > Ho, Wo
]


def switch_env(env):
  """EPOS_DW_* switches -> keyword arguments of regime() (EPOS_DW_THREADS changes only the
  workgroup size, not the regime)."""
  kw = {}
  if 'EPOS_DW_ROWS' in env:
    kw['rows_env'] = int(env['EPOS_DW_ROWS'])
  if 'EPOS_DW_MODE' in env:
    kw['mode_env'] = int(env['EPOS_DW_MODE'])
  return kw
