"""Shape tables of the glue-layer and correspondence kernels (tests/test_gpu_glue_layers.py,
tests/test_gpu_corresp_regimes.py) and, per kernel, a host-side mirror of what its launcher and
the kernel itself branch on (epos_amd/csrc/glue.hip, layers.hip, softmax.hip, bf16.hip,
corresp.hip), in the
style of tests/helpers/dw_regimes.py. Pure Python: tests/test_glue_cases_host.py checks without a
GPU that every table reaches every regime its mirror distinguishes.

Offsets are in ELEMENTS of the tensor's type, from the start of an allocation the caching
allocator hands out 512-byte aligned. Every tensor stays below 64 MB (but the [B, P, O, F, 3]
fragment coordinates of the largest correspondence cases: up to 112 MB). The real-plan shapes are
those of C2 (640x480: 60x80 features, 120x160 heads), C4 (720x540: 68x90, 135x180) and C5
(ResNet-101-beta, 640x480: a 240x320 stem).
"""
import collections


def _cdiv(a, b):
  return -(-a // b)


def _nt(name, fields, **defaults):
  t = collections.namedtuple(name, fields)
  n = len(t._fields)
  vals = [defaults.get(f) for f in t._fields]
  k = next((i for i, f in enumerate(t._fields) if f in defaults), n)
  t.__new__.__defaults__ = tuple(vals[k:])
  return t


def by_name(table):
  d = {c.name: c for c in table}
  assert len(d) == len(table), 'duplicate case names'
  return d


# --------------------------------------------------------------------------------- means ---
# global_avg_pool_kernel: workgroup = (image, 64 channels), 16 float4 lanes x 64 row phases;
# phase p adds rows p, p + 64, ... -- eight at a time while r + 7 * 64 < HW, then one by one --
# and phase 0 adds the 64 partial sums in index order. global_avg_pool_bf16_kernel: 8 lanes of
# 8 channels x 32 phases, no eight-row loop.
Mean = _nt('Mean', 'name b hw c ldx off seed', off=0, seed=0)

MeanRegime = collections.namedtuple(
    'MeanRegime', 'phases main_loop main_iters0 tail_rows0 empty_phases ragged_c padded groups')


def mean_regime(hw, c, ldx, bf16=False):
  phases = 32 if bf16 else 64
  main_iters0 = 0
  r = 0
  if not bf16:
    while r + 7 * 64 < hw:                    # phase 0; higher phases take the same or one less
      main_iters0 += 1
      r += 8 * 64
  tail_rows0 = len(range(r, hw, phases))
  return MeanRegime(phases, (not bf16) and hw > 448, main_iters0, tail_rows0, hw < phases,
                    c % 64 != 0, ldx > c, _cdiv(c, 64))


MEAN = [
    Mean('issue_hw300_c72', 2, 300, 72, 72),                 # the old test's shape
    Mean('hw1200_c256', 2, 1200, 256, 256),                  # 30x40: main loop + single rows
    Mean('hw30_c8_ld16_off', 3, 30, 8, 16, off=4),           # phases without a row, C < 64
    Mean('hw1_c4', 2, 1, 4, 4),                              # one row, one float4
    Mean('hw448_c64', 1, 448, 64, 64),                       # the last size without the main loop
    Mean('hw449_c64_ld72', 1, 449, 64, 72),                  # main loop in phase 0 alone
    Mean('hw512_c128', 2, 512, 128, 128),                    # main loop, no single rows
    Mean('hw6075_c72_ld80_off', 2, 6075, 72, 80, off=8),     # 45x135, ragged C, padded, offset
    Mean('c2_hw4800_c2048', 1, 4800, 2048, 2048),            # C2 / C5: 60x80 encoder features
    Mean('c4_hw6120_c2048', 1, 6120, 2048, 2048),            # C4: 68x90
]
# bf16: C, ldx, offsets multiples of 8
MEAN_BF16 = [
    Mean('issue_hw300_c256', 2, 300, 256, 256),              # the old test's shape (15x20)
    Mean('hw1200_c256', 2, 1200, 256, 256),
    Mean('hw30_c8_ld16_off', 3, 30, 8, 16, off=8),           # phases without a row, C < 64
    Mean('hw1_c8', 2, 1, 8, 8),
    Mean('hw32_c64', 1, 32, 64, 64),                         # one row per phase
    Mean('hw33_c72_ld80', 2, 33, 72, 80),                    # ragged C, padded
    Mean('hw6075_c72_ld80_off', 2, 6075, 72, 80, off=16),
    Mean('c2_hw4800_c2048', 1, 4800, 2048, 2048),
    Mean('c4_hw6120_c2048', 1, 6120, 2048, 2048),
]

# pool_partial_kernel: workgroup = (image, 64 channels), 16 row groups x 16 float4 lanes; row
# group r adds block rows r, r + 16, ...; group 0 adds the 16 partial sums in index order.
Partial = _nt('Partial', 'name b blocks c ldp hw off seed', off=0, seed=0)
PartialRegime = collections.namedtuple('PartialRegime',
                                       'empty_groups ragged_blocks ragged_c padded groups')


def partial_regime(blocks, c, ldp):
  return PartialRegime(blocks < 16, blocks % 16 != 0, c % 64 != 0, ldp > c, _cdiv(c, 64))


PARTIAL = [
    Partial('c2_blocks150_c256', 2, 150, 256, 256, 4800),    # C2: 4800 rows in 32-row blocks
    Partial('c4_blocks192_c256_ld384', 1, 192, 256, 384, 6120),   # 6120 rows -> 192 blocks
    Partial('blocks1_c4', 2, 1, 4, 4, 7),
    Partial('blocks5_c72_ld80_off', 3, 5, 72, 80, 150, off=4),    # blocks < 16
    Partial('blocks16_c64', 1, 16, 64, 64, 512),             # one row per group
    Partial('blocks33_c136_ld144', 2, 33, 136, 144, 1050),   # blocks % 16 != 0, ldp > C
]

# -------------------------------------------------------------------------------- resize ---
Resize = _nt('Resize', 'name b hi wi ho wo c ldx ldy xoff yoff seed', xoff=0, yoff=0, seed=0)
ResizeRegime = collections.namedtuple(
    'ResizeRegime', 'down_y down_x sy0 sx0 identity broadcast padded_x padded_y tail_block '
    'blocks')


def resize_regime(s, vec=4):
  """vec = channels per thread: 4 (fp32 kernel) or 8 (bf16 kernel)."""
  total = s.b * s.ho * s.wo * (s.c // vec)
  return ResizeRegime(s.ho > 1 and s.hi - 1 > s.ho - 1, s.wo > 1 and s.wi - 1 > s.wo - 1,
                      s.ho == 1, s.wo == 1, (s.hi, s.wi) == (s.ho, s.wo),
                      s.hi == 1 and s.wi == 1, s.ldx > s.c, s.ldy > s.c, total % 256 != 0,
                      _cdiv(total, 256))


RESIZE = [
    Resize('issue_15x20_29x39', 2, 15, 20, 29, 39, 72, 72, 80, yoff=4),
    Resize('issue_15x20_30x40', 2, 15, 20, 30, 40, 72, 72, 80, yoff=4),
    Resize('issue_identity', 2, 15, 20, 15, 20, 72, 72, 80, yoff=4),
    Resize('issue_broadcast_6x7', 2, 1, 1, 6, 7, 72, 72, 72),
    Resize('bf16_15x20_59x79', 2, 15, 20, 59, 79, 256, 256, 304),   # the old bf16 test's shapes
    Resize('bf16_1x1_9x13', 2, 1, 1, 9, 13, 256, 256, 304),
    Resize('down_120x160_30x40', 1, 120, 160, 30, 40, 8, 16, 8, xoff=8),
    Resize('down_61x83_17x1', 2, 61, 83, 17, 1, 8, 8, 16),          # Wo == 1: sx = 0
    Resize('7x9_1x5', 1, 7, 9, 1, 5, 16, 24, 24, xoff=8, yoff=8),   # Ho == 1: sy = 0
    Resize('1x1_1x1', 1, 1, 1, 1, 1, 8, 8, 8),
    Resize('identity_9x11_c16', 2, 9, 11, 9, 11, 16, 16, 24, yoff=8),
    Resize('mixed_9x40_33x10', 2, 9, 40, 33, 10, 24, 32, 24),       # up in y, down in x
    Resize('c4_f32only_5x6_11x13', 3, 5, 6, 11, 13, 4, 4, 8),       # one float4 per pixel
    Resize('c12_f32only_34x45_135x180', 1, 34, 45, 135, 180, 12, 20, 12, xoff=4),
    Resize('os16_30x40_120x160', 1, 30, 40, 120, 160, 256, 256, 304),
    Resize('c2_decoder_60x80_120x160', 1, 60, 80, 120, 160, 256, 256, 304),   # C2 / C5 decoder
    Resize('c4_decoder_68x90_135x180', 1, 68, 90, 135, 180, 256, 256, 304),   # C4 decoder
    Resize('c2_pool_1x1_60x80', 1, 1, 1, 60, 80, 256, 256, 1280),   # image pooling into the ASPP
]


def bf16_ok(s):
  """A case the bf16 twins accept: channels, pitches and offsets in multiples of 8."""
  vals = [s.c] + [getattr(s, f) for f in ('ldx', 'ldy', 'ldp', 'xoff', 'yoff', 'off')
                  if hasattr(s, f)]
  return all(v % 8 == 0 for v in vals)


RESIZE_BF16 = [s for s in RESIZE if bf16_ok(s)]

# ------------------------------------------------------------------- max pool, subsample ---
Pool = _nt('Pool', 'name b hi wi c ldx ldy xoff yoff negative seed', xoff=0, yoff=0,
           negative=False, seed=0)
PoolRegime = collections.namedtuple('PoolRegime', 'ho wo pad_y pad_x padded_x padded_y '
                                    'tail_block blocks')


def pool_regime(s, vec=4):
  ho, wo = (s.hi + 1) // 2, (s.wi + 1) // 2                    # TF 'SAME'
  ty, tx = (ho - 1) * 2 + 3 - s.hi, (wo - 1) * 2 + 3 - s.wi
  total = s.b * ho * wo * (s.c // vec)
  return PoolRegime(ho, wo, ty // 2 if ty > 0 else 0, tx // 2 if tx > 0 else 0, s.ldx > s.c,
                    s.ldy > s.c, total % 256 != 0, _cdiv(total, 256))


POOL = [
    Pool('issue_12x16', 2, 12, 16, 8, 8, 8),
    Pool('issue_11x15', 2, 11, 15, 8, 8, 8),
    Pool('odd_even_11x16_ld', 2, 11, 16, 8, 16, 24, xoff=8, yoff=8),
    Pool('even_odd_12x15_ld', 2, 12, 15, 16, 24, 16),
    Pool('1x1', 2, 1, 1, 8, 8, 16),
    Pool('1x2', 1, 1, 2, 8, 8, 16),
    Pool('2x1', 1, 2, 1, 8, 8, 16),
    Pool('2x2', 3, 2, 2, 8, 16, 8),
    Pool('1x7', 1, 1, 7, 8, 8, 8),
    Pool('negative_12x15', 2, 12, 15, 8, 16, 16, negative=True),    # a 0-initialised maximum
    Pool('negative_2x2', 1, 2, 2, 8, 8, 8, negative=True),
    Pool('c4_f32only_7x10', 2, 7, 10, 4, 4, 8),
    Pool('bf16_25x31_c64', 2, 25, 31, 64, 64, 64),                  # the old bf16 test's shape
    Pool('c5_stem_240x320_c64', 1, 240, 320, 64, 64, 64),           # ResNet stem
    Pool('c5_stem_240x320_c128_ld', 1, 240, 320, 128, 128, 136),    # beta stem (128 channels)
]
POOL_BF16 = [s for s in POOL if bf16_ok(s)]

Sub = _nt('Sub', 'name b hi wi c factor ldx ldy xoff yoff seed', xoff=0, yoff=0, seed=0)
SubRegime = collections.namedtuple('SubRegime', 'ho wo padded_x padded_y tail_block blocks')


def sub_regime(s, vec=4):
  ho, wo = (s.hi - 1) // s.factor + 1, (s.wi - 1) // s.factor + 1
  total = s.b * ho * wo * (s.c // vec)
  return SubRegime(ho, wo, s.ldx > s.c, s.ldy > s.c, total % 256 != 0, _cdiv(total, 256))


SUB = [
    Sub('issue_12x16_f2', 2, 12, 16, 8, 2, 8, 8),
    Sub('issue_11x15_f2', 2, 11, 15, 8, 2, 8, 8),
    Sub('f1_5x7_ld', 2, 5, 7, 8, 1, 16, 24, xoff=8, yoff=8),        # factor 1: a strided copy
    Sub('f3_11x16_ld', 2, 11, 16, 16, 3, 24, 16),
    Sub('f3_2x5', 1, 2, 5, 8, 3, 8, 16),                            # factor > H
    Sub('f2_1x1', 2, 1, 1, 8, 2, 8, 8),
    Sub('f2_12x15_mixed', 1, 12, 15, 8, 2, 8, 16),
    Sub('c4_f32only_9x4_f2', 2, 9, 4, 4, 2, 4, 8),
    Sub('bf16_25x31_c64_f2', 2, 25, 31, 64, 2, 64, 64),             # the old bf16 test's shape
    Sub('c5_shortcut_120x160_c256_f2', 1, 120, 160, 256, 2, 256, 264),   # block1's last unit
]
SUB_BF16 = [s for s in SUB if bf16_ok(s)]

# ------------------------------------------------------------------------------ add+relu ---
AddRelu = _nt('AddRelu', 'name n off negative seed', off=0, negative=False, seed=0)
AddReluRegime = collections.namedtuple('AddReluRegime', 'threads blocks tail_block')


def add_relu_regime(n, vec=4):
  """vec = values per thread: 4 (fp32) or 8 (bf16); 256 threads per workgroup."""
  t = n // vec
  return AddReluRegime(t, _cdiv(t, 256), t % 256 != 0)


ADD_RELU = [
    AddRelu('issue_n1024', 1024),                             # exactly one workgroup
    AddRelu('n4', 4),
    AddRelu('n1000_off', 1000, off=4),                        # one partial workgroup
    AddRelu('n1028', 1028),                                   # one full + one thread
    AddRelu('n3072', 3072),                                   # three full workgroups
    AddRelu('n5000_negative_off', 5000, off=8, negative=True),
    AddRelu('c5_unit_60x80x1024', 60 * 80 * 1024),            # block3 unit output
    AddRelu('odd_tail_61x83x36', 61 * 83 * 36),
]
ADD_RELU_BF16 = [
    AddRelu('issue_25x31x64x2', 2 * 25 * 31 * 64),            # the old bf16 test's size
    AddRelu('n8', 8),
    AddRelu('n2048', 2048),                                   # exactly one workgroup
    AddRelu('n2000_off', 2000, off=8),
    AddRelu('n2056', 2056),
    AddRelu('n6144', 6144),
    AddRelu('n5000_negative_off', 5000, off=16, negative=True),
    AddRelu('c5_unit_60x80x1024', 60 * 80 * 1024),
    AddRelu('odd_tail_61x83x40', 61 * 83 * 40),
]

# -------------------------------------------------------------------------------- argmax ---
# one thread per row, 256 per workgroup; scalar loads, so any element offset is allowed
Argmax = _nt('Argmax', 'name p c ldx off seed', off=0, seed=0)
ArgmaxRegime = collections.namedtuple('ArgmaxRegime', 'blocks tail_block padded single')


def argmax_regime(p, c, ldx):
  return ArgmaxRegime(_cdiv(p, 256), p % 256 != 0, ldx > c, c == 1)


ARGMAX = [
    Argmax('issue_p1000_c22', 1000, 22, 22),
    Argmax('p300_c22_ld24_off3', 300, 22, 24, off=3),
    Argmax('p5_c1', 5, 1, 1),
    Argmax('p7_c1_ld3_off1', 7, 1, 3, off=1),
    Argmax('p256_c2', 256, 2, 2),
    Argmax('p512_c31_ld32', 512, 31, 32),
    Argmax('p100_c64', 100, 64, 64),
    Argmax('p1_c5', 1, 5, 5),
    Argmax('c2_p19200_c22', 19200, 22, 22),                   # 120x160, 21 objects + background
    Argmax('c4_p24300_c31_ld32', 24300, 31, 32),              # 135x180, 30 objects
]

# ------------------------------------------------------------------------------- softmax ---
# softmax_launch (csrc/softmax.hip) picks one of four row forms from (G, alignment of the base),
# the same for epos_softmax_groups_f32 and epos_softmax_slots_f32:
#   'vec4x16'   G == 64, 16-byte aligned: 16 lanes x float4 per row, 16 rows per workgroup; a
#               lane past the last row takes row 0 and stores nothing
#   'strided1'  any other G <= 64: one value per lane, one wave per row, 4 rows per workgroup
#   'vec4x64'   G == 256, 16-byte aligned: 64 lanes x float4, 4 rows per workgroup
#   'strided4'  any other G in (64, 256]: lane l owns values l + 64k, 4 rows per workgroup
# The rows of a launch are the n groups (dense) or the P pixels of each slot (softmax_slots).
Softmax = _nt('Softmax', 'name g n off seed', off=0, seed=0)
SoftmaxRegime = collections.namedtuple('SoftmaxRegime', 'kernel per_block blocks partial_block')


def softmax_regime(g, n, off):
  assert 1 <= g <= 256
  aligned = (4 * off) % 16 == 0
  if g > 64:
    k = 'vec4x64' if g == 256 and aligned else 'strided4'
  else:
    k = 'vec4x16' if g == 64 and aligned else 'strided1'
  per = 16 if k == 'vec4x16' else 4
  return SoftmaxRegime(k, per, _cdiv(n, per), n % per != 0)


def softmax_slots(n):
  """(B, O, P, slots) of the slot form of a case with n groups: its first B * P * O groups laid
  out as [B, P, O, G], softmax on the listed (image, object) slots only."""
  if n >= 6:
    return 2, 3, n // 6, [(0, 2), (1, 1), (1, 3)]
  return 1, 1, n, [(0, 1)]


SOFTMAX = [Softmax('g%d_n1000' % g, g, 1000) for g in (2, 22, 31, 64)] + [   # the old test
    Softmax('g1_n1000', 1, 1000),
    Softmax('g33_n1000_off1', 33, 1000, off=1),
    Softmax('g63_n1000', 63, 1000),
    Softmax('g64_n1000_off1', 64, 1000, off=1),               # unaligned: one value per lane
    Softmax('g64_n1000_off4', 64, 1000, off=4),               # aligned again
    Softmax('g64_n1', 64, 1), Softmax('g64_n3', 64, 3), Softmax('g64_n17', 64, 17),
    Softmax('g22_n1', 22, 1), Softmax('g22_n3', 22, 3), Softmax('g22_n17', 22, 17),
    Softmax('g64_n1024', 64, 1024),                           # full workgroups only
    Softmax('c2_g64_n76800', 64, 19200 * 4),                  # 120x160, four objects' fragments
    Softmax('c2_g22_n19200', 22, 19200),                      # the object head of C2
    # 64 < G <= 256
    Softmax('g65_n1', 65, 1), Softmax('g65_n3', 65, 3), Softmax('g65_n17', 65, 17),
    Softmax('g128_n1000', 128, 1000),
    Softmax('g255_n17_off1', 255, 17, off=1),
    Softmax('g256_n1', 256, 1), Softmax('g256_n3', 256, 3), Softmax('g256_n17', 256, 17),
    Softmax('g256_n1000', 256, 1000),
    Softmax('g256_n1000_off1', 256, 1000, off=1),             # unaligned: the strided form
    Softmax('g256_n1000_off4', 256, 1000, off=4),             # aligned again
    Softmax('g128_n24', 128, 24), Softmax('g256_n24', 256, 24),   # slots: P = 4, one full workgroup
]

# ------------------------------------------------------------------------------- scatter ---
# block b of `width` floats goes to dst + offsets[b]; one thread per float. order: how the
# destination offsets are laid out ('asc', 'desc', 'shuffled'); gap: free floats between blocks.
Scatter = _nt('Scatter', 'name n_blocks width gap order seed', gap=0, order='asc', seed=0)
ScatterRegime = collections.namedtuple('ScatterRegime', 'total blocks tail_block')


def scatter_regime(n_blocks, width):
  t = n_blocks * width
  return ScatterRegime(t, _cdiv(t, 256), t % 256 != 0)


SCATTER = [
    Scatter('one_float', 1, 1, gap=3),
    Scatter('b7_w64_dense', 7, 64),
    Scatter('b4_w64_full_block', 4, 64, gap=1),               # exactly one workgroup
    Scatter('b300_w192_shuffled', 300, 192, gap=64, order='shuffled'),   # planted frag coords
    Scatter('b1000_w1_desc', 1000, 1, gap=21, order='desc'),  # planted object confidences
    Scatter('b5000_w22_shuffled', 5000, 22, gap=2, order='shuffled'),
    Scatter('b513_w3', 513, 3, gap=5),
]

# ------------------------------------------------------------------------ correspondences ---
# B = 2 images, O = 4 objects: object 1 ('a') and 3 ('c') are ordinary, object 2 ('b') is masked
# nowhere, object 4 ('d') -- where the case has it -- is masked everywhere with every fragment
# kept. Slots (1, a), (0, b), (1, c), (0, a) [, (1, d)]: two images interleaved, one object
# twice. off: offset of px_off / corr_off in int32 elements from an aligned base. capacity:
# None = exactly the total; 'total-1', 'slot0' (the first slot's rows), 'zero'.
Corr = _nt('Corr', 'name f h w off capacity all_obj seed', off=0, capacity=None, all_obj=False,
           seed=0)
CorrRegime = collections.namedtuple('CorrRegime', 'wide nw vec chunks tail_wave pad_lanes')
CORR_O = 4
CORR_B = 2


def corr_slots(case):
  return [(1, 1), (0, 2), (1, 3), (0, 1)] + ([(1, 4)] if case.all_obj else [])


def corr_regime(f, p, off=0):
  """corr_mask / corr_fill: one wave per 16 pixels, lane = fragment, F > 64 -> the wide kernels
  with nw = ceil(F / 64) words. corr_scan: VEC = 4 when P % 4 == 0 and both arrays are 16-byte
  aligned (slot rows stay aligned because P % 4 == 0), chunks of 1024 * VEC elements."""
  vec = 4 if p % 4 == 0 and (4 * off) % 16 == 0 else 1
  return CorrRegime(f > 64, _cdiv(f, 64), vec, _cdiv(p, 1024 * vec), p % 16 != 0, f % 64 != 0)


CORR = [Corr('f%d_%dx%d' % (f, h, w), f, h, w, all_obj=(f == 22 and h == 61), seed=f + h)
        for f in (1, 22, 63, 64) for (h, w) in ((61, 83), (120, 160), (135, 180))] + [
    Corr('kinds_f22_7x13', 22, 7, 13, all_obj=True, seed=1),           # P = 91 < one chunk
    Corr('kinds_f64_32x32_off1', 64, 32, 32, off=1, all_obj=True, seed=2),
    Corr('f64_120x160_off1', 64, 120, 160, off=1, seed=64 + 120),      # scan<1>, P % 4 == 0
    Corr('f22_120x160_off1', 22, 120, 160, off=1, seed=22 + 120),
    Corr('f64_61x83_cap_total-1', 64, 61, 83, capacity='total-1', seed=64 + 61),
    Corr('f64_61x83_cap_slot0', 64, 61, 83, capacity='slot0', seed=64 + 61),
    Corr('f64_61x83_cap_zero', 64, 61, 83, capacity='zero', seed=64 + 61),
    Corr('f22_120x160_cap_slot0', 22, 120, 160, capacity='slot0', seed=22 + 120),
    Corr('wide_f65_61x83', 65, 61, 83, seed=65),
    Corr('wide_f129_61x83', 129, 61, 83, seed=129),
    Corr('wide_f129_61x83_cap_total-1', 129, 61, 83, capacity='total-1', seed=129),
]
# pairs (unaligned case, aligned case) on the same data: the results must be equal
CORR_ALIGN_PAIRS = [('f64_120x160_off1', 'f64_120x160'), ('f22_120x160_off1', 'f22_120x160')]
