"""CPU-only checks of the glue-layer and correspondence test tables (tests/helpers/glue_cases.py)
and their references (tests/helpers/glue_ref.py): the tables reach every regime the launchers and
kernels distinguish, the mirrors give the values worked out by hand from glue.hip / layers.hip /
bf16.hip / corresp.hip, the float32 restatements lie within derived bounds of float64, and the inputs have
the properties that make the GPU comparisons mean something."""
import numpy as np
import pytest
import torch

from helpers import glue_cases as gc
from helpers import glue_ref as gr
from helpers.bf16_ref import bf16_round

EPS = 2.0 ** -24                 # unit roundoff of float32


def _names(table):
  return [c.name for c in table]


def test_case_names_are_unique_and_tensors_stay_small():
  for t in (gc.MEAN, gc.MEAN_BF16, gc.PARTIAL, gc.RESIZE, gc.POOL, gc.SUB, gc.ADD_RELU,
            gc.ADD_RELU_BF16, gc.ARGMAX, gc.SOFTMAX, gc.SCATTER, gc.CORR):
    gc.by_name(t)
  mb = 64 << 20
  assert all(4 * c.b * c.hw * c.ldx <= mb for c in gc.MEAN + gc.MEAN_BF16)
  assert all(4 * c.b * max(c.hi * c.wi * c.ldx, c.ho * c.wo * c.ldy) <= mb for c in gc.RESIZE)
  assert all(4 * c.b * c.hi * c.wi * max(c.ldx, c.ldy) <= mb for c in gc.POOL + gc.SUB)
  assert all(4 * c.n <= mb for c in gc.ADD_RELU + gc.ADD_RELU_BF16)
  assert all(4 * c.n * c.g <= mb for c in gc.SOFTMAX)
  # the correspondence cases: every tensor but the [B, P, O, F, 3] fragment coordinates, which
  # at F >= 63 and the 120x160 / 135x180 maps the issue asks for take up to 112 MB
  for c in gc.CORR:
    o = gr.corr_num_objs(c)
    assert 4 * gc.CORR_B * c.h * c.w * o * c.f <= mb
    assert 12 * gc.CORR_B * c.h * c.w * o * c.f <= 2 * mb


# ------------------------------------------------------------------------------- mirrors ---
def test_mirrors_give_the_values_worked_out_by_hand():
  # mean: 1200 rows -> phase 0 takes rows 0..448 and 512..960 in two eight-row steps, then
  # 1024, 1088, 1152 singly
  r = gc.mean_regime(1200, 256, 256)
  assert (r.main_loop, r.main_iters0, r.tail_rows0, r.empty_phases) == (True, 2, 3, False)
  r = gc.mean_regime(448, 64, 64)
  assert (r.main_loop, r.main_iters0, r.tail_rows0) == (False, 0, 7)
  r = gc.mean_regime(449, 64, 72)
  assert (r.main_loop, r.main_iters0, r.tail_rows0, r.padded) == (True, 1, 0, True)
  r = gc.mean_regime(300, 72, 72)
  assert (r.main_loop, r.tail_rows0, r.ragged_c, r.groups) == (False, 5, True, 2)
  assert gc.mean_regime(30, 8, 16).empty_phases and not gc.mean_regime(64, 8, 8).empty_phases
  r = gc.mean_regime(300, 256, 256, bf16=True)
  assert (r.phases, r.main_loop, r.tail_rows0) == (32, False, 10)
  assert gc.mean_regime(30, 8, 16, bf16=True).empty_phases
  # partial sums: 150 block rows in 16 groups -> group 0 takes 10, the last group 9
  r = gc.partial_regime(150, 256, 256)
  assert (r.empty_groups, r.ragged_blocks, r.groups) == (False, True, 4)
  assert gc.partial_regime(5, 72, 80) == (True, True, True, True, 2)
  # resize 15x20 -> 29x39 at 72 channels: 2 * 29 * 39 * 18 threads = 159 workgroups + 12 threads
  r = gc.resize_regime(gc.Resize('x', 2, 15, 20, 29, 39, 72, 72, 80))
  assert (r.blocks, r.tail_block, r.down_y, r.padded_x, r.padded_y) == (160, True, False, False,
                                                                        True)
  r = gc.resize_regime(gc.Resize('x', 2, 61, 83, 17, 1, 8, 8, 16))
  assert (r.down_y, r.down_x, r.sx0, r.sy0) == (True, False, True, False)
  # max pool: even sizes pad 0 before / 1 after, odd sizes 1 / 1
  r = gc.pool_regime(gc.Pool('x', 2, 12, 15, 8, 8, 8))
  assert (r.ho, r.wo, r.pad_y, r.pad_x) == (6, 8, 0, 1)
  r = gc.pool_regime(gc.Pool('x', 1, 1, 2, 8, 8, 8))
  assert (r.ho, r.wo, r.pad_y, r.pad_x) == (1, 1, 1, 0)
  r = gc.sub_regime(gc.Sub('x', 1, 2, 5, 8, 3, 8, 16))
  assert (r.ho, r.wo, r.padded_y) == (1, 2, True)
  # add+relu: 1028 floats = 257 float4 threads = one full workgroup + one thread
  assert gc.add_relu_regime(1028) == (257, 2, True)
  assert gc.add_relu_regime(1024) == (256, 1, False)
  assert gc.add_relu_regime(2056, vec=8) == (257, 2, True)
  assert gc.argmax_regime(1000, 22, 22) == (4, True, False, False)
  assert gc.argmax_regime(256, 1, 3) == (1, False, True, True)
  # softmax: G = 64 takes the 16-rows-per-workgroup form only on a 16-byte aligned base, G = 256
  # the float4 form likewise
  assert gc.softmax_regime(64, 17, 0) == ('vec4x16', 16, 2, True)
  assert gc.softmax_regime(64, 17, 1) == ('strided1', 4, 5, True)
  assert gc.softmax_regime(64, 17, 4).kernel == 'vec4x16'
  assert gc.softmax_regime(63, 1000, 0) == ('strided1', 4, 250, False)
  assert gc.softmax_regime(65, 17, 0) == ('strided4', 4, 5, True)
  assert gc.softmax_regime(256, 17, 0) == ('vec4x64', 4, 5, True)
  assert gc.softmax_regime(256, 1000, 1) == ('strided4', 4, 250, False)
  assert gc.softmax_regime(256, 1000, 4).kernel == 'vec4x64'
  assert gc.softmax_regime(255, 17, 0).kernel == 'strided4'
  assert gc.softmax_slots(1000) == (2, 3, 166, [(0, 2), (1, 1), (1, 3)])
  assert gc.softmax_slots(3) == (1, 1, 3, [(0, 1)])
  assert gc.scatter_regime(4, 64) == (256, 1, False)
  # scan: 19200 elements in chunks of 4096 when aligned, of 1024 otherwise
  r = gc.corr_regime(64, 19200)
  assert (r.vec, r.chunks, r.wide, r.pad_lanes, r.tail_wave) == (4, 5, False, False, False)
  r = gc.corr_regime(64, 19200, off=1)
  assert (r.vec, r.chunks) == (1, 19)
  r = gc.corr_regime(22, 5063)
  assert (r.vec, r.chunks, r.pad_lanes, r.tail_wave) == (1, 5, True, True)
  r = gc.corr_regime(129, 5063)
  assert (r.wide, r.nw) == (True, 3)
  assert gc.corr_regime(64, 91).chunks == 1          # the only ragged golden: no carry


# ------------------------------------------------------------------------------ coverage ---
def _mean_coverage(table, bf16):
  regs = {c.name: gc.mean_regime(c.hw, c.c, c.ldx, bf16) for c in table}
  case = gc.by_name(table)
  if not bf16:
    assert any(r.main_loop and r.tail_rows0 for r in regs.values()), 'main loop + single rows'
    assert any(r.main_loop and not r.tail_rows0 for r in regs.values()), 'main loop alone'
    assert any(r.main_iters0 >= 2 for r in regs.values()), 'two eight-row steps'
    assert any(not r.main_loop and not r.empty_phases for r in regs.values())
    assert any(c.hw == 448 for c in table) and any(c.hw == 449 for c in table), 'the threshold'
    assert any(c.hw == 1200 for c in table), '30x40'
  assert any(r.empty_phases for r in regs.values()), 'phases without a row'
  assert any(r.padded for r in regs.values()), 'ldx > C'
  assert any(case[n].c < 64 for n in regs), 'C < 64'
  assert any(r.ragged_c and r.groups > 1 for r in regs.values()), 'C % 64 != 0 over two groups'
  assert any(case[n].off for n in regs), 'offset base'
  assert any(case[n].hw in (4800, 6120) and case[n].c == 2048 for n in regs), 'real plans'
  assert any(case[n].hw == 300 for n in regs), 'the old test'


def test_mean_tables_cover_every_regime():
  _mean_coverage(gc.MEAN, False)
  _mean_coverage(gc.MEAN_BF16, True)
  assert all(gc.bf16_ok(c) for c in gc.MEAN_BF16)
  assert all(c.c % 4 == 0 and c.ldx % 4 == 0 and c.off % 4 == 0 for c in gc.MEAN)
  regs = [gc.partial_regime(c.blocks, c.c, c.ldp) for c in gc.PARTIAL]
  assert any(r.empty_groups for r in regs), 'blocks < 16'
  assert any(r.ragged_blocks and not r.empty_groups for r in regs), 'blocks % 16 != 0'
  assert any(not r.ragged_blocks for r in regs)
  assert any(r.padded for r in regs), 'ldp > C'
  assert any(r.ragged_c for r in regs) and any(c.off for c in gc.PARTIAL)
  assert any(c.blocks == 150 and c.c == 256 for c in gc.PARTIAL), 'C2'


def _resize_coverage(table, vec):
  regs = {c.name: gc.resize_regime(c, vec) for c in table}
  case = gc.by_name(table)
  assert any(r.down_y and r.down_x for r in regs.values()), 'a downscale'
  assert any(r.down_x != r.down_y and not (r.sy0 or r.sx0) for r in regs.values()), 'mixed'
  assert any(r.sy0 for r in regs.values()), 'Ho == 1'
  assert any(r.sx0 for r in regs.values()), 'Wo == 1'
  assert any(r.identity and case[n].hi > 1 for n, r in regs.items()), 'identity'
  assert any(r.broadcast for r in regs.values()), '1x1 broadcast'
  assert any(r.padded_x for r in regs.values()), 'ldx > C'
  assert any(r.padded_y for r in regs.values()), 'ldy > C'
  assert any(c.xoff for c in table) and any(c.yoff for c in table), 'offset bases'
  assert any(r.tail_block for r in regs.values()) and \
      any(not r.tail_block for r in regs.values())
  assert any((c.hi, c.wi, c.ho, c.wo, c.c, c.ldy) == (30, 40, 120, 160, 256, 304) for c in table)
  assert any((c.hi, c.wi, c.ho, c.wo) == (60, 80, 120, 160) for c in table), 'C2 decoder'
  assert any((c.hi, c.wi, c.ho, c.wo) == (68, 90, 135, 180) for c in table), 'C4 decoder'
  assert any((c.hi, c.wi, c.ho, c.wo, c.ldy) == (1, 1, 60, 80, 1280) for c in table), 'C2 pooling'


def test_resize_tables_cover_every_regime():
  _resize_coverage(gc.RESIZE, 4)
  _resize_coverage(gc.RESIZE_BF16, 8)
  want = {(15, 20, 29, 39), (15, 20, 30, 40), (15, 20, 15, 20), (1, 1, 6, 7)}   # the old tests
  assert want <= {(c.hi, c.wi, c.ho, c.wo) for c in gc.RESIZE}
  assert {(15, 20, 59, 79), (1, 1, 9, 13)} <= {(c.hi, c.wi, c.ho, c.wo) for c in gc.RESIZE_BF16}
  assert any(c.c // 4 % 2 for c in gc.RESIZE), 'an odd number of float4 per pixel'


def _pool_coverage(table, vec):
  regs = {c.name: gc.pool_regime(c, vec) for c in table}
  case = gc.by_name(table)
  par = {(case[n].hi % 2, case[n].wi % 2) for n in regs if case[n].hi > 2 and case[n].wi > 2}
  assert par == {(0, 0), (1, 1), (0, 1), (1, 0)}, 'all four parities'
  assert {(r.pad_y, r.pad_x) for r in regs.values()} == {(0, 0), (1, 1), (0, 1), (1, 0)}
  sizes = {(c.hi, c.wi) for c in table}
  assert {(1, 1), (1, 2), (2, 1), (2, 2)} <= sizes, 'H, W of 1 and 2'
  assert any(c.negative for c in table), 'an all-negative tensor'
  assert any(r.padded_x for r in regs.values()) and any(r.padded_y for r in regs.values())
  assert any(c.xoff for c in table) and any(c.yoff for c in table)
  assert any((c.hi, c.wi, c.c) == (240, 320, 64) for c in table), 'ResNet stem'
  assert any(r.tail_block for r in regs.values()) and \
      any(not r.tail_block and r.blocks > 1 for r in regs.values())


def test_pool_and_subsample_tables_cover_every_regime():
  _pool_coverage(gc.POOL, 4)
  _pool_coverage(gc.POOL_BF16, 8)
  assert {(12, 16), (11, 15)} <= {(c.hi, c.wi) for c in gc.POOL if c.c == 8}, 'the old test'
  assert any((c.hi, c.wi, c.c) == (25, 31, 64) for c in gc.POOL_BF16), 'the old bf16 test'
  for table, vec in ((gc.SUB, 4), (gc.SUB_BF16, 8)):
    regs = [gc.sub_regime(c, vec) for c in table]
    assert {1, 2, 3} <= {c.factor for c in table}, 'factor 1, 2, 3'
    assert any(c.hi % 2 != c.wi % 2 and c.factor == 2 for c in table), 'mixed parity'
    assert any(c.hi == 1 and c.wi == 1 for c in table) and any(c.factor > c.hi for c in table)
    assert any(r.padded_x for r in regs) and any(r.padded_y for r in regs)
    assert any(c.xoff for c in table) and any(c.yoff for c in table)
    assert any(c.hi * c.wi >= 120 * 160 and c.c >= 256 for c in table), 'a real-size map'
    assert any(r.tail_block for r in regs) and any(not r.tail_block for r in regs)
  assert {(12, 16), (11, 15)} <= {(c.hi, c.wi) for c in gc.SUB if c.factor == 2}
  assert any((c.hi, c.wi, c.c) == (25, 31, 64) for c in gc.SUB_BF16)


def test_add_relu_argmax_softmax_scatter_tables_cover_every_regime():
  for table, vec in ((gc.ADD_RELU, 4), (gc.ADD_RELU_BF16, 8)):
    regs = [gc.add_relu_regime(c.n, vec) for c in table]
    assert any(r.blocks == 1 and not r.tail_block for r in regs), 'exactly one workgroup'
    assert any(r.blocks == 1 and r.tail_block for r in regs), 'one partial workgroup'
    assert any(r.threads > 256 and r.tail_block and r.threads // 256 == 1 for r in regs), \
        'a tail after one full workgroup (a grid of n / 256 drops it)'
    assert any(r.blocks > 2 and not r.tail_block for r in regs), 'several full workgroups'
    assert any(r.threads == 1 for r in regs), 'one thread'
    assert any(c.n >= 4 << 20 for c in table), 'a real-size tensor'
    assert any(c.negative for c in table) and any(c.off for c in table)
  assert any(c.n == 1024 for c in gc.ADD_RELU)
  regs = {c.name: gc.argmax_regime(c.p, c.c, c.ldx) for c in gc.ARGMAX}
  case = gc.by_name(gc.ARGMAX)
  assert any(r.padded and case[n].off for n, r in regs.items()), 'ldx > C at an offset base'
  assert any(r.single for r in regs.values()), 'C = 1'
  assert any(r.single and r.padded for r in regs.values())
  assert any(not r.tail_block and r.blocks == 1 for r in regs.values()), 'P = 256'
  assert any(not r.tail_block and r.blocks > 1 for r in regs.values()), 'P a multiple of 256'
  assert any(r.blocks == 1 and r.tail_block for r in regs.values()), 'P < 256'
  assert any(c.p == 1000 and c.ldx == c.c for c in gc.ARGMAX), 'the old test'
  assert any(c.p >= 19200 for c in gc.ARGMAX)
  regs = {c.name: gc.softmax_regime(c.g, c.n, c.off) for c in gc.SOFTMAX}
  case = gc.by_name(gc.SOFTMAX)
  assert {1, 2, 22, 31, 33, 63, 64, 65, 128, 255, 256} <= {c.g for c in gc.SOFTMAX}
  for g, vec, other in ((64, 'vec4x16', 'strided1'), (256, 'vec4x64', 'strided4')):
    assert any(case[n].g == g and r.kernel == other for n, r in regs.items()), \
        'G = %d at an unaligned base' % g
    assert any(case[n].g == g and case[n].off and r.kernel == vec for n, r in regs.items())
  # every form x {dense rows, slot rows} x {one row, a partial last workgroup, full workgroups}
  slot_regs = {c.name: gc.softmax_regime(c.g, gc.softmax_slots(c.n)[2], c.off)
               for c in gc.SOFTMAX}
  for k in ('vec4x16', 'strided1', 'vec4x64', 'strided4'):
    ns = {case[n].n for n, r in regs.items() if r.kernel == k}
    assert {1, 3, 17} <= ns, (k, 'n_groups of 1, 3, 17')
    for rows, rg in (('dense', regs), ('slots', slot_regs)):
      of_k = [r for r in rg.values() if r.kernel == k]
      assert any(r.blocks == 1 and r.partial_block for r in of_k), (k, rows)
      assert any(r.blocks > 1 and r.partial_block for r in of_k), (k, rows)
      assert any(not r.partial_block for r in of_k), (k, rows)
    assert any(gc.softmax_slots(case[n].n)[2] == 1 for n, r in regs.items() if r.kernel == k)
  assert all(c.n == 1000 for c in gc.SOFTMAX[:4]) and [c.g for c in gc.SOFTMAX[:4]] == \
      [2, 22, 31, 64], 'the old test'
  regs = [gc.scatter_regime(c.n_blocks, c.width) for c in gc.SCATTER]
  assert any(r.total == 1 for r in regs) and any(r.blocks == 1 and not r.tail_block for r in regs)
  assert any(r.blocks > 1 and r.tail_block for r in regs)
  assert {'asc', 'desc', 'shuffled'} <= {c.order for c in gc.SCATTER}
  assert any(c.width == 1 and c.n_blocks > 256 for c in gc.SCATTER)
  assert any(c.gap == 0 for c in gc.SCATTER) and any(c.width % 4 for c in gc.SCATTER)


def test_correspondence_table_covers_every_regime():
  case = gc.by_name(gc.CORR)
  regs = {c.name: gc.corr_regime(c.f, c.h * c.w, c.off) for c in gc.CORR}
  plain = {(c.f, c.h * c.w) for c in gc.CORR if not c.off and c.capacity is None}
  assert {(f, p) for f in (1, 22, 63, 64) for p in (5063, 19200, 24300)} <= plain
  assert any(r.pad_lanes and not r.wide for r in regs.values()), 'F < 64'
  assert any(r.vec == 1 and r.chunks > 1 and case[n].h * case[n].w % 4 for n, r in regs.items()), \
      'scan<1> over several chunks, P % 4 != 0'
  assert any(r.vec == 1 and r.chunks > 1 and case[n].off and case[n].h * case[n].w % 4 == 0
             for n, r in regs.items()), 'scan<1> picked for unaligned arrays with P % 4 == 0'
  assert any(r.vec == 4 and r.chunks > 1 for r in regs.values()), 'scan<4> over several chunks'
  assert any(r.tail_wave for r in regs.values()), 'a last wave with fewer than 16 pixels'
  assert {c.capacity for c in gc.CORR} == {None, 'total-1', 'slot0', 'zero'}
  assert {2, 3} <= {r.nw for n, r in regs.items() if r.wide and r.vec == 1 and r.chunks > 1}, \
      'wide kernels with the multi-chunk scan<1>'
  assert any(r.wide and case[n].capacity for n, r in regs.items()), 'wide fill overflow'
  for un, al in gc.CORR_ALIGN_PAIRS:
    a, b = case[un], case[al]
    assert (a.f, a.h, a.w, a.seed, a.all_obj) == (b.f, b.h, b.w, b.seed, b.all_obj)
    assert regs[un].vec == 1 and regs[al].vec == 4
  for c in gc.CORR:
    slots = gc.corr_slots(c)
    assert slots[:4] == [(1, 1), (0, 2), (1, 3), (0, 1)]
    assert len({i for i, _ in slots}) == 2 and sum(o == 1 for _, o in slots) == 2


# ---------------------------------------------------------- the float32 restatements ---
@pytest.mark.parametrize('name', _names(gc.MEAN))
def test_mean_restatement_within_derived_bound(name):
  """|err| <= (ceil(HW / phases) + phases + 1) * 2^-24 * mean(|x|) per (image, channel): an
  element passes through at most ceil(HW / phases) - 1 additions in its phase and phases - 1
  across the phases, each with a relative error of 2^-24 of a partial sum that is at most
  sum(|x|); the division adds one more."""
  c = gc.by_name(gc.MEAN)[name]
  x = gr.mean_input(c)
  err = np.abs(gr.mean_f32(x, 64).astype(np.float64) - gr.mean_f64(x))
  bound = (-(-c.hw // 64) + 64 + 1) * EPS * np.abs(x.astype(np.float64)).mean(1)
  assert (err <= bound).all(), (err / bound).max()


@pytest.mark.parametrize('name', _names(gc.MEAN_BF16))
def test_mean_bf16_restatement_within_derived_bound(name):
  c = gc.by_name(gc.MEAN_BF16)[name]
  x = gr.mean_input(c, bf16=True)
  assert np.array_equal(x, bf16_round(x))
  err = np.abs(gr.mean_f32(x, 32).astype(np.float64) - gr.mean_f64(x))
  bound = (-(-c.hw // 32) + 32 + 1) * EPS * np.abs(x.astype(np.float64)).mean(1)
  assert (err <= bound).all(), (err / bound).max()


@pytest.mark.parametrize('name', _names(gc.PARTIAL))
def test_partial_mean_restatement_within_derived_bound(name):
  """The same derivation with 16 row groups; the divisor hw scales value and bound alike."""
  c = gc.by_name(gc.PARTIAL)[name]
  x = gr.partial_input(c)
  err = np.abs(gr.mean_f32(x, 16, c.hw).astype(np.float64) - gr.mean_f64(x, c.hw))
  bound = (-(-c.blocks // 16) + 16 + 1) * EPS * np.abs(x.astype(np.float64)).sum(1) / c.hw
  assert (err <= bound).all(), (err / bound).max()


@pytest.mark.parametrize('name', _names(gc.RESIZE))
def test_resize_restatement_within_derived_bound(name):
  """With d = 4 * 2^-24 * max(Hi, Wi) -- the rounding of the scale and of yo * sy, each relative
  2^-24 of a coordinate below max(Hi, Wi), doubled for the subtraction of the cell index and
  slack -- the weights lx, ly are off by at most d each, which moves the result by at most
  2 d (|tl| + |tr| + |bl| + |br|); the six float32 operations of the two-level lerp add at most
  6 * 2^-24 of the same magnitude. Where rounding puts the float32 sample position into the
  neighbouring cell (a position within d of a grid line), the magnitudes of both cells count.
  Against the exact-position float64 interpolation and against the torch oracle in float64."""
  from oracle import net_ref
  c = gc.by_name(gc.RESIZE)[name]
  x = gr.resize_input(c)
  got, _ = gr.resize_f32(x, c.ho, c.wo)
  ref, _ = gr.resize_f64(x, c.ho, c.wo)
  bound = gr.resize_bound(x, c.ho, c.wo)
  err = np.abs(got.astype(np.float64) - ref)
  assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
  tref = net_ref.resize_bilinear_align_corners(
      torch.from_numpy(x).double().permute(0, 3, 1, 2), (c.ho, c.wo)).permute(0, 2, 3, 1).numpy()
  err = np.abs(got.astype(np.float64) - tref)
  assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
  if (c.hi, c.wi) == (c.ho, c.wo) or (c.hi, c.wi) == (1, 1):
    assert np.array_equal(got, np.broadcast_to(x[:, :1, :1] if c.hi == 1 else x, got.shape))


@pytest.mark.parametrize('name', _names(gc.POOL))
def test_max_pool_reference_equals_the_oracle(name):
  from oracle import net_ref
  c = gc.by_name(gc.POOL)[name]
  x = gr.pool_input(c)
  ref = net_ref.max_pool_3x3_s2_same(torch.from_numpy(x).permute(0, 3, 1, 2))
  got = gr.max_pool_3x3_s2_same(x)
  assert np.array_equal(got, ref.permute(0, 2, 3, 1).numpy())
  r = gc.pool_regime(c)
  assert got.shape == (c.b, r.ho, r.wo, c.c) and np.isfinite(got).all()
  if c.negative:
    assert (x < 0).all() and (got < 0).all()           # a zero-initialised maximum would differ


# -------------------------------------------------------------------------------- inputs ---
def test_inputs_have_the_properties_the_comparisons_need():
  for c in gc.ADD_RELU + gc.ADD_RELU_BF16:
    a, b = gr.add_relu_input(c)
    out = gr.add_relu(a, b)
    if c.negative:
      assert (a + b < 0).all() and not out.any()
    else:
      assert (out > 0).any() and (out == 0).any()
  for c in gc.ARGMAX:
    x = gr.argmax_input(c)
    assert not np.isnan(x).any()
    assert gr.argmax_planted_ok(c, x, gr.argmax(x)), c.name
  big = [c for c in gc.ARGMAX if c.c >= 4 and c.p >= 16]
  assert len(big) >= 4 and any(c.ldx > c.c for c in big)
  x = gr.argmax_input(gc.by_name(gc.ARGMAX)['p300_c22_ld24_off3'])
  assert np.isneginf(x[9]).all() and np.isneginf(x[10, 0]) and (x[8] == x[8].max()).sum() == 2
  for c in gc.SCATTER:
    dst0, offs, src = gr.scatter_problem(c)
    ends = np.sort(offs) + c.width
    assert (np.sort(offs)[1:] >= ends[:-1]).all() and ends[-1] <= dst0.size and offs.min() > 0
    out = gr.scatter(dst0, offs, src, c.width)
    assert (out != dst0).sum() == src.size or c.width * c.n_blocks != src.size


SMALL_CORR = [c.name for c in gc.CORR if c.h * c.w <= 5063]


@pytest.mark.parametrize('name', SMALL_CORR)
def test_correspondence_inputs_hold_every_slot_kind(name):
  """From the oracle's output: the empty slot is empty although some of its pixels sit exactly
  at the threshold, the all-kept slot has P * F rows, the planted tie keeps fragment 2 and drops
  fragment 1, and an ordinary slot has more than 1024 masked pixels (where P allows)."""
  c = gc.by_name(gc.CORR)[name]
  (obj, frag, _, _, _), per_slot, totals, slot_base, pooled = gr.corr_reference(c)
  P, F = c.h * c.w, c.f
  slots = gc.corr_slots(c)
  assert totals[1].tolist() == [0, 0] and (obj[0, :, 2] == np.float32(gr.TAU_A)).any()
  assert totals[0, 0] > 0 and totals[2, 0] > 0 and totals[3, 0] > 0
  if P >= 5063:
    assert max(totals[0, 0], totals[2, 0], totals[3, 0]) > 1024
  if c.all_obj:
    assert totals[4].tolist() == [P, P * F]
  assert slot_base[-1] == len(pooled['px_id']) == totals[:, 1].sum()
  if F >= 3:
    for s in (0, 3):                                  # the two slots of object 1
      img = slots[s][0]
      res = per_slot[s]
      p = gr.TIE_PIXELS[0]
      px = int((obj[img, :p, 1] > np.float32(gr.TAU_A)).sum())     # masked pixels before it
      kept = res['frag_id'][res['px_id'] == px].tolist()
      assert kept == [0, 2], kept
      row = frag[img, p, 0]
      assert row[1] == np.float32(row.max() * np.float32(gr.TAU_B)) and row[2] > row[1]
  for k in gr.CORR_KEYS:
    assert pooled[k].dtype == gr.CORR_DTYPES[k]
  # a capacity case really overflows
  cap = gr.corr_capacity(c, totals, slot_base)
  if c.capacity is not None:
    assert 0 <= cap < slot_base[-1]
