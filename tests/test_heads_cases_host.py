"""CPU-only checks of the dense-heads case table (tests/helpers/heads_cases.py) and of the plan
query epos_heads_gemm_plan: the Python mirrors of choose_range / the block map give what the
library computes, the values pinned in the kernel's header comment hold, the block map covers
every (panel, tile) exactly once, the table reaches every regime tests/test_gpu_heads_regimes.py
is written for, and the query says 0 for every group the kernel does not take. Pointers are
plain host integers: the query dereferences nothing."""
import ctypes

import pytest

from helpers import heads_cases as hc

CASES = hc.by_name(hc.CASES)


@pytest.fixture(scope='module')
def lib():
  from epos_amd import _lib
  return _lib.load()


def _one(**kw):
  """A one-problem group the kernel takes, with fields overridden."""
  from epos_amd import _lib
  f = dict(A=0x7f0000000000, lda=256, Wp=0x7f1000000000, bias=0x7f2000000000, R=None, ldr=0,
           C=0x7f3000000000, ldc=640, M=130, N=640, K=256, relu=0, sub=1, Wh=0x7f4000000000,
           a_amax=0x7f5000000000, a_amax2=None, a_gain=0.0, a_bias=0.0, c_stream=1)
  f.update(kw)
  return _lib.PointwiseArgs(**f)


def _group(*problems):
  from epos_amd import _lib
  return (_lib.PointwiseArgs * len(problems))(*problems)


def _rc(lib, *problems, **kw):
  return lib.epos_heads_gemm_plan(_group(*problems), kw.get('count', len(problems)), 256, None)


def test_case_names_are_unique_and_tensors_stay_small():
  assert len(CASES) == len(hc.CASES)
  for c in hc.CASES:
    assert hc.device_bytes(c) < 64 << 20, (c.name, hc.device_bytes(c))
    big = hc.regime(c).nt > 256
    assert big or hc.device_bytes(c) < 16 << 20, c.name
  assert sum(hc.regime(c).nt > 256 for c in hc.CASES) == 2


def test_mirror_equals_the_plan_query_for_every_case(lib):
  for c in hc.CASES:
    rc, plan = hc.query_plan(lib, hc.host_args(c), len(c.heads), 256)
    assert rc == 1, c.name
    r = hc.regime(c, 256)
    assert plan == [r.nt, r.panels, r.range, r.nr, r.blocks], c.name
    assert plan == list(hc.plan_of([n for n, _ in c.heads], c.m, 256)), c.name


@pytest.mark.parametrize('cus', [256, 304, 64, 8])
def test_mirror_equals_the_plan_query_on_a_sweep(lib, cus):
  """Small (nt, panels) and a few larger ones: one problem of N = 64 nt columns, M = 128
  panels rows (one less: a partial last panel)."""
  for nt in list(range(1, 41)) + [85, 257, 337]:
    for panels in list(range(1, 21)) + [150, 190, 600]:
      n, m = 64 * nt - 3, 128 * panels - 1
      rc, plan = hc.query_plan(lib, _group(_one(N=n, ldc=n, M=m)), 1, cus)
      assert rc == 1
      assert plan == list(hc.plan_of([n], m, cus)), (nt, panels, cus)


def test_pinned_values_of_the_header_comment(lib):
  def plan(m, ns):
    g = _group(*[_one(N=n, ldc=n, M=m, C=0x7f3000000000 + (i << 32))
                 for i, n in enumerate(ns)])
    rc, p = hc.query_plan(lib, g, len(ns), 256)
    assert rc == 1
    assert p == list(hc.plan_of(ns, m, 256))
    return p
  p = plan(19200, [22, 1344, 4032])            # C2
  assert (p[0], p[1], p[2], p[3]) == (85, 150, 9, 10)
  assert max(hc.xcd_panels(150)) == 19 and p[4] == 8 * 190
  p = plan(19200, [22, 21 * 256, 63 * 256])    # F = 256
  assert (p[0], p[2], p[3]) == (337, 17, 20) and p[4] == 8 * 380
  p = plan(24300, [22, 1344, 4032])            # C4
  assert (p[1], p[2], p[3]) == (190, 11, 8) and p[4] == 8 * 192


def _assert_covers(nt, panels, cus=256):
  rng = hc.choose_range(nt, panels, cus)
  nr = -(-nt // rng)
  blocks = 8 * max(px * nr for px in hc.xcd_panels(panels))
  seen = {}
  for b in range(blocks):
    item = hc.block_item(b, nt, panels, rng, nr)
    if item is None:
      continue
    p, t0, t1 = item
    assert 0 <= p < panels and 0 <= t0 < t1 <= nt and t1 - t0 <= rng
    for t in range(t0, t1):
      assert (p, t) not in seen, (nt, panels, p, t)
      seen[(p, t)] = b
  assert len(seen) == nt * panels, (nt, panels)
  # nothing behind the grid: the first workgroup past it has no item either
  for b in range(blocks, blocks + 8):
    assert hc.block_item(b, nt, panels, rng, nr) is None


def test_block_map_covers_every_panel_and_tile_once():
  for panels in range(1, 21):
    for nt in range(1, 41):
      _assert_covers(nt, panels)
  for c in hc.CASES:
    r = hc.regime(c)
    _assert_covers(r.nt, r.panels)


def test_mirrors_give_the_values_worked_out_by_hand():
  assert hc.tile0([22, 64, 65]) == [0, 1, 2, 4]
  assert [hc.hd_tile([22, 64, 65], t) for t in range(4)] == [(0, 0, 0), (1, 0, 0), (2, 0, 0),
                                                              (2, 1, 1)]
  assert hc.hd_tile([64, 192], 1) == (1, 0, 0) and hc.hd_tile([64, 192], 2) == (1, 1, 1)
  assert hc.vec(64, 64, 0) and not hc.vec(64, 65, 0) and not hc.vec(64, 64, 1)
  assert hc.vec(64, 68, 4) and not hc.vec(22, 24, 0)
  assert hc.xcd_panels(7) == [0, 1, 1, 1, 1, 1, 1, 1]
  assert hc.xcd_panels(9) == [1, 1, 1, 1, 1, 1, 1, 2]
  assert hc.xcd_panels(17) == [2, 2, 2, 2, 2, 2, 2, 3]
  # a slot word of 12.5 (exponent 3): s = 2^11; 16.0: 2^10; Inf: 1
  assert hc.h2_scale_exp([hc._bits(12.5)]) == 11
  assert hc.h2_scale_exp([hc._bits(16.0)]) == 10
  assert hc.h2_scale_exp([hc._bits(15.999999)]) == 11
  assert hc.h2_scale_exp([0x7f800000]) == 0
  assert hc.h2_scale_exp([hc._bits(3.0), hc._bits(12.5)]) == 11
  assert hc.h2_scale_exp([hc._bits(12.5)], 2.0, 1.0) == 10           # 26: exponent 4
  ratios = {k: hc.scale_ratio(CASES['d_scale_' + k], 12.5) for k in hc.SCALES if k}
  assert ratios == {'pow2': 2.0, 'pow2_below': 1.0, 'stale': 1024.0, 'amax2': 1.0,
                    'gain': 2.0, 'inf': 2048.0}
  r = hc.regime(CASES['a_nt257'])
  assert (r.nt, r.range, r.nr, r.last_len, r.odd_start) == (257, 5, 52, 2, True)
  r = hc.regime(CASES['a_nt337_m200'])
  assert (r.nt, r.range, r.nr, r.last_len, r.last_rows) == (337, 6, 57, 1, 72)
  r = hc.regime(CASES['a_nt4_evee'])
  assert (r.paths, r.switches, r.partial, r.vec_partial) == ('evee', 2, (0, 3), False)
  r = hc.regime(CASES['a_group8'])
  assert (r.range, r.nr, r.switches, r.paths) == (4, 2, 3, 'veveveve')
  r = hc.regime(CASES['b_vec_partial'])
  assert r.paths == 'vvvvvv' and r.partial == (0, 1, 3, 5) and r.vec_partial
  r = hc.regime(CASES['a_nt1_single'])
  assert (r.panels, r.last_rows, r.xcds_without_panel, r.blocks) == (2, 2, 6, 8)
  r = hc.regime(CASES['d_shared'])
  assert r.paths == 'evvv'
  assert [p[1:] for p in hc.head_places(CASES['d_shared'])] == [
      (4 * 164, 164), (4 * 164 + 24, 164), (4 * 164 + 92, 164)]
  assert hc.regime(CASES['d_elem_by_alignment']).paths == 'eee'
  assert hc.regime(CASES['d_elem_by_ldc']).paths == 'eeeee'


def test_table_reaches_every_regime_by_name():
  reached = {}
  for c in hc.CASES:
    names = hc.regime_names(c, 256)
    # what a case is named for holds at 256 CUs
    assert set(c.expect) <= names, (c.name, set(c.expect) - names)
    for n in c.expect:
      reached.setdefault(n, []).append(c.name)
  missing = [n for n in hc.REQUIRED_REGIMES if n not in reached]
  assert not missing, missing
  assert set(reached) <= set(hc.REQUIRED_REGIMES), set(reached) - set(hc.REQUIRED_REGIMES)
  assert CASES[hc.HISTORY_PAIR[0]] and CASES[hc.HISTORY_PAIR[1]]
  x, y = (hc.regime(CASES[n]) for n in hc.HISTORY_PAIR)
  assert x.nt != y.nt and x.last_len % 2 != y.last_len % 2 and set(x.paths) != set(y.paths)


# --------------------------------------------------------------------------- eligibility ---
def test_the_base_group_is_taken(lib):
  assert _rc(lib, _one()) == 1
  assert _rc(lib, _one(), _one(N=22, ldc=22, C=0x7f6000000000, bias=None)) == 1


@pytest.mark.parametrize('name,fields', [
    ('k128', dict(K=128)),
    ('m8', dict(M=8)),
    ('residual', dict(R=0x7f7000000000, ldr=640)),
    ('relu', dict(relu=1)),
    ('relu_in', dict(relu_in=1)),
    ('sub2', dict(sub=2, Ho=5, Wo=13, Hi=10, Wi=26)),
    ('c_amax', dict(c_amax=0x7f8000000000)),
    ('col_sums', dict(col_sums=0x7f9000000000, col_ld=640)),
    ('a_presplit', dict(a_presplit=1)),
    ('no_a_amax', dict(a_amax=None)),
    ('no_wh', dict(Wh=None)),
    ('ldc_lt_n', dict(ldc=639)),
    ('ldc_gt_2p20', dict(ldc=(1 << 20) + 4)),
    ('lda_not_multiple_of_4', dict(lda=258)),
    ('a_misaligned', dict(A=0x7f0000000008)),
    ('wh_misaligned', dict(Wh=0x7f4000000008)),
    ('bias_misaligned_2_bytes', dict(bias=0x7f2000000002)),
])
def test_query_returns_0_outside_the_kernels_shape(lib, name, fields):
  assert _rc(lib, _one(**fields)) == 0, name
  # also as the second problem of a group whose first problem is fine (fields every problem
  # must share are changed in both)
  shared = {k: v for k, v in fields.items() if k in ('M', 'lda', 'A', 'a_amax')}
  assert _rc(lib, _one(**shared), _one(C=0x7f6000000000, **fields)) == 0, name


def test_query_neighbours_that_are_taken(lib):
  assert _rc(lib, _one(M=9)) == 1
  assert _rc(lib, _one(ldc=1 << 20)) == 1
  assert _rc(lib, _one(bias=0x7f2000000004)) == 1          # offset by one float
  assert _rc(lib, _one(ldc=640 + 1)) == 1
  assert _rc(lib, _one(lda=260)) == 1
  assert _rc(lib, _one(A=0x7f0000000010)) == 1


@pytest.mark.parametrize('field,other', [
    ('A', 0x7f0000001000), ('lda', 260), ('M', 131), ('a_amax', 0x7f5000001000),
    ('a_amax2', 0x7f5000002000), ('a_gain', 2.0), ('a_bias', 1.0)])
def test_query_returns_0_when_the_problems_differ(lib, field, other):
  second = dict(N=22, ldc=22, C=0x7f6000000000)
  assert _rc(lib, _one(), _one(**second)) == 1
  second[field] = other
  assert _rc(lib, _one(), _one(**second)) == 0, field


def test_query_count(lib):
  from epos_amd import _lib
  eight = [_one(N=64, ldc=64, C=0x7f3000000000 + (i << 32)) for i in range(9)]
  assert _rc(lib, *eight[:8]) == 1
  assert _rc(lib, *eight) < 0                                # count 9: an error
  assert b'1..8' in lib.epos_last_error()
  assert lib.epos_heads_gemm_plan(_group(*eight), 0, 256, None) < 0
  assert lib.epos_heads_gemm_plan(None, 1, 256, None) < 0
  assert lib.epos_heads_gemm_plan(_group(_one()), 1, -1, None) < 0
  # plan untouched when the group falls back
  out = (ctypes.c_int32 * 5)(7, 7, 7, 7, 7)
  assert lib.epos_heads_gemm_plan(_group(_one(K=128)), 1, 256, out) == 0
  assert list(out) == [7] * 5
  assert _lib.SYMBOLS['epos_heads_gemm_plan'][0] is ctypes.c_int


def test_query_without_a_device_count_given(lib):
  """cus = 0: the current device's count, or 256 on a machine without one."""
  rc, plan = hc.query_plan(lib, _group(_one()), 1, 0)
  assert rc == 1 and plan[0] == 10 and plan[1] == 2 and 1 <= plan[2] <= 10
