"""CPU-only checks of the case tables of the small-M GEMV and the bf16 x 6 GEMM (tests/helpers/
gemm_fallback_cases.py): each table reaches every regime tests/test_gpu_gemm_fallback.py is
written for and has no dead case; the routing mirror gives the table the GPU test asserts on the
product library; the launcher mirrors give the counts worked out by hand from the sources; the
exact-integer inputs are exact in any order; the restatement of the GEMV's summation order stays
inside the derived fp64 bound and flags fewer elements than its cap."""
import numpy as np
import pytest

from helpers import gemm_fallback_cases as fc

CASES = fc.by_name(fc.ALL_CASES)


@pytest.mark.parametrize('kernel', ['gemv', 'split'])
def test_every_required_regime_is_taken_and_no_case_is_dead(kernel):
  required = fc.REQUIRED_REGIMES[kernel]
  known = set(required) | set(fc.OPTIONAL_REGIMES[kernel])
  assert len(set(required)) == len(required)
  seen = set()
  table = [c for c in fc.ALL_CASES if c.kernel == kernel]
  for c in table:
    names = fc.regime_names(c)
    unknown = names - known
    assert not unknown, (c.name, sorted(unknown))
    missing = set(c.expect) - names
    assert not missing, '%s is not in the regime(s) %s it is named for' % (c.name, sorted(missing))
    assert c.expect, c.name
    new = names - seen
    assert new, '%s adds no regime the cases before it do not have' % c.name
    seen |= names
  left = [r for r in required if r not in seen]
  assert not left, 'no case takes %s' % left
  print('%s: %d cases, %d regimes' % (kernel, len(table), len(seen)))


def test_routing_mirror_gives_the_table():
  want = {'m8_wp': 'gemv', 'm8_wp_ws': 'gemv', 'm8_wp_wh_bound': 'gemv', 'm8_relu_in': 'gemv',
          'm9_relu_in': 'refused', 'm8_c_amax': 'refused', 'm8_in_group': 'refused',
          'm8_sub2': 'refused', 'm9_ws': 'split', 'm9_wp_only': 'refused',
          'presplit_without_wh': 'refused'}
  assert [r[0] for r in fc.ROUTES] == list(want)
  for name, problems, has, expect in fc.ROUTES:
    assert expect == want[name]
    assert fc.route(problems, set(has)) == expect, name
  # the test build computes what the product library refuses for want of an fp32-MFMA kernel,
  # and nothing else
  ref = {n: fc.route(p, set(h), ref_build=True) for n, p, h, _ in fc.ROUTES}
  assert [n for n in want if ref[n] != want[n]] == ['m9_relu_in', 'm8_in_group', 'm8_sub2',
                                                    'm9_wp_only']
  assert all(ref[n] == 'fp32_mfma' for n in ('m9_relu_in', 'm8_in_group', 'm8_sub2', 'm9_wp_only'))
  # every case of the tables is routed to the kernel it is listed under
  for c in fc.ALL_CASES:
    has = {'Ws'} if c.kernel == 'split' else ({'Ws', 'Wh', 'a_amax'} if c.extra else set())
    assert fc.route(c.problems, has) == c.kernel, c.name
    assert fc.split_eligible(c.problems) == (c.kernel == 'split'), c.name
  for n in fc.SMALL_M_REFUSALS:
    assert want[n] == 'refused'


def test_gemv_slice_loops_by_hand():
  it = fc.gemv_slice_iters
  # K = 2048: 512 quads, 32 per slice = four main iterations of eight, no remainder
  assert {it(2048, s) for s in range(16)} == {(4, 0)}
  # K = 2052: quad 512 is slice 0's
  assert it(2052, 0) == (4, 1) and {it(2052, s) for s in range(1, 16)} == {(4, 0)}
  # K / 4 = 120: slices 0..7 hold 8 quads, slices 8..15 hold 7
  assert [it(480, s) for s in range(16)] == [(1, 0)] * 8 + [(0, 7)] * 8
  assert {it(448, s) for s in range(16)} == {(0, 7)}
  assert [it(4, s) for s in range(16)] == [(0, 1)] + [(0, 0)] * 15
  assert [it(36, s) for s in range(16)] == [(0, 1)] * 9 + [(0, 0)] * 7
  for k in (4, 36, 64, 448, 480, 516, 2048, 2052):        # every quad is taken exactly once
    assert sum(8 * m + r for m, r in (it(k, s) for s in range(16))) == k // 4
    assert max(4 * (8 * m + r) for m, r in (it(k, s) for s in range(16))) == fc.gemv_chain(k)
  assert fc.gemv_grid(fc.P(3, 100, 480)) == (2, 3) and fc.gemv_grid(fc.P(2, 130, 8)) == (4, 2)
  assert fc.gemv_grid(fc.P(1, 1, 4)) == (2, 1)


def test_split_launch_shapes_by_hand():
  P = fc.P
  # 137 x 200: 2 x 2 tiles of 128 x 128 -> 64-row tiles: 3 x 2
  assert fc.split_launch((P(137, 200, 48),)) == (64, 6, [(3, 2)], 'single_plain_64')
  # 199 tiles of 128 x 128 keep the 64-row tile, 200 take the 128-row one
  assert fc.split_launch((P(199 * 128, 128, 16),))[:2] == (64, 398)
  assert fc.split_launch((P(199 * 128 + 1, 128, 16, res=True),)) == (
      128, 200, [(200, 1)], 'single_res_128')
  # a group: the count is the sum over the problems
  g = (P(2900, 1100, 16), P(9, 40, 36))
  assert fc.split_launch(g) == (128, 208, [(23, 9), (1, 1)], 'group_plain_128')
  assert fc.split_launch(g[:1])[0] == 128 and fc.split_launch((P(2816, 1100, 16),))[0] == 64
  assert fc.split_launch((P(9, 22, 20, res=True),) * 2)[3] == 'group_res_64'
  # the float4 epilogue
  assert fc.vec(P(137, 136, 16, c_off=4, pad=4)) and not fc.vec(P(137, 136, 16, c_off=3, pad=1))
  assert not fc.vec(P(137, 22, 16)) and not fc.vec(P(137, 36, 16, res=True, ldr_pad=5))
  assert fc.vec(P(137, 36, 16, res=True))
  # eight column tiles, or one row tile, is no band case
  for p in (P(129, 1024, 16), P(64, 1100, 16)):
    assert not {'band_64', 'band_128'} & fc.regime_names(fc.Case('x', 'split', [p], ['vec']))


@pytest.mark.parametrize('total', [1, 2, 7, 8, 9, 15, 27, 200, 208])
def test_xcd_remap_is_a_permutation(total):
  assert sorted(fc.xcd_remap(raw, total) for raw in range(total)) == list(range(total))
  # the workgroups of one XCD take a contiguous range
  for x in range(min(8, total)):
    mine = [fc.xcd_remap(raw, total) for raw in range(x, total, 8)]
    assert mine == list(range(mine[0], mine[0] + len(mine)))


@pytest.mark.parametrize('tm,tn', [(1, 1), (3, 2), (2, 8), (3, 9), (23, 9), (2, 17)])
def test_band_order_visits_every_tile_once(tm, tn):
  tiles = [fc.split_tile(b, tm, tn) for b in range(tm * tn)]
  assert sorted(tiles) == [(i, j) for i in range(tm) for j in range(tn)]
  if tn > 8:          # all row tiles of the first band come before the second band
    assert {j for _, j in tiles[:tm * 8]} == set(range(8))


def test_shapes_stay_small_and_legal():
  big = 0
  for c in fc.ALL_CASES:
    for p in c.problems:
      assert p.k % 4 == 0 and p.lda % 4 == 0 and p.lda >= p.k and p.ldc >= p.c_off + p.n
      if c.kernel == 'gemv':
        assert len(c.problems) == 1 and 1 <= p.m <= 8 and p.sub == 1 and not p.c_amax
        assert p.n <= 256 and p.k <= 2052
      else:
        assert p.m >= 9 and p.relu_in == 0
        if p.m > 300:
          assert p.k <= 20 and c.name.startswith('big_'), c.name
        else:
          assert p.n <= 300 or (p.k == 16 and p.n <= 1100), c.name
          assert p.k <= 160 or p.k == 728, c.name
      if p.c_amax:
        assert fc.vec(p), c.name
      if p.sub > 1:
        rows = fc.gather_rows(p)
        assert len(set(rows)) == p.m and rows.max() < fc.a_rows(p) and p.m < fc.a_rows(p)
    assert all(q.res == c.problems[0].res for q in c.problems), c.name
    big += c.name.startswith('big_')
    assert fc.split_launch(c.problems)[0] == (128 if c.name.startswith('big_') else 64) or \
        c.kernel == 'gemv', c.name
  assert big == 4
  names = sum(fc.HISTORY_PAIRS, ()) + fc.STREAM_CASES + fc.GRAPH_CASES + (fc.ROW_ALONE_CASE,)
  assert all(n in CASES for n in names)
  for x, y in fc.HISTORY_PAIRS:
    assert fc.regime_names(CASES[x]) != fc.regime_names(CASES[y])
  assert {CASES[n].kernel for n in fc.STREAM_CASES} == {'gemv', 'split'}
  assert {CASES[n].kernel for n in fc.GRAPH_CASES} == {'gemv', 'split'}
  assert CASES[fc.ROW_ALONE_CASE].problems[0].m == 8


def test_layout_masks_are_disjoint_and_inside_the_guards():
  for c in fc.ALL_CASES:
    for bi, b in enumerate(fc.layout(c)):
      mask = fc.written_mask(c, bi)
      assert mask.sum() == sum(c.problems[i].m * c.problems[i].n for i, _, _ in b.problems)
      first, last = np.flatnonzero(mask)[[0, -1]]
      assert first >= fc.GUARD_BEFORE * b.width and last < (b.rows - 2) * b.width


def test_input_buffers_hold_nan_wherever_nothing_may_be_read():
  assert np.isnan(np.array([fc.SENTINEL_BITS], np.uint32).view(np.float32)).all()
  for name in ('k36_m2_n40', 'sub2_single_odd', 'k40_res_ldr'):
    c = CASES[name]
    p = c.problems[0]
    inp = fc.inputs(name, 0)
    buf = fc.a_buffer(p, inp)
    rows = fc.gather_rows(p)
    assert buf.shape == (fc.a_rows(p) + fc.A_NAN_ROWS, p.lda) and p.lda > p.k
    assert np.array_equal(buf[rows, :p.k], inp.a)
    dead = np.ones(buf.shape, bool)
    dead[np.ix_(rows, np.arange(p.k))] = False
    assert np.isnan(buf[dead]).all() and not np.isnan(buf[~dead]).any()
    b = fc.bias_buffer(p, inp.bias)
    assert np.array_equal(b[fc.BIAS_GUARD:fc.BIAS_GUARD + p.n], inp.bias)
    assert np.isnan(b[:fc.BIAS_GUARD]).all() and np.isnan(b[fc.BIAS_GUARD + p.n:]).all()
    if p.res:
      r = fc.r_buffer(p, inp.r)
      g = fc.R_GUARD_ROWS
      assert np.array_equal(r[g:g + p.m, :p.n], inp.r) and p.ldr > p.n
      assert np.isnan(r[:g]).all() and np.isnan(r[g + p.m:]).all() and np.isnan(r[:, p.n:]).all()
  p = CASES['sub2_single_odd'].problems[0]      # 7 x 9 map: rows and columns 0, 2, 4, 6(, 8)
  assert list(fc.gather_rows(p)[:6]) == [0, 2, 4, 6, 8, 18] and fc.gather_rows(p)[20] == 63


def test_exact_integer_inputs_are_exact_in_any_order():
  n = 0
  for c in fc.ALL_CASES:
    if c.values != 'integers':
      continue
    for i, p in enumerate(c.problems):
      inp = fc.inputs(c.name, i)
      for x in (inp.a, inp.w, inp.bias, inp.r):
        assert x is None or np.array_equal(x, np.round(x))
      assert fc.integer_partial_sum_bound(c.name, i) < 2.0 ** 24, (c.name, i)
      exact, _ = fc.expected(c.name, i)
      assert np.array_equal(exact, exact.astype(np.float32).astype(np.float64))
      assert np.abs(exact).max() > 2.0 ** 16         # not a trivially small product either
      # the split kernel's pieces: W fits the first bf16 piece, A needs more than one
      assert np.abs(inp.w).max() <= 7
      if c.kernel == 'split':
        assert np.abs(inp.a).max() >= 2 ** 9
      n += 1
  assert n >= 6


def test_value_kinds_hold_what_they_are_named_for():
  inp = fc.inputs('negative_relu_in', 0)
  assert (inp.a < 0).all()
  exact, mag = fc.expected('negative_relu_in', 0)
  assert np.array_equal(exact, inp.bias.astype(np.float64) + inp.r.astype(np.float64))
  v, flagged = fc.gemv_restated('negative_relu_in')
  assert np.array_equal(v, (np.float32(0) + inp.bias) + inp.r) and not flagged.any()
  inp = fc.inputs('nan_row', 0)
  bad = ~np.isfinite(inp.a).all(axis=1)
  assert list(bad) == [False, True, False, False]
  assert np.isnan(inp.a[1]).sum() == 1 and np.isinf(inp.a[1]).sum() == 1
  exact, _ = fc.expected('nan_row', 0)
  assert np.isnan(exact[1]).all() and np.isfinite(exact[[0, 2, 3]]).all()
  v, _ = fc.gemv_restated('nan_row')
  assert np.isnan(v[1]).all() and np.isfinite(v[[0, 2, 3]]).all()
  assert (fc.inputs('k36_m2_n40', 0).a >= 0).all() and (fc.inputs('k4_m1_n1', 0).a < 0).any()


@pytest.mark.parametrize('name', [c.name for c in fc.GEMV_CASES])
def test_gemv_restatement_is_inside_the_bound_and_rarely_flagged(name):
  """The kernel's order, restated in numpy, against fp64: inside the derived bound with room (a
  restatement near or over it would mean the bound is not one), exact on integers, and with
  fewer flagged elements than the cap the GPU test allows."""
  case = CASES[name]
  p, = case.problems
  v, flagged = fc.gemv_restated(name)
  exact, mag = fc.expected(name, 0)
  frac = float(flagged.mean())
  print('%s: %d of %d elements flagged' % (name, flagged.sum(), flagged.size))
  assert frac < fc.FLAG_CAP or flagged.sum() == 0
  ok = np.isfinite(exact)
  assert np.array_equal(ok, np.isfinite(v))
  if case.values == 'integers':
    assert np.array_equal(v.astype(np.float64), exact) and not flagged.any()
    return
  bound = fc.gemv_bound(p, mag)
  err = np.abs(v.astype(np.float64) - exact)
  assert (err[ok] <= bound[ok]).all()
  live = ok & (bound > 0)
  ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
  print('%s: restatement worst error / bound = %.4f' % (name, ratio))
  assert ratio < 0.5


def test_restatement_notices_a_lost_quad():
  """Zeroing the last quad of A moves almost every element outside the bound: the bound is tight
  enough to see one quad of 513."""
  name = 'k2052_m2_n130'
  p, = CASES[name].problems
  inp = fc.inputs(name, 0)
  exact, mag = fc.expected(name, 0)
  a = np.maximum(inp.a, 0).astype(np.float64)
  a[:, -4:] = 0
  wrong = a @ inp.w.astype(np.float64) + inp.bias + inp.r
  outside = np.abs(wrong - exact) > fc.gemv_bound(p, mag)
  assert outside.mean() > 0.9
