"""CPU-only checks of the pre-split fp16-pair GEMM's case table (tests/helpers/
h2_presplit_cases.py): the table reaches every regime tests/test_gpu_h2_presplit.py is written
for and has no dead case; the host encoder of every value kind and the decoder the fp64
expectation rests on agree; the classifier's tile counts and narrow / wide choice are the ones
worked out by hand from launch_grouped_h2."""
import numpy as np
import pytest

from helpers import h2_presplit_cases as pc
from helpers import pointwise_wgrad_ref as wr

CASES = pc.by_name(pc.CASES)


def test_every_required_regime_is_taken_and_no_case_is_dead():
  assert len(set(pc.REQUIRED_REGIMES)) == len(pc.REQUIRED_REGIMES)
  seen = set()
  for c in pc.CASES:
    names = pc.regime_names(c)
    unknown = names - set(pc.REQUIRED_REGIMES)
    assert not unknown, (c.name, sorted(unknown))
    missing = set(c.expect) - names
    assert not missing, '%s is not in the regime(s) %s it is named for' % (c.name, sorted(missing))
    new = names - seen
    assert new, '%s adds no regime the cases before it do not have' % c.name
    seen |= names
  left = [r for r in pc.REQUIRED_REGIMES if r not in seen]
  assert not left, 'no case takes %s' % left
  print('%d cases, %d regimes' % (len(pc.CASES), len(seen)))


def test_shapes_stay_small_and_legal():
  for c in pc.CASES:
    for p in c.problems:
      assert p.m >= 9 and p.k % 4 == 0 and p.lda % 4 == 0 and p.lda >= p.k
      assert p.ldc >= p.c_off + p.n or c.shared
      band = p.n > 300
      assert p.m <= 300 and (p.n <= 300 or (band and p.k == 16 and p.n <= 1100)), c.name
      assert p.k <= 176 or (p.k == 728 and c.name == 'k728_long'), c.name
      if p.c_amax or p.col_sums:            # what the entry point demands of these outputs
        assert pc.vec(p), c.name
      if p.col_sums:
        assert not p.res, c.name
    ms = {p.m for p in c.problems}
    assert not c.shared or len(ms) == 1
  for n in pc.HISTORY_PAIR + (pc.STREAM_CASE, pc.GRAPH_CASE, pc.REFUSAL_CASE):
    assert n in CASES


def test_tile_counts_and_width_choice_by_hand():
  """launch_grouped_h2: 128 x 128 tiles are counted first; the launch runs as 128 x 64 tiles
  when that count is at most the limit and no problem wants block sums."""
  P = pc.P
  # 137 x 200: 2 row tiles x 2 wide column tiles = 4 -> narrow at limit >= 4: 2 x 4 = 8
  assert pc.launch_shape((P(137, 200, 48),), 0) == (128, 4, [(2, 2)])
  assert pc.launch_shape((P(137, 200, 48),), 3) == (128, 4, [(2, 2)])
  assert pc.launch_shape((P(137, 200, 48),), 4) == (64, 8, [(2, 4)])
  # block sums keep the wide tiles whatever the limit
  assert pc.launch_shape((P(137, 136, 48, col_sums=True),), pc.BIG) == (128, 4, [(2, 2)])
  # a group: the limit is held against the sum over the problems (2*2 + 2*1 + 2*2 = 10)
  g = (P(137, 136, 80), P(200, 72, 48), P(137, 200, 80))
  assert pc.launch_shape(g, 9) == (128, 10, [(2, 2), (2, 1), (2, 2)])
  assert pc.launch_shape(g, 10) == (64, 18, [(2, 3), (2, 2), (2, 4)])
  # N = 1100: 9 wide column tiles (one band of 8 and one of 1), 18 narrow (8 + 8 + 2)
  assert pc.launch_shape((P(129, 1100, 16),), 0) == (128, 18, [(2, 9)])
  assert pc.launch_shape((P(129, 1100, 16),), pc.BIG) == (64, 36, [(2, 18)])
  assert 'band_wide' in pc.regime_names(CASES['band_wide'])
  assert 'band_narrow' in pc.regime_names(CASES['band_narrow'])
  # eight column tiles, or one row tile, is no band case
  c8 = pc.Case('x', [P(129, 1024, 16)], [])
  c1 = pc.Case('y', [P(128, 1100, 16)], [])
  assert not {'band_wide', 'band_narrow'} & (pc.regime_names(c8) | pc.regime_names(c1))
  # a group with residuals goes out problem by problem, each launch choosing for itself
  gr = CASES['group_res']
  assert [len(l) for l in pc.launches(gr)] == [1, 1]
  assert {'group_res_serial', 'single_128_res'} <= pc.regime_names(gr)
  assert not {'group_128', 'narrow_64_group'} & pc.regime_names(gr)
  # the float4 epilogue
  assert pc.vec(P(137, 136, 16, c_off=4, pad=4)) and not pc.vec(P(137, 136, 16, c_off=3, pad=1))
  assert not pc.vec(P(137, 22, 16)) and not pc.vec(P(137, 37, 16, res=True))


def test_layout_masks_are_disjoint_and_inside_the_guards():
  for c in pc.CASES:
    for bi, b in enumerate(pc.layout(c)):
      mask = pc.written_mask(c, bi)
      assert mask.sum() == sum(c.problems[i].m * c.problems[i].n for i, _, _ in b.problems)
      first, last = np.flatnonzero(mask)[[0, -1]]
      assert first >= pc.GUARD_BEFORE * b.width and last < (b.rows - 2) * b.width


@pytest.mark.parametrize('name', [c.name for c in pc.CASES])
def test_encoder_and_decoder_round_trip(name):
  """Decoded canonical pairs are within 2^-22 relative of x wherever |x| >= 2^-26 bound, within
  2^-49 bound below; |hi| < 2^15 unless the bound is not finite; x never exceeds its bound."""
  case = CASES[name]
  for i, p in enumerate(case.problems):
    inp = pc.inputs(name, i)
    hi, mid = pc.halves(inp.words)
    bound = float(wr.slot_bound([inp.slot], [inp.slot2] if inp.slot2 is not None else None,
                                inp.gain, inp.bias_a))
    s, inv = wr.h2_scale(bound)
    assert inv == inp.inv and s * inv == 1.0
    if case.scale == 'inf':
      assert not np.isfinite(bound) and s == 1.0
      assert inp.bad_rows.sum() == 2 and inp.bad_rows[3] and inp.bad_rows[5]
    else:
      assert 2.0 ** 14 <= s * bound < 2.0 ** 15
      assert np.isfinite(hi).all() and np.isfinite(mid).all()
      assert np.abs(hi.astype(np.float64)).max() < 2.0 ** 15
      assert not inp.bad_rows.any()
    ok = ~inp.bad_rows
    dec = inp.a64[ok]
    assert np.array_equal(
        dec, (hi[ok].astype(np.float64) + mid[ok].astype(np.float64) * 2.0 ** -11) * inv)
    if case.values in pc.CANONICAL:
      x = inp.x[ok].astype(np.float64)
      if case.scale != 'inf':
        assert np.abs(x).max() <= bound
        big = np.abs(x) >= 2.0 ** -26 * bound
        assert (np.abs(dec - x)[big] <= 2.0 ** -22 * np.abs(x)[big]).all()
        assert (np.abs(dec - x)[~big] <= 2.0 ** -49 * bound).all()
      else:                             # s = 1: a plain fp16 pair of each value
        assert (np.abs(dec - x) <= 2.0 ** -22 * np.abs(x) + 2.0 ** -36).all()
      assert (np.signbit(hi[ok]) == np.signbit(inp.x[ok]))[hi[ok] != 0].all()
    else:
      assert inp.x is None
      assert np.abs(hi.astype(np.float64)).max() == pc.HI_MAX
      j = mid.astype(np.float64) / np.spacing(np.abs(hi)).astype(np.float64)
      assert (j == np.round(j)).all() and np.abs(j).max() == 2047
      assert (np.abs(j) > 1024).any(), 'no pair a canonical split could not produce'


def test_value_kinds_hold_what_they_are_named_for():
  inp = pc.inputs('k64_m129_res_narrow', 0)                  # 'window'
  hi, mid = pc.halves(inp.words)
  sub = lambda h: (h != 0) & (np.abs(h.astype(np.float64)) < 2.0 ** -14)   # noqa: E731
  assert sub(hi).any() and sub(mid).any() and (mid < 0).any() and (mid == 0).any()
  assert (np.signbit(hi) & (hi == 0)).any()                  # -0.0
  assert (np.abs(inp.x) == np.abs(inp.x).max()).sum() >= 2 * inp.x.shape[0]
  exact, mag = pc.expected('k64_m129_res_narrow', 0)
  assert np.isfinite(exact).all() and (mag > 0).all()
  inp = pc.inputs('k48_m128_res', 0)                         # 'zero_rows'
  assert (inp.words[[0, 5, 127]] == 0).all() and (inp.words[32:64] == 0).all()
  inp = pc.inputs('k32_m127_narrow', 0)                      # 'signed'
  assert (inp.x < 0).any() and (inp.x > 0).any()
  exact, _ = pc.expected('scale_inf', 0)
  assert (~np.isfinite(exact)).all(axis=1).sum() == 2 and np.isfinite(exact).all(axis=1).sum() == 135


def test_the_poison_pattern_is_nan_in_both_halves_and_as_fp32():
  w = np.array([pc.A_POISON_BITS], np.uint32)
  assert np.isnan(w.view(np.float16)).all() and np.isnan(w.view(np.float32)).all()
  assert np.isnan(np.array([pc.SENTINEL_BITS], np.uint32).view(np.float32)).all()
  case = CASES['k112_padded']
  buf = pc.a_buffer(case, 0)
  p = case.problems[0]
  assert buf.shape == (p.m + pc.A_NAN_ROWS, p.lda) and p.lda == 128
  assert (buf[:p.m, p.k:] == pc.A_POISON_BITS).all() and (buf[p.m:] == pc.A_POISON_BITS).all()
  assert np.array_equal(buf[:p.m, :p.k], pc.inputs(case.name, 0).words)
  with np.errstate(invalid='ignore'):
    assert np.isnan(wr.h2_values(buf, p.lda, 1.0)[:, p.k:]).all()
