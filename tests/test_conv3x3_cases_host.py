"""CPU-only checks of the implicit 3x3 conv's case table (tests/helpers/conv3x3_cases.py): the
table reaches every regime tests/test_gpu_conv3x3_regimes.py is written for and has no dead
case; the fp64 reference written from the header's sentence equals the oracle's conv2d_same on
every case's geometry; the classifier's tile counts and row-tile choice are the ones worked out
by hand from launch_grouped_split; the 'int' inputs satisfy what the bit-equality of the GPU
test rests on."""
import numpy as np
import pytest
import torch

from helpers import conv3x3_cases as cc

CASES = cc.by_name(cc.CASES)


def test_every_required_regime_is_taken_and_no_case_is_dead():
  assert len(set(cc.REQUIRED_REGIMES)) == len(cc.REQUIRED_REGIMES)
  seen = set()
  for c in cc.CASES:
    names = cc.regime_names(c)
    unknown = names - set(cc.REQUIRED_REGIMES)
    assert not unknown, (c.name, sorted(unknown))
    missing = set(c.expect) - names
    assert not missing, '%s is not in the regime(s) %s it is named for' % (c.name, sorted(missing))
    new = names - seen
    assert new, '%s adds no regime the cases before it do not have' % c.name
    seen |= names
  left = [r for r in cc.REQUIRED_REGIMES if r not in seen]
  assert not left, 'no case takes %s' % left
  print('%d cases, %d regimes' % (len(cc.CASES), len(seen)))


def test_k_steps_reach_every_phase_of_both_rings():
  """Both kernels walk a tap in blocks of 16 channels (H2_BK = SP_BK = 16): 9 Cin / 16 steps.
  Cin = 32 .. 160 reach every residue mod 5 of the h2 ring; 9 Cin / 16 is even for every legal
  Cin, so the split ring sees residues 0 and 2 mod 4 and no others."""
  cins = (32, 64, 96, 128, 160)
  one = {cin: [c for c in cc.CASES if c.cin == cin][0] for cin in cins}
  assert [cc.k_steps(one[c], 'h2') for c in cins] == [18, 36, 54, 72, 90]
  assert {cc.k_steps(one[c], 'h2') % cc.H2_NST for c in cins} == {0, 1, 2, 3, 4}
  assert {cc.k_steps(one[c], 'split') % cc.SP_NST for c in cins} == {0, 2}
  assert cc.k_steps(CASES['cin512'], 'h2') == cc.k_steps(CASES['cin512'], 'split') == 288
  assert 9 * CASES['cin512'].cin == 4608


def test_shapes_stay_small_and_legal():
  big = []
  for c in cc.CASES:
    assert c.cin % 32 == 0 and c.ldx % 4 == 0 and c.ldx >= c.cin and c.rate >= 1
    assert c.ldy >= c.y_off + c.cout and cc.m_of(c) > 8
    if c.y_amax:
      assert cc.vec(c), c.name
    if not (c.b * c.h * c.w <= 400 and c.cin <= 160 and c.cout <= 264):
      big.append(c.name)
  assert tuple(big) == cc.SIZE_EXCEPTIONS == ('rows128', 'tiles_200', 'cin512')
  c = CASES['cin512']
  assert (c.b, c.h, c.w, c.cin, c.cout) == (1, 5, 7, 512, 40)
  for n in cc.HISTORY_PAIR + (cc.STREAM_CASE, cc.GRAPH_CASE, cc.REFUSAL_CASE, cc.IMAGES_CASE):
    assert n in CASES
  x, y = (CASES[n] for n in cc.HISTORY_PAIR)
  assert x.cin != y.cin and x.rate != y.rate and cc.tiles128(x) != cc.tiles128(y)
  assert cc.k_steps(x, 'h2') % cc.H2_NST != cc.k_steps(y, 'h2') % cc.H2_NST
  # the captured launch brings its own slot (the library's slot ring is not for captures), the
  # refusal case has what every refusal is a change of, the image-wise launches three images
  assert CASES[cc.GRAPH_CASE].slot == 'given'
  r = CASES[cc.REFUSAL_CASE]
  assert r.y_amax and cc.vec(r) and r.ldx == r.cin and r.slot == 'given'
  assert CASES[cc.IMAGES_CASE].b == 3 and CASES[cc.IMAGES_CASE].slot == 'given'


def test_tile_counts_and_row_tile_choice_by_hand():
  """launch_grouped_split: 128-row tiles from ceil(M/128) * ceil(N/128) = 200 on, 64-row tiles
  below; launch_grouped_h2 runs a conv on that many 128 x 128 tiles whatever the narrow limit."""
  def shape(b, h, w, cin, cout):
    return cc.Case('x', b, h, w, cin, cout, [])
  # tests/test_gpu_layers.py's largest conv: M = 4*60*80 = 19200 = 150 * 128, N = 64: 150 tiles
  old = shape(4, 60, 80, 32, 64)
  assert cc.m_of(old) == 19200 and cc.tiles128(old) == 150 and cc.split_rows(old) == 64
  # M = 2*80*81 = 12960 = 101 * 128 + 32: 102 row tiles, N = 136: 2 column tiles
  big = CASES['rows128']
  assert cc.m_of(big) == 12960 and cc.m_of(big) % 128 == 32 and big.cout == 136
  assert cc.tiles128(big) == 204 and cc.split_rows(big) == 128
  assert {'split_rows128', 'ragged_m', 'n_two_tiles'} <= cc.regime_names(big)
  # exactly at the threshold: M = 80*160 = 12800 = 100 * 128, two column tiles
  at = CASES['tiles_200']
  assert cc.m_of(at) == 12800 and cc.tiles128(at) == 200 and cc.split_rows(at) == 128
  # one below: 199 is prime, so one column tile and 199 row tiles, M = 127*200 = 25400 =
  # 198 * 128 + 56 (a shape for the classifier alone: the table stays at three large cases)
  below = shape(1, 127, 200, 32, 128)
  assert cc.m_of(below) == 25400 and cc.tiles128(below) == 199 and cc.split_rows(below) == 64
  assert 'split_rows64' in cc.regime_names(below)
  # stride 2: Ho = (H-1)/2 + 1
  assert cc.out_hw(CASES['s2_odd_measured']) == (8, 11) and cc.m_of(CASES['s2_odd_measured']) == 88
  assert cc.out_hw(CASES['s2_even_y_slice']) == (6, 8)
  # the kernel taken
  assert cc.kernel_taken(True, True, 9) == 'h2' and cc.kernel_taken(False, True, 9) == 'split'
  assert cc.kernel_taken(False, False, 9) is None and cc.kernel_taken(True, True, 8) is None
  # the float4 epilogue
  assert cc.vec(CASES['s2_even_y_slice']) and not cc.vec(CASES['cin128_n37'])
  c = CASES['cin160_y_off1']
  assert c.cout % 4 == 0 and c.ldy % 4 and c.y_off == 1 and not cc.vec(c)
  assert {CASES['cin160_y_off1'].ldx - 160, CASES['rate_ge_w'].ldx - 32} == {4, 36}


def test_geometry_edges_are_what_they_are_named_for():
  c = CASES['rate_ge_w']
  assert c.w <= c.rate < c.h
  c = CASES['rate_ge_h']
  assert c.h <= c.rate < c.w
  c = CASES['rate_ge_hw']
  assert c.rate >= c.h and c.rate >= c.w
  inp = cc.inputs(c.name, 'int')
  ref, _ = cc.expected(c.name, 'int')
  gemm = inp.x.reshape(-1, c.cin).astype(np.float64) @ inp.w[1, 1].astype(np.float64) + inp.bias
  assert np.array_equal(ref, np.maximum(gemm, 0))          # only the centre tap is inside
  c = CASES['images_3']
  ho, wo = cc.out_hw(c)
  assert (ho * wo) % 128 and 128 // (ho * wo) == 1        # tile 0 ends inside the second image


def _oracle(x, w, stride, rate):
  from oracle import net_ref
  # float32 (the oracle's type): 72 integer products of at most 225 each are exact in it
  y = net_ref.conv2d_same_raw(torch.from_numpy(x).permute(0, 3, 1, 2), w, stride, rate)
  return y.permute(0, 2, 3, 1).numpy().astype(np.float64)


@pytest.mark.parametrize('name', [c.name for c in cc.CASES])
def test_reference_equals_the_oracle_on_every_geometry(name):
  """conv_ref == oracle.net_ref.conv2d_same_raw exactly on integer data, on the case's B, H, W,
  stride and rate with Cin cut to 8 and Cout to 5."""
  c = CASES[name]
  rng = np.random.default_rng(c.seed)
  x = rng.integers(-15, 16, (c.b, c.h, c.w, 8)).astype(np.float32)
  w = rng.integers(-15, 16, (3, 3, 8, 5)).astype(np.float32)
  ref = cc.conv_ref(x, w, None, c.stride, c.rate, False)
  assert ref.shape == (c.b,) + cc.out_hw(c) + (5,)
  assert np.array_equal(ref, _oracle(x, w, c.stride, c.rate))
  # ... and the im2col the float32 yardstick of cin512 multiplies is the same convolution
  assert np.array_equal(
      (cc.im2col(x, c.stride, c.rate).astype(np.float64) @ w.reshape(72, 5)).reshape(ref.shape),
      ref)


def test_reference_reproduces_the_slim_known_answers():
  """external/slim/nets/resnet_v1_test.py:72-109, the values test_slim_conv2d_same_kat_on_device
  holds the im2col path to: x, w = i + j grids, 4x4 input; stride 2 gives [[14, 43], [43, 84]],
  not TF-SAME's [[48, 37], [37, 22]]."""
  x = np.add.outer(np.arange(4), np.arange(4)).astype(np.float32).reshape(1, 4, 4, 1)
  w = np.add.outer(np.arange(3), np.arange(3)).astype(np.float32).reshape(3, 3, 1, 1)
  y1 = cc.conv_ref(x, w, None, 1, 1, False).reshape(4, 4)
  assert y1.tolist() == [[14, 28, 43, 26], [28, 48, 66, 37], [43, 66, 84, 46], [26, 37, 46, 22]]
  assert cc.conv_ref(x, w, None, 2, 1, False).reshape(2, 2).tolist() == [[14, 43], [43, 84]]
  # bias and ReLU
  y = cc.conv_ref(x, w, np.float32([-50]), 2, 1, True).reshape(2, 2)
  assert y.tolist() == [[0, 0], [0, 34]]
  ref, mag = cc.conv_ref_mag(-x, w, np.float32([-50]), 2, 1, True)
  assert not ref.any() and mag.reshape(2, 2).tolist() == [[64, 93], [93, 134]]


def test_layout_masks_are_disjoint_and_inside_the_guards():
  for c in cc.CASES:
    m = cc.m_of(c)
    b = cc.y_layout(c)
    mask = cc.written_mask(c)
    assert mask.sum() == m * c.cout
    first, last = np.flatnonzero(mask)[[0, -1]]
    assert first >= cc.GUARD_BEFORE * b.width and last < (b.rows - 2) * b.width
    assert b.rows - cc.GUARD_BEFORE >= -(-m // 128) * 128 + 2
    assert (b.off % 4 == 0) == (c.y_off % 4 == 0)
    # X: the farthest tap of the first and the last pixel stays inside the NaN guard rows
    assert cc.x_guard_rows(c) > c.rate * c.w + c.rate
  c = CASES['cin160_y_off1']
  buf = cc.x_buffer(c, 'int')
  g, n = cc.x_guard_rows(c), c.b * c.h * c.w
  assert buf.shape == (2 * g + n, c.ldx)
  assert np.isnan(buf[:g]).all() and np.isnan(buf[g + n:]).all() and np.isnan(buf[:, c.cin:]).all()
  assert np.array_equal(buf[g:g + n, :c.cin], cc.inputs(c.name, 'int').x.reshape(n, c.cin))
  assert np.isnan(np.array([cc.SENTINEL_BITS], np.uint32).view(np.float32)).all()


@pytest.mark.parametrize('name', [c.name for c in cc.CASES])
def test_int_inputs_are_exact_in_fp32(name):
  """What the bit-equality on 'int' data rests on: integers of at most 4 bits (exact as one fp16
  and as one bf16 piece), x without a zero, every sum of |x||w| + |bias| below 2^24."""
  c = CASES[name]
  inp = cc.inputs(name, 'int')
  for a in (inp.x, inp.w) + ((inp.bias,) if c.bias else ()):
    assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= cc.INT_MAX
  assert (inp.x != 0).all() and inp.true_max == cc.INT_MAX and (inp.bias is None) == (not c.bias)
  ref, mag = cc.expected(name, 'int')
  assert ref.shape == mag.shape == (cc.m_of(c), c.cout)
  assert mag.max() < 2.0 ** 24 and np.array_equal(ref, ref.astype(np.float32))
  assert np.abs(ref).max() > 0


def test_measured_slot_inputs_hide_the_maximum_from_a_short_measurement():
  """slot 'measured': the first B*Ho*Wo pixels stay at a quarter of max |x| or below, the last
  pixel holds the maximum -- at stride 2 a bound measured over M rows would be 4x too small."""
  for c in cc.CASES:
    if c.slot != 'measured':
      continue
    for kind in c.kinds:
      inp = cc.inputs(c.name, kind)
      flat = np.abs(inp.x.reshape(-1, c.cin))
      assert flat[-1, -1] == inp.true_max
      if c.stride == 2:
        assert cc.m_of(c) < flat.shape[0] and 4 * flat[:cc.m_of(c)].max() <= inp.true_max
      assert cc.slot_word(c, inp.true_max) is None and cc.scale_ratio(c, inp.true_max) == 1.0
  c = CASES['s2_r2_stale']
  t = cc.inputs(c.name, 'int').true_max
  assert cc.slot_word(c, t) == int(np.float32(t * 1024).view(np.uint32))
  assert cc.scale_ratio(c, t) == 1024.0
  assert cc.scale_ratio(CASES['s1_r1_cin32'], t) == 1.0
