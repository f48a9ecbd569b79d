"""The augmentation's host side and its numpy yardstick (tests/helpers/augment_ref.py): Philox
against Random123's known answers, HSV against colorsys, the blur against scipy, the noise's
moments, the JPEG round trip against PIL, and parse / draw / train_heads.prepare."""
import colorsys
import io
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import augment_ref as R      # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'augment_images.npz')

SEVEN = ('{random_adjust_brightness: {min_delta: -0.2, max_delta: 0.2}, '
         'random_adjust_contrast: {min_delta: 0.8, max_delta: 1.2}, '
         'random_adjust_saturation: {min_delta: 0.8, max_delta: 1.2}, '
         'random_adjust_hue: {max_delta: 0.02}, random_blur: {max_sigma: 1.5}, '
         'random_gaussian_noise: {max_sigma: 0.05}, jpeg_artifacts: {min_quality: 80}}')
SEVEN_NAMES = ['random_adjust_brightness', 'random_adjust_contrast', 'random_adjust_saturation',
               'random_adjust_hue', 'random_blur', 'random_gaussian_noise', 'jpeg_artifacts']


def test_philox_known_answers():
  """Random123's kat_vectors for philox4x32-10."""
  def run(ctr, key):
    return ['%08x' % v for v in R.philox4x32_10(np.array(ctr, np.uint64),
                                                np.array(key, np.uint64))]
  assert run([0] * 4, [0] * 2) == ['6627e8d5', 'e169c58d', 'bc57ac4c', '9b00dbd8']
  assert run([0xffffffff] * 4, [0xffffffff] * 2) == ['408f276d', '41c83b0e', 'a20bc7c6',
                                                     '6d5451fd']
  assert run([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [
      'd16cfe09', '94fdcceb', '5001e420', '24126ea1']
  # vectorised: a batch of counters equals one call per counter
  ctr = np.zeros((5, 4), np.uint64)
  ctr[:, 0] = np.arange(5)
  batch = R.philox4x32_10(ctr, np.array([7, 9], np.uint64))
  for j in range(5):
    assert (batch[j] == R.philox4x32_10(ctr[j], np.array([7, 9], np.uint64))).all()


def test_hsv_against_colorsys():
  rng = np.random.RandomState(0)
  rgb = rng.rand(500, 3)
  rgb[:20] = rgb[:20, :1]                         # greys: max = min, h = 0
  rgb[20:40, 1] = rgb[20:40, 0]                   # two channels tie for the maximum
  rgb[40] = 0.0
  hsv = R.rgb_to_hsv(rgb)
  want = np.array([colorsys.rgb_to_hsv(*p) for p in rgb])
  assert np.abs(hsv - want).max() <= 1e-12
  assert (hsv[:20, 0] == 0).all() and (hsv[..., 0] < 1).all()
  back = R.hsv_to_rgb(hsv)
  want = np.array([colorsys.hsv_to_rgb(*p) for p in hsv])
  assert np.abs(back - want).max() <= 1e-12
  assert np.abs(back - rgb).max() <= 1e-12


def test_blur_against_scipy():
  from scipy import ndimage
  # ksize = round_half_even(8 sigma + 1) | 1, by hand: 3.4 -> 3, 5.8 -> 6 | 1 = 7, 9, 25
  assert [R.blur_ksize(s) for s in (0.3, 0.6, 1.0, 3.0)] == [3, 7, 9, 25]
  assert R.blur_ksize(0.0625) == 3 and R.blur_ksize(0.05) == 1      # 1.5 -> 2 | 1; 1.4 -> 1
  rng = np.random.RandomState(1)
  x = rng.rand(24, 40, 3)
  for sigma in (0.3, 1.0, 2.9):
    ksize = R.blur_ksize(sigma)
    i = np.arange(ksize) - (ksize - 1) // 2
    s32 = float(np.float32(sigma))
    k = np.exp(-i.astype(np.float64) ** 2 / (2 * s32 * s32))
    k = (k / k.sum()).astype(np.float32).astype(np.float64)
    assert np.array_equal(k, R.blur_weights(sigma)) and abs(k.sum() - 1) < 1e-6
    want = ndimage.correlate1d(ndimage.correlate1d(x, k, axis=1, mode='mirror'), k, axis=0,
                               mode='mirror')
    assert np.abs(R.blur(x, sigma) - want).max() <= 1e-13
  assert R.blur(x, 0.0) is x and R.blur(x, 0.05) is x


def test_noise_moments():
  n = 64 * 64 * 3
  z = R.normals(n, 0x12345678, 0x9abcdef0)
  assert z.shape == (n,) and np.isfinite(z).all()
  # four standard errors: of the mean 1 / sqrt(n), of the standard deviation 1 / sqrt(2 n)
  assert abs(z.mean()) <= 4 / np.sqrt(n)
  assert abs(z.std() - 1) <= 4 / np.sqrt(2 * n)
  assert not np.array_equal(z, R.normals(n, 0x12345679, 0x9abcdef0))
  assert np.array_equal(z[:10], R.normals(10, 0x12345678, 0x9abcdef0))


def _pil_round_trip(v, quality):
  from PIL import Image
  buf = io.BytesIO()
  Image.fromarray(v).save(buf, 'JPEG', quality=quality)
  return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB')).astype(np.int64)


# The helper's deviation from PIL (libjpeg's integer DCTs) in grey levels, as measured:
# {fixture: {quality: (mean, max)}}. Asserted: twice the mean, the maximum plus 2.
PIL_MEASURED = {'im_33x47': {80: (0.3484, 9), 90: (0.8839, 7), 99: (0.4092, 4)},
                'im_40x56': {80: (0.5628, 7), 90: (0.5128, 6), 99: (0.4557, 3)}}


@pytest.mark.parametrize('name', sorted(PIL_MEASURED))
def test_jpeg_against_pil(name):
  v = np.load(GOLDEN)[name]
  for q, (mean, worst) in sorted(PIL_MEASURED[name].items()):
    ours = R.jpeg_levels(v, q)
    pil = _pil_round_trip(v, q)
    d = np.abs(ours - pil)
    print('%s q=%d: mean |helper - PIL| = %.4f, max = %d' % (name, q, d.mean(), d.max()))
    assert d.mean() <= 2 * mean and d.max() <= worst + 2, (q, d.mean(), d.max())
    # the bound discriminates: ten quality steps move PIL's own result four times as far
    step = np.abs(pil - _pil_round_trip(v, q - 10)).mean()
    assert step >= 4 * 2 * mean, (q, step)
    assert np.abs(ours - v).mean() > 1.0          # and the round trip is no identity


def test_jpeg_fixtures_are_tie_free():
  """No pre-rounding value of the quantisation or the inverse DCT within 1e-6 of a tie: the
  order of a sum cannot decide a level, so the device can be held to the helper's bytes."""
  golden = np.load(GOLDEN)
  assert sorted(golden.files) == sorted(['im_%dx%d' % s for s in R.FIXTURE_SHAPES] + ['im_low'])
  for name in golden.files:
    v = golden[name]
    assert v.dtype == np.uint8
    for q in (R.LOW_QUALITY,) if name == 'im_low' else R.FIXTURE_QUALITIES:
      out, tie = R.jpeg_levels(v, q, with_ties=True)
      assert tie >= 1e-6, (name, q, tie)
      assert out.shape == v.shape and out.min() >= 0 and out.max() <= 255
  # the smallest fixture is what make_fixtures builds
  h, w = R.FIXTURE_SHAPES[0]
  made = R.tie_free(R.gradient_noise(h, w, h), R.FIXTURE_QUALITIES)
  assert np.array_equal(made, golden['im_%dx%d' % (h, w)])


def test_jpeg_quant_tables_and_upsampling_by_hand():
  assert R.quant_table(R.LUMA, 50)[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61]
  assert R.quant_table(R.LUMA, 75)[0, :3].tolist() == [8, 6, 5]        # scale 50
  assert R.quant_table(R.LUMA, 25)[0, :3].tolist() == [32, 22, 20]     # scale 200
  assert R.quant_table(R.CHROMA, 100).max() == 1 and R.quant_table(R.CHROMA, 1).max() == 255
  # a flat image survives the round trip up to the colour transforms' rounding
  flat = np.full((20, 20, 3), 100, np.int64)
  assert np.abs(R.jpeg_levels(flat, 90) - 100).max() <= 1
  # triangle filter on a 1 x 2 chroma plane: 3/4 near + 1/4 far horizontally
  c = np.array([[100, 200]], np.int64)
  assert R._fancy_upsample(c, 2, 4).tolist() == [[100, 125, 175, 200]] * 2


def test_apply_order_none_and_identity():
  img = np.load(GOLDEN)['im_24x40'].astype(np.float64)
  a = R.apply(img, [(R.BRIGHTNESS, 0.3), (R.CONTRAST, 1.5)])
  b = R.apply(img, [(R.CONTRAST, 1.5), (R.BRIGHTNESS, 0.3)])
  assert np.abs(a - b).max() > 1.0
  assert np.array_equal(R.apply(img, []), img)
  assert np.array_equal(R.apply(img, [(R.NONE, 1.0), (R.BLUR, 0.0)]), img)
  assert np.array_equal(R.apply(img, [(R.NONE, 0.0), (R.BRIGHTNESS, 0.3)]),
                        R.apply(img, [(R.BRIGHTNESS, 0.3)]))
  m = R.apply(img, [(R.CONTRAST, 0.0)])          # factor 0: every pixel becomes the mean
  assert np.abs(m - img.reshape(-1, 3).mean(0)).max() < 1e-9


def test_parse_keeps_order_and_refuses():
  from epos_amd import augment
  ops = augment.parse(SEVEN)
  assert [n for n, _ in ops] == SEVEN_NAMES
  assert ops[0][1] == {'min_delta': -0.2, 'max_delta': 0.2} and ops[6][1] == {'min_quality': 80}
  rev = augment.parse({'jpeg_artifacts': {'min_quality': 90},
                       'random_adjust_hue': {'max_delta': 0.1}})
  assert [n for n, _ in rev] == ['jpeg_artifacts', 'random_adjust_hue']
  for empty in (None, '', 'None', {}, []):
    assert augment.parse(empty) == []
  with pytest.raises(NotImplementedError, match='data_augmentations'):
    augment.parse('random_adjust_brightness')
  with pytest.raises(NotImplementedError, match='data_augmentations'):
    augment.parse('[random_blur]')
  for bad, word in (
      ({'random_adjust_brightnes': {'min_delta': 0, 'max_delta': 1}}, 'random_adjust_brightnes'),
      ({'random_adjust_contrast': {'min_delta': 0.8}}, 'random_adjust_contrast lacks max_delta'),
      ({'random_adjust_saturation': {'min_delta': 1.2, 'max_delta': 0.8}},
       'random_adjust_saturation'),
      ({'random_adjust_hue': {'max_delta': -0.1}}, 'random_adjust_hue'),
      ({'random_blur': {'max_sigma': 8.2}}, 'random_blur'),
      ({'random_blur': {'max_sigma': -1.0}}, 'random_blur'),
      ({'random_gaussian_noise': {'max_sigma': 'x'}}, 'random_gaussian_noise'),
      ({'random_gaussian_noise': None}, 'random_gaussian_noise'),
      ({'jpeg_artifacts': {'min_quality': 0}}, 'jpeg_artifacts'),
      ({'jpeg_artifacts': {'min_quality': 100}}, 'jpeg_artifacts'),
      ({'jpeg_artifacts': {'min_quality': 80.5}}, 'jpeg_artifacts'),
      ({'jpeg_artifacts': {'min_quality': 80, 'max_quality': 90}}, 'jpeg_artifacts')):
    with pytest.raises(ValueError, match=re.escape(word)):
      augment.parse(bad)
  augment.parse({'random_blur': {'max_sigma': 8.0}})      # 65 taps: radius 32, the largest
  assert augment.blur_radius(8.0) == 32 and augment.blur_radius(8.2) == 33
  assert [augment.blur_radius(s) for s in (0.3, 0.6, 1.0, 3.0)] == [1, 3, 4, 12]


def test_draw_is_reproducible_and_inside_its_ranges():
  from epos_amd import augment
  ops = augment.parse(SEVEN)
  a = augment.draw(ops, seed=3, step=17, b=1)
  assert a.dtype == augment.OP_DTYPE and a.dtype.itemsize == 20 and a.shape == (7,)
  assert a.tobytes() == augment.draw(ops, 3, 17, 1).tobytes()
  assert a['kind'].tolist() == [augment.BRIGHTNESS, augment.CONTRAST, augment.SATURATION,
                                augment.HUE, augment.BLUR, augment.NOISE, augment.JPEG]
  seen = set()
  for seed, step, b in ((3, 17, 0), (3, 18, 1), (4, 17, 1), (3, 17, 2)):
    assert augment.draw(ops, seed, step, b).tobytes() != a.tobytes()
  for step in range(200):
    d = augment.draw(ops, 0, step, step % 3)
    assert -0.2 <= d['a'][0] <= 0.2 and 0.8 <= d['a'][1] <= 1.2 and 0.8 <= d['a'][2] <= 1.2
    assert -0.02 <= d['a'][3] <= 0.02 and 0 <= d['a'][4] <= 1.5 and 0 <= d['a'][5] <= 0.05
    assert 80 <= d['a'][6] < 100 and d['a'][6] == int(d['a'][6])
    assert (d['key_lo'][:5] == 0).all() and (d['b'] == 0).all()
    seen.add((int(d['key_lo'][5]), int(d['key_hi'][5]), float(d['a'][6])))
  assert len(seen) == 200 and len({q for _, _, q in seen}) >= 15
  # a degenerate range draws its only value
  one = augment.draw(augment.parse({'random_adjust_contrast': {'min_delta': 1.1,
                                                               'max_delta': 1.1},
                                    'jpeg_artifacts': {'min_quality': 99}}), 0, 0, 0)
  assert one['a'].tolist() == [float(np.float32(1.1)), 99.0]
  # the table of a batch: image b's row is draw(..., b)
  aug = augment.Augmenter(SEVEN, seed=5)
  t = aug.ops(9, 3)
  assert t.shape == (3, 7) and aug.names == SEVEN_NAMES
  for b in range(3):
    assert t[b].tobytes() == augment.draw(ops, 5, 9, b).tobytes()
  assert augment.Augmenter(None).ops(0, 2).shape == (2, 0)


def test_train_heads_prepare_takes_a_mapping(tmp_path, monkeypatch):
  import train_heads
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  base = ['--model=toy', '--dataset', 'lm', '--synthetic', '2']
  args, _ = train_heads.prepare(base)
  assert args.data_augmentations == []
  args, _ = train_heads.prepare(base + ['--data_augmentations', SEVEN])
  assert [n for n, _ in args.data_augmentations] == SEVEN_NAMES
  with pytest.raises(NotImplementedError, match='data_augmentations'):
    train_heads.prepare(base + ['--data_augmentations', 'random_adjust_brightness'])
  with pytest.raises(ValueError, match='random_blurr'):
    train_heads.prepare(base + ['--data_augmentations', '{random_blurr: {max_sigma: 1.0}}'])
  # params.yml sets it as a mapping, in its own order
  (tmp_path / 'toy').mkdir()
  (tmp_path / 'toy' / 'params.yml').write_text(
      'data_augmentations:\n  jpeg_artifacts:\n    min_quality: 85\n'
      '  random_adjust_hue:\n    max_delta: 0.05\n')
  args, _ = train_heads.prepare(base)
  assert args.data_augmentations == [('jpeg_artifacts', {'min_quality': 85}),
                                     ('random_adjust_hue', {'max_delta': 0.05})]
  (tmp_path / 'toy' / 'params.yml').write_text(
      'data_augmentations:\n  jpeg_artifacts:\n    min_quality: 0\n')
  with pytest.raises(ValueError, match='jpeg_artifacts'):
    train_heads.prepare(base)


def test_symbols_are_declared_and_bound():
  import ctypes
  from epos_amd import _lib, augment
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  lib = _lib.load()
  for name in ('epos_augment_workspace_bytes', 'epos_augment_f32'):
    assert name in _lib.SYMBOLS and re.search(r'\b%s\s*\(' % name, header)
    assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
  for kind, name in enumerate(('NONE', 'BRIGHTNESS', 'CONTRAST', 'SATURATION', 'HUE', 'BLUR',
                               'NOISE', 'JPEG')):
    assert re.search(r'#define EPOS_AUG_%s %d\b' % (name, kind), header)
    assert getattr(augment, name) == getattr(R, name) == kind
  assert lib.epos_abi_version() == 7
  # the host side of the entries: sizes and refusals need no device
  ws = lib.epos_augment_workspace_bytes
  assert ws(0, 480, 640) == 0 and ws(8, 480, 640) == 8 * ws(1, 480, 640)
  assert ws(1, 480, 640) >= 480 * 640 * 12 + 480 * 640 * 3 // 2 + 64 * 3 * 8
  assert ws(1, 33, 47) >= 33 * 47 * 12 + 48 * 48 * 3 // 2 and ws(1, 33, 47) % 16 == 0
  assert ws(-1, 4, 4) == -1 and ws(1, 0, 4) == -1 and ws(1, 1 << 15, 1 << 15) == -1
  table = np.zeros((1, 1), augment.OP_DTYPE)
  call = lambda img, B, h, w, n: lib.epos_augment_f32(      # noqa: E731
      img, B, h, w, ctypes.c_void_p(table.ctypes.data), n, None, None)
  assert call(None, 1, 8, 8, 0) == 0 and call(None, 0, 8, 8, 1) == 0      # nothing to do
  assert call(None, 1, 8, 8, 1) == -1 and b'null' in lib.epos_last_error()
  assert call(ctypes.c_void_p(64), 1, 8, 8, 9) == -1 and call(ctypes.c_void_p(64), 1, 0, 8, 1) == -1
  table['kind'] = 8
  assert call(ctypes.c_void_p(64), 1, 8, 8, 1) == -1 and b'kind' in lib.epos_last_error()
