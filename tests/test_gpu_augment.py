"""csrc/augment.hip on the device against tests/helpers/augment_ref.py: every op alone, JPEG to
the byte, chains, batches with a table per image, determinism and the refusals.

Bounds. JPEG alone: the 0..255 levels are equal (the fixtures are free of rounding ties,
test_augment_host.py). Every other case: |device - reference| <= 2e-3 on the [0,255] scale:
at most about 100 fp32 roundings of values <= 255, each <= 255 * 2^-24 = 1.5e-5. A chain that
ends in JPEG: both sides quantised by the round trip's first step may differ only where the
reference's x * 255.5 lies within 2e-3 of an integer."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import augment_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 2e-3
SHAPES = ['im_24x40', 'im_33x47', 'im_40x56', 'im_96x128']
KEY = (0x12345678, 0x9abcdef0)


@pytest.fixture(scope='module')
def golden():
  g = np.load(os.path.join(ROOT, 'tests', 'golden', 'augment_images.npz'))
  return {k: g[k] for k in g.files}


def fractional(levels, seed=0):
  """The fixture off the integer levels, so that roundings take part: float32 in [0,255]."""
  rng = np.random.RandomState(seed)
  return np.clip(levels.astype(np.float64) + rng.rand(*levels.shape) - 0.5, 0,
                 255).astype(np.float32)


def table(rows, n_ops=None):
  """rows: per image a list of (kind, a[, key_lo, key_hi]) -> EposAugmentOp records."""
  from epos_amd import augment
  n_ops = max(len(r) for r in rows) if n_ops is None else n_ops
  t = np.zeros((len(rows), n_ops), augment.OP_DTYPE)
  for b, row in enumerate(rows):
    for k, op in enumerate(row):
      t[b, k]['kind'], t[b, k]['a'] = op[0], op[1]
      if len(op) > 2:
        t[b, k]['key_lo'], t[b, k]['key_hi'] = op[2], op[3]
  return t


def run(images, t):
  """images f32 [B,h,w,3] (numpy) through the device entry; returns the result as numpy."""
  from epos_amd import augment
  x = torch.from_numpy(np.ascontiguousarray(images, np.float32)).cuda()
  augment.apply_ops(x, t)
  return x.cpu().numpy()


def single_ops(name):
  sigma = 2.9 if name == 'im_24x40' else 1.3      # 24 x 40: R = 12, reflections overlap
  return [('brightness', (R.BRIGHTNESS, 0.15)), ('brightness_down', (R.BRIGHTNESS, -0.6)),
          ('contrast', (R.CONTRAST, 1.4)), ('saturation_up', (R.SATURATION, 1.6)),
          ('saturation_down', (R.SATURATION, 0.3)), ('hue', (R.HUE, 0.3)),
          ('hue_back', (R.HUE, -0.45)), ('blur', (R.BLUR, sigma)),
          ('noise', (R.NOISE, 0.05) + KEY)]


@pytest.mark.parametrize('name', SHAPES)
def test_each_op_alone(golden, name):
  img = fractional(golden[name])
  for label, op in single_ops(name):
    ref = R.apply(img, [op])
    assert np.abs(ref - img).mean() > 1.0, label          # a no-op cannot pass
    dev = run(img[None], table([[op]]))[0]
    err = np.abs(dev - ref).max()
    print('%s %s: max |device - reference| = %.3g' % (name, label, err))
    assert err <= TOL, (label, err)


def test_blur_radius_rule_on_the_device(golden):
  """sigma 0.3 -> 3 taps, 0.6 -> 7: the device takes the radius the helper takes; sigma 0 and
  a ksize of 1 leave the bytes alone."""
  img = fractional(golden['im_24x40'])
  for sigma in (0.3, 0.6, 1.0):
    dev = run(img[None], table([[(R.BLUR, sigma)]]))[0]
    assert np.abs(dev - R.apply(img, [(R.BLUR, sigma)])).max() <= TOL
  for sigma in (0.0, 0.05):
    assert run(img[None], table([[(R.BLUR, sigma)]]))[0].tobytes() == img.tobytes()


@pytest.mark.parametrize('name', SHAPES + ['im_low'])
def test_jpeg_alone_is_exact(golden, name):
  v = golden[name]
  img = v.astype(np.float32)
  for q in (R.LOW_QUALITY,) if name == 'im_low' else R.FIXTURE_QUALITIES:
    want = R.jpeg_levels(v, q)
    assert np.abs(want - v).mean() > 1.0
    dev = run(img[None], table([[(R.JPEG, q)]]))[0]
    assert np.array_equal(np.rint(dev).astype(np.int64), want), (name, q)
    assert np.abs(dev - want).max() <= TOL
    # the round trip behind and in front of another stage: the same levels (x + 0 = x)
    for row in ([(R.BRIGHTNESS, 0.0), (R.JPEG, q)], [(R.JPEG, q), (R.BRIGHTNESS, 0.0)],
                [(R.NONE, 0.0), (R.JPEG, q), (R.NONE, 0.0)]):
      dev = run(img[None], table([row]))[0]
      assert np.array_equal(np.rint(dev).astype(np.int64), want), (name, q, row)


def seven(name, q=87):
  sigma = 2.9 if name == 'im_24x40' else 1.1
  return [(R.BRIGHTNESS, 0.07), (R.CONTRAST, 1.15), (R.SATURATION, 1.2), (R.HUE, -0.015),
          (R.BLUR, sigma), (R.NOISE, 0.04) + KEY, (R.JPEG, q)]


@pytest.mark.parametrize('name', SHAPES)
def test_all_seven_in_the_reference_order(golden, name):
  img = fractional(golden[name], 1)
  ops = seven(name)
  # the six ops in front of the round trip, and every prefix of them
  for n in range(1, 7):
    ref = R.apply(img, ops[:n])
    dev = run(img[None], table([ops[:n]]))[0]
    assert np.abs(dev - ref).max() <= TOL, n
  assert np.abs(ref - img).mean() > 1.0
  # what enters the round trip: quantised by its first step on both sides
  before = []
  full_ref = R.apply(img, ops, levels_before_jpeg=before)
  assert np.abs(full_ref - img).mean() > 1.0
  scaled = before[0]
  near = np.abs(scaled - np.rint(scaled)) <= TOL
  assert near.mean() < 0.01
  dev_levels = R.to_levels(dev.astype(np.float64) / 255.0)
  ref_levels = np.clip(np.floor(scaled), 0, 255).astype(np.int64)
  differ = dev_levels != ref_levels
  print('%s: %d of %d levels differ in front of the round trip, %d lie near an integer' % (
      name, differ.sum(), differ.size, near.sum()))
  assert not (differ & ~near).any()
  assert np.abs(dev_levels - ref_levels).max() <= 1
  # the whole chain: levels come out, the same in every run
  full = run(img[None], table([ops]))[0]
  assert np.abs(full - np.rint(full)).max() <= TOL and full.min() >= 0 and full.max() <= 255
  assert run(img[None], table([ops]))[0].tobytes() == full.tobytes()
  # where no level differed going in, the reference's levels come out
  if not differ.any() and R.jpeg_round_trip(ref_levels, 87)[1].min() >= 1e-6:
    assert np.array_equal(np.rint(full).astype(np.int64), np.rint(full_ref).astype(np.int64))


def test_batch_with_a_table_per_image(golden):
  """B = 3, another table per image, one of them empty; then nine images: two chunks."""
  base = golden['im_33x47']
  imgs = np.stack([fractional(base, s) for s in range(3)])
  rows = [[(R.BLUR, 1.7), (R.NOISE, 0.03) + KEY, (R.NONE, 0.0)],
          [(R.NONE, 0.0)] * 3,
          [(R.CONTRAST, 0.7), (R.HUE, 0.2), (R.BRIGHTNESS, -0.1)]]
  dev = run(imgs, table(rows))
  assert dev[1].tobytes() == imgs[1].tobytes()
  for b in (0, 2):
    ref = R.apply(imgs[b], rows[b])
    assert np.abs(ref - imgs[b]).mean() > 1.0
    assert np.abs(dev[b] - ref).max() <= TOL
    assert run(imgs[b][None], table([rows[b]]))[0].tobytes() == dev[b].tobytes()
  # with the round trip and the contrast sums in the mix
  rows = [seven('im_33x47'), [(R.JPEG, 91), (R.CONTRAST, 1.3)], []]
  dev = run(imgs, table(rows, 7))
  assert dev[2].tobytes() == imgs[2].tobytes()
  for b in (0, 1):
    assert run(imgs[b][None], table([rows[b]], 7))[0].tobytes() == dev[b].tobytes()
  # nine images: the ninth goes into a second chunk of launches
  small = golden['im_24x40']
  nine = np.stack([fractional(small, s) for s in range(9)])
  rows = [seven('im_24x40', 80 + b) if b % 2 else [(R.CONTRAST, 1.0 + 0.05 * b),
                                                  (R.BLUR, 0.5 + 0.2 * b)] for b in range(9)]
  dev = run(nine, table(rows, 7))
  for b in (0, 7, 8):
    assert run(nine[b][None], table([rows[b]], 7))[0].tobytes() == dev[b].tobytes()
  ref = R.apply(nine[8], rows[8])
  assert np.abs(dev[8] - ref).max() <= TOL and np.abs(ref - nine[8]).mean() > 1.0


def test_nothing_to_do_leaves_the_bytes(golden):
  from epos_amd import augment
  img = fractional(golden['im_40x56'])[None]
  assert run(img, np.zeros((1, 0), augment.OP_DTYPE)).tobytes() == img.tobytes()
  assert run(img, table([[(R.NONE, 3.0)] * 8])).tobytes() == img.tobytes()


def test_refusals_write_nothing(golden):
  from epos_amd import augment
  from epos_amd._lib import EposError
  img = fractional(golden['im_24x40'])[None]
  small = np.ascontiguousarray(img[:, :8, :8])
  ok = (R.BRIGHTNESS, 0.1)
  for images, row in ((img, [ok, (R.BLUR, 8.2)]),             # radius 33
                      (small, [ok, (R.BLUR, 2.0)]),           # radius 8 > min(h, w) - 1
                      (img, [ok, (R.BLUR, -1.0)]),
                      (img, [ok, (R.NOISE, -0.1)]),
                      (img, [ok, (R.JPEG, 0)]),
                      (img, [ok, (R.JPEG, 101)]),
                      (img, [ok, (R.JPEG, 80.5)]),
                      (img, [ok, (R.CONTRAST, float('nan'))]),
                      (img, [ok, (8, 1.0)]),
                      (img, [ok, (-1, 1.0)])):
    x = torch.from_numpy(images).cuda()
    with pytest.raises(EposError, match=r'\(-1\)'):
      augment.apply_ops(x, table([row]))
    assert x.cpu().numpy().tobytes() == images.tobytes(), row
  x = torch.from_numpy(img).cuda()
  with pytest.raises(EposError, match=r'\(-1\)'):
    augment.apply_ops(x, table([[ok] * 9]))                   # n_ops = 9
  assert x.cpu().numpy().tobytes() == img.tobytes()
  # radius 7 on 8 x 8 is the largest that fits
  run(small, table([[(R.BLUR, 1.8)]]))


def test_augmenter_applies_the_table_it_reports(golden):
  from epos_amd import augment
  from tests.test_augment_host import SEVEN
  imgs = np.stack([fractional(golden['im_40x56'], s) for s in range(2)])
  aug = augment.Augmenter(SEVEN, seed=11, device='cuda:0')
  x = torch.from_numpy(imgs).cuda()
  assert aug.apply(x, 5) is x
  got = x.cpu().numpy()
  assert got.tobytes() == run(imgs, aug.ops(5, 2)).tobytes()
  assert got[0].tobytes() != got[1].tobytes()
  y = torch.from_numpy(imgs).cuda()
  aug.apply(y, 6)
  assert y.cpu().numpy().tobytes() != got.tobytes()           # another step, another draw
  torch.cuda.synchronize()
