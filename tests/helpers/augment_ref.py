"""The augmentation ops of csrc/augment.hip restated in numpy (include/epos_hip.h,
"Augmentation"): the colour ops, the blur and the noise in fp64, the JPEG round trip with
exact integer steps and an fp64 DCT, and a pure-numpy Philox4x32-10.

An op is (kind, a, key_lo, key_hi) or an EposAugmentOp record; apply(image, ops) takes one
image [h,w,3] with values in [0,255] and returns the fp64 result on the same scale.
"""
import numpy as np

NONE, BRIGHTNESS, CONTRAST, SATURATION, HUE, BLUR, NOISE, JPEG = range(8)

M32 = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
  """counter: uint32 [..., 4], key: uint32 [..., 2] (broadcast) -> uint32 [..., 4]."""
  c0, c1, c2, c3 = (np.asarray(counter, np.uint64)[..., i] for i in range(4))
  k0, k1 = (np.asarray(key, np.uint64)[..., i] for i in range(2))
  for _ in range(10):
    p0 = np.uint64(0xD2511F53) * c0
    p1 = np.uint64(0xCD9E8D57) * c2
    c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, \
        p0 & M32
    k0 = (k0 + np.uint64(0x9E3779B9)) & M32
    k1 = (k1 + np.uint64(0xBB67AE85)) & M32
  return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def normals(n, key_lo, key_hi):
  """z(0..n-1): value i takes its number from counter (i // 4, 0, 0, 0)."""
  nj = (n + 3) // 4
  ctr = np.zeros((nj, 4), np.uint64)
  ctr[:, 0] = np.arange(nj)
  r = philox4x32_10(ctr, np.array([key_lo, key_hi], np.uint64)).astype(np.float64)
  z = np.empty((nj, 4))
  for k in (0, 2):
    u1 = (np.floor(r[:, k] / 256.0) + 0.5) * 2.0 ** -24
    u2 = np.floor(r[:, k + 1] / 256.0) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    z[:, k] = rad * np.cos(2.0 * np.pi * u2)
    z[:, k + 1] = rad * np.sin(2.0 * np.pi * u2)
  return z.reshape(-1)[:n]


def rgb_to_hsv(rgb):
  r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
  mx, mn = rgb.max(-1), rgb.min(-1)
  d = mx - mn
  safe = np.where(d == 0, 1.0, d)
  s = np.where(mx > 0, d / np.where(mx > 0, mx, 1.0), 0.0)
  t = np.where(mx == r, (g - b) / safe, np.where(mx == g, (b - r) / safe + 2.0,
                                                 (r - g) / safe + 4.0))
  h = np.where(d == 0, 0.0, np.mod(t / 6.0, 1.0))
  return np.stack([h, s, mx], -1)


def hsv_to_rgb(hsv):
  h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
  fi = np.floor(h * 6.0)
  f = h * 6.0 - fi
  i = fi.astype(np.int64) % 6
  p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
  r = np.choose(i, [v, q, p, p, t, v])
  g = np.choose(i, [t, v, v, q, p, p])
  b = np.choose(i, [p, p, t, v, v, q])
  return np.stack([r, g, b], -1)


def blur_ksize(sigma):
  return int(round(float(np.float32(sigma)) * 8.0 + 1.0)) | 1


def blur_weights(sigma):
  """The 2R+1 weights as fp32 values (held in fp64)."""
  sigma = float(np.float32(sigma))
  R = (blur_ksize(sigma) - 1) // 2
  i = np.arange(-R, R + 1, dtype=np.float64)
  e = np.exp(-i * i / (2.0 * sigma * sigma))
  return (e / e.sum()).astype(np.float32).astype(np.float64)


def blur(x, sigma):
  if float(sigma) == 0.0 or blur_ksize(sigma) == 1:
    return x
  w = blur_weights(sigma)
  R = len(w) // 2
  for axis in (1, 0):                       # rows (along x) first, then columns
    n = x.shape[axis]
    idx = np.arange(-R, n + R)
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)
    padded = np.take(x, idx, axis=axis)
    out = np.zeros_like(x)
    for k in range(2 * R + 1):
      out += w[k] * np.take(padded, np.arange(k, k + n), axis=axis)
    x = out
  return x


LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
CHROMA = np.full((8, 8), 99, np.int64)
CHROMA[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]


def _fix(c):
  return int(np.floor(c * 65536 + 0.5))


def dct_matrix():
  u, x = np.arange(8)[:, None], np.arange(8)[None, :]
  return 0.5 * np.where(u == 0, np.sqrt(0.5), 1.0) * np.cos((2 * x + 1) * u * np.pi / 16.0)


def quant_table(base, quality):
  scale = 5000 // quality if quality < 50 else 200 - 2 * quality
  return np.clip((base * scale + 50) // 100, 1, 255)


def _blocks(plane):
  H, W = plane.shape
  return plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(blocks):
  nh, nw = blocks.shape[:2]
  return blocks.transpose(0, 2, 1, 3).reshape(nh * 8, nw * 8)


def _code_plane(plane, table):
  """DCT, quantise, dequantise, inverse DCT of an integer plane (sizes multiples of 8).
  Returns the plane and, per 8x8 block, the smallest distance of a value from a rounding tie
  in front of the two roundings (the quantisation and the inverse DCT's)."""
  T = dct_matrix()
  f = _blocks(plane.astype(np.float64) - 128.0)
  F = np.einsum('uy,abyx,vx->abuv', T, f, T)
  pre = np.abs(F) / table + 0.5
  tie = np.abs(pre - np.rint(pre)).min((2, 3))
  D = np.sign(F) * np.floor(pre) * table
  back = np.einsum('uy,abuv,vx->abyx', T, D, T) + 128.0
  tie = np.minimum(tie, np.abs(back - np.floor(back) - 0.5).min((2, 3)))
  return _unblocks(np.clip(np.rint(back), 0, 255).astype(np.int64)), tie


def _fancy_upsample(c, h, w):
  """IJG h2v2 'fancy' upsampling of the ceil(h/2) x ceil(w/2) samples of c to h x w."""
  ch, cw = (h + 1) // 2, (w + 1) // 2
  c = c[:ch, :cw]
  up, down = np.vstack([c[:1], c[:-1]]), np.vstack([c[1:], c[-1:]])
  rows = np.empty((2 * ch, cw), np.int64)
  rows[0::2] = 3 * c + up
  rows[1::2] = 3 * c + down
  out = np.empty((2 * ch, 2 * cw), np.int64)
  last = np.hstack([rows[:, :1], rows[:, :-1]])
  nxt = np.hstack([rows[:, 1:], rows[:, -1:]])
  out[:, 0::2] = (3 * rows + last + 8) >> 4
  out[:, 1::2] = (3 * rows + nxt + 7) >> 4
  out[:, 0] = (4 * rows[:, 0] + 8) >> 4
  out[:, 2 * cw - 1] = (4 * rows[:, -1] + 7) >> 4
  return out[:h, :w]


def jpeg_levels(v, quality, with_ties=False):
  """v: integer levels [h,w,3] in 0..255 -> the levels after the round trip (int64). With
  with_ties also the smallest distance of a pre-rounding value (quantisation, inverse DCT)
  from a rounding tie."""
  out, ties = jpeg_round_trip(v, quality)
  return (out, float(ties.min())) if with_ties else out


def tie_free(v, qualities, min_dist=1e-6, seed=0, max_rounds=2000):
  """v with single levels nudged until no rounding of the round trip at any of `qualities`
  lies within min_dist of a tie. A block's DC and its (0,4), (4,0), (4,4) coefficients are
  multiples of 1/8, so random levels DO hit exact ties, where the order of a sum decides."""
  v = np.array(v, np.int64)
  h, w = v.shape[:2]
  rng = np.random.RandomState(seed)
  for rnd in range(max_rounds):
    amp = 3 + rnd // 10       # coarse tables need larger steps before a coefficient moves
    bad = np.zeros((-(-h // 16), -(-w // 16)), bool)
    for q in qualities:
      bad |= jpeg_round_trip(v, q)[1] < min_dist
    if not bad.any():
      return v
    for my, mx in zip(*np.nonzero(bad)):
      y = min(my * 16 + rng.randint(16), h - 1)
      x = min(mx * 16 + rng.randint(16), w - 1)
      c = rng.randint(3)
      v[y, x, c] = np.clip(v[y, x, c] + rng.randint(1, amp + 1) * rng.choice([-1, 1]), 0, 255)
  raise RuntimeError('no tie-free image found')


FIXTURE_QUALITIES = (80, 90, 99)
LOW_QUALITY = 30          # the other branch of the quality scaling; 'im_low' is free of ties there
FIXTURE_SHAPES = ((24, 40), (33, 47), (40, 56), (96, 128))


def gradient_noise(h, w, seed):
  """A colour gradient plus noise, integer levels [h,w,3]."""
  rng = np.random.RandomState(seed)
  yy, xx = np.mgrid[0:h, 0:w]
  base = np.stack([40 + 150.0 * xx / w, 200 - 120.0 * yy / h,
                   60 + 60.0 * (xx + yy) / (h + w)], -1)
  return np.clip(np.rint(base + rng.normal(0, 16, (h, w, 3))), 0, 255).astype(np.int64)


def make_fixtures():
  """What tests/golden/augment_images.npz holds: gradient_noise(h, w, h) made tie-free at
  FIXTURE_QUALITIES, uint8, under 'im_<h>x<w>'; 'im_low': 40 x 56, tie-free at LOW_QUALITY."""
  out = {'im_%dx%d' % (h, w): tie_free(gradient_noise(h, w, h), FIXTURE_QUALITIES).astype(
      np.uint8) for h, w in FIXTURE_SHAPES}
  out['im_low'] = tie_free(gradient_noise(40, 56, 7), (LOW_QUALITY,)).astype(np.uint8)
  return out


def jpeg_round_trip(v, quality):
  """(levels after the round trip [h,w,3], tie distance per 16x16 MCU)."""
  v = np.asarray(v, np.int64)
  h, w = v.shape[:2]
  R, G, B = v[..., 0], v[..., 1], v[..., 2]
  Y = (_fix(.299) * R + _fix(.587) * G + _fix(.114) * B + 32768) >> 16
  Cb = (-_fix(.16874) * R - _fix(.33126) * G + _fix(.5) * B + (128 << 16) + 32767) >> 16
  Cr = (_fix(.5) * R - _fix(.41869) * G - _fix(.08131) * B + (128 << 16) + 32767) >> 16
  H16, W16 = -(-h // 16) * 16, -(-w // 16) * 16
  Y = np.pad(Y, ((0, H16 - h), (0, W16 - w)), mode='edge')
  bias = np.tile(np.array([1, 2], np.int64), W16 // 4)[None, :]

  def down(p):
    # pixels replicated to W16 columns and to an even number of rows, 2x2 means, then the
    # last chroma ROW replicated to H16 / 2 (as libjpeg pads: PIL decided this)
    p = np.pad(p, ((0, h % 2), (0, W16 - w)), mode='edge')
    d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return np.pad(d, ((0, H16 // 2 - d.shape[0]), (0, 0)), mode='edge')
  Y2, tie_y = _code_plane(Y, quant_table(LUMA, quality))
  qc = quant_table(CHROMA, quality)
  Cb2, tie_cb = _code_plane(down(Cb), qc)
  Cr2, tie_cr = _code_plane(down(Cr), qc)
  ties = np.minimum(np.minimum(tie_cb, tie_cr),
                    tie_y.reshape(H16 // 16, 2, W16 // 16, 2).min((1, 3)))
  Yc = Y2[:h, :w]
  cb, cr = _fancy_upsample(Cb2, h, w) - 128, _fancy_upsample(Cr2, h, w) - 128
  out = np.stack([Yc + ((_fix(1.402) * cr + 32768) >> 16),
                  Yc + ((-_fix(.34414) * cb - _fix(.71414) * cr + 32768) >> 16),
                  Yc + ((_fix(1.772) * cb + 32768) >> 16)], -1)
  return np.clip(out, 0, 255), ties


def to_levels(x):
  """Step 1 on x in [0,1]: v = min(255, floor(x * 255.5)), in fp32 as the device takes it."""
  x32 = np.asarray(x, np.float64).astype(np.float32)
  return np.clip(np.floor(x32 * np.float32(255.5)), 0, 255).astype(np.int64)


def _fields(op):
  if isinstance(op, np.void):
    return int(op['kind']), float(op['a']), int(op['key_lo']), int(op['key_hi'])
  kind, a = op[0], op[1]
  key = tuple(op[2:4]) if len(op) >= 4 else (0, 0)
  return int(kind), float(np.float32(a)), int(key[0]), int(key[1])


def apply(image, ops, levels_before_jpeg=None):
  """One image [h,w,3] in [0,255] through ops, fp64. An image without an effective op comes
  back unchanged. levels_before_jpeg: a list that receives x * 255.5 (fp64) in front of every
  JPEG op (what decides step 1)."""
  ops = [_fields(op) for op in ops]
  ops = [op for op in ops if op[0] != NONE and not (
      op[0] == BLUR and (op[1] == 0.0 or blur_ksize(op[1]) == 1))]
  img = np.asarray(image, np.float64)
  if not ops:
    return img.copy()
  x = np.asarray(image, np.float32).astype(np.float64) / 255.0
  for kind, a, key_lo, key_hi in ops:
    if kind == BRIGHTNESS:
      x = np.clip(x + a, 0.0, 1.0)
    elif kind == CONTRAST:
      m = x.reshape(-1, 3).mean(0)
      x = np.clip((x - m) * a + m, 0.0, 1.0)
    elif kind == SATURATION:
      hsv = rgb_to_hsv(x)
      hsv[..., 1] = np.clip(hsv[..., 1] * a, 0.0, 1.0)
      x = np.clip(hsv_to_rgb(hsv), 0.0, 1.0)
    elif kind == HUE:
      hsv = rgb_to_hsv(x)
      hsv[..., 0] = np.mod(hsv[..., 0] + a, 1.0)
      hsv[..., 0] = np.where(hsv[..., 0] >= 1.0, 0.0, hsv[..., 0])
      x = np.clip(hsv_to_rgb(hsv), 0.0, 1.0)
    elif kind == BLUR:
      x = blur(x, a)
    elif kind == NOISE:
      x = np.clip(x + a * normals(x.size, key_lo, key_hi).reshape(x.shape), 0.0, 1.0)
    elif kind == JPEG:
      if levels_before_jpeg is not None:
        levels_before_jpeg.append(x * 255.5)
      x = jpeg_levels(to_levels(x), int(a)).astype(np.float32) / np.float32(255.0)
      x = x.astype(np.float64)
    else:
      raise ValueError('unknown op kind %r' % (kind,))
  return x * 255.0
