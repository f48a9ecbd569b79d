"""epos_resize_bilinear_dgrad_f32 on the device (csrc/resize_grad.hip), through the C ABI and
through decoder_train.resize_input_grad, against tests/helpers/resize_grad_ref.py: bit for bit,
and within the derived bound of the exact sum. Outputs are pre-filled with a sentinel and framed
by guard words: every element must be written and nothing around them touched."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import resize_grad_ref as ref                          # noqa: E402
from tests.helpers.loss_device import _lib, _p, _stream                   # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = -1                               # EPOS_E_INVALID
SENT32 = 0x7FA55A5A                        # a NaN no kernel produces
GUARD = 8                                  # sentinel words in front of and behind the output

# (B, Hi, Wi, Ho, Wo, C)
SWEEP = [(1, 2, 2, 3, 3, 4), (2, 12, 16, 24, 32, 8), (1, 60, 80, 120, 160, 4),
         (1, 5, 7, 5, 7, 12),              # the identity
         (1, 7, 9, 4, 3, 4),               # downscale: sources without a footprint
         (1, 4, 6, 1, 1, 4), (2, 3, 4, 7, 10, 48),
         (1, 7, 15, 75, 47, 4)]            # fp32 moves samples into the neighbouring cell
IDS = ['x'.join(str(v) for v in c) for c in SWEEP]


def _padded(a, ld):
  """a [rows, width] on the device as rows of stride ld with NaN padding."""
  rows, width = a.shape
  host = np.full((rows, ld), np.nan, np.float32)
  host.view(np.uint32)[:, :width] = np.ascontiguousarray(a).view(np.uint32)
  return torch.from_numpy(host.reshape(-1)).cuda()


def run(grad, hi, wi, mask=None, pads=(0, 0, 0), **over):
  """One call on D = grad [B,Ho,Wo,C] with Y = mask: dX [B,hi,wi,C] as uint32 words after the
  sentinel check, or None when refused (the sentinels then untouched). pads = (ldd - C, ldy - C,
  ldx - C); over: arguments of the C entry to replace."""
  lib = _lib()
  B, ho, wo, C = grad.shape
  ldd, ldy, ldx = C + pads[0], C + pads[1], C + pads[2]
  dD = _padded(grad.reshape(-1, C), ldd)
  dY = _padded(mask.reshape(-1, C), ldy) if mask is not None else None
  rows = B * hi * wi
  buf = torch.full((rows * ldx + 2 * GUARD,), SENT32, dtype=torch.int32, device='cuda')
  out = buf[GUARD:]
  f = dict(D=_p(dD), ldd=ldd, Y=_p(dY), ldy=ldy, dX=_p(out), ldx=ldx, B=B, Hi=hi, Wi=wi, Ho=ho,
           Wo=wo, C=C)
  f.update(over)
  rc = lib.epos_resize_bilinear_dgrad_f32(f['D'], f['ldd'], f['Y'], f['ldy'], f['dX'], f['ldx'],
                                          f['B'], f['Hi'], f['Wi'], f['Ho'], f['Wo'], f['C'],
                                          _stream())
  torch.cuda.synchronize()
  raw = buf.cpu().numpy().view(np.uint32)
  if rc != 0:
    assert rc == INVALID and (raw == SENT32).all(), over
    return None
  body = raw[GUARD:GUARD + rows * ldx].reshape(rows, ldx)
  assert (raw[:GUARD] == SENT32).all() and (raw[GUARD + rows * ldx:] == SENT32).all()
  assert (body[:, C:] == SENT32).all(), 'padding columns written'
  assert not (body[:, :C] == SENT32).any(), 'elements not written'
  return np.ascontiguousarray(body[:, :C]).reshape(B, hi, wi, C)


@functools.lru_cache(maxsize=None)
def problem(case):
  """(D, Y, the restatement's bits without and with the mask, exact sum, sum |w||D|, footprint
  counts) of a sweep case: computed once, shared, never changed."""
  B, hi, wi, ho, wo, C = case
  rng = np.random.RandomState(sum(case))
  D = (rng.randn(B, ho, wo, C) * 1e-2).astype(np.float32)
  D[rng.rand(B, ho, wo, C) < 0.3] = 0.0
  Y = np.maximum(rng.randn(B, hi, wi, C), 0).astype(np.float32)         # behind a ReLU
  Y.reshape(-1)[0] = -0.0
  Y.reshape(-1)[3] = np.nan
  exact, mag, count = ref.resize_dgrad(D, hi, wi, dtype=np.longdouble)
  out = (D, Y, ref.resize_dgrad(D, hi, wi), ref.resize_dgrad(D, hi, wi, Y=Y),
         exact.astype(np.float64), mag.astype(np.float64), count)
  for a in out:
    a.setflags(write=False)
  return out


def test_exact_integer_layout():
  """3x5 -> 5x9: the weights are 0, 1/2 and 1, so small integers stay exact and the result is
  fixed bit for bit whatever the order. D depends on b, y, x and c through a non-symmetric
  expression, so swapping y and x or shifting a footprint changes bytes."""
  B, hi, wi, ho, wo, C = 2, 3, 5, 5, 9, 8
  b, y = np.arange(B)[:, None, None, None], np.arange(ho)[None, :, None, None]
  x, c = np.arange(wo)[None, None, :, None], np.arange(C)[None, None, None, :]
  D = ((b * 3 + y * 2 + x * 5 + c * 7 + (y + 2 * x) % 3) % 13 - 6).astype(np.float32) * 4
  Wy, Wx = ref.axis_matrix(hi, ho), ref.axis_matrix(wi, wo)
  assert set(np.unique(Wy)) | set(np.unique(Wx)) == {0.0, 0.5, 1.0}
  want = np.einsum('oy,bopc,pw->bywc', Wy, D.astype(np.float64), Wx)
  assert np.array_equal(want, np.round(want)) and np.abs(want).max() < 2 ** 20
  got = run(D, hi, wi, pads=(4, 0, 8))
  assert np.array_equal(got.view(np.float32), want.astype(np.float32))
  assert np.array_equal(got, ref.resize_dgrad(D, hi, wi).view(np.uint32))


@pytest.mark.parametrize('case', SWEEP, ids=IDS)
def test_sweep_is_bit_equal_to_the_restatement_and_within_the_bound(case):
  """With and without the mask, in sentinel-filled buffers with padded pitches on every
  operand."""
  B, hi, wi, ho, wo, C = case
  D, Y, bits, bits_masked, exact, mag, count = problem(case)
  got = run(D, hi, wi, pads=(4, 0, 8))
  assert np.array_equal(got, bits.view(np.uint32))
  err = np.abs(got.view(np.float32).astype(np.float64) - exact)
  bound = ref.bound(exact, mag, count)
  print('%s: worst error / bound = %.3g, footprints of %d..%d pixels' % (
      case, float((err / np.maximum(bound, 1e-300)).max()), count.min(), count.max()))
  assert np.all(err <= bound)
  if (hi, wi) == (ho, wo):
    assert np.array_equal(got, D.view(np.uint32))                       # the identity: D's bytes
  if ho < hi:
    assert count.min() == 0 and not got[:, count == 0].any()           # no footprint: +0.0
  got = run(D, hi, wi, mask=Y, pads=(4, 8, 8))
  assert np.array_equal(got, bits_masked.view(np.uint32))
  with np.errstate(invalid='ignore'):
    off = Y <= 0
  assert off.reshape(-1)[0] and not off.reshape(-1)[3]                  # -0.0 masks, a NaN not
  assert not got[off].any()                                            # the BYTES of +0.0
  assert np.array_equal(got[~off], bits.view(np.uint32)[~off])


def test_a_channel_slice_of_a_wider_tensor():
  """D as the [:256] slice of a 304-wide tensor, as trainer.decoder_grads hands it over, through
  the wrapper; the mask and the output slices of wider tensors too."""
  from epos_amd import decoder_train as DT
  B, hi, wi, ho, wo, C = 1, 3, 4, 6, 7, 256
  rng = np.random.RandomState(11)
  wide = rng.randn(B, ho, wo, 304).astype(np.float32)
  Y = rng.randn(B, hi, wi, 260).astype(np.float32)
  d = torch.from_numpy(wide).cuda()
  y = torch.from_numpy(Y).cuda()
  out = torch.full((B, hi, wi, 264), float('nan'), device='cuda')
  got = DT.resize_input_grad(d[..., :C], (hi, wi), relu_of=y[..., :C], out=out[..., :C])
  assert got.data_ptr() == out.data_ptr()
  want = ref.resize_dgrad(wide[..., :C], hi, wi, Y=Y[..., :C])
  host = out.cpu().numpy()
  assert np.array_equal(host[..., :C].view(np.uint32), want.view(np.uint32))
  assert np.isnan(host[..., C:]).all()                                  # the padding is kept
  fresh = DT.resize_input_grad(d[..., :C], (hi, wi))
  assert tuple(fresh.shape) == (B, hi, wi, C) and fresh.is_contiguous()
  assert np.array_equal(fresh.cpu().numpy().view(np.uint32),
                        ref.resize_dgrad(wide[..., :C], hi, wi).view(np.uint32))
  for kwargs, exc in ((dict(relu_of=y[..., :8]), ValueError), (dict(out=out[..., :8]), ValueError),
                      (dict(d=d.double()[..., :C]), TypeError),
                      (dict(d=d.cpu()[..., :C]), DT.EposError),
                      (dict(in_hw=(1, 4)), DT.EposError)):                # the broadcast: refused
    args = dict(d=d[..., :C], in_hw=(hi, wi))
    args.update(kwargs)
    with pytest.raises(exc):
      DT.resize_input_grad(**args)


def test_a_nan_reaches_exactly_the_sources_of_its_taps():
  B, hi, wi, ho, wo, C = 2, 5, 6, 11, 13, 8
  rng = np.random.RandomState(4)
  D = rng.randn(B, ho, wo, C).astype(np.float32)
  base = run(D, hi, wi)
  bad = D.copy()
  where = ((1, 4, 5, 3), (0, 0, 12, 6), (0, 10, 2, 1), (1, 6, 6, 0))
  hit = np.zeros((B, hi, wi, C), bool)
  counts = []
  for (b, yo, xo, c) in where:
    bad[b, yo, xo, c] = np.nan
    src = ref.sources_of(yo, xo, hi, wi, ho, wo)
    counts.append(len(src))
    for yi, xi in src:
      hit[b, yi, xi, c] = True
  assert sorted(counts) == [1, 2, 4, 4]          # a corner, an edge sample on a row, two inside
  got = run(bad, hi, wi)
  assert np.isnan(got.view(np.float32)[hit]).all() and hit.sum() == sum(counts)
  assert np.array_equal(got[~hit], base[~hit])


def test_an_image_does_not_depend_on_its_position_and_runs_agree():
  case = (3, 12, 16, 24, 32, 8)
  rng = np.random.RandomState(6)
  D = rng.randn(3, 24, 32, 8).astype(np.float32)
  Y = rng.randn(3, 12, 16, 8).astype(np.float32)
  got = run(D, 12, 16, mask=Y)
  for b in range(3):
    alone = run(D[b:b + 1], 12, 16, mask=Y[b:b + 1])
    assert np.array_equal(alone[0], got[b]), (case, b)
  assert np.array_equal(got, run(D, 12, 16, mask=Y))                       # the same in every run


def test_a_captured_graph_replays_to_the_eager_bytes():
  from epos_amd import decoder_train as DT
  B, hi, wi, ho, wo, C = 2, 12, 16, 24, 32, 8
  rng = np.random.RandomState(8)
  d = torch.from_numpy(rng.randn(B, ho, wo, C).astype(np.float32)).cuda()
  y = torch.from_numpy(rng.randn(B, hi, wi, C).astype(np.float32)).cuda()
  out = torch.empty((B, hi, wi, C), device='cuda')
  DT.resize_input_grad(d, (hi, wi), relu_of=y, out=out)
  torch.cuda.synchronize()
  eager = out.clone()
  assert np.array_equal(eager.cpu().numpy().view(np.uint32), ref.resize_dgrad(
      d.cpu().numpy(), hi, wi, Y=y.cpu().numpy()).view(np.uint32))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    DT.resize_input_grad(d, (hi, wi), relu_of=y, out=out)
  for _ in range(2):
    out.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))


def test_refusals_leave_the_sentinels():
  lib = _lib()
  rng = np.random.RandomState(1)
  D = rng.randn(1, 5, 7, 8).astype(np.float32)
  Y = rng.randn(1, 3, 4, 8).astype(np.float32)
  positive = b'B, Hi, Wi, Ho, Wo and C must be positive'
  broadcast = b'a source of one row or column broadcasts: its adjoint is a sum, not this entry'
  fake = 1 << 20
  for over, msg in ((dict(D=None), b'null pointer'), (dict(dX=None), b'null pointer'),
                    (dict(B=0), positive), (dict(Hi=0), positive), (dict(Wo=-1), positive),
                    (dict(C=0), positive), (dict(C=6), b'C must be a multiple of 4'),
                    (dict(ldd=4), b'ldd must be >= C and a multiple of 4'),
                    (dict(ldd=10), b'ldd must be >= C and a multiple of 4'),
                    (dict(ldx=6), b'ldx must be >= C and a multiple of 4'),
                    (dict(ldy=9), b'ldy must be >= C and a multiple of 4'),
                    (dict(D=ctypes.c_void_p(fake + 4)), b'D, Y and dX must be 16-byte aligned'),
                    (dict(Y=ctypes.c_void_p(fake + 8)), b'D, Y and dX must be 16-byte aligned'),
                    (dict(Hi=1), broadcast), (dict(Wi=1), broadcast)):
    assert run(D, 3, 4, mask=Y, **over) is None, over
    assert lib.epos_last_error() == b'epos_resize_bilinear_dgrad_f32: ' + msg, over
  d = torch.from_numpy(D).cuda()
  y = torch.from_numpy(Y).cuda()
  for args, msg in (((_p(d), 8, _p(y), 8, _p(d), 8), b'dX may not start at D'),
                    ((_p(d), 8, _p(y), 8, _p(y), 8), b'dX may not start at Y')):
    assert lib.epos_resize_bilinear_dgrad_f32(*args, 1, 3, 4, 5, 7, 8, _stream()) == INVALID
    assert lib.epos_last_error() == b'epos_resize_bilinear_dgrad_f32: ' + msg
  torch.cuda.synchronize()
  assert np.array_equal(d.cpu().numpy(), D) and np.array_equal(y.cpu().numpy(), Y)
  # one source pixel under one output pixel is no broadcast
  got = run(D[:, :1, :1], 1, 1)
  assert np.array_equal(got, D[:, :1, :1].view(np.uint32))
