"""The bf16-mode kernels (csrc/bf16.hip, csrc/glue.hip) on the GPU against float64 numpy restatements on the
bf16-rounded operands: the grouped GEMM (every epilogue, sub = 2, column offsets, K / M / N
tails at the plans' layer shapes, fp32 and bf16 outputs), the depthwise 3x3, the im2col, and the
glue layers. Padding columns of A hold NaN and must not reach the output; sentinels behind C
must survive."""
import ctypes

import numpy as np
import pytest
import torch

from helpers.bf16_ref import bf16_round, bf16_round_bits, bf16_to_f32
from helpers.glue_ref import resize_f32

pytestmark = pytest.mark.gpu

SENT = 0x7FC1          # a NaN pattern in bf16, never produced by the kernels' arithmetic


def _lib():
  from epos_amd import _lib as L
  return L, L.load()


def _p(t, off=0):
  return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _bf16_dev(x_f32):
  """fp32 numpy -> (device bf16 tensor, its values as fp64)"""
  bits = bf16_round_bits(x_f32)
  t = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).cuda()
  return t, bf16_to_f32(bits).astype(np.float64)


def _half_ulp(x):
  """half a bf16 ulp of |x| (0 at 0): 2^(floor(log2|x|) - 8)"""
  x = np.abs(x)
  return np.where(x > 0, np.ldexp(1.0, np.frexp(x)[1] - 9), 0.0)


def _pack(lib, w):
  k, n = w.shape
  total = lib.epos_pack_pointwise_weights_bf16(None, k, n, None)
  dst = np.empty(total, np.uint16)
  w = np.ascontiguousarray(w, np.float32)
  lib.epos_pack_pointwise_weights_bf16(w.ctypes.data_as(ctypes.c_void_p), k, n,
                                       dst.ctypes.data_as(ctypes.c_void_p))
  return torch.from_numpy(dst.view(np.int16)).cuda()


def _problem(L, lib, rng, M, N, K, lda, ldc, c_off, out_f32, bias=True, res=False, relu=False,
             sub=1, geo=None):
  """One GEMM problem: device buffers, launch args and the fp64 expectation + bound."""
  rows = M if sub == 1 else geo[0] * geo[3] * geo[4]
  a = rng.standard_normal((rows, lda)).astype(np.float32)
  a[:, K:] = np.nan                                  # padding columns: never read
  a_dev, a64 = _bf16_dev(a)
  w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
  wq = bf16_round(w).astype(np.float64)
  wp = _pack(lib, w)
  b = rng.standard_normal(N).astype(np.float32) if bias else None
  b_dev = torch.from_numpy(b).cuda() if bias else None
  if sub == 1:
    arows = a64[:M, :K]
  else:
    B_, Ho, Wo, Hi, Wi = geo
    idx = np.array([(bb * Hi + y * sub) * Wi + x * sub for bb in range(B_)
                    for y in range(Ho) for x in range(Wo)])
    arows = a64[idx, :K]
  r_dev, r64, ldr = None, None, 0
  if res:
    ldr = N + 8
    r = rng.standard_normal((M, ldr)).astype(np.float32)
    r_dev, r64 = _bf16_dev(r)
    r64 = r64[:, :N]
  dt = torch.float32 if out_f32 else torch.bfloat16
  c = torch.empty((M + 1) * ldc, dtype=dt).cuda()
  c.view(torch.int16 if not out_f32 else torch.int32).fill_(SENT if not out_f32 else 0x7FC00001)
  exact = arows @ wq
  mag = np.abs(arows) @ np.abs(wq)
  if bias:
    exact = exact + b.astype(np.float64)
    mag = mag + np.abs(b.astype(np.float64))
  if res:
    exact = exact + r64
    mag = mag + np.abs(r64)
  if relu:
    exact = np.maximum(exact, 0.0)
  args = L.PointwiseBf16Args(
      A=_p(a_dev), lda=lda, Wp=_p(wp), bias=_p(b_dev) if bias else None,
      R=_p(r_dev) if res else None, ldr=ldr, C=_p(c, c_off), ldc=ldc, M=M, N=N, K=K,
      relu=int(relu), sub=sub, Ho=geo[1] if geo else 0, Wo=geo[2] if geo else 0,
      Hi=geo[3] if geo else 0, Wi=geo[4] if geo else 0, c_f32=int(out_f32), c_stream=0)
  keep = (a_dev, wp, b_dev, r_dev)
  return dict(args=args, c=c, exact=exact, mag=mag, M=M, N=N, ldc=ldc, c_off=c_off,
              f32=out_f32, keep=keep)


def _check(pb):
  c = pb['c']
  M, N, ldc, off = pb['M'], pb['N'], pb['ldc'], pb['c_off']
  if pb['f32']:
    raw = c.view(torch.int32).cpu().numpy().reshape(-1)
    got = c.cpu().numpy().reshape(-1)
    sent = 0x7FC00001
  else:
    raw = c.view(torch.int16).cpu().numpy().reshape(-1).astype(np.int64) & 0xffff
    got = c.float().cpu().numpy().reshape(-1)
    sent = SENT
  body = got[:M * ldc].reshape(M, ldc)[:, off:off + N].astype(np.float64)
  bound = 2.0 ** -18 * pb['mag']
  if not pb['f32']:
    bound = bound + _half_ulp(pb['exact'])
  err = np.abs(body - pb['exact'])
  assert np.isfinite(body).all(), 'NaN / inf reached the output'
  assert (err <= bound).all(), (err.max(), (err - bound).max())
  # everything outside [M) x [off, off + N) keeps its sentinel
  mask = np.ones(raw.size, bool)
  for m in range(M):
    mask[m * ldc + off:m * ldc + off + N] = False
  assert (raw[mask] == sent).all(), 'a write outside C'


def _run(L, lib, probs):
  arr = (L.PointwiseBf16Args * len(probs))(*[p['args'] for p in probs])
  L.check(lib.epos_pointwise_conv_bf16(arr, len(probs), None), 'gemm bf16')
  torch.cuda.synchronize()


# (M, N, K, lda) at the plans' real layer shapes (reduced M): the stem's 27 columns padded to
# 32, the 7x7 root's 147 -> 152, 64, 288 (conv1_2 im2col), 304 (decoder), 728, 1280 (ASPP
# concat), 2048, 4608 (ResNet block4 3x3 im2col)
SHAPES = [(300, 32, 32, 32), (333, 64, 152, 152), (257, 128, 64, 64), (200, 64, 288, 288),
          (190, 256, 304, 304), (129, 728, 728, 768), (160, 256, 1280, 1280),
          (97, 256, 2048, 2048), (70, 512, 4608, 4608), (64, 48, 256, 256)]


@pytest.mark.parametrize('out_f32', [False, True])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_gemm_shapes(shape, out_f32):
  L, lib = _lib()
  M, N, K, lda = shape
  rng = np.random.default_rng(M * 7 + K)
  pb = _problem(L, lib, rng, M, N, K, lda, N + 16, 0, out_f32, relu=True)
  _run(L, lib, [pb])
  _check(pb)


EPI = [(b, r, relu) for b in (False, True) for r in (False, True) for relu in (False, True)]


@pytest.mark.parametrize('out_f32', [False, True])
@pytest.mark.parametrize('epi', EPI, ids=['b%dr%du%d' % e for e in EPI])
def test_gemm_epilogues(epi, out_f32):
  L, lib = _lib()
  bias, res, relu = epi
  rng = np.random.default_rng(hash(epi) % 1000)
  # N tail (N = 22, 37: scalar epilogue), a column offset into a wider ldc
  for (M, N, K, ldc, off) in [(150, 96, 40, 96, 0), (131, 22, 56, 22, 0), (77, 37, 24, 64, 5),
                              (100, 48, 64, 304, 256)]:
    pb = _problem(L, lib, rng, M, N, K, (K + 15) // 8 * 8, ldc, off, out_f32, bias=bias,
                  res=res, relu=relu)
    _run(L, lib, [pb])
    _check(pb)


def test_gemm_sub2():
  L, lib = _lib()
  rng = np.random.default_rng(5)
  for B_, Hi, Wi, K, N in [(2, 13, 17, 64, 128), (1, 30, 40, 728, 728)]:
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    pb = _problem(L, lib, rng, B_ * Ho * Wo, N, K, (K + 63) // 64 * 64, N, 0, False,
                  sub=2, geo=(B_, Ho, Wo, Hi, Wi))
    _run(L, lib, [pb])
    _check(pb)


def test_gemm_grouped_mixed_and_deterministic():
  L, lib = _lib()
  rng = np.random.default_rng(9)
  probs = [_problem(L, lib, rng, 300, 256, 64, 64, 1280, 256, False, relu=True),
           _problem(L, lib, rng, 300, 256, 728, 768, 1280, 512, False, relu=True),
           _problem(L, lib, rng, 45, 22, 256, 256, 22, 0, True),
           _problem(L, lib, rng, 77, 1344, 256, 256, 1344, 0, True),
           _problem(L, lib, rng, 128, 64, 8, 8, 64, 0, False, res=True)]
  # problems 0 and 1 write disjoint column slices of their own buffers
  _run(L, lib, probs)
  for pb in probs:
    _check(pb)
  first = [pb['c'].clone() for pb in probs]
  _run(L, lib, probs)
  for pb, f in zip(probs, first):
    assert torch.equal(pb['c'].view(torch.int16), f.view(torch.int16))


def test_gemm_head_size_c2():
  """the frag-loc head at C2 size (120 x 160 pixels, 21 objects, 64 fragments), fp32 out with
  streaming stores"""
  L, lib = _lib()
  rng = np.random.default_rng(11)
  pb = _problem(L, lib, rng, 19200, 4032, 256, 256, 4032, 0, True)
  pb['args'].c_stream = 1
  _run(L, lib, [pb])
  _check(pb)


def test_gemm_rejects_bad_args():
  L, lib = _lib()
  rng = np.random.default_rng(1)
  pb = _problem(L, lib, rng, 64, 64, 64, 64, 64, 0, False)
  bad = L.PointwiseBf16Args.from_buffer_copy(pb['args'])
  bad.K = 60
  assert lib.epos_pointwise_conv_bf16(ctypes.byref(bad), 1, None) < 0
  bad = L.PointwiseBf16Args.from_buffer_copy(pb['args'])
  bad.lda = 36
  assert lib.epos_pointwise_conv_bf16(ctypes.byref(bad), 1, None) < 0
  assert lib.epos_pointwise_conv_bf16(ctypes.byref(pb['args']), 9, None) < 0


# ---------------------------------------------------------------- depthwise ---
def _dw_ref(x, w9c, bias, stride, rate, relu_in, relu_out):
  B, Hi, Wi, C = x.shape
  xs = np.maximum(x, 0) if relu_in else x
  pad = rate
  Ho = Hi if stride == 1 else (Hi - 1) // 2 + 1
  Wo = Wi if stride == 1 else (Wi - 1) // 2 + 1
  xp = np.zeros((B, Hi + 2 * pad + 2, Wi + 2 * pad + 2, C))
  xp[:, pad:pad + Hi, pad:pad + Wi] = xs
  y = np.zeros((B, Ho, Wo, C)) + bias
  mag = np.zeros((B, Ho, Wo, C)) + np.abs(bias)
  for ky in range(3):
    for kx in range(3):
      tap = xp[:, ky * rate:ky * rate + (Ho - 1) * stride + 1:stride,
               kx * rate:kx * rate + (Wo - 1) * stride + 1:stride]
      y = y + tap * w9c[ky * 3 + kx]
      mag = mag + np.abs(tap * w9c[ky * 3 + kx])
  if relu_out:
    y = np.maximum(y, 0)
  return y, mag


DW = [(1, 1, 64, False, True), (2, 1, 128, True, False), (1, 2, 728, False, False),
      (1, 4, 728, True, True), (2, 1, 728, False, True), (1, 12, 2048, False, True),
      (1, 1, 304, False, True), (1, 24, 256, False, True), (2, 1, 256, True, True)]


@pytest.mark.parametrize('case', DW, ids=['s%dr%dc%d_%d%d' % c for c in DW])
def test_depthwise(case):
  L, lib = _lib()
  stride, rate, C, relu_in, relu_out = case
  B, Hi, Wi = 2, 19, 27
  ld = (C + 63) // 64 * 64 if C >= 256 else C
  rng = np.random.default_rng(C + rate)
  x = rng.standard_normal((B, Hi, Wi, ld)).astype(np.float32)
  x[..., C:] = np.nan
  x_dev, x64 = _bf16_dev(x)
  w9c = rng.standard_normal((9, C)).astype(np.float32) * 0.3
  bias = rng.standard_normal(C).astype(np.float32)
  Ho = Hi if stride == 1 else (Hi - 1) // 2 + 1
  Wo = Wi if stride == 1 else (Wi - 1) // 2 + 1
  y = torch.empty(B * Ho * Wo * ld, dtype=torch.bfloat16).cuda()
  y.view(torch.int16).fill_(SENT)
  wd, bd = torch.from_numpy(w9c).cuda(), torch.from_numpy(bias).cuda()
  args = L.DepthwiseBf16Args(X=_p(x_dev), ldx=ld, w9c=_p(wd), bias=_p(bd), Y=_p(y), ldy=ld,
                             B=B, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, C=C, stride=stride, rate=rate,
                             relu_in=int(relu_in), relu_out=int(relu_out))
  L.check(lib.epos_depthwise3x3_bf16(ctypes.byref(args), None), 'dw')
  torch.cuda.synchronize()
  want, mag = _dw_ref(x64[..., :C], w9c.astype(np.float64), bias.astype(np.float64), stride,
                      rate, relu_in, relu_out)
  got = y.float().cpu().numpy().reshape(B, Ho, Wo, ld)
  raw = y.view(torch.int16).cpu().numpy().reshape(B, Ho, Wo, ld).astype(np.int64) & 0xffff
  assert (raw[..., C:] == SENT).all()
  err = np.abs(got[..., :C] - want)
  bound = 2.0 ** -18 * mag + _half_ulp(want)
  assert np.isfinite(got[..., :C]).all()
  assert (err <= bound).all(), err.max()


# ------------------------------------------------------------------- im2col ---
@pytest.mark.parametrize('src,mode', [('f32', 0), ('f32', 1), ('f32', 2), ('bf16', 0)])
def test_im2col(src, mode):
  L, lib = _lib()
  rng = np.random.default_rng(mode)
  cases = [(3, 7, 2, 1, 3), (3, 3, 2, 1, 1)] if src == 'f32' else \
          [(64, 3, 1, 2, 2), (32, 3, 1, 1, 1), (64, 3, 2, 1, 1), (5, 3, 1, 1, 1)]
  for C, k, stride, rate, pad in cases:
    B, Hi, Wi = 2, 15, 22
    Ho, Wo = (Hi + 2 * pad - rate * (k - 1) - 1) // stride + 1, \
        (Wi + 2 * pad - rate * (k - 1) - 1) // stride + 1
    ldcol = (k * k * C + 7) // 8 * 8 + 8
    x = (rng.random((B, Hi, Wi, C)) * 255).astype(np.float32)
    if src == 'bf16':
      x_dev, x64 = _bf16_dev(x)
    else:
      x_dev, x64 = torch.from_numpy(x).cuda(), x.astype(np.float64)
    col = torch.empty(B * Ho * Wo * ldcol, dtype=torch.bfloat16).cuda()
    col.view(torch.int16).fill_(SENT)
    mean = np.array([123.15, 115.90, 103.06], np.float32)
    args = L.Im2colBf16Args(X=_p(x_dev), ldx=C, x_bf16=int(src == 'bf16'), col=_p(col),
                            ldcol=ldcol, B=B, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, C=C, k=k,
                            stride=stride, rate=rate, pad=pad, preprocess=mode,
                            mean_rgb=(ctypes.c_float * 3)(*mean))
    L.check(lib.epos_im2col_bf16(ctypes.byref(args), None), 'im2col')
    torch.cuda.synchronize()
    # expectation: the fp32 preprocessing of the kernel (same fp32 operations), then RNE
    xs = x.copy()
    if mode == 1:
      xs = np.float32(2.0 / 255.0) * xs - np.float32(1.0)
    elif mode == 2:
      xs = xs - mean[:C]
    if src == 'bf16':
      xs = x64.astype(np.float32)
    want = np.zeros((B, Ho, Wo, ldcol), np.float32)
    for ky in range(k):
      for kx in range(k):
        for yo in range(Ho):
          yi = yo * stride - pad + ky * rate
          if not 0 <= yi < Hi:
            continue
          for xo in range(Wo):
            xi = xo * stride - pad + kx * rate
            if 0 <= xi < Wi:
              want[:, yo, xo, (ky * k + kx) * C:(ky * k + kx + 1) * C] = xs[:, yi, xi]
    got = col.view(torch.int16).cpu().numpy().reshape(B, Ho, Wo, ldcol)
    np.testing.assert_array_equal(got.view(np.uint16), bf16_round_bits(want))
  if src == 'bf16':
    args.preprocess = 1
    assert lib.epos_im2col_bf16(ctypes.byref(args), None) < 0


# ------------------------------------------------------------- glue layers ---
def test_maxpool_subsample_add_relu_exact():
  L, lib = _lib()
  rng = np.random.default_rng(3)
  B, Hi, Wi, C = 2, 25, 31, 64
  x = rng.standard_normal((B, Hi, Wi, C)).astype(np.float32)
  x_dev, x64 = _bf16_dev(x)
  Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
  y = torch.empty(B * Ho * Wo * C, dtype=torch.bfloat16).cuda()
  L.check(lib.epos_maxpool3x3_s2_bf16(_p(x_dev), C, _p(y), C, B, Hi, Wi, C, None), 'maxpool')
  ty, tx = (Ho - 1) * 2 + 3 - Hi, (Wo - 1) * 2 + 3 - Wi
  py, px = max(ty, 0) // 2, max(tx, 0) // 2
  xp = np.full((B, Hi + 4, Wi + 4, C), -np.inf)
  xp[:, py:py + Hi, px:px + Wi] = x64
  want = np.full((B, Ho, Wo, C), -np.inf)
  for ky in range(3):
    for kx in range(3):
      want = np.maximum(want, xp[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2])
  np.testing.assert_array_equal(y.float().cpu().numpy().reshape(B, Ho, Wo, C), want)
  # subsample by 2
  s = torch.empty(B * Ho * Wo * C, dtype=torch.bfloat16).cuda()
  L.check(lib.epos_subsample_bf16(_p(x_dev), C, _p(s), C, B, Hi, Wi, C, 2, None), 'sub')
  np.testing.assert_array_equal(s.float().cpu().numpy().reshape(B, Ho, Wo, C),
                                x64[:, ::2, ::2])
  # add + relu: one RNE of the fp32 sum
  z = rng.standard_normal(x.shape).astype(np.float32)
  z_dev, z64 = _bf16_dev(z)
  o = torch.empty_like(x_dev)
  L.check(lib.epos_add_relu_bf16(_p(x_dev), _p(z_dev), _p(o), x.size, None), 'add_relu')
  torch.cuda.synchronize()
  want = bf16_round_bits(np.maximum((x64 + z64).astype(np.float32), 0))
  got = o.view(torch.int16).cpu().numpy().view(np.uint16)
  np.testing.assert_array_equal(got.reshape(want.shape), want)


@pytest.mark.parametrize('src_f32', [False, True])
def test_resize_and_mean(src_f32):
  L, lib = _lib()
  rng = np.random.default_rng(4)
  B, C = 2, 256
  Hi, Wi, Ho, Wo = (1, 1, 9, 13) if src_f32 else (15, 20, 59, 79)
  x = rng.standard_normal((B, Hi, Wi, C)).astype(np.float32)
  if src_f32:
    x_dev, x32 = torch.from_numpy(x).cuda(), x
  else:
    x_dev, x64 = _bf16_dev(x)
    x32 = x64.astype(np.float32)
  ldy = 304
  y = torch.empty(B * Ho * Wo * ldy, dtype=torch.bfloat16).cuda()
  y.view(torch.int16).fill_(SENT)
  L.check(lib.epos_resize_bilinear_bf16(_p(x_dev), C, int(src_f32), _p(y), ldy, B, Hi, Wi, Ho,
                                        Wo, C, None), 'resize')
  torch.cuda.synchronize()
  # the fp32 kernel's arithmetic restated in numpy float32 (tests/helpers/glue_ref.py)
  want, (tl, tr, bl, br) = resize_f32(x32, Ho, Wo)
  raw = y.view(torch.int16).cpu().numpy().view(np.uint16).reshape(B, Ho, Wo, ldy)
  got = bf16_to_f32(raw[..., :C]).astype(np.float64)
  # the kernel's fp32 arithmetic in numpy's float32, then one RNE: half a bf16 ulp, plus a few
  # fp32 roundings of the corner values where the interpolation cancels
  mag = np.abs(tl) + np.abs(tr) + np.abs(bl) + np.abs(br)
  assert (np.abs(got - want) <= _half_ulp(want) + 2.0 ** -21 * mag).all()
  assert (raw[..., C:] == SENT).all()
  if not src_f32:
    # global mean to fp32 over a bf16 map
    m = torch.empty(B * C, dtype=torch.float32).cuda()
    L.check(lib.epos_global_avg_pool_bf16(_p(x_dev), C, _p(m), B, Hi * Wi, C, None), 'mean')
    torch.cuda.synchronize()
    want = x64.reshape(B, Hi * Wi, C).mean(1)
    mag = np.abs(x64).reshape(B, Hi * Wi, C).mean(1)
    np.testing.assert_array_less(np.abs(m.cpu().numpy().reshape(B, C) - want),
                                  Hi * Wi * 2.0 ** -23 * mag + 1e-12)
