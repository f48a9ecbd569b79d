"""GPU tests of the dense-heads kernel (heads_gemm_h2_f32, csrc/heads_gemm_h2.hip: the
A-stationary form of the fp16-pair GEMM, reached through epos_heads_gemm_f32). It must give
the generic grouped fp16-pair GEMM's bits (epos_pointwise_conv_grouped_f32, the kernel the
plan uses with EPOS_HEADS_KERNEL=0 and the sparse heads always use) for every head shape the
network builds: equal bit patterns, no tolerance; and the plan query (epos_heads_gemm_plan)
must say that the A-stationary kernel is what ran. The launch regimes are swept in
tests/test_gpu_heads_regimes.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


@pytest.fixture(scope='module')
def lib():
  from epos_amd import _lib
  assert torch.cuda.is_available(), 'GPU tests need a HIP device'
  return _lib.load()


def _p(t):
  return ctypes.c_void_p(t.data_ptr())


def _pack(lib, w_kn, which):
  k, n = w_kn.shape
  w = np.ascontiguousarray(w_kn, np.float32)
  fn = {'plain': lib.epos_pack_pointwise_weights,
        'h2': lib.epos_pack_pointwise_weights_h2}[which]
  total = fn(w.ctypes.data_as(ctypes.c_void_p), k, n, None)
  assert total > 0, which
  dst = np.empty(total, np.float32 if which == 'plain' else np.uint8)
  fn(w.ctypes.data_as(ctypes.c_void_p), k, n, dst.ctypes.data_as(ctypes.c_void_p))
  return torch.from_numpy(dst).cuda()


def _run_both(lib, a, heads, c_stream=1, pad=0):
  """a: [M, 256] fp32 (numpy); heads: list of (w [256, N], bias [N] or None). Returns the
  outputs of the generic grouped GEMM and of epos_heads_gemm_f32 (full [M, ldc] buffers,
  ldc = N + pad, pre-filled with a sentinel), per head."""
  from epos_amd import _lib
  m, k = a.shape
  A = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  slot = torch.zeros(_lib.AMAX_WORDS, dtype=torch.int32, device='cuda')
  _lib.check(lib.epos_absmax_f32(_p(A), k, m, k, _p(slot), stream), 'absmax')
  keep, outs = [A, slot], []
  for kind in ('generic', 'heads'):
    args, cs = [], []
    for w, b in heads:
      n = w.shape[1]
      wp, wh = _pack(lib, w, 'plain'), _pack(lib, w, 'h2')
      bias = torch.from_numpy(np.ascontiguousarray(b, np.float32)).cuda() if b is not None else None
      C = torch.full((m, n + pad), SENTINEL, device='cuda')
      keep += [wp, wh, bias, C]
      cs.append(C)
      args.append(_lib.PointwiseArgs(
          A=_p(A), lda=k, Wp=_p(wp), bias=_p(bias) if bias is not None else None, R=None,
          ldr=0, C=_p(C), ldc=n + pad, M=m, N=n, K=k, relu=0, sub=1, Wh=_p(wh),
          a_amax=_p(slot), a_amax2=None, a_gain=0.0, a_bias=0.0, c_stream=c_stream))
    arr = (_lib.PointwiseArgs * len(args))(*args)
    fn = lib.epos_heads_gemm_f32 if kind == 'heads' else lib.epos_pointwise_conv_grouped_f32
    if kind == 'heads':
      # the entry point falls back silently: the A-stationary kernel must be what runs
      assert lib.epos_heads_gemm_plan(arr, len(args), 0, None) == 1
    _lib.check(fn(arr, len(args), stream), kind)
    torch.cuda.synchronize()
    outs.append(cs)
  return outs


def _heads(rng, ns, bias=True):
  return [(rng.standard_normal((256, n)).astype(np.float32) * 0.06,
           rng.standard_normal(n).astype(np.float32) * 0.5 if bias else None) for n in ns]


def _assert_equal(outs, m, ns, pad=0):
  for g, h, n in zip(outs[0], outs[1], ns):
    # bit patterns: NaN == NaN, -0.0 != 0.0
    gi, hi = g.view(torch.int32), h.view(torch.int32)
    assert torch.equal(gi, hi), (n, (gi != hi).sum().item())
    # every element written, the padding columns untouched
    assert not (g[:, :n] == SENTINEL).any()
    if pad:
      assert (h[:, n:] == SENTINEL).all()


def _decoder_like(rng, m):
  return np.maximum(rng.standard_normal((m, 256)), 0).astype(np.float32) * 3.0


@pytest.mark.parametrize('f', [64, 256], ids=['F64_C2', 'F256'])
def test_heads_c2_group(lib, f):
  """The C2 head group: M 19 200 (160 x 120 decoder pixels), 21 objects: 22 / 21 F / 63 F
  channels (F = 64: N 5 398; F = 256: N 21 526)."""
  rng = np.random.default_rng(10 + f)
  m, o = 19200, 21
  ns = [o + 1, o * f, 3 * o * f]
  outs = _run_both(lib, _decoder_like(rng, m), _heads(rng, ns))
  _assert_equal(outs, m, ns)


def test_heads_one_object_c1(lib):
  """C1: one object, N = 2 + 64 + 192 = 258."""
  rng = np.random.default_rng(1)
  m, ns = 19200, [2, 64, 192]
  outs = _run_both(lib, _decoder_like(rng, m), _heads(rng, ns))
  _assert_equal(outs, m, ns)


def test_heads_ragged_m_c4(lib):
  """C4: a 720 x 540 image gives 135 x 180 = 24 300 decoder rows (the last 128-row panel
  partial); also without streaming stores and with padded output rows (ldc > N)."""
  rng = np.random.default_rng(4)
  m, ns = 24300, [22, 1344, 4032]
  outs = _run_both(lib, _decoder_like(rng, m), _heads(rng, ns), c_stream=0, pad=4)
  _assert_equal(outs, m, ns, pad=4)


def test_heads_batch4(lib):
  """Batch 4 (the C3 shard): M = 76 800."""
  rng = np.random.default_rng(3)
  m, ns = 76800, [22, 1344, 4032]
  outs = _run_both(lib, _decoder_like(rng, m), _heads(rng, ns))
  _assert_equal(outs, m, ns)


@pytest.mark.parametrize('m', [9, 200, 1000, 4001])
def test_heads_small_and_odd_m(lib, m):
  """Panels and work items smaller than the chip (several XCDs without a panel), odd M,
  no bias on one head."""
  rng = np.random.default_rng(m)
  ns = [7, 64, 640]
  heads = _heads(rng, ns)
  heads[1] = (heads[1][0], None)
  outs = _run_both(lib, _decoder_like(rng, m), heads)
  _assert_equal(outs, m, ns)


def test_heads_zero_rows_and_heavy_tails(lib):
  """A with all-zero rows (whole panels and single rows) and heavy-tailed values (Cauchy:
  magnitudes over many binades, so that small elements sit far below the scale)."""
  rng = np.random.default_rng(7)
  m, ns = 6000, [22, 1344, 4032]
  a = rng.standard_cauchy((m, 256)).astype(np.float32)
  a[:256] = 0.0                       # two whole panels
  a[1000:1003] = 0.0
  a[rng.integers(0, m, 50)] = 0.0
  a[4000:4010] *= 1e-30               # tiny rows next to the large bound
  outs = _run_both(lib, a, _heads(rng, ns))
  _assert_equal(outs, m, ns)


def test_heads_falls_back_for_other_groups(lib):
  """A group outside the kernel's shape (here: K != 256) goes to the generic GEMM through the
  same entry point, with the same results."""
  from epos_amd import _lib
  rng = np.random.default_rng(5)
  m, k, n = 1000, 128, 96
  a = torch.from_numpy(rng.standard_normal((m, k)).astype(np.float32)).cuda()
  w = rng.standard_normal((k, n)).astype(np.float32)
  wp, wh = _pack(lib, w, 'plain'), _pack(lib, w, 'h2')
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  slot = torch.zeros(_lib.AMAX_WORDS, dtype=torch.int32, device='cuda')
  _lib.check(lib.epos_absmax_f32(_p(a), k, m, k, _p(slot), stream), 'absmax')
  outs = []
  for fn in (lib.epos_pointwise_conv_grouped_f32, lib.epos_heads_gemm_f32):
    c = torch.zeros(m, n, device='cuda')
    args = (_lib.PointwiseArgs * 1)(_lib.PointwiseArgs(
        A=_p(a), lda=k, Wp=_p(wp), bias=None, R=None, ldr=0, C=_p(c), ldc=n, M=m, N=n, K=k,
        relu=0, sub=1, Wh=_p(wh), a_amax=_p(slot)))
    assert lib.epos_heads_gemm_plan(args, 1, 0, None) == 0
    _lib.check(fn(args, 1, stream), 'gemm')
    torch.cuda.synchronize()
    outs.append(c)
  assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
