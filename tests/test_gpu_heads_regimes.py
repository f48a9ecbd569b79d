"""The dense-heads kernel (heads_gemm_h2_f32, csrc/heads_gemm_h2.hip, entry epos_heads_gemm_f32)
in every launch regime of tests/helpers/heads_cases.py, K = 256. Every case
 (a) asks epos_heads_gemm_plan whether the A-stationary kernel runs at all -- the entry point
     falls back silently -- and holds the plan to the Python mirror and the case to the regime
     it is named for on THIS device;
 (b) runs the group through epos_heads_gemm_f32 and through epos_pointwise_conv_grouped_f32 into
     buffers filled with a NaN sentinel and demands the same bit patterns, no sentinel left
     inside [:, :N] and every sentinel intact outside (padding columns, neighbouring heads'
     columns, guard rows before and behind the matrix);
 (c) compares with the fp64 product, relative to sum |a||w| + |bias|, at the bar of
     test_pointwise_gemm_h2_accuracy (times the power of two by which the slot moves the scale);
 (d) has NaN behind column K of A (lda > K) and in 128 rows behind row M - 1: no NaN may come
     out of a finite case.
The fp64 references are computed once per (A, N) and shared."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import heads_cases as hc

pytestmark = pytest.mark.gpu

CASES = hc.by_name(hc.CASES)


@pytest.fixture(scope='module')
def lib():
  from epos_amd import _lib
  assert torch.cuda.is_available(), 'GPU tests need a HIP device'
  return _lib.load()


@pytest.fixture(scope='module')
def cus():
  return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------- inputs ---
@functools.lru_cache(maxsize=None)
def _a_host(m, seed, kind):
  """Decoder-like A [M, 256]; kind 'inf': one Inf row and one NaN row."""
  rng = np.random.default_rng(1000 + seed)
  a = np.maximum(rng.standard_normal((m, hc.K)), 0).astype(np.float32) * 3.0
  if kind == 'inf':
    a[3, 17] = np.inf
    a[70, 5] = np.nan
  a.setflags(write=False)
  return a


@functools.lru_cache(maxsize=None)
def _w_host(n):
  rng = np.random.default_rng(5000 + n)
  w = rng.standard_normal((hc.K, n)).astype(np.float32) * 0.06
  b = rng.standard_normal(n).astype(np.float32) * 0.5
  w.setflags(write=False)
  b.setflags(write=False)
  return w, b


@functools.lru_cache(maxsize=None)
def _reference(m, seed, n, has_bias):
  """(fp64 product + bias, sum |a||w| + |bias|), finite inputs."""
  a = _a_host(m, seed, None).astype(np.float64)
  w, b = _w_host(n)
  ref = a @ w.astype(np.float64)
  den = np.abs(a) @ np.abs(w).astype(np.float64)
  if has_bias:
    ref += b.astype(np.float64)
    den += np.abs(b).astype(np.float64)
  assert (den > 0).all(), 'sum |a||w| must be nowhere zero'
  return ref, den


def _pack(lib, w, which):
  k, n = w.shape
  fn = {'plain': lib.epos_pack_pointwise_weights,
        'h2': lib.epos_pack_pointwise_weights_h2}[which]
  src = w.ctypes.data_as(ctypes.c_void_p)
  total = fn(src, k, n, None)
  assert total > 0, which
  dst = np.empty(total, np.float32 if which == 'plain' else np.uint8)
  fn(src, k, n, dst.ctypes.data_as(ctypes.c_void_p))
  return torch.from_numpy(dst).cuda()


_W_DEV = {}


def _w_dev(lib, n, bias_off):
  """(Wp, Wh, bias allocation) on the device, kept for the module. Above PLAIN_PACK_MAX_N
  columns Wp -- required, but never read on the fp16-pair path -- is Wh's (larger) buffer."""
  if ('w', n) not in _W_DEV:
    w, _ = _w_host(n)
    wh = _pack(lib, w, 'h2')
    assert wh.numel() == hc.wh_bytes(n)
    _W_DEV[('w', n)] = (_pack(lib, w, 'plain') if n <= hc.PLAIN_PACK_MAX_N else wh, wh)
  if ('b', n, bias_off) not in _W_DEV:
    flat = np.full(-(-n // 128) * 128 + 4, np.nan, np.float32)   # NaN around the N values
    flat[bias_off:bias_off + n] = _w_host(n)[1]
    _W_DEV[('b', n, bias_off)] = torch.from_numpy(flat).cuda()
  return _W_DEV[('w', n)] + (_W_DEV[('b', n, bias_off)],)


class Group(object):
  """A case's inputs on the device and its argument arrays."""

  def __init__(self, lib, case):
    from epos_amd import _lib
    self.lib, self.case = lib, case
    a = _a_host(case.m, case.seed, 'inf' if case.scale == 'inf' else None)
    flat = np.full(hc.a_floats(case), np.nan, np.float32)
    view = flat[case.a_off:].reshape(case.m + hc.A_NAN_ROWS, case.lda)
    view[:case.m, :hc.K] = a
    self.A = torch.from_numpy(flat).cuda()
    assert self.A.data_ptr() % 512 == 0
    self.true_max = np.float32(np.abs(_a_host(case.m, case.seed, None)).max())
    w, w2, self.gain, self.bias = hc.slot_words(case, self.true_max)
    self.slot = torch.zeros(_lib.AMAX_WORDS, dtype=torch.int32, device='cuda')
    self.slot2 = None
    if w is None:
      _lib.check(lib.epos_absmax_f32(self.A.data_ptr() + 4 * case.a_off, case.lda, case.m, hc.K,
                                     self.slot.data_ptr(), _stream()), 'absmax')
    else:
      self.slot[37] = w                       # one word; the bound is the maximum over all 64
    if w2 is not None:
      self.slot2 = torch.zeros(_lib.AMAX_WORDS, dtype=torch.int32, device='cuda')
      self.slot2[5] = w2
    self.weights = [_w_dev(lib, n, case.bias_off) for n, _ in case.heads]
    self.layout = hc.layout(case)
    self.places = hc.head_places(case)

  def buffers(self):
    bufs = [torch.full((b.floats,), hc.SENTINEL_BITS, dtype=torch.int32, device='cuda')
            for b in self.layout]
    assert all(b.data_ptr() % 512 == 0 for b in bufs)
    return bufs

  def args(self, bufs):
    hp = [(wp.data_ptr(), wh.data_ptr(), b.data_ptr(), bufs[bi].data_ptr())
          for (wp, wh, b), (bi, _, _) in zip(self.weights, self.places)]
    return hc.make_args(self.case, self.A.data_ptr(), self.slot.data_ptr(),
                        self.slot2.data_ptr() if self.slot2 is not None else None, self.gain,
                        self.bias, hp)

  def launch(self, kind, bufs):
    """Enqueues the group on the current stream; returns what must stay alive."""
    from epos_amd import _lib
    arr = self.args(bufs)
    fn = (self.lib.epos_heads_gemm_f32 if kind == 'heads'
          else self.lib.epos_pointwise_conv_grouped_f32)
    _lib.check(fn(arr, len(self.case.heads), _stream()), kind)
    return arr

  def run(self, kind):
    """One launch into fresh sentinel-filled buffers; the buffers as host int32 arrays."""
    bufs = self.buffers()
    keep = self.launch(kind, bufs)
    torch.cuda.synchronize()
    del keep
    return [b.cpu().numpy() for b in bufs]


def _written(case, buf_index):
  """Boolean mask over a flat C buffer: the elements the group must write."""
  b = hc.layout(case)[buf_index]
  mask = np.zeros(b.floats, bool)
  for i, off, ldc in b.heads:
    n = case.heads[i][0]
    idx = off + np.arange(case.m)[:, None] * ldc + np.arange(n)[None, :]
    assert not mask[idx].any()
    mask[idx] = True
  return mask


def _head_values(case, outs, i):
  bi, off, ldc = hc.head_places(case)[i]
  n = case.heads[i][0]
  idx = off + np.arange(case.m)[:, None] * ldc + np.arange(n)[None, :]
  return outs[bi][idx].view(np.float32)


def _check_plan(lib, g, cus):
  """(a): the A-stationary kernel runs, as the mirror plans it, in the case's regime."""
  case = g.case
  arr = g.args(g.buffers())
  rc, plan = hc.query_plan(lib, arr, len(case.heads), 0)
  assert rc == 1, '%s: epos_heads_gemm_f32 would fall back to the grouped GEMM' % case.name
  r = hc.regime(case, cus)
  assert plan == [r.nt, r.panels, r.range, r.nr, r.blocks], (case.name, plan, r)
  missing = set(case.expect) - hc.regime_names(case, cus)
  assert not missing, ('%s: with %d CUs the case is no longer in the regime(s) %s it is named '
                       'for' % (case.name, cus, sorted(missing)))


def _check_bits(case, gen, hd):
  """(b): identical bit patterns; all of [:, :N] written; every sentinel elsewhere intact."""
  for bi in range(len(gen)):
    mask = _written(case, bi)
    for name, out in (('generic', gen[bi]), ('heads', hd[bi])):
      left = int((out[mask] == np.int32(hc.SENTINEL_BITS)).sum())
      assert left == 0, '%s: %s left %d elements of buffer %d unwritten' % (
          case.name, name, left, bi)
      broken = np.flatnonzero(out[~mask] != np.int32(hc.SENTINEL_BITS))
      assert broken.size == 0, '%s: %s wrote %d elements outside its columns / rows of ' \
          'buffer %d (first at flat index %d of the outside)' % (
              case.name, name, broken.size, bi, broken[0] if broken.size else -1)
    diff = np.flatnonzero(gen[bi] != hd[bi])
    assert diff.size == 0, '%s: %d bit patterns of buffer %d differ from the grouped GEMM ' \
        '(first at flat index %d)' % (case.name, diff.size, bi, diff[0] if diff.size else -1)


def _check_fp64(case, g, gen, hd):
  """(c) and (d)."""
  bound = hc.H2_MAX_REL_ERR * hc.scale_ratio(case, g.true_max)
  for i, (n, has_bias) in enumerate(case.heads):
    ref, den = _reference(case.m, case.seed, n, has_bias)
    got = _head_values(case, hd, i)
    rows = np.ones(case.m, bool)
    if case.scale == 'inf':
      # only the rows that are finite in the generic kernel's own output
      rows = np.isfinite(_head_values(case, gen, i)).all(axis=1)
      assert rows.sum() == case.m - 2 and not rows[3] and not rows[70], case.name
    else:
      assert np.isfinite(got).all(), '%s: head %d has non-finite values' % (case.name, i)
    err = float((np.abs(got[rows].astype(np.float64) - ref[rows]) / den[rows]).max())
    print('%s head %d (N %d): max error / (sum|a||w| + |b|) = %.3g (bound %.3g)' % (
        case.name, i, n, err, bound))
    assert err < bound, (case.name, i, n, err, bound)


@pytest.mark.parametrize('name', [c.name for c in hc.CASES])
def test_heads_regime(lib, cus, name):
  case = CASES[name]
  g = Group(lib, case)
  _check_plan(lib, g, cus)
  gen = g.run('generic')
  hd = g.run('heads')
  _check_bits(case, gen, hd)
  _check_fp64(case, g, gen, hd)


# -------------------------------------------------------------------- history and capture ---
def _same(a, b):
  return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_heads_launch_is_independent_of_the_one_before(lib, cus):
  """X, then a different group Y (other tile count, other parity count, other store paths),
  then X again into fresh buffers: X's bits do not depend on the LDS, parity slot and ring
  stages Y leaves behind."""
  gx, gy = (Group(lib, CASES[n]) for n in hc.HISTORY_PAIR)
  _check_plan(lib, gx, cus)
  _check_plan(lib, gy, cus)
  x0 = gx.run('heads')
  y0 = gy.run('heads')
  x1 = gx.run('heads')
  y1 = gy.run('heads')
  assert _same(x0, x1) and _same(y0, y1)
  _check_bits(gx.case, gx.run('generic'), x1)
  _check_bits(gy.case, gy.run('generic'), y1)
  # back to back on the stream, nothing in between
  bx, by, bx2 = gx.buffers(), gy.buffers(), gx.buffers()
  keep = [gx.launch('heads', bx), gy.launch('heads', by), gx.launch('heads', bx2)]
  torch.cuda.synchronize()
  del keep
  assert _same([b.cpu().numpy() for b in bx], x0)
  assert _same([b.cpu().numpy() for b in by], y0)
  assert _same([b.cpu().numpy() for b in bx2], x0)


def test_heads_on_a_non_default_stream(lib, cus):
  g = Group(lib, CASES['a_nt9'])
  _check_plan(lib, g, cus)
  ref = g.run('heads')
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  with torch.cuda.stream(s):
    assert torch.cuda.current_stream().cuda_stream == s.cuda_stream
    out = g.run('heads')
  assert _same(ref, out)
  _check_bits(g.case, g.run('generic'), out)


def test_heads_in_a_captured_graph(lib, cus):
  """One heads launch captured on a single stream (after an eager one: the first launch on a
  device allocates) and replayed twice into re-sentinelled buffers: the eager bits."""
  g = Group(lib, CASES['c_m257'])
  _check_plan(lib, g, cus)
  eager = g.run('heads')
  bufs = g.buffers()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    keep = g.launch('heads', bufs)
  for _ in range(2):
    for b in bufs:
      b.fill_(hc.SENTINEL_BITS)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(eager, [b.cpu().numpy() for b in bufs])
  del keep


# ------------------------------------------------------------------------------ network ---
def test_net_head_group_runs_on_the_heads_kernel_with_the_generic_bits(lib, monkeypatch):
  """The smallest fp32 EposNet of the suite, built with EPOS_HEADS_KERNEL=0 and =1 (read when
  the plan is built): same weights, same input, bit-identical dense head outputs; and the =1
  plan's head group is one epos_heads_gemm_plan says the A-stationary kernel takes."""
  from epos_amd import model, weights
  num_objs, h, w = 1, 64, 64
  ckpt = weights.random_init(num_objs=num_objs, seed=0)
  img = torch.from_numpy(
      np.random.RandomState(0).randint(0, 256, (1, h, w, 3)).astype('f')).cuda()
  mo = model.ModelOptions(model.get_outputs_to_num_channels(num_objs, 64))
  outs, nets = [], []
  for flag, inst in (('0', 40), ('1', 41)):
    monkeypatch.setenv('EPOS_HEADS_KERNEL', flag)
    net = model.get_net(ckpt, 1, h, w, num_objs, 64, mo, instance=inst)
    out = net.forward_logits(img)
    torch.cuda.synchronize()
    outs.append({k: v.clone() for k, v in out.items()})
    nets.append(net)
  assert nets[0].heads_group is None
  arr, count = nets[1].heads_group
  assert count == 3
  rc, plan = hc.query_plan(lib, arr, count, 0)
  assert rc == 1
  assert plan[0] == sum(-(-arr[i].N // 64) for i in range(count))
  assert set(outs[0]) == set(outs[1]) and len(outs[0]) == 3
  for k in outs[0]:
    a, b = outs[0][k].contiguous(), outs[1][k].contiguous()
    assert a.dtype == torch.float32 and a.shape == b.shape
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert torch.isfinite(a).all() and float(a.abs().max()) > 0
