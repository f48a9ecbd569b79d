"""The correspondence kernels (csrc/corresp.hip) over the table of tests/helpers/glue_cases.py,
through epos_corr_count, epos_corr_slot_bases and epos_corr_fill directly, so that the base
alignment of the scan arrays, the batch and the capacity are the test's: F below, at and above
64, maps whose scan needs several chunks in both of its forms, two images interleaved with one
object twice, capacities that overflow. The reference is oracle/corresp_ref.py, slot by slot:
array_equal on all seven outputs, on `totals` and on `slot_base`. Every scratch and output array
sits between sentinels (-1 / 0xff bytes) that must survive; every case runs twice."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import glue_cases as gc
from helpers import glue_ref as gr

pytestmark = pytest.mark.gpu

GUARD = 64
LEAD = 8                    # elements before a base: keeps 16-byte alignment for every type
E_INVALID = -1
TORCH = {np.dtype(np.int64): torch.int64, np.dtype(np.float64): torch.float64,
         np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}


def _lib():
  from epos_amd import _lib as L
  return L, L.load()


def _p(t, off=0):
  return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded(object):
  """n elements at element offset off inside an allocation of 0xff bytes (-1 for integers, a NaN
  for floats) with GUARD more behind them."""

  def __init__(self, n, dtype, off=LEAD):
    self.n, self.off = n, off
    raw = torch.full(((off + n + GUARD) * np.dtype(dtype).itemsize,), -1, dtype=torch.int8,
                     device='cuda')
    self.buf = raw.view(TORCH[np.dtype(dtype)])
    self.dtype = np.dtype(dtype)
    self.ptr = _p(self.buf, off)
    assert self.buf.data_ptr() % 256 == 0

  def read(self, written=None):
    """The first `written` (default: all n) elements; everything else must still be 0xff."""
    written = self.n if written is None else written
    raw = self.buf.cpu().numpy().view(np.uint8)
    sz = self.dtype.itemsize
    lo, hi = self.off * sz, (self.off + written) * sz
    assert (raw[:lo] == 0xff).all(), 'write before the base'
    assert (raw[hi:] == 0xff).all(), 'write at or beyond the end'
    return raw[lo:hi].copy().view(self.dtype)


def _run(case, prob_dev, off, capacity, total):
  """One count + slot_bases + fill; returns dict of host arrays (sentinels checked)."""
  L, lib = _lib()
  obj, frag, coords, centers, sizes = prob_dev
  B, O, F, P = gc.CORR_B, gr.corr_num_objs(case), case.f, case.h * case.w
  slots = gc.corr_slots(case)
  S = len(slots)
  nw = (F + 63) // 64
  sl = torch.tensor(slots, dtype=torch.int32, device='cuda')
  px, co = Guarded(S * P, np.int32, LEAD + off), Guarded(S * P, np.int32, LEAD + off)
  fm = Guarded(S * P * nw, np.int64)
  tot, base, ovf = Guarded(2 * S, np.int32), Guarded(S + 1, np.int64), Guarded(1, np.int32)
  ovf.buf[ovf.off] = 0
  s = _stream()
  L.check(lib.epos_corr_count(_p(obj), _p(frag), _p(sl), S, B, P, O, F, gr.TAU_A, gr.TAU_B,
                              px.ptr, co.ptr, fm.ptr, tot.ptr, s), 'epos_corr_count')
  L.check(lib.epos_corr_slot_bases(tot.ptr, S, base.ptr, s), 'epos_corr_slot_bases')
  outs = {k: Guarded(total * gr.CORR_WIDTH[k], gr.CORR_DTYPES[k]) for k in gr.CORR_KEYS}
  co_struct = L.CorrOut(**{k: outs[k].ptr for k in gr.CORR_KEYS})
  L.check(lib.epos_corr_fill(_p(obj), _p(frag), _p(coords), _p(centers), _p(sizes), _p(sl), S, B,
                             P, case.w, O, F, 1.0 / gr.OUTPUT_SCALE, px.ptr, co.ptr, fm.ptr,
                             base.ptr, capacity, ctypes.byref(co_struct), ovf.ptr, s),
          'epos_corr_fill')
  torch.cuda.synchronize()
  res = {k: outs[k].read(capacity * gr.CORR_WIDTH[k]) for k in gr.CORR_KEYS}
  res.update(px_off=px.read(), corr_off=co.read(), frag_mask=fm.read(), totals=tot.read(),
             slot_base=base.read(), overflow=ovf.read())
  return res


def _case_results(case):
  prob, per_slot, totals, slot_base, pooled = gr.corr_reference(case)
  dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in prob]
  total = int(slot_base[-1])
  cap = gr.corr_capacity(case, totals, slot_base)
  a = _run(case, dev, case.off, cap, total)
  b = _run(case, dev, case.off, cap, total)
  for k in a:
    assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), ('two runs differ', k)
  return a, (totals, slot_base, pooled, total, cap)


@pytest.mark.parametrize('name', [c.name for c in gc.CORR])
def test_corr_count_and_fill_equal_the_oracle(name):
  case = gc.by_name(gc.CORR)[name]
  got, (totals, slot_base, pooled, total, cap) = _case_results(case)
  P = case.h * case.w
  S = len(gc.corr_slots(case))
  assert np.array_equal(got['totals'].reshape(S, 2), totals)
  assert np.array_equal(got['slot_base'], slot_base)
  # the exclusive scans end in the totals
  px, co = got['px_off'].reshape(S, P), got['corr_off'].reshape(S, P)
  assert (px[:, 0] == 0).all() and (co[:, 0] == 0).all()
  assert (np.diff(px, axis=1) >= 0).all() and (np.diff(px, axis=1) <= 1).all()
  masked = np.concatenate([np.diff(px, axis=1), (totals[:, :1] - px[:, -1:])], axis=1)
  assert np.array_equal(masked.sum(1), totals[:, 0])
  assert got['overflow'][0] == (1 if cap < total else 0)
  for k in gr.CORR_KEYS:
    want = pooled[k].reshape(-1)[:cap * gr.CORR_WIDTH[k]]
    assert got[k].dtype == want.dtype and np.array_equal(got[k], want), k


@pytest.mark.parametrize('unaligned,aligned', gc.CORR_ALIGN_PAIRS)
def test_corr_scan_unaligned_arrays_give_the_aligned_result(unaligned, aligned):
  """px_off / corr_off 4 bytes off a 16-byte boundary with P % 4 == 0: the launcher must take
  the one-element scan, and every array must equal the aligned run's."""
  cases = gc.by_name(gc.CORR)
  assert gc.corr_regime(cases[unaligned].f, cases[unaligned].h * cases[unaligned].w,
                        cases[unaligned].off).vec == 1
  a, _ = _case_results(cases[unaligned])
  b, _ = _case_results(cases[aligned])
  for k in a:
    assert np.array_equal(a[k], b[k]), k


def test_corr_launchers_refuse_invalid_arguments():
  """Every EPOS_REQUIRE of the three launchers once: EPOS_E_INVALID, a message that names the
  function, nothing launched."""
  L, lib = _lib()
  B, P, W, O, F, S = 1, 8, 4, 1, 4, 1
  z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device='cuda')   # noqa: E731
  obj, frag, coords = z(B * P * (O + 1)), z(B * P * O * F), z(B * P * O * F * 3)
  cen, siz = z(O * F * 3, torch.float64), z(O * F, torch.float64)
  sl = torch.tensor([[0, 1]], dtype=torch.int32, device='cuda')
  px, co, fm = Guarded(S * P, np.int32), Guarded(S * P, np.int32), Guarded(S * P, np.int64)
  tot, base, ovf = Guarded(2 * S, np.int32), Guarded(S + 1, np.int64), Guarded(1, np.int32)
  outs = {k: Guarded(4 * gr.CORR_WIDTH[k], gr.CORR_DTYPES[k]) for k in gr.CORR_KEYS}
  s = _stream()

  def refused(rc, fn):
    assert rc == E_INVALID, (fn, rc)
    msg = lib.epos_last_error().decode()
    assert fn in msg and len(msg) > len(fn) + 2, msg

  good = [_p(obj), _p(frag), _p(sl), S, B, P, O, F, 0.1, 0.5, px.ptr, co.ptr, fm.ptr, tot.ptr]
  for i, v in [(0, None), (1, None), (2, None), (10, None), (11, None), (12, None), (13, None),
               (7, 0), (7, 257), (4, 0), (5, 0), (6, 0), (3, -1)]:
    args = list(good)
    args[i] = v
    refused(lib.epos_corr_count(*args, s), 'epos_corr_count')
  refused(lib.epos_corr_slot_bases(None, S, base.ptr, s), 'epos_corr_slot_bases')
  refused(lib.epos_corr_slot_bases(tot.ptr, S, None, s), 'epos_corr_slot_bases')
  refused(lib.epos_corr_slot_bases(tot.ptr, -1, base.ptr, s), 'epos_corr_slot_bases')
  out = L.CorrOut(**{k: outs[k].ptr for k in gr.CORR_KEYS})
  good = [_p(obj), _p(frag), _p(coords), _p(cen), _p(siz), _p(sl), S, B, P, W, O, F, 4.0,
          px.ptr, co.ptr, fm.ptr, base.ptr, 4, ctypes.byref(out), ovf.ptr]
  for i, v in [(0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (13, None),
               (14, None), (15, None), (16, None), (18, None), (19, None),
               (11, 0), (11, 257), (9, 0), (9, 3), (7, 0), (8, 0), (10, 0), (6, -1)]:
    args = list(good)
    args[i] = v
    refused(lib.epos_corr_fill(*args, s), 'epos_corr_fill')
  for k in gr.CORR_KEYS:                                  # a missing output array
    holed = L.CorrOut(**{j: (None if j == k else outs[j].ptr) for j in gr.CORR_KEYS})
    args = list(good)
    args[18] = ctypes.byref(holed)
    refused(lib.epos_corr_fill(*args, s), 'epos_corr_fill')
  torch.cuda.synchronize()
  for g in [px, co, fm, tot, base, ovf] + list(outs.values()):
    g.read(0)                                             # nothing written anywhere
