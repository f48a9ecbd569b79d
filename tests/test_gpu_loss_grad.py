"""The loss gradients (csrc/loss_grad.hip) through the C ABI against
tests/helpers/loss_grad_ref.py: zeros and the localisation gradient as bytes, the two softmax
gradients to the derived bound; every launch regime, views and alignment, null outputs,
extreme and non-finite logits, the Huber knee, the pixel rules, determinism and position; the
reduction of the tables against loss.summarize; differentiable_losses through autograd, a
descent on the logits, and a captured graph."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import loss_cases, loss_grad_ref, loss_ref                     # noqa: E402
from tests.helpers.loss_device import (IGNORE, KEYS, MEAN, POOLED, UPSTREAM,      # noqa: E402
                                       WEIGHTS, _lib, _off, _out, _p, _stream, ref_counts,
                                       tensors)

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc12345                     # the bits of a NaN no kernel produces


def share_of(P, O, F):
  s = _lib().epos_loss_grad_share_pixels(P, O, F)
  assert s >= 1
  return int(s)


def take(c, images):
  return {k: np.ascontiguousarray(v[list(images)]) for k, v in c.items()}


def run_grads(c, scale, upstream=None, ignore=IGNORE, ld_obj=None, ld_dobj=None,
              in_off=(0, 0, 0), out_off=(0, 0, 0), need=(True, True, True)):
  """One call over a host case. Returns the three outputs as uint32 arrays (the bits):
  d_obj [B,P,O+1], d_frag [B,P,O,F], d_loc [B,P,O,F,3], or None for a head not asked for,
  whose buffer must still hold the sentinel, as must the padding columns of d_obj."""
  lib = _lib()
  B, P, O1 = c['obj_logits'].shape
  O, F = c['frag_logits'].shape[2:4]
  ld = O1 if ld_obj is None else ld_obj
  ldd = O1 if ld_dobj is None else ld_dobj
  padded = np.full((B * P, ld), np.nan, np.float32)     # the padding must never be read
  padded[:, :O1] = c['obj_logits'].reshape(B * P, O1)
  obj = _off(padded, in_off[0])
  frag = _off(c['frag_logits'], in_off[1])
  loc = _off(c['frag_loc'], in_off[2])
  g_obj = torch.from_numpy(np.ascontiguousarray(c['gt_obj'], np.int32)).cuda()
  g_frag = torch.from_numpy(np.ascontiguousarray(c['gt_frag'], np.int32)).cuda()
  g_loc = torch.from_numpy(np.ascontiguousarray(c['gt_loc'], np.float32)).cuda()
  g_w = torch.from_numpy(np.ascontiguousarray(c['gt_weight'], np.float32)).cuda()
  sc = torch.from_numpy(np.ascontiguousarray(scale, np.float64)).cuda()
  up = None if upstream is None else torch.tensor(upstream, dtype=torch.float64, device='cuda')
  bufs = [_out(B * P * ldd, out_off[0], SENTINEL), _out(B * P * O * F, out_off[1], SENTINEL),
          _out(B * P * O * F * 3, out_off[2], SENTINEL)]
  ptrs = [_p(b) if n else None for b, n in zip(bufs, need)]
  rc = lib.epos_loss_grads(_p(obj), ld, _p(frag), _p(loc), _p(g_obj), _p(g_frag), _p(g_loc),
                           _p(g_w), B, P, O, F, ignore, _p(sc), _p(up), ptrs[0], ldd, ptrs[1],
                           ptrs[2], _stream())
  assert rc == 0, lib.epos_last_error()
  torch.cuda.synchronize()
  raw = [b.view(torch.int32).cpu().numpy().view(np.uint32) for b in bufs]
  for r, n in zip(raw, need):
    if not n:
      assert (r == SENTINEL).all()                      # a skipped head is not touched
  d_obj = raw[0].reshape(B * P, ldd)
  assert (d_obj[:, O1:] == SENTINEL).all()              # nor are the padding columns
  outs = [np.ascontiguousarray(d_obj[:, :O1]).reshape(B, P, O1), raw[1].reshape(B, P, O, F),
          raw[2].reshape(B, P, O, F, 3)]
  for r, n in zip(outs, need):
    if n:
      assert not (r == SENTINEL).any()                  # every element is written
  return tuple(r if n else None for r, n in zip(outs, need))


def compare(got, c, scale, upstream=None, ignore=IGNORE):
  """Zeros as bytes (+0.0), d_loc as bytes, d_obj and d_frag to
  2^-23 |ref| + |s_k| (row + 16) 2^-52 + 2^-149."""
  ref = loss_grad_ref.grads(c, scale, upstream, ignore)
  masks = loss_grad_ref.active_masks(c, ignore)
  u = loss_grad_ref.upstream_factors(upstream)
  O, F = c['frag_logits'].shape[2:4]
  for k, row_len in enumerate((O + 1, F, 3)):
    if got[k] is None:
      continue
    assert got[k].shape == ref[k].shape
    assert not got[k][~masks[k]].any(), k               # +0.0, not -0.0
    assert not ref[k][~masks[k]].any()
    if k == 2:
      assert got[k].tobytes() == ref[k].view(np.uint32).tobytes()
      continue
    val = got[k].view(np.float32)
    for b in range(ref[k].shape[0]):
      tol = loss_grad_ref.bound(ref[k][b], scale[b, k] * u[k], row_len)
      err = np.abs(val[b].astype(np.float64) - ref[k][b].astype(np.float64))
      assert (err <= tol).all(), (k, b, float(err.max()))
  return ref


@pytest.mark.parametrize('O', [1, 3, 21])
@pytest.mark.parametrize('F', [1, 3, 4, 63, 64, 65, 256])
def test_sweep(F, O):
  # L = 1..64 lanes per pixel; 16-byte and scalar loads (F, O + 1 multiples of 4 or not); rows
  # and spans on and off 16-byte boundaries (O * F and share * O * F odd or not); a quad that
  # lies in two pixels (O * F not a multiple of 4); a short last share; a single pixel
  share = share_of(64, O, F)
  sizes = [share - 1, share, share + 1, 1]
  assert all(share_of(P, O, F) == share for P in sizes)
  for P in sizes:
    c = loss_cases.make_case(3, P, O, F, seed=1000 * F + 10 * O + (P % 7), empty_images=(1,))
    counts = ref_counts(c)
    assert counts[1, 1:, 0].sum() == 0 and (counts[[0, 2], 1:, 0].sum(axis=1) > 0).all()
    for reduction, upstream in ((MEAN, UPSTREAM), (POOLED, None)):
      scale = loss_grad_ref.scales(counts, WEIGHTS, reduction)
      got = run_grads(c, scale, upstream)
      compare(got, c, scale, upstream)
      assert not got[1][1].any() and not got[2][1].any()      # the image without foreground
      # B = 1: image 0 alone, with its factors of the batch, the same bytes as in the batch
      one = run_grads(take(c, [0]), scale[:1], upstream)
      for a, b in zip(one, got):
        assert a[0].tobytes() == b[0].tobytes()


OFFSETS = [((1, 0, 0), (0, 0, 0)), ((0, 2, 0), (0, 0, 0)), ((0, 0, 3), (0, 0, 0)),
           ((0, 0, 0), (1, 0, 0)), ((0, 0, 0), (0, 2, 0)), ((0, 0, 0), (0, 0, 3)),
           ((3, 1, 2), (2, 3, 1)), ((0, 0, 0), (3, 1, 2))]
LDS = [(0, 1), (1, 0), (2, 2), (3, 5), (5, 3), (2, 0), (0, 5)]


@pytest.fixture(scope='module')
def view_case():
  B, O, F = 2, 21, 64
  P = share_of(64, O, F) + 3
  c = loss_cases.make_case(B, P, O, F, seed=5)
  scale = loss_grad_ref.scales(ref_counts(c), WEIGHTS, MEAN)
  base = run_grads(c, scale, UPSTREAM)
  compare(base, c, scale, UPSTREAM)
  return c, scale, base


@pytest.mark.parametrize('in_off,out_off,ld_extra,ldd_extra',
                         [(i, o, 0, 0) for i, o in OFFSETS] +
                         [((0, 0, 0), (0, 0, 0), a, b) for a, b in LDS] +
                         [((1, 2, 3), (3, 2, 1), 3, 2)])
def test_views_and_alignment(view_case, in_off, out_off, ld_extra, ldd_extra):
  # a lane's values, the butterfly and an element's value do not depend on the load or the
  # store width: the same bytes as the aligned, dense run
  c, scale, base = view_case
  O = 21
  got = run_grads(c, scale, UPSTREAM, ld_obj=O + 1 + ld_extra, ld_dobj=O + 1 + ldd_extra,
                  in_off=in_off, out_off=out_off)
  for a, b in zip(got, base):
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('need', [n for n in itertools.product([True, False], repeat=3)
                                  if not all(n)])
def test_null_outputs(view_case, need):
  c, scale, base = view_case
  got = run_grads(c, scale, UPSTREAM, need=need)        # checks the sentinel of skipped heads
  for a, b, n in zip(got, base, need):
    assert (a is None) == (not n)
    if n:
      assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('F', [5, 64])
def test_extreme_logits(F):
  # the case of test_gpu_loss.test_extreme_logits: the target 200 below the maximum, every other
  # logit 1e4 below it. p(target) = 1.4e-87, so its gradient is fl32(-s), and all is finite
  B, P, O = 1, 37, 3
  c = loss_cases.make_case(B, P, O, F, seed=2, ignore_band=False)
  c['obj_logits'][:] = -1e4
  c['frag_logits'][:] = -1e4
  for p in range(P):
    g = int(c['gt_obj'][0, p])
    c['obj_logits'][0, p, (g + 1) % (O + 1)] = 30.0
    c['obj_logits'][0, p, g] = -170.0
    if g:
      f = int(c['gt_frag'][0, p])
      c['frag_logits'][0, p, g - 1, (f + 1) % F] = -20.0
      c['frag_logits'][0, p, g - 1, f] = -220.0
  scale = loss_grad_ref.scales(ref_counts(c), WEIGHTS, MEAN)
  got = run_grads(c, scale)
  compare(got, c, scale)
  d_obj, d_frag, d_loc = (g.view(np.float32) for g in got)
  assert all(np.isfinite(d).all() for d in (d_obj, d_frag, d_loc))
  n_fg = 0
  for p in range(P):
    g = int(c['gt_obj'][0, p])
    assert d_obj[0, p, g] == np.float32(-scale[0, 0])
    assert d_obj[0, p, (g + 1) % (O + 1)] == np.float32(scale[0, 0])
    if g:
      f = int(c['gt_frag'][0, p])
      assert d_frag[0, p, g - 1, f] == np.float32(-scale[0, 1])
      n_fg += 1
  assert n_fg > 0


def test_huber_knee():
  # the differences of test_gpu_loss.test_huber_knee, in every coordinate, both signs of s
  B, O, F = 1, 2, 4
  eps = 2.0 ** -23
  d = np.array([1.0, -1.0, 1.0 + eps, -1.0 - eps, 1.0 - eps / 2, -1.0 + eps / 2, 0.0, 0.5, 3.0],
               np.float32)
  P = len(d) * 3
  c = loss_cases.make_case(B, P, O, F, seed=3, ignore_band=False)
  c['gt_obj'][:] = 1 + (np.arange(P) % O)
  c['gt_frag'][:] = np.arange(P) % F
  c['gt_weight'][:] = 1.0
  c['gt_loc'][:] = 0.0
  for p in range(P):
    v = np.zeros(3, np.float32)
    v[p % 3] = d[p // 3]
    c['frag_loc'][0, p, c['gt_obj'][0, p] - 1, c['gt_frag'][0, p]] = v
  scale = loss_grad_ref.scales(ref_counts(c), WEIGHTS, MEAN)
  for upstream in (None, [0.0, 0.0, -1.0, 0.25]):
    got = run_grads(c, scale, upstream)
    compare(got, c, scale, upstream)
    s2 = scale[0, 2] * loss_grad_ref.upstream_factors(upstream)[2]
    d_loc = got[2].view(np.float32)
    for p in range(P):
      x = np.zeros(3)
      x[p % 3] = float(d[p // 3])
      # a zero difference times a negative factor is -0.0, on both sides
      hand = np.array([s2 * (1.0 * max(-1.0, min(1.0, v))) for v in x], np.float32)
      row = d_loc[0, p, c['gt_obj'][0, p] - 1, c['gt_frag'][0, p]]
      assert row.tobytes() == hand.tobytes(), (p, x)


def test_bad_and_ignored_pixels_get_zero_rows():
  # one pixel of every kind of test_loss_host.test_bad_pixel_rules_of_the_helper
  O, F = 2, 3
  kinds = [(-1, 0, 1.0), (O + 1, 0, 1.0), (2 ** 31 - 1, 0, 1.0), (1, -1, 1.0), (2, F, 1.0),
           (1, 0, 0.0), (1, 0, -1.0), (1, 0, np.inf), (1, 0, np.nan), (IGNORE, -5, np.nan)]
  fine = [(0, -5, np.nan), (1, F - 1, 1e-30), (2, 1, 1.5)]      # background reads neither
  pixels = kinds + fine
  P = len(pixels)
  c = loss_cases.make_case(1, P, O, F, seed=11, ignore_band=False)
  for p, (g, f, w) in enumerate(pixels):
    c['gt_obj'][0, p], c['gt_frag'][0, p], c['gt_weight'][0, p] = g, f, w
  sums, counts, bad = loss_cases.ref_terms(loss_ref, c, 64)
  assert bad[0] == len(kinds) - 1 and counts[0, 0, 1] == 1 and counts[0, :, 0].sum() == len(fine)
  scale = loss_grad_ref.scales(counts, WEIGHTS, MEAN)
  got = run_grads(c, scale)
  compare(got, c, scale)
  for p in range(P):
    zero = [not got[k][0, p].any() for k in range(3)]
    if p < len(kinds):
      assert zero == [True, True, True], p
    else:
      assert zero == [False, pixels[p][0] == 0, pixels[p][0] == 0], p
  # the ignore rule wins over every other rule, also with a label inside 0..O
  got = run_grads(c, scale, ignore=2)
  compare(got, c, scale, ignore=2)
  assert not got[0][0, P - 1].any() and not got[1][0, P - 1].any()


@pytest.mark.parametrize('value', [np.nan, np.inf])
@pytest.mark.parametrize('where', ['obj', 'frag', 'loc'])
def test_non_finite_logit_marks_its_row_only(where, value):
  B, O, F = 2, 3, 8
  P = share_of(64, O, F) + 9
  c = loss_cases.make_case(B, P, O, F, seed=6)
  scale = loss_grad_ref.scales(ref_counts(c), WEIGHTS, MEAN)
  clean = [g.copy() for g in run_grads(c, scale)]
  p = P - 1                                # an object-1 pixel of image 1 (make_case)
  assert c['gt_obj'][1, p] == 1
  f = c['gt_frag'][1, p]
  if where == 'obj':
    c['obj_logits'][1, p, 2] = value
  elif where == 'frag':
    c['frag_logits'][1, p, 0, (f + 1) % F] = value
  else:
    c['frag_loc'][1, p, 0, f, 1] = value
  got = run_grads(c, scale)
  ref = loss_grad_ref.grads(c, scale)
  k = {'obj': 0, 'frag': 1, 'loc': 2}[where]
  row = {'obj': (1, p), 'frag': (1, p, 0), 'loc': (1, p, 0, f, 1)}[where]
  vals = got[k].view(np.float32)
  if where == 'loc' and value == np.inf:     # an infinite difference is clamped: the knee's 1
    assert vals[row] == np.float32(scale[1, 2] * (float(c['gt_weight'][1, p]) * 1.0))
  else:
    assert not np.isfinite(vals[row]).any()
  assert (np.isfinite(vals) == np.isfinite(ref[k])).all()
  clean[k][row] = got[k][row]
  for a, b in zip(got, clean):             # and nothing else changed
    assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- reduce ---
def run_reduce(sums, counts, weights, reduction):
  lib = _lib()
  B, O1 = sums.shape[:2]
  d_sums = torch.from_numpy(np.ascontiguousarray(sums)).cuda()
  d_counts = torch.from_numpy(np.ascontiguousarray(counts)).cuda()
  values = torch.full((4,), -7.0, dtype=torch.float64, device='cuda')
  scale = torch.full((B, 3), -7.0, dtype=torch.float64, device='cuda')
  rc = lib.epos_loss_reduce(_p(d_sums), _p(d_counts), B, O1 - 1, weights[0], weights[1],
                            weights[2], reduction, _p(values), _p(scale), _stream())
  assert rc == 0, lib.epos_last_error()
  torch.cuda.synchronize()
  return values.cpu().numpy(), scale.cpu().numpy()


def device_terms(c, ignore=IGNORE):
  lib = _lib()
  B, P, O1 = c['obj_logits'].shape
  O, F = c['frag_logits'].shape[2:4]
  t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in c.items()}
  ws = torch.empty((max(lib.epos_loss_workspace_bytes(B, P, O, F) // 8, 1),), dtype=torch.int64,
                   device='cuda')
  sums = torch.empty((B, O1, 3), dtype=torch.float64, device='cuda')
  counts = torch.empty((B, O1, 2), dtype=torch.int64, device='cuda')
  bad = torch.empty((B,), dtype=torch.int64, device='cuda')
  rc = lib.epos_loss_terms(_p(t['obj_logits']), O1, _p(t['frag_logits']), _p(t['frag_loc']),
                           _p(t['gt_obj']), _p(t['gt_frag']), _p(t['gt_loc']), _p(t['gt_weight']),
                           B, P, O, F, ignore, _p(ws), _p(sums), _p(counts), _p(bad), _stream())
  assert rc == 0, lib.epos_last_error()
  torch.cuda.synchronize()
  return sums.cpu().numpy(), counts.cpu().numpy(), bad.cpu().numpy()


def check_reduce(sums, counts, weights):
  from epos_amd import loss
  B, O1 = sums.shape[:2]
  host = loss.summarize(sums, counts, np.zeros(B, np.int64), weights, O1 - 1)
  for reduction, key in ((MEAN, 'mean'), (POOLED, 'pooled')):
    values, scale = run_reduce(sums, counts, weights, reduction)
    exp = np.array([host[key][n] for n in loss.NAMES], np.float64)
    assert values.tobytes() == exp.tobytes(), (key, values, exp)
    assert scale.tobytes() == loss_grad_ref.scales(counts, weights, reduction).tobytes(), key
  return host


def test_reduce_on_device_tables():
  O, F = 3, 5
  c = loss_cases.make_case(4, 61, O, F, seed=12, empty_images=(1,))
  sums, counts, bad = device_terms(c)
  assert not bad.any() and counts[1, 1:, 0].sum() == 0
  host = check_reduce(sums, counts, WEIGHTS)
  assert host['per_image'][1]['frag_cls_loss'] == 0.0
  assert host['mean']['frag_cls_loss'] != host['pooled']['frag_cls_loss']
  check_reduce(sums[:1], counts[:1], (1.0, 1.0, 100.0))
  check_reduce(sums[1:2], counts[1:2], WEIGHTS)           # no foreground at all


@pytest.mark.parametrize('B,O', [(1, 1), (3, 300), (300, 3), (257, 256)])
def test_reduce_on_hand_made_tables(B, O):
  # more images and more objects than one round of the workgroup takes
  rng = np.random.RandomState(B + O)
  counts = np.zeros((B, O + 1, 2), np.int64)
  counts[:, :, 0] = rng.randint(0, 50, (B, O + 1))
  counts[:, 0, 0] += 1
  counts[:, 0, 1] = rng.randint(0, 9, B)
  if B > 1:
    counts[B // 2, 1:, 0] = 0
  sums = rng.uniform(0.0, 3.0, (B, O + 1, 3)) * counts[:, :, :1]
  sums[:, 0, 1:] = 0.0
  check_reduce(sums, counts, WEIGHTS)


# ---------------------------------------------------------------- determinism ---
@pytest.mark.parametrize('O,F', [(3, 64), (21, 5)])
def test_determinism_and_position(O, F):
  share = share_of(64, O, F)
  P = 2 * share + 5                        # three workgroups per image, the last one short
  assert share_of(P, O, F) == share
  c = loss_cases.make_case(3, P, O, F, seed=7, empty_images=(2,))
  sums, counts, bad = device_terms(c)
  for reduction in (MEAN, POOLED):
    _, scale = run_reduce(sums, counts, WEIGHTS, reduction)
    first = run_grads(c, scale, UPSTREAM)
    compare(first, c, scale, UPSTREAM)
    again = run_grads(c, scale, UPSTREAM)
    for a, b in zip(first, again):
      assert a.tobytes() == b.tobytes()
    for order in ([1, 2, 0], [2, 0, 1], [1, 0, 2]):
      part = take(c, order)
      p_sums, p_counts, _ = device_terms(part)
      _, p_scale = run_reduce(p_sums, p_counts, WEIGHTS, reduction)
      assert p_scale.tobytes() == scale[order].tobytes()
      moved = run_grads(part, p_scale, UPSTREAM)
      for a, b in zip(moved, first):
        assert a.tobytes() == np.ascontiguousarray(b[order]).tobytes(), order


# ---------------------------------------------------------------- through Python ---
@pytest.mark.parametrize('reduction', ['mean', 'pooled'])
def test_differentiable_losses(reduction):
  from epos_amd import loss
  B, h, w, O, F = 3, 7, 9, 3, 8
  c = loss_cases.make_case(B, h * w, O, F, seed=13, empty_images=(1,))
  logits, gt = tensors(c, h, w)
  for k in KEYS:
    logits[k].requires_grad_()
  values, bad = loss.differentiable_losses(logits, gt, WEIGHTS, reduction)
  assert values.dtype == torch.float64 and values.shape == (4,) and values.grad_fn is not None
  assert bad.dtype == torch.int64 and bad.tolist() == [0, 0, 0] and not bad.requires_grad
  # the values are LossEval's, bit for bit
  ev = loss.LossEval(O, F, 'cuda:0', *WEIGHTS)
  ev.update({k: v.detach() for k, v in logits.items()}, gt)
  exp = np.array([ev.result()[reduction][n] for n in loss.NAMES], np.float64)
  assert values.detach().cpu().numpy().tobytes() == exp.tobytes()
  # total_loss.backward(): .grad is loss_grads with the upstream {0, 0, 0, 1}
  values[3].backward(retain_graph=True)
  sums, counts, _ = loss.loss_terms({k: v.detach() for k, v in logits.items()}, gt)
  values2, scales = loss.loss_values(sums, counts, WEIGHTS, reduction)
  assert torch.equal(values2, values.detach())
  direct = loss.loss_grads({k: v.detach() for k, v in logits.items()}, gt, scales)
  for k, d in zip(KEYS, direct):
    assert d.shape == logits[k].shape and d.dtype == torch.float32
    assert logits[k].grad.cpu().numpy().tobytes() == d.cpu().numpy().tobytes()
  scale = scales.cpu().numpy()
  assert scale.tobytes() == loss_grad_ref.scales(ref_counts(c), WEIGHTS,
                                                 loss.REDUCTIONS[reduction]).tobytes()
  compare(tuple(d.cpu().numpy().reshape(c[n].shape).view(np.uint32)
                for d, n in zip(direct, ('obj_logits', 'frag_logits', 'frag_loc'))), c, scale)
  # frag_cls_loss.backward(): the other two heads get zeros
  for k in KEYS:
    logits[k].grad = None
  values[1].backward()
  assert not logits['pred_obj_conf'].grad.any() and not logits['pred_frag_loc'].grad.any()
  only = loss.loss_grads({k: v.detach() for k, v in logits.items()}, gt, scales,
                         upstream=torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64,
                                               device='cuda'), need=(False, True, False))
  assert only[0] is None and only[2] is None
  assert torch.equal(logits['pred_frag_conf'].grad, only[1]) and only[1].any()


def test_differentiable_losses_honours_needs_input_grad():
  from epos_amd import loss
  B, h, w, O, F = 2, 5, 6, 3, 8
  c = loss_cases.make_case(B, h * w, O, F, seed=14)
  logits, gt = tensors(c, h, w)
  logits['pred_frag_conf'].requires_grad_()
  values, _ = loss.differentiable_losses(logits, gt)
  values[3].backward()
  assert logits['pred_obj_conf'].grad is None and logits['pred_frag_loc'].grad is None
  sums, counts, _ = loss.loss_terms({k: v.detach() for k, v in logits.items()}, gt)
  _, scales = loss.loss_values(sums, counts, (1.0, 1.0, 100.0))
  direct = loss.loss_grads({k: v.detach() for k, v in logits.items()}, gt, scales)
  assert torch.equal(logits['pred_frag_conf'].grad, direct[1])
  # a strided object head (a slice of a wider buffer) and a strided d_obj keep their padding
  wide = torch.full((B, h, w, O + 4), float('nan'), device='cuda')
  wide[..., :O + 1] = logits['pred_obj_conf']
  d_wide = torch.full((B, h, w, O + 3), -7.0, device='cuda')
  view = dict(logits, pred_obj_conf=wide[..., :O + 1])
  out = loss.loss_grads({k: v.detach() for k, v in view.items()}, gt, scales,
                        out=(d_wide[..., :O + 1], None, None), need=(True, False, True))
  assert out[1] is None and torch.equal(out[0], direct[0]) and torch.equal(out[2], direct[2])
  assert (d_wide[..., O + 1:] == -7.0).all()


def test_descent_on_the_logits():
  # the losses are convex in the logits; a cross-entropy row's Hessian has norm <= 1/2 and the
  # Huber term's is <= 1, so a step of 1 / Lip along the negative gradient cannot increase the
  # total
  from epos_amd import loss
  B, P, O, F = 2, 67, 3, 8
  c = loss_cases.make_case(B, P, O, F, seed=4)
  weights = (1.0, 1.0, 100.0)
  counts = ref_counts(c)
  n_min = int(counts[:, 1:, 0].sum(axis=1).min())
  w_max = float(c['gt_weight'].max())
  assert n_min > 0
  lip = max(weights[0] / (2 * P), weights[1] / (2 * n_min),
            weights[2] * w_max / (3 * n_min)) / B
  logits, gt = tensors(c, 1, P)
  totals = []
  for step in range(4):
    leaves = {k: v.detach().clone().requires_grad_() for k, v in logits.items()}
    values, bad = loss.differentiable_losses(leaves, gt, weights, 'mean')
    totals.append(float(values[3].detach()))
    values[3].backward()
    logits = {k: (v.detach() - v.grad / lip) for k, v in leaves.items()}
  assert not bad.any()
  print('totals', totals)
  assert totals[1] < totals[0] and totals[2] < totals[1] and totals[3] < totals[2], totals


def test_capture_in_a_graph():
  from epos_amd import loss
  B, h, w, O, F = 2, 6, 7, 3, 8
  c = loss_cases.make_case(B, h * w, O, F, seed=15)
  logits, gt = tensors(c, h, w)
  sums, counts, _ = loss.loss_terms(logits, gt)
  values, scales = loss.loss_values(sums, counts, WEIGHTS, 'mean')
  eager = loss.loss_grads(logits, gt, scales)
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    out_v = (torch.zeros((4,), dtype=torch.float64, device='cuda'),
             torch.zeros((B, 3), dtype=torch.float64, device='cuda'))
    out_g = tuple(torch.full_like(logits[k], -7.0) for k in KEYS)
    loss.loss_values(sums, counts, WEIGHTS, 'mean', out=out_v)        # warm-up outside capture
    loss.loss_grads(logits, gt, out_v[1], out=out_g)
  torch.cuda.synchronize()
  for t in out_v + out_g:
    t.fill_(-7.0)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    loss.loss_values(sums, counts, WEIGHTS, 'mean', out=out_v)
    loss.loss_grads(logits, gt, out_v[1], out=out_g)
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(out_v[0], values) and torch.equal(out_v[1], scales)
  for a, b in zip(out_g, eager):
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_element_index_past_2_to_31():
  # O * F * 3 * P > 2^31: the last share's elements lie past a 32-bit index in d_loc (and its
  # frag_loc reads with them). Sparse foreground, so the check of all 2.1e9 elements stays on
  # the device; the last pixels against the same pixels as a small case of their own
  lib = _lib()
  O, F, K = 21, 64, 96
  P = 2 ** 31 // (O * F * 3) + 200
  assert P * O * F * 3 > 2 ** 31 and share_of(P, O, F) == 64
  gen = torch.Generator(device='cuda').manual_seed(16)
  obj = 4 * torch.randn((P, O + 1), device='cuda', generator=gen)
  frag = 4 * torch.randn((P, O, F), device='cuda', generator=gen)
  loc = torch.randn((P, O, F, 3), device='cuda', generator=gen)
  g_obj = torch.zeros((P,), dtype=torch.int32, device='cuda')
  g_obj[::997] = 1 + (torch.arange(0, P, 997, device='cuda') % O).int()
  g_obj[P - K:] = torch.randint(0, O + 1, (K,), device='cuda', generator=gen).int()
  g_obj[P - 1] = O
  g_frag = torch.randint(0, F, (P,), device='cuda', generator=gen).int()
  g_loc = torch.randn((P, 3), device='cuda', generator=gen)
  g_w = torch.rand((P,), device='cuda', generator=gen) + 0.5
  scale = np.array([[1.0 / P, 1e-3, 1e-2]])
  sc = torch.from_numpy(scale).cuda()
  d_frag = torch.full((P, O, F), float('nan'), device='cuda')
  d_loc = torch.full((P, O, F, 3), float('nan'), device='cuda')
  rc = lib.epos_loss_grads(_p(obj), O + 1, _p(frag), _p(loc), _p(g_obj), _p(g_frag), _p(g_loc),
                           _p(g_w), 1, P, O, F, IGNORE, _p(sc), None, None, O + 1, _p(d_frag),
                           _p(d_loc), _stream())
  assert rc == 0, lib.epos_last_error()
  torch.cuda.synchronize()
  # the last K pixels: the bytes of the same pixels as a batch of one of K pixels
  tail = slice(P - K, P)
  c = {'obj_logits': obj[tail].cpu().numpy()[None], 'frag_logits': frag[tail].cpu().numpy()[None],
       'frag_loc': loc[tail].cpu().numpy()[None], 'gt_obj': g_obj[tail].cpu().numpy()[None],
       'gt_frag': g_frag[tail].cpu().numpy()[None], 'gt_loc': g_loc[tail].cpu().numpy()[None],
       'gt_weight': g_w[tail].cpu().numpy()[None]}
  small = run_grads(c, scale)
  compare(small, c, scale)
  assert d_frag[tail].cpu().numpy().tobytes() == small[1].tobytes()
  assert d_loc[tail].cpu().numpy().tobytes() == small[2].tobytes()
  assert small[2][0, K - 1, O - 1].any()                 # the very last pixel's row is there
  # everything else: written, and zero outside the foreground pixels' rows
  fg = torch.nonzero(g_obj > 0).reshape(-1)
  assert 0 < fg.numel() < 4096
  rows = (g_obj[fg] - 1).long()
  frs = g_frag[fg].long()
  act_frag, act_loc = d_frag[fg, rows], d_loc[fg, rows, frs]
  assert torch.isfinite(act_frag).all() and torch.isfinite(act_loc).all()
  assert int(torch.count_nonzero(d_frag)) == int(torch.count_nonzero(act_frag)) > 0
  assert int(torch.count_nonzero(d_loc)) == int(torch.count_nonzero(act_loc)) > 0
