"""The loss reduction (csrc/loss.hip) through the C ABI against tests/helpers/loss_ref.py:
counts, bad-pixel counts and localisation sums exactly, cross-entropy sums to the derived
bound; head views, extreme logits, the Huber knee, the bad-pixel rules, determinism, refusals,
and LossEval over the launcher."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import loss_cases, loss_ref      # noqa: E402
from tests.helpers.loss_device import IGNORE, _lib, _off, _p, _stream      # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7


def run_terms(c, ignore=IGNORE, ld_obj=None, offsets=(0, 0, 0), outputs=None):
  """One call over a host case; returns (sums, counts, bad) as numpy arrays. ld_obj: the row
  stride of the object logits (default O+1); offsets: floats by which the three head views
  start behind a 16-byte boundary."""
  lib = _lib()
  B, P, O1 = c['obj_logits'].shape
  O, F = c['frag_logits'].shape[2:4]
  ld = O1 if ld_obj is None else ld_obj
  padded = np.full((B * P, ld), np.nan, np.float32)     # the padding must never be read
  padded[:, :O1] = c['obj_logits'].reshape(B * P, O1)
  obj = _off(padded, offsets[0])
  frag = _off(c['frag_logits'], offsets[1])
  loc = _off(c['frag_loc'], offsets[2])
  g_obj = torch.from_numpy(np.ascontiguousarray(c['gt_obj'], np.int32)).cuda()
  g_frag = torch.from_numpy(np.ascontiguousarray(c['gt_frag'], np.int32)).cuda()
  g_loc = torch.from_numpy(np.ascontiguousarray(c['gt_loc'], np.float32)).cuda()
  g_w = torch.from_numpy(np.ascontiguousarray(c['gt_weight'], np.float32)).cuda()
  nbytes = lib.epos_loss_workspace_bytes(B, P, O, F)
  assert nbytes > 0, lib.epos_last_error()
  ws = torch.full((nbytes // 8,), SENTINEL, dtype=torch.int64, device='cuda')
  if outputs is None:
    outputs = (torch.full((B, O1, 3), float(SENTINEL), dtype=torch.float64, device='cuda'),
               torch.full((B, O1, 2), SENTINEL, dtype=torch.int64, device='cuda'),
               torch.full((B,), SENTINEL, dtype=torch.int64, device='cuda'))
  sums, counts, bad = outputs
  rc = lib.epos_loss_terms(_p(obj), ld, _p(frag), _p(loc), _p(g_obj), _p(g_frag), _p(g_loc),
                           _p(g_w), B, P, O, F, ignore, _p(ws), _p(sums), _p(counts), _p(bad),
                           _stream())
  assert rc == 0, lib.epos_last_error()
  torch.cuda.synchronize()
  return sums.cpu().numpy(), counts.cpu().numpy(), bad.cpu().numpy()


def share_of(P, O, F):
  s = _lib().epos_loss_share_pixels(P, O, F)
  assert s >= 1
  return int(s)


def compare(got, exp, O, F):
  """Counts, bad and the localisation sums exactly (integers, and + - * only, in the helper's
  order); the cross-entropy sums to (row length + 16) 2^-52 (n + ref)."""
  (sums, counts, bad), (e_sums, e_counts, e_bad) = got, exp
  assert counts.dtype == np.int64 and counts.tobytes() == e_counts.tobytes()
  assert bad.tobytes() == e_bad.tobytes()
  assert sums[:, :, 2].tobytes() == e_sums[:, :, 2].tobytes()
  assert (sums[:, 0, 1:] == 0).all()                      # background has no fragment terms
  for k, row_len in enumerate(loss_ref.row_lengths(O, F)):
    for b in range(sums.shape[0]):
      for g in range(O + 1):
        ref, n = e_sums[b, g, k], int(e_counts[b, g, 0])
        err = abs(sums[b, g, k] - ref)
        assert err <= loss_ref.ce_bound(row_len, n, ref), (b, g, k, sums[b, g, k], ref, n)


def take(c, images):
  return {k: np.ascontiguousarray(v[list(images)]) for k, v in c.items()}


@pytest.mark.parametrize('O', [1, 3, 21])
@pytest.mark.parametrize('F', [1, 3, 4, 63, 64, 65, 256])
def test_sweep(F, O):
  share = share_of(64, O, F)
  sizes = [share - 1, share, share + 1, 1]
  assert all(share_of(P, O, F) == share for P in sizes)   # P = one share - 1, one share, + 1
  for P in sizes:
    c = loss_cases.make_case(3, P, O, F, seed=1000 * F + 10 * O + (P % 7), empty_images=(1,))
    exp = loss_cases.ref_terms(loss_ref, c, share)
    got = run_terms(c)
    compare(got, exp, O, F)
    assert exp[2].sum() == 0 and exp[1][1, 1:, 0].sum() == 0
    if P >= 8:
      assert exp[1][0, 0, 1] > 0 and (exp[1][[0, 2], 1:, 0].sum(axis=1) > 0).all()
    # B = 1: image 0 alone, the same bytes as in the batch
    one = run_terms(take(c, [0]))
    compare(one, tuple(a[:1] for a in exp), O, F)
    for a, b in zip(one, got):
      assert a[0].tobytes() == b[0].tobytes()


@pytest.mark.parametrize('offsets,ld_extra', [((1, 0, 0), 0), ((0, 1, 0), 0), ((0, 0, 1), 0),
                                              ((1, 1, 1), 3), ((0, 0, 0), 2), ((0, 0, 0), 5),
                                              ((2, 3, 2), 1)])
def test_head_views(offsets, ld_extra):
  # O+1 = 22 with ld 24: 16-byte rows with a scalar tail; ld 22 / 23 / 25 / 27: scalar rows
  B, O, F = 2, 21, 64
  P = share_of(64, O, F) + 3
  c = loss_cases.make_case(B, P, O, F, seed=5)
  exp = loss_cases.ref_terms(loss_ref, c, share_of(P, O, F))
  base = run_terms(c)
  compare(base, exp, O, F)
  got = run_terms(c, ld_obj=O + 1 + ld_extra, offsets=offsets)
  compare(got, exp, O, F)
  # a lane's values and the butterfly do not depend on the load width
  for a, b in zip(got, base):
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('F', [5, 64])
def test_extreme_logits(F):
  # the target 200 below the maximum, every other logit 1e4 below it: p(target) = 1.4e-87 is
  # 0 in fp32, so a cross-entropy taken from probabilities is inf; from logits it is 200
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
  exp = loss_cases.ref_terms(loss_ref, c, share_of(P, O, F))
  sums, counts, bad = run_terms(c)
  compare((sums, counts, bad), exp, O, F)
  assert np.isfinite(sums).all()
  n = counts[0, :, 0]
  assert (exp[0][0, :, 0] == 200.0 * n).all() and (exp[0][0, 1:, 1] == 200.0 * n[1:]).all()
  assert n[1:].sum() > 0


def test_huber_knee():
  # differences exactly at +-1 and +-(1 + 2^-23), and around them, in every coordinate
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
  exp = loss_cases.ref_terms(loss_ref, c, share_of(P, O, F))
  got = run_terms(c)
  compare(got, exp, O, F)
  # the same terms by hand, object by object in pixel order
  hand = np.zeros(O + 1)
  for p in range(P):
    x = float(d[p // 3])
    hand[c['gt_obj'][0, p]] += 0.5 * x * x if abs(x) <= 1.0 else abs(x) - 0.5
  assert got[0][0, :, 2].tolist() == hand.tolist()
  # gt on the other side: the same differences with the other sign
  c['gt_loc'], c['frag_loc'] = c['gt_loc'] + 0, c['frag_loc'] + 0
  for p in range(P):
    g, f = c['gt_obj'][0, p] - 1, c['gt_frag'][0, p]
    c['gt_loc'][0, p] = c['frag_loc'][0, p, g, f]
    c['frag_loc'][0, p, g, f] = 0.0
  assert run_terms(c)[0][0, :, 2].tolist() == hand.tolist()


def _tiny(O=3, F=5, P=12, seed=4):
  c = loss_cases.make_case(1, P, O, F, seed=seed, ignore_band=False)
  c['gt_obj'][0] = np.arange(P) % (O + 1)
  fg = c['gt_obj'][0] > 0
  c['gt_frag'][0] = np.where(fg, np.arange(P) % F, -1)
  c['gt_weight'][0] = np.where(fg, 1.0, 0.0)
  return c


@pytest.mark.parametrize('rule', ['obj_low', 'obj_high', 'obj_far', 'frag_low', 'frag_high',
                                  'w_zero', 'w_neg', 'w_inf', 'w_nan'])
def test_bad_pixel_rules(rule):
  O, F, P = 3, 5, 12
  c = _tiny(O, F, P)
  good = run_terms(c)
  assert good[2][0] == 0
  p = 5                                   # an object-1 pixel (5 % 4 == 1)
  assert c['gt_obj'][0, p] == 1
  if rule.startswith('obj'):
    c['gt_obj'][0, p] = {'obj_low': -1, 'obj_high': O + 1, 'obj_far': -2 ** 31}[rule]
  elif rule.startswith('frag'):
    c['gt_frag'][0, p] = {'frag_low': -1, 'frag_high': F}[rule]
  else:
    c['gt_weight'][0, p] = {'w_zero': 0.0, 'w_neg': -1.0, 'w_inf': np.inf, 'w_nan': np.nan}[rule]
  exp = loss_cases.ref_terms(loss_ref, c, share_of(P, O, F))
  got = run_terms(c)
  compare(got, exp, O, F)
  assert got[2][0] == 1 and got[1][0, 1, 0] == good[1][0, 1, 0] - 1
  assert got[0][0, 1, 0] < good[0][0, 1, 0]               # the pixel added nothing at all
  # background reads neither the fragment label nor the weight
  c2 = _tiny(O, F, P)
  c2['gt_frag'][0, 4], c2['gt_weight'][0, 4] = F + 3, np.nan
  assert c2['gt_obj'][0, 4] == 0
  assert all(a.tobytes() == b.tobytes() for a, b in zip(run_terms(c2), good))
  # the ignore rule wins: the same pixel with the ignore label on top is ignored, not bad
  if not rule.startswith('obj'):
    c['gt_obj'][0, p] = IGNORE
    got = run_terms(c)
    assert got[2][0] == 0 and got[1][0, 0, 1] == 1
  # an ignore label inside 0..O: the ignore rule comes first, its row stays empty
  got = run_terms(_tiny(O, F, P), ignore=2)
  exp = loss_cases.ref_terms(loss_ref, _tiny(O, F, P), share_of(P, O, F), ignore=2)
  compare(got, exp, O, F)
  assert got[1][0, 2, 0] == 0 and got[1][0, 0, 1] == 3 and (got[0][0, 2] == 0).all()


@pytest.mark.parametrize('where', ['obj', 'frag', 'loc'])
def test_non_finite_logit_marks_its_image_only(where):
  B, O, F = 3, 3, 8
  P = share_of(64, O, F) + 9
  c = loss_cases.make_case(B, P, O, F, seed=6)
  exp = loss_cases.ref_terms(loss_ref, c, share_of(P, O, F))
  p = P - 1                                # an object-1 pixel of image 1 (make_case)
  assert c['gt_obj'][1, p] == 1
  f = c['gt_frag'][1, p]
  if where == 'obj':
    c['obj_logits'][1, p, 2] = np.nan
  elif where == 'frag':
    c['frag_logits'][1, p, 0, (f + 1) % F] = np.nan
  else:
    c['frag_loc'][1, p, 0, f, 1] = np.inf
  sums, counts, bad = run_terms(c)
  k = {'obj': 0, 'frag': 1, 'loc': 2}[where]
  assert not np.isfinite(sums[1, 1, k]) and bad.tolist() == [0, 0, 0]
  finite = np.ones_like(sums, bool)
  finite[1, 1, k] = False
  assert np.isfinite(sums[finite]).all()
  assert counts.tobytes() == exp[1].tobytes()
  compare((sums[[0, 2]], counts[[0, 2]], bad[[0, 2]]), tuple(a[[0, 2]] for a in exp), O, F)
  from epos_amd import loss
  from epos_amd._lib import EposError
  with pytest.raises(EposError, match=r'^Loss is inf or nan\.$'):
    loss.summarize(sums, counts, bad, (1.0, 1.0, 100.0), O)


@pytest.mark.parametrize('O,F', [(3, 64), (21, 5)])
def test_determinism(O, F):
  share = share_of(64, O, F)
  P = 2 * share + 5                        # three workgroups per image, the last one short
  assert share_of(P, O, F) == share
  c = loss_cases.make_case(3, P, O, F, seed=7, empty_images=(2,))
  first = run_terms(c)
  compare(first, loss_cases.ref_terms(loss_ref, c, share), O, F)
  again = run_terms(c)
  for a, b in zip(first, again):
    assert a.tobytes() == b.tobytes()
  for i in range(3):
    alone = run_terms(take(c, [i]))
    for pos in range(3):                   # image i at position pos of a batch of 3
      order = [(i - pos + j) % 3 for j in range(3)]
      assert order[pos] == i
      batch = run_terms(take(c, order))
      for a, b in zip(alone, batch):
        assert a[0].tobytes() == b[pos].tobytes(), (i, pos)


def test_refusals_come_before_any_launch():
  lib = _lib()
  O, F, P = 3, 5, 10
  c = loss_cases.make_case(1, P, O, F, seed=8)
  t = {k: torch.from_numpy(v).cuda() for k, v in c.items()}
  ws = torch.full((1024,), SENTINEL, dtype=torch.int64, device='cuda')
  sums = torch.full((1, O + 1, 3), float(SENTINEL), dtype=torch.float64, device='cuda')
  counts = torch.full((1, O + 1, 2), SENTINEL, dtype=torch.int64, device='cuda')
  bad = torch.full((1,), SENTINEL, dtype=torch.int64, device='cuda')

  def call(B=1, P=P, O=O, F=F, ld=O + 1, obj=t['obj_logits'], out=sums):
    return lib.epos_loss_terms(
        _p(obj), ld, _p(t['frag_logits']), _p(t['frag_loc']), _p(t['gt_obj']), _p(t['gt_frag']),
        _p(t['gt_loc']), _p(t['gt_weight']), B, P, O, F, IGNORE, _p(ws), _p(out), _p(counts),
        _p(bad), _stream())
  for kwargs, msg in (({'O': 0}, b'num_objs must be in 1..4095'),
                      ({'O': 4096}, b'num_objs must be in 1..4095'),
                      ({'F': 0}, b'num_frags must be in 1..256'),
                      ({'F': 257}, b'num_frags must be in 1..256'),
                      ({'ld': O}, b'ld_obj must be >= num_objs + 1'),
                      ({'obj': None}, b'null pointer'),
                      ({'out': None}, b'null pointer'),
                      ({'B': -1}, b'B must be >= 0'),
                      ({'P': -1}, b'P must be in 0..2^31')):
    assert call(**kwargs) == -1, kwargs
    assert lib.epos_last_error() == b'epos_loss_terms: ' + msg
  # the empty batch and the empty image do nothing, null pointers included
  assert call(B=0) == 0 and call(P=0) == 0 and call(B=0, obj=None, out=None) == 0
  torch.cuda.synchronize()
  for x in (ws, counts, bad):
    assert (x == SENTINEL).all()
  assert (sums == float(SENTINEL)).all()
  assert call() == 0                       # and the same arguments, unchanged, run
  torch.cuda.synchronize()
  assert int(bad[0]) == 0 and int(counts.sum()) == P


def test_loss_eval_over_batches_equals_the_helper_on_the_concatenation():
  from epos_amd import loss
  O, F, h, w = 3, 5, 4, 5
  P = h * w
  weights = (0.5, 2.0, 100.0)
  sizes = [2, 3, 17]                       # the third batch outgrows the table's first 16 rows
  c = loss_cases.make_case(sum(sizes), P, O, F, seed=9, empty_images=(3,))
  ev = loss.LossEval(O, F, 'cuda:0', *weights)
  i0 = 0
  for n in sizes:
    part = take(c, range(i0, i0 + n))
    logits = {'pred_obj_conf': torch.from_numpy(part['obj_logits']).cuda().view(n, h, w, O + 1),
              'pred_frag_conf': torch.from_numpy(part['frag_logits']).cuda().view(n, h, w, O, F),
              'pred_frag_loc': torch.from_numpy(part['frag_loc']).cuda().view(n, h, w, O, F, 3)}
    gt = {'obj_label': torch.from_numpy(part['gt_obj']).cuda().view(n, h, w),
          'frag_label': torch.from_numpy(part['gt_frag']).cuda().view(n, h, w),
          'frag_loc': torch.from_numpy(part['gt_loc']).cuda().view(n, h, w, 3),
          'frag_weight': torch.from_numpy(part['gt_weight']).cuda().view(n, h, w)}
    ev.update(logits, gt)
    i0 += n
  res = ev.result()
  exp = loss_ref.dataset_losses(*loss_cases.ref_terms(loss_ref, c, share_of(P, O, F))[:2],
                                weights=weights)
  assert len(res['per_image']) == sum(sizes) and ev.rows == sum(sizes)

  def close(got, ref, w_k, row_len):
    # a mean of cross-entropy sums within (row + 16) 2^-52 (n + sum) each, i.e. per pixel
    # (row + 16) 2^-52 (1 + loss / w), plus one rounding on either side for each of the host's
    # additions (O + 1 objects, at most all the images), its product and its division
    tol = (w_k * (row_len + 16) * 2.0 ** -52 * (1 + ref / w_k) +
           (O + 4 + sum(sizes)) * 2.0 ** -52 * ref)
    assert abs(got - ref) <= tol, (got, ref, tol)
  for got, ref in list(zip(res['per_image'], exp['per_image'])) + [
      (res['mean'], exp['mean']), (res['pooled'], exp['pooled'])]:
    close(got['obj_cls_loss'], ref['obj_cls_loss'], weights[0], O + 1)
    close(got['frag_cls_loss'], ref['frag_cls_loss'], weights[1], F)
    assert got['frag_loc_loss'] == ref['frag_loc_loss']      # + - * / in one order on both sides
    parts = (got['obj_cls_loss'] + got['frag_cls_loss']) + got['frag_loc_loss']
    if got is res['mean']:               # the mean of the totals, not the total of the means
      assert abs(got['total_loss'] - parts) <= (sum(sizes) + 4) * 2.0 ** -52 * parts
    else:
      assert got['total_loss'] == parts
  assert res['per_image'][3]['frag_cls_loss'] == 0.0
  for g in range(1, O + 1):
    assert res['per_object'][g]['pixels'] == exp['per_object'][g]['pixels'] > 0
    assert res['per_object'][g]['frag_loc_loss'] == exp['per_object'][g]['frag_loc_loss']
    close(res['per_object'][g]['frag_cls_loss'], exp['per_object'][g]['frag_cls_loss'],
          weights[1], F)
  # a bad pixel is reported with its count
  part = take(c, [0])
  part['gt_frag'][0, P - 1] = F
  ev.update({'pred_obj_conf': torch.from_numpy(part['obj_logits']).cuda(),
             'pred_frag_conf': torch.from_numpy(part['frag_logits']).cuda(),
             'pred_frag_loc': torch.from_numpy(part['frag_loc']).cuda()},
            {'obj_label': torch.from_numpy(part['gt_obj']).cuda(),
             'frag_label': torch.from_numpy(part['gt_frag']).cuda(),
             'frag_loc': torch.from_numpy(part['gt_loc']).cuda(),
             'frag_weight': torch.from_numpy(part['gt_weight']).cuda()})
  from epos_amd._lib import EposError
  with pytest.raises(EposError, match=r'^1 pixel\(s\)'):
    ev.result()
