"""The evaluation reductions (csrc/eval.hip) against tests/helpers/eval_ref.py, exactly: the
confusion matrix in both of its regimes, accumulation, the fragment hit counts, the launchers'
argument checks, and SegmentationEval over them."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import eval_ref, mesh_cases, render_ref as rr      # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 29, 37                   # odd, no multiple of 64 or of a vector width
IGNORE = 255


def _p(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
  from epos_amd import _lib as binding
  return binding.load()


def _num_cls(spec):
  lim = _lib().epos_eval_lds_max_cls()
  return {'lds': lim, 'lds+1': lim + 1}.get(spec, spec)


def run_confusion(gt, pred, num_cls, ignore=IGNORE, cm=None, bad=None):
  """One launch over host labels; returns the device tables (given ones are added to)."""
  g = torch.from_numpy(np.ascontiguousarray(gt, np.int32).reshape(-1)).cuda()
  q = torch.from_numpy(np.ascontiguousarray(pred, np.int64).reshape(-1)).cuda()
  cm = torch.zeros((num_cls, num_cls), dtype=torch.int64, device='cuda') if cm is None else cm
  bad = torch.zeros((1,), dtype=torch.int64, device='cuda') if bad is None else bad
  rc = _lib().epos_eval_confusion(_p(g), _p(q), g.numel(), num_cls, ignore, _p(cm), _p(bad),
                                  _stream())
  assert rc == 0, _lib().epos_last_error()
  torch.cuda.synchronize()
  return cm, bad


def check_confusion(gt, pred, num_cls, ignore=IGNORE):
  cm, bad = run_confusion(gt, pred, num_cls, ignore)
  exp, exp_bad = eval_ref.confusion(gt, pred, num_cls, ignore)
  got = cm.cpu().numpy()
  assert got.dtype == np.int64 and got.tobytes() == exp.tobytes()
  assert int(bad.cpu()[0]) == exp_bad
  return exp, exp_bad


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('spec', [1, 2, 22, 31, 'lds', 'lds+1', 256])
def test_confusion_matrix(spec, batch):
  num_cls = _num_cls(spec)
  P = batch * H * W
  rng = np.random.RandomState(num_cls * 7 + batch)
  gt = rng.randint(0, num_cls, P)
  pred = rng.randint(0, num_cls, P)
  # 255 is a class of its own at num_cls = 256: there the ignore rule wins (checked below too)
  exp, bad = check_confusion(gt, pred, num_cls)
  assert bad == 0 and exp.sum() == P - (gt == IGNORE).sum()
  # every pixel on one pair: the worst contention
  a, b = num_cls - 1, num_cls // 2
  exp, _ = check_confusion(np.full(P, a), np.full(P, b), num_cls, ignore=-1)
  assert exp[a, b] == P
  # every pixel ignored
  exp, bad = check_confusion(np.full(P, IGNORE), pred, num_cls)
  assert exp.sum() == 0 and bad == 0
  # about 5 % of the labels out of range, on either side and far beyond 32 bits
  gt2, pred2 = gt.astype(np.int64), pred.astype(np.int64)
  out = rng.rand(P) < 0.05
  gt_out = np.array([v for v in (-1, -7, num_cls, num_cls + 7, 2 ** 31 - 1, -2 ** 31)
                     if v != IGNORE])
  side = rng.rand(P) < 0.5
  gt2[out & side] = gt_out[rng.randint(0, len(gt_out), int((out & side).sum()))]
  pred_out = np.array([-1, num_cls, num_cls + 300, 2 ** 40, -2 ** 35, 2 ** 32, 2 ** 32 + 1])
  pred2[out & ~side] = pred_out[rng.randint(0, len(pred_out), int((out & ~side).sum()))]
  exp, bad = check_confusion(gt2, pred2, num_cls)
  assert bad > 0 and exp.sum() + bad + ((gt2 == IGNORE).sum()) == P
  # an ignore label inside 0..num_cls-1: the ignore rule wins, its row stays empty
  ign = num_cls // 2
  exp, bad = check_confusion(gt, pred, num_cls, ignore=ign)
  assert exp[ign].sum() == 0 and bad == 0 and exp.sum() == (gt != ign).sum()


@pytest.mark.parametrize('spec', [22, 'lds+1'])
def test_confusion_accumulates(spec):
  num_cls = _num_cls(spec)
  rng = np.random.RandomState(5)
  P = H * W
  parts = [(rng.randint(0, num_cls, P), rng.randint(-1, num_cls, P)) for _ in range(2)]
  cm = torch.zeros((num_cls, num_cls), dtype=torch.int64, device='cuda')
  cm[3, 5] = 2 ** 31 - 5                       # a preloaded cell crosses 2^31 exactly
  parts[0][0][:40], parts[0][1][:40] = 3, 5
  bad = torch.zeros((1,), dtype=torch.int64, device='cuda')
  exp = np.zeros((num_cls, num_cls), np.int64)
  exp[3, 5] = 2 ** 31 - 5
  exp_bad = 0
  for gt, pred in parts:
    run_confusion(gt, pred, num_cls, cm=cm, bad=bad)
    c, b = eval_ref.confusion(gt, pred, num_cls, IGNORE)
    exp += c
    exp_bad += b
  assert cm.cpu().numpy().tobytes() == exp.tobytes()
  assert exp[3, 5] >= 2 ** 31 + 35 and exp_bad > 0
  assert int(bad.cpu()[0]) == exp_bad


@pytest.mark.parametrize('spec', [22, 256])
def test_confusion_large_single_pair(spec):
  """2^22 pixels on one pair: every workgroup counts a full pixel share (the bound that keeps
  its 32-bit counters from wrapping) and the shares add up across workgroups."""
  num_cls = _num_cls(spec)
  P = 1 << 22
  cm, bad = run_confusion(np.full(P, 3, np.int32), np.full(P, 5, np.int64), num_cls)
  exp = np.zeros((num_cls, num_cls), np.int64)
  exp[3, 5] = P                                # by hand: every pixel is the pair (3, 5)
  assert cm.cpu().numpy().tobytes() == exp.tobytes() and int(bad.cpu()[0]) == 0


# ---------------------------------------------------------------- fragment hits ---
def _rot(axis, angle):
  axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
  a, b, c = axis
  S = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]])
  return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


@pytest.fixture(scope='module')
def field_inputs():
  """The field of tests/test_gpu_render.py: three overlapping instances (objects 2, 1, 2) at
  37x29, rendered by the reference."""
  verts, faces = mesh_cases.icosphere(1, 30.0)
  ts = [np.array([0.0, 0.0, 300.0]), np.array([14.0, 5.0, 340.0]), np.array([-9.0, 6.0, 280.0])]
  outs = [rr.render(verts, faces, None, _rot([1, 1, 0], 0.3 * i), t, 100.0, 100.0, 18.0, 14.0,
                    H, W) for i, t in enumerate(ts)]
  depth = np.stack([o['depth'] for o in outs])
  local = np.stack([o['local_pos'] for o in outs])
  masks = np.random.RandomState(0).rand(3, H, W) < 0.8
  return depth, local, masks, [2, 1, 2]


def frag_case(field_inputs, O, F):
  """Label maps of the field for F fragments, with an ignored patch and an id beyond every O,
  and confidences with the planted rows."""
  depth, local, masks, obj_ids = field_inputs
  rng = np.random.RandomState(100 * O + F)
  centers = rng.uniform(-30, 30, (3, F, 3))
  f = rr.gt_fields(depth, local, masks, obj_ids, centers, rng.uniform(4, 15, (3, F)))
  gt_obj = f['obj_label'].copy().reshape(-1)
  gt_frag = f['frag_label'].copy().reshape(-1)
  assert set(np.unique(gt_obj)) == {0, 1, 2}
  fg = np.nonzero(gt_obj > 0)[0]
  gt_obj[fg[:5]] = IGNORE
  gt_obj[fg[5:9]] = 7                                 # outside 1..O for every O tested
  gt_obj[fg[9]] = -3
  P = H * W
  conf = rng.rand(P, O, F).astype(np.float32)
  pred_obj = rng.randint(0, O + 1, P).astype(np.int64)
  rows = [p for p in fg[10:] if 1 <= gt_obj[p] <= O]
  assert len(rows) > 40
  # half of the remaining rows are hits by construction, and there the prediction mostly agrees
  for p in rows[::2]:
    conf[p, gt_obj[p] - 1, gt_frag[p]] = 2.0
    if p % 3:
      pred_obj[p] = gt_obj[p]
  if F > 1:
    p, o = rows[0], gt_obj[rows[0]] - 1               # a tie: the first maximum wins
    conf[p, o, :] = 0.1
    conf[p, o, [F // 3, F - 1]] = 5.0
    gt_frag[p] = F // 3
    p, o = rows[1], gt_obj[rows[1]] - 1               # the same tie, the label on the loser
    conf[p, o, :] = 0.1
    conf[p, o, [F // 3, F - 1]] = 5.0
    gt_frag[p] = F - 1
    p, o = rows[2], gt_obj[rows[2]] - 1               # a NaN ahead of the maximum
    conf[p, o, :] = 0.2
    conf[p, o, 0] = np.nan
    conf[p, o, F - 1] = 0.9
    gt_frag[p] = F - 1
    p, o = rows[3], gt_obj[rows[3]] - 1               # NaNs around a maximum in the middle
    conf[p, o, :] = np.nan
    conf[p, o, F // 2] = -4.0
    gt_frag[p] = F // 2
  p, o = rows[4], gt_obj[rows[4]] - 1                 # all equal: fragment 0
  conf[p, o, :] = 0.5
  gt_frag[p] = 0
  p, o = rows[5], gt_obj[rows[5]] - 1                 # nothing but NaN: fragment 0 by definition
  conf[p, o, :] = np.nan
  gt_frag[p] = 0
  return gt_obj.astype(np.int32), gt_frag.astype(np.int32), pred_obj, conf


def run_frag_hits(gt_obj, gt_frag, pred_obj, conf, O, F, counts=None):
  t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None
       for a in (gt_obj, gt_frag, pred_obj, conf)]
  counts = torch.zeros((O + 1, 3), dtype=torch.int64, device='cuda') if counts is None else counts
  rc = _lib().epos_eval_frag_hits(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), len(gt_obj), O, F,
                                  IGNORE, _p(counts), _stream())
  assert rc == 0, _lib().epos_last_error()
  torch.cuda.synchronize()
  return counts


@pytest.mark.parametrize('F', [1, 63, 64, 65, 256])
@pytest.mark.parametrize('O', [1, 3])
def test_frag_hits(field_inputs, O, F):
  gt_obj, gt_frag, pred_obj, conf = frag_case(field_inputs, O, F)
  exp = eval_ref.frag_hits(gt_obj, gt_frag, pred_obj, conf, O, IGNORE)
  got = run_frag_hits(gt_obj, gt_frag, pred_obj, conf, O, F).cpu().numpy()
  assert got.dtype == np.int64 and got.tobytes() == exp.tobytes()
  assert (exp[0] == 0).all() and exp[1, 0] > 0
  assert (exp[:, 0] >= exp[:, 1]).all() and (exp[:, 1] >= exp[:, 2]).all()
  assert exp[:, 2].sum() > 0 and exp[:, 1].sum() > exp[:, 2].sum()
  if F > 1:
    assert exp[:, 0].sum() > exp[:, 1].sum()           # the planted loser, at least
  # no predicted labels: column 2 is left as it was; a second call adds to the first
  counts = torch.zeros((O + 1, 3), dtype=torch.int64, device='cuda')
  counts[:, 2] = 11
  for _ in range(2):
    run_frag_hits(gt_obj, gt_frag, None, conf, O, F, counts)
  twice = np.stack([2 * exp[:, 0], 2 * exp[:, 1], np.full(O + 1, 11)], axis=1)
  assert counts.cpu().numpy().tobytes() == twice.astype(np.int64).tobytes()


def test_frag_hits_unaligned_confidences(field_inputs):
  """A confidence tensor that starts 4 bytes off a 16-byte boundary takes the scalar loads."""
  O, F = 3, 64
  gt_obj, gt_frag, pred_obj, conf = frag_case(field_inputs, O, F)
  exp = eval_ref.frag_hits(gt_obj, gt_frag, pred_obj, conf, O, IGNORE)
  buf = torch.zeros(conf.size + 1, dtype=torch.float32, device='cuda')
  view = buf[1:]
  view.copy_(torch.from_numpy(conf.reshape(-1)))
  assert view.data_ptr() % 16 == 4
  t = [torch.from_numpy(a).cuda() for a in (gt_obj, gt_frag, pred_obj)]
  counts = torch.zeros((O + 1, 3), dtype=torch.int64, device='cuda')
  assert _lib().epos_eval_frag_hits(_p(t[0]), _p(t[1]), _p(t[2]), _p(view), len(gt_obj), O, F,
                                    IGNORE, _p(counts), _stream()) == 0
  torch.cuda.synchronize()
  assert counts.cpu().numpy().tobytes() == exp.tobytes()


# ---------------------------------------------------------------- argument checks ---
def test_eval_launchers_refuse_invalid_arguments():
  """Return codes only: every refusal happens before anything is launched."""
  lib = _lib()
  dev = 'cuda:0'
  gt = torch.zeros((16,), dtype=torch.int32, device=dev)
  fr = torch.zeros((16,), dtype=torch.int32, device=dev)
  pred = torch.zeros((16,), dtype=torch.int64, device=dev)
  cm = torch.zeros((256, 256), dtype=torch.int64, device=dev)
  bad = torch.zeros((1,), dtype=torch.int64, device=dev)
  conf = torch.zeros((16, 2, 256), dtype=torch.float32, device=dev)
  counts = torch.zeros((3, 3), dtype=torch.int64, device=dev)
  s = _stream()
  E = -1                                            # EPOS_E_INVALID

  def confusion(g=_p(gt), q=_p(pred), P=16, n=22, c=_p(cm), b=_p(bad)):
    return lib.epos_eval_confusion(g, q, P, n, IGNORE, c, b, s)
  assert confusion() == 0
  for kw in (dict(g=None), dict(q=None), dict(c=None), dict(b=None), dict(P=-1), dict(n=0),
             dict(n=-1), dict(n=257)):
    assert confusion(**kw) == E, kw
  assert b'epos_eval_confusion' in lib.epos_last_error()
  assert confusion(n=256) == 0 and confusion(n=1) == 0
  assert confusion(P=0, g=None, q=None, c=None, b=None) == 0      # nothing to do

  def hits(g=_p(gt), f=_p(fr), q=_p(pred), x=_p(conf), P=16, O=2, F=64, c=_p(counts)):
    return lib.epos_eval_frag_hits(g, f, q, x, P, O, F, IGNORE, c, s)
  assert hits() == 0
  for kw in (dict(g=None), dict(f=None), dict(x=None), dict(c=None), dict(P=-1), dict(O=0),
             dict(O=-2), dict(F=0), dict(F=257)):
    assert hits(**kw) == E, kw
  assert b'epos_eval_frag_hits' in lib.epos_last_error()
  assert hits(q=None) == 0 and hits(F=256) == 0 and hits(F=1) == 0
  assert hits(P=0, g=None, f=None, q=None, x=None, c=None) == 0
  torch.cuda.synchronize()
  assert int(bad.cpu()[0]) == 0 and int(cm.sum().cpu()) == 3 * 16   # the three launches above


# ---------------------------------------------------------------- SegmentationEval ---
def test_segmentation_eval_over_two_batches(field_inputs):
  from epos_amd import eval_utils
  from epos_amd._lib import EposError
  O, F = 3, 64
  gt_obj, gt_frag, pred_obj, conf = frag_case(field_inputs, O, F)
  gt_obj = np.where((gt_obj == 7) | (gt_obj == -3), 0, gt_obj).astype(np.int32)
  rng = np.random.RandomState(9)
  second = (rng.permutation(gt_obj), rng.permutation(gt_frag),
            rng.randint(0, O + 1, len(gt_obj)).astype(np.int64),
            rng.rand(*conf.shape).astype(np.float32))
  ev = eval_utils.SegmentationEval(O, ignore_label=IGNORE, device='cuda:0', num_frags=F)
  exp_cm = np.zeros((O + 1, O + 1), np.int64)
  exp_counts = np.zeros((O + 1, 3), np.int64)
  for shape, (g, fl, q, c) in (((1, H, W), (gt_obj, gt_frag, pred_obj, conf)),
                               ((H, W), second)):
    ev.update(torch.from_numpy(g.reshape(shape)).cuda(), torch.from_numpy(q.reshape(shape)).cuda(),
              torch.from_numpy(fl.reshape(shape)).cuda(),
              torch.from_numpy(c.reshape(shape + (O, F))).cuda())
    cm, bad = eval_ref.confusion(g, q, O + 1, IGNORE)
    assert bad == 0
    exp_cm += cm
    exp_counts += eval_ref.frag_hits(g, fl, q, c, O, IGNORE)
  got = ev.confusion_matrix()
  assert got.dtype == np.int64 and got.tobytes() == exp_cm.tobytes()
  assert ev.miou() == pytest.approx(eval_ref.miou(exp_cm), abs=1e-15)
  fa = ev.frag_accuracy()
  assert fa['per_object'] == {o: tuple(int(v) for v in exp_counts[o]) for o in range(1, O + 1)}
  assert fa['frag_acc'] == exp_counts[1:, 1].sum() / float(exp_counts[1:, 0].sum())
  assert fa['frag_acc_seg'] == exp_counts[1:, 2].sum() / float(exp_counts[1:, 0].sum())
  # a label outside 0..O is an error at the end, as the reference's IndexError would be
  g = gt_obj.copy()
  g[0] = O + 1
  ev.update(torch.from_numpy(g).cuda(), torch.from_numpy(pred_obj).cuda())
  with pytest.raises(EposError, match='outside'):
    ev.confusion_matrix()
