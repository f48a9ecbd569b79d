"""Host side of eval_loss.py: the numpy restatement of the loss rules against torch's
cross_entropy and huber_loss in fp64 and against hand-computed values, mean versus pooled, the
binding of the loss symbols, the command line, and the errors of LossEval.result."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import loss_cases, loss_ref      # noqa: E402

IGNORE = loss_cases.IGNORE
WEIGHTS = (1.0, 1.0, 100.0)


def torch_image_losses(c, b, O, F, weights):
  """One image as the reference's batch of one, in torch fp64 on the CPU: the gather / mean
  structure of epos_lib/loss.py -- every pixel's object cross-entropy weighted by the
  not-ignored mask and averaged over all pixels; the foreground pixels gathered, their
  fragment cross-entropy against the normalised target distribution averaged, their Huber
  losses weighted and averaged over pixels x 3."""
  TF = torch.nn.functional
  w_obj, w_cls, w_loc = weights
  gt = torch.from_numpy(c['gt_obj'][b].astype(np.int64))
  logits = torch.from_numpy(c['obj_logits'][b]).double()
  keep = gt != IGNORE
  ce = TF.cross_entropy(logits, torch.where(keep, gt, torch.zeros_like(gt)), reduction='none')
  obj = (ce * keep.double() * w_obj).mean()
  fg = torch.nonzero(keep & (gt > 0)).reshape(-1)
  if fg.numel() == 0:
    return float(obj), 0.0, 0.0
  objs = gt[fg] - 1
  frag = torch.from_numpy(c['gt_frag'][b].astype(np.int64))[fg]
  wgt = torch.from_numpy(c['gt_weight'][b]).double()[fg]
  rows = torch.from_numpy(c['frag_logits'][b]).double()[fg, objs]          # [n, F]
  distrib = torch.zeros((fg.numel(), F), dtype=torch.float64)
  distrib[torch.arange(fg.numel()), frag] = wgt
  distrib = distrib / distrib.sum(dim=1, keepdim=True)
  cls = (TF.cross_entropy(rows, distrib, reduction='none') * w_cls).mean()
  pred = torch.from_numpy(c['frag_loc'][b]).double()[fg, objs, frag]       # [n, 3]
  target = torch.from_numpy(c['gt_loc'][b]).double()[fg]
  hub = TF.huber_loss(pred, target, delta=1.0, reduction='none') * w_loc
  loc = (hub * wgt.reshape(-1, 1)).mean()
  return float(obj), float(cls), float(loc)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_helper_agrees_with_torch_fp64(seed):
  B, P, O, F = 3, 61, 3, 5
  c = loss_cases.make_case(B, P, O, F, seed, empty_images=(1,))
  weights = (0.7, 1.3, 100.0)
  sums, counts, bad = loss_cases.ref_terms(loss_ref, c, share=16)
  assert bad.tolist() == [0, 0, 0]
  assert (counts[:, 0, 1] == (c['gt_obj'] == IGNORE).sum(axis=1)).all() and counts[0, 0, 1] > 0
  assert counts[1, 1:, 0].sum() == 0 and (counts[0, 1:, 0] > 0).sum() >= 2
  for b in range(B):
    got = loss_ref.image_losses(sums[b], counts[b], weights)
    exp = torch_image_losses(c, b, O, F, weights)
    # both sides are fp64 sums of P (or 3 n_fg) non-negative terms of a few ulp each
    for name, e in zip(loss_ref.NAMES, exp):
      assert got[name] == pytest.approx(e, rel=64 * P * 2.0 ** -52, abs=0.0), (b, name)
    assert got['total_loss'] == (got['obj_cls_loss'] + got['frag_cls_loss']) + got['frag_loc_loss']
  assert loss_ref.image_losses(sums[1], counts[1], weights)['frag_cls_loss'] == 0.0
  assert loss_ref.image_losses(sums[1], counts[1], weights)['frag_loc_loss'] == 0.0
  # the shares only regroup the additions
  other = loss_cases.ref_terms(loss_ref, c, share=P)
  assert np.allclose(other[0], sums, rtol=1e-14, atol=0) and (other[1] == counts).all()


def test_hand_computed_values():
  for n in (1, 2, 22, 64):
    assert loss_ref.cross_entropy(np.full(n, 3.25, np.float32), n // 2) == math.log(n)
  assert [loss_ref.huber(d) for d in (0.5, -0.5, 1.0, -1.0, 3.0, -3.0)] == [
      0.125, 0.125, 0.5, 0.5, 2.5, 2.5]
  # a target 200 below the maximum with every other logit 1e4 below it: nothing underflows
  row = np.full(8, -1e4, np.float32)
  row[2], row[5] = 0.0, -200.0
  assert loss_ref.cross_entropy(row, 5) == 200.0
  # one foreground pixel (object 2, fragment 1, weight 0.5), one background, one ignored
  O, F = 2, 3
  obj = np.zeros((1, 3, O + 1), np.float32)
  frag = np.zeros((1, 3, O, F), np.float32)
  loc = np.zeros((1, 3, O, F, 3), np.float32)
  loc[0, 0, 1, 1] = [0.5, -1.0, 3.0]
  sums, counts, bad = loss_ref.terms(
      obj, frag, loc, np.array([[2, 0, IGNORE]]), np.array([[1, -1, -1]]),
      np.zeros((1, 3, 3), np.float32), np.array([[0.5, 0.0, 0.0]], np.float32), IGNORE, 64)
  assert bad[0] == 0 and counts[0].tolist() == [[1, 1], [0, 0], [1, 0]]
  assert sums[0].tolist() == [[math.log(3), 0.0, 0.0], [0.0, 0.0, 0.0],
                              [math.log(3), math.log(3), 0.5 * ((0.125 + 0.5) + 2.5)]]
  got = loss_ref.image_losses(sums[0], counts[0], WEIGHTS)
  assert got['obj_cls_loss'] == 2 * math.log(3) / 3          # the ignored pixel is in the mean
  assert got['frag_cls_loss'] == math.log(3)
  assert got['frag_loc_loss'] == 100.0 * (1.5625 / 3)
  # no foreground: fragment losses 0
  sums, counts, bad = loss_ref.terms(
      obj, frag, loc, np.array([[0, 0, IGNORE]]), np.array([[-1, -1, -1]]),
      np.zeros((1, 3, 3), np.float32), np.zeros((1, 3), np.float32), IGNORE, 64)
  got = loss_ref.image_losses(sums[0], counts[0], WEIGHTS)
  assert got['frag_cls_loss'] == 0.0 and got['frag_loc_loss'] == 0.0
  assert got['total_loss'] == got['obj_cls_loss'] == 2 * math.log(3) / 3


def test_bad_pixel_rules_of_the_helper():
  O, F = 2, 3
  row, frows, lrows = np.zeros(O + 1, np.float32), np.zeros((O, F)), np.zeros((O, F, 3))

  def kind(g, f=0, w=1.0):
    return loss_ref.pixel_terms(row, frows, lrows, g, f, np.zeros(3), w, O, F, IGNORE)[0]
  assert [kind(-1), kind(O + 1), kind(2 ** 31 - 1)] == ['bad'] * 3
  assert [kind(1, -1), kind(2, F)] == ['bad'] * 2
  assert [kind(1, 0, w) for w in (0.0, -1.0, np.inf, np.nan)] == ['bad'] * 4
  assert [kind(0, -5, np.nan), kind(1, F - 1, 1e-30)] == ['ok'] * 2   # background reads neither
  assert kind(IGNORE, -5, np.nan) == 'ignored'
  assert loss_ref.pixel_terms(row, frows, lrows, 1, -1, np.zeros(3), 1.0, O, F, 1)[0] == 'ignored'


def test_mean_versus_pooled():
  from epos_amd import loss
  # image 0: 2 foreground pixels of object 1; image 1: 6 of object 2; 8 pixels each
  O = 2
  sums = np.zeros((2, O + 1, 3))
  counts = np.zeros((2, O + 1, 2), np.int64)
  counts[0, :, 0], counts[1, :, 0] = [6, 2, 0], [1, 0, 6]
  counts[1, 0, 1] = 1
  sums[0, :, 0], sums[1, :, 0] = [3.0, 1.0, 0.0], [0.5, 0.0, 3.5]
  sums[0, 1, 1:], sums[1, 2, 1:] = [4.0, 0.06], [3.0, 0.36]
  for res in (loss.summarize(sums, counts, np.zeros(2, np.int64), WEIGHTS, O),
              loss_ref.dataset_losses(sums, counts, WEIGHTS)):
    assert [r['frag_cls_loss'] for r in res['per_image']] == [2.0, 0.5]
    assert res['mean']['frag_cls_loss'] == 1.25 and res['pooled']['frag_cls_loss'] == 7.0 / 8
    assert res['mean']['obj_cls_loss'] == res['pooled']['obj_cls_loss'] == 0.5
    assert res['mean']['frag_loc_loss'] == (100 * (0.06 / 6) + 100 * (0.36 / 18)) / 2
    assert res['pooled']['frag_loc_loss'] == 100 * ((0.06 + 0.36) / 24)
    assert res['per_object'][1] == {'frag_cls_loss': 2.0, 'frag_loc_loss': 100 * (0.06 / 6),
                                    'pixels': 2}
    assert res['per_object'][2]['pixels'] == 6 and res['per_object'][2]['frag_cls_loss'] == 0.5
    t = res['pooled']
    assert t['total_loss'] == (t['obj_cls_loss'] + t['frag_cls_loss']) + t['frag_loc_loss']
    totals = [r['total_loss'] for r in res['per_image']]
    assert res['mean']['total_loss'] == (totals[0] + totals[1]) / 2      # the mean of the totals
  # an image without foreground pulls the mean toward 0 and leaves pooled alone
  sums3 = np.concatenate([sums, np.zeros((1, O + 1, 3))])
  counts3 = np.concatenate([counts, np.array([[[8, 0], [0, 0], [0, 0]]])])
  res = loss.summarize(sums3, counts3, np.zeros(3, np.int64), WEIGHTS, O)
  assert res['mean']['frag_cls_loss'] == 2.5 / 3 and res['pooled']['frag_cls_loss'] == 7.0 / 8
  assert res['per_image'][2]['frag_cls_loss'] == 0.0


def test_result_errors_on_hand_made_tables():
  from epos_amd import loss
  from epos_amd._lib import EposError
  O = 2
  sums = np.ones((2, O + 1, 3))
  counts = np.ones((2, O + 1, 2), np.int64)
  loss.summarize(sums, counts, np.zeros(2, np.int64), WEIGHTS, O)
  with pytest.raises(EposError, match=r'^5 pixel\(s\)'):
    loss.summarize(sums, counts, np.array([2, 3]), WEIGHTS, O)
  for v in (np.inf, np.nan):
    s = sums.copy()
    s[1, 2, 1] = v
    with pytest.raises(EposError, match=r'^Loss is inf or nan\.$'):
      loss.summarize(s, counts, np.zeros(2, np.int64), WEIGHTS, O)
    with pytest.raises(EposError, match=r'^1 pixel\(s\)'):       # the bad pixels are named first
      loss.summarize(s, counts, np.array([0, 1]), WEIGHTS, O)


# ---------------------------------------------------------------- binding ---
def test_loss_symbols_are_declared_and_bound():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  nargs = {'epos_loss_share_pixels': ('int64_t', ctypes.c_int64, 3),
           'epos_loss_workspace_bytes': ('int64_t', ctypes.c_int64, 4),
           'epos_loss_terms': ('int', ctypes.c_int, 18)}
  for name, (ctype, want, n) in nargs.items():
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is want and len(argtypes) == n, name
    decl = re.search(r'\b%s %s\s*\(([^)]*)\)\s*;' % (ctype, name), header)
    assert decl, name
    assert decl.group(1).count(',') + 1 == n, name
  lib = _lib.load()
  assert lib.epos_abi_version() == 7
  # the host side of the entry points needs no device: sizes and refusals
  assert lib.epos_loss_workspace_bytes(0, 100, 3, 5) == 0
  assert lib.epos_loss_workspace_bytes(2, 0, 3, 5) == 0
  share = lib.epos_loss_share_pixels(19200, 21, 64)
  assert share >= 1 and lib.epos_loss_workspace_bytes(8, 19200, 21, 64) == (
      8 * -(-19200 // share) * (5 * 22 + 1) * 8)
  for B in (1, 3, 8):                                  # the share does not know the batch
    assert lib.epos_loss_workspace_bytes(B, 19200, 21, 64) == (
        B * lib.epos_loss_workspace_bytes(1, 19200, 21, 64))
  assert lib.epos_loss_workspace_bytes(1, 100, 0, 5) < 0
  assert b'epos_loss_workspace_bytes' in lib.epos_last_error()
  assert lib.epos_loss_workspace_bytes(1, 100, 3, 257) < 0
  assert lib.epos_loss_terms(None, 3, None, None, None, None, None, None, 1, 10, 3, 5, IGNORE,
                             None, None, None, None, None) < 0
  assert lib.epos_last_error() == b'epos_loss_terms: ld_obj must be >= num_objs + 1'
  assert lib.epos_loss_terms(None, 4, None, None, None, None, None, None, 1, 10, 3, 5, IGNORE,
                             None, None, None, None, None) < 0
  assert lib.epos_last_error() == b'epos_loss_terms: null pointer'
  assert lib.epos_loss_terms(None, 4, None, None, None, None, None, None, 0, 10, 3, 5, IGNORE,
                             None, None, None, None, None) == 0


# ---------------------------------------------------------------- command line ---
@pytest.fixture
def script():
  import importlib
  return importlib.import_module('eval_loss')


def test_eval_loss_cli_defaults_and_params_yml(script, tmp_path, monkeypatch):
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  args, model_dir = script.prepare(['--model=m', '--dataset', 'lm', '--master', 'x'])
  assert model_dir == os.path.join(str(tmp_path), 'm')
  assert args.eval_crop_size == '640,480' and args.eval_max_height_before_crop == 480
  assert args.eval_tfrecord_names is None and args.batch_size == 1
  assert (args.obj_cls_loss_weight, args.frag_cls_loss_weight, args.frag_loc_loss_weight) == (
      1.0, 1.0, 100.0)
  assert args.precision == 'fp32' and args.num_frags == 64 and args.synthetic == 0
  assert args.checkpoint_name is None and args.seed == 0 and args.frames is None
  # eval.py's own flags are not this script's
  assert not hasattr(args, 'eval_interval_secs') and not hasattr(args, 'eval_frag_labels')
  (tmp_path / 'm').mkdir()
  (tmp_path / 'm' / 'params.yml').write_text(
      'obj_cls_loss_weight: 2.0\nfrag_cls_loss_weight: 0.5\nfrag_loc_loss_weight: 50.0\n'
      'eval_crop_size: "128,96"\ntrain_steps: 1000\n')
  args, _ = script.prepare(['--model=m', '--dataset', 'lm'])
  assert (args.obj_cls_loss_weight, args.frag_cls_loss_weight, args.frag_loc_loss_weight) == (
      2.0, 0.5, 50.0)
  assert args.eval_crop_size == '128,96' and not hasattr(args, 'train_steps')
  with pytest.raises(ValueError, match='--batch_size must be >= 1'):
    script.prepare(['--model=m', '--dataset', 'lm', '--batch_size', '0'])


def test_eval_loss_cli_refusals(script, tmp_path, monkeypatch):
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  with pytest.raises(NotImplementedError, match='single-scale'):
    script.prepare(['--model=m', '--dataset', 'lm', '--image_pyramid', '0.5,1.0',
                    '--multi_scale_inference', 'true'])
  with pytest.raises(NotImplementedError, match='image_pyramid'):    # check_supported_flags
    script.prepare(['--model=m', '--dataset', 'lm', '--image_pyramid', '0.5,1.0'])
  script.prepare(['--model=m', '--dataset', 'lm', '--image_pyramid', '1.0',
                  '--multi_scale_inference', 'true'])                # [1.0] is single scale
  with pytest.raises(NotImplementedError, match='upsample_logits'):
    script.prepare(['--model=m', '--dataset', 'lm', '--upsample_logits', 'true'])
  monkeypatch.delenv('BOP_PATH', raising=False)
  with pytest.raises(ValueError, match=r'needs --dataset and \$BOP_PATH \(object models\)'):
    script.prepare(['--model=m', '--dataset', 'lm'])


def test_the_three_existing_parsers_do_not_know_the_loss_flags():
  import importlib
  for name in ('infer', 'eval', 'eval_poses'):
    ap = importlib.import_module(name).build_parser()
    flags = {s for a in ap._actions for s in a.option_strings}
    assert not flags & {'--obj_cls_loss_weight', '--frag_cls_loss_weight',
                        '--frag_loc_loss_weight'}, name
