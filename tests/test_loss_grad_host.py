"""Host side of the loss gradients: the numpy restatement (tests/helpers/loss_grad_ref.py)
against torch's fp64 autograd through an independent formulation and against hand-computed
values, the binding of the new symbols, their host-side refusals, and the error without a
device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import loss_cases, loss_grad_ref, loss_ref      # noqa: E402

IGNORE = loss_cases.IGNORE
UPSTREAM = [0.3, -1.0, 2.0, 0.5]


def torch_losses(obj_logits, frag_logits, frag_loc, c, images, O, F, weights):
  """The three losses of the example set `images` (one image: the reference's batch of one;
  all of them: the pooled batch) in torch fp64, differentiable: the gather / mean structure of
  epos_lib/loss.py -- every pixel's object cross-entropy weighted by the not-ignored mask and
  averaged over all pixels; the foreground pixels gathered, their fragment cross-entropy
  against the normalised target distribution averaged, their Huber losses weighted and
  averaged over pixels x 3."""
  TF = torch.nn.functional
  w_obj, w_cls, w_loc = weights
  idx = torch.tensor(list(images))
  gt = torch.from_numpy(c['gt_obj'][list(images)].astype(np.int64)).reshape(-1)
  logits = obj_logits[idx].reshape(-1, O + 1)
  keep = gt != IGNORE
  ce = TF.cross_entropy(logits, torch.where(keep, gt, torch.zeros_like(gt)), reduction='none')
  obj = (ce * keep.double() * w_obj).mean()
  fg = torch.nonzero(keep & (gt > 0)).reshape(-1)
  zero = torch.zeros((), dtype=torch.float64)
  if fg.numel() == 0:
    return obj, zero, zero
  objs = gt[fg] - 1
  frag = torch.from_numpy(c['gt_frag'][list(images)].astype(np.int64)).reshape(-1)[fg]
  wgt = torch.from_numpy(c['gt_weight'][list(images)]).double().reshape(-1)[fg]
  rows = frag_logits[idx].reshape(-1, O, F)[fg, objs]                       # [n, F]
  distrib = torch.zeros((fg.numel(), F), dtype=torch.float64)
  distrib[torch.arange(fg.numel()), frag] = wgt
  distrib = distrib / distrib.sum(dim=1, keepdim=True)
  cls = (TF.cross_entropy(rows, distrib, reduction='none') * w_cls).mean()
  pred = frag_loc[idx].reshape(-1, O, F, 3)[fg, objs, frag]                 # [n, 3]
  target = torch.from_numpy(c['gt_loc'][list(images)]).double().reshape(-1, 3)[fg]
  hub = TF.huber_loss(pred, target, delta=1.0, reduction='none') * w_loc
  loc = (hub * wgt.reshape(-1, 1)).mean()
  return obj, cls, loc


@pytest.mark.parametrize('reduction', ['mean', 'pooled'])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_restatement_agrees_with_torch_fp64_autograd(seed, reduction):
  B, P, O, F = 3, 61, 3, 5
  c = loss_cases.make_case(B, P, O, F, seed, empty_images=(1,))
  weights = (0.7, 1.3, 100.0)
  leaves = [torch.from_numpy(c[k]).double().requires_grad_() for k in (
      'obj_logits', 'frag_logits', 'frag_loc')]
  if reduction == 'mean':
    per_image = [torch_losses(*leaves, c, [b], O, F, weights) for b in range(B)]
    losses = [sum(r[k] for r in per_image) / B for k in range(3)]
  else:
    losses = list(torch_losses(*leaves, c, range(B), O, F, weights))
  total = (losses[0] + losses[1]) + losses[2]
  up = UPSTREAM
  (up[0] * losses[0] + up[1] * losses[1] + up[2] * losses[2] + up[3] * total).backward()
  _, counts, bad = loss_cases.ref_terms(loss_ref, c, share=16)
  assert bad.tolist() == [0, 0, 0] and counts[1, 1:, 0].sum() == 0
  scale = loss_grad_ref.scales(counts, weights, {'mean': 0, 'pooled': 1}[reduction])
  got = loss_grad_ref.grads(c, scale, up, IGNORE, rounded=False)
  u = loss_grad_ref.upstream_factors(up)
  assert u == [0.8, -0.5, 2.5]
  for k, row_len in enumerate((O + 1, F, 3)):
    exp = leaves[k].grad.numpy()
    assert np.abs(exp).max() > 0
    for b in range(B):
      tol = abs(scale[b, k] * u[k]) * 64 * row_len * 2.0 ** -52
      assert np.abs(got[k][b] - exp[b]).max() <= tol, (k, b)
  # ignored pixels and the image without foreground
  assert (got[0][c['gt_obj'] == IGNORE] == 0).all() and (c['gt_obj'] == IGNORE).any()
  assert (got[1][1] == 0).all() and (got[2][1] == 0).all()
  assert (scale[[0, 2], 1:] > 0).all()
  if reduction == 'mean':
    assert (scale[1, 1:] == 0).all()
  else:                                    # one example set: the same factors for every image
    assert (scale == scale[0]).all()


def test_hand_computed_values():
  # uniform logits of n classes: s * (1/n - [c == t])
  for n in (1, 2, 22, 64):
    row = loss_grad_ref.softmax_minus_one_hot(np.full(n, 3.25, np.float32), n // 2)
    assert row == [1.0 / n - (1.0 if k == n // 2 else 0.0) for k in range(n)]
  assert [loss_grad_ref.clamp1(d) for d in (0.5, 1.0, 3.0, -3.0)] == [0.5, 1.0, 1.0, -1.0]
  # one foreground pixel (object 2, fragment 1, weight 0.5), one background, one ignored
  O, F = 2, 3
  c = {'obj_logits': np.zeros((1, 4, O + 1), np.float32),
       'frag_logits': np.zeros((1, 4, O, F), np.float32),
       'frag_loc': np.zeros((1, 4, O, F, 3), np.float32),
       'gt_obj': np.array([[2, 0, IGNORE, 1]]), 'gt_frag': np.array([[1, -1, -1, 0]]),
       'gt_loc': np.zeros((1, 4, 3), np.float32),
       'gt_weight': np.array([[0.5, 0.0, 0.0, 2.0]], np.float32)}
  c['frag_loc'][0, 0, 1, 1] = [0.5, 1.0, 3.0]
  c['frag_loc'][0, 3, 0, 0] = [-3.0, -0.5, 0.0]
  _, counts, bad = loss_cases.ref_terms(loss_ref, c, share=64)
  assert bad[0] == 0
  weights = (1.0, 1.0, 100.0)
  scale = loss_grad_ref.scales(counts, weights, 0)
  assert scale.tolist() == [[1.0 / 4, 1.0 / 2, 100.0 / 6]]
  assert loss_grad_ref.scales(counts, weights, 1).tolist() == scale.tolist()
  s = scale[0]
  d_obj, d_frag, d_loc = loss_grad_ref.grads(c, scale, None, IGNORE, rounded=False)
  third = 1.0 / 3
  assert d_obj[0].tolist() == [[s[0] * third, s[0] * third, s[0] * (third - 1.0)],
                               [s[0] * (third - 1.0), s[0] * third, s[0] * third],
                               [0.0, 0.0, 0.0],
                               [s[0] * third, s[0] * (third - 1.0), s[0] * third]]
  assert d_frag[0, 0].tolist() == [[0.0] * 3, [s[1] * third, s[1] * (third - 1.0), s[1] * third]]
  assert d_frag[0, 3].tolist() == [[s[1] * (third - 1.0), s[1] * third, s[1] * third], [0.0] * 3]
  assert (d_frag[0, 1:3] == 0).all()
  assert d_loc[0, 0, 1, 1].tolist() == [s[2] * (0.5 * 0.5), s[2] * (0.5 * 1.0), s[2] * (0.5 * 1.0)]
  assert d_loc[0, 3, 0, 0].tolist() == [s[2] * (2.0 * -1.0), s[2] * (2.0 * -0.5), 0.0]
  assert np.count_nonzero(d_loc) == 5
  # rounded once to fp32; an upstream of {1, 0, 0, 2} triples the object gradient
  r_obj = loss_grad_ref.grads(c, scale, [1.0, 0.0, 0.0, 2.0], IGNORE)[0]
  assert r_obj.dtype == np.float32 and r_obj[0, 0, 2] == np.float32(s[0] * 3.0 * (third - 1.0))
  # an image without foreground: all-zero fragment gradients, fragment factors 0
  c['gt_obj'][:] = [[0, 0, IGNORE, 0]]
  _, counts, _ = loss_cases.ref_terms(loss_ref, c, share=64)
  scale = loss_grad_ref.scales(counts, weights, 0)
  assert scale.tolist() == [[1.0 / 4, 0.0, 0.0]]
  d_obj, d_frag, d_loc = loss_grad_ref.grads(c, scale, None, IGNORE)
  assert not d_frag.any() and not d_loc.any() and d_obj[0, :2].all() and not d_obj[0, 2].any()


# ---------------------------------------------------------------- binding ---
FAKE = ctypes.c_void_p(4096)            # a non-null pointer no refused call dereferences


def test_loss_grad_symbols_are_declared_and_bound():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  nargs = {'epos_loss_reduce': ('int', ctypes.c_int, 11),
           'epos_loss_grad_share_pixels': ('int64_t', ctypes.c_int64, 3),
           'epos_loss_grads': ('int', ctypes.c_int, 20)}
  for name, (ctype, want, n) in nargs.items():
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is want and len(argtypes) == n, name
    decl = re.search(r'\b%s %s\s*\(([^)]*)\)\s*;' % (ctype, name), header)
    assert decl, name
    assert decl.group(1).count(',') + 1 == n, name
  assert re.search(r'#define EPOS_LOSS_MEAN 0\b', header)
  assert re.search(r'#define EPOS_LOSS_POOLED 1\b', header)
  lib = _lib.load()
  assert lib.epos_abi_version() == 7
  # the share is a function of P alone
  assert lib.epos_loss_grad_share_pixels(0, 3, 5) == 0
  share = lib.epos_loss_grad_share_pixels(19200, 21, 64)
  assert share >= 1
  assert {lib.epos_loss_grad_share_pixels(19200, O, F) for O in (1, 21, 4095)
          for F in (1, 64, 256)} == {share}
  assert lib.epos_loss_grad_share_pixels(10, 0, 5) < 0
  assert lib.epos_last_error() == b'epos_loss_grad_share_pixels: num_objs must be in 1..4095'


def test_host_side_refusals_of_epos_loss_reduce():
  from epos_amd import _lib
  lib = _lib.load()

  def call(B=1, O=3, reduction=0, ptr=FAKE):
    return lib.epos_loss_reduce(ptr, ptr, B, O, 1.0, 1.0, 100.0, reduction, ptr, ptr, None)
  for kwargs, msg in (({'B': -1}, b'B must be >= 0'),
                      ({'O': 0}, b'num_objs must be in 1..4095'),
                      ({'O': 4096}, b'num_objs must be in 1..4095'),
                      ({'reduction': 2}, b'reduction must be EPOS_LOSS_MEAN or EPOS_LOSS_POOLED'),
                      ({'reduction': -1}, b'reduction must be EPOS_LOSS_MEAN or EPOS_LOSS_POOLED'),
                      ({'ptr': None}, b'null pointer')):
    assert call(**kwargs) == -1, kwargs
    assert lib.epos_last_error() == b'epos_loss_reduce: ' + msg
  assert call(B=0) == 0 and call(B=0, ptr=None) == 0 and call(B=0, reduction=1) == 0


def test_host_side_refusals_of_epos_loss_grads():
  from epos_amd import _lib
  lib = _lib.load()
  O, F = 3, 5

  def call(B=1, P=10, O=O, F=F, ld=O + 1, ld_d=O + 1, obj=FAKE, scales=FAKE, upstream=None,
           outs=(None, None, None)):
    return lib.epos_loss_grads(obj, ld, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, B, P, O, F, IGNORE,
                               scales, upstream, outs[0], ld_d, outs[1], outs[2], None)
  for kwargs, msg in (({'B': -1}, b'B must be >= 0'),
                      ({'B': 65536}, b'B must be <= 65535'),
                      ({'P': -1}, b'P must be in 0..2^31'),
                      ({'P': 2 ** 31 + 1}, b'P must be in 0..2^31'),
                      ({'O': 0}, b'num_objs must be in 1..4095'),
                      ({'O': 4096, 'ld': 4097, 'ld_d': 4097}, b'num_objs must be in 1..4095'),
                      ({'F': 0}, b'num_frags must be in 1..256'),
                      ({'F': 257}, b'num_frags must be in 1..256'),
                      ({'B': 65535, 'P': 2 ** 31},
                       b'B * workgroups per image must be below 2^31'),
                      ({'ld': O}, b'ld_obj must be >= num_objs + 1'),
                      ({'ld_d': O}, b'ld_dobj must be >= num_objs + 1'),
                      ({'obj': None}, b'null pointer'),
                      ({'scales': None}, b'null pointer'),
                      ({'outs': (FAKE, None, None)},
                       b'an output buffer starts at an input pointer'),
                      ({'outs': (None, None, FAKE)},
                       b'an output buffer starts at an input pointer'),
                      ({'outs': (None, ctypes.c_void_p(8192), None),
                        'upstream': ctypes.c_void_p(8192)},
                       b'an output buffer starts at an input pointer')):
    assert call(**kwargs) == -1, kwargs
    assert lib.epos_last_error() == b'epos_loss_grads: ' + msg
  # nothing to do: the empty batch, the empty image, no output asked for
  assert call(B=0) == 0 and call(P=0) == 0 and call(B=0, obj=None, scales=None) == 0
  assert call() == 0 and call(upstream=FAKE) == 0


def test_differentiable_losses_needs_a_device():
  from epos_amd import loss
  from epos_amd._lib import EposError
  O, F = 3, 5                              # host tensors: refused with or without a device
  c = loss_cases.make_case(1, 6, O, F, seed=0)
  logits = {'pred_obj_conf': torch.from_numpy(c['obj_logits']).requires_grad_(),
            'pred_frag_conf': torch.from_numpy(c['frag_logits']),
            'pred_frag_loc': torch.from_numpy(c['frag_loc'])}
  gt = {'obj_label': torch.from_numpy(c['gt_obj']), 'frag_label': torch.from_numpy(c['gt_frag']),
        'frag_loc': torch.from_numpy(c['gt_loc']), 'frag_weight': torch.from_numpy(c['gt_weight'])}
  with pytest.raises(EposError, match='need a HIP device'):
    loss.differentiable_losses(logits, gt)
  with pytest.raises(EposError, match='need a HIP device'):
    loss.loss_grads(logits, gt, torch.zeros((1, 3), dtype=torch.float64))
  with pytest.raises(EposError, match='need a HIP device'):
    loss.loss_values(torch.zeros((1, O + 1, 3), dtype=torch.float64),
                     torch.zeros((1, O + 1, 2), dtype=torch.int64), (1.0, 1.0, 100.0))
