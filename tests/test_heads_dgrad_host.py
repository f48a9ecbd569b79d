"""Host side of the logits layers' input gradient: the numpy restatement
(tests/helpers/heads_dgrad_ref.py) against the dense fp64 product and against torch's fp64
autograd through "features -> three 1x1 convolutions -> the losses", the ReLU mask, the binding
of the new symbol, the host-side refusals and the Python entries without a device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import (heads_dgrad_ref, heads_wgrad_ref, loss_cases, loss_grad_ref,  # noqa: E402
                           loss_ref)
from tests.test_loss_grad_host import torch_losses                           # noqa: E402

IGNORE = loss_cases.IGNORE
UPSTREAM = [0.3, -1.0, 2.0, 0.5]
INVALID = -1                                  # EPOS_E_INVALID


def head_matrices(O, F, K, seed):
  rng = np.random.RandomState(seed)
  return [(0.5 * rng.randn(K, n)).astype(np.float32) for n in (O + 1, O * F, O * F * 3)]


def case_with_every_class(B, P, O, F, seed):
  """A seeded case with ignored, background and foreground pixels, plus bad ones: an object
  label outside 0..O, a fragment label outside 0..F-1 and weights that are no finite number
  > 0. The bad pixels carry non-finite logits: they must never be read."""
  c = loss_cases.make_case(B, P, O, F, seed)
  g, f, w = c['gt_obj'][0], c['gt_frag'][0], c['gt_weight'][0]
  g[20], g[21] = -1, O + 1
  g[22:27] = 2
  f[22:27] = 1
  f[22], w[23], w[24], w[25], w[26] = F, 0.0, -1.0, np.nan, np.inf
  for p in range(20, 27):
    c['obj_logits'][0, p] = np.nan
    c['frag_logits'][0, p] = np.inf
    c['frag_loc'][0, p] = np.nan
  return c


def test_restatement_agrees_with_the_dense_product():
  B, P, O, F, K = 2, 61, 3, 5, 7
  c = case_with_every_class(B, P, O, F, seed=3)
  cls, frag = heads_wgrad_ref.classes(c, IGNORE)
  assert (cls[20:27] == -1).all() and (cls == 0).any() and (cls >= 1).any()
  assert (c['gt_obj'] == IGNORE).any()
  _, counts, bad = loss_cases.ref_terms(loss_ref, c, share=16)
  assert bad.tolist() == [7, 0]
  scale = loss_grad_ref.scales(counts, (0.7, 1.3, 100.0), 0)
  Ws = head_matrices(O, F, K, 4)
  for rounded in (True, False):
    d = loss_grad_ref.grads(c, scale, UPSTREAM, IGNORE, rounded=rounded)
    sums, abs_sums, n_active = heads_dgrad_ref.dgrad(*d, *Ws, cls, frag)
    assert np.isfinite(sums).all()
    dense = sum(np.asarray(dh, np.float64).reshape(B * P, -1) @ W.astype(np.float64).T
                for dh, W in zip(d, Ws))
    assert np.abs(dense).max() > 0
    assert (np.abs(sums - dense) <= 1e-12 * abs_sums).all()
    # per class: nothing for an ignored or a bad pixel, O+1 columns for the background,
    # O+1 + F + 3 for the foreground
    assert (n_active[cls < 0] == 0).all() and not sums[cls < 0].any()
    assert not np.signbit(sums[cls < 0]).any()
    assert (n_active[cls == 0] == O + 1).all() and (n_active[cls >= 1] == O + 1 + F + 3).all()
    assert sums[cls == 0].all() and sums[cls >= 1].all()


def test_restatement_reads_active_columns_only():
  # a NaN in an inactive column of d, or in a weight column no pixel activates, stays out
  B, P, O, F, K = 1, 12, 2, 3, 4
  c = loss_cases.make_case(B, P, O, F, seed=8, ignore_band=False)
  c['gt_obj'][0, :] = [0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1]       # object 2 never
  fg = c['gt_obj'] == 1
  c['gt_frag'][:] = np.where(fg, 1, -1)
  c['gt_weight'][:] = np.where(fg, 0.5, 0.0)
  cls, frag = heads_wgrad_ref.classes(c, IGNORE)
  _, counts, _ = loss_cases.ref_terms(loss_ref, c, share=16)
  scale = loss_grad_ref.scales(counts, (1.0, 1.0, 100.0), 1)
  d = [np.array(x) for x in loss_grad_ref.grads(c, scale, None, IGNORE)]
  Ws = head_matrices(O, F, K, 9)
  exp = heads_dgrad_ref.dgrad(*d, *Ws, cls, frag)[0]
  d[1][:, :, 1] = np.nan                                    # rows of object 2
  d[2][:, :, 0, [0, 2]] = np.nan                            # fragments 0 and 2 of object 1
  Ws[1][:, F:] = np.nan
  Ws[2][:, :3] = np.nan
  got, _, n_active = heads_dgrad_ref.dgrad(*d, *Ws, cls, frag)
  assert np.array_equal(got, exp) and np.isfinite(got).all()
  assert n_active.tolist() == [O + 1 + (F + 3) * int(v) for v in fg[0]]
  # an active NaN marks its own pixel's row and no other
  d[0][0, 5, 1] = np.nan
  got = heads_dgrad_ref.dgrad(*d, *Ws, cls, frag)[0]
  assert np.isnan(got[5]).all() and np.array_equal(np.delete(got, 5, 0), np.delete(exp, 5, 0))


@pytest.mark.parametrize('upstream', [None, UPSTREAM])
@pytest.mark.parametrize('reduction', ['mean', 'pooled'])
def test_restatement_agrees_with_torch_fp64_autograd(reduction, upstream):
  B, P, O, F, K = 3, 61, 3, 5, 7
  c = loss_cases.make_case(B, P, O, F, seed=5, empty_images=(1,))
  rng = np.random.RandomState(11)
  X = torch.from_numpy(rng.randn(B, P, K).astype(np.float32)).double().requires_grad_()
  Ws = head_matrices(O, F, K, 12)
  bs = [0.5 * rng.randn(W.shape[1]) for W in Ws]
  shapes = [(B, P, O + 1), (B, P, O, F), (B, P, O, F, 3)]
  leaves = []
  for k, name in enumerate(('obj_logits', 'frag_logits', 'frag_loc')):
    # a 1x1 convolution is a matrix product over the channels
    lin = (X @ torch.from_numpy(Ws[k]).double() + torch.from_numpy(bs[k])).reshape(shapes[k])
    c[name] = lin.detach().numpy().astype(np.float32)
    # the fp32 values the restatement reads, with the derivative of the linear layer
    leaves.append(lin + (torch.from_numpy(c[name]).double() - lin).detach())
  weights = (0.7, 1.3, 100.0)
  if reduction == 'mean':
    per_image = [torch_losses(*leaves, c, [b], O, F, weights) for b in range(B)]
    losses = [sum(r[k] for r in per_image) / B for k in range(3)]
  else:
    losses = list(torch_losses(*leaves, c, range(B), O, F, weights))
  total = (losses[0] + losses[1]) + losses[2]
  up = upstream if upstream is not None else [0.0, 0.0, 0.0, 1.0]
  (up[0] * losses[0] + up[1] * losses[1] + up[2] * losses[2] + up[3] * total).backward()
  _, counts, bad = loss_cases.ref_terms(loss_ref, c, share=16)
  assert bad.tolist() == [0, 0, 0]
  scale = loss_grad_ref.scales(counts, weights, {'mean': 0, 'pooled': 1}[reduction])
  d = loss_grad_ref.grads(c, scale, upstream, IGNORE, rounded=False)
  cls, frag = heads_wgrad_ref.classes(c, IGNORE)
  sums, abs_sums, n_active = heads_dgrad_ref.dgrad(*d, *Ws, cls, frag)
  exp = X.grad.numpy().reshape(B * P, K)
  assert np.abs(exp).max() > 0
  # the logit gradients' tolerance of tests/test_loss_grad_host.py, |s_bk u_k| 64 row 2^-52 per
  # element, carried through the pixel's sum: times the absolute row sum of the head's weights
  # over the pixel's active columns, bounded by the whole row sum; plus the order of the sum
  u = loss_grad_ref.upstream_factors(upstream)
  tol = (n_active[:, None] + 16.0) * 2.0 ** -52 * abs_sums
  for k, row_len in enumerate((O + 1, F, 3)):
    per_image = np.array([abs(scale[b, k] * u[k]) * 64 * row_len * 2.0 ** -52 for b in range(B)])
    tol = tol + np.repeat(per_image, P)[:, None] * np.abs(Ws[k].astype(np.float64)).sum(axis=1)
  assert (np.abs(sums - exp) <= tol).all()
  assert float(np.abs(sums - exp).max()) <= 1e-12 * float(np.abs(exp).max())
  # the image without foreground has object columns only
  assert (n_active[P:2 * P][cls[P:2 * P] >= 0] == O + 1).all()


def test_relu_mask_and_bound():
  dx = np.array([[1.0, -2.0, 3.0, -4.0, 5.0]])
  y = np.array([[2.0, -1.0, 0.0, -0.0, np.nan]], np.float32)
  out = heads_dgrad_ref.relu_mask(dx, y)
  assert out.tolist()[0][:4] == [1.0, 0.0, 0.0, 0.0] and out[0, 4] == 5.0
  assert not np.signbit(out[0, 1:4]).any() and dx[0, 1] == -2.0     # a copy, +0.0
  b = heads_dgrad_ref.bound(np.array([[3.0, -4.0]]), np.array([[10.0, 0.0]]), np.array([5]))
  assert b.tolist() == [[2.0 ** -24 * 3 + 21 * 2.0 ** -52 * 10, 2.0 ** -24 * 4]]
  ok, worst = heads_dgrad_ref.within(np.float32([[3.0, np.nan, 0.0]]), np.array([[3.0, np.nan, 0.0]]),
                                     np.array([[3.0, np.nan, 0.0]]), np.array([1]))
  assert ok and worst == 0.0
  assert not heads_dgrad_ref.within(np.float32([[3.0, 1.0]]), np.array([[3.0, np.nan]]),
                                    np.array([[3.0, np.nan]]), np.array([1]))[0]
  assert not heads_dgrad_ref.within(np.float32([[3.000001]]), np.array([[3.0]]),
                                    np.array([[3.0]]), np.array([1]))[0]
  assert not heads_dgrad_ref.within(np.float32([[1e-30]]), np.array([[0.0]]), np.array([[0.0]]),
                                    np.array([0]))[0]


# ---------------------------------------------------------------- binding ---
FAKE = ctypes.c_void_p(4096)            # a non-null pointer no refused call dereferences
C_NAMES = {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t', ctypes.c_float: 'float'}


def test_symbol_is_declared_bound_and_exported():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  assert 'Input gradient (csrc/heads_dgrad.hip' in header
  assert ('dX[p,k] = fl32( sum_h sum_{n active at p} (double)d_h[p,n] * (double)Wt_h[n,k] )'
          in header)
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  name, ctype = 'epos_heads_dgrad_f32', 'int'
  restype, argtypes = _lib.SYMBOLS[name]
  assert C_NAMES[restype] == ctype
  decl = re.search(r'\b%s %s\s*\(([^)]*)\)\s*;' % (ctype, name), header)
  assert decl
  args = [a.strip() for a in decl.group(1).split(',')]
  assert len(args) == len(argtypes) == 25
  for arg, t in zip(args, argtypes):                     # pointer or the scalar type by name
    if '*' in arg:
      assert t is ctypes.c_void_p, arg
    else:
      assert arg.split()[0] == C_NAMES[t], arg
  # the sixteen inputs of epos_loss_grads, under the same names and in the same order
  grads = re.search(r'\bint epos_loss_grads\s*\(([^)]*)\)\s*;', header).group(1).split(',')
  assert [a.split()[-1] for a in args[:15]] == [a.split()[-1] for a in grads[:15]]
  assert os.path.exists(os.path.join(ROOT, 'epos_amd', 'csrc', 'heads_dgrad.hip'))
  lib = _lib.load()
  assert lib.epos_abi_version() == 7                     # added without a version change
  assert ctypes.CDLL(_lib.lib_path()).epos_heads_dgrad_f32  # exported by the built library


def test_host_side_refusals_of_epos_heads_dgrad_f32():
  from epos_amd import _lib
  lib = _lib.load()
  O, F, K = 3, 5, 4
  OUT = ctypes.c_void_p(8192)

  def call(B=1, P=10, O=O, F=F, K=K, ld=O + 1, obj=FAKE, frag=FAKE, scales=FAKE, upstream=None,
           wt=(FAKE, FAKE, FAKE), ldwt=K, Y=None, ldy=0, dX=OUT, ldx=K):
    return lib.epos_heads_dgrad_f32(obj, ld, frag, FAKE, FAKE, FAKE, FAKE, FAKE, B, P, O, F,
                                    IGNORE, scales, upstream, wt[0], wt[1], wt[2], ldwt, K, Y,
                                    ldy, dX, ldx, None)
  Y = ctypes.c_void_p(12288)
  for kwargs, msg in (({'B': -1}, b'B must be >= 0'),
                      ({'B': 65536}, b'B must be <= 65535'),
                      ({'P': -1}, b'P must be in 0..2^31'),
                      ({'P': 2 ** 31 + 1}, b'P must be in 0..2^31'),
                      ({'O': 0}, b'num_objs must be in 1..4095'),
                      ({'O': 4096, 'ld': 4097}, b'num_objs must be in 1..4095'),
                      ({'F': 0}, b'num_frags must be in 1..256'),
                      ({'F': 257}, b'num_frags must be in 1..256'),
                      ({'B': 65535, 'P': 2 ** 31},
                       b'B * workgroups per image must be below 2^31'),
                      ({'K': 0}, b'K must be in 1..1024'),
                      ({'K': 1025, 'ldwt': 1025, 'ldx': 1025}, b'K must be in 1..1024'),
                      ({'ldx': K - 1}, b'ldx must be >= K'),
                      ({'ldwt': K - 1}, b'ldwt must be >= K'),
                      ({'Y': Y, 'ldy': K - 1}, b'ldy must be >= K'),
                      ({'ld': O}, b'ld_obj must be >= num_objs + 1'),
                      ({'obj': None}, b'null pointer'),
                      ({'frag': None}, b'null pointer'),
                      ({'scales': None}, b'null pointer'),
                      ({'wt': (FAKE, None, FAKE)}, b'null pointer'),
                      ({'wt': (FAKE, FAKE, None)}, b'null pointer'),
                      ({'dX': None}, b'null pointer'),
                      ({'dX': FAKE}, b'the output buffer starts at an input pointer'),
                      ({'upstream': OUT}, b'the output buffer starts at an input pointer'),
                      ({'wt': (FAKE, OUT, FAKE)},
                       b'the output buffer starts at an input pointer'),
                      ({'Y': OUT, 'ldy': K}, b'the output buffer starts at an input pointer')):
    assert call(**kwargs) == INVALID, kwargs
    assert lib.epos_last_error() == b'epos_heads_dgrad_f32: ' + msg, kwargs
  # no pixel: returns 0 and launches nothing, null pointers or not
  assert call(B=0) == 0 and call(P=0) == 0
  assert call(P=0, obj=None, scales=None, wt=(None, None, None), dX=None) == 0


def test_modules_import_without_torch():
  code = ('import sys; sys.modules["torch"] = None\n'
          'from epos_amd import heads_train, loss\n'
          'assert callable(heads_train.heads_input_grad)\n'
          'assert callable(heads_train.net_feature_grad)\n'
          'assert callable(loss.differentiable_losses_from_features)\n'
          'assert loss.HEAD_VARIABLES[0] == "logits/pred_obj_conf/weights"\n'
          'assert "torch" not in [m for m in sys.modules if sys.modules[m] is not None]\n')
  subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)


def test_python_entries_refuse_host_tensors():
  from epos_amd import heads_train, loss
  from epos_amd._lib import EposError
  O, F, K = 3, 5, 4
  c = loss_cases.make_case(1, 6, O, F, seed=0)
  logits = {'pred_obj_conf': torch.from_numpy(c['obj_logits']),
            'pred_frag_conf': torch.from_numpy(c['frag_logits']),
            'pred_frag_loc': torch.from_numpy(c['frag_loc'])}
  gt = {'obj_label': torch.from_numpy(c['gt_obj']), 'frag_label': torch.from_numpy(c['gt_frag']),
        'frag_loc': torch.from_numpy(c['gt_loc']), 'frag_weight': torch.from_numpy(c['gt_weight'])}
  Ws = head_matrices(O, F, K, 1)
  head_weights = {}
  for name, W in zip(('pred_obj_conf', 'pred_frag_conf', 'pred_frag_loc'), Ws):
    head_weights['logits/%s/weights' % name] = torch.from_numpy(W).view(1, 1, K, -1)
    head_weights['logits/%s/biases' % name] = torch.zeros(W.shape[1])
  with pytest.raises(EposError, match='needs a HIP device'):
    heads_train.heads_input_grad(logits, gt, torch.zeros((1, 3), dtype=torch.float64),
                                 head_weights)
  with pytest.raises(EposError, match='need a HIP device'):
    loss.differentiable_losses_from_features(torch.zeros((6, K)), head_weights, gt)
