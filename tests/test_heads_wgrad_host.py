"""Host side of the logits layers' weight gradients and of the momentum step: the numpy
restatement (tests/helpers/heads_wgrad_ref.py) against torch's fp64 autograd through A @ W + b
and against hand-computed values, the binding of the new symbols, the workspace formula, the
host-side refusals, and the import without torch."""
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

from tests.helpers import heads_wgrad_ref, loss_cases, loss_grad_ref, loss_ref   # noqa: E402
from tests.test_loss_grad_host import torch_losses                           # noqa: E402

IGNORE = loss_cases.IGNORE
UPSTREAM = [0.3, -1.0, 2.0, 0.5]
INVALID = -1                                  # EPOS_E_INVALID


@pytest.mark.parametrize('upstream', [None, UPSTREAM])
@pytest.mark.parametrize('reduction', ['mean', 'pooled'])
def test_restatement_agrees_with_torch_fp64_autograd(reduction, upstream):
  B, P, O, F, K = 3, 61, 3, 5, 7
  c = loss_cases.make_case(B, P, O, F, seed=5, empty_images=(1,))
  rng = np.random.RandomState(11)
  A = rng.randn(B * P, K).astype(np.float32)
  widths = (O + 1, O * F, O * F * 3)
  Ws = [torch.from_numpy(0.5 * rng.randn(K, n)).double().requires_grad_() for n in widths]
  bs = [torch.from_numpy(0.5 * rng.randn(n)).double().requires_grad_() for n in widths]
  A64 = torch.from_numpy(A).double()
  shapes = [(B, P, O + 1), (B, P, O, F), (B, P, O, F, 3)]
  leaves = []
  for k, name in enumerate(('obj_logits', 'frag_logits', 'frag_loc')):
    lin = (A64 @ Ws[k] + bs[k]).reshape(shapes[k])
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
  sums, abs_sums, n_terms = heads_wgrad_ref.wgrads(A, *d, cls, frag)
  u = loss_grad_ref.upstream_factors(upstream)
  absA = np.abs(A.astype(np.float64)).reshape(B, P, K)
  for k, (head, row_len) in enumerate(zip(heads_wgrad_ref.HEADS, (O + 1, F, 3))):
    # the logit gradients' tolerance of tests/test_loss_grad_host.py, |s_bk u_k| 64 row 2^-52
    # per element, carried through the sum over the pixels, plus the order of that sum
    per_pixel = np.array([abs(scale[b, k] * u[k]) * 64 * row_len * 2.0 ** -52 for b in range(B)])
    tol_W = (absA.sum(axis=1) * per_pixel[:, None]).sum(axis=0)[:, None] + \
        (n_terms[head] + 16.0) * 2.0 ** -52 * abs_sums[head][0]
    tol_b = P * per_pixel.sum() + (n_terms[head] + 16.0) * 2.0 ** -52 * abs_sums[head][1]
    exp_W, exp_b = Ws[k].grad.numpy(), bs[k].grad.numpy()
    assert np.abs(exp_W).max() > 0 and np.abs(exp_b).max() > 0
    assert (np.abs(sums[head][0] - exp_W) <= tol_W).all(), head
    assert (np.abs(sums[head][1] - exp_b) <= tol_b).all(), head


def hand_case(gt_obj, gt_frag, weight):
  O, F, P = 2, 3, len(gt_obj)
  c = {'obj_logits': np.zeros((1, P, O + 1), np.float32),
       'frag_logits': np.zeros((1, P, O, F), np.float32),
       'frag_loc': np.zeros((1, P, O, F, 3), np.float32),
       'gt_obj': np.array([gt_obj]), 'gt_frag': np.array([gt_frag]),
       'gt_loc': np.zeros((1, P, 3), np.float32),
       'gt_weight': np.array([weight], np.float32)}
  return c, O, F


def test_hand_computed_values():
  # one foreground pixel (object 2, fragment 1), one background, one ignored
  c, O, F = hand_case([2, 0, IGNORE], [1, -1, -1], [0.5, 0.0, 0.0])
  c['frag_loc'][0, 0, 1, 1] = [0.5, 1.0, 3.0]
  A = np.array([[2.0, -3.0], [5.0, 7.0], [np.nan, np.nan]], np.float32)   # the ignored row: unread
  _, counts, _ = loss_cases.ref_terms(loss_ref, c, share=64)
  scale = loss_grad_ref.scales(counts, (1.0, 1.0, 100.0), 0)
  d = loss_grad_ref.grads(c, scale, None, IGNORE, rounded=False)
  cls, frag = heads_wgrad_ref.classes(c, IGNORE)
  assert cls.tolist() == [2, 0, -1]
  sums, abs_sums, n_terms = heads_wgrad_ref.wgrads(A, *d, cls, frag)
  a = A[0].astype(np.float64)
  dW = sums['frag'][0].reshape(2, O, F)
  assert (dW[:, 1, :] == np.outer(a, d[1][0, 0, 1])).all() and not dW[:, 0, :].any()
  assert (sums['frag'][1].reshape(O, F)[1] == d[1][0, 0, 1]).all()
  assert n_terms['frag'].reshape(O, F).tolist() == [[0, 0, 0], [1, 1, 1]]
  dWl = sums['loc'][0].reshape(2, O, F, 3)
  assert (dWl[:, 1, 1] == np.outer(a, d[2][0, 0, 1, 1])).all()
  assert np.count_nonzero(dWl) == 6 and np.count_nonzero(sums['loc'][1]) == 3
  # the object head: both valid pixels, 1/3 - [c == g] each, the ignored pixel stays out
  s0, third = scale[0, 0], 1.0 / 3
  exp = np.outer(A[0], [s0 * third, s0 * third, s0 * (third - 1.0)]) + \
      np.outer(A[1], [s0 * (third - 1.0), s0 * third, s0 * third])
  assert np.abs(sums['obj'][0] - exp).max() <= 1e-15 and np.isfinite(sums['obj'][0]).all()
  assert n_terms['obj'].tolist() == [2, 2, 2]
  assert (abs_sums['obj'][0] >= np.abs(sums['obj'][0])).all()
  # no foreground: zero fragment and localisation gradients
  c, O, F = hand_case([0, 0, IGNORE], [-1, -1, -1], [0.0, 0.0, 0.0])
  _, counts, _ = loss_cases.ref_terms(loss_ref, c, share=64)
  scale = loss_grad_ref.scales(counts, (1.0, 1.0, 100.0), 0)
  d = loss_grad_ref.grads(c, scale, None, IGNORE, rounded=False)
  sums, _, n_terms = heads_wgrad_ref.wgrads(A, *d, *heads_wgrad_ref.classes(c, IGNORE))
  for head in ('frag', 'loc'):
    assert not sums[head][0].any() and not sums[head][1].any() and not n_terms[head].any()
  assert sums['obj'][0].any()
  # a bad pixel (fragment label out of range, weight 0) contributes nothing anywhere
  c, O, F = hand_case([1, 2], [3, 0], [1.0, 0.0])
  assert heads_wgrad_ref.classes(c, IGNORE)[0].tolist() == [-1, -1]


def test_bound_is_the_stated_formula():
  b = heads_wgrad_ref.bound(np.array([3.0, -4.0]), np.array([10.0, 0.0]), np.array([5, 0]))
  assert b.tolist() == [2.0 ** -24 * 3 + 21 * 2.0 ** -52 * 10 + 2.0 ** -149,
                        2.0 ** -24 * 4 + 2.0 ** -149]
  ok, worst = heads_wgrad_ref.within(np.float32([3.0, np.nan]), np.array([3.0, np.nan]),
                                     np.array([3.0, np.nan]), np.array([1, 1]))
  assert ok and worst == 0.0
  assert not heads_wgrad_ref.within(np.float32([3.0, 1.0]), np.array([3.0, np.nan]),
                                    np.array([3.0, np.nan]), np.array([1, 1]))[0]
  assert not heads_wgrad_ref.within(np.float32([3.000001]), np.array([3.0]), np.array([3.0]),
                                    np.array([1]))[0]


def test_momentum_restatement_against_hand_values():
  f = np.float32
  w, a, g = f([1.0, -2.0]), f([0.5, 0.25]), f([0.125, 4.0])
  # momentum = 0 is plain SGD on the regularised gradient
  w2, a2 = heads_wgrad_ref.momentum_step(w, a, g, 0.5, 0.0, 0.0, 1.0)
  assert a2.tolist() == [0.125, 4.0] and w2.tolist() == [1.0 - 0.0625, -4.0]
  # weight_decay acts before the multiplier: 2 * (g + 0.25 * w)
  w2, a2 = heads_wgrad_ref.momentum_step(w, a, g, 1.0, 0.0, 0.25, 2.0)
  assert a2.tolist() == [2 * (0.125 + 0.25), 2 * (4.0 - 0.5)]
  assert w2.tolist() == [1.0 - 0.75, -2.0 - 7.0]
  # the accumulator: a' = 0.5 * a + g, w' = w - 0.25 * a'
  w2, a2 = heads_wgrad_ref.momentum_step(w, a, g, 0.25, 0.5, 0.0, 1.0)
  assert a2.tolist() == [0.375, 4.125] and w2.tolist() == [1.0 - 0.09375, -2.0 - 1.03125]
  # each operation rounded once in fp32: 1 + 2^-24 rounds to 1 before the next step sees it
  w2, a2 = heads_wgrad_ref.momentum_step(f([1.0]), f([0.0]), f([2.0 ** -24]), 1.0, 0.0, 1.0, 1.0)
  assert a2[0] == f(1.0) and w2[0] == f(0.0) and w2.dtype == np.float32


# ---------------------------------------------------------------- binding ---
FAKE = ctypes.c_void_p(4096)            # a non-null pointer no refused call dereferences
C_NAMES = {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t', ctypes.c_float: 'float'}


def test_symbols_are_declared_and_bound():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  for name, ctype in (('epos_heads_wgrad_workspace_bytes', 'int64_t'),
                      ('epos_heads_wgrad_range_pixels', 'int64_t'),
                      ('epos_heads_wgrad_f32', 'int'), ('epos_momentum_step_f32', 'int')):
    restype, argtypes = _lib.SYMBOLS[name]
    assert C_NAMES[restype] == ctype, name
    decl = re.search(r'\b%s %s\s*\(([^)]*)\)\s*;' % (ctype, name), header)
    assert decl, name
    args = [a.strip() for a in decl.group(1).split(',')]
    assert len(args) == len(argtypes), name
    for arg, t in zip(args, argtypes):                   # pointer or the scalar type by name
      if '*' in arg:
        assert t is ctypes.c_void_p, (name, arg)
      else:
        assert arg.split()[0] == C_NAMES[t], (name, arg)
  assert _lib.load().epos_abi_version() == 7


SIZES = [(1, 1, 1, 1, 1), (3, 257, 1, 1, 256), (3, 63, 21, 256, 8), (1, 19200, 21, 64, 256),
         (8, 19200, 21, 64, 256), (2, 100, 3, 65, 1024), (65535, 7, 4095, 256, 3), (0, 50, 3, 5, 4),
         (4, 0, 3, 5, 4), (1, 2047, 3, 5, 3), (1, 2048, 3, 5, 3), (3, 2049, 3, 5, 3),
         (1, 3073, 3, 5, 3), (2, 8200, 3, 5, 3), (1, 100000, 3, 5, 3), (1, 4111, 3, 5, 256),
         (1, 4112, 3, 5, 256), (1, 2 ** 20, 1, 1, 1024), (1, 2 ** 20, 1, 2, 1024),
         (1, 2 ** 31, 4095, 256, 1024)]


def ranges(P, O, F, K):
  """The header's R."""
  N = O + 1 + 4 * O * F
  return 1 if N < 10 else min(8, max(1, P // max(1024, 8 * (K + 1))))


def test_workspace_formula_and_range():
  from epos_amd import _lib
  lib = _lib.load()
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  assert 'R = 1 when N < 10, else min(8, max(1, floor(P / max(1024, 8 (K+1)))))' in header
  assert ('epos_heads_wgrad_workspace_bytes(B, P, O, F, K) = 20 * B * P + '
          '(R > 1 ? R * 8 * (K+1) * N : 0),') in header
  seen = set()
  for B, P, O, F, K in SIZES:
    R, N = ranges(P, O, F, K), O + 1 + 4 * O * F
    seen.add(R)
    got = lib.epos_heads_wgrad_workspace_bytes(B, P, O, F, K)
    assert got == 20 * B * P + (R * 8 * (K + 1) * N if R > 1 else 0), (B, P, O, F, K)
    if B * P:
      assert got < 4 * B * P * N                         # below the dense gradients
    # a function of its arguments only: there is no B to pass
    assert lib.epos_heads_wgrad_range_pixels(P, O, F, K) == -(-P // R)
  assert seen >= {1, 2, 3, 8}
  assert ranges(19200, 21, 64, 256) == 8 and ranges(2 ** 20, 1, 1, 1024) == 1
  for args, msg in (((1, 10, 0, 5, 4), b'num_objs must be in 1..4095'),
                    ((1, 10, 3, 257, 4), b'num_frags must be in 1..256'),
                    ((-1, 10, 3, 5, 4), b'B must be >= 0'),
                    ((1, -1, 3, 5, 4), b'P must be in 0..2^31'),
                    ((1, 10, 3, 5, 0), b'K must be in 1..1024'),
                    ((1, 10, 3, 5, 1025), b'K must be in 1..1024')):
    assert lib.epos_heads_wgrad_workspace_bytes(*args) == INVALID, args
    assert lib.epos_last_error() == b'epos_heads_wgrad_workspace_bytes: ' + msg
  assert lib.epos_heads_wgrad_range_pixels(10, 3, 5, 0) == INVALID
  assert lib.epos_last_error() == b'epos_heads_wgrad_range_pixels: K must be in 1..1024'


def test_host_side_refusals_of_epos_heads_wgrad_f32():
  from epos_amd import _lib
  lib = _lib.load()
  O, F, K = 3, 5, 4
  OUT = ctypes.c_void_p(8192)

  def call(B=1, P=10, O=O, F=F, K=K, lda=K, ld=O + 1, A=FAKE, obj=FAKE, scales=FAKE,
           upstream=None, ws=FAKE, outs=(OUT, None, None, None, None, None)):
    return lib.epos_heads_wgrad_f32(A, lda, K, obj, ld, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, B, P,
                                    O, F, IGNORE, scales, upstream, ws, *outs, None)
  only = lambda i, p=OUT: tuple(p if j == i else None for j in range(6))       # noqa: E731
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
                      ({'K': 0, 'lda': 4}, b'K must be in 1..1024'),
                      ({'K': 1025, 'lda': 1025}, b'K must be in 1..1024'),
                      ({'lda': K - 1}, b'lda must be >= K'),
                      ({'ld': O}, b'ld_obj must be >= num_objs + 1'),
                      ({'A': None}, b'null pointer'),
                      ({'obj': None}, b'null pointer'),
                      ({'scales': None}, b'null pointer'),
                      ({'ws': None}, b'null pointer'),
                      ({'ws': ctypes.c_void_p(4100)}, b'workspace must be 8-byte aligned'),
                      ({'outs': only(0, FAKE)}, b'an output buffer starts at an input pointer'),
                      ({'outs': only(3, FAKE)}, b'an output buffer starts at an input pointer'),
                      ({'outs': only(5, FAKE)}, b'an output buffer starts at an input pointer'),
                      ({'outs': only(2), 'upstream': OUT},
                       b'an output buffer starts at an input pointer'),
                      ({'outs': only(4), 'ws': OUT},
                       b'an output buffer starts at an input pointer')):
    assert call(**kwargs) == INVALID, kwargs
    assert lib.epos_last_error() == b'epos_heads_wgrad_f32: ' + msg, kwargs
  # nothing asked for: returns 0 and launches nothing, null inputs or not
  none = (None,) * 6
  assert call(outs=none) == 0 and call(outs=none, A=None, scales=None, ws=None) == 0
  assert call(B=0, outs=none) == 0 and call(P=0, outs=none) == 0


def test_host_side_refusals_of_epos_momentum_step_f32():
  from epos_amd import _lib
  lib = _lib.load()

  def call(n=4, w=FAKE, a=FAKE, g=FAKE):
    return lib.epos_momentum_step_f32(w, a, g, n, 0.1, 0.9, 0.0, 1.0, None)
  for kwargs, msg in (({'n': -1}, b'n must be >= 0'),
                      ({'w': None}, b'null pointer'), ({'a': None}, b'null pointer'),
                      ({'g': None}, b'null pointer'),
                      ({'n': 2 ** 38 + 1}, b'n must be <= 2^38'),
                      ({'g': ctypes.c_void_p(4098)}, b'pointers must be 4-byte aligned')):
    assert call(**kwargs) == INVALID, kwargs
    assert lib.epos_last_error() == b'epos_momentum_step_f32: ' + msg
  assert call(n=0) == 0 and call(n=0, w=None, a=None, g=None) == 0


def test_heads_train_imports_without_torch():
  code = ('import sys; sys.modules["torch"] = None\n'
          'from epos_amd import heads_train\n'
          'assert heads_train.variable_names("pred_obj_conf") == '
          '("logits/pred_obj_conf/weights", "logits/pred_obj_conf/biases")\n'
          'assert "torch" not in [m for m in sys.modules if sys.modules[m] is not None]\n')
  subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)


def test_python_entries_refuse_host_tensors():
  from epos_amd import heads_train
  from epos_amd._lib import EposError
  O, F, K = 3, 5, 4
  c = loss_cases.make_case(1, 6, O, F, seed=0)
  logits = {'pred_obj_conf': torch.from_numpy(c['obj_logits']),
            'pred_frag_conf': torch.from_numpy(c['frag_logits']),
            'pred_frag_loc': torch.from_numpy(c['frag_loc'])}
  gt = {'obj_label': torch.from_numpy(c['gt_obj']), 'frag_label': torch.from_numpy(c['gt_frag']),
        'frag_loc': torch.from_numpy(c['gt_loc']), 'frag_weight': torch.from_numpy(c['gt_weight'])}
  with pytest.raises(EposError, match='need a HIP device'):
    heads_train.heads_weight_grads(torch.zeros((6, K)), logits, gt,
                                   torch.zeros((1, 3), dtype=torch.float64))
  with pytest.raises(EposError, match='needs a HIP device'):
    heads_train.momentum_step(torch.zeros(4), torch.zeros(4), torch.zeros(4), 0.1)
