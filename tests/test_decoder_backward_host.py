"""Host side of the backward pass through decoder_conv1: the numpy restatements
(tests/helpers/decoder_backward_ref.py) against torch's fp64 autograd, the binding of the new
symbols, the host-side refusals, the torch-free import and what the plan records for the depthwise
layer."""
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

from tests.helpers import decoder_backward_ref as ref                     # noqa: E402
from tests.helpers import pointwise_wgrad_ref as wref                     # noqa: E402

INVALID = -1                                  # EPOS_E_INVALID
EPS = 1e-5


@pytest.mark.parametrize('rate', [1, 3])
def test_restatements_agree_with_torch_fp64_autograd(rate):
  """x -> depthwise(rate) -> BN -> ReLU -> 1x1 -> BN scale, with a random cotangent at the 1x1
  layer's pre-activation: dw, dgamma, dbeta of the depthwise layer and dX, to 1e-12 relative."""
  B, H, Wd, C, N = 2, 5, 7, 8, 6
  rng = np.random.RandomState(rate)
  x = rng.randn(B, H, Wd, C).astype(np.float32)
  w = (0.5 * rng.randn(3, 3, C, 1)).astype(np.float32)
  gamma = (0.5 + rng.rand(C)).astype(np.float32) * np.where(np.arange(C) % 3 == 0, -1, 1)
  gamma = gamma.astype(np.float32)
  beta = (0.3 * rng.randn(C)).astype(np.float32)
  mean = (0.2 * rng.randn(C)).astype(np.float32)
  var = (0.2 + rng.rand(C)).astype(np.float32)
  W2 = (0.5 * rng.randn(C, N)).astype(np.float32)
  gamma2 = rng.randn(N).astype(np.float32)
  var2 = (0.2 + rng.rand(N)).astype(np.float32)
  G = rng.randn(B * H * Wd, N).astype(np.float32)          # the cotangent

  xt = torch.from_numpy(x).double().requires_grad_()
  wt = torch.from_numpy(w).double().requires_grad_()
  gt_ = torch.from_numpy(gamma).double().requires_grad_()
  bt = torch.from_numpy(beta).double().requires_grad_()
  mt, vt = torch.from_numpy(mean).double(), torch.from_numpy(var).double()
  conv = torch.nn.functional.conv2d(
      xt.permute(0, 3, 1, 2), wt[:, :, :, 0].permute(2, 0, 1).unsqueeze(1), padding=rate,
      dilation=rate, groups=C).permute(0, 2, 3, 1)
  rstd = 1.0 / torch.sqrt(vt + EPS)
  a = torch.relu(gt_ * rstd * conv + (bt - mt * gt_ * rstd))
  Wf = ref.fold(W2, gamma2, var2, EPS)                     # the matrix the forward multiplies by
  z = a.reshape(-1, C) @ torch.from_numpy(Wf).double()
  (z * torch.from_numpy(G).double()).sum().backward()

  # the restatements, chained as trainer.decoder_conv1_grads chains the kernels
  A = a.detach().numpy().reshape(-1, C)
  D, _ = ref.pointwise_dgrad(G, Wf, mask=A)
  D4 = D.reshape(B, H, Wd, C)
  T, t, _, _ = ref.depthwise_wgrad(x, D4, rate)
  scale = (gamma.astype(np.float64) * rstd.numpy())
  dw, dgamma, dbeta = wref.close(T, t, w.reshape(9, C), gamma, mean, var, EPS, scale=scale)
  w9c = w.reshape(9, C).astype(np.float64) * scale[None, :]
  dX = np.zeros_like(D4)
  for ky in range(3):
    for kx in range(3):
      dX += w9c[3 * ky + kx] * ref._shifted(D4, -(ky - 1) * rate, -(kx - 1) * rate)

  def close_to(got, want, what):
    err = np.abs(got - want).max()
    assert err <= 1e-12 * np.abs(want).max(), (what, err)
  close_to(dw.reshape(3, 3, C, 1), wt.grad.numpy(), 'dw')
  close_to(dgamma, gt_.grad.numpy(), 'dgamma')
  close_to(dbeta, bt.grad.numpy(), 'dbeta')
  close_to(dX, xt.grad.numpy(), 'dX')
  assert np.abs(xt.grad.numpy()).max() > 0 and (A > 0).any() and (A == 0).any()
  # the bit-exact restatement of the depthwise input gradient is that same sum on fp32 inputs
  D32, w32 = D4.astype(np.float32), w9c.astype(np.float32)
  exact = np.zeros_like(D4)
  for ky in range(3):
    for kx in range(3):
      exact += w32[3 * ky + kx].astype(np.float64) * ref._shifted(
          D32.astype(np.float64), -(ky - 1) * rate, -(kx - 1) * rate)
  got = ref.depthwise_dgrad(D32, w32, rate)
  assert got.dtype == np.float32 and np.array_equal(got, exact.astype(np.float32))
  masked = ref.depthwise_dgrad(D32, w32, rate, Y=x)
  assert np.array_equal(masked, np.where(x <= 0, np.float32(0), got))
  assert not masked[x <= 0].view(np.uint32).any()
  # and depthwise_forward is the layer: the A autograd went through
  bias = beta.astype(np.float64) - mean.astype(np.float64) * scale
  fwd = ref.depthwise_forward(x, w9c, bias, rate)
  assert np.abs(fwd - a.detach().numpy()).max() <= 1e-12


def test_fold_mask_and_bounds():
  W = np.float32([[1.5, -2.0], [0.25, 3.0]])
  gamma, var = np.float32([2.0, -1.0]), np.float32([0.75, 0.5])
  sc = [np.float32(2.0 / np.sqrt(np.float64(np.float32(0.75)) + EPS)),
        np.float32(-1.0 / np.sqrt(0.5 + EPS))]
  Wf = ref.fold(W, gamma, var, EPS)
  assert Wf.dtype == np.float32
  assert Wf.tolist() == [[np.float32(1.5) * sc[0], np.float32(-2.0) * sc[1]],
                         [np.float32(0.25) * sc[0], np.float32(3.0) * sc[1]]]
  assert np.array_equal(ref.fold(W), W)
  G = np.float32([[1.0, 2.0], [3.0, -1.0]])
  mask = np.float32([[1.0, -0.0], [np.nan, 0.5]])
  D, A = ref.pointwise_dgrad(G, W, mask)
  assert D.tolist() == [[1.5 - 4.0, 0.0], [4.5 + 2.0, 0.75 - 3.0]]       # -0.0 masks, NaN does not
  assert A.tolist() == [[5.5, 0.0], [6.5, 3.75]]
  assert not D[0, 1:].view(np.uint64).any()
  b = ref.bound_pointwise_dgrad(2, D, A)
  assert b[0, 0] == 2.0 ** -24 * 2.5 + 18 * 2.0 ** -52 * 5.5
  assert ref.bound_depthwise_wgrad(4, np.array([10.0])).tolist() == [20 * 2.0 ** -52 * 10]
  # fp16 pairs: only the sign of hi + mid 2^-11 matters
  raw = wref.h2_split(np.float32([[0.0, -3.0, 5.0, 1e-15]]), 2.0 ** 10)
  v = ref.pair_values(raw, 4)
  assert v[0, 0] == 0 and v[0, 1] < 0 and v[0, 2] > 0 and v[0, 3] == 0   # flushed to zero
  # a tap in the padding adds nothing: rate 3 on H = 3 leaves the centre row of taps
  X = np.ones((1, 3, 4, 4))
  T, t, _, _ = ref.depthwise_wgrad(X, X, 3)
  assert not T[:3].any() and not T[6:].any() and T[4, 0] == 12 and T[3, 0] == 3 and t[0] == 12


# ---------------------------------------------------------------- binding ---
C_NAMES = {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t', ctypes.c_float: 'float',
           ctypes.c_double: 'double'}


def _struct_fields(header, name):
  body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), header, flags=re.S).group(1)
  fields = []
  for stmt in body.split(';'):
    stmt = stmt.strip()
    if stmt:
      first, *rest = [p.strip() for p in stmt.split(',')]
      fields.append(first.split()[-1].lstrip('*'))
      fields += [r.lstrip('*') for r in rest]
  return fields


def test_symbols_are_declared_bound_and_exported():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  assert 'Pointwise input gradient (csrc/pointwise_dgrad.hip' in header
  assert 'Depthwise gradients (csrc/depthwise_grad.hip' in header
  assert 'D[p,k] = fl32( sum_c (double)G[p,c] * (double)Wf[k,c] )' in header
  assert 'that the split flushed to zero is masked' in header
  # both sections say that the depthwise closing is the pointwise closing entry with K = 9
  wgrad = header[header.index('/* Pointwise weight gradient ('):header.index(
      '/* Pointwise input gradient (')]
  depthwise = header[header.index('/* Depthwise gradients ('):]
  assert 'It is also the closing of the depthwise gradients' in wgrad and 'with K = 9' in wgrad
  assert 'epos_pointwise_wgrad_close_f32(T, t, w, K = 9, N = C' in depthwise
  assert '#define EPOS_ABI_VERSION 7' in header
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  for name, ctype, n_args in (('epos_pointwise_dgrad_workspace_bytes', 'int64_t', 2),
                              ('epos_pointwise_dgrad_f32', 'int', 2),
                              ('epos_depthwise_wgrad_range_pixels', 'int64_t', 4),
                              ('epos_depthwise_wgrad_workspace_bytes', 'int64_t', 4),
                              ('epos_depthwise_wgrad_f32', 'int', 2),
                              ('epos_depthwise_dgrad_f32', 'int', 13)):
    restype, argtypes = _lib.SYMBOLS[name]
    assert C_NAMES[restype] == ctype
    decl = re.search(r'\b%s %s\s*\(([^)]*)\)\s*;' % (ctype, name), header)
    assert decl, name
    args = [a.strip() for a in decl.group(1).split(',')]
    assert len(args) == len(argtypes) == n_args, name
    for arg, t in zip(args, argtypes):                     # pointer or the scalar type by name
      if '*' in arg:
        assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), arg
      else:
        assert arg.split()[0] == C_NAMES[t], arg
    assert getattr(ctypes.CDLL(_lib.lib_path()), name)     # exported by the built library
  for struct, cls, size in (('EposPointwiseDgradArgs', _lib.PointwiseDgradArgs, 112),
                            ('EposDepthwiseWgradArgs', _lib.DepthwiseWgradArgs, 80)):
    assert _struct_fields(header, struct) == [f[0] for f in cls._fields_]
    assert ctypes.sizeof(cls) == size
  for unit in ('pointwise_dgrad.hip', 'depthwise_grad.hip'):
    assert os.path.exists(os.path.join(ROOT, 'epos_amd', 'csrc', unit))
  assert _lib.load().epos_abi_version() == 7               # added without a version change


def test_pointwise_dgrad_host_side_refusals():
  from epos_amd import _lib
  lib = _lib.load()
  fake = 4096

  def call(**over):
    f = dict(G=fake, ldg=8, W=fake * 2, gamma=fake * 3, moving_variance=fake * 4, eps=EPS,
             mask=fake * 5, ldm=8, mask_h2=0, M=10, K=8, N=8, D=fake * 6, ldd=8,
             workspace=fake * 7)
    f.update(over)
    return lib.epos_pointwise_dgrad_f32(ctypes.byref(_lib.PointwiseDgradArgs(**f)), None)
  positive = b'M, K and N must be positive'
  wide = b'K and N must be in 1..1024'
  null = b'null pointer'
  together = b'gamma and moving_variance are given together or not at all'
  eps = b'eps must be a non-negative number'
  aligned = (b'G, W, D, mask, gamma and moving_variance must be 4-byte aligned, the workspace '
             b'16-byte aligned')
  pairs = b'a pre-split mask needs K % 4 == 0, ldm % 4 == 0 and 16-byte aligned rows'
  for over, msg in ((dict(M=0), positive), (dict(K=0), positive), (dict(N=-1), positive),
                    (dict(K=1025, ldd=1025, ldm=1025), wide), (dict(N=1025, ldg=1025), wide),
                    (dict(ldg=7), b'ldg must be >= N'), (dict(ldd=7), b'ldd must be >= K'),
                    (dict(ldm=7), b'ldm must be >= K'),
                    (dict(G=None), null), (dict(W=None), null), (dict(D=None), null),
                    (dict(workspace=None), null),
                    (dict(moving_variance=None), together), (dict(gamma=None), together),
                    (dict(eps=-1.0), eps), (dict(eps=float('nan')), eps),
                    (dict(G=fake + 2), aligned), (dict(D=fake * 6 + 1), aligned),
                    (dict(mask=fake * 5 + 2), aligned), (dict(workspace=fake * 7 + 8), aligned),
                    (dict(mask_h2=1, K=6, ldd=8), pairs), (dict(mask_h2=1, ldm=10), pairs),
                    (dict(mask_h2=1, mask=fake * 5 + 4), pairs),
                    (dict(D=fake), b'D may not start at G or at mask'),
                    (dict(D=fake * 5), b'D may not start at G or at mask')):
    assert call(**over) == INVALID, over
    assert lib.epos_last_error() == b'epos_pointwise_dgrad_f32: ' + msg, over
  assert lib.epos_pointwise_dgrad_f32(None, None) == INVALID
  assert lib.epos_last_error() == b'epos_pointwise_dgrad_f32: null args'
  nbytes = lib.epos_pointwise_dgrad_workspace_bytes
  assert nbytes(256, 256) == 8 * 256 * 256 and nbytes(1, 1) == 8 * 64 * 16
  assert nbytes(132, 200) == 8 * 192 * 208 and nbytes(1024, 1024) == 8 << 20
  assert nbytes(0, 8) == INVALID and nbytes(8, 1025) == INVALID


def test_depthwise_grad_host_side_refusals():
  from epos_amd import _lib
  lib = _lib.load()
  fake = 4096

  def wgrad(**over):
    f = dict(X=fake, ldx=8, D=fake * 2, ldd=8, B=1, H=4, W=4, C=8, stride=1, rate=1, T=fake * 3,
             t=fake * 4, workspace=fake * 5)
    f.update(over)
    return lib.epos_depthwise_wgrad_f32(ctypes.byref(_lib.DepthwiseWgradArgs(**f)), None)
  positive = b'B, H, W and C must be positive'
  for over, msg in ((dict(B=0), positive), (dict(H=0), positive), (dict(W=-1), positive),
                    (dict(C=0), positive), (dict(C=6), b'C must be a multiple of 4'),
                    (dict(stride=2), b'stride must be 1'), (dict(rate=0), b'rate must be >= 1'),
                    (dict(ldx=4), b'ldx must be >= C and a multiple of 4'),
                    (dict(ldx=10), b'ldx must be >= C and a multiple of 4'),
                    (dict(ldd=9), b'ldd must be >= C and a multiple of 4'),
                    (dict(X=None), b'null pointer'), (dict(D=None), b'null pointer'),
                    (dict(T=None), b'null pointer'), (dict(t=None), b'null pointer'),
                    (dict(X=fake + 4), b'X and D must be 16-byte aligned, T and t 8-byte aligned'),
                    (dict(t=fake * 4 + 4),
                     b'X and D must be 16-byte aligned, T and t 8-byte aligned'),
                    (dict(H=40, workspace=None), b'the workspace must be given, 8-byte aligned')):
    assert wgrad(**over) == INVALID, over
    assert lib.epos_last_error() == b'epos_depthwise_wgrad_f32: ' + msg, over
  assert lib.epos_depthwise_wgrad_f32(None, None) == INVALID

  def dgrad(**over):
    f = dict(D=fake, ldd=8, w9c=fake * 2, Y=fake * 3, ldy=8, dX=fake * 4, ldx=8, B=1, H=4, W=4,
             C=8, rate=1)
    f.update(over)
    return lib.epos_depthwise_dgrad_f32(f['D'], f['ldd'], f['w9c'], f['Y'], f['ldy'], f['dX'],
                                        f['ldx'], f['B'], f['H'], f['W'], f['C'], f['rate'], None)
  for over, msg in ((dict(B=0), positive), (dict(C=10), b'C must be a multiple of 4'),
                    (dict(rate=0), b'rate must be >= 1'),
                    (dict(ldd=6), b'ldd must be >= C and a multiple of 4'),
                    (dict(ldx=9), b'ldx must be >= C and a multiple of 4'),
                    (dict(ldy=4), b'ldy must be >= C and a multiple of 4'),
                    (dict(D=None), b'null pointer'), (dict(w9c=None), b'null pointer'),
                    (dict(dX=None), b'null pointer'),
                    (dict(Y=fake * 3 + 8), b'D, w9c, Y and dX must be 16-byte aligned'),
                    (dict(dX=fake), b'dX may not start at D')):
    assert dgrad(**over) == INVALID, over
    assert lib.epos_last_error() == b'epos_depthwise_dgrad_f32: ' + msg, over
  # the cut into pixel ranges is a function of (B, H, W, C) only
  pixels = lib.epos_depthwise_wgrad_range_pixels
  nbytes = lib.epos_depthwise_wgrad_workspace_bytes
  assert pixels(1, 4, 4, 8) == 64 and nbytes(1, 4, 4, 8) == 0         # one range: no slabs
  assert pixels(1, 120, 160, 256) == 75 and nbytes(1, 120, 160, 256) == 256 * 80 * 256
  assert pixels(8, 120, 160, 256) == 600 and nbytes(8, 120, 160, 256) == 256 * 80 * 256
  assert pixels(1, 80, 81, 8) == 64 and nbytes(1, 80, 81, 8) == 102 * 80 * 8
  assert pixels(0, 4, 4, 8) == INVALID and nbytes(1, 4, 4, 6) == INVALID


# ------------------------------------------------------------- the package ---
def test_modules_import_without_torch_and_entries_need_a_device():
  code = ('import sys; sys.modules["torch"] = None\n'
          'from epos_amd import decoder_train, trainer, weights\n'
          'assert callable(decoder_train.pointwise_input_grad)\n'
          'assert callable(decoder_train.depthwise_weight_grads)\n'
          'assert callable(decoder_train.depthwise_input_grad)\n'
          'assert callable(trainer.decoder_conv1_grads)\n'
          'assert list(weights.DEPTHWISE_BACKWARD_LAYERS) == [weights.DECODER_CONV1_DEPTHWISE]\n'
          'assert "torch" not in [m for m in sys.modules if sys.modules[m] is not None]\n')
  subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)
  from epos_amd import decoder_train as DT
  from epos_amd._lib import EposError
  z = torch.zeros
  with pytest.raises(EposError, match='no CPU fallback'):
    DT.pointwise_input_grad(z(4, 8), z(8, 8))
  with pytest.raises(EposError, match='no CPU fallback'):
    DT.depthwise_weight_grads(z(1, 2, 2, 8), z(1, 2, 2, 8), z(3, 3, 8, 1), (z(8), z(8), z(8)),
                              EPS)
  with pytest.raises(EposError, match='no CPU fallback'):
    DT.depthwise_input_grad(z(1, 2, 2, 8), z(9, 8))


def test_the_plan_records_the_depthwise_operand():
  from epos_amd import decoder_train as DT
  from epos_amd import net, trainer, weights
  from epos_amd._lib import EposError
  ckpt = weights.random_init('xception_65', num_objs=2, num_frags=4, seed=0)
  plan = net.EposNet(ckpt, 1, 64, 64, 2, 4, dry_run=True)
  op = plan.depthwise_operand()
  assert sorted(op) == sorted(['x', 'ldx', 'b', 'h', 'w', 'c', 'rate', 'w9c', 'bias', 'eps'])
  assert op['c'] == 256 and (op['h'], op['w']) == (16, 16) and op['rate'] == 1 and op['b'] == 1
  assert op['eps'] == weights.DEPTHWISE_BACKWARD_LAYERS[DT.DEPTHWISE_LAYER] == 1e-5
  assert tuple(op['w9c'].shape) == (9, 256) and tuple(op['bias'].shape) == (256,)
  # x is the very buffer decoder_conv0_pointwise writes behind its ReLU, and the layer's output
  # is the A of decoder_conv1_pointwise
  assert tuple(op['x'].shape) == (1, 16, 16, op['ldx']) and op['ldx'] >= 256
  assert plan._expr_of(op['x'], 0, 256) == 'relu(L:decoder/decoder_conv0_pointwise)'
  a = plan.mode.layer_operands[DT.LAYER][0]
  assert plan._expr_of(a, 0, 256) == 'relu(L:%s)' % DT.DEPTHWISE_LAYER
  trace = [t for t in plan.trace_layers if t['scope'] == DT.DEPTHWISE_LAYER][0]
  assert trace['rate'] == op['rate'] and trace['stride'] == 1 and trace['cin'] == op['c']
  with pytest.raises(ValueError, match='decoder_conv0_depthwise'):
    plan.depthwise_operand('decoder/decoder_conv0_depthwise')
  # the layer's variables and statistics: uploaded once, the same tensors at every call
  consts = plan.depthwise_constants()
  assert [tuple(t.shape) for t in consts] == [(3, 3, 256, 1), (256,), (256,), (256,)]
  assert all(a is b for a, b in zip(consts, plan.depthwise_constants()))
  with pytest.raises(ValueError, match='decoder_conv0_depthwise'):
    plan.depthwise_constants('decoder/decoder_conv0_depthwise')
  with pytest.raises(EposError, match='no CPU fallback'):                 # a dry run has no device
    trainer.decoder_conv1_grads(plan, None, {})
  bf16 = net.EposNet(ckpt, 1, 64, 64, 2, 4, dry_run=True, precision='bf16')
  with pytest.raises(NotImplementedError, match='bf16'):
    bf16.depthwise_operand()
  # nothing became trainable
  assert len(weights.trainable_variables()) == 9 and len(weights.TRAINABLE_LAYERS) == 4
  assert DT.DEPTHWISE_LAYER not in weights.TRAINABLE_LAYERS
  assert trainer.VARIABLES == DT.VARIABLES == weights.trainable_variables()
  assert DT.DEPTHWISE_VARIABLES == tuple(
      DT.DEPTHWISE_LAYER + '/' + v
      for v in ('depthwise_weights', 'BatchNorm/gamma', 'BatchNorm/beta'))
