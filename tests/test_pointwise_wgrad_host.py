"""Host side of the decoder layer's weight and batch-norm gradients: the numpy restatement
(tests/helpers/pointwise_wgrad_ref.py) against torch's fp64 autograd, the fp16-pair
reconstruction, the binding of the new symbols, train_heads.py's acceptance of the scope and the
optimiser's multiplier and decay table."""
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

from tests.helpers import pointwise_wgrad_ref as ref                      # noqa: E402

INVALID = -1                                  # EPOS_E_INVALID
EPS = 1e-5


def test_restatement_agrees_with_torch_fp64_autograd():
  """y = relu(scale (.) (A W) + bias) with scale = fl32(gamma / sqrt(var + eps)) and bias =
  beta - mean scale, followed by a random linear functional; a column with gamma = 0, a column
  whose ReLU is off everywhere, and one whose ReLU is on everywhere."""
  M, K, N = 97, 13, 9
  rng = np.random.RandomState(0)
  A = np.maximum(rng.randn(M, K), 0).astype(np.float32)
  W = (0.5 * rng.randn(K, N)).astype(np.float32)
  gamma = rng.randn(N).astype(np.float32)
  beta = (0.3 * rng.randn(N)).astype(np.float32)
  mean = rng.randn(N).astype(np.float32)
  var = (0.2 + rng.rand(N)).astype(np.float32)
  gamma[2] = 0.0
  beta[2] = 0.5                               # gamma = 0: the column is its bias, ReLU on
  beta[5] = -1e3                              # ReLU off everywhere
  beta[7] = 1e3                               # ReLU on everywhere
  R = rng.randn(M, N)

  At = torch.from_numpy(A).double()
  Wt = torch.from_numpy(W).double().requires_grad_()
  gt_ = torch.from_numpy(gamma).double().requires_grad_()
  bt = torch.from_numpy(beta).double().requires_grad_()
  mt, vt = torch.from_numpy(mean).double(), torch.from_numpy(var).double()
  rstd = 1.0 / torch.sqrt(vt + EPS)
  scale = gt_ * rstd
  # the forward multiplies with the fp32-rounded scale; its derivative is the exact one's
  scale32 = scale + (scale.detach().float().double() - scale.detach())
  # d scale32 / d gamma = rstd, while the VALUE in dW is the rounded scale: two graphs
  z = At @ Wt
  pre = scale32.detach() * z + (bt - mt * scale.detach())
  y = torch.relu(pre)
  (y * torch.from_numpy(R)).sum().backward()
  dW_auto, dbeta_auto = Wt.grad.numpy(), bt.grad.numpy()
  # gamma: through the exact scale in both places (the restatement's formula is the derivative
  # of scale z + beta - mean scale with respect to gamma at frozen statistics)
  Wt2 = torch.from_numpy(W).double()
  pre2 = scale * (At @ Wt2) + (torch.from_numpy(beta).double() - mt * scale)
  mask = (pre > 0).double()                   # the same ReLU pattern as the rounded forward
  ((pre2 * mask) * torch.from_numpy(R)).sum().backward()
  dgamma_auto = gt_.grad.numpy()

  G = (R * (pre.detach().numpy() > 0))        # the gradient at the pre-activation
  assert not G[:, 5].any() and G[:, 7].all() and G[:, 2].all()
  S, g, aS, ag = ref.sums(A, G)
  dW, dgamma, dbeta = ref.close(S, g, W, gamma, mean, var, EPS)
  scale_ref, rstd_ref = ref.fold_scale(gamma, var, EPS)
  assert np.array_equal(scale_ref, scale32.detach().numpy())
  tol = 64 * 2.0 ** -52
  assert (np.abs(dW - dW_auto) <= tol * np.abs(scale_ref)[None, :] * aS + 1e-300).all()
  assert (np.abs(dbeta - dbeta_auto) <= tol * ag + 1e-300).all()
  mag = rstd_ref * ((np.abs(W.astype(np.float64)) * aS).sum(axis=0) + np.abs(mean) * ag)
  assert (np.abs(dgamma - dgamma_auto) <= (K + 64) * 2.0 ** -52 * mag + 1e-300).all()
  # the special columns
  assert not dW[:, 5].any() and dgamma[5] == 0 and dbeta[5] == 0
  assert not dW[:, 2].any() and dgamma[2] != 0 and dbeta[2] != 0      # no division by gamma
  assert np.abs(dW).max() > 0 and np.abs(dgamma_auto).max() > 0
  # without a batch norm
  dW0, none, db0 = ref.close(S, g)
  assert none is None and np.array_equal(dW0, S) and np.array_equal(db0, g)


def h2_split_pair_numpy(x, s):
  """A restatement of h2_split_pair (csrc/h2_scale.h) of its own, element by element."""
  t = np.float32(x) * np.float32(s)
  hi = np.float16(t)
  mid = np.float16((t - np.float32(hi)) * np.float32(2048.0))
  return hi, mid


def test_pair_reconstruction_inverts_the_split():
  rng = np.random.RandomState(1)
  M, K = 23, 12
  x = (rng.randn(M, K) * 10 ** rng.uniform(-3, 1, (M, K))).astype(np.float32)
  x[0, :4] = [0.0, -0.0, 1.0, -7.5]
  bound = np.float32(np.abs(x).max())
  s, inv = ref.h2_scale(bound)
  assert 2.0 ** 14 <= s * float(bound) < 2.0 ** 15 and s * inv == 1.0
  raw = ref.h2_split(x, s)
  assert raw.dtype == np.float32 and raw.shape == (M, K)
  halves = raw.view(np.float16).reshape(M, K // 4, 2, 4)
  for p, k in ((0, 2), (3, 7), (22, 11)):
    hi, mid = h2_split_pair_numpy(x[p, k], s)
    assert halves[p, k // 4, 0, k % 4] == hi and halves[p, k // 4, 1, k % 4] == mid
  back = ref.h2_values(raw, K, inv)
  # hi + mid 2^-11 keeps 22 bits of t = x s: within 2^-22 |x|, and 2^-11 of the smallest fp16
  # subnormal where mid underflows
  err = np.abs(back - x.astype(np.float64))
  assert (err <= 2.0 ** -22 * np.abs(x) + 2.0 ** -36 * inv).all()
  assert err.max() > 0                        # the split rounds: it is no identity
  assert back[0, 0] == 0 and back[0, 2] == 1.0 and back[0, 3] == -7.5
  # padding columns behind K are not looked at
  wide = np.full((M, K + 4), np.nan, np.float32)
  wide.view(np.uint32)[:, :K] = raw.view(np.uint32)
  assert np.array_equal(ref.h2_values(wide, K, inv), back)
  # the scale of a bound: capped, and 1 for a bound that is not finite
  assert ref.h2_scale(np.float32(0.0)) == (2.0 ** 126, 2.0 ** -126)
  assert ref.h2_scale(np.float32(np.inf)) == (1.0, 1.0)
  slot = np.zeros(64, np.uint32)
  slot[9] = np.float32(3.0).view(np.uint32)
  assert ref.slot_bound(slot) == 3.0 and ref.slot_bound(slot, None, 2.0, 0.5) == 6.5
  slot2 = np.zeros(64, np.uint32)
  slot2[1] = np.float32(4.0).view(np.uint32)
  assert ref.slot_bound(slot, slot2) == 4.0


def test_bounds():
  assert ref.bound(4, np.array([10.0])).tolist() == [20 * 2.0 ** -52 * 10]
  S, g = np.array([[3.0], [-4.0]]), np.array([2.0])
  aS, ag = np.array([[5.0], [6.0]]), np.array([7.0])
  W = np.array([[0.5], [-2.0]], np.float32)
  gamma, mean, var = np.float32([1.5]), np.float32([-0.25]), np.float32([0.75])
  sc, rstd = ref.fold_scale(gamma, var, EPS)
  assert sc[0] == float(np.float32(1.5 / np.sqrt(0.75 + EPS)))
  assert rstd[0] == 1 / np.sqrt(0.75 + EPS)
  dW, dgamma, dbeta = ref.close(S, g, W, gamma, mean, var, EPS)
  assert dW.tolist() == [[sc[0] * 3.0], [sc[0] * -4.0]] and dbeta.tolist() == [2.0]
  assert dgamma[0] == rstd[0] * ((0.5 * 3.0 + -2.0 * -4.0) - -0.25 * 2.0)
  tW, tg, tb = ref.bounds_close(4, S, g, aS, ag, W, gamma, mean, var, EPS)
  bS, bg = ref.bound(4, aS), ref.bound(4, ag)
  assert tb[0] == 2.0 ** -24 * 2.0 + bg[0] + 2.0 ** -149
  assert tW[0, 0] == (2.0 ** -24 + 2.0 ** -52) * abs(dW[0, 0]) + sc[0] * bS[0, 0] + 2.0 ** -149
  want = (2.0 ** -24 * abs(dgamma[0]) +
          rstd[0] * ((0.5 * bS[0, 0] + 2.0 * bS[1, 0]) + 0.25 * bg[0]) +
          10.0 * 2.0 ** -52 * rstd[0] * ((0.5 * 3.0 + 2.0 * 4.0) + 0.25 * 2.0) + 2.0 ** -149)
  assert abs(tg[0] - want) <= 1e-15 * want
  ok, worst = ref.within(np.float32([1.0, np.nan]), np.array([1.0, np.nan]), np.array([0.0, 0.0]))
  assert ok and worst == 0.0
  assert not ref.within(np.float32([1.0]), np.array([np.nan]), np.array([1.0]))[0]
  assert not ref.within(np.float32([1.5]), np.array([1.0]), np.array([0.25]))[0]


# ---------------------------------------------------------------- binding ---
C_NAMES = {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t', ctypes.c_float: 'float',
           ctypes.c_double: 'double'}


def test_symbols_are_declared_bound_and_exported():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  assert 'Pointwise weight gradient (csrc/pointwise_wgrad.hip' in header
  assert 'dgamma_c  = rstd_c (sum_k W[k,c] S[k,c] - mean_c g_c)' in header
  assert '#define EPOS_ABI_VERSION 7' in header
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  for name, ctype, n_args in (('epos_pointwise_wgrad_workspace_bytes', 'int64_t', 3),
                              ('epos_pointwise_wgrad_range_rows', 'int64_t', 3),
                              ('epos_pointwise_wgrad_f32', 'int', 2),
                              ('epos_pointwise_wgrad_close_f32', 'int', 13)):
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
  # the struct, field by field, in the header's order
  body = re.search(r'typedef struct EposPointwiseWgradArgs \{(.*?)\} EposPointwiseWgradArgs;',
                   header, flags=re.S).group(1)
  fields = []
  for stmt in body.split(';'):
    stmt = stmt.strip()
    if stmt:
      first, *rest = [p.strip() for p in stmt.split(',')]
      fields.append(first.split()[-1].lstrip('*'))
      fields += [r.lstrip('*') for r in rest]
  assert fields == [f[0] for f in _lib.PointwiseWgradArgs._fields_]
  assert ctypes.sizeof(_lib.PointwiseWgradArgs) == 104
  assert os.path.exists(os.path.join(ROOT, 'epos_amd', 'csrc', 'pointwise_wgrad.hip'))
  assert _lib.load().epos_abi_version() == 7               # added without a version change


def test_host_side_refusals():
  from epos_amd import _lib
  lib = _lib.load()
  fake = 4096

  def call(**over):
    f = dict(A=fake, lda=8, G=fake, ldg=8, M=10, K=8, N=8, S=fake * 2, g=fake * 3,
             workspace=fake * 4)
    f.update(over)
    return lib.epos_pointwise_wgrad_f32(ctypes.byref(_lib.PointwiseWgradArgs(**f)), None)
  for over, msg in ((dict(M=0), b'M, K and N must be positive'),
                    (dict(K=-1), b'M, K and N must be positive'),
                    (dict(lda=7), b'lda must be >= K'), (dict(ldg=7), b'ldg must be >= N'),
                    (dict(A=None), b'null pointer'), (dict(g=None), b'null pointer'),
                    (dict(S=fake + 4), b'A and G must be 4-byte aligned, S and g 8-byte aligned'),
                    (dict(M=1000, workspace=None), b'the workspace must be given, 8-byte aligned'),
                    (dict(a_presplit=1), b'a pre-split A needs its absmax slot (a_amax)'),
                    (dict(a_presplit=1, a_amax=fake, A=fake + 4),
                     b'a pre-split A needs K % 4 == 0, lda % 4 == 0 and 16-byte aligned rows')):
    assert call(**over) == INVALID, over
    assert lib.epos_last_error() == b'epos_pointwise_wgrad_f32: ' + msg, over
  # the cut into row ranges is a function of (M, K, N) only
  rows = lib.epos_pointwise_wgrad_range_rows
  nbytes = lib.epos_pointwise_wgrad_workspace_bytes
  assert rows(100, 8, 8) == 100 and nbytes(100, 8, 8) == 0            # one range: no slabs
  assert rows(19200, 256, 256) == 300 and nbytes(19200, 256, 256) == 64 * 8 * (256 * 256 + 256)
  assert rows(8 * 19200, 256, 256) == 2400
  assert rows(20000, 16, 8) == 128 and nbytes(20000, 16, 8) == 157 * 8 * (16 * 8 + 8)
  assert rows(0, 8, 8) == INVALID and nbytes(8, 0, 8) == INVALID


# ------------------------------------------------------------ train_heads ---
def test_train_heads_prepare_accepts_the_layer(tmp_path, monkeypatch):
  import train_heads
  from epos_amd import decoder_train
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  base = ['--model=toy', '--dataset', 'lm', '--synthetic', '2']
  args, _ = train_heads.prepare(base)
  assert args.layer_trainable == () and args.last_layers_contain_logits_only is False
  only = '^(?!logits|decoder/decoder_conv1_pointwise)'
  args, _ = train_heads.prepare(base + ['--freeze_regex_list', only])
  assert args.layer_trainable == decoder_train.LAYER_VARIABLES
  args, _ = train_heads.prepare(base + ['--freeze_regex_list', only,
                                        '--freeze_regex_list', 'BatchNorm',
                                        '--last_layers_contain_logits_only', 'true'])
  assert args.layer_trainable == (decoder_train.LAYER + '/weights',)
  assert train_heads.cli.str2bool(args.last_layers_contain_logits_only) is True
  args, _ = train_heads.prepare(base + ['--freeze_regex_list', only,
                                        '--freeze_regex_list', 'pointwise/weights'])
  assert args.layer_trainable == decoder_train.LAYER_VARIABLES[1:]
  # everything frozen below the logits, as before: the heads-only loop
  args, _ = train_heads.prepare(base + ['--freeze_regex_list', '^(?!logits)'])
  assert args.layer_trainable == ()
  for extra, name in ((['--freeze_regex_list', 'xception_65'], 'freeze_regex_list'),
                      (['--freeze_regex_list', '^(?!logits|decoder/decoder_conv)'],
                       'decoder/decoder_conv0_depthwise/depthwise_weights'),
                      (['--freeze_regex_list', '^(?!logits|decoder/decoder_conv1)'],
                       'decoder/decoder_conv1_depthwise/depthwise_weights'),
                      (['--freeze_regex_list', only, '--fine_tune_batch_norm', 'true'],
                       'fine_tune_batch_norm')):
    with pytest.raises(NotImplementedError, match=re.escape(name)):
      train_heads.prepare(base + extra)


def test_multiplier_and_decay_table():
  from epos_amd.decoder_train import LAYER, VARIABLES
  from epos_amd.trainer import gradient_rule
  assert len(VARIABLES) == 9 and VARIABLES[6:] == (
      LAYER + '/weights', LAYER + '/BatchNorm/gamma', LAYER + '/BatchNorm/beta')
  m, wd = 10.0, 4e-5
  # last_layers_contain_logits_only=False (the reference's default): decoder is a last layer
  table = {'logits/pred_obj_conf/weights': (10.0, wd), 'logits/pred_obj_conf/biases': (20.0, 0.0),
           'logits/pred_frag_loc/weights': (10.0, wd), 'logits/pred_frag_loc/biases': (20.0, 0.0),
           LAYER + '/weights': (10.0, wd), LAYER + '/BatchNorm/gamma': (10.0, 0.0),
           LAYER + '/BatchNorm/beta': (10.0, 0.0),
           'xception_65/entry_flow/conv1_1/weights': (1.0, wd),
           'xception_65/entry_flow/conv1_1/BatchNorm/beta': (1.0, 0.0)}
  for name, want in table.items():
    assert gradient_rule(name, m, wd, False) == want, name
  # True: the logits layers only
  table.update({LAYER + '/weights': (1.0, wd), LAYER + '/BatchNorm/gamma': (1.0, 0.0),
                LAYER + '/BatchNorm/beta': (1.0, 0.0)})
  for name, want in table.items():
    assert gradient_rule(name, m, wd, True) == want, name
  # the defaults: multiplier 1 (biases 2), decay 4e-5 on weights
  assert gradient_rule(LAYER + '/weights') == (1.0, 4e-5)
  assert gradient_rule('logits/pred_frag_conf/biases') == (2.0, 0.0)


def test_module_imports_without_torch_and_entries_need_a_device(monkeypatch):
  code = ('import sys; sys.modules["torch"] = None\n'
          'from epos_amd import decoder_train, trainer\n'
          'assert callable(decoder_train.pointwise_weight_grads)\n'
          'assert trainer.gradient_rule("logits/x/biases", 3.0) == (6.0, 0.0)\n'
          'assert "torch" not in [m for m in sys.modules if sys.modules[m] is not None]\n')
  subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)
  from epos_amd import decoder_train, net, trainer, weights
  from epos_amd._lib import EposError
  with pytest.raises(EposError, match='no CPU fallback'):
    decoder_train.pointwise_weight_grads(torch.zeros(4, 8), torch.zeros(4, 8),
                                         torch.zeros(8, 8))
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  ckpt = weights.random_init('xception_65', num_objs=2, num_frags=4, seed=0)
  with pytest.raises(EposError, match='no CPU fallback'):
    trainer.Optimizer(ckpt, 1e-4, trainable=decoder_train.VARIABLES)
  with pytest.raises(EposError, match='no CPU fallback'):
    trainer.train_step(None, None, None, None, 1e-4)
  plan = net.EposNet(ckpt, 1, 64, 64, 2, 4, dry_run=True)
  nine = {n: ckpt[n] for n in decoder_train.VARIABLES}
  with pytest.raises(EposError, match='no CPU fallback'):
    plan.set_weights(nine)
  with pytest.raises(EposError, match='no CPU fallback'):
    plan.pointwise_operand()
  # the plan recorded the layer while it was built: A is the depthwise output, K = N = 256
  a, lda, m, k, n, args, ab = plan.mode.layer_operands[decoder_train.LAYER]
  packs = plan.mode.packs[decoder_train.LAYER][2]
  assert plan.mode.packs[decoder_train.LAYER][:2] == (k, n)
  assert (lda, k, n) == (256, 256, 256) and m == 16 * 16 and tuple(a.shape) == (1, 16, 16, 256)
  assert args.M == m and args.K == k and args.N == n and len(packs) == 4
  bf16 = net.EposNet(ckpt, 1, 64, 64, 2, 4, dry_run=True, precision='bf16')
  with pytest.raises(NotImplementedError, match='bf16'):
    bf16.set_weights(nine)
  with pytest.raises(NotImplementedError, match='bf16'):
    bf16.pointwise_operand()
