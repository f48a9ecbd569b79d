"""The weight update without a device: the binding of epos_pack_weights_device_f32 and its
host-side refusals, trainer.learning_rate against hand-computed values, what
train_heads.prepare refuses, and the entries' behaviour on a machine without a GPU."""
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

INVALID = -1
FAKE = 4096                                 # a non-null pointer no refused call dereferences
C_NAMES = {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t', ctypes.c_float: 'float'}


def test_symbols_are_declared_and_bound():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  name = 'epos_pack_weights_device_f32'
  restype, argtypes = _lib.SYMBOLS[name]
  assert C_NAMES[restype] == 'int'
  decl = re.search(r'\bint %s\s*\(([^)]*)\)\s*;' % name, header)
  assert decl, name
  args = [a.strip() for a in decl.group(1).split(',')]
  assert len(args) == len(argtypes)
  assert args[0].startswith('const EposWeightPackArgs*')
  assert argtypes[0] is ctypes.POINTER(_lib.WeightPackArgs)
  for arg, t in zip(args[1:], argtypes[1:]):
    if '*' in arg:
      assert t is ctypes.c_void_p, arg
    else:
      assert arg.split()[0] == C_NAMES[t], arg
  # the struct, field by field
  body = re.search(r'typedef struct EposWeightPackArgs \{(.*?)\} EposWeightPackArgs;', header,
                   re.S).group(1)
  fields = []
  for stmt in body.split(';'):
    stmt = stmt.strip()
    if stmt:
      names = stmt.replace(',', ' ').split()
      if '*' in stmt:
        fields.append((names[-1], ctypes.c_void_p))
      else:
        base = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32}[names[0]]
        fields += [(n, base) for n in names[1:]]
  assert fields == list(_lib.WeightPackArgs._fields_)
  lib = _lib.load()
  assert hasattr(lib, name) and lib.epos_abi_version() == 7


def test_host_side_refusals_of_epos_pack_weights_device_f32():
  from epos_amd import _lib
  lib = _lib.load()

  def call(count=1, table=True, status=FAKE, second=None, **fields):
    good = dict(W=FAKE, ldw=8, col0=0, bias=FAKE, plain=FAKE, split=FAKE, h2=FAKE,
                bias_pad=FAKE, K=4, N=8)
    arr = (_lib.WeightPackArgs * 2)(_lib.WeightPackArgs(**dict(good, **fields)),
                                    _lib.WeightPackArgs(**dict(good, **(second or {}))))
    return lib.epos_pack_weights_device_f32(arr if table else None, count, status, None)
  for kwargs, msg in (({'table': False}, b'null problem table'),
                      ({'count': -1}, b'count must be in 0..256'),
                      ({'count': 257}, b'count must be in 0..256'),
                      ({'status': None}, b'null status'),
                      ({'status': 4098}, b'status must be 4-byte aligned'),
                      ({'K': 0}, b'K must be a multiple of 4 in 4..1024'),
                      ({'K': 6}, b'K must be a multiple of 4 in 4..1024'),
                      ({'K': 1028}, b'K must be a multiple of 4 in 4..1024'),
                      ({'N': 0}, b'N must be in 1..2^24'),
                      ({'N': 2 ** 24 + 1, 'ldw': 2 ** 25}, b'N must be in 1..2^24'),
                      ({'col0': -1}, b'need 0 <= col0 and col0 + N <= ldw <= 2^31'),
                      ({'col0': 1}, b'need 0 <= col0 and col0 + N <= ldw <= 2^31'),
                      ({'ldw': 7}, b'need 0 <= col0 and col0 + N <= ldw <= 2^31'),
                      ({'ldw': 2 ** 31 + 1}, b'need 0 <= col0 and col0 + N <= ldw <= 2^31'),
                      ({'W': None}, b'null W'),
                      ({'bias': None}, b'bias_pad needs bias'),
                      ({'W': 4098}, b'W and bias must be 4-byte aligned'),
                      ({'bias': 4097}, b'W and bias must be 4-byte aligned'),
                      ({'plain': 4100}, b'plain, split and h2 must be 16-byte aligned, '
                                        b'bias_pad 4-byte aligned'),
                      ({'split': 4104}, b'plain, split and h2 must be 16-byte aligned, '
                                        b'bias_pad 4-byte aligned'),
                      ({'h2': 4097}, b'plain, split and h2 must be 16-byte aligned, '
                                     b'bias_pad 4-byte aligned'),
                      ({'bias_pad': 4098}, b'plain, split and h2 must be 16-byte aligned, '
                                           b'bias_pad 4-byte aligned'),
                      # the second problem of the table is checked too
                      ({'count': 2, 'second': {'K': 2}},
                       b'K must be a multiple of 4 in 4..1024')):
    assert call(**kwargs) == INVALID, kwargs
    assert lib.epos_last_error() == b'epos_pack_weights_device_f32: ' + msg, kwargs
  # count = 0 returns 0 and launches nothing, whatever else it is given
  assert call(count=0) == 0 and call(count=0, status=None, W=None, K=0) == 0


def test_learning_rate_against_hand_computed_values():
  from epos_amd.trainer import learning_rate as lr
  T = 1000
  close = lambda a, b: abs(a - b) <= 4 * 2.0 ** -53 * abs(b)        # noqa: E731
  # poly, end_learning_rate = 0, the step clipped to train_steps
  assert lr(0, train_steps=T) == 1e-4
  assert close(lr(1, train_steps=T), 1e-4 * 0.999 ** 0.9)
  assert close(lr(T // 2, train_steps=T), 1e-4 * 0.5 ** 0.9)
  assert close(lr(T // 2, train_steps=T, base_learning_rate=0.007, power=2.0), 0.007 * 0.25)
  assert lr(T, train_steps=T) == 0.0 and lr(T + 5, train_steps=T) == 0.0
  # step: staircase, on either side of a decay boundary
  kw = dict(policy='step', base_learning_rate=0.01, decay_step=2000, decay_factor=0.1)
  assert lr(0, **kw) == 0.01 and lr(1999, **kw) == 0.01
  assert close(lr(2000, **kw), 0.001) and close(lr(3999, **kw), 0.001)
  assert close(lr(4000, **kw), 0.0001)
  # slow start without burn-in: the slow rate below slow_start_step, the unshifted policy from it
  kw = dict(train_steps=T, base_learning_rate=0.01, slow_start_step=100,
            slow_start_learning_rate=0.001)
  assert lr(0, **kw) == 0.001 and lr(99, **kw) == 0.001
  assert close(lr(100, **kw), 0.01 * 0.9 ** 0.9)
  # linear burn-in: rises from the slow rate; from slow_start_step on the policy runs on the
  # global step SHIFTED by slow_start_step
  assert lr(0, burnin='linear', **kw) == 0.001
  assert close(lr(99, burnin='linear', **kw), 0.001 + 0.009 * 99 / 100)
  assert lr(100, burnin='linear', **kw) == 0.01
  assert close(lr(150, burnin='linear', **kw), 0.01 * 0.95 ** 0.9)
  skw = dict(policy='step', base_learning_rate=0.01, decay_step=50, decay_factor=0.5,
             slow_start_step=100, slow_start_learning_rate=0.001, burnin='linear')
  assert lr(149, **skw) == 0.01 and close(lr(150, **skw), 0.005)
  with pytest.raises(ValueError, match='Unknown learning policy'):
    lr(0, policy='cosine')
  with pytest.raises(ValueError, match='Unknown burnin type'):
    lr(0, burnin='quadratic')
  assert isinstance(lr(3), float)


def test_train_heads_prepare_refuses_by_name(tmp_path, monkeypatch):
  import train_heads
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  base = ['--model=toy', '--dataset', 'lm', '--synthetic', '2']
  args, model_dir = train_heads.prepare(base)
  assert model_dir == str(tmp_path / 'toy')
  # the reference's names and defaults (scripts/train.py:53-149)
  assert (args.learning_policy, args.base_learning_rate, args.learning_rate_decay_factor,
          args.learning_rate_decay_step, args.learning_power, args.train_steps, args.momentum,
          args.weight_decay, args.train_batch_size, args.last_layer_gradient_multiplier,
          args.slow_start_step, args.slow_start_learning_rate, args.obj_cls_loss_weight,
          args.frag_cls_loss_weight, args.frag_loc_loss_weight, args.log_steps,
          args.save_interval_steps, args.train_crop_size, args.fine_tune_batch_norm) == (
              'poly', 1e-4, 0.1, 2000, 0.9, 2000000, 0.9, 4e-5, 1, 1.0, 0, 1e-4, 1.0, 1.0, 100.0,
              100, 50000, '640,480', False)
  for extra, name in ((['--precision', 'bf16'], '--precision bf16'),
                      (['--image_pyramid', '0.5,1.0', '--multi_scale_inference', 'true'],
                       'image_pyramid'),
                      (['--fine_tune_batch_norm', 'true'], 'fine_tune_batch_norm'),
                      (['--data_augmentations', 'random_adjust_brightness'],
                       'data_augmentations'),
                      (['--freeze_regex_list', 'xception_65'], 'freeze_regex_list'),
                      (['--freeze_regex_list', '^(?!logits)', '--freeze_regex_list', 'aspp'],
                       None)):
    if name is None:
      train_heads.prepare(base + extra)         # freezes everything below the logits
    else:
      with pytest.raises(NotImplementedError, match=re.escape(name)):
        train_heads.prepare(base + extra)
  # a params.yml sets them as well
  (tmp_path / 'toy').mkdir()
  (tmp_path / 'toy' / 'params.yml').write_text('fine_tune_batch_norm: true\n')
  with pytest.raises(NotImplementedError, match='fine_tune_batch_norm'):
    train_heads.prepare(base)


def test_heads_train_still_imports_without_torch():
  code = ('import sys; sys.modules["torch"] = None\n'
          'from epos_amd import heads_train, trainer\n'
          'assert callable(heads_train.heads_weight_grads)\n'
          'assert trainer.learning_rate(0) == 1e-4\n'
          'assert "torch" not in [m for m in sys.modules if sys.modules[m] is not None]\n')
  subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)


def test_entries_without_a_device(monkeypatch):
  from epos_amd import heads_train, net, trainer, weights
  from epos_amd._lib import EposError
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  ckpt = weights.random_init('xception_65', num_objs=2, num_frags=4, seed=0)
  six = {n: ckpt[n] for h in heads_train.HEADS for n in heads_train.variable_names(h)}
  with pytest.raises(EposError, match='no CPU fallback'):
    net.EposNet(ckpt, 1, 64, 64, 2, 4)
  plan = net.EposNet(ckpt, 1, 64, 64, 2, 4, dry_run=True)
  with pytest.raises(EposError, match='no CPU fallback'):
    plan.set_weights(six)
  with pytest.raises(EposError, match='no CPU fallback'):
    trainer.train_step(plan, None, None, None, 1e-4)


def test_nets_out_of_scope_say_so():
  from epos_amd import heads_train, multiscale, net, weights
  ckpt = weights.random_init('xception_65', num_objs=2, num_frags=4, seed=0)
  six = {n: ckpt[n] for h in heads_train.HEADS for n in heads_train.variable_names(h)}
  plan = net.EposNet(ckpt, 1, 64, 64, 2, 4, dry_run=True, precision='bf16')
  with pytest.raises(NotImplementedError, match='bf16'):
    plan.set_weights(six)
  with pytest.raises(NotImplementedError, match='multi-scale'):
    multiscale.MultiScaleNet.set_weights(None, six)
  # the plan keeps references to the logits layers' weight tensors, and nothing else changed
  plan = net.EposNet(ckpt, 1, 64, 64, 2, 4, dry_run=True)
  assert sorted(plan.mode.packs) == sorted(weights.TRAINABLE_LAYERS)
  assert sorted(s[len('logits/'):] for s in weights.LOGITS_LAYERS) == sorted(heads_train.HEADS)
  assert np.all([len(packs) == 4 for _, _, packs in plan.mode.packs.values()])


NINE = ('logits/pred_obj_conf/weights', 'logits/pred_obj_conf/biases',
        'logits/pred_frag_conf/weights', 'logits/pred_frag_conf/biases',
        'logits/pred_frag_loc/weights', 'logits/pred_frag_loc/biases',
        'decoder/decoder_conv1_pointwise/weights',
        'decoder/decoder_conv1_pointwise/BatchNorm/gamma',
        'decoder/decoder_conv1_pointwise/BatchNorm/beta')


def test_gradient_rule_gives_the_logits_variables_the_literals_of_the_logits_only_step():
  """The optimiser of the logits layers alone hard-coded (m, decay) for weights and (2 m, 0)
  for biases; gradient_rule gives the six variables the same under both scope settings."""
  from epos_amd.trainer import gradient_rule
  wd = 4e-5
  table = {1.0: {'weights': (1.0, 4e-5), 'biases': (2.0, 0.0)},
           3.0: {'weights': (3.0, 4e-5), 'biases': (6.0, 0.0)}}
  for m, want in table.items():
    for logits_only in (False, True):
      for name in NINE[:6]:
        assert gradient_rule(name, m, wd, logits_only) == want[name.rsplit('/', 1)[1]], (
            name, m, logits_only)


def test_the_table_is_the_only_source_of_names():
  from epos_amd import decoder_train, loss, net, trainer, weights
  assert loss.HEAD_VARIABLES == NINE[:6]
  assert trainer.VARIABLES == NINE and decoder_train.VARIABLES == NINE
  assert decoder_train.LAYER_VARIABLES == NINE[6:]
  assert weights.trainable_variables() == NINE
  # what set_weights accepts: a name alone is an incomplete layer, any other name is unknown
  ckpt = weights.random_init('xception_65', num_objs=2, num_frags=4, seed=0)
  plan = net.EposNet(ckpt, 1, 64, 64, 2, 4, dry_run=True)
  accepted = []
  for name in sorted(set(ckpt) | set(NINE)) + ['logits/pred_obj_conf/weights/Momentum']:
    with pytest.raises(ValueError) as err:
      plan.set_weights({name: np.zeros((1,), np.float32) if name not in ckpt else ckpt[name]})
    if 'are set together' in str(err.value):
      accepted.append(name)
    else:
      assert 'is not a variable' in str(err.value), name
  assert len(ckpt) > 100 and sorted(accepted) == sorted(NINE)
