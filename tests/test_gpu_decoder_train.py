"""Training decoder/decoder_conv1_pointwise on the device (epos_amd/decoder_train.py and
trainer.py, EposNet.pointwise_operand and set_weights, train_heads.py with the layer unfrozen) on the
small net of tests/helpers/loss_device.py: the gradients against their parts and against
tests/helpers/pointwise_wgrad_ref.py fed the net's own A bytes and the device's own G, the
in-place weight update against a freshly built net, a training step against its parts, and the
command line end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import loss_cases, mesh_cases, pointwise_wgrad_ref as ref     # noqa: E402
from tests.helpers.loss_device import (NET_B, NET_F, NET_H, NET_O, NET_W,     # noqa: E402,F401
                                       gt_tensors, small_net)

pytestmark = pytest.mark.gpu

LOSS_WEIGHTS = (0.7, 1.3, 100.0)


def nine(ckpt):
  from epos_amd import decoder_train
  return {n: np.asarray(ckpt[n]) for n in decoder_train.VARIABLES}


def on_device(d):
  return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def host(d):
  torch.cuda.synchronize()
  return {k: v.cpu().numpy().copy() for k, v in d.items()}


def build(ckpt, instance=0, batch=NET_B):
  from epos_amd import model
  mo = model.ModelOptions(model.get_outputs_to_num_channels(NET_O, NET_F),
                          crop_size=(NET_W, NET_H))
  return model.get_net(ckpt, batch, NET_H, NET_W, NET_O, NET_F, mo, 'cuda:0', instance=instance)


@pytest.fixture(scope='module')
def images():
  from epos_amd import synthetic
  return np.stack([synthetic.image(i, NET_H, NET_W) for i in range(NET_B)]).astype(np.float32)


def same_bytes(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and \
      a.contiguous().view(torch.uint8).equal(b.contiguous().view(torch.uint8))


# ------------------------------------------------------------- gradients ---
def check_grads(net, ckpt, gt, presplit):
  """net_grads of all nine variables after a forward_logits: byte-equal to its parts called by hand, and the
  layer's three gradients within bound of the restatement on the net's own A bytes and the
  device's own G."""
  from epos_amd import decoder_train as DT, heads_train as HT, loss as L, trainer
  from epos_amd import weights as W
  op = net.pointwise_operand()
  assert op['presplit'] is presplit and (op['a_h2'] is not None) == presplit
  assert (op['k'], op['n'], op['lda']) == (256, 256, 256)
  assert op['m'] == NET_B * net.out_h * net.out_w
  assert (DT.LAYER in net.presplit_layers) == presplit
  variables = on_device(nine(ckpt))
  values, bad, grads = trainer.net_grads(net, gt, variables, tuple(W.TRAINABLE_LAYERS),
                                         LOSS_WEIGHTS, 'pooled')
  assert sorted(grads) == sorted(DT.VARIABLES) and bad.tolist() == [0] * NET_B
  assert tuple(grads[DT.LAYER + '/weights'].shape) == (1, 1, 256, 256)
  # the parts, by hand
  logits = HT.net_logits(net)
  sums, counts, bad2 = L.loss_terms(logits, gt)
  values2, scales = L.loss_values(sums, counts, LOSS_WEIGHTS, 'pooled')
  assert same_bytes(values, values2) and same_bytes(bad, bad2)
  raw = HT.heads_weight_grads(net.decoder_out, logits, gt, scales)
  for head in HT.HEADS:
    wname, bname = HT.variable_names(head)
    assert same_bytes(grads[wname].view(256, -1), raw[head][0]), wname
    assert same_bytes(grads[bname], raw[head][1]), bname
  G = HT.heads_input_grad(logits, gt, scales, variables, relu_of=net.decoder_out)
  mean, var = net.layer_constants()
  w, gamma = variables[DT.LAYER + '/weights'], variables[DT.LAYER + '/BatchNorm/gamma']
  layer = DT.pointwise_weight_grads(op['a'], G, w, bn=(gamma, mean, var), eps=op['eps'],
                                    a_h2=op['a_h2'])
  for short, t in layer.items():
    assert same_bytes(grads[DT.LAYER + '/' + short], t), short
  # the restatement on the bytes of A and G
  M = op['m']
  a_raw = op['a'].cpu().numpy().reshape(M, op['lda'])
  if presplit:
    slot, slot2, gain, bias = op['a_h2']
    words = [None if s is None else s.cpu().numpy().view(np.uint32) for s in (slot, slot2)]
    bound = ref.slot_bound(words[0], words[1], gain, bias)
    assert np.isfinite(bound) and bound > 0
    A64 = ref.h2_values(a_raw, 256, ref.h2_scale(bound)[1])
    assert np.abs(A64).max() <= float(bound)
  else:
    A64 = a_raw.astype(np.float64)
  assert A64.min() >= 0 and A64.max() > 0               # behind the depthwise layer's ReLU
  Gh = G.cpu().numpy()
  assert not Gh[net.decoder_out.cpu().numpy().reshape(M, 256) <= 0].any() and np.abs(Gh).max() > 0
  S, g, aS, ag = ref.sums(A64, Gh)
  Wh, gh = ckpt[DT.LAYER + '/weights'].reshape(256, 256), ckpt[DT.LAYER + '/BatchNorm/gamma']
  mh, vh = mean.cpu().numpy(), var.cpu().numpy()
  assert np.array_equal(mh, ckpt[DT.LAYER + '/BatchNorm/moving_mean'])
  want = ref.close(S, g, Wh, gh, mh, vh, op['eps'])
  tol = ref.bounds_close(M, S, g, aS, ag, Wh, gh, mh, vh, op['eps'])
  for short, wv, t in zip(('weights', 'BatchNorm/gamma', 'BatchNorm/beta'), want, tol):
    got = layer[short].cpu().numpy().reshape(wv.shape)
    ok, worst = ref.within(got, wv, t)
    print('%s (presplit=%s): worst error / bound = %.3g' % (short, presplit, worst))
    assert ok, (short, worst)
    assert np.abs(got).max() > 0
  return host(grads)


def test_net_grads_equal_their_parts_and_the_restatement(small_net, images, monkeypatch):
  net, ckpt, mo, c, gt = small_net
  net.forward_logits(images)
  pairs = check_grads(net, ckpt, gt, presplit=True)
  # the same net with an fp32 A: the switch is read when a plan is built
  monkeypatch.setenv('EPOS_H2_PRESPLIT', '0')
  plain = build(ckpt, instance=7)
  monkeypatch.delenv('EPOS_H2_PRESPLIT')
  plain.forward_logits(images)
  f32 = check_grads(plain, ckpt, gt, presplit=False)
  # both modes compute the same network: the fp16 pairs keep 22 bits of A
  from epos_amd import decoder_train as DT
  for n in DT.LAYER_VARIABLES:
    scale = np.abs(f32[n]).max()
    assert np.abs(pairs[n] - f32[n]).max() <= 1e-3 * scale, n


def test_python_layer_argument_checks(small_net):
  from epos_amd import decoder_train as DT, trainer
  net = small_net[0]
  a = torch.zeros(10, 8, device='cuda')
  g = torch.zeros(10, 4, device='cuda')
  w = torch.zeros(8, 4, device='cuda')
  bn = tuple(torch.ones(4, device='cuda') for _ in range(3))
  out = DT.pointwise_weight_grads(a, g, w, bn=bn)
  assert sorted(out) == ['BatchNorm/beta', 'BatchNorm/gamma', 'weights']
  assert sorted(DT.pointwise_weight_grads(a, g, w)) == ['biases', 'weights']
  for kwargs, exc in ((dict(a=a.double()), TypeError), (dict(g=g[:9]), ValueError),
                      (dict(weights=w.t()), ValueError), (dict(a=a.cpu()), DT.EposError),
                      (dict(bn=bn[:2]), ValueError), (dict(bn=(bn[0][:3],) + bn[1:]), ValueError),
                      (dict(out={'weights': torch.zeros(3, device='cuda')}), ValueError),
                      (dict(workspace=torch.zeros(3, dtype=torch.int64, device='cuda')),
                       ValueError),
                      (dict(a_h2=(None, None, 1.0, 0.0)), ValueError),
                      (dict(a_h2=(torch.zeros(3, dtype=torch.int32, device='cuda'), None, 1.0,
                                  0.0)), ValueError)):
    args = dict(a=a, g=g, weights=w, bn=bn)
    args.update(kwargs)
    with pytest.raises(exc):
      DT.pointwise_weight_grads(**args)
  with pytest.raises(ValueError, match='not a trainable layer'):
    net.pointwise_operand('decoder/decoder_conv0_pointwise')
  with pytest.raises(ValueError, match='not a variable this optimiser holds'):
    trainer.Optimizer(nine(small_net[1]), 1e-3, trainable=('logits/other/weights',))


# ---------------------------------------------------------- weight update ---
def loss_names():
  from epos_amd import loss
  return loss.HEAD_VARIABLES


def all_runs(n, images):
  return {'logits_eager': host(n.forward_logits(images)),
          'logits_graph': host(n.forward_logits(images, use_graph=True)),
          'forward_graph': host(n.forward(images, use_graph=True))}


def assert_same(got, want, tag):
  for run in want:
    for k in want[run]:
      assert got[run][k].tobytes() == want[run][k].tobytes(), (tag, run, k)


def test_set_weights_of_the_layer_equals_a_freshly_built_net(small_net, images):
  from epos_amd import decoder_train as DT, weights
  from epos_amd._lib import EposError
  a = small_net[1]
  b = weights.random_init('xception_65', num_objs=NET_O, num_frags=NET_F, seed=6,
                          randomize_bn=True)
  ab = dict(a)
  ab.update(nine(b))                          # the nine variables of b, the statistics of a
  upd = build(a, instance=1)
  upd.forward_logits(images, use_graph=True)
  upd.forward(images, use_graph=True)         # both graphs captured before any update
  graphs = (upd._graph, upd._graph_logits)
  assert None not in graphs
  want_a = all_runs(small_net[0], images)     # built from a and never updated so far
  want_ab = all_runs(build(ab, instance=3), images)
  assert_same(all_runs(upd, images), want_a, 'before')
  # all nine, tensors on the device: one grouped pack call
  status = upd.set_weights(on_device(nine(ab)))
  assert status.dtype == torch.int32 and status.tolist() == [0] * (3 + 2 * NET_O + 1)
  assert_same(all_runs(upd, images), want_ab, 'nine')
  assert (upd._graph, upd._graph_logits) == graphs
  # back to a, then the layer alone, numpy arrays with [K, N] weights
  upd.set_weights(nine(a))
  assert_same(all_runs(upd, images), want_a, 'back')
  lay = {n: np.asarray(b[n]) for n in DT.LAYER_VARIABLES}
  lay[DT.LAYER + '/weights'] = lay[DT.LAYER + '/weights'].reshape(256, 256)
  assert upd.set_weights(lay).tolist() == [0]
  want_layer = all_runs(upd, images)          # the layer of b under the logits layers of a
  for run in want_layer:
    for k in ('pred_obj_conf', 'pred_frag_conf', 'pred_frag_loc'):
      assert want_layer[run][k].tobytes() != want_a[run][k].tobytes(), (run, k)
      assert want_layer[run][k].tobytes() != want_ab[run][k].tobytes(), (run, k)
  # ... and the logits layers of b on top of it, in a call of their own: all nine of b
  upd.set_weights({n: b[n] for n in loss_names()})
  assert_same(all_runs(upd, images), want_ab, 'layer, then heads')
  upd.set_weights({n: a[n] for n in loss_names()})
  assert_same(all_runs(upd, images), want_layer, 'layer')
  # a refused update leaves everything as it was: the layer and the logits layers together
  bad = nine(a)
  w = bad[DT.LAYER + '/weights'].copy()
  w[0, 0, 17, 100] = np.nan
  bad[DT.LAYER + '/weights'] = w
  with pytest.raises(EposError,
                     match=r'set_weights.*refused %s.*previous weights' % DT.LAYER):
    upd.set_weights(bad)
  assert_same(all_runs(upd, images), want_layer, 'refused')
  status = upd.set_weights(bad, check=False)
  assert torch.nonzero(status).flatten().tolist() == [3 + 2 * NET_O]
  assert_same(all_runs(upd, images), want_layer, 'refused, unchecked')
  # argument checks: before anything is enqueued
  good = on_device(nine(a))
  name = DT.LAYER + '/BatchNorm/gamma'
  for variables, exc in ((dict(good, **{name: good[name].double()}), TypeError),
                         (dict(good, **{name: good[name].cpu()}), ValueError),
                         (dict(good, **{name: good[name][:3]}), ValueError),
                         ({name: good[name]}, ValueError),
                         (dict(good, **{'decoder/other/weights': good[name]}), ValueError)):
    with pytest.raises(exc):
      upd.set_weights(variables)
  assert_same(all_runs(upd, images), want_layer, 'after the argument checks')
  assert upd.set_weights({}).numel() == 0


# -------------------------------------------------------------- train step ---
def test_train_step_with_the_layer_equals_its_parts(small_net, images):
  from epos_amd import decoder_train as DT, loss, trainer
  from epos_amd import weights as W
  a = small_net[1]
  lr, kw = 1e-3, dict(momentum=0.9, weight_decay=4e-5, last_layer_gradient_multiplier=3.0,
                      trainable=DT.VARIABLES)
  c = loss_cases.make_case(NET_B, small_net[0].out_h * small_net[0].out_w, NET_O, NET_F, seed=41)
  gt = gt_tensors(c, small_net[0].out_h, small_net[0].out_w)
  # by hand, on one net (the plan of the update test, put back to a)
  hand, ref_opt = build(a, instance=1), trainer.Optimizer(a, lr=lr, **kw)
  hand.set_weights(nine(a))
  ref_values = []
  for _ in range(2):
    hand.forward_logits(images)
    values, bad, grads = trainer.net_grads(hand, gt, ref_opt.params, ref_opt.layers)
    ref_values.append(values.cpu().numpy().copy())
    ref_opt.step(grads, lr)
    assert hand.set_weights(ref_opt.params).tolist() == [0] * (3 + 2 * NET_O + 1)
  ref_state = ref_opt.state()
  hand.set_weights(nine(a))             # the cached plan as it was built
  # two train steps on another
  trainee, opt = small_net[0], trainer.Optimizer(a, lr=lr, **kw)
  got_values = []
  for _ in range(2):
    values, bad, status = trainer.train_step(trainee, images, gt, opt, lr)
    got_values.append(values.cpu().numpy().copy())
    assert bad.tolist() == [0] * NET_B and status.tolist() == [0] * (3 + 2 * NET_O + 1)
  for step in range(2):
    assert got_values[step].tobytes() == ref_values[step].tobytes(), step
  assert np.isfinite(got_values).all() and got_values[1][3] != got_values[0][3]
  state = opt.state()
  assert sorted(state) == sorted(ref_state) and len(state) == 18
  for k in ref_state:
    assert state[k].tobytes() == ref_state[k].tobytes(), k
  for n in DT.VARIABLES:                      # every variable moved
    assert state[n].tobytes() != np.asarray(a[n], np.float32).tobytes(), n
  # the update follows the rule: one momentum step by hand on gamma, from the first gradients
  from tests.helpers import heads_wgrad_ref
  name = DT.LAYER + '/BatchNorm/gamma'
  check_opt = trainer.Optimizer(a, lr=lr, **kw)
  hand.forward_logits(images)
  _, _, grads = trainer.net_grads(hand, gt, check_opt.params, tuple(W.TRAINABLE_LAYERS))
  g0 = grads[name].cpu().numpy()
  w1, a1 = heads_wgrad_ref.momentum_step(a[name], np.zeros(256, np.float32), g0, lr, 0.9, 0.0, 3.0)
  check_opt.step(grads, lr)
  assert check_opt.params[name].cpu().numpy().tobytes() == w1.tobytes()
  assert check_opt.accums[name].cpu().numpy().tobytes() == a1.tobytes()
  # resuming: an optimiser restored from the state continues with the same bytes
  resumed = trainer.Optimizer(state, lr=lr, **kw)
  for k in state:
    t = resumed.accums[k[:-9]] if k.endswith('/Momentum') else resumed.params[k]
    assert t.cpu().numpy().tobytes() == state[k].tobytes(), k
  # gamma and beta frozen: their bytes stay, they have no accumulator, the weights move
  frozen = trainer.Optimizer(a, lr=lr, **dict(
      kw, trainable=loss.HEAD_VARIABLES + (DT.LAYER + '/weights',)))
  trainee.set_weights(nine(a))
  trainer.train_step(trainee, images, gt, frozen, lr)
  st = frozen.state()
  assert len(st) == 9 + 7
  for short in ('BatchNorm/gamma', 'BatchNorm/beta'):
    n = DT.LAYER + '/' + short
    assert st[n].tobytes() == np.asarray(a[n], np.float32).tobytes() and n + '/Momentum' not in st
  n = DT.LAYER + '/weights'
  assert st[n].tobytes() != np.asarray(a[n], np.float32).tobytes() and n + '/Momentum' in st
  trainee.set_weights(nine(a))


def test_logits_only_step_leaves_the_layer_alone(small_net, images, monkeypatch):
  from epos_amd import decoder_train as DT, heads_train as HT, loss, trainer
  net, a, _, _, gt = small_net
  net.set_weights(nine(a))
  calls = {'pointwise_weight_grads': 0, 'heads_input_grad': 0}

  def count(module, name):
    real = getattr(module, name)

    def counted(*args, **kwargs):
      calls[name] += 1
      return real(*args, **kwargs)
    monkeypatch.setattr(module, name, counted)
  count(DT, 'pointwise_weight_grads')
  count(HT, 'heads_input_grad')
  packs = net.pointwise_operand()['packs']
  assert len(packs) == 4 and None not in packs
  torch.cuda.synchronize()
  before = [t.clone() for t in packs]
  opt = trainer.Optimizer(a, lr=1e-3)
  values, bad, status = trainer.train_step(net, images, gt, opt, 1e-3)
  assert calls == {'pointwise_weight_grads': 0, 'heads_input_grad': 0}
  assert status.tolist() == [0] * (3 + 2 * NET_O) and bad.tolist() == [0] * NET_B
  for t, was in zip(packs, before):
    assert same_bytes(t, was)
  state = opt.state()
  assert sorted(state) == sorted(loss.HEAD_VARIABLES +
                                 tuple(n + '/Momentum' for n in loss.HEAD_VARIABLES))
  assert len(state) == 12
  for n in loss.HEAD_VARIABLES:                # the step itself was a step
    assert state[n].tobytes() != np.asarray(a[n], np.float32).tobytes(), n
  # the counters do count: the same step with the layer trained calls each once
  net.set_weights(nine(a))
  trainer.train_step(net, images, gt, trainer.Optimizer(a, lr=1e-3, trainable=DT.VARIABLES), 1e-3)
  assert calls == {'pointwise_weight_grads': 1, 'heads_input_grad': 1}
  net.set_weights(nine(a))


def test_one_method_same_words(small_net, images):
  from epos_amd import decoder_train as DT, weights
  a = small_net[1]
  b = weights.random_init('xception_65', num_objs=NET_O, num_frags=NET_F, seed=6,
                          randomize_bn=True)
  upd = build(a, instance=1)                  # the plan of the update test
  upd.set_weights(nine(a))
  want_a = all_runs(upd, images)
  # the logits layers of b, then the layer of b ...
  logits_status = upd.set_weights({n: b[n] for n in loss_names()})
  layer_status = upd.set_weights({n: b[n] for n in DT.LAYER_VARIABLES})
  in_two = all_runs(upd, images)
  for run in in_two:
    for k in ('pred_obj_conf', 'pred_frag_conf', 'pred_frag_loc'):
      assert in_two[run][k].tobytes() != want_a[run][k].tobytes(), (run, k)
  # ... and all nine in one call, from a again
  upd.set_weights(nine(a))
  assert_same(all_runs(upd, images), want_a, 'back')
  all_status = upd.set_weights(nine(b))
  assert_same(all_runs(upd, images), in_two, 'one call')
  for status, words in ((logits_status, 3 + 2 * NET_O), (layer_status, 1),
                        (all_status, 3 + 2 * NET_O + 1)):
    assert status.dtype == torch.int32 and status.tolist() == [0] * words
  upd.set_weights(nine(a))


# ------------------------------------------------------------ command line ---
H, W, O, F = 96, 128, 3, 64
UNFREEZE = '^(?!logits|decoder/decoder_conv1_pointwise)'


def _rot(axis, angle):
  axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
  a, b, c = axis
  S = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]])
  return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def _run(model_root, bop, fdir, *extra):
  # the 'step' policy: the rate of a step does not depend on --train_steps
  return subprocess.run(
      ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'train_heads.py'),
       '--model=toy', '--synthetic', '2', '--frames', str(fdir), '--dataset', 'lm',
       '--num_objs', str(O), '--learning_policy', 'step'] + list(extra),
      env=dict(os.environ, TF_MODELS_PATH=str(model_root), BOP_PATH=str(bop)),
      capture_output=True, text=True)


def test_train_heads_cli_with_the_layer_unfrozen(tmp_path, gpu_children):
  from epos_amd import cli, decoder_train as DT, eval_utils, frames as eframes, loss, model
  from epos_amd import ply, render, synthetic, tf_checkpoint, trainer, weights
  store = synthetic.ModelStore(O, F, seed=0)           # the store --synthetic builds
  bop = tmp_path / 'bop'
  (bop / 'lm' / 'models_eval').mkdir(parents=True)
  for o in store.dp_model['obj_ids']:
    v, f = mesh_cases.icosphere(1, 1.0, scale=store.radii[o])
    ply.save_ply(ply.model_path(str(bop), 'lm', o, 'eval'), v, f)
  fdir = tmp_path / 'frames'
  fdir.mkdir()
  K = np.array([[150.0, 0.0, 64.0], [0.0, 150.0, 48.0], [0.0, 0.0, 1.0]])
  poses = [[{'obj_id': 1, 'R': np.eye(3), 't': [0.0, 0.0, 500.0]},
            {'obj_id': 2, 'R': _rot([0, 1, 0], 0.5), 't': [60.0, 20.0, 600.0]}],
           [{'obj_id': 3, 'R': _rot([1, 0, 0], 0.3), 't': [-60.0, 10.0, 450.0]},
            {'obj_id': 1, 'R': _rot([0, 0, 1], 1.1), 't': [60.0, -10.0, 550.0]}]]
  images, meta = [], []
  for i, gt in enumerate(poses):
    images.append(synthetic.image(i, H, W).astype(np.uint8))
    np.save(str(fdir / ('%d.npy' % i)), images[-1])
    meta.append({'path': '%d.npy' % i, 'im_id': i + 1, 'scene_id': 1, 'K': K.tolist(),
                 'targets': {str(p['obj_id']): 1 for p in gt},
                 'gt_poses': [{'obj_id': p['obj_id'], 'R': np.asarray(p['R']).tolist(),
                               't': p['t']} for p in gt]})
  (fdir / 'frames.json').write_text(json.dumps(meta))
  for root in ('whole', 'resumed', 'default'):
    (tmp_path / root / 'toy').mkdir(parents=True)
    (tmp_path / root / 'toy' / 'params.yml').write_text('train_crop_size: "%d,%d"\n' % (W, H))
  flags = ['--freeze_regex_list', UNFREEZE, '--last_layer_gradient_multiplier', '2']

  def ckpt_of(root, step):
    return tf_checkpoint.load_checkpoint(
        str(tmp_path / root / 'toy' / 'train' / ('model.ckpt-%d' % step)))

  # three steps with the layer unfrozen, in one run and stopped after the first
  out = _run(tmp_path / 'whole', bop, fdir, '--train_steps', '3', '--log_steps', '1', *flags)
  assert out.returncode == 0, out.stdout + out.stderr
  assert 'Training below the logits: ' + ', '.join(DT.LAYER_VARIABLES) in out.stdout
  whole = ckpt_of('whole', 3)
  out = _run(tmp_path / 'resumed', bop, fdir, '--train_steps', '1', *flags)
  assert out.returncode == 0, out.stdout + out.stderr
  out = _run(tmp_path / 'resumed', bop, fdir, '--train_steps', '3', *flags)
  assert out.returncode == 0, out.stdout + out.stderr
  assert 'from step 1' in out.stdout
  resumed = ckpt_of('resumed', 3)
  # the default invocation, one step
  out = _run(tmp_path / 'default', bop, fdir, '--train_steps', '1')
  assert out.returncode == 0, out.stdout + out.stderr
  assert 'Training below the logits' not in out.stdout
  default = ckpt_of('default', 1)

  # the same steps here
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), crop_size=(W, H))
  ren = render.Renderer('cuda:0')
  for o, m in sorted(ply.load_models(str(bop), 'lm', 'eval', obj_ids=[1, 2, 3]).items()):
    ren.add_model(o, m)
  frag_pool = render.pool_fragments(store.frag_centers, store.frag_sizes, O)
  frames = eframes.frames_from_dir(str(fdir), meta, H, W)

  def steps(n, opt, instance, status_words):
    net = model.get_net(ckpt, 1, H, W, O, F, mo, 'cuda:0', instance=instance)
    for s in range(n):
      gt = eval_utils.gt_loss_fields_device(ren, frames[s % 2], (W // 4, H // 4), frag_pool,
                                            'lm', input_size=(W, H))
      lr = trainer.learning_rate(s, policy='step')
      values, bad, status = trainer.train_step(net, torch.from_numpy(images[s % 2][None]),
                                               {k: gt[k][None] for k in loss.GT_KEYS}, opt, lr)
      assert bad.tolist() == [0] and status.tolist() == [0] * status_words
    return opt.state()

  state = steps(3, trainer.Optimizer(ckpt, 1e-4, momentum=0.9, weight_decay=4e-5,
                                     last_layer_gradient_multiplier=2.0, trainable=DT.VARIABLES),
                0, 3 + 2 * O + 1)
  assert len(state) == 18 and int(whole['global_step']) == 3 and int(resumed['global_step']) == 3
  assert sorted(whole) == sorted(resumed) == sorted(
      list(ckpt) + [n + '/Momentum' for n in DT.VARIABLES] + ['global_step'])
  for name, want in state.items():
    assert whole[name].dtype == np.float32 and whole[name].shape == want.shape, name
    assert whole[name].tobytes() == want.tobytes(), name
  for name in whole:
    assert whole[name].tobytes() == resumed[name].tobytes(), name
  for name in ckpt:
    moved = whole[name].tobytes() != np.asarray(ckpt[name]).tobytes()
    assert moved == (name in DT.VARIABLES), name       # the statistics and all else stay
  # the default: the logits layers only, the bytes the default Optimizer's train_step gives
  plain = steps(1, trainer.Optimizer(ckpt, 1e-4, momentum=0.9, weight_decay=4e-5), 1, 3 + 2 * O)
  assert len(plain) == 12
  assert sorted(default) == sorted(list(ckpt) + [n + '/Momentum' for n in loss.HEAD_VARIABLES] +
                                   ['global_step'])
  for name, want in plain.items():
    assert default[name].tobytes() == want.tobytes(), name
  for name in ckpt:
    if name not in plain:
      assert default[name].tobytes() == np.asarray(ckpt[name]).tobytes(), name

  # what infer.py would load from the folder: the step-3 weights, the layer's included
  class Args(object):
    checkpoint_name, synthetic, num_objs, num_frags, model_variant = None, 0, None, F, 'xception_65'
  loaded, num_objs, path = cli.load_checkpoint(Args, str(tmp_path / 'whole' / 'toy' / 'train'))
  assert num_objs == O and sorted(loaded) == sorted(ckpt)
  for name in DT.VARIABLES:
    assert loaded[name].tobytes() == state[name].tobytes(), name
  torch.cuda.synchronize()
  model._NETS.clear()
