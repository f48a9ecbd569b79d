"""gt_knn_frags > 1 through Python, on a 64 x 64 net with 2 objects x 4 fragments: the ground
truth of render.gt_fields_device, train_step against its parts, differentiable_losses' backward
against loss_grads, and eval_loss.py / train_heads.py with --gt_knn_frags on two frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import knn_ref, mesh_cases      # noqa: E402

pytestmark = pytest.mark.gpu

H, W, O, F, KNN = 64, 64, 2, 4, 2
WEIGHTS = (0.7, 1.3, 100.0)


def same_bytes(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and \
      a.contiguous().view(torch.uint8).equal(b.contiguous().view(torch.uint8))


def build(ckpt, batch, instance=0):
  from epos_amd import model
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), crop_size=(W, H))
  return model.get_net(ckpt, batch, H, W, O, F, mo, 'cuda:0', instance=instance)


@pytest.fixture(scope='module')
def setup():
  """(checkpoint, images u8 [2,64,64,3], host case, gt with two fragments per pixel on the
  16 x 16 heads)."""
  from epos_amd import model, synthetic, weights
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=3, randomize_bn=True)
  images = np.stack([synthetic.image(i, H, W) for i in range(2)]).astype(np.uint8)
  h, w = H // 4, W // 4
  c = knn_ref.make_case(2, h * w, O, F, KNN, seed=21)
  gt = {'obj_label': torch.from_numpy(c['gt_obj']).cuda().view(2, h, w),
        'frag_label': torch.from_numpy(c['gt_frag']).cuda().view(2, h, w, KNN),
        'frag_loc': torch.from_numpy(c['gt_loc']).cuda().view(2, h, w, KNN, 3),
        'frag_weight': torch.from_numpy(c['gt_weight']).cuda().view(2, h, w, KNN)}
  yield ckpt, images, c, gt
  model._NETS.clear()


def test_gt_fields_device_shapes_and_generator():
  from epos_amd import render
  from epos_amd._lib import EposError
  rng = np.random.RandomState(0)
  depth = torch.ones((1, 5, 7), device='cuda')
  lp = torch.from_numpy(rng.uniform(-50, 50, (1, 5, 7, 3)).astype(np.float32)).cuda()
  centers, sizes = rng.uniform(-50, 50, (1, F, 3)), rng.uniform(5, 40, (1, F))
  one = render.gt_fields_device(depth, lp, [1], centers, sizes)
  assert tuple(one['frag_label'].shape) == (5, 7) and tuple(one['frag_loc'].shape) == (5, 7, 3)
  for k in (2, 4):
    f = render.gt_fields_device(depth, lp, [1], centers, sizes, knn_frags=k)
    assert tuple(f['frag_label'].shape) == (5, 7, k)
    assert tuple(f['frag_loc'].shape) == (5, 7, k, 3)
    assert tuple(f['frag_weight'].shape) == (5, 7, k)
    exp = knn_ref.gt_fields(np.ones((1, 5, 7), np.float32), lp.cpu().numpy(), None, [1], centers,
                            sizes, k)
    for key in ('frag_label', 'frag_loc', 'frag_weight', 'obj_label'):
      assert f[key].cpu().numpy().tobytes() == exp[key].tobytes(), key
    assert same_bytes(f['frag_label'][..., 0].contiguous(), one['frag_label'])
  for k in (0, 5, 1.5):
    with pytest.raises(ValueError, match='knn_frags must be in 1..4'):
      render.gt_fields_device(depth, lp, [1], centers, sizes, knn_frags=k)
  gen = render.FragmentFieldGenerator({1: centers[0]}, {1: sizes[0]}, None, knn_frags=2)
  assert gen.knn_frags == 2
  with pytest.raises(EposError, match='knn_frags must be in 1..4'):
    render.FragmentFieldGenerator({1: centers[0]}, {1: sizes[0]}, None, knn_frags=5)


def test_batch_reads_knn_from_the_shapes(setup):
  from epos_amd import loss
  ckpt, images, c, gt = setup
  h, w = H // 4, W // 4
  logits = {'pred_obj_conf': torch.zeros(2, h, w, O + 1, device='cuda'),
            'pred_frag_conf': torch.zeros(2, h, w, O, F, device='cuda'),
            'pred_frag_loc': torch.zeros(2, h, w, O, F, 3, device='cuda')}
  assert loss.Batch(logits, gt, 'x').knn == KNN
  for key, shape in (('frag_loc', (2, h, w, 3)), ('frag_weight', (2, h, w))):
    wrong = dict(gt)
    wrong[key] = torch.zeros(shape, device='cuda')
    with pytest.raises(ValueError, match='frag_loc must be'):
      loss.Batch(logits, wrong, 'x')
  five = dict(gt)
  five['frag_label'] = torch.zeros((2, h, w, 5), dtype=torch.int32, device='cuda')
  with pytest.raises(ValueError, match='gt_knn_frags must be in 1..4'):
    loss.Batch(logits, five, 'x')
  ev = loss.LossEval(O, F, 'cuda:0')
  with pytest.raises(ValueError, match='2 fragment\\(s\\) per pixel, expected 1'):
    ev.update(logits, gt)


def test_train_step_equals_its_parts(setup):
  from epos_amd import heads_train as HT, loss as L, trainer
  ckpt, images, c, gt = setup
  net, twin = build(ckpt, 2), build(ckpt, 2, instance=1)
  opt = trainer.Optimizer(ckpt, 1e-3, momentum=0.9, weight_decay=4e-5)
  opt2 = trainer.Optimizer(ckpt, 1e-3, momentum=0.9, weight_decay=4e-5)
  imgs = torch.from_numpy(images)
  values, bad, status = trainer.train_step(net, imgs, gt, opt, 1e-3, WEIGHTS)
  assert bad.tolist() == [0, 0] and not status.any()
  # the parts, by hand, on a twin net
  twin.forward_logits(imgs, use_graph=True)
  logits = HT.net_logits(twin)
  sums, counts, bad2 = L.loss_terms(logits, gt)
  values2, scales = L.loss_values(sums, counts, WEIGHTS, 'pooled', knn=KNN)
  assert same_bytes(values, values2) and same_bytes(bad, bad2)
  raw = HT.heads_weight_grads(twin.decoder_out, logits, gt, scales)
  v3, b3, grads = trainer.net_grads(twin, gt, opt2.params, opt2.layers, WEIGHTS, 'pooled')
  assert same_bytes(values, v3)
  for head in HT.HEADS:
    wname, bname = HT.variable_names(head)
    assert same_bytes(grads[wname].view(raw[head][0].shape), raw[head][0]), wname
    assert same_bytes(grads[bname], raw[head][1]), bname
  opt2.step(grads, 1e-3)
  for name in opt.params:
    assert same_bytes(opt.params[name], opt2.params[name]), name
  # the tables and the values are those of the restatement's rules, not of one slot
  torch.cuda.synchronize()
  h_sums, h_counts = sums.cpu().numpy(), counts.cpu().numpy()
  want = L.summarize(h_sums, h_counts, bad2.cpu().numpy(), WEIGHTS, O, knn=KNN)['pooled']
  assert values.cpu().tolist() == [want[n] for n in L.NAMES]
  one = L.summarize(h_sums, h_counts, bad2.cpu().numpy(), WEIGHTS, O)['pooled']
  assert one['frag_cls_loss'] == 2 * want['frag_cls_loss']
  # the input gradient follows: net_feature_grad equals its parts
  v4, b4, dX = HT.net_feature_grad(twin, gt, ckpt, WEIGHTS, 'pooled', relu=True)
  G = HT.heads_input_grad(logits, gt, scales, ckpt, relu_of=twin.decoder_out)
  assert same_bytes(dX, G) and same_bytes(v4, values)


def test_differentiable_losses_backward_gives_loss_grads(setup):
  from epos_amd import loss as L
  ckpt, images, c, gt = setup
  logits = {k: torch.from_numpy(c[n]).cuda().view(s).requires_grad_(True) for k, n, s in (
      ('pred_obj_conf', 'obj_logits', (2, 16, 16, O + 1)),
      ('pred_frag_conf', 'frag_logits', (2, 16, 16, O, F)),
      ('pred_frag_loc', 'frag_loc', (2, 16, 16, O, F, 3)))}
  values, bad = L.differentiable_losses(logits, gt, WEIGHTS, 'mean')
  up = torch.tensor([0.3, -1.0, 2.0, 0.5], dtype=torch.float64, device='cuda')
  (values * up).sum().backward()
  plain = {k: v.detach() for k, v in logits.items()}
  sums, counts, _ = L.loss_terms(plain, gt)
  v2, scales = L.loss_values(sums, counts, WEIGHTS, 'mean', knn=KNN)
  assert same_bytes(values.detach(), v2) and bad.tolist() == [0, 0]
  d = L.loss_grads(plain, gt, scales, upstream=up)
  for k, g in zip(L.HEADS, d):
    assert same_bytes(logits[k].grad, g), k
  torch.cuda.synchronize()
  exp = knn_ref.grads(c, scales.cpu().numpy(), up.cpu().numpy())
  assert d[2].cpu().numpy().tobytes() == exp[2].reshape(d[2].shape).tobytes()
  assert np.abs(d[1].cpu().numpy()).max() > 0


# ------------------------------------------------------------------ the scripts ---
def _rot(axis, angle):
  axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
  a, b, c = axis
  S = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]])
  return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def _frames(tmp_path):
  """Two frames with ground-truth poses, the meshes of the store --synthetic builds."""
  from epos_amd import ply, synthetic
  store = synthetic.ModelStore(O, F, seed=0)
  bop = tmp_path / 'bop'
  (bop / 'lm' / 'models_eval').mkdir(parents=True)
  for o in store.dp_model['obj_ids']:
    v, f = mesh_cases.icosphere(1, 1.0, scale=store.radii[o])
    ply.save_ply(ply.model_path(str(bop), 'lm', o, 'eval'), v, f)
  fdir = tmp_path / 'frames'
  fdir.mkdir()
  K = np.array([[150.0, 0.0, 32.0], [0.0, 150.0, 32.0], [0.0, 0.0, 1.0]])
  poses = [[{'obj_id': 1, 'R': np.eye(3), 't': [0.0, 0.0, 500.0]},
            {'obj_id': 2, 'R': _rot([0, 1, 0], 0.5), 't': [40.0, 20.0, 600.0]}],
           [{'obj_id': 2, 'R': _rot([1, 0, 0], 0.3), 't': [-40.0, 10.0, 450.0]},
            {'obj_id': 1, 'R': _rot([0, 0, 1], 1.1), 't': [40.0, -10.0, 550.0]}]]
  meta = []
  for i, gt in enumerate(poses):
    np.save(str(fdir / ('%d.npy' % i)), synthetic.image(i, H, W).astype(np.uint8))
    meta.append({'path': '%d.npy' % i, 'im_id': i + 1, 'scene_id': 1, 'K': K.tolist(),
                 'targets': {str(p['obj_id']): 1 for p in gt},
                 'gt_poses': [{'obj_id': p['obj_id'], 'R': np.asarray(p['R']).tolist(),
                               't': p['t']} for p in gt]})
  (fdir / 'frames.json').write_text(json.dumps(meta))
  return bop, fdir


def _run(script, root, bop, fdir, *extra, params=''):
  (root / 'toy').mkdir(parents=True, exist_ok=True)
  (root / 'toy' / 'params.yml').write_text(
      'eval_crop_size: "%d,%d"\ntrain_crop_size: "%d,%d"\n' % (W, H, W, H) + params)
  out = subprocess.run(
      ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, script), '--model=toy',
       '--synthetic', '2', '--frames', str(fdir), '--dataset', 'lm', '--num_objs', str(O),
       '--num_frags', str(F)] + list(extra),
      env=dict(os.environ, TF_MODELS_PATH=str(root), BOP_PATH=str(bop)),
      capture_output=True, text=True)
  assert out.returncode == 0, out.stdout + out.stderr
  return out


def test_eval_loss_cli_with_gt_knn_frags(tmp_path, gpu_children):
  bop, fdir = _frames(tmp_path)
  docs = {}
  for name, extra in (('none', ()), ('one', ('--gt_knn_frags', '1')),
                      ('two', ('--gt_knn_frags', '2'))):
    _run('eval_loss.py', tmp_path / name, bop, fdir, *extra)
    docs[name] = (tmp_path / name / 'toy' / 'eval_loss' / 'losses_0.json').read_bytes()
  assert docs['none'] == docs['one']                       # the default: the same bytes
  one, two = json.loads(docs['one']), json.loads(docs['two'])
  assert 'gt_knn_frags' not in one and two['gt_knn_frags'] == 2
  assert two['mean']['obj_cls_loss'] == one['mean']['obj_cls_loss']
  assert two['per_object']['1']['pixels'] == one['per_object']['1']['pixels'] > 0
  assert two['mean']['frag_loc_loss'] > 0 and one['mean']['frag_loc_loss'] > 0
  assert two['mean']['frag_loc_loss'] != one['mean']['frag_loc_loss']
  assert two['mean']['frag_cls_loss'] != one['mean']['frag_cls_loss']
  # a training params.yml supplies the flag
  root = tmp_path / 'yml'
  _run('eval_loss.py', root, bop, fdir, params='gt_knn_frags: 2\n')
  assert (root / 'toy' / 'eval_loss' / 'losses_0.json').read_bytes() == docs['two']


def test_train_heads_cli_with_gt_knn_frags(tmp_path, gpu_children):
  from epos_amd import tf_checkpoint
  bop, fdir = _frames(tmp_path)
  # a rate that does not depend on --train_steps, so that a resumed run is an uninterrupted one
  common = ('--learning_policy', 'step', '--base_learning_rate', '0.001')

  def ckpt(name, step):
    return tf_checkpoint.load_checkpoint(
        str(tmp_path / name / 'toy' / 'train' / ('model.ckpt-%d' % step)))

  def same(a, b):
    return sorted(a) == sorted(b) and all(
        np.asarray(a[n]).tobytes() == np.asarray(b[n]).tobytes() for n in a)
  _run('train_heads.py', tmp_path / 'whole', bop, fdir, '--gt_knn_frags', '2', '--train_steps',
       '4', *common)
  _run('train_heads.py', tmp_path / 'parts', bop, fdir, '--gt_knn_frags', '2', '--train_steps',
       '2', *common)
  out = _run('train_heads.py', tmp_path / 'parts', bop, fdir, '--gt_knn_frags', '2',
             '--train_steps', '4', *common)
  assert 'from step 2' in out.stdout
  whole = ckpt('whole', 4)
  assert same(whole, ckpt('parts', 4))
  # the default: the same bytes as without the flag, and not those of two fragments
  _run('train_heads.py', tmp_path / 'none', bop, fdir, '--train_steps', '2', *common)
  _run('train_heads.py', tmp_path / 'one', bop, fdir, '--gt_knn_frags', '1', '--train_steps', '2',
       *common)
  assert same(ckpt('none', 2), ckpt('one', 2))
  for name in ('model.ckpt-2.index', 'model.ckpt-2.data-00000-of-00001', 'checkpoint'):
    assert (tmp_path / 'none' / 'toy' / 'train' / name).read_bytes() == \
        (tmp_path / 'one' / 'toy' / 'train' / name).read_bytes(), name
  assert not same(ckpt('none', 2), ckpt('parts', 2))
