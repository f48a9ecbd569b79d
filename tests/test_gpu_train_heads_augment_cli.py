"""train_heads.py with data_augmentations in params.yml: a run of four steps, a run of two
resumed to four, four train_steps with an Augmenter here -- the same bytes -- and the same four
steps without augmentation -- other bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import mesh_cases      # noqa: E402

pytestmark = pytest.mark.gpu

H, W, O, F = 96, 128, 3, 64

AUGMENTATIONS = [
    ('random_adjust_brightness', {'min_delta': -0.2, 'max_delta': 0.2}),
    ('random_adjust_contrast', {'min_delta': 0.8, 'max_delta': 1.2}),
    ('random_adjust_saturation', {'min_delta': 0.8, 'max_delta': 1.2}),
    ('random_adjust_hue', {'max_delta': 0.02}),
    ('random_blur', {'max_sigma': 1.5}),
    ('random_gaussian_noise', {'max_sigma': 0.05}),
    ('jpeg_artifacts', {'min_quality': 80})]


def _rot(axis, angle):
  axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
  a, b, c = axis
  S = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]])
  return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def _run(model_root, bop, fdir, *extra):
  # the 'step' policy: the rate of a step does not depend on --train_steps, so a run of two
  # steps resumed to four takes the rates of a run of four
  return subprocess.run(
      ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'train_heads.py'),
       '--model=toy', '--synthetic', '2', '--frames', str(fdir), '--dataset', 'lm',
       '--num_objs', str(O), '--learning_policy', 'step'] + list(extra),
      env=dict(os.environ, TF_MODELS_PATH=str(model_root), BOP_PATH=str(bop)),
      capture_output=True, text=True)


def test_train_heads_cli_with_augmentations(tmp_path, gpu_children):
  from epos_amd import augment, eval_utils, frames as eframes, loss, model, ply
  from epos_amd import render, synthetic, tf_checkpoint, trainer, weights
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
  yml = 'train_crop_size: "%d,%d"\ndata_augmentations:\n' % (W, H) + ''.join(
      '  %s:\n%s' % (name, ''.join('    %s: %r\n' % kv for kv in params.items()))
      for name, params in AUGMENTATIONS)
  for root in ('whole', 'resumed'):
    (tmp_path / root / 'toy').mkdir(parents=True)
    (tmp_path / root / 'toy' / 'params.yml').write_text(yml)

  # one run of four steps
  out = _run(tmp_path / 'whole', bop, fdir, '--train_steps', '4', '--log_steps', '1')
  assert out.returncode == 0, out.stdout + out.stderr
  assert 'Augmentations: ' + ', '.join(n for n, _ in AUGMENTATIONS) in out.stdout
  whole = tf_checkpoint.load_checkpoint(str(tmp_path / 'whole' / 'toy' / 'train' / 'model.ckpt-4'))
  # two steps, then resumed to four, in another folder
  out = _run(tmp_path / 'resumed', bop, fdir, '--train_steps', '2')
  assert out.returncode == 0, out.stdout + out.stderr
  out = _run(tmp_path / 'resumed', bop, fdir, '--train_steps', '4')
  assert out.returncode == 0, out.stdout + out.stderr
  assert 'from step 2' in out.stdout
  resumed = tf_checkpoint.load_checkpoint(
      str(tmp_path / 'resumed' / 'toy' / 'train' / 'model.ckpt-4'))
  assert int(whole['global_step']) == 4 and int(resumed['global_step']) == 4

  # the same four steps here, with and without the augmenter
  def four_steps(augmenter):
    ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0,
                               randomize_bn=True)
    mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), crop_size=(W, H))
    net = model.get_net(ckpt, 1, H, W, O, F, mo, 'cuda:0')
    ren = render.Renderer('cuda:0')
    for o, m in sorted(ply.load_models(str(bop), 'lm', 'eval', obj_ids=[1, 2, 3]).items()):
      ren.add_model(o, m)
    frag_pool = render.pool_fragments(store.frag_centers, store.frag_sizes, O)
    frames = eframes.frames_from_dir(str(fdir), meta, H, W)
    opt = trainer.Optimizer(ckpt, 1e-4, momentum=0.9, weight_decay=4e-5)
    for s in range(4):
      gt = eval_utils.gt_loss_fields_device(ren, frames[s % 2], (W // 4, H // 4), frag_pool,
                                            'lm', input_size=(W, H))
      lr = trainer.learning_rate(s, policy='step')
      values, bad, status = trainer.train_step(
          net, torch.from_numpy(images[s % 2][None]), {k: gt[k][None] for k in loss.GT_KEYS},
          opt, lr, augment=augmenter, step=s)
      assert bad.tolist() == [0] and status.tolist() == [0] * (3 + 2 * O)
    return opt.state()

  spec = dict(AUGMENTATIONS)
  assert [n for n, _ in augment.parse(spec)] == [n for n, _ in AUGMENTATIONS]
  state = four_steps(augment.Augmenter(spec, seed=0, device='cuda:0'))
  plain = four_steps(None)
  assert len(state) == 12
  for name, ref in state.items():
    assert whole[name].dtype == np.float32 and whole[name].shape == ref.shape, name
    assert whole[name].tobytes() == resumed[name].tobytes(), name
    assert whole[name].tobytes() == ref.tobytes(), name
    assert plain[name].tobytes() != ref.tobytes(), name
  torch.cuda.synchronize()
