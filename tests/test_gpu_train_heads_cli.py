"""train_heads.py end to end on two frames with ground-truth poses: the checkpoints, the state
file and the event file it writes, resuming, and its weights against four train_steps run here."""
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


def _rot(axis, angle):
  axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
  a, b, c = axis
  S = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]])
  return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def _run(model_root, bop, fdir, *extra):
  return subprocess.run(
      ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'train_heads.py'),
       '--model=toy', '--synthetic', '2', '--frames', str(fdir), '--dataset', 'lm',
       '--num_objs', str(O)] + list(extra),
      env=dict(os.environ, TF_MODELS_PATH=str(model_root), BOP_PATH=str(bop)),
      capture_output=True, text=True)


def test_train_heads_cli(tmp_path, gpu_children):
  from epos_amd import cli, eval_utils, frames as eframes, loss, model, ply, render
  from epos_amd import synthetic, tf_checkpoint, tf_events, trainer, weights
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
  (tmp_path / 'toy').mkdir()
  (tmp_path / 'toy' / 'params.yml').write_text('train_crop_size: "%d,%d"\n' % (W, H))
  tdir = tmp_path / 'toy' / 'train'

  # run 1: two steps, one checkpoint, the state file, one event file
  out = _run(tmp_path, bop, fdir, '--train_steps', '2', '--save_interval_steps', '2',
             '--log_steps', '1')
  assert out.returncode == 0, out.stdout + out.stderr
  events = [p for p in tdir.iterdir() if p.name.startswith('events.out.tfevents.')]
  assert sorted(p.name for p in tdir.iterdir() if p not in events) == [
      'checkpoint', 'model.ckpt-2.data-00000-of-00001', 'model.ckpt-2.index']
  assert len(events) == 1
  assert tf_checkpoint.latest_checkpoint(str(tdir)) == str(tdir / 'model.ckpt-2')
  two = tf_checkpoint.load_checkpoint(str(tdir / 'model.ckpt-2'))
  assert two['global_step'].dtype == np.int64 and int(two['global_step']) == 2
  recs = tf_events.read_events(str(events[0]))
  assert [r['step'] for r in recs] == [0, 1, 2] and recs[0]['file_version']
  tags = ['train/obj_cls_loss', 'train/frag_cls_loss', 'train/frag_loc_loss', 'train/total_loss']
  for r in recs[1:]:
    assert [t for t, _ in r['scalars']] == tags
    assert all(np.isfinite(v) and v > 0 for _, v in r['scalars'])
  lines = [ln for ln in out.stdout.split('\n') if ln.startswith('step ')]
  assert len(lines) == 2 and lines[1].startswith('step 2: lr=')

  # run 2 on the same folder resumes at step 2
  out = _run(tmp_path, bop, fdir, '--train_steps', '4')
  assert out.returncode == 0, out.stdout + out.stderr
  assert 'from step 2' in out.stdout
  assert (tdir / 'model.ckpt-4.index').exists() and (tdir / 'model.ckpt-2.index').exists()
  four = tf_checkpoint.load_checkpoint(str(tdir / 'model.ckpt-4'))
  assert int(four['global_step']) == 4

  # the same four steps here: the net --synthetic builds, the schedule of each run
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), crop_size=(W, H))
  net = model.get_net(ckpt, 1, H, W, O, F, mo, 'cuda:0')
  ren = render.Renderer('cuda:0')
  for o, m in sorted(ply.load_models(str(bop), 'lm', 'eval', obj_ids=[1, 2, 3]).items()):
    ren.add_model(o, m)
  frag_pool = render.pool_fragments(store.frag_centers, store.frag_sizes, O)
  frames = eframes.frames_from_dir(str(fdir), meta, H, W)
  opt = trainer.Optimizer(ckpt, 1e-4, momentum=0.9, weight_decay=4e-5)
  totals = []
  for s in range(4):
    frame = frames[s % 2]
    gt = eval_utils.gt_loss_fields_device(ren, frame, (W // 4, H // 4), frag_pool, 'lm',
                                          input_size=(W, H))
    lr = trainer.learning_rate(s, train_steps=2 if s < 2 else 4)
    values, bad, status = trainer.train_step(
        net, torch.from_numpy(images[s % 2][None]), {k: gt[k][None] for k in loss.GT_KEYS},
        opt, lr)
    assert bad.tolist() == [0] and status.tolist() == [0] * (3 + 2 * O)
    totals.append(float(values[3]))
  state = opt.state()
  assert len(state) == 12
  for name, ref in state.items():
    assert four[name].dtype == np.float32 and four[name].shape == ref.shape, name
    assert four[name].tobytes() == ref.tobytes(), name
    assert four[name].tobytes() != (two[name].tobytes()), name
  assert sorted(four) == sorted(list(ckpt) + [n + '/Momentum' for n in state
                                              if not n.endswith('/Momentum')] + ['global_step'])
  for name in ckpt:
    if name not in state:
      assert four[name].tobytes() == np.asarray(ckpt[name]).tobytes(), name
  # the logged total of step 2 is this loop's second value
  assert dict(recs[2]['scalars'])['train/total_loss'] == float(np.float32(totals[1]))

  # what infer.py would load from the folder: the step-4 weights
  class Args(object):
    checkpoint_name, synthetic, num_objs, num_frags, model_variant = None, 0, None, F, 'xception_65'
  loaded, num_objs, path = cli.load_checkpoint(Args, str(tdir))
  assert num_objs == O and path == str(tdir / 'model.ckpt-4')
  assert sorted(loaded) == sorted(ckpt)
  for name in state:
    if not name.endswith('/Momentum'):
      assert loaded[name].tobytes() == state[name].tobytes(), name
  torch.cuda.synchronize()
