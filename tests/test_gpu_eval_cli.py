"""eval.py end to end on two frames with ground-truth poses: the files it writes, its confusion
matrix against the numpy restatement on maps recomputed here, and the skip of a second run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import eval_ref, mesh_cases      # noqa: E402

pytestmark = pytest.mark.gpu

H, W, O, F = 96, 128, 3, 64


def _rot(axis, angle):
  axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
  a, b, c = axis
  S = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]])
  return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def _run_eval(model_root, bop, fdir):
  return subprocess.run(
      ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'eval.py'),
       '--model=toy', '--synthetic', '2', '--frames', str(fdir), '--dataset', 'lm',
       '--num_objs', str(O)],
      env=dict(os.environ, TF_MODELS_PATH=str(model_root), BOP_PATH=str(bop)),
      capture_output=True, text=True)


def test_eval_cli(tmp_path, gpu_children):
  from epos_amd import model, ply, render, synthetic, tf_events, weights
  store = synthetic.ModelStore(O, F, seed=0)           # the store eval.py --synthetic builds
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
  (tmp_path / 'toy' / 'params.yml').write_text('eval_crop_size: "%d,%d"\n' % (W, H))

  out = _run_eval(tmp_path, bop, fdir)
  assert out.returncode == 0, out.stdout + out.stderr
  edir = tmp_path / 'toy' / 'eval'
  events = [p for p in edir.iterdir() if p.name.startswith('events.out.tfevents.')]
  assert sorted(p.name for p in edir.iterdir() if p not in events) == [
      'cm_0.txt', 'last_evaluation.json', 'metrics_0.json']
  assert len(events) == 1
  metrics = json.loads((edir / 'metrics_0.json').read_text())
  last = json.loads((edir / 'last_evaluation.json').read_text())
  assert last['checkpoint_path'] is None and last['time'] > 0
  closing = [ln for ln in out.stdout.split('\n') if ln.startswith('eval: ')]
  assert len(closing) == 1 and closing[0].startswith('eval: 2 images, miou_all=')

  # the same maps, recomputed here: the rendered ground truth against the network's labels
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), crop_size=(W, H))
  ren = render.Renderer('cuda:0')
  for o, m in sorted(ply.load_models(str(bop), 'lm', 'eval', obj_ids=[1, 2, 3]).items()):
    ren.add_model(o, m)
  oK = np.array([[150.0 / 4, 0.0, 64.0 / 4], [0.0, 150.0 / 4, 48.0 / 4], [0.0, 0.0, 1.0]])
  exp = np.zeros((O + 1, O + 1), np.int64)
  for img, gt in zip(images, poses):
    pred = model.predict(img[None].astype(np.float32), mo, ckpt, num_objs=O, num_frags=F)
    label = pred['pred_obj_label'].cpu().numpy()
    assert label.shape == (1, H // 4, W // 4)
    gt_map = render.gt_label_map(ren, oK, [p['obj_id'] for p in gt],
                                 np.stack([p['R'] for p in gt]),
                                 np.stack([np.asarray(p['t'], np.float64) for p in gt]),
                                 (W // 4, H // 4))
    assert len(np.unique(gt_map)) == 3               # background and both objects
    cm, bad = eval_ref.confusion(gt_map, label, O + 1, 255)
    assert bad == 0
    exp += cm
  got = np.asarray(metrics['confusion_matrix'], np.int64)
  assert got.tobytes() == exp.tobytes()
  assert got.sum() == 2 * 24 * 32
  assert (metrics['miou_all'], metrics['miou_fg']) == pytest.approx(eval_ref.miou(exp), abs=1e-15)
  table = [[int(x) for x in r.split()] for r in (edir / 'cm_0.txt').read_text().split('\n') if r]
  assert [r[1:] for r in table[1:]] == exp.tolist()
  counts = np.array([metrics['frag_counts'][str(o)] for o in range(1, O + 1)])
  assert (counts[:, 0] == exp[1:].sum(axis=1)).all()          # one count per ground-truth pixel
  scalars = dict(tf_events.read_events(str(events[0]))[1]['scalars'])
  assert sorted(scalars) == ['eval/frag_acc', 'eval/frag_acc_seg', 'eval/obj_cls_miou_all',
                             'eval/obj_cls_miou_fg']
  assert scalars['eval/obj_cls_miou_all'] == float(np.float32(metrics['miou_all']))

  # the same checkpoint again: skipped with the reference's message, nothing rewritten
  before = {p.name: p.stat().st_mtime_ns for p in edir.iterdir()}
  again = _run_eval(tmp_path, bop, fdir)
  assert again.returncode == 0, again.stdout + again.stderr
  assert 'Skipping evaluation (checkpoint None has been evaluated).' in again.stdout
  assert {p.name: p.stat().st_mtime_ns for p in edir.iterdir()} == before
  torch.cuda.synchronize()
