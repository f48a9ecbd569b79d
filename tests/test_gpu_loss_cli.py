"""eval_loss.py end to end on two frames with ground-truth poses: the files it writes and its
losses against the numpy restatement on logits and ground-truth fields recomputed here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import loss_ref, mesh_cases      # noqa: E402

pytestmark = pytest.mark.gpu

H, W, O, F = 96, 128, 3, 64
NAMES = loss_ref.NAMES


def _rot(axis, angle):
  axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
  a, b, c = axis
  S = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]])
  return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def _run(model_root, bop, fdir, *extra):
  return subprocess.run(
      ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'eval_loss.py'),
       '--model=toy', '--synthetic', '2', '--frames', str(fdir), '--dataset', 'lm',
       '--num_objs', str(O)] + list(extra),
      env=dict(os.environ, TF_MODELS_PATH=str(model_root), BOP_PATH=str(bop)),
      capture_output=True, text=True)


def test_eval_loss_cli(tmp_path, gpu_children):
  from epos_amd import eval_utils, frames as eframes, model, ply, render, synthetic, tf_events
  from epos_amd import weights
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
  (tmp_path / 'toy' / 'params.yml').write_text('eval_crop_size: "%d,%d"\n' % (W, H))

  out = _run(tmp_path, bop, fdir)
  assert out.returncode == 0, out.stdout + out.stderr
  edir = tmp_path / 'toy' / 'eval_loss'
  events = [p for p in edir.iterdir() if p.name.startswith('events.out.tfevents.')]
  assert sorted(p.name for p in edir.iterdir() if p not in events) == ['losses_0.json']
  assert len(events) == 1
  assert not (tmp_path / 'toy' / 'eval').exists()
  doc = json.loads((edir / 'losses_0.json').read_text())
  assert doc['num_images'] == 2 and doc['global_step'] == 0
  assert doc['weights'] == {'obj_cls_loss_weight': 1.0, 'frag_cls_loss_weight': 1.0,
                            'frag_loc_loss_weight': 100.0}
  assert sorted(doc['per_image']) == ['1/1', '1/2']
  closing = [ln for ln in out.stdout.split('\n') if ln.startswith('eval_loss: ')]
  assert len(closing) == 1 and closing[0].startswith('eval_loss: 2 images, obj_cls=')
  scalars = dict(tf_events.read_events(str(events[0]))[1]['scalars'])
  assert sorted(scalars) == ['eval/frag_cls_loss', 'eval/frag_loc_loss', 'eval/obj_cls_loss',
                             'eval/total_loss']
  for name in NAMES:
    assert scalars['eval/' + name] == float(np.float32(doc['mean'][name]))

  # the same logits and ground-truth fields, recomputed here
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), crop_size=(W, H))
  net = model.get_net(ckpt, 1, H, W, O, F, mo, 'cuda:0')
  ren = render.Renderer('cuda:0')
  for o, m in sorted(ply.load_models(str(bop), 'lm', 'eval', obj_ids=[1, 2, 3]).items()):
    ren.add_model(o, m)
  frag_pool = render.pool_fragments(store.frag_centers, store.frag_sizes, O)
  frames = eframes.frames_from_dir(str(fdir), meta, H, W)
  h, w = H // 4, W // 4
  P = h * w
  from epos_amd import _lib
  share = int(_lib.load().epos_loss_share_pixels(P, O, F))
  sums, counts = [], []
  for img, frame in zip(images, frames):
    lg = net.forward_logits(img[None])
    gt = eval_utils.gt_loss_fields_device(ren, frame, (w, h), frag_pool, 'lm', input_size=(W, H))
    torch.cuda.synchronize()
    s, c, bad = loss_ref.terms(
        lg['pred_obj_conf'].cpu().numpy().reshape(1, P, O + 1),
        lg['pred_frag_conf'].cpu().numpy().reshape(1, P, O, F),
        lg['pred_frag_loc'].cpu().numpy().reshape(1, P, O, F, 3),
        gt['obj_label'].cpu().numpy().reshape(1, P), gt['frag_label'].cpu().numpy().reshape(1, P),
        gt['frag_loc'].cpu().numpy().reshape(1, P, 3),
        gt['frag_weight'].cpu().numpy().reshape(1, P), 255, share)
    assert bad[0] == 0 and (c[0, 1:, 0] > 0).sum() == 2          # both objects are seen
    sums.append(s[0])
    counts.append(c[0])
  exp = loss_ref.dataset_losses(np.stack(sums), np.stack(counts), (1.0, 1.0, 100.0))

  def close(got, ref, w_k, row_len):
    # per pixel (row + 16) 2^-52 (1 + loss / w) from the bound of the sums, plus one rounding
    # on either side for each of the host's additions, its product and its division
    tol = w_k * (row_len + 16) * 2.0 ** -52 * (1 + ref / w_k) + (O + 6) * 2.0 ** -52 * ref
    assert abs(got - ref) <= tol, (got, ref, tol)
  rows = [(doc['per_image']['1/%d' % (i + 1)], exp['per_image'][i]) for i in range(2)]
  for got, ref in rows + [(doc['mean'], exp['mean']), (doc['pooled'], exp['pooled'])]:
    assert got['obj_cls_loss'] > 0 and got['frag_cls_loss'] > 0 and got['frag_loc_loss'] > 0
    close(got['obj_cls_loss'], ref['obj_cls_loss'], 1.0, O + 1)
    close(got['frag_cls_loss'], ref['frag_cls_loss'], 1.0, F)
    assert got['frag_loc_loss'] == ref['frag_loc_loss']
    parts = (got['obj_cls_loss'] + got['frag_cls_loss']) + got['frag_loc_loss']
    if got is doc['mean']:               # the mean of the totals, not the total of the means
      assert abs(got['total_loss'] - parts) <= 6 * 2.0 ** -52 * parts
    else:
      assert got['total_loss'] == parts
  assert {int(o): v['pixels'] for o, v in doc['per_object'].items()} == {
      o: v['pixels'] for o, v in exp['per_object'].items()}

  # --frag_loc_loss_weight 1: frag_loc_loss divided by 100, to one rounding; a rerun overwrites
  again = _run(tmp_path, bop, fdir, '--frag_loc_loss_weight', '1')
  assert again.returncode == 0, again.stdout + again.stderr
  doc1 = json.loads((edir / 'losses_0.json').read_text())
  assert doc1['weights']['frag_loc_loss_weight'] == 1.0
  # the weight is applied last: b = fl(100 a), and fl(b / 100) is within two half-ulp roundings
  # of a, i.e. one ulp; the mean adds the rounding of one more addition on either side
  for part, ulps in [('pooled', 1), ('mean', 2)] + [(k, 1) for k in doc['per_image']]:
    a = (doc1[part] if part in doc1 else doc1['per_image'][part])['frag_loc_loss']
    b = (doc[part] if part in doc else doc['per_image'][part])['frag_loc_loss']
    assert a > 0 and abs(a - b / 100.0) <= ulps * 2.0 ** -52 * a, part
  for part in ('mean', 'pooled'):
    assert doc1[part]['obj_cls_loss'] == doc[part]['obj_cls_loss']
    assert doc1[part]['frag_cls_loss'] == doc[part]['frag_cls_loss']
  assert sorted(p.name for p in edir.iterdir()
                if not p.name.startswith('events.out.tfevents.')) == ['losses_0.json']
  torch.cuda.synchronize()
