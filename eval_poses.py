#!/usr/bin/env python
"""Scores the poses ``infer.py`` estimated -- MSSD, MSPD, ADD(-S) and, with --vsd, VSD recalls
and BOP's AR on MI355X.

    python eval_poses.py --model=<model_name> --dataset <d>
        (--infer_tfrecord_names a,b | --frames <dir>)
        [--infer_name N | --result_path file.csv] [--adi true|false]
        [--vsd true --depth_split test [--vsd_delta 15] [--vsd_max_instances N]]
        [--min_visib_fract 0.1]

The reference has no such script: it leaves pose scoring to ``bop_toolkit``, an empty submodule
there. Environment as for ``eval.py``: TF_DATA_PATH / TF_MODELS_PATH / BOP_PATH, and
<TF_MODELS_PATH>/<model>/params.yml overrides flag defaults.

  * estimates: <model>/infer/estimated-poses[_<infer_name>].csv as ``infer.py`` wrote it (BOP'19
    format), or --result_path;
  * frames: metadata only -- ids, camera, targets and ground-truth poses from the TFRecords or
    from <dir>/frames.json. No pixel is decoded, no image file has to exist, no checkpoint is
    read;
  * targets: Frame.targets, as in ``infer.py`` (every annotated instance of the dataset's
    objects). Per (scene, image, object) the n best-scored estimates are kept, n = the
    instance count. BOP'19's own test_targets_bop19.json and its rule that only instances
    visible by at least 10 % count are NOT applied, so the recalls are not the leaderboard's;
  * models: <BOP_PATH>/<dataset>/models_eval/ with models_info.json (diameters, symmetries);
  * errors: epos_amd/pose_error.py, this build's definitions (include/epos_hip.h, "Pose
    errors"); one launch sequence and one download for the whole run;
  * results in <model>/eval/: pose_scores[_<infer_name>].json (thresholds, per-object and
    overall recalls, counts of estimates, targets and non-finite pairs) and
    pose_errors[_<infer_name>].csv, one row per (estimate, ground truth) pair.

``mean_ar_mssd_mspd`` is the mean of AR_MSSD and AR_MSPD; it is not BOP's AR, which also
averages AR_VSD.

--vsd true adds VSD (epos_amd/vsd.py, include/epos_hip.h "VSD"): the ground truth and the
estimate of every pair are rendered on the device, compared with the test depth image, and
``ar_vsd`` (mean recall over 10 taus x 10 thresholds) and ``ar`` = (ar_vsd + ar_mssd +
ar_mspd) / 3 are reported next to the figures above, which stay. The test depth comes from
  * --depth_split <split>: <BOP_PATH>/<dataset>/<split>/<scene:06d>/depth/<im:06d>.png with
    the scene's scene_camera.json (cam_K, depth_scale), at the dataset's native resolution --
    a pose is metric, so the crop or resize the network saw does not matter. This is the route
    for TFRecord frames. Parity unpinned vs a real BOP folder (none was available);
  * --frames <dir>: the ``depth_path`` (relative to <dir>; 16-bit PNG or .npy) and
    ``depth_scale`` (default 1) of a frames.json entry, in the frame's own geometry and K.
A frame without depth is an error, not a skip. --min_visib_fract F > 0 (needs a depth source
too) first measures the visible fraction of every ground-truth instance and drops those below F
from the targets -- BOP's "visible by at least 10 %" rule as an opt-in.
Unpinned, as for the other errors: the VSD values are this build's definitions after the
published formulas, not bop_toolkit's numbers; the ray of a pixel goes through x + .5, the
sample point of this build's renderer, not necessarily bop_toolkit's; and
test_targets_bop19.json is still not applied, so ``ar`` is BOP's formula over this script's
targets.
"""
import argparse
import json
import os
import sys

import numpy as np     # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from epos_amd import cli   # noqa: E402


def build_parser():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawTextHelpFormatter)
  a = ap.add_argument
  a('--model', required=True)
  a('--dataset', default=None)
  a('--infer_tfrecord_names', default=None)
  a('--infer_max_height_before_crop', type=int, default=480)
  a('--infer_crop_size', default='640,480')
  a('--infer_name', default=None)
  a('--frames', default=None, help='directory with frames.json (the images are not read)')
  a('--synthetic', type=int, default=0,
    help='refused: synthetic frames carry no ground-truth poses')
  a('--seed', type=int, default=0)
  a('--result_path', default=None,
    help='the BOP\'19 CSV (default: <model>/infer/estimated-poses[_<infer_name>].csv)')
  a('--adi', type=cli.str2bool, default=True,
    help='compute ADI (O(vertices^2) per pair); false: ADD(-S) recall uses ADD only for '
         'objects without symmetries and is left out for the others')
  a('--vsd', type=cli.str2bool, default=False,
    help='also score VSD and report ar_vsd and ar (needs --depth_split, or depth_path entries '
         'in <frames>/frames.json)')
  a('--depth_split', default=None,
    help='read the test depth from <BOP_PATH>/<dataset>/<split>/<scene:06d>/depth/ and the '
         'camera from that scene\'s scene_camera.json')
  a('--vsd_delta', type=float, default=15.0, help='visibility tolerance in mm')
  a('--min_visib_fract', type=float, default=0.0,
    help='> 0: ground-truth instances visible by less than this fraction are no targets')
  a('--vsd_max_instances', type=int, default=None,
    help='instances rendered per chunk (default: from the image size and a 1 GiB workspace)')
  return ap


def prepare(argv=None):
  """Parses the command line, applies params.yml and refuses what cannot be scored."""
  args = build_parser().parse_args(argv)
  model_dir = cli.model_dir(args)
  cli.update_flags(args, os.path.join(model_dir, cli.PARAMS_FILENAME))
  if args.synthetic:
    raise ValueError('eval_poses.py: --synthetic frames carry no ground-truth poses; give '
                     '--infer_tfrecord_names or --frames <dir> with gt_poses')
  if not (args.dataset and os.environ.get('BOP_PATH')):
    raise ValueError('eval_poses.py needs --dataset and $BOP_PATH (models_eval)')
  if not (args.infer_tfrecord_names or args.frames):
    raise ValueError('No input files: give --infer_tfrecord_names or --frames <dir>.')
  if not 0.0 <= args.min_visib_fract <= 1.0:
    raise ValueError('--min_visib_fract must be in 0..1')
  if (args.vsd or args.min_visib_fract > 0) and not (args.depth_split or args.frames):
    raise ValueError('eval_poses.py: {} needs the test depth images: give --depth_split <split> '
                     '(read from $BOP_PATH) or --frames <dir> with depth_path entries'.format(
                         '--vsd' if args.vsd else '--min_visib_fract'))
  return args, model_dir


def result_path(args, model_dir):
  if args.result_path:
    return args.result_path
  return os.path.join(model_dir, 'infer',
                      'estimated-poses{}.csv'.format(cli.result_suffix(args.infer_name)))


class DepthFrames(object):
  """The (depth_mm f32 [h,w], K) of every frame, read on demand (the last `keep` stay in
  memory: the VSD chunks walk the frames in order)."""

  def __init__(self, sources, keep=256):
    self.sources, self.keep = sources, keep
    self._cache = {}

  def __len__(self):
    return len(self.sources)

  def __getitem__(self, i):
    if i not in self._cache:
      from epos_amd import bop_io
      path, scale, K = self.sources[i]
      while len(self._cache) >= self.keep:
        self._cache.pop(next(iter(self._cache)))
      self._cache[i] = (bop_io.load_depth(path, scale), K)
    return self._cache[i]


def depth_sources(args, frames, meta):
  """Per frame (path, depth_scale, K) of its test depth image; a frame without one is an
  error that names it. meta: the frames.json entries the frames were made from (not read with
  --depth_split)."""
  from epos_amd import bop_io
  out = []
  if args.depth_split:
    cams = {}
    bop = os.environ['BOP_PATH']
    for f in frames:
      if f.scene_id not in cams:
        cam_path = bop_io.scene_camera_path(bop, args.dataset, args.depth_split, f.scene_id)
        if not os.path.exists(cam_path):
          raise ValueError('no scene_camera.json for scene {} at {}'.format(f.scene_id, cam_path))
        cams[f.scene_id] = bop_io.load_scene_camera(cam_path)
      path = bop_io.depth_path(bop, args.dataset, args.depth_split, f.scene_id, f.im_id)
      if f.im_id not in cams[f.scene_id] or not os.path.exists(path):
        raise ValueError('frame scene {} image {} has no test depth ({}, or its entry in '
                         'scene_camera.json)'.format(f.scene_id, f.im_id, path))
      cam = cams[f.scene_id][f.im_id]
      out.append((path, cam['depth_scale'], cam['cam_K']))
    return out
  for f, m in zip(frames, meta):
    path = os.path.join(args.frames, m['depth_path']) if m.get('depth_path') else None
    if path is None or not os.path.exists(path):
      raise ValueError('frame scene {} image {} has no test depth (frames.json entry without '
                       'depth_path, or the file is missing: {})'.format(
                           f.scene_id, f.im_id, path))
    out.append((path, float(m.get('depth_scale', 1.0)), f.K))
  return out


def build_groups(frames, results, dropped=None):
  """One group per (frame, target object): the n best-scored estimates (n = the instance count;
  ties keep file order) and the object's ground-truth poses. Returns (groups, ignored): the
  estimates of images or objects that are no target. dropped: {(frame index, obj_id): indices
  into that object's ground-truth poses} that are no targets (--min_visib_fract); the instance
  count shrinks with them."""
  by_key = {}
  for r in results:
    by_key.setdefault((r['scene_id'], r['im_id'], r['obj_id']), []).append(r)
  groups, used = [], 0
  for fi, f in enumerate(frames):
    for o in sorted(f.targets):
      n_inst = f.targets[o]
      gone = (dropped or {}).get((fi, int(o)), ())
      if n_inst >= 0:
        n_inst = max(0, n_inst - len(gone))
      ests = by_key.get((f.scene_id, f.im_id, o), [])
      order = np.argsort(-np.array([e['score'] for e in ests], np.float64), kind='stable')
      if n_inst >= 0:
        order = order[:n_inst]
      used += len(order)
      gts = [p for p in f.gt_poses if p['obj_id'] == o]
      groups.append({'frame': f, 'frame_index': fi, 'obj_id': int(o),
                     'ests': [ests[i] for i in order],
                     'gts': [p for k, p in enumerate(gts) if k not in gone]})
  return groups, len(results) - used


def invisible_targets(groups, vsd_eval, depth, args):
  """The ground-truth-only pass of --min_visib_fract: {(frame index, obj_id): indices of the
  ground truths whose visible fraction is below the bound}."""
  queries, owner = [], []
  for g in groups:
    for ti, t in enumerate(g['gts']):
      queries.append({'frame': g['frame_index'], 'obj_id': g['obj_id'], 'R_g': t['R'],
                      't_g': t['t'], 'R_e': None, 't_e': None})
      owner.append((g['frame_index'], g['obj_id'], ti))
  _, fract = vsd_eval.errors(depth, queries, delta=args.vsd_delta)
  dropped = {}
  for (fi, o, ti), v in zip(owner, fract):
    if v < args.min_visib_fract:
      dropped.setdefault((fi, o), set()).add(ti)
  return dropped


def main(argv=None):
  args, model_dir = prepare(argv)
  from epos_amd import bop_io, ply, pose_error
  # metadata only: no pixel is decoded, and a --frames directory needs no image files
  meta = cli.read_frames_json(args.frames) if args.frames else None
  obj_ids = ply.BOP_OBJ_IDS.get(args.dataset)
  frames = cli.load_frames(
      args.infer_tfrecord_names, args.frames, 0, args.infer_crop_size,
      args.infer_max_height_before_crop, args.seed, len(obj_ids or ()), obj_ids=obj_ids,
      pixels=False, meta=meta)[0]
  if not frames:
    raise ValueError('no frames to score')
  if any(f.gt_poses is None for f in frames):
    raise ValueError('eval_poses.py: input without ground-truth poses cannot be scored '
                     '(frames.json entries need gt_poses)')
  # a frame without test depth is refused before anything touches a device
  use_depth = args.vsd or args.min_visib_fract > 0
  depth = DepthFrames(depth_sources(args, frames, meta)) if use_depth else None
  path = result_path(args, model_dir)
  if not os.path.exists(path):
    raise ValueError('no pose estimates at {} (run infer.py first)'.format(path))
  results = bop_io.load_bop_results(path)
  groups, ignored = build_groups(frames, results)

  bop = os.environ['BOP_PATH']
  obj_ids = sorted(set(g['obj_id'] for g in groups))
  info = pose_error.load_models_info(pose_error.models_info_path(bop, args.dataset, 'eval'))
  models = ply.load_models(bop, args.dataset, 'eval', obj_ids=obj_ids)
  dev = 'cuda:%d' % cli.device_from_env()
  ev = pose_error.PoseErrorEval(models, info, dev)
  vsd_eval = n_dropped = None
  if use_depth:
    from epos_amd import vsd
    vsd_eval = vsd.VsdEval(models, info, dev, max_instances=args.vsd_max_instances)
  if args.min_visib_fract > 0:
    dropped = invisible_targets(groups, vsd_eval, depth, args)
    n_dropped = sum(len(v) for v in dropped.values())
    groups, ignored = build_groups(frames, results, dropped)

  pairs, owner = [], []
  for gi, g in enumerate(groups):
    for ei, e in enumerate(g['ests']):
      for ti, t in enumerate(g['gts']):
        pairs.append({'obj_id': g['obj_id'], 'R_e': e['R'], 't_e': e['t'], 'R_g': t['R'],
                      't_g': t['t'], 'K': g['frame'].K})
        owner.append((gi, ei, ti))
  err = ev.errors(pairs, want_adi=args.adi)
  non_finite = int(np.isinf(err[:, 5]).sum()) if len(err) else 0
  if args.vsd:
    vsd_err, gt_visib = vsd_eval.errors(
        depth, [{'frame': groups[gi]['frame_index'], 'obj_id': p['obj_id'], 'R_g': p['R_g'],
                 't_g': p['t_g'], 'R_e': p['R_e'], 't_e': p['t_e']}
                for p, (gi, _, _) in zip(pairs, owner)], delta=args.vsd_delta)

  for g in groups:
    g['errors'] = np.zeros((len(g['ests']), len(g['gts']), 6))
    g['scores'] = [e['score'] for e in g['ests']]
  for (gi, ei, ti), row in zip(owner, err):
    groups[gi]['errors'][ei, ti] = row
  n_syms = {o: ev.n_sym(o) for o in obj_ids}
  width = cli.crop_size(args.infer_crop_size)[0]
  missing = [o for o in obj_ids if o not in ev.diameters]
  if missing:
    raise ValueError('models_info.json gives no diameter for object(s) {}'.format(missing))
  rec = pose_error.recalls(groups, ev.diameters, n_syms, width)
  if not args.adi:                       # no ADI: no ADD(-S) figure for symmetric objects
    for o, r in rec['per_object'].items():
      if n_syms[o] > 1:
        r['add_s_recall'] = None
    if any(n_syms[o] > 1 for o in obj_ids):
      rec['overall']['add_s_recall'] = None
  if args.vsd:
    for g in groups:
      g['vsd'] = np.ones((len(g['ests']), len(g['gts']), len(vsd.VSD_TAUS)))
    for (gi, ei, ti), row in zip(owner, vsd_err):
      groups[gi]['vsd'][ei, ti] = row
    rec_vsd = vsd.recalls_vsd(groups)
    for r, rv in [(rec['overall'], rec_vsd['overall'])] + [
        (rec['per_object'][o], rec_vsd['per_object'][o]) for o in rec['per_object']]:
      r['recall_vsd'], r['ar_vsd'] = rv['recall_vsd'], rv['ar_vsd']
      r['ar'] = vsd.ar(rv['ar_vsd'], r['ar_mssd'], r['ar_mspd'])

  eval_dir = os.path.join(model_dir, 'eval')
  os.makedirs(eval_dir, exist_ok=True)
  suffix = cli.result_suffix(args.infer_name)
  scores = {
      'result_path': path, 'dataset': args.dataset, 'image_width': width, 'adi': bool(args.adi),
      'thresholds': {
          'mssd_x_diameter': list(pose_error.MSSD_FACTORS),
          'mspd_px_at_width_640': list(pose_error.MSPD_FACTORS),
          'mspd_px': [c * (width / 640.0) for c in pose_error.MSPD_FACTORS],
          'add_s_x_diameter': pose_error.ADD_FACTOR,
          'max_sym_disc_step': pose_error.MAX_SYM_DISC_STEP},
      'diameters': {str(o): ev.diameters[o] for o in obj_ids},
      'n_symmetries': {str(o): n_syms[o] for o in obj_ids},
      'counts': {'frames': len(frames), 'estimates_in_file': len(results),
                 'estimates_scored': len(results) - ignored, 'estimates_ignored': ignored,
                 'targets': rec['overall']['targets'], 'pairs': len(pairs),
                 'non_finite_pairs': non_finite},
      'per_object': {str(o): r for o, r in rec['per_object'].items()},
      'overall': rec['overall'],
  }
  if args.vsd:
    scores['thresholds']['vsd_taus'] = list(vsd.VSD_TAUS)
    scores['thresholds']['vsd_thresholds'] = list(vsd.VSD_THRESHOLDS)
    scores['vsd_delta'] = args.vsd_delta
  if n_dropped is not None:
    scores['min_visib_fract'] = args.min_visib_fract
    scores['counts']['targets_dropped_by_visibility'] = n_dropped
  scores_path = os.path.join(eval_dir, 'pose_scores{}.json'.format(suffix))
  with open(scores_path, 'w') as f:
    json.dump(scores, f, indent=1)
  with open(os.path.join(eval_dir, 'pose_errors{}.csv'.format(suffix)), 'w') as f:
    f.write('scene_id,im_id,obj_id,est_rank,gt_index,score,' +
            ','.join(pose_error.ERROR_NAMES) + (
                ',' + ','.join('vsd_%.2f' % t for t in vsd.VSD_TAUS) + ',gt_visib_fract'
                if args.vsd else '') + '\n')
    for k, ((gi, ei, ti), row) in enumerate(zip(owner, err)):
      g = groups[gi]
      if args.vsd:
        row = list(row) + list(vsd_err[k]) + [gt_visib[k]]
      f.write('{},{},{},{},{},{},{}\n'.format(
          g['frame'].scene_id, g['frame'].im_id, g['obj_id'], ei, ti, g['scores'][ei],
          ','.join(repr(float(v)) for v in row)))
  o = rec['overall']
  print('eval_poses: {} targets, {} estimates scored, AR_MSSD={:.4f}, AR_MSPD={:.4f}, '
        'mean={:.4f}, ADD(-S) recall={}'.format(
            o['targets'], len(results) - ignored, o['ar_mssd'], o['ar_mspd'],
            o['mean_ar_mssd_mspd'],
            'n/a' if o['add_s_recall'] is None else '{:.4f}'.format(o['add_s_recall'])))
  if args.vsd:
    print('eval_poses: AR_VSD={:.4f}, AR={:.4f} (this build\'s definitions; '
          'test_targets_bop19.json is not applied)'.format(o['ar_vsd'], o['ar']))
  print('Saved pose scores to: {}'.format(scores_path))
  return scores


if __name__ == '__main__':
  main()
