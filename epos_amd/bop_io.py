"""BOP'19 result files -- restates what ``bop_toolkit_lib.inout.save_bop_results(
path, poses, version='bop19')`` writes (called at scripts/infer.py:753-760; the
bop_toolkit submodule is empty, format per the BOP'19 spec cited at
infer.py:751-752): a header line and one row per estimate,
``scene_id,im_id,obj_id,score,R,t,time`` with R (9 values, row-major) and t (3
values, mm) space separated.

Also the depth side of a BOP dataset folder, which VSD scoring reads (eval_poses.py --vsd):
``load_depth``, ``load_scene_camera`` and the path templates of the BOP format
(<split>/<scene:06d>/depth/<im:06d>.png, <split>/<scene:06d>/scene_camera.json). PARITY
UNPINNED against a real BOP folder: none is available, the layout is taken from the published
format description."""
import json
import os

import numpy as np


def load_depth(path, depth_scale=1.0):
  """A depth image as float32 [h,w] in mm: a 16-bit PNG (read with PIL as uint16) or a .npy
  (as stored), multiplied by depth_scale. 0 = no measurement."""
  if path.endswith('.npy'):
    raw = np.load(path)
  else:
    from PIL import Image
    with Image.open(path) as pil:
      raw = np.asarray(pil)
    if raw.dtype != np.uint16:
      raw = raw.astype(np.uint16)      # PIL hands 16-bit PNGs out as int32 ('I') in places
  if raw.ndim != 2:
    raise ValueError('depth image %s is %s, expected [h,w]' % (path, raw.shape))
  return np.ascontiguousarray(raw.astype(np.float32) * np.float32(depth_scale))


def save_depth_png(path, depth):
  """uint16 [h,w] -> 16-bit PNG (fixtures and tools)."""
  from PIL import Image
  Image.fromarray(np.ascontiguousarray(depth, np.uint16)).save(path)


def load_scene_camera(path):
  """scene_camera.json -> {im_id: {'cam_K': f64 [3,3], 'depth_scale': float}}."""
  with open(path) as f:
    raw = json.load(f)
  return {int(k): {'cam_K': np.asarray(v['cam_K'], np.float64).reshape(3, 3),
                   'depth_scale': float(v.get('depth_scale', 1.0))} for k, v in raw.items()}


def scene_dir(datasets_path, dataset, split, scene_id):
  return os.path.join(datasets_path, dataset, split, '%06d' % int(scene_id))


def depth_path(datasets_path, dataset, split, scene_id, im_id):
  return os.path.join(scene_dir(datasets_path, dataset, split, scene_id), 'depth',
                      '%06d.png' % int(im_id))


def scene_camera_path(datasets_path, dataset, split, scene_id):
  return os.path.join(scene_dir(datasets_path, dataset, split, scene_id), 'scene_camera.json')


def save_bop_results(path, results, version='bop19'):
  if version != 'bop19':
    raise ValueError('Unknown version of BOP results.')
  lines = ['scene_id,im_id,obj_id,score,R,t,time']
  for res in results:
    run_time = res['time'] if 'time' in res else -1
    lines.append('{scene_id},{im_id},{obj_id},{score},{R},{t},{time}'.format(
        scene_id=res['scene_id'], im_id=res['im_id'], obj_id=res['obj_id'],
        score=res['score'],
        R=' '.join(map(str, np.asarray(res['R']).flatten().tolist())),
        t=' '.join(map(str, np.asarray(res['t']).flatten().tolist())),
        time=run_time))
  with open(path, 'w') as f:
    f.write('\n'.join(lines))


def load_bop_results(path, version='bop19'):
  if version != 'bop19':
    raise ValueError('Unknown version of BOP results.')
  results = []
  with open(path, 'r') as f:
    for i, line in enumerate(f):
      if i == 0 or not line.strip():
        continue
      e = line.strip().split(',')
      results.append({
          'scene_id': int(e[0]), 'im_id': int(e[1]), 'obj_id': int(e[2]),
          'score': float(e[3]),
          'R': np.array(list(map(float, e[4].split())), np.float64).reshape(3, 3),
          't': np.array(list(map(float, e[5].split())), np.float64).reshape(3, 1),
          'time': float(e[6])})
  return results
