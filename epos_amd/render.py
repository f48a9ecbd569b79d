"""Mesh renderer on the device (csrc/render.hip): a ``bop_renderer.Renderer``-shaped class
over the batched z-buffered rasteriser, and the ground-truth maps the reference builds from
per-instance renderings (datagen.py:570-604, datagen_utils.py:65-94,161-232).

The geometry rules (sample point, near rule without clipping, 1/256-pixel snapping, integer
edge functions, the key that decides visibility, the headlight term) are listed in
include/epos_hip.h under "Mesh renderer" and in DESIGN.md, "Renderer". PARITY UNPINNED against
bop_renderer, which is not available: the sample point, the near rule and the shading are this
build's definitions.

There is no CPU fallback: without the library or a device every entry point raises EposError.
"""
import ctypes

import numpy as np

from epos_amd import _call as C
from epos_amd import _lib
from epos_amd._lib import EposError

NEAR = 10.0                       # mm; a triangle with a vertex nearer than this is dropped
OUTPUTS = ('depth', 'face', 'local_pos', 'color')

_INST = np.dtype([('vert_base', np.int32), ('face_base', np.int32), ('n_faces', np.int32),
                  ('reserved0', np.int32), ('R', np.float64, 9), ('t', np.float64, 3),
                  ('fx', np.float64), ('fy', np.float64), ('cx', np.float64),
                  ('cy', np.float64)])
assert _INST.itemsize == ctypes.sizeof(_lib.RenderInst) == 144


def _torch_device(device):
  import torch
  C.need_device(None, 'the mesh renderer needs a HIP device (there is no CPU fallback)')
  return torch.device(device if device is not None else 'cuda:0')


def vertex_colors(model):
  """u8 [V,3]: the model's 'colors', else the object-frame colouring of vis.colorize_xyz."""
  if model.get('colors') is not None:
    return np.ascontiguousarray(np.clip(np.asarray(model['colors'])[:, :3], 0, 255), np.uint8)
  from epos_amd import vis
  return np.ascontiguousarray(vis.colorize_xyz(model['pts']))


def quaternion_to_matrix(q):
  """(w, x, y, z) -> 3x3 rotation (the convention of the reference's gt_obj_quats)."""
  w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
  return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _rotations(Rs):
  Rs = np.asarray(Rs, np.float64)
  if Rs.ndim == 2 and Rs.shape[1] == 4:
    return np.stack([quaternion_to_matrix(q) for q in Rs]) if len(Rs) else np.zeros((0, 3, 3))
  return Rs.reshape(-1, 3, 3)


class Renderer(object):
  """bop_renderer's method names (init, add_object, render_object, get_*_image), so that code
  written against it -- the reference's vis.visualize_object_poses and datagen_utils -- binds
  to an instance unchanged, plus the batched render_instances."""

  def __init__(self, device=None, near=NEAR):
    self.lib = _lib.load()
    self.device = _torch_device(device)
    self.near = float(near)
    self.width = self.height = None
    self._models = {}               # obj_id -> (vert_base, face_base, n_faces)
    self._verts, self._faces, self._colors = [], [], []
    self._nv = self._nf = 0
    self._pool = None               # device tensors, rebuilt after add_*
    self._work = {}                 # (h, w) -> {name: buffer for the most instances seen}
    self._last = {}                 # obj_id -> host images of the last render_object

  def init(self, width, height):
    self.width, self.height = int(width), int(height)

  def add_object(self, obj_id, path):
    from epos_amd import ply
    self.add_model(obj_id, ply.load_ply(path))

  def add_model(self, obj_id, model):
    if model.get('faces') is None or len(model['faces']) == 0:
      raise EposError('object %d: the model has no faces, the mesh renderer needs them' % obj_id)
    pts = np.ascontiguousarray(model['pts'], np.float64).reshape(-1, 3)
    faces = np.ascontiguousarray(model['faces'], np.int32).reshape(-1, 3)
    if faces.min() < 0 or faces.max() >= len(pts):
      raise EposError('object %d: face indices outside the vertex array' % obj_id)
    if self._nv + len(pts) >= 2 ** 31 or self._nf + len(faces) >= 2 ** 31:
      raise EposError('mesh pool too large')
    self._models[int(obj_id)] = (self._nv, self._nf, len(faces))
    self._verts.append(pts)
    self._faces.append(faces)
    self._colors.append(vertex_colors(model))
    self._nv += len(pts)
    self._nf += len(faces)
    self._pool = None

  def has_object(self, obj_id):
    return int(obj_id) in self._models

  def _upload(self):
    import torch
    if self._pool is None:
      self._pool = tuple(torch.from_numpy(np.concatenate(a)).to(self.device)
                         for a in (self._verts, self._faces, self._colors))
    return self._pool

  _WORK = {'keys': ('int64', ()), 'depth': ('float32', ()), 'face': ('int32', ()),
           'local_pos': ('float32', (3,)), 'color': ('uint8', (3,))}

  def _workspace(self, n, h, w, names):
    """Buffers of the image size (h, w), kept per size and carved once: each holds as many
    instances as the largest call of that size asked for (a larger call regrows it), only the
    buffers a call names exist. Returns views of the first n instances."""
    import torch
    sized = self._work.setdefault((h, w), {})
    out = {}
    for name in names:
      buf = sized.get(name)
      if buf is None or buf.shape[0] < n:
        dtype, tail = self._WORK[name]
        buf = torch.empty((max(n, 1), h, w) + tail, dtype=getattr(torch, dtype),
                          device=self.device)
        sized[name] = buf
      out[name] = buf[:n]
    return out

  def instance_table(self, obj_ids, Rs, ts, K):
    """The host side of EposRenderInst [N]: K is [3,3] for all instances or [N,3,3]."""
    n = len(obj_ids)
    Rs = _rotations(Rs)
    ts = np.asarray(ts, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64)
    K = np.broadcast_to(K, (n, 3, 3)) if K.ndim == 2 else K.reshape(-1, 3, 3)
    if not (len(Rs) == len(ts) == len(K) == n):
      raise ValueError('obj_ids, Rs, ts and K disagree on the number of instances')
    tab = np.zeros(n, _INST)
    for i, o in enumerate(obj_ids):
      if int(o) not in self._models:
        raise EposError('object %d was not added to the renderer' % int(o))
      tab['vert_base'][i], tab['face_base'][i], tab['n_faces'][i] = self._models[int(o)]
    tab['R'] = Rs.reshape(n, 9)
    tab['t'] = ts
    tab['fx'], tab['fy'], tab['cx'], tab['cy'] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    return tab

  def render_instances(self, obj_ids, Rs, ts, K, size=None, outputs=OUTPUTS):
    """N instances in one raster and one resolve launch. Returns {name: device tensor} for the
    names in `outputs` (depth f32 [N,h,w], face i32 [N,h,w], local_pos f32 [N,h,w,3], color
    u8 [N,h,w,3]) plus 'keys' (i64 [N,h,w], the bits of the u64 keys). The tensors are the
    renderer's workspace: the next call of the same image size writes over them."""
    import torch
    w, h = (self.width, self.height) if size is None else (int(size[0]), int(size[1]))
    if not w or not h or w < 0 or h < 0:
      raise ValueError('no image size: call init(width, height) or pass size=(w, h)')
    unknown = set(outputs) - set(OUTPUTS)
    if unknown:
      raise ValueError('unknown outputs %s' % sorted(unknown))
    n = len(obj_ids)
    tab = self.instance_table(obj_ids, Rs, ts, K)
    ws = self._workspace(n, h, w, tuple(outputs) + ('keys',))
    if n == 0:
      return ws
    verts, faces, colors = self._upload()
    insts = torch.from_numpy(tab.view(np.uint8).reshape(n, -1)).to(self.device)
    with C.launch(self.device) as q:
      q.keep(insts)
      _lib.check(self.lib.epos_render_raster(
          C.ptr(verts), self._nv, C.ptr(faces), self._nf, C.ptr(insts), n, h, w, self.near,
          C.ptr(ws['keys']), q.handle), 'epos_render_raster')
      _lib.check(self.lib.epos_render_resolve(
          C.ptr(ws['keys']), C.ptr(verts), self._nv, C.ptr(faces), self._nf, C.ptr(colors),
          C.ptr(insts), n, h, w, self.near,
          *[C.ptr(ws.get(k)) for k in OUTPUTS], q.handle),
                 'epos_render_resolve')
    return ws

  # ---- bop_renderer's single-object form ----
  def render_object(self, obj_id, R_list, t_list, fx, fy, cx, cy):
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    out = self.render_instances([obj_id], np.asarray(R_list, np.float64).reshape(1, 3, 3),
                                np.asarray(t_list, np.float64).reshape(1, 3), K,
                                outputs=('depth', 'local_pos', 'color'))
    self._last[int(obj_id)] = {k: out[k][0].cpu().numpy()
                               for k in ('depth', 'local_pos', 'color')}

  def _image(self, obj_id, name):
    if int(obj_id) not in self._last:
      raise EposError('object %d has not been rendered' % int(obj_id))
    return self._last[int(obj_id)][name]

  def get_depth_image(self, obj_id):
    return self._image(obj_id, 'depth')

  def get_color_image(self, obj_id):
    return self._image(obj_id, 'color')

  def get_local_pos_image(self, obj_id):
    return self._image(obj_id, 'local_pos')


def pool_fragments(frag_centers, frag_sizes, num_objs=None):
  """{obj_id: [F,3]}, {obj_id: [F]} -> f64 [O,F,3], f64 [O,F] (objects without fragments:
  centres 0, sizes 1 -- they are never looked up by an instance that is rendered)."""
  ids = sorted(int(o) for o in frag_centers)
  if not ids:
    raise EposError('no fragment centres')
  O = max(ids) if num_objs is None else int(num_objs)
  F = len(frag_centers[ids[0]])
  if not 1 <= F <= 256:
    raise EposError('num_frags must be in 1..256')
  centers, sizes = np.zeros((O, F, 3)), np.ones((O, F))
  for o in ids:
    if 1 <= o <= O:
      centers[o - 1] = np.asarray(frag_centers[o], np.float64).reshape(F, 3)
      sizes[o - 1] = np.asarray(frag_sizes[o], np.float64).reshape(F)
  return centers, sizes


MAX_KNN_FRAGS = 4                            # EPOS_LOSS_MAX_KNN


def gt_fields_device(depth, local_pos, obj_ids, centers, sizes, masks=None, knn_frags=1):
  """epos_gt_fields_knn on device tensors depth f32 [N,h,w], local_pos f32 [N,h,w,3], optional
  masks u8 [N,h,w]; obj_ids a sequence, centers / sizes the pooled host arrays. Returns
  {obj_label, instance, frag_label, frag_loc, frag_weight} as device tensors. knn_frags = k > 1
  (at most min(F, 4)): frag_label [h,w,k], frag_loc [h,w,k,3] and frag_weight [h,w,k] hold the
  k nearest fragments in ascending distance; with 1 the shapes are [h,w], [h,w,3], [h,w]."""
  import torch
  lib = _lib.load()
  dev = depth.device
  C.need_device(depth, 'the ground-truth fields need a HIP device (there is no CPU fallback)')
  n, h, w = depth.shape
  centers = np.ascontiguousarray(centers, np.float64)
  sizes = np.ascontiguousarray(sizes, np.float64)
  O, F = sizes.shape
  if centers.shape != (O, F, 3):
    raise ValueError('centers %s do not match sizes %s' % (centers.shape, sizes.shape))
  if masks is not None and tuple(masks.shape) != (n, h, w):
    raise ValueError('masks %s do not match depth %s' % (tuple(masks.shape), (n, h, w)))
  k = int(knn_frags)
  if k != knn_frags or k < 1 or k > min(F, MAX_KNN_FRAGS):
    raise ValueError('knn_frags must be in 1..%d, got %r' % (min(F, MAX_KNN_FRAGS), knn_frags))
  slots = () if k == 1 else (k,)
  ids = torch.tensor([int(o) for o in obj_ids] or [0], dtype=torch.int32, device=dev)
  c_dev, s_dev = torch.from_numpy(centers).to(dev), torch.from_numpy(sizes).to(dev)
  out = {'obj_label': torch.empty((h, w), dtype=torch.int32, device=dev),
         'instance': torch.empty((h, w), dtype=torch.int32, device=dev),
         'frag_label': torch.empty((h, w) + slots, dtype=torch.int32, device=dev),
         'frag_loc': torch.empty((h, w) + slots + (3,), dtype=torch.float32, device=dev),
         'frag_weight': torch.empty((h, w) + slots, dtype=torch.float32, device=dev)}
  with C.launch(dev) as q:
    q.keep(ids, c_dev, s_dev)
    _lib.check(lib.epos_gt_fields_knn(
        C.ptr(depth), C.ptr(local_pos), C.ptr(masks), C.ptr(ids), n, h, w, C.ptr(c_dev),
        C.ptr(s_dev), O, F, k, C.ptr(out['obj_label']), C.ptr(out['instance']),
        C.ptr(out['frag_label']), C.ptr(out['frag_loc']), C.ptr(out['frag_weight']),
        q.handle), 'epos_gt_fields_knn')
  return out


def _masks_to_device(masks, device):
  import torch
  if masks is None:
    return None
  m = np.ascontiguousarray(np.asarray(masks) != 0, np.uint8)
  return torch.from_numpy(m).to(device)


def gt_fields(renderer, K, obj_ids, Rs, ts, size, centers, sizes, masks=None, knn_frags=1):
  """Renders every instance at `size` = (w, h) and builds the ground-truth maps; returns the
  dict of gt_fields_device. masks: optional [N,h,w] instance masks (host); knn_frags: the
  fragments per pixel, as gt_fields_device takes it."""
  out = renderer.render_instances(obj_ids, Rs, ts, K, size=size,
                                  outputs=('depth', 'local_pos'))
  return gt_fields_device(out['depth'], out['local_pos'], obj_ids, centers, sizes,
                          _masks_to_device(masks, renderer.device), knn_frags)


def make_masks_exclusive(renderer, K, obj_ids, Rs, ts, masks):
  """datagen_utils.make_masks_exclusive_tf: bool [N,h,w], every pixel in at most one mask (the
  last instance whose mask and rendering cover it)."""
  masks = np.asarray(masks)
  n, h, w = masks.shape
  O = max([int(o) for o in obj_ids] + [1])
  f = gt_fields(renderer, K, obj_ids, Rs, ts, (w, h), np.zeros((O, 1, 3)), np.ones((O, 1)),
                masks)
  inst = f['instance'].cpu().numpy()
  return inst[None] == np.arange(n).reshape(n, 1, 1)


def gt_label_map(renderer, K, obj_ids, Rs, ts, size, masks=None):
  """The ground-truth object label map i32 [h,w] (0 = background) of datagen.py:570-604: from
  the exclusive masks when the frame carries instance masks, else by nearest depth."""
  O = max([int(o) for o in obj_ids] + [1])
  f = gt_fields(renderer, K, obj_ids, Rs, ts, size, np.zeros((O, 1, 3)), np.ones((O, 1)), masks)
  return f['obj_label'].cpu().numpy()


class FragmentFieldGenerator(object):
  """datagen_utils.FragmentFieldGenerator over epos_gt_fields_knn: knn_frags nearest fragments
  per pixel, 1..min(num_frags, 4)."""

  def __init__(self, frag_centers, frag_sizes, renderer, knn_frags=1):
    self.frag_centers, self.frag_sizes = frag_centers, frag_sizes
    self.renderer = renderer
    self.centers, self.sizes = pool_fragments(frag_centers, frag_sizes)
    self.knn_frags = int(knn_frags)
    if self.knn_frags != knn_frags or not 1 <= self.knn_frags <= min(self.sizes.shape[1],
                                                                     MAX_KNN_FRAGS):
      raise EposError('knn_frags must be in 1..%d, got %r' % (
          min(self.sizes.shape[1], MAX_KNN_FRAGS), knn_frags))

  def construct_frag_fields(self, width, height, K, gt_obj_ids, gt_obj_Rs, gt_obj_trans,
                            gt_obj_masks=None, return_all=False):
    """-> (frag_ids i32 [h,w,k], frag_coords f32 [h,w,k,3], frag_weights f32 [h,w,k]) as
    construct_frag_fields_py returns them, k = knn_frags. gt_obj_Rs: rotations [N,3,3] or
    quaternions [N,4] (w, x, y, z). return_all: the whole dict of host arrays instead (label map, instances)."""
    for o in gt_obj_ids:
      if int(o) not in self.frag_centers:
        raise EposError('object %d has no fragments' % int(o))
    f = gt_fields(self.renderer, K, list(gt_obj_ids), gt_obj_Rs, gt_obj_trans,
                  (width, height), self.centers, self.sizes, gt_obj_masks, self.knn_frags)
    f = {k: v.cpu().numpy() for k, v in f.items()}
    if return_all:
      return f
    if self.knn_frags == 1:
      return (f['frag_label'][:, :, None], f['frag_loc'][:, :, None, :],
              f['frag_weight'][:, :, None])
    return f['frag_label'], f['frag_loc'], f['frag_weight']
