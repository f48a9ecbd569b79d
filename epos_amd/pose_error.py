"""Pose errors of estimated against ground-truth poses -- MSSD, MSPD, ADD and ADI on the device
(csrc/pose_error.hip), rotation / translation errors, and the matching and recalls of the
BOP'19 localisation task on the host.

The reference leaves pose scoring to ``bop_toolkit`` (an empty submodule there). The errors
here are THIS BUILD'S DEFINITIONS, written out in include/epos_hip.h, "Pose errors": they
follow the published BOP'19 formulas, parity with bop_toolkit's numbers is unpinned, and
tests/helpers/pose_error_ref.py restates them in numpy, bit for bit.

There is no CPU fallback: without the library or a device PoseErrorEval raises EposError. The
symmetry sets, ``match`` and ``recalls`` are plain numpy and need neither.
"""
import ctypes
import json
import math
import os

import numpy as np

from epos_amd import _call as C
from epos_amd import _lib

MAX_SYM_DISC_STEP = 0.01
MSSD_FACTORS = tuple(0.05 * k for k in range(1, 11))     # x object diameter
MSPD_FACTORS = tuple(5.0 * k for k in range(1, 11))      # x image width / 640, pixels
ADD_FACTOR = 0.1                                         # x object diameter
ERROR_NAMES = ('mssd', 'mspd', 'add', 'adi', 're', 'te')

# EposPosePair as a numpy record (240 bytes)
PAIR_DTYPE = np.dtype([('vert_base', '<i4'), ('n_verts', '<i4'), ('sym_base', '<i4'),
                       ('n_sym', '<i4'), ('R_e', '<f8', (9,)), ('t_e', '<f8', (3,)),
                       ('R_g', '<f8', (9,)), ('t_g', '<f8', (3,)), ('cam', '<f8', (4,))])
assert PAIR_DTYPE.itemsize == ctypes.sizeof(_lib.PosePair)


def load_models_info(path):
  """models_info.json -> {obj_id (int): info dict}."""
  with open(path) as f:
    return {int(k): v for k, v in json.load(f).items()}


def models_info_path(datasets_path, dataset, model_type='eval'):
  folder = 'models' if model_type is None else 'models_' + model_type
  return os.path.join(datasets_path, dataset, folder, 'models_info.json')


def axis_rotation(angle, axis):
  """Rotation by `angle` about the direction `axis` (Rodrigues); angle 0 is exactly I."""
  a = np.asarray(axis, np.float64).reshape(3)
  a = a / np.linalg.norm(a)
  S = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
  return np.eye(3) + math.sin(angle) * S + (1.0 - math.cos(angle)) * S.dot(S)


def symmetry_transformations(model_info, max_sym_disc_step=MAX_SYM_DISC_STEP):
  """The symmetry set of an object as f64 [n, 12] (R row-major, then t), from the
  'symmetries_discrete' (lists of 16 numbers, row-major 4x4) and 'symmetries_continuous'
  ([{axis, offset}]) entries of its models_info record; include/epos_hip.h, "Pose errors".
  Element 0 is the identity. The rotation i = 0 of a continuous symmetry is included on
  purpose, so that the set holds the discrete symmetries themselves."""
  disc = [(np.eye(3), np.zeros(3))]
  for s in model_info.get('symmetries_discrete', []) or []:
    m = np.asarray(s, np.float64).reshape(4, 4)
    disc.append((m[:3, :3].copy(), m[:3, 3].copy()))
  cont = []
  for s in model_info.get('symmetries_continuous', []) or []:
    offset = np.asarray(s['offset'], np.float64).reshape(3)
    n = int(math.ceil(math.pi / max_sym_disc_step))
    for i in range(n):
      R = axis_rotation(i * 2.0 * math.pi / n, s['axis'])
      cont.append((R, offset - R.dot(offset)))
  if cont:
    out = [(Rc.dot(Rd), Rc.dot(td) + tc) for Rc, tc in cont for Rd, td in disc]
  else:
    out = disc
  return np.stack([np.concatenate([R.reshape(9), t]) for R, t in out])


def rotation_error(R_e, R_g):
  """re = arccos(clamp((tr(R_e R_g^T) - 1) / 2, -1, 1)), radians."""
  tr = float(np.sum(np.asarray(R_e, np.float64).reshape(9) *
                    np.asarray(R_g, np.float64).reshape(9)))
  return math.acos(min(1.0, max(-1.0, (tr - 1.0) / 2.0)))


def translation_error(t_e, t_g):
  d = np.asarray(t_g, np.float64).reshape(3) - np.asarray(t_e, np.float64).reshape(3)
  return float(np.sqrt(np.sum(d * d)))


class PoseErrorEval(object):
  """The vertices of ``models`` ({obj_id: {'pts': [V,3]}}, as ply.load_models returns them) and
  the symmetry sets of ``models_info`` ({obj_id: record}), pooled on the device once."""

  def __init__(self, models, models_info, device=None, max_sym_disc_step=MAX_SYM_DISC_STEP,
               chunk_pairs=1 << 16):
    import torch
    C.need_device(None, 'pose errors need a HIP device (there is no CPU fallback)')
    self.lib = _lib.load()
    self.device = torch.device(device if device is not None else 'cuda:0')
    self.chunk_pairs = int(chunk_pairs)
    self.objects = {}          # obj_id -> (vert_base, n_verts, sym_base, n_sym)
    self.diameters = {}
    verts, syms = [], []
    nv = ns = 0
    for o in sorted(models):
      pts = np.ascontiguousarray(models[o]['pts'], np.float64).reshape(-1, 3)
      info = models_info.get(o, {})
      sym = symmetry_transformations(info, max_sym_disc_step)
      if not len(pts):
        raise ValueError('object %d has no vertices' % o)
      self.objects[o] = (nv, len(pts), ns, len(sym))
      if 'diameter' in info:
        self.diameters[o] = float(info['diameter'])
      verts.append(pts)
      syms.append(sym)
      nv += len(pts)
      ns += len(sym)
    if not verts:
      raise ValueError('no object models')
    if nv >= 2 ** 31 or ns >= 2 ** 31:
      raise ValueError('the pooled models exceed 2^31 vertices or symmetries')
    self.n_verts_total, self.n_syms_total = nv, ns
    self.verts = torch.from_numpy(np.concatenate(verts)).to(self.device)
    self.syms = torch.from_numpy(np.concatenate(syms)).to(self.device)

  def n_sym(self, obj_id):
    return self.objects[obj_id][3]

  def table(self, pairs):
    """The EposPosePair records of `pairs` (PAIR_DTYPE) and the mask of the finite ones."""
    n = len(pairs)
    tab = np.zeros(n, PAIR_DTYPE)
    finite = np.ones(n, bool)
    for i, p in enumerate(pairs):
      tab[i]['vert_base'], tab[i]['n_verts'], tab[i]['sym_base'], tab[i]['n_sym'] = \
          self.objects[int(p['obj_id'])]
      K = np.asarray(p['K'], np.float64).reshape(3, 3)
      cam = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
      vals = [np.asarray(p[k], np.float64).reshape(-1) for k in ('R_e', 't_e', 'R_g', 't_g')]
      finite[i] = all(np.isfinite(v).all() for v in vals) and np.isfinite(cam).all()
      tab[i]['R_e'], tab[i]['t_e'], tab[i]['R_g'], tab[i]['t_g'] = vals
      tab[i]['cam'] = cam
    return tab, finite

  def staging(self, tab):
    """(host, dev, err) for a record table: the records in pinned host memory, the device
    buffer the launcher copies a chunk of them into, and the f64 [n, 4] result (nan)."""
    import torch
    n, size = len(tab), PAIR_DTYPE.itemsize
    host = torch.empty((n * size,), dtype=torch.uint8).pin_memory()
    host.numpy()[:] = np.ascontiguousarray(tab).view(np.uint8).reshape(-1)
    dev = torch.empty((min(n, self.chunk_pairs) * size,), dtype=torch.uint8, device=self.device)
    err = torch.full((n, 4), float('nan'), dtype=torch.float64, device=self.device)
    return host, dev, err

  def enqueue(self, host, dev, err, want_adi=True):
    """One launcher call per chunk_pairs records on the current stream; nothing is awaited, so
    `host` and `dev` stay alive until the stream has been synchronised."""
    n, size = err.shape[0], PAIR_DTYPE.itemsize
    with C.launch(self.device) as q:
      for i0 in range(0, n, self.chunk_pairs):
        m = min(self.chunk_pairs, n - i0)
        _lib.check(self.lib.epos_pose_errors_f64(
            C.ptr(self.verts), self.n_verts_total, C.ptr(self.syms), self.n_syms_total,
            C.ptr(host, i0 * size), C.ptr(dev), m, int(bool(want_adi)), C.ptr(err, i0 * 4),
            q.handle), 'epos_pose_errors_f64')

  def device_errors(self, tab, want_adi=True):
    """f64 [n, 4] (mssd, mspd, add, adi; adi = nan without want_adi) of a record table whose
    every pair is finite: one launcher call per chunk_pairs records, one download."""
    if len(tab) == 0:
      return np.zeros((0, 4))
    host, dev, err = self.staging(tab)
    self.enqueue(host, dev, err, want_adi)
    return err.cpu().numpy()          # synchronises: `host` and `dev` are done with

  def errors(self, pairs, want_adi=True):
    """pairs: [{obj_id, R_e, t_e, R_g, t_g, K}] -> f64 [n, 6]: mssd, mspd, add, adi (mm, px,
    mm, mm), re (radians), te (mm). A pair with a non-finite number in either pose or in K
    never reaches the device and gets +inf everywhere. Without want_adi column 3 is nan."""
    tab, finite = self.table(pairs)
    out = np.full((len(pairs), 6), np.inf)
    idx = np.nonzero(finite)[0]
    out[idx, :4] = self.device_errors(tab[idx], want_adi)
    for i in idx:
      out[i, 4] = rotation_error(tab[i]['R_e'], tab[i]['R_g'])
      out[i, 5] = translation_error(tab[i]['t_e'], tab[i]['t_g'])
    return out


# ------------------------------------------------------------------ matching and recall ---
def match(scores, err_matrix, threshold):
  """Greedy matching of one (image, object): err_matrix [n_est, n_gt]. The estimates are
  walked by descending score (ties keep their order); each takes the still unmatched ground
  truth with the smallest error STRICTLY below the threshold (ties: the lowest index).
  Returns i64 [n_est]: the matched ground-truth index, or -1."""
  err = np.asarray(err_matrix, np.float64)
  scores = np.asarray(scores, np.float64).reshape(-1)
  if err.ndim != 2 or err.shape[0] != len(scores):
    raise ValueError('err_matrix must be [n_est, n_gt]')
  out = np.full(len(scores), -1, np.int64)
  free = np.ones(err.shape[1], bool)
  for e in np.argsort(-scores, kind='stable'):
    cand = np.where(free & (err[e] < threshold), err[e], np.inf)
    if np.isfinite(cand).any():
      g = int(np.argmin(cand))
      out[e] = g
      free[g] = False
  return out


def thresholds(diameter, image_width):
  return {'mssd': [c * diameter for c in MSSD_FACTORS],
          'mspd': [c * (image_width / 640.0) for c in MSPD_FACTORS],
          'add': ADD_FACTOR * diameter}


def recalls(groups, diameters, n_syms, image_width):
  """groups: [{obj_id, scores [n_est], errors [n_est, n_gt, >=4]}], one per (image, object),
  already cut to the top estimates. Recall = true positives / ground-truth instances, pooled
  over the groups of an object ('per_object') and over all of them ('overall'):
    ar_mssd   mean recall over the thresholds c * diameter, c = 0.05 .. 0.50
    ar_mspd   mean recall over c * (image_width / 640) px, c = 5 .. 50
    add_s     recall at 0.1 * diameter of ADI for an object whose symmetry set has more than
              one element, of ADD otherwise
    mean_ar_mssd_mspd   (ar_mssd + ar_mspd) / 2 -- NOT BOP's AR, which also averages VSD."""
  objs = sorted(set(int(g['obj_id']) for g in groups))
  tp = {o: {'mssd': np.zeros(len(MSSD_FACTORS), np.int64),
            'mspd': np.zeros(len(MSPD_FACTORS), np.int64), 'add_s': 0} for o in objs}
  n_gt = dict.fromkeys(objs, 0)
  n_est = dict.fromkeys(objs, 0)
  for g in groups:
    o = int(g['obj_id'])
    err = np.asarray(g['errors'], np.float64)
    scores = np.asarray(g['scores'], np.float64).reshape(-1)
    if err.ndim != 3 or err.shape[0] != len(scores) or err.shape[2] < 4:
      raise ValueError('errors must be [n_est, n_gt, >=4], got %s for %d scores' % (
          err.shape, len(scores)))
    n_gt[o] += err.shape[1]
    n_est[o] += len(scores)
    if not len(scores) or not err.shape[1]:
      continue
    th = thresholds(diameters[o], image_width)
    for k, t in enumerate(th['mssd']):
      tp[o]['mssd'][k] += int((match(scores, err[:, :, 0], t) >= 0).sum())
    for k, t in enumerate(th['mspd']):
      tp[o]['mspd'][k] += int((match(scores, err[:, :, 1], t) >= 0).sum())
    col = 3 if n_syms[o] > 1 else 2
    tp[o]['add_s'] += int((match(scores, err[:, :, col], th['add']) >= 0).sum())

  def summary(ids):
    n = sum(n_gt[o] for o in ids)
    rec = lambda hits: float(hits) / n if n else 0.0      # noqa: E731
    r3 = [rec(sum(tp[o]['mssd'][k] for o in ids)) for k in range(len(MSSD_FACTORS))]
    r2 = [rec(sum(tp[o]['mspd'][k] for o in ids)) for k in range(len(MSPD_FACTORS))]
    ar3, ar2 = float(np.mean(r3)), float(np.mean(r2))
    return {'targets': int(n), 'estimates': int(sum(n_est[o] for o in ids)),
            'recall_mssd': r3, 'recall_mspd': r2, 'ar_mssd': ar3, 'ar_mspd': ar2,
            'mean_ar_mssd_mspd': (ar3 + ar2) / 2.0,
            'add_s_recall': rec(sum(tp[o]['add_s'] for o in ids))}
  per = {}
  for o in objs:
    per[o] = summary([o])
    per[o]['add_s_error'] = 'adi' if n_syms[o] > 1 else 'add'
  return {'per_object': per, 'overall': summary(objs)}
