"""Evaluation of the segmentation and fragment heads on the device -- the work of the
reference's ``eval_utils.EvalHook`` (epos_lib/eval_utils.py) over the reductions of
csrc/eval.hip.

The reference downloads the ground-truth and the predicted label map of every image and counts
label pairs on the host (eval_utils.py:56-70); here both maps stay on the device, the confusion
matrix is an int64 device table that ``update`` adds to, and nothing is downloaded before
``confusion_matrix`` / ``miou`` / ``write``. mIoU follows eval_utils.py:89-107 to the letter.

The fragment counts (``frag_accuracy``) are THIS BUILD'S DEFINITION: the reference's hook lists
GT_FRAG_LABEL and PRED_FRAG_CONF among its tensors commented out and defines no fragment
metric (include/epos_hip.h, "Evaluation"; DESIGN.md, "Evaluation").

There is no CPU fallback: without the library or a device SegmentationEval raises EposError.
"""
import json
import os

import numpy as np

from epos_amd import _call as C
from epos_amd import _lib
from epos_amd._lib import EposError

TAG_MIOU_ALL = 'eval/obj_cls_miou_all'       # eval_utils.py:110
TAG_MIOU_FG = 'eval/obj_cls_miou_fg'         # eval_utils.py:113
TAG_FRAG_ACC = 'eval/frag_acc'               # this build
TAG_FRAG_ACC_SEG = 'eval/frag_acc_seg'
LAST_EVALUATION = 'last_evaluation.json'


def miou_from_confusion(cm):
  """(miou_all, miou_fg) of a confusion matrix (row = ground truth), eval_utils.py:89-107: the
  IoU of a class is diagonal / (row sum + column sum - diagonal); classes with an empty union
  are left out; the background IoU counts as 1.0 when class 0 is absent; both values are 0.0
  when no foreground class is present."""
  cm = np.asarray(cm, np.int64)
  inter = np.diag(cm)
  union = cm.sum(axis=1) + cm.sum(axis=0) - inter
  bg_iou = inter[0] / float(union[0]) if union[0] > 0 else 1.0
  fg = [inter[c] / float(union[c]) for c in range(1, len(cm)) if union[c] > 0]
  if not fg:
    return 0.0, 0.0
  return float(np.mean(fg + [bg_iou])), float(np.mean(fg))


def skip_reason(last_evaluation, checkpoint_path, now, interval_secs):
  """scripts/eval.py:74-92 as a function: None to evaluate, else the reference's log message.
  last_evaluation: the text of last_evaluation.json, or None when the file does not exist."""
  if last_evaluation is None:
    return None
  info = json.loads(last_evaluation)
  if checkpoint_path == info['checkpoint_path']:
    return 'Skipping evaluation (checkpoint {} has been evaluated).'.format(checkpoint_path)
  since = now - info['time']
  if since < interval_secs:
    return 'Skipping evaluation (only {} s from the last evaluation).'.format(since)
  return None


def format_table(cm):
  """The confusion matrix as a plain aligned table: a header row of predicted classes, one row
  per ground-truth class behind its index."""
  cm = np.asarray(cm)
  n = len(cm)
  width = max(len(str(int(v))) for v in list(cm.reshape(-1)) + [n]) + 1
  rows = [' ' * width + ''.join('%*d' % (width, c) for c in range(n))]
  for r in range(n):
    rows.append('%*d' % (width, r) + ''.join('%*d' % (width, int(v)) for v in cm[r]))
  return '\n'.join(rows) + '\n'


class SegmentationEval(object):
  """Device-resident evaluation state: cm i64 [O+1,O+1] (row = ground truth), bad i64 [1]
  (labels outside 0..O, see epos_eval_confusion) and, with num_frags, frag_counts i64 [O+1,3]
  (pixels, fragment hits, hits where the object label agrees too)."""

  def __init__(self, num_objs, ignore_label=255, device=None, num_frags=None):
    import torch
    C.need_device(None, 'evaluation needs a HIP device (there is no CPU fallback)')
    self.lib = _lib.load()
    self.device = torch.device(device if device is not None else 'cuda:0')
    self.num_objs, self.num_cls = int(num_objs), int(num_objs) + 1
    self.ignore_label = int(ignore_label)
    self.num_frags = None if num_frags is None else int(num_frags)
    self.cm = torch.zeros((self.num_cls, self.num_cls), dtype=torch.int64, device=self.device)
    self.bad = torch.zeros((1,), dtype=torch.int64, device=self.device)
    self.frag_counts = torch.zeros((self.num_cls, 3), dtype=torch.int64, device=self.device)

  def update(self, gt_obj_label, pred_obj_label, gt_frag_label=None, pred_frag_conf=None):
    """Adds one batch: gt_obj_label i32 and pred_obj_label i64 of one (any) batch shape, and
    for the fragment counts gt_frag_label i32 of that shape and pred_frag_conf f32 [..., O, F].
    Enqueues on the current stream; does not synchronise."""
    import torch
    def flat(t, dtype, numel, what):
      return C.flat(t, self.device, dtype, numel, what, 'the evaluation')

    gt = flat(gt_obj_label, torch.int32, None, 'gt_obj_label')
    P = gt.numel()
    pred = flat(pred_obj_label, torch.int64, P, 'pred_obj_label')
    with C.launch(self.device) as q:
      q.keep(gt, pred)                  # contiguous copies made here outlive this call
      _lib.check(self.lib.epos_eval_confusion(
          C.ptr(gt), C.ptr(pred), P, self.num_cls, self.ignore_label, C.ptr(self.cm),
          C.ptr(self.bad), q.handle), 'epos_eval_confusion')
      if gt_frag_label is not None or pred_frag_conf is not None:
        if self.num_frags is None or gt_frag_label is None or pred_frag_conf is None:
          raise ValueError('fragment counts need num_frags, gt_frag_label and pred_frag_conf')
        gf = flat(gt_frag_label, torch.int32, P, 'gt_frag_label')
        conf = flat(pred_frag_conf, torch.float32, P * self.num_objs * self.num_frags,
                    'pred_frag_conf')
        q.keep(gf, conf)
        _lib.check(self.lib.epos_eval_frag_hits(
            C.ptr(gt), C.ptr(gf), C.ptr(pred), C.ptr(conf), P, self.num_objs, self.num_frags,
            self.ignore_label, C.ptr(self.frag_counts), q.handle), 'epos_eval_frag_hits')

  def confusion_matrix(self):
    """The matrix as a host int64 array (synchronises). Raises EposError when a label outside
    0..num_objs was met, where the reference raises IndexError (eval_utils.py:70)."""
    bad = int(self.bad.cpu()[0])
    if bad:
      raise EposError('%d pixel(s) carry a ground-truth or predicted label outside 0..%d' % (
          bad, self.num_objs))
    return self.cm.cpu().numpy()

  def miou(self):
    return miou_from_confusion(self.confusion_matrix())

  def frag_accuracy(self):
    """{'per_object': {obj_id: (pixels, hits, hits_seg)}, 'frag_acc': hits / pixels,
    'frag_acc_seg': hits_seg / pixels} pooled over the objects (0.0 without pixels)."""
    counts = self.frag_counts.cpu().numpy()
    per = {o: tuple(int(v) for v in counts[o]) for o in range(1, self.num_cls)}
    pixels, hits, hits_seg = (int(counts[1:, k].sum()) for k in range(3))
    return {'per_object': per,
            'frag_acc': hits / float(pixels) if pixels else 0.0,
            'frag_acc_seg': hits_seg / float(pixels) if pixels else 0.0}

  def write(self, log_dir, global_step):
    """eval_utils.py:78-115: cm_<step>.txt, the scalar summaries as a TensorBoard event file,
    and metrics_<step>.json. The table is plain aligned text, not the psql frame tabulate
    draws for the reference: the numbers are the contract. Returns the metrics dict."""
    from epos_amd import tf_events
    cm = self.confusion_matrix()
    miou_all, miou_fg = miou_from_confusion(cm)
    os.makedirs(log_dir, exist_ok=True)
    with open(os.path.join(log_dir, 'cm_{}.txt'.format(global_step)), 'w') as f:
      f.write(format_table(cm))
    scalars = [(TAG_MIOU_ALL, miou_all), (TAG_MIOU_FG, miou_fg)]
    metrics = {'global_step': int(global_step), 'miou_all': miou_all, 'miou_fg': miou_fg,
               'confusion_matrix': cm.tolist()}
    if self.num_frags is not None:
      fa = self.frag_accuracy()
      scalars += [(TAG_FRAG_ACC, fa['frag_acc']), (TAG_FRAG_ACC_SEG, fa['frag_acc_seg'])]
      metrics.update(frag_acc=fa['frag_acc'], frag_acc_seg=fa['frag_acc_seg'],
                     frag_counts={str(o): list(v) for o, v in fa['per_object'].items()})
    with open(os.path.join(log_dir, 'metrics_{}.json'.format(global_step)), 'w') as f:
      json.dump(metrics, f)
    metrics['event_file'] = tf_events.write_scalars(log_dir, scalars, int(global_step))
    return metrics


def output_K(K, input_size, output_size):
  """The camera of the output maps (datagen.py:482-488): K scaled by output / input size."""
  (w, h), (ow, oh) = input_size, output_size
  sy, sx = h / float(oh), w / float(ow)
  return np.array([[K[0, 0] / sx, 0.0, K[0, 2] / sx],
                   [0.0, K[1, 1] / sy, K[1, 2] / sy], [0.0, 0.0, 1.0]])


def relabels_background(dataset_name, image_path):
  """datagen.py:606-614: T-LESS training images of the PrimeSense sensor show the objects on a
  black background that is not annotated, so label 0 becomes the ignore label there."""
  return dataset_name == 'tless' and 'tless/train_primesense' in (image_path or '')


def gt_fields_device(renderer, frame, output_size, frag_pool, counts, input_size=None,
                     allow_empty=True, knn_frags=1):
  """render.gt_fields of one frame's ground truth at output_size = (ow, oh), with the output
  camera, from the instance masks when the frame carries them (by nearest depth otherwise).
  Only the instances whose object the renderer holds and for which counts(obj_id) is true
  take part. frag_pool: (centers [O,F,3], sizes [O,F]) of render.pool_fragments. input_size =
  (w, h) of the frame's pixels (default: four times the output, the decoder stride). Without
  such an instance the fields are those of an empty scene, or None with allow_empty=False.
  knn_frags: the fragments per pixel, as render.gt_fields_device takes it."""
  from epos_amd import render
  centers, sizes = frag_pool
  gi = [i for i, p in enumerate(frame.gt_poses or [])
        if renderer.has_object(p['obj_id']) and counts(p['obj_id'])]
  gt = [frame.gt_poses[i] for i in gi]
  if not gt and not allow_empty:
    return None
  ow, oh = output_size
  if input_size is None:
    input_size = (4 * ow, 4 * oh)
  masks = frame.gt_masks((ow, oh)) if gt else None
  if masks is not None:
    if len(masks) != len(frame.gt_poses):
      raise ValueError('frame %s/%s: %d instance masks for %d ground-truth poses' % (
          frame.scene_id, frame.im_id, len(masks), len(frame.gt_poses)))
    masks = masks[gi]
  return render.gt_fields(
      renderer, output_K(frame.K, input_size, output_size), [p['obj_id'] for p in gt],
      np.stack([p['R'] for p in gt]) if gt else np.zeros((0, 3, 3)),
      np.stack([np.asarray(p['t']).reshape(3) for p in gt]) if gt else np.zeros((0, 3)),
      (ow, oh), centers, sizes, masks, knn_frags)


def gt_maps_device(renderer, frame, output_size, frag_pool, dataset_name=None, input_size=None,
                   ignore_label=255):
  """The ground-truth maps of one frame, left on the device: (obj_label, frag_label), i32
  [oh,ow] each, at output_size = (ow, oh) -- gt_fields_device over the instances of the
  objects 1..O of the fragment pool, plus the background rule of relabels_background."""
  import torch
  O = frag_pool[1].shape[0]
  f = gt_fields_device(renderer, frame, output_size, frag_pool, lambda o: 1 <= o <= O,
                       input_size)
  obj_label = f['obj_label']
  if relabels_background(dataset_name, frame.image_path):
    obj_label = torch.where(obj_label == 0, torch.full_like(obj_label, int(ignore_label)),
                            obj_label)
  return obj_label, f['frag_label']


def gt_loss_fields_device(renderer, frame, output_size, frag_pool, dataset_name=None,
                          input_size=None, ignore_label=255, knn_frags=1):
  """All four ground-truth maps of one frame, left on the device, as epos_amd/loss.py takes
  them: {obj_label i32 [oh,ow], frag_label i32 [oh,ow], frag_loc f32 [oh,ow,3], frag_weight
  f32 [oh,ow]} -- the fields gt_maps_device is built on (one assigned fragment per pixel), with
  the same background rule of relabels_background. With knn_frags = k > 1 the three fragment
  fields carry the k nearest fragments: [oh,ow,k], [oh,ow,k,3], [oh,ow,k]."""
  import torch
  O = frag_pool[1].shape[0]
  f = gt_fields_device(renderer, frame, output_size, frag_pool, lambda o: 1 <= o <= O,
                       input_size, knn_frags=knn_frags)
  obj_label = f['obj_label']
  if relabels_background(dataset_name, frame.image_path):
    obj_label = torch.where(obj_label == 0, torch.full_like(obj_label, int(ignore_label)),
                            obj_label)
  return {'obj_label': obj_label, 'frag_label': f['frag_label'], 'frag_loc': f['frag_loc'],
          'frag_weight': f['frag_weight']}
