"""Numpy restatement of the evaluation reductions (csrc/eval.hip; include/epos_hip.h,
"Evaluation"), written from that description: plain loops, no shared code with the package."""
import numpy as np


def confusion(gt, pred, num_cls, ignore):
  """(cm i64 [num_cls,num_cls] with row = ground truth, bad): pixels whose ground truth equals
  `ignore` are skipped first; a remaining pixel with either label outside 0..num_cls-1 counts
  in `bad` and not in cm."""
  cm = np.zeros((num_cls, num_cls), np.int64)
  bad = 0
  for g, q in zip(np.asarray(gt).reshape(-1).tolist(), np.asarray(pred).reshape(-1).tolist()):
    if g == ignore:
      continue
    if not (0 <= g < num_cls and 0 <= q < num_cls):
      bad += 1
      continue
    cm[g, q] += 1
  return cm, bad


def miou(cm):
  """(miou_all, miou_fg): IoU of a class = diagonal / (row sum + column sum - diagonal);
  classes with union 0 are left out; a missing background counts as IoU 1.0 in miou_all; no
  foreground class at all gives (0.0, 0.0)."""
  cm = np.asarray(cm)
  bg, fg = 1.0, []
  for c in range(cm.shape[0]):
    union = int(cm[c, :].sum()) + int(cm[:, c].sum()) - int(cm[c, c])
    if union == 0:
      continue
    iou = int(cm[c, c]) / float(union)
    if c == 0:
      bg = iou
    else:
      fg.append(iou)
  if not fg:
    return 0.0, 0.0
  return sum(fg + [bg]) / (len(fg) + 1), sum(fg) / len(fg)


def frag_hits(gt_obj, gt_frag, pred_obj, conf, num_objs, ignore):
  """counts i64 [num_objs+1,3] = (pixels, fragment hits, hits where pred_obj agrees) per
  ground-truth object; conf [P,num_objs,F]. The predicted fragment is the first maximum of the
  object's row with every NaN read as -inf. pred_obj None: column 2 stays 0."""
  gt_obj = np.asarray(gt_obj).reshape(-1)
  gt_frag = np.asarray(gt_frag).reshape(-1)
  conf = np.asarray(conf, np.float32).reshape(len(gt_obj), num_objs, -1)
  pred = None if pred_obj is None else np.asarray(pred_obj).reshape(-1)
  counts = np.zeros((num_objs + 1, 3), np.int64)
  for p in range(len(gt_obj)):
    o = int(gt_obj[p])
    if o == ignore or o < 1 or o > num_objs:
      continue
    row = conf[p, o - 1].copy()
    row[np.isnan(row)] = -np.inf
    best, arg = -np.inf, 0
    for f in range(len(row)):
      if row[f] > best:
        best, arg = row[f], f
    counts[o, 0] += 1
    if arg == gt_frag[p]:
      counts[o, 1] += 1
      if pred is not None and pred[p] == o:
        counts[o, 2] += 1
  return counts
