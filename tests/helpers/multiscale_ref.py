"""numpy / torch statement of multi-scale inference (model.py:515-626) for the tests:
the bilinear resize (align_corners=True) in TF's arithmetic order, the max / mean merge, and
the composite `oracle/net_ref.py` per scale + resize + merge + predict's softmaxes.

In float32 the resize and the merge are the very operations epos_resize_merge_f32 performs
(scale = (in-1)/(out-1) as a float, f = o*scale, lo = floor(f), hi = min(ceil(f), in-1),
top = tl + (tr-tl)*lx, top + (bot-top)*ly, no fused multiply-add; max, or a sum in source
order divided by S), so the kernel is held to them bit for bit. In float64 (the dtype of the
input arrays) the same statement serves the emulated-bf16 comparison.
"""
import numpy as np
import torch

from oracle import net_ref

HEADS = ('pred_obj_conf', 'pred_frag_conf', 'pred_frag_loc')


def scale_dimension(dim, scale):
  """model.py:100-114."""
  return int((float(dim) - 1.0) * scale + 1.0)


def merged_size(h, w, pyramid):
  s = max(1.0, max(pyramid)) / 4
  return scale_dimension(h, s), scale_dimension(w, s)


def _coords(n_in, n_out, dt):
  sc = dt(n_in - 1) / dt(n_out - 1) if n_out > 1 else dt(0)
  f = np.arange(n_out).astype(dt) * sc
  lo = np.minimum(np.floor(f).astype(np.int64), n_in - 1)
  hi = np.minimum(np.ceil(f).astype(np.int64), n_in - 1)
  return lo, hi, (f - lo.astype(dt)).astype(dt)


def resize(x, ho, wo):
  """x [B, Hi, Wi, C] (float32 or float64) -> [B, ho, wo, C] in x's dtype."""
  x = np.asarray(x)
  dt = x.dtype.type
  y0, y1, ly = _coords(x.shape[1], ho, dt)
  x0, x1, lx = _coords(x.shape[2], wo, dt)
  lx = lx[None, None, :, None]
  ly = ly[None, :, None, None]
  tl, tr = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
  bl, br = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
  top = tl + (tr - tl) * lx
  bot = bl + (br - bl) * lx
  return top + (bot - top) * ly


def resize_merge(srcs, ho, wo, merge):
  """merge 'max' | 'avg' of the resized sources, in source order."""
  outs = [resize(s, ho, wo) for s in srcs]
  acc = outs[0]
  for o in outs[1:]:
    acc = np.maximum(acc, o) if merge == 'max' else acc + o
  if merge == 'avg' and len(outs) > 1:
    acc = acc / acc.dtype.type(len(outs))
  return acc


def merged_scales(pyramid):
  """The scales behind the reference's merge entries: its per-scale dict is keyed by
  'logits_%.2f' % scale (model.py:603-606); a later scale that prints alike replaces the
  earlier one's logits at the earlier one's position."""
  entries = {}
  for s in pyramid:
    entries['%.2f' % s] = s
  return list(entries.values())


def logits(img, wts, num_objs, num_frags, pyramid, merge='max', predict_fn=None, **kw):
  """The merged NHWC logits {head: [B, Lh, Lw, ch]} of multi_scale_logits: `predict_fn`
  (net_ref.predict by default) at every merged scale on the float32 resized image. A scale
  != 1.0 gets crop_size = [scaled_height, scaled_width] (model.py:572,581), which the decoder
  reads as [width, height] (model.py:355-356): crop_size_wh=(h_s, w_s) here."""
  predict_fn = predict_fn or net_ref.predict
  img = np.asarray(img, np.float32)
  h, w = img.shape[1:3]
  per = []
  for s in merged_scales(pyramid):
    if s == 1.0:
      per.append(predict_fn(img, wts, num_objs=num_objs, num_frags=num_frags,
                            **kw)['_logits'])
      continue
    hs, ws = scale_dimension(h, s), scale_dimension(w, s)
    x = resize(img, hs, ws)
    per.append(predict_fn(x, wts, num_objs=num_objs, num_frags=num_frags,
                          crop_size_wh=(hs, ws), **kw)['_logits'])
  lh, lw = merged_size(h, w, pyramid)
  return {k: resize_merge([p[k] for p in per], lh, lw, merge) for k in HEADS}


def predict(img, wts, num_objs, num_frags, pyramid, merge='max', predict_fn=None, **kw):
  """model.py:629-687 on the merged logits: the dict of net_ref.predict."""
  lg = logits(img, wts, num_objs, num_frags, pyramid, merge, predict_fn, **kw)
  b, h, w = lg['pred_obj_conf'].shape[:3]
  obj = torch.from_numpy(lg['pred_obj_conf'])
  frag = torch.from_numpy(lg['pred_frag_conf']).reshape(b, h, w, num_objs, num_frags)
  obj_conf = torch.softmax(obj, dim=-1)
  return {
      'pred_obj_conf': obj_conf.numpy(),
      'pred_obj_label': torch.argmax(obj_conf, dim=3).numpy(),
      'pred_frag_conf': torch.softmax(frag, dim=-1).numpy(),
      'pred_frag_loc': lg['pred_frag_loc'].reshape(b, h, w, num_objs, num_frags, 3),
      '_logits': lg,
  }
