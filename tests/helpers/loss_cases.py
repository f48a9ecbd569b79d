"""Seeded inputs for the loss tests: logits of the three heads and ground-truth fields with
background, several objects, an ignore band and, on request, images without foreground."""
import numpy as np

IGNORE = 255


def make_case(B, P, O, F, seed, empty_images=(), ignore_band=True):
  """dict of numpy arrays: obj_logits f32 [B,P,O+1], frag_logits f32 [B,P,O,F], frag_loc f32
  [B,P,O,F,3], gt_obj i32 [B,P], gt_frag i32 [B,P], gt_loc f32 [B,P,3], gt_weight f32 [B,P].
  The pixels run through background and every object in runs of uneven length; the first
  eighth of every image (at least one pixel when P >= 4) carries the ignore label; the images
  of `empty_images` are entirely background. Background pixels carry fragment fields that the
  rules must not read as they are: label -1, weight 0."""
  rng = np.random.RandomState(seed)
  c = {'obj_logits': (4.0 * rng.randn(B, P, O + 1)).astype(np.float32),
       'frag_logits': (4.0 * rng.randn(B, P, O, F)).astype(np.float32),
       'frag_loc': (1.5 * rng.randn(B, P, O, F, 3)).astype(np.float32),
       'gt_loc': (1.5 * rng.randn(B, P, 3)).astype(np.float32)}
  gt_obj = np.zeros((B, P), np.int32)
  for b in range(B):
    p = 0
    while p < P:
      run = int(rng.randint(1, 8))
      gt_obj[b, p:p + run] = rng.randint(0, O + 1)
      p += run
    if P >= 2 and O >= 2:                      # two objects at least, whatever the draw
      gt_obj[b, P - 1], gt_obj[b, P - 2] = 1, 2
    elif P >= 1:
      gt_obj[b, P - 1] = 1
    if ignore_band and P >= 4:
      gt_obj[b, :max(1, P // 8)] = IGNORE
  for b in empty_images:
    gt_obj[b] = 0
  fg = (gt_obj >= 1) & (gt_obj <= O)
  c['gt_obj'] = gt_obj
  c['gt_frag'] = np.where(fg, rng.randint(0, F, (B, P)), -1).astype(np.int32)
  c['gt_weight'] = np.where(fg, rng.uniform(0.25, 2.0, (B, P)), 0.0).astype(np.float32)
  return c


def ref_terms(loss_ref, c, share, ignore=IGNORE):
  return loss_ref.terms(c['obj_logits'], c['frag_logits'], c['frag_loc'], c['gt_obj'],
                        c['gt_frag'], c['gt_loc'], c['gt_weight'], ignore, share)
