"""The three training losses on the device -- the validation value of what the reference
trains on (epos_lib/loss.py:99-303, called from scripts/train.py:198-235): object
cross-entropy, fragment cross-entropy and the fragment-localisation Huber loss, over the
reduction of csrc/loss.hip (include/epos_hip.h, "Losses").

The losses are taken from the RAW logits (EposNet.forward_logits), never from probabilities,
and from ground-truth fields with one assigned fragment per pixel (render.gt_fields /
epos_gt_fields: the reference's gt_knn_frags = 1, train.py:82) or with the k nearest
(gt_knn_frags = k <= MAX_KNN: the fields carry a slot dimension and Batch reads k from their
shapes; include/epos_hip.h, "k nearest fragments"). The dense heads stay on the device; what
comes down is one row of (O+1) x 5 + 1 numbers per image.

``total_loss`` is the sum of the three weighted losses and has NO REGULARISATION TERM, unlike
the total of train.py:280 (tf.losses.get_total_loss adds the weight decay): it is a
validation value, comparable between checkpoints, not the number the trainer logs.

Parity with TensorFlow's numbers is unpinned: there is no TensorFlow to compare with. The
formulas are pinned to tests/helpers/loss_ref.py and, through it, to torch's cross_entropy and
huber_loss in fp64 (tests/test_loss_host.py; DESIGN.md, "Losses").

Gradients (csrc/loss_grad.hip; DESIGN.md, "Losses", "Gradients"): loss_values reduces the
tables to the batch's four values and the per-image gradient factors, loss_grads writes the
derivative with respect to the three logit tensors, and differentiable_losses puts both behind
a torch.autograd.Function, so that an optimiser and torch's own conv backward can fine-tune the
logits layers on EposNet.decoder_out. Pinned to tests/helpers/loss_grad_ref.py and, through it,
to torch's fp64 autograd; parity with TensorFlow's gradients is unpinned.
differentiable_losses_from_features is the same behind the logits layers: a function of the
features those layers read and of their six variables, whose backward is the input gradient
(csrc/heads_dgrad.hip) and the weight gradients (csrc/heads_wgrad.hip) of
epos_amd/heads_train.py; DESIGN.md, "Losses", "Input gradient".

There is no CPU fallback: without the library or a device this raises EposError.
"""
import json
import os

from epos_amd import _call as C
from epos_amd import _lib
from epos_amd._lib import EposError
from epos_amd import weights as W

NAMES = ('obj_cls_loss', 'frag_cls_loss', 'frag_loc_loss', 'total_loss')
TAGS = tuple('eval/' + n for n in NAMES)
GT_KEYS = ('obj_label', 'frag_label', 'frag_loc', 'frag_weight')
MAX_KNN = 4                                  # EPOS_LOSS_MAX_KNN


def check_knn(knn, num_frags=None):
  """knn as an int; ValueError unless 1 <= knn <= min(num_frags, MAX_KNN)."""
  k = int(knn)
  top = MAX_KNN if num_frags is None else min(MAX_KNN, int(num_frags))
  if k != knn or k < 1 or k > top:
    raise ValueError('gt_knn_frags must be in 1..%d (at most %d fragments per pixel, and no '
                     'more than num_frags), got %r' % (top, MAX_KNN, knn))
  return k


def gt_knn(gt):
  """The number of fragments per pixel a ground truth carries: frag_label with one more
  dimension than obj_label has it as its last dimension; the same number of dimensions is 1."""
  extra = gt['frag_label'].dim() - gt['obj_label'].dim()
  if extra == 0:
    return 1
  if extra != 1:
    raise ValueError('frag_label must have the dimensions of obj_label, or one more (the '
                     'fragments per pixel), got %s and %s' % (
                         tuple(gt['frag_label'].shape), tuple(gt['obj_label'].shape)))
  return int(gt['frag_label'].shape[-1])


def need_fp32(features):
  import torch
  if features.dtype != torch.float32:
    raise TypeError('features must be torch.float32, got %s (a bf16 decoder_out is not '
                    'supported: run the net with precision=\'fp32\')' % features.dtype)


HEADS = (W.PRED_OBJ_CONF, W.PRED_FRAG_CONF, W.PRED_FRAG_LOC)


def variable_names(head):
  """(weights, biases): the checkpoint variable names of a logits layer."""
  return W.trainable_variables(('logits/' + head,))


HEAD_VARIABLES = W.trainable_variables(W.LOGITS_LAYERS)


def _head_dicts(obj, frag, loc, gt_obj, gt_frag, gt_loc, gt_weight):
  """(logits, gt) as loss_terms takes them, from the seven tensors."""
  return (dict(zip(HEADS, (obj, frag, loc))),
          dict(zip(GT_KEYS, (gt_obj, gt_frag, gt_loc, gt_weight))))


class Batch(object):
  """A batch of logits and ground truth as the C entries take it: dev, B, P, O, F, n = B * P;
  shapes of the three logit tensors; ins = [obj rows, frag, loc, obj_label, frag_label, frag_loc,
  frag_weight] flattened, in ABI order, with ld the row stride of the first; scales and upstream
  flattened (or None); keep = what the launch keeps (_call.launch.keep); knn = the fragments
  per pixel, read from the shapes (gt_knn): frag_label [..., knn], frag_loc [..., knn, 3] and
  frag_weight [..., knn] against obj_label [...]."""

  def __init__(self, logits, gt, who, scales=None, upstream=None):
    import torch
    obj, frag, loc = (logits[k] for k in HEADS)
    C.need_device(obj, '%s a HIP device (there is no CPU fallback)' % who)
    dev = obj.device

    def flat(t, dtype, numel, what):
      return C.flat(t, dev, dtype, numel, what, 'the losses')
    if frag.dim() < 3 or obj.dim() < 2:
      raise ValueError('pred_frag_conf must be [..., O, F] and pred_obj_conf [..., O+1]')
    O, F = int(frag.shape[-2]), int(frag.shape[-1])
    if obj.shape[-1] != O + 1:
      raise ValueError('pred_obj_conf has %d channels, pred_frag_conf %d objects' % (
          obj.shape[-1], O))
    gt_obj = gt['obj_label']
    B = int(gt_obj.shape[0]) if gt_obj.dim() > 1 else 1
    n = gt_obj.numel()
    if B == 0 or n % B:
      raise ValueError('obj_label must be [B, ...] with B >= 1')
    if obj.dtype != torch.float32:
      raise TypeError('pred_obj_conf must be torch.float32, got %s' % obj.dtype)
    obj2, self.ld = C.rows(obj, O + 1)
    if obj2.shape[0] != n:
      raise ValueError('pred_obj_conf holds %d rows, expected %d' % (obj2.shape[0], n))
    self.dev, self.B, self.P, self.O, self.F, self.n = dev, B, n // B, O, F, n
    self.shapes = (obj.shape, frag.shape, loc.shape)
    knn = self.knn = gt_knn(gt)
    if knn != 1:                             # knn == 1: the checks and messages of flat alone
      check_knn(knn, F)
      want = tuple(gt['frag_label'].shape)
      if tuple(gt['frag_loc'].shape) != want + (3,) or tuple(gt['frag_weight'].shape) != want:
        raise ValueError('with frag_label %s, frag_loc must be %s and frag_weight %s, got %s '
                         'and %s' % (want, want + (3,), want, tuple(gt['frag_loc'].shape),
                                     tuple(gt['frag_weight'].shape)))
    self.ins = [obj2,
                flat(frag, torch.float32, n * O * F, 'pred_frag_conf'),
                flat(loc, torch.float32, n * O * F * 3, 'pred_frag_loc'),
                flat(gt_obj, torch.int32, n, 'obj_label'),
                flat(gt['frag_label'], torch.int32, n * knn, 'frag_label'),
                flat(gt['frag_loc'], torch.float32, n * knn * 3, 'frag_loc'),
                flat(gt['frag_weight'], torch.float32, n * knn, 'frag_weight')]
    self.scales = self.upstream = None
    if scales is not None:
      self.scales = flat(scales, torch.float64, B * 3, 'scales')
    if upstream is not None:
      self.upstream = flat(upstream, torch.float64, 4, 'upstream')
    self.keep = self.ins + [self.scales, self.upstream]

  def args(self, ignore_label):
    """The arguments every _knn entry shares: obj, ld_obj, frag, loc, the four ground-truth
    fields, B, P, O, F, ignore_label, knn."""
    i = [C.ptr(t) for t in self.ins]
    return (i[0], self.ld) + tuple(i[1:]) + (self.B, self.P, self.O, self.F, int(ignore_label),
                                             self.knn)

  def grad_args(self, ignore_label):
    """args, then scales and upstream (NULL without)."""
    return self.args(ignore_label) + (C.ptr(self.scales), C.ptr(self.upstream))


def loss_terms(logits, gt, ignore_label=255, out=None):
  """epos_loss_terms_knn over one batch. logits: the dict of EposNet.forward_logits --
  pred_obj_conf f32 [B,h,w,O+1], pred_frag_conf f32 [B,h,w,O,F], pred_frag_loc f32
  [B,h,w,O,F,3]; gt: {obj_label i32 [B,h,w], frag_label i32 [B,h,w], frag_loc f32 [B,h,w,3],
  frag_weight f32 [B,h,w]} (render.gt_fields per image, stacked), or with k fragments per
  pixel frag_label [B,h,w,k], frag_loc [B,h,w,k,3], frag_weight [B,h,w,k]. Returns (sums f64 [B,O+1,3],
  counts i64 [B,O+1,2], bad i64 [B]) on the device; `out` = three such tensors (rows of a
  larger table) to write into. Enqueues on the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  bt = Batch(logits, gt, 'the losses need')
  dev, B, P, O, F = bt.dev, bt.B, bt.P, bt.O, bt.F
  sums, counts, bad = (
      C.out(t, dev, dtype, shape, 'out: ' + what, flat=True) for t, dtype, shape, what in zip(
          out or (None, None, None), (torch.float64, torch.int64, torch.int64),
          ((B, O + 1, 3), (B, O + 1, 2), (B,)), ('sums', 'counts', 'bad')))
  nbytes = lib.epos_loss_workspace_bytes(B, P, O, F)
  _lib.check(nbytes, 'epos_loss_workspace_bytes')
  ws = C.workspace(None, dev, nbytes)
  with C.launch(dev) as q:
    q.keep(ws, *bt.keep)
    _lib.check(lib.epos_loss_terms_knn(
        *bt.args(ignore_label), C.ptr(ws), C.ptr(sums), C.ptr(counts), C.ptr(bad), q.handle),
               'epos_loss_terms_knn')
  return sums, counts, bad


def image_losses(sums, counts, weights, knn=1):
  """One image's losses as the reference's batch of one (loss.py:149,224-229,298-303), from
  its host rows sums [O+1,3] and counts [O+1,2]:
    obj_cls_loss  = w_obj * sum_g sums[g,0] / P -- over ALL P pixels, ignored ones included
                    (reduce_mean runs over the weighted vector)
    frag_cls_loss = w_cls * sum_{g>=1} sums[g,1] / n_fg
    frag_loc_loss = w_loc * sum_{g>=1} sums[g,2] / (3 n_fg)
  both fragment losses 0 when n_fg = 0; objects added in index order, the mean taken first and
  the weight applied last; total_loss = their sum, without a regularisation term. With knn
  fragments per pixel the two fragment means run over the n_fg * knn (pixel, fragment) rows."""
  w_obj, w_cls, w_loc = weights
  P = int(counts[:, 0].sum()) + int(counts[0, 1])
  n_fg = int(counts[1:, 0].sum()) * int(knn)
  s = [0.0, 0.0, 0.0]
  for g in range(sums.shape[0]):
    s[0] += float(sums[g, 0])
    if g >= 1:
      s[1] += float(sums[g, 1])
      s[2] += float(sums[g, 2])
  out = {'obj_cls_loss': w_obj * (s[0] / P),
         'frag_cls_loss': w_cls * (s[1] / n_fg) if n_fg else 0.0,
         'frag_loc_loss': w_loc * (s[2] / (3 * n_fg)) if n_fg else 0.0}
  out['total_loss'] = (out['obj_cls_loss'] + out['frag_cls_loss']) + out['frag_loc_loss']
  return out


def summarize(sums, counts, bad, weights, num_objs, knn=1):
  """LossEval.result on host tables sums f64 [N,O+1,3], counts i64 [N,O+1,2], bad i64 [N]; knn
  = the fragments per pixel the tables were taken with (they do not carry it). per_object keeps
  counting pixels."""
  import numpy as np
  n_bad = int(np.asarray(bad).sum())
  if n_bad:
    raise EposError(
        '%d pixel(s) carry an object label outside 0..%d, a fragment label outside the '
        'fragments, or a weight that is not a finite number > 0' % (n_bad, num_objs))
  if not np.isfinite(sums).all():
    raise EposError('Loss is inf or nan.')                       # train.py:281
  w_obj, w_cls, w_loc = weights
  N, O1 = sums.shape[0], sums.shape[1]
  knn = check_knn(knn)
  per_image = [image_losses(sums[i], counts[i], weights, knn) for i in range(N)]
  mean = {}
  for name in NAMES:
    acc = 0.0
    for r in per_image:
      acc += r[name]
    mean[name] = acc / N if N else 0.0
  tot = np.zeros((O1, 3), np.float64)
  n = np.zeros((O1,), np.int64)
  pixels = 0
  for i in range(N):                                   # image order
    tot += sums[i]
    n += counts[i, :, 0]
    pixels += int(counts[i, :, 0].sum()) + int(counts[i, 0, 1])
  n_fg = int(n[1:].sum()) * knn
  s = [0.0, 0.0, 0.0]
  for g in range(O1):
    s[0] += float(tot[g, 0])
    if g >= 1:
      s[1] += float(tot[g, 1])
      s[2] += float(tot[g, 2])
  pooled = {'obj_cls_loss': w_obj * (s[0] / pixels) if pixels else 0.0,
            'frag_cls_loss': w_cls * (s[1] / n_fg) if n_fg else 0.0,
            'frag_loc_loss': w_loc * (s[2] / (3 * n_fg)) if n_fg else 0.0}
  pooled['total_loss'] = ((pooled['obj_cls_loss'] + pooled['frag_cls_loss']) +
                          pooled['frag_loc_loss'])
  per_object = {}
  for g in range(1, O1):
    c = int(n[g])
    rows = c * knn
    per_object[g] = {'frag_cls_loss': w_cls * (float(tot[g, 1]) / rows) if c else 0.0,
                     'frag_loc_loss': w_loc * (float(tot[g, 2]) / (3 * rows)) if c else 0.0,
                     'pixels': c}
  return {'per_image': per_image, 'mean': mean, 'pooled': pooled, 'per_object': per_object}


class LossEval(object):
  """Device-resident loss tables, one row per image: sums f64 [N,O+1,3], counts i64
  [N,O+1,2], bad i64 [N]. The weight defaults are those of train.py:72-80. knn = the fragments
  per pixel of every ground truth passed to update (the reference's gt_knn_frags)."""

  def __init__(self, num_objs, num_frags, device=None, obj_cls_loss_weight=1.0,
               frag_cls_loss_weight=1.0, frag_loc_loss_weight=100.0, ignore_label=255, knn=1):
    import torch
    C.need_device(None, 'the losses need a HIP device (there is no CPU fallback)')
    _lib.load()
    self.device = torch.device(device if device is not None else 'cuda:0')
    self.num_objs, self.num_frags = int(num_objs), int(num_frags)
    self.knn = check_knn(knn, self.num_frags)
    self.weights = (float(obj_cls_loss_weight), float(frag_cls_loss_weight),
                    float(frag_loc_loss_weight))
    self.ignore_label = int(ignore_label)
    self.rows = 0
    self._alloc(16)

  def _alloc(self, capacity):
    import torch
    O1 = self.num_objs + 1
    new = (torch.empty((capacity, O1, 3), dtype=torch.float64, device=self.device),
           torch.empty((capacity, O1, 2), dtype=torch.int64, device=self.device),
           torch.empty((capacity,), dtype=torch.int64, device=self.device))
    if self.rows:
      for dst, src in zip(new, self.tables):
        dst[:self.rows].copy_(src[:self.rows])        # on the stream, no synchronisation
    self.tables = new

  def update(self, logits, gt_fields):
    """Appends one row per image of the batch: logits as EposNet.forward_logits returns them,
    gt_fields as loss_terms takes them. Enqueues on the current stream; no download, no
    synchronisation."""
    O, F = logits[W.PRED_FRAG_CONF].shape[-2:]
    if (int(O), int(F)) != (self.num_objs, self.num_frags):
      raise ValueError('logits of %d objects x %d fragments, expected %d x %d' % (
          O, F, self.num_objs, self.num_frags))
    if gt_knn(gt_fields) != self.knn:
      raise ValueError('ground truth with %d fragment(s) per pixel, expected %d' % (
          gt_knn(gt_fields), self.knn))
    B = int(gt_fields['obj_label'].shape[0])
    capacity = self.tables[2].shape[0]
    if self.rows + B > capacity:
      while self.rows + B > capacity:
        capacity *= 2
      self._alloc(capacity)
    r0, r1 = self.rows, self.rows + B
    loss_terms(logits, gt_fields, self.ignore_label, out=tuple(t[r0:r1] for t in self.tables))
    self.rows = r1

  def result(self):
    """Downloads the tables once (synchronises) and returns
      per_image   one {obj_cls_loss, frag_cls_loss, frag_loc_loss, total_loss} per image, in
                  the order of the updates (image_losses)
      mean        the mean over the images of each loss -- what the reference's summaries of a
                  batch-of-one evaluation average to
      pooled      dataset sums over dataset counts: an image without foreground does not pull
                  the fragment losses toward 0
      per_object  {obj_id: {frag_cls_loss, frag_loc_loss, pixels}}, pooled per object id
    total_loss has no regularisation term (see the module docstring). Raises EposError naming
    the count when a bad pixel was met, and EposError('Loss is inf or nan.') when a sum is not
    finite, as train.py:281 does."""
    import torch
    n, O1 = self.rows, self.num_objs + 1
    sums, counts, bad = self.tables
    packed = torch.cat([sums[:n].reshape(n, -1).view(torch.int64), counts[:n].reshape(n, -1),
                        bad[:n].reshape(n, 1)], dim=1).cpu().numpy()
    h_sums = packed[:, :3 * O1].copy().view('float64').reshape(n, O1, 3)
    h_counts = packed[:, 3 * O1:5 * O1].reshape(n, O1, 2)
    return summarize(h_sums, h_counts, packed[:, 5 * O1], self.weights, self.num_objs,
                     self.knn)

  def write(self, log_dir, global_step, image_keys=None):
    """losses_<step>.json -- mean, pooled, per_object, the weights, the number of images and
    per_image keyed by image_keys ('scene_id/im_id'; the row index without) -- and one
    TensorBoard event file with eval/obj_cls_loss, eval/frag_cls_loss, eval/frag_loc_loss and
    eval/total_loss (the means over the images). Returns the result dict."""
    from epos_amd import tf_events
    res = self.result()
    keys = [str(i) for i in range(self.rows)] if image_keys is None else list(image_keys)
    if len(keys) != self.rows or len(set(keys)) != len(keys):
      raise ValueError('image_keys must name each of the %d images once' % self.rows)
    os.makedirs(log_dir, exist_ok=True)
    doc = {'global_step': int(global_step), 'num_images': self.rows,
           'weights': dict(zip(('obj_cls_loss_weight', 'frag_cls_loss_weight',
                                'frag_loc_loss_weight'), self.weights)),
           'mean': res['mean'], 'pooled': res['pooled'],
           'per_object': {str(o): v for o, v in res['per_object'].items()},
           'per_image': dict(zip(keys, res['per_image']))}
    if self.knn != 1:                        # with one fragment per pixel: the file as before
      doc['gt_knn_frags'] = self.knn
    with open(os.path.join(log_dir, 'losses_{}.json'.format(global_step)), 'w') as f:
      json.dump(doc, f)
    res['event_file'] = tf_events.write_scalars(
        log_dir, [(t, res['mean'][k]) for t, k in zip(TAGS, NAMES)], int(global_step))
    return res


# ------------------------------------------------------------------ gradients ---
REDUCTIONS = {'mean': 0, 'pooled': 1}        # EPOS_LOSS_MEAN, EPOS_LOSS_POOLED


def loss_values(sums, counts, weights, reduction='mean', out=None, knn=1):
  """epos_loss_reduce_knn over the tables loss_terms wrote (device tensors sums f64 [B,O+1,3],
  counts i64 [B,O+1,2]): returns (values f64 [4], scales f64 [B,3]) on the device -- the
  batch's weighted obj_cls_loss, frag_cls_loss, frag_loc_loss and total_loss, bit-equal to
  summarize(...)['mean'] or ['pooled'], and the per-image factors loss_grads multiplies the
  per-pixel derivatives with. weights = (w_obj, w_cls, w_loc); `out` = two such tensors to
  write into; knn = the fragments per pixel loss_terms ran with (the tables do not carry it).
  Enqueues on the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  if reduction not in REDUCTIONS:
    raise ValueError("reduction must be 'mean' or 'pooled', got %r" % (reduction,))
  knn = check_knn(knn)
  C.need_device(sums, 'the losses need a HIP device (there is no CPU fallback)')
  dev = sums.device
  if sums.dim() != 3 or sums.shape[0] < 1 or sums.shape[2] != 3:
    raise ValueError('sums must be [B, O+1, 3] with B >= 1')
  B, O1 = int(sums.shape[0]), int(sums.shape[1])
  if out is None:
    out = (torch.empty((4,), dtype=torch.float64, device=dev),
           torch.empty((B, 3), dtype=torch.float64, device=dev))
  values, scales = out
  for t, dtype, numel, what in ((sums, torch.float64, B * O1 * 3, 'sums'),
                                (counts, torch.int64, B * O1 * 2, 'counts'),
                                (values, torch.float64, 4, 'values'),
                                (scales, torch.float64, B * 3, 'scales')):
    C.dense(t, dev, dtype, what, numel=numel)
  w_obj, w_cls, w_loc = (float(w) for w in weights)
  with C.launch(dev) as q:
    _lib.check(lib.epos_loss_reduce_knn(
        C.ptr(sums), C.ptr(counts), B, O1 - 1, w_obj, w_cls, w_loc, REDUCTIONS[reduction], knn,
        C.ptr(values), C.ptr(scales), q.handle), 'epos_loss_reduce_knn')
  return values, scales


def loss_grads(logits, gt, scales, upstream=None, ignore_label=255, need=(True, True, True),
               out=None):
  """epos_loss_grads_knn over one batch: the derivative of the losses with respect to the three
  logit tensors. logits and gt as loss_terms takes them; scales f64 [B,3] from loss_values;
  upstream f64 [4] on the device (the gradient arriving at loss_values' values; None = the
  total loss alone). Returns (d_obj, d_frag, d_loc), f32 tensors shaped like pred_obj_conf,
  pred_frag_conf and pred_frag_loc with EVERY element written, None where need[k] is false
  (that head is then neither read nor written). `out` = three tensors (or None) to write into;
  a d_obj whose rows lie a constant stride apart keeps its padding columns. Ignored and bad
  pixels get zero gradient. Enqueues on the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  bt = Batch(logits, gt, 'the losses need', scales, upstream)
  dev, O, shapes = bt.dev, bt.O, bt.shapes
  outs = list(out) if out is not None else [None, None, None]
  for k in range(3):
    if not need[k]:
      outs[k] = None
    elif outs[k] is None:
      outs[k] = torch.empty(shapes[k], dtype=torch.float32, device=dev)
    elif (outs[k].device != dev or outs[k].dtype != torch.float32 or
          outs[k].shape != shapes[k] or (k > 0 and not outs[k].is_contiguous())):
      raise ValueError('out[%d] must be a float32 tensor of shape %s on %s%s' % (
          k, tuple(shapes[k]), dev, ', contiguous' if k else ''))
  d_obj2, ld_d = None, O + 1
  if outs[0] is not None:
    d_obj2, ld_d = C.rows(outs[0], O + 1)
    if d_obj2.data_ptr() != outs[0].data_ptr():
      raise ValueError('out[0]: the rows of d_obj must lie a constant stride apart')
  with C.launch(dev) as q:
    q.keep(*bt.keep)
    _lib.check(lib.epos_loss_grads_knn(
        *bt.grad_args(ignore_label), C.ptr(d_obj2), ld_d, C.ptr(outs[1]), C.ptr(outs[2]),
        q.handle), 'epos_loss_grads_knn')
  return tuple(outs)


_function = None


def _losses_function():
  """The torch.autograd.Function behind differentiable_losses, defined at first use: this
  module imports without torch."""
  global _function
  if _function is not None:
    return _function
  import torch
  from torch.autograd.function import once_differentiable

  class EposLosses(torch.autograd.Function):

    @staticmethod
    def forward(ctx, obj, frag, loc, gt_obj, gt_frag, gt_loc, gt_weight, weights, reduction,
                ignore_label):
      logits, gt = _head_dicts(obj, frag, loc, gt_obj, gt_frag, gt_loc, gt_weight)
      sums, counts, bad = loss_terms(logits, gt, ignore_label)
      values, scales = loss_values(sums, counts, weights, reduction, knn=gt_knn(gt))
      ctx.save_for_backward(obj, frag, loc, gt_obj, gt_frag, gt_loc, gt_weight, scales)
      ctx.ignore_label = ignore_label
      ctx.mark_non_differentiable(bad)
      return values, bad

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_values, grad_bad):
      obj, frag, loc, gt_obj, gt_frag, gt_loc, gt_weight, scales = ctx.saved_tensors
      logits, gt = _head_dicts(obj, frag, loc, gt_obj, gt_frag, gt_loc, gt_weight)
      grads = loss_grads(logits, gt, scales, upstream=grad_values.to(torch.float64),
                         ignore_label=ctx.ignore_label, need=tuple(ctx.needs_input_grad[:3]))
      return grads + (None,) * 7

  _function = EposLosses
  return _function


def logits_from_features(features, head_weights):
  """The three logit tensors of features f32 [..., K] under the six logits variables
  (HEAD_VARIABLES; weights [1,1,K,N] or [K,N], biases [N]; device tensors): plain torch,
  features.reshape(-1, K) @ W + b in fp32 per head -- NOT the net's grouped heads launch, whose
  rounding differs. Returns the dict loss_terms takes: pred_obj_conf [n,O+1], pred_frag_conf
  [n,O,F], pred_frag_loc [n,O,F,3]."""
  K = int(features.shape[-1])
  x = features.reshape(-1, K)
  n = x.shape[0]
  flat = [x @ head_weights[HEAD_VARIABLES[2 * k]].reshape(K, -1) +
          head_weights[HEAD_VARIABLES[2 * k + 1]] for k in range(3)]
  O = int(flat[0].shape[1]) - 1
  if O < 1 or flat[1].shape[1] % O or flat[2].shape[1] != 3 * flat[1].shape[1]:
    raise ValueError('the logits variables have %d, %d and %d columns: not O+1, O*F and O*F*3' %
                     tuple(t.shape[1] for t in flat))
  F = int(flat[1].shape[1]) // O
  return dict(zip(HEADS, (flat[0], flat[1].view(n, O, F), flat[2].view(n, O, F, 3))))


_features_function = None


def _features_losses_function():
  """The torch.autograd.Function behind differentiable_losses_from_features, defined at first
  use: this module imports without torch."""
  global _features_function
  if _features_function is not None:
    return _features_function
  import torch
  from torch.autograd.function import once_differentiable

  class EposLossesFromFeatures(torch.autograd.Function):

    @staticmethod
    def forward(ctx, features, w_obj, b_obj, w_frag, b_frag, w_loc, b_loc, gt_obj, gt_frag,
                gt_loc, gt_weight, weights, reduction, ignore_label):
      variables = (w_obj, b_obj, w_frag, b_frag, w_loc, b_loc)
      made = logits_from_features(features, dict(zip(HEAD_VARIABLES, variables)))
      logits, gt = _head_dicts(*(made[k] for k in HEADS), gt_obj, gt_frag, gt_loc, gt_weight)
      sums, counts, bad = loss_terms(logits, gt, ignore_label)
      values, scales = loss_values(sums, counts, weights, reduction, knn=gt_knn(gt))
      ctx.save_for_backward(features, w_obj, w_frag, w_loc, *(logits[k] for k in HEADS),
                            gt_obj, gt_frag, gt_loc, gt_weight, scales)
      ctx.ignore_label = ignore_label
      ctx.shapes = tuple(v.shape for v in variables)
      ctx.mark_non_differentiable(bad)
      return values, bad

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_values, grad_bad):
      from epos_amd import heads_train
      (features, w_obj, w_frag, w_loc, obj, frag, loc, gt_obj, gt_frag, gt_loc, gt_weight,
       scales) = ctx.saved_tensors
      logits, gt = _head_dicts(obj, frag, loc, gt_obj, gt_frag, gt_loc, gt_weight)
      up = grad_values.to(torch.float64)
      d_feat = None
      if ctx.needs_input_grad[0]:
        d_feat = heads_train.heads_input_grad(
            logits, gt, scales, dict(zip(HEAD_VARIABLES[0::2], (w_obj, w_frag, w_loc))),
            upstream=up, ignore_label=ctx.ignore_label).view(features.shape)
      need = tuple(ctx.needs_input_grad[1 + 2 * k] or ctx.needs_input_grad[2 + 2 * k]
                   for k in range(3))
      grads = [None] * 6
      if any(need):
        raw = heads_train.heads_weight_grads(features, logits, gt, scales, upstream=up,
                                             ignore_label=ctx.ignore_label, need=need)
        for k, head in enumerate(HEADS):
          if need[k]:
            grads[2 * k] = raw[head][0].view(ctx.shapes[2 * k])
            grads[2 * k + 1] = raw[head][1].view(ctx.shapes[2 * k + 1])
      return (d_feat,) + tuple(grads) + (None,) * 7

  _features_function = EposLossesFromFeatures
  return _features_function


def differentiable_losses_from_features(features, head_weights, gt, weights=(1.0, 1.0, 100.0),
                                        reduction='mean', ignore_label=255):
  """The three losses of one batch as a differentiable function of the FEATURES the logits
  layers read and of the six logits variables: with it a torch.nn restatement of the decoder,
  or any module that produces [B,h,w,K] features, trains against these losses with
  loss.backward(). features f32 [B,h,w,K] or [B*P,K] on the device; head_weights =
  {HEAD_VARIABLES: device tensor} in the checkpoint layout (trainer.Optimizer.params); gt as
  loss_terms takes it. Forward: the logits by plain torch matmuls in fp32
  (logits_from_features), then loss_terms and loss_values: (values f64 [4], bad i64 [B]),
  bit-equal to differentiable_losses on those logits. Backward, once differentiable: d features
  through epos_heads_dgrad_f32 (heads_train.heads_input_grad), dW and db of the six variables
  through epos_heads_wgrad_f32 (heads_train.heads_weight_grads), each only where a gradient is
  needed; the dense logit gradients are never formed. The logits themselves are kept for the
  backward pass. Nothing synchronises."""
  _lib.load()
  C.need_device(features, 'the losses need a HIP device (there is no CPU fallback)')
  if reduction not in REDUCTIONS:
    raise ValueError("reduction must be 'mean' or 'pooled', got %r" % (reduction,))
  need_fp32(features)
  for name in HEAD_VARIABLES:
    if name not in head_weights:
      raise KeyError('head_weights lack %r' % name)
  return _features_losses_function().apply(
      features, *(head_weights[name] for name in HEAD_VARIABLES), *(gt[k] for k in GT_KEYS),
      tuple(float(w) for w in weights), reduction, int(ignore_label))


def differentiable_losses(logits, gt, weights=(1.0, 1.0, 100.0), reduction='mean',
                          ignore_label=255):
  """The three losses of one batch as a differentiable device tensor. logits and gt as
  loss_terms takes them (the logits, e.g., from torch's own convolutions on
  EposNet.decoder_out). Returns (values, bad): values f64 [4] on the device -- obj_cls_loss,
  frag_cls_loss, frag_loc_loss, total_loss, bit-equal to LossEval's 'mean' (or 'pooled') for
  the same batch -- carrying a grad_fn whose backward is epos_loss_grads, once differentiable,
  run only for the logit tensors that need a gradient; bad i64 [B], the bad-pixel counts.
  Nothing synchronises: the caller decides when to look at `bad`. Bad and ignored pixels get
  ZERO gradient and add nothing to the values -- a batch with bad pixels is not refused here as
  LossEval.result refuses it. total_loss has no regularisation term (module docstring)."""
  _lib.load()
  obj = logits[W.PRED_OBJ_CONF]
  C.need_device(obj, 'the losses need a HIP device (there is no CPU fallback)')
  if reduction not in REDUCTIONS:
    raise ValueError("reduction must be 'mean' or 'pooled', got %r" % (reduction,))
  return _losses_function().apply(
      obj, logits[W.PRED_FRAG_CONF], logits[W.PRED_FRAG_LOC], *(gt[k] for k in GT_KEYS),
      tuple(float(w) for w in weights), reduction, int(ignore_label))
