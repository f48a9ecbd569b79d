"""The logits layers' weight gradients and the reference's optimiser step on the device
(csrc/heads_wgrad.hip; include/epos_hip.h, "Weight gradients"; DESIGN.md, "Losses", "Weight
gradients"): the next piece of a trainer after loss.differentiable_losses.

  heads_weight_grads  epos_heads_wgrad_knn_f32: dW and db of logits/pred_obj_conf, pred_frag_conf
                      and pred_frag_loc from EposNet.decoder_out and the raw logits, without the
                      dense logit gradients.
  heads_input_grad    epos_heads_dgrad_knn_f32 (csrc/heads_dgrad.hip; "Input gradient"): the gradient
                      at EposNet.decoder_out, or behind its ReLU, from the raw logits and the
                      three weight matrices, without the dense logit gradients.
  momentum_step       epos_momentum_step_f32: tf.train.MomentumOptimizer on the regularised,
                      multiplied gradient (train.py:340-384), in place.
  net_logits          the logits of a net that has run forward_logits, as the losses take them.
  net_feature_grad    from such a net to the gradient at its decoder output.

What stands above these kernels -- the optimiser, the training step, the learning-rate schedules
-- is epos_amd/trainer.py; the layer below the logits, decoder_conv1_pointwise, gets its weight
and batch-norm gradients from heads_input_grad's output in epos_amd/decoder_train.py.

Pinned to tests/helpers/heads_wgrad_ref.py and, through loss_grad_ref.py, to torch's fp64
autograd; parity with TensorFlow's numbers is unpinned, as for the losses. There is no CPU
fallback: without the library or a device this raises EposError.
"""
from epos_amd import _call as C
from epos_amd import _lib
from epos_amd._lib import EposError
from epos_amd import loss as L
from epos_amd import weights as W

HEADS, variable_names = L.HEADS, L.variable_names


def heads_weight_grads(features, logits, gt, scales, upstream=None, ignore_label=255,
                       need=(True, True, True), out=None, workspace=None):
  """epos_heads_wgrad_knn_f32 over one batch. features: the tensor the logits layers read
  (EposNet.decoder_out), f32 [B,h,w,K] or [B*P,K], rows a constant stride apart; logits, gt,
  scales, upstream as loss.loss_grads takes them. Returns {head name: (dW f32 [K,N], db f32
  [N])} for pred_obj_conf (N = O+1), pred_frag_conf (O*F) and pred_frag_loc (O*F*3), None for a
  head with need[k] false (it is then neither read nor written). `out` = {head name: (dW, db)}
  of tensors to write into (either may be None: not computed); `workspace` = an int64 tensor of
  at least epos_heads_wgrad_workspace_bytes / 8 values. Every element of every output is
  written. Enqueues on the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  bt = L.Batch(logits, gt, 'the weight gradients need', scales, upstream)
  dev, B, P, O, F, n = bt.dev, bt.B, bt.P, bt.O, bt.F, bt.n
  if features.device != dev:
    raise EposError('features are on %s, the logits on %s' % (features.device, dev))
  L.need_fp32(features)
  K = int(features.shape[-1])
  feat2, lda = C.rows(features, K)
  if feat2.shape[0] != n:
    raise ValueError('features hold %d rows, expected %d' % (feat2.shape[0], n))
  widths = (O + 1, O * F, O * F * 3)
  result, ptrs = {}, []
  for k, head in enumerate(HEADS):
    pair = [None, None]
    if need[k]:
      given = (out or {}).get(head)
      for j, shape in enumerate(((K, widths[k]), (widths[k],))):
        if given is None or given[j] is not None:
          pair[j] = C.out(given and given[j], dev, torch.float32, shape,
                           'out[%r][%d]' % (head, j))
    ptrs += pair
    result[head] = tuple(pair) if need[k] else None
  nbytes = lib.epos_heads_wgrad_workspace_bytes(B, P, O, F, K)
  _lib.check(nbytes, 'epos_heads_wgrad_workspace_bytes')
  ws = C.workspace(workspace, dev, nbytes)
  with C.launch(dev) as q:
    q.keep(feat2, ws, *bt.keep)
    _lib.check(lib.epos_heads_wgrad_knn_f32(
        C.ptr(feat2), lda, K, *bt.grad_args(ignore_label), C.ptr(ws),
        *[C.ptr(t) for t in ptrs], q.handle), 'epos_heads_wgrad_knn_f32')
  return result


def heads_input_grad(logits, gt, scales, head_weights, upstream=None, relu_of=None,
                     ignore_label=255, out=None, workspace=None):
  """epos_heads_dgrad_knn_f32 over one batch: the gradient of the losses with respect to the tensor
  the logits layers read (EposNet.decoder_out), without the dense logit gradients. logits, gt,
  scales, upstream as loss.loss_grads takes them; head_weights = {variable name: tensor or
  array} with 'logits/<name>/weights' in the checkpoint layout [1,1,K,N] (or [K,N]), as
  trainer.Optimizer.params and state() hold them (other keys are ignored). The kernel reads the
  matrices transposed, [N,K]: they are transposed here, with torch, on the current stream, into
  `workspace` (a contiguous float32 tensor of at least (O+1 + 4*O*F) * K values) or a new
  tensor. relu_of: the forward activation f32 [B,h,w,K] or [B*P,K], rows a constant stride
  apart (it may be the features themselves): the result is +0.0 wherever it is <= 0, the
  gradient with respect to the pre-activation. Returns dX f32 [B*P, K], or `out` (f32 [..., K],
  rows a constant stride apart, B*P of them; its padding columns are kept). Every element is
  written. Enqueues on the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  bt = L.Batch(logits, gt, 'the input gradient needs', scales, upstream)
  dev, O, F, n = bt.dev, bt.O, bt.F, bt.n
  widths = (O + 1, O * F, O * F * 3)
  mats, K = [], None
  for head, width in zip(HEADS, widths):
    wname = variable_names(head)[0]
    if wname not in head_weights:
      raise KeyError('head_weights lack %r' % wname)
    m = torch.as_tensor(head_weights[wname])
    if m.dim() < 2 or m.shape[-1] != width or m.numel() != m.shape[-2] * width:
      raise ValueError('%s must be [1, 1, K, %d], got %s' % (wname, width, tuple(m.shape)))
    if K is None:
      K = int(m.shape[-2])
    elif m.shape[-2] != K:
      raise ValueError('%s has %d input channels, expected %d' % (wname, m.shape[-2], K))
    mats.append(m.reshape(K, width))
  rows = sum(widths)
  wt = C.workspace(workspace, dev, 4 * rows * K, torch.float32).view(-1)[:rows * K].view(rows, K)
  r0 = 0
  for m, width in zip(mats, widths):
    wt[r0:r0 + width].copy_(m.t())                 # to the device and to float32 where needed
    r0 += width
  y2, ldy = None, K
  if relu_of is not None:
    if relu_of.device != dev:
      raise EposError('relu_of is on %s, the logits on %s' % (relu_of.device, dev))
    if relu_of.dtype != torch.float32 or relu_of.shape[-1] != K:
      raise TypeError('relu_of must be torch.float32 [..., %d], got %s %s' % (
          K, relu_of.dtype, tuple(relu_of.shape)))
    y2, ldy = C.rows(relu_of, K)
    if y2.shape[0] != n:
      raise ValueError('relu_of holds %d rows, expected %d' % (y2.shape[0], n))
  out = C.out(out, dev, torch.float32, (n, K), 'out', rows=True)
  out2, ldx = C.rows(out, K)
  if out2.data_ptr() != out.data_ptr() or out2.shape[0] != n:
    raise ValueError('out: %d rows of dX must lie a constant stride apart' % n)
  with C.launch(dev) as q:
    q.keep(wt, y2, *bt.keep)
    _lib.check(lib.epos_heads_dgrad_knn_f32(
        *bt.grad_args(ignore_label), C.ptr(wt[:widths[0]]),
        C.ptr(wt[widths[0]:widths[0] + widths[1]]), C.ptr(wt[widths[0] + widths[1]:]), K, K,
        C.ptr(y2), ldy, C.ptr(out2), ldx, q.handle), 'epos_heads_dgrad_knn_f32')
  return out


def momentum_step(param, accum, grad, lr, momentum=0.9, weight_decay=0.0, grad_mult=1.0):
  """epos_momentum_step_f32, in place on param and accum (f32, contiguous, on the device):
  g = grad_mult * (grad + weight_decay * param); accum = momentum * accum + g;
  param = param - lr * accum, each operation rounded once in fp32. Enqueues on the current
  stream; does not synchronise."""
  import torch
  lib = _lib.load()
  C.need_device(param, 'the momentum step needs a HIP device (there is no CPU fallback)')
  n = param.numel()
  for t, what in ((param, 'param'), (accum, 'accum'), (grad, 'grad')):
    C.dense(t, param.device, torch.float32, what, numel=n, name='float32')
  with C.launch(param.device) as q:
    _lib.check(lib.epos_momentum_step_f32(
        C.ptr(param), C.ptr(accum), C.ptr(grad), n, float(lr), float(momentum),
        float(weight_decay), float(grad_mult), q.handle), 'epos_momentum_step_f32')
  return param


def net_logits(net):
  """The logits of a net that has run forward_logits, as loss.loss_terms takes them: views
  [B,h,w,O+1], [B,h,w,O,F] and [B,h,w,O,F,3] of the net's own buffers."""
  B, h, w = (int(d) for d in net.decoder_out.shape[:3])
  O, F = int(net.num_objs), int(net.num_frags)
  return {W.PRED_OBJ_CONF: net.logits[W.PRED_OBJ_CONF],
          W.PRED_FRAG_CONF: net.logits[W.PRED_FRAG_CONF].view(B, h, w, O, F),
          W.PRED_FRAG_LOC: net.logits[W.PRED_FRAG_LOC].view(B, h, w, O, F, 3)}


def _net_losses(net, gt, weights, reduction, ignore_label):
  """loss_terms -> loss_values on an fp32 net's logits: (logits, values, bad, scales)."""
  L.need_fp32(net.decoder_out)
  logits = net_logits(net)
  sums, counts, bad = L.loss_terms(logits, gt, ignore_label)
  values, scales = L.loss_values(sums, counts, weights, reduction, knn=L.gt_knn(gt))
  return logits, values, bad, scales


def net_feature_grad(net, gt, head_weights, weights=(1.0, 1.0, 100.0), reduction='pooled',
                     relu=False, ignore_label=255):
  """From a running network to the gradient at its decoder output: call after
  net.forward_logits(). Runs loss_terms -> loss_values -> heads_input_grad on the net's logits
  with head_weights (the six logits variables the net was built from, or
  trainer.Optimizer.params). Returns (values f64 [4], bad i64 [B], dX f32 [B*P, K]): values and
  bad as loss.differentiable_losses returns them, dX the gradient with respect to
  net.decoder_out or, with relu=True, masked with net.decoder_out: with respect to the
  pre-activation of decoder_conv1_pointwise (batch norm folded). fp32 single-scale nets only.
  Does not synchronise."""
  logits, values, bad, scales = _net_losses(net, gt, weights, reduction, ignore_label)
  dX = heads_input_grad(logits, gt, scales, head_weights,
                        relu_of=net.decoder_out if relu else None, ignore_label=ignore_label)
  return values, bad, dX
