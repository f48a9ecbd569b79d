"""The logits layers' weight gradients and the reference's optimiser step on the device
(csrc/heads_wgrad.hip; include/epos_hip.h, "Weight gradients"; DESIGN.md, "Losses", "Weight
gradients"): the next piece of a trainer after loss.differentiable_losses.

  heads_weight_grads  epos_heads_wgrad_f32: dW and db of logits/pred_obj_conf, pred_frag_conf
                      and pred_frag_loc from EposNet.decoder_out and the raw logits, without the
                      dense logit gradients.
  heads_input_grad    epos_heads_dgrad_f32 (csrc/heads_dgrad.hip; "Input gradient"): the gradient
                      at EposNet.decoder_out, or behind its ReLU, from the raw logits and the
                      three weight matrices, without the dense logit gradients.
  momentum_step       epos_momentum_step_f32: tf.train.MomentumOptimizer on the regularised,
                      multiplied gradient (train.py:340-384), in place.
  net_head_grads      from a net that has run forward_logits to checkpoint-shaped gradients.
  net_feature_grad    from such a net to the gradient at its decoder output.
  HeadsOptimizer      fp32 master copies and accumulators of the six variables; restores the
                      accumulators from '<name>/Momentum' entries, so that a run can resume.
  learning_rate       the reference's schedules (train_utils.py:117-195) in Python floats.
  train_step          one step of the loop: forward_logits -> net_head_grads -> the optimiser
                      step -> EposNet.set_head_weights (the device weight packer,
                      csrc/weight_pack.hip: the updated weights reach the built net, its
                      captured graphs included, without a round trip through the host).

The loop itself, its checkpoints and its logging are train_heads.py. train_step keeps
everything below the logits frozen; the layer below them, decoder_conv1_pointwise, is trained by
epos_amd/decoder_train.py (its weight and batch-norm gradients from heads_input_grad's output,
DecoderOptimizer, train_step_decoder). Not built: backpropagation from decoder_conv1_depthwise
down, which starts with the input gradient G W^T of decoder_conv1_pointwise; batch-norm
statistics, bf16 mode, multi-scale nets and more than one device. Augmentation is
epos_amd/augment.py; train_step applies it between the upload and the forward pass.

Pinned to tests/helpers/heads_wgrad_ref.py and, through loss_grad_ref.py, to torch's fp64
autograd; parity with TensorFlow's numbers is unpinned, as for the losses -- that holds for
learning_rate too: TensorFlow evaluates the schedules in float32, this module in Python
floats. There is no CPU fallback: without the library or a device this raises EposError.
"""
import ctypes
import math

from epos_amd import _lib
from epos_amd._lib import EposError
from epos_amd import loss as L
from epos_amd import weights as W

HEADS, variable_names = L.HEADS, L.variable_names


def heads_weight_grads(features, logits, gt, scales, upstream=None, ignore_label=255,
                       need=(True, True, True), out=None, workspace=None):
  """epos_heads_wgrad_f32 over one batch. features: the tensor the logits layers read
  (EposNet.decoder_out), f32 [B,h,w,K] or [B*P,K], rows a constant stride apart; logits, gt,
  scales, upstream as loss.loss_grads takes them. Returns {head name: (dW f32 [K,N], db f32
  [N])} for pred_obj_conf (N = O+1), pred_frag_conf (O*F) and pred_frag_loc (O*F*3), None for a
  head with need[k] false (it is then neither read nor written). `out` = {head name: (dW, db)}
  of tensors to write into (either may be None: not computed); `workspace` = an int64 tensor of
  at least epos_heads_wgrad_workspace_bytes / 8 values. Every element of every output is
  written. Enqueues on the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  bt = L._Batch(logits, gt, 'the weight gradients need', scales, upstream)
  dev, B, P, O, F, n = bt.dev, bt.B, bt.P, bt.O, bt.F, bt.n
  if features.device != dev:
    raise EposError('features are on %s, the logits on %s' % (features.device, dev))
  L._need_fp32(features)
  K = int(features.shape[-1])
  feat2, lda = L._rows(features, K)
  if feat2.shape[0] != n:
    raise ValueError('features hold %d rows, expected %d' % (feat2.shape[0], n))
  widths = (O + 1, O * F, O * F * 3)
  result, ptrs = {}, []
  for k, head in enumerate(HEADS):
    pair = [None, None]
    if need[k]:
      given = (out or {}).get(head)
      for j, shape in enumerate(((K, widths[k]), (widths[k],))):
        if given is None:
          pair[j] = torch.empty(shape, dtype=torch.float32, device=dev)
        elif given[j] is not None:
          t = given[j]
          if (t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != shape or
              not t.is_contiguous()):
            raise ValueError('out[%r][%d] must be a contiguous float32 tensor of shape %s on '
                             '%s' % (head, j, shape, dev))
          pair[j] = t
    ptrs += pair
    result[head] = tuple(pair) if need[k] else None
  nbytes = lib.epos_heads_wgrad_workspace_bytes(B, P, O, F, K)
  _lib.check(nbytes, 'epos_heads_wgrad_workspace_bytes')
  if workspace is None:
    ws = torch.empty(((nbytes + 7) // 8 or 1,), dtype=torch.int64, device=dev)
  else:
    ws = workspace
    if (ws.device != dev or not ws.is_contiguous() or
        ws.numel() * ws.element_size() < nbytes):
      raise ValueError('workspace must be a contiguous tensor of at least %d bytes on %s' % (
          nbytes, dev))
  stream = torch.cuda.current_stream(dev)
  with torch.cuda.device(dev):
    _lib.check(lib.epos_heads_wgrad_f32(
        L._ptr(feat2), lda, K, *bt.grad_args(ignore_label), L._ptr(ws),
        *[L._ptr(t) for t in ptrs], ctypes.c_void_p(stream.cuda_stream)), 'epos_heads_wgrad_f32')
  for t in bt.keep + [feat2, ws]:
    t.record_stream(stream)           # temporaries and dense copies made here outlive the call
  return result


def heads_input_grad(logits, gt, scales, head_weights, upstream=None, relu_of=None,
                     ignore_label=255, out=None, workspace=None):
  """epos_heads_dgrad_f32 over one batch: the gradient of the losses with respect to the tensor
  the logits layers read (EposNet.decoder_out), without the dense logit gradients. logits, gt,
  scales, upstream as loss.loss_grads takes them; head_weights = {variable name: tensor or
  array} with 'logits/<name>/weights' in the checkpoint layout [1,1,K,N] (or [K,N]), as
  HeadsOptimizer.params and state() hold them (other keys are ignored). The kernel reads the
  matrices transposed, [N,K]: they are transposed here, with torch, on the current stream, into
  `workspace` (a contiguous float32 tensor of at least (O+1 + 4*O*F) * K values) or a new
  tensor. relu_of: the forward activation f32 [B,h,w,K] or [B*P,K], rows a constant stride
  apart (it may be the features themselves): the result is +0.0 wherever it is <= 0, the
  gradient with respect to the pre-activation. Returns dX f32 [B*P, K], or `out` (f32 [..., K],
  rows a constant stride apart, B*P of them; its padding columns are kept). Every element is
  written. Enqueues on the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  bt = L._Batch(logits, gt, 'the input gradient needs', scales, upstream)
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
  if workspace is None:
    wt = torch.empty((rows, K), dtype=torch.float32, device=dev)
  else:
    if (workspace.device != dev or workspace.dtype != torch.float32 or
        not workspace.is_contiguous() or workspace.numel() < rows * K):
      raise ValueError('workspace must be a contiguous float32 tensor of at least %d values '
                       'on %s' % (rows * K, dev))
    wt = workspace.view(-1)[:rows * K].view(rows, K)
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
    y2, ldy = L._rows(relu_of, K)
    if y2.shape[0] != n:
      raise ValueError('relu_of holds %d rows, expected %d' % (y2.shape[0], n))
  if out is None:
    out = torch.empty((n, K), dtype=torch.float32, device=dev)
  elif out.device != dev or out.dtype != torch.float32 or out.shape[-1] != K:
    raise ValueError('out must be a float32 tensor [..., %d] on %s' % (K, dev))
  out2, ldx = L._rows(out, K)
  if out2.data_ptr() != out.data_ptr() or out2.shape[0] != n:
    raise ValueError('out: %d rows of dX must lie a constant stride apart' % n)
  stream = torch.cuda.current_stream(dev)
  with torch.cuda.device(dev):
    _lib.check(lib.epos_heads_dgrad_f32(
        *bt.grad_args(ignore_label), L._ptr(wt[:widths[0]]),
        L._ptr(wt[widths[0]:widths[0] + widths[1]]), L._ptr(wt[widths[0] + widths[1]:]), K, K,
        L._ptr(y2), ldy, L._ptr(out2), ldx, ctypes.c_void_p(stream.cuda_stream)),
               'epos_heads_dgrad_f32')
  for t in bt.keep + [wt] + ([y2] if y2 is not None else []):
    t.record_stream(stream)           # temporaries and dense copies made here outlive the call
  return out


def momentum_step(param, accum, grad, lr, momentum=0.9, weight_decay=0.0, grad_mult=1.0):
  """epos_momentum_step_f32, in place on param and accum (f32, contiguous, on the device):
  g = grad_mult * (grad + weight_decay * param); accum = momentum * accum + g;
  param = param - lr * accum, each operation rounded once in fp32. Enqueues on the current
  stream; does not synchronise."""
  import torch
  lib = _lib.load()
  if not param.is_cuda:
    raise EposError('the momentum step needs a HIP device (there is no CPU fallback)')
  n = param.numel()
  for t, what in ((param, 'param'), (accum, 'accum'), (grad, 'grad')):
    if (t.device != param.device or t.dtype != torch.float32 or t.numel() != n or
        not t.is_contiguous()):
      raise ValueError('%s must be a contiguous float32 tensor of %d values on %s' % (
          what, n, param.device))
  stream = torch.cuda.current_stream(param.device)
  with torch.cuda.device(param.device):
    _lib.check(lib.epos_momentum_step_f32(
        L._ptr(param), L._ptr(accum), L._ptr(grad), n, float(lr), float(momentum),
        float(weight_decay), float(grad_mult), ctypes.c_void_p(stream.cuda_stream)),
               'epos_momentum_step_f32')
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
  L._need_fp32(net.decoder_out)
  logits = net_logits(net)
  sums, counts, bad = L.loss_terms(logits, gt, ignore_label)
  values, scales = L.loss_values(sums, counts, weights, reduction)
  return logits, values, bad, scales


def net_head_grads(net, gt, weights=(1.0, 1.0, 100.0), reduction='pooled', ignore_label=255):
  """From a running network to checkpoint-shaped gradients: call after net.forward_logits().
  Runs loss_terms -> loss_values -> heads_weight_grads on net.decoder_out and the net's logits.
  Returns (values f64 [4], bad i64 [B], grads): values and bad as loss.differentiable_losses
  returns them, grads = {'logits/<name>/weights': f32 [1,1,K,N], 'logits/<name>/biases': f32
  [N]} on the device. fp32 single-scale nets only. Does not synchronise."""
  logits, values, bad, scales = _net_losses(net, gt, weights, reduction, ignore_label)
  raw = heads_weight_grads(net.decoder_out, logits, gt, scales, ignore_label=ignore_label)
  grads = {}
  for head in HEADS:
    dW, db = raw[head]
    wname, bname = variable_names(head)
    grads[wname] = dW.view(1, 1, dW.shape[0], dW.shape[1])
    grads[bname] = db
  return values, bad, grads


def net_feature_grad(net, gt, head_weights, weights=(1.0, 1.0, 100.0), reduction='pooled',
                     relu=False, ignore_label=255):
  """From a running network to the gradient at its decoder output: call after
  net.forward_logits(). Runs loss_terms -> loss_values -> heads_input_grad on the net's logits
  with head_weights (the six logits variables the net was built from, or
  HeadsOptimizer.params). Returns (values f64 [4], bad i64 [B], dX f32 [B*P, K]): values and
  bad as loss.differentiable_losses returns them, dX the gradient with respect to
  net.decoder_out or, with relu=True, masked with net.decoder_out: with respect to the
  pre-activation of decoder_conv1_pointwise (batch norm folded). fp32 single-scale nets only.
  Does not synchronise."""
  logits, values, bad, scales = _net_losses(net, gt, weights, reduction, ignore_label)
  dX = heads_input_grad(logits, gt, scales, head_weights,
                        relu_of=net.decoder_out if relu else None, ignore_label=ignore_label)
  return values, bad, dX


def learning_rate(step, policy='poly', base_learning_rate=1e-4, decay_step=2000,
                  decay_factor=0.1, train_steps=2000000, power=0.9, slow_start_step=0,
                  slow_start_learning_rate=1e-4, burnin='none'):
  """The reference's learning rate at global step `step` (train_utils.py:117-195), in Python
  floats. 'poly': base * (1 - min(s, train_steps) / train_steps) ^ power
  (tf.train.polynomial_decay with end_learning_rate = 0); 'step': base * decay_factor ^
  floor(s / decay_step) (exponential_decay, staircase); s = step, or step - slow_start_step
  when there is a burn-in. While step < slow_start_step the rate is slow_start_learning_rate
  (burnin 'none') or rises linearly from it towards base_learning_rate ('linear')."""
  if policy not in ('poly', 'step'):
    raise ValueError('Unknown learning policy: %r (poly, step).' % (policy,))
  if burnin not in ('none', 'linear'):
    raise ValueError('Unknown burnin type: %r (none, linear).' % (burnin,))
  s = step - slow_start_step if burnin != 'none' else step
  if policy == 'step':
    lr = base_learning_rate * decay_factor ** math.floor(s / decay_step)
  else:
    lr = base_learning_rate * (1.0 - min(s, train_steps) / train_steps) ** power
  if step < slow_start_step:
    lr = slow_start_learning_rate
    if burnin == 'linear':
      lr += (base_learning_rate - slow_start_learning_rate) * step / slow_start_step
  return float(lr)


def train_step(net, images, gt, opt, lr, weights=(1.0, 1.0, 100.0), reduction='pooled',
               augment=None, step=None):
  """One training step of the logits layers, enqueued on the current stream without a
  synchronisation: net.forward_logits(images, use_graph=True), net_head_grads, opt.step(grads,
  lr), net.set_head_weights(opt.params, check=False). With augment (an augment.Augmenter) the
  images are uploaded first (net.set_images), augmented in place on the device with the draws
  of global step `step` (augment.apply(net.images, step)) and the forward pass reads them
  there. Returns (values f64 [4], bad i64 [B],
  status i32): the losses of THIS step's forward (before its update) and the bad-pixel counts
  as loss.differentiable_losses returns them, and set_head_weights' status words -- non-zero
  when the packer refused the updated weights and the net kept the previous ones. The caller
  reads them when it chooses."""
  import torch
  if not torch.cuda.is_available():
    raise EposError('train_step needs a HIP device (there is no CPU fallback)')
  if augment is not None:
    if step is None:
      raise ValueError('train_step: augment needs the global step its draws are keyed by')
    net.set_images(images)
    augment.apply(net.images, step)
    images = None
  net.forward_logits(images, use_graph=True)
  values, bad, grads = net_head_grads(net, gt, weights, reduction)
  opt.step(grads, lr)
  status = net.set_head_weights(opt.params, check=False)
  return values, bad, status


class HeadsOptimizer(object):
  """fp32 master copies and momentum accumulators of the six logits variables on the device.
  variables: {'logits/<name>/weights': [1,1,K,N], 'logits/<name>/biases': [N]} (numpy arrays or
  tensors) and, optionally, their accumulators '<variable name>/Momentum' as state() and the
  trainer's checkpoints hold them (absent: zeros); other keys are ignored. step(grads) applies
  momentum_step per variable as the reference's trainer does: weights get the multiplier
  m = last_layer_gradient_multiplier and the l2 decay, biases 2 * m and no decay
  (train_utils.py:84-114). `params` is what EposNet.set_head_weights takes."""

  def __init__(self, variables, lr, momentum=0.9, weight_decay=4e-5,
               last_layer_gradient_multiplier=1.0, device=None):
    import torch
    if not torch.cuda.is_available():
      raise EposError('the optimiser needs a HIP device (there is no CPU fallback)')
    _lib.load()
    self.device = torch.device(device if device is not None else 'cuda:0')
    self.lr, self.momentum = float(lr), float(momentum)
    self.weight_decay = float(weight_decay)
    self.multiplier = float(last_layer_gradient_multiplier)
    self.params, self.accums = {}, {}
    for head in HEADS:
      for name in variable_names(head):
        if name not in variables:
          raise KeyError('variables lack %r' % name)
        v = torch.as_tensor(variables[name]).to(device=self.device, dtype=torch.float32)
        self.params[name] = v.contiguous().clone()
        slot = variables.get(name + '/Momentum')
        if slot is None:
          self.accums[name] = torch.zeros_like(self.params[name])
        else:
          a = torch.as_tensor(slot).to(device=self.device, dtype=torch.float32)
          if a.numel() != self.params[name].numel():
            raise ValueError('%s/Momentum holds %d values, the variable %d' % (
                name, a.numel(), self.params[name].numel()))
          self.accums[name] = a.reshape(self.params[name].shape).contiguous().clone()

  def step(self, grads, lr=None):
    """One update of every variable from grads (as net_head_grads returns them). lr overrides
    the constructor's for this step (the schedules are the caller's)."""
    lr = self.lr if lr is None else float(lr)
    for name, param in self.params.items():
      g = grads[name]
      if g.numel() != param.numel():
        raise ValueError('%s: gradient of %d values, variable of %d' % (
            name, g.numel(), param.numel()))
      bias = name.endswith('/biases')
      momentum_step(param, self.accums[name], g.contiguous().view(param.shape), lr,
                    self.momentum, 0.0 if bias else self.weight_decay,
                    2.0 * self.multiplier if bias else self.multiplier)

  def state(self, with_slots=True):
    """{variable name: numpy array} for tf_checkpoint.write_checkpoint: the six variables and,
    with_slots, their '<name>/Momentum' accumulators. Synchronises."""
    out = {name: p.cpu().numpy() for name, p in self.params.items()}
    if with_slots:
      for name, a in self.accums.items():
        out[name + '/Momentum'] = a.cpu().numpy()
    return out
