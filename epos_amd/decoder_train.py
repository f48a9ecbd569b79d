"""Training decoder/decoder_conv1_pointwise, the layer below the logits, on the device
(csrc/pointwise_wgrad.hip; include/epos_hip.h, "Pointwise weight gradient"; DESIGN.md, "Losses",
"Decoder layer gradients"): the first step of backpropagation below the logits layers.

  pointwise_weight_grads  epos_pointwise_wgrad_f32 + epos_pointwise_wgrad_close_f32: dW, dgamma
                          and dbeta of a 1x1 conv layer with a frozen batch norm (or dW and db
                          of one with biases) from its input A -- fp32 or the fp16 pairs the
                          depthwise kernel wrote -- and the gradient G at its pre-activation.
  net_decoder_grads       from a net that has run forward_logits to the gradients of the nine
                          variables: the six of the logits layers and the layer's weights,
                          BatchNorm/gamma and BatchNorm/beta.
  gradient_rule           the reference's multiplier and decay of a variable, in Python.
  DecoderOptimizer        heads_train.HeadsOptimizer's contract over the nine variables, any
                          subset of them trainable.
  train_step_decoder      heads_train.train_step with the layer unfrozen: forward_logits ->
                          net_decoder_grads -> the optimiser step -> EposNet.set_layer_weights.

The batch-norm statistics are frozen (the reference's fine_tune_batch_norm=False): moving_mean
and moving_variance are inputs. Not built: the input gradient of this layer, G W^T, and with it
everything from decoder_conv1_depthwise down; batch-norm statistics, bf16 mode, multi-scale nets
and more than one device. Pinned to tests/helpers/pointwise_wgrad_ref.py and, through it, to
torch's fp64 autograd; parity with TensorFlow's gradients is unpinned. There is no CPU fallback.
"""
import ctypes

from epos_amd import _lib
from epos_amd._lib import EposError
from epos_amd import heads_train as HT
from epos_amd import loss as L
from epos_amd import weights as W

LAYER = W.DECODER_CONV1_POINTWISE
LAYER_VARIABLES = (LAYER + '/weights', LAYER + '/BatchNorm/gamma', LAYER + '/BatchNorm/beta')
LAYER_CONSTANTS = (LAYER + '/BatchNorm/moving_mean', LAYER + '/BatchNorm/moving_variance')
VARIABLES = L.HEAD_VARIABLES + LAYER_VARIABLES
BN_EPS = 1e-5                    # model.py:307-312, the decoder's batch norms
# model.py: get_extra_layer_scopes(last_layers_contain_logits_only=False) -- every scope above
# the backbone counts as a last layer (train_utils.py:84-114 tests `scope in variable name`)
LAST_LAYER_SCOPES = ('logits', 'image_pooling', 'aspp', 'concat_projection', 'decoder',
                     'meta_architecture')


def workspace_words(M, K, N):
  """int64 words pointwise_weight_grads needs for M rows: S and g in fp64 and the kernel's
  slabs."""
  nbytes = _lib.load().epos_pointwise_wgrad_workspace_bytes(M, K, N)
  _lib.check(nbytes, 'epos_pointwise_wgrad_workspace_bytes')
  return K * N + N + (nbytes + 7) // 8


def pointwise_weight_grads(a, g, weights, bn=None, eps=BN_EPS, a_h2=None, out=None,
                           workspace=None):
  """The weight gradients of the layer y = relu(scale (.) (A W) + bias) from its input and the
  gradient at its pre-activation. a: the layer's input, f32 [..., K], rows a constant stride
  apart -- or, with a_h2 = (slot, slot2 or None, gain, bias), the fp16 pairs the depthwise
  kernel wrote into such a tensor (EposNet.pointwise_operand gives both); slot, slot2: the 64
  uint32 words of an absmax slot as an int32 tensor. g: f32 [..., N], as many rows, as
  heads_train.heads_input_grad(relu_of=...) writes it. weights: f32 [1,1,K,N] or [K,N] on the
  device. bn = (gamma, moving_mean, moving_variance), f32 [N] on the device, with eps; None: a
  conv with biases. Returns {'weights': dW f32 [1,1,K,N], 'BatchNorm/gamma': f32 [N],
  'BatchNorm/beta': f32 [N]}, or {'weights', 'biases'} without a batch norm. `out` = such a
  dict of contiguous tensors to write into; `workspace` = an int64 tensor of at least
  workspace_words(rows, K, N) values. Every element of every output is written. Enqueues on
  the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  if not g.is_cuda:
    raise EposError('the weight gradients need a HIP device (there is no CPU fallback)')
  dev = g.device
  for t, what in ((a, 'a'), (g, 'g'), (weights, 'weights')):
    if t.device != dev:
      raise EposError('%s is on %s, g on %s' % (what, t.device, dev))
    if t.dtype != torch.float32:
      raise TypeError('%s must be torch.float32, got %s' % (what, t.dtype))
  K, N = int(a.shape[-1]), int(g.shape[-1])
  if weights.dim() < 2 or tuple(weights.shape[-2:]) != (K, N) or weights.numel() != K * N:
    raise ValueError('weights must be [1, 1, %d, %d], got %s' % (K, N, tuple(weights.shape)))
  if not weights.is_contiguous():
    raise ValueError('weights must be contiguous')
  a2, lda = L._rows(a, K)
  g2, ldg = L._rows(g, N)
  M = int(a2.shape[0])
  if g2.shape[0] != M or M < 1:
    raise ValueError('a holds %d rows, g %d' % (M, g2.shape[0]))
  if a_h2 is not None and a2.data_ptr() != a.data_ptr():
    raise ValueError('a pre-split a must have rows a constant stride apart')
  names = ('weights', 'BatchNorm/gamma', 'BatchNorm/beta') if bn is not None else \
      ('weights', 'biases')
  consts = [None, None, None]
  if bn is not None:
    if len(bn) != 3:
      raise ValueError('bn = (gamma, moving_mean, moving_variance)')
    for t, what in zip(bn, ('gamma', 'moving_mean', 'moving_variance')):
      if (t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != (N,) or
          not t.is_contiguous()):
        raise ValueError('%s must be a contiguous float32 tensor of shape (%d,) on %s' % (
            what, N, dev))
    consts = list(bn)
  slots = [None, None]
  gain = bias = 0.0
  if a_h2 is not None:
    slots, gain, bias = [a_h2[0], a_h2[1]], float(a_h2[2]), float(a_h2[3])
    for t in slots:
      if t is not None and (t.device != dev or t.element_size() != 4 or
                            t.numel() != _lib.AMAX_WORDS or not t.is_contiguous()):
        raise ValueError('a_h2: a slot is %d contiguous 4-byte words on %s' % (
            _lib.AMAX_WORDS, dev))
    if slots[0] is None:
      raise ValueError('a_h2: a pre-split a needs its absmax slot')
  result = {}
  for name in names:
    shape = (1, 1, K, N) if name == 'weights' else (N,)
    t = (out or {}).get(name)
    if t is None:
      t = torch.empty(shape, dtype=torch.float32, device=dev)
    elif (t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or
          t.numel() != (K * N if name == 'weights' else N)):
      raise ValueError('out[%r] must be a contiguous float32 tensor of shape %s on %s' % (
          name, shape, dev))
    result[name] = t
  words = workspace_words(M, K, N)
  if workspace is None:
    ws = torch.empty((words,), dtype=torch.int64, device=dev)
  else:
    ws = workspace
    if (ws.device != dev or ws.dtype != torch.int64 or not ws.is_contiguous() or
        ws.numel() < words):
      raise ValueError('workspace must be a contiguous int64 tensor of at least %d values on '
                       '%s' % (words, dev))
  S, gsum, slabs = ws[:K * N], ws[K * N:K * N + N], ws[K * N + N:]
  args = _lib.PointwiseWgradArgs(
      A=L._ptr(a2), lda=lda, G=L._ptr(g2), ldg=ldg, M=M, K=K, N=N,
      a_presplit=int(a_h2 is not None), a_amax=L._ptr(slots[0]), a_amax2=L._ptr(slots[1]),
      a_gain=gain, a_bias=bias, S=L._ptr(S), g=L._ptr(gsum),
      workspace=L._ptr(slabs) if slabs.numel() else None)
  stream = torch.cuda.current_stream(dev)
  sp = ctypes.c_void_p(stream.cuda_stream)
  with torch.cuda.device(dev):
    _lib.check(lib.epos_pointwise_wgrad_f32(ctypes.byref(args), sp), 'epos_pointwise_wgrad_f32')
    _lib.check(lib.epos_pointwise_wgrad_close_f32(
        L._ptr(S), L._ptr(gsum), L._ptr(weights), K, N, L._ptr(consts[0]), L._ptr(consts[1]),
        L._ptr(consts[2]), float(eps), L._ptr(result['weights']),
        L._ptr(result['BatchNorm/gamma']) if bn is not None else None,
        L._ptr(result[names[-1]]), sp), 'epos_pointwise_wgrad_close_f32')
  for t in (a2, g2, ws):
    t.record_stream(stream)             # temporaries and dense copies made here outlive the call
  return result


def _layer_inputs(net, variables):
  """(weights, (gamma, moving_mean, moving_variance)) of the layer on the net's device: the
  variables from `variables`, the statistics from it too or else the net's checkpoint."""
  import torch
  mean, var = net.layer_constants(LAYER)
  given = [variables.get(n) for n in LAYER_CONSTANTS]
  if given[0] is not None:
    mean = torch.as_tensor(given[0], dtype=torch.float32).to(net.dev)
  if given[1] is not None:
    var = torch.as_tensor(given[1], dtype=torch.float32).to(net.dev)
  for n in LAYER_VARIABLES:
    if n not in variables:
      raise KeyError('variables lack %r' % n)
  w, gamma = (torch.as_tensor(variables[n], dtype=torch.float32).to(net.dev).contiguous()
              for n in LAYER_VARIABLES[:2])
  return w, (gamma, mean.contiguous(), var.contiguous())


def net_decoder_grads(net, gt, variables, weights=(1.0, 1.0, 100.0), reduction='pooled',
                      ignore_label=255):
  """From a running network to the gradients of the nine variables: call after
  net.forward_logits(). variables: the nine variables the net currently runs on (as
  DecoderOptimizer.params holds them; the logits weights give the input gradient, the layer's
  weights and gamma its own gradients). Runs loss_terms -> loss_values once, then
  heads_weight_grads, heads_input_grad(relu_of=net.decoder_out) and pointwise_weight_grads on
  the net's own A (EposNet.pointwise_operand: fp16 pairs by default). Returns (values f64 [4],
  bad i64 [B], grads): values and bad as loss.differentiable_losses returns them, grads = the
  six entries of heads_train.net_head_grads and 'decoder/decoder_conv1_pointwise/weights' f32
  [1,1,256,256], '/BatchNorm/gamma' and '/BatchNorm/beta' f32 [256], on the device. fp32
  single-scale nets only. Does not synchronise."""
  op = net.pointwise_operand(LAYER)
  logits, values, bad, scales = HT._net_losses(net, gt, weights, reduction, ignore_label)
  raw = HT.heads_weight_grads(net.decoder_out, logits, gt, scales, ignore_label=ignore_label)
  grads = {}
  for head in HT.HEADS:
    dW, db = raw[head]
    wname, bname = HT.variable_names(head)
    grads[wname] = dW.view(1, 1, dW.shape[0], dW.shape[1])
    grads[bname] = db
  G = HT.heads_input_grad(logits, gt, scales, variables, relu_of=net.decoder_out,
                          ignore_label=ignore_label)
  w, bn = _layer_inputs(net, variables)
  a = op['a'].view(-1, op['a'].shape[-1])[:, :op['k']] if op['lda'] != op['k'] else op['a']
  layer = pointwise_weight_grads(a, G, w, bn=bn, eps=op['eps'], a_h2=op['a_h2'])
  for short, t in layer.items():
    grads[LAYER + '/' + short] = t
  return values, bad, grads


def gradient_rule(name, last_layer_gradient_multiplier=1.0, weight_decay=4e-5,
                  last_layers_contain_logits_only=False):
  """(gradient multiplier, l2 decay) of a variable by its name, as the reference's trainer sets
  them and heads_train.HeadsOptimizer applies them to the logits layers: variables of a last
  layer get m = last_layer_gradient_multiplier, its biases 2 m, other biases 2, everything else
  1 (train_utils.py:84-114); with last_layers_contain_logits_only=False, the reference's
  default, every scope above the backbone -- `decoder` among them -- is a last layer, with True
  the logits only. The l2 regulariser is on `weights` alone (model.py:96): gamma, beta and
  biases carry none."""
  m = float(last_layer_gradient_multiplier)
  scopes = ('logits',) if last_layers_contain_logits_only else LAST_LAYER_SCOPES
  last = any(s in name for s in scopes)
  mult = (m if last else 1.0) * (2.0 if 'biases' in name else 1.0)
  return mult, (float(weight_decay) if name.endswith('/weights') else 0.0)


class DecoderOptimizer(object):
  """heads_train.HeadsOptimizer's contract over the nine variables: fp32 master copies on the
  device of the six logits variables and of decoder/decoder_conv1_pointwise/{weights,
  BatchNorm/gamma, BatchNorm/beta}, momentum accumulators of the trainable ones, restored from
  '<name>/Momentum' entries when present (absent: zeros). trainable: the names that step()
  updates (default: all nine) -- --freeze_regex_list filters per variable name
  (train.py:369-371); a frozen variable keeps its bytes and has no accumulator.
  step(grads) applies heads_train.momentum_step per trainable variable with gradient_rule's
  multiplier and decay. `params` is what EposNet.set_layer_weights takes."""

  def __init__(self, variables, lr, momentum=0.9, weight_decay=4e-5,
               last_layer_gradient_multiplier=1.0, last_layers_contain_logits_only=False,
               trainable=None, device=None):
    import torch
    if not torch.cuda.is_available():
      raise EposError('the optimiser needs a HIP device (there is no CPU fallback)')
    _lib.load()
    self.device = torch.device(device if device is not None else 'cuda:0')
    self.lr, self.momentum = float(lr), float(momentum)
    self.trainable = tuple(n for n in VARIABLES if trainable is None or n in trainable)
    unknown = sorted(set(trainable or ()) - set(VARIABLES))
    if unknown:
      raise ValueError('not a variable this optimiser holds: %s' % ', '.join(unknown))
    self.rules = {n: gradient_rule(n, last_layer_gradient_multiplier, weight_decay,
                                   last_layers_contain_logits_only) for n in VARIABLES}
    self.params, self.accums = {}, {}
    for name in VARIABLES:
      if name not in variables:
        raise KeyError('variables lack %r' % name)
      v = torch.as_tensor(variables[name]).to(device=self.device, dtype=torch.float32)
      self.params[name] = v.contiguous().clone()
      if name not in self.trainable:
        continue
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
    """One update of every trainable variable from grads (as net_decoder_grads returns them).
    lr overrides the constructor's for this step."""
    lr = self.lr if lr is None else float(lr)
    for name in self.trainable:
      param, g = self.params[name], grads[name]
      if g.numel() != param.numel():
        raise ValueError('%s: gradient of %d values, variable of %d' % (
            name, g.numel(), param.numel()))
      mult, decay = self.rules[name]
      HT.momentum_step(param, self.accums[name], g.contiguous().view(param.shape), lr,
                       self.momentum, decay, mult)

  def state(self, with_slots=True):
    """{variable name: numpy array} for tf_checkpoint.write_checkpoint: the nine variables and,
    with_slots, the '<name>/Momentum' accumulators of the trainable ones. Synchronises."""
    out = {name: p.cpu().numpy() for name, p in self.params.items()}
    if with_slots:
      for name, a in self.accums.items():
        out[name + '/Momentum'] = a.cpu().numpy()
    return out


def train_step_decoder(net, images, gt, opt, lr, weights=(1.0, 1.0, 100.0), reduction='pooled',
                       augment=None, step=None):
  """heads_train.train_step with decoder/decoder_conv1_pointwise unfrozen, enqueued on the
  current stream without a synchronisation: net.forward_logits(images, use_graph=True),
  net_decoder_grads with opt.params (the weights that forward ran on), opt.step(grads, lr),
  net.set_layer_weights(opt.params, check=False) -- one grouped pack call for the logits layers
  and the layer. augment and step as for train_step. Returns (values f64 [4], bad i64 [B],
  status i32): the losses of THIS step's forward and the bad-pixel counts, and
  set_layer_weights' status words -- non-zero when the packer refused the updated weights and
  the net kept ALL its previous ones."""
  import torch
  if not torch.cuda.is_available():
    raise EposError('train_step_decoder needs a HIP device (there is no CPU fallback)')
  if augment is not None:
    if step is None:
      raise ValueError('train_step_decoder: augment needs the global step its draws are keyed by')
    net.set_images(images)
    augment.apply(net.images, step)
    images = None
  net.forward_logits(images, use_graph=True)
  values, bad, grads = net_decoder_grads(net, gt, opt.params, weights, reduction)
  opt.step(grads, lr)
  status = net.set_layer_weights(opt.params, check=False)
  return values, bad, status
