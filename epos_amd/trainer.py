"""The trainer above the gradient kernels ("Losses", "Weight gradients", "Decoder
layer gradients"): which variables are trained is data -- the layers of weights.TRAINABLE_LAYERS,
any subset of their variables -- not a choice between code paths.

  gradient_rule   the reference's multiplier and l2 decay of a variable, by its name.
  Optimizer       fp32 master copies and momentum accumulators on the device; restores the
                  accumulators from '<name>/Momentum' entries, so that a run can resume.
  net_grads       from a net that has run forward_logits to checkpoint-named gradients of the
                  variables the optimiser holds.
  train_step      one step of the loop: forward_logits -> net_grads -> Optimizer.step ->
                  EposNet.set_weights (the device weight packer, csrc/weight_pack.hip: the
                  updated weights reach the built net, its captured graphs included, without a
                  round trip through the host).
  learning_rate   the reference's schedules (train_utils.py:117-195) in Python floats.

The kernels' wrappers are epos_amd/heads_train.py (the logits layers' weight and input
gradients, the momentum step) and epos_amd/decoder_train.py (the weight and batch-norm
gradients of decoder_conv1_pointwise); the loop itself, its checkpoints and its logging are
train_heads.py; augmentation is epos_amd/augment.py, applied between the upload and the
forward pass. Not built: backpropagation from decoder_conv1_depthwise down, which starts with
the input gradient G W^T of decoder_conv1_pointwise; batch-norm statistics, bf16 mode,
multi-scale nets and more than one device. A further trained layer is a row of
weights.TRAINABLE_LAYERS, its gradient kernel's wrapper and a clause in net_grads.

Parity with TensorFlow's numbers is unpinned -- that holds for learning_rate too: TensorFlow
evaluates the schedules in float32, this module in Python floats. There is no CPU fallback:
without the library or a device the entries raise EposError.
"""
import math

from epos_amd import _lib
from epos_amd._lib import EposError
from epos_amd import decoder_train as DT
from epos_amd import heads_train as HT
from epos_amd import weights as W

VARIABLES = W.trainable_variables()
# model.py: get_extra_layer_scopes(last_layers_contain_logits_only=False) -- every scope above
# the backbone counts as a last layer (train_utils.py:84-114 tests `scope in variable name`)
LAST_LAYER_SCOPES = ('logits', 'image_pooling', 'aspp', 'concat_projection', 'decoder',
                     'meta_architecture')


def gradient_rule(name, last_layer_gradient_multiplier=1.0, weight_decay=4e-5,
                  last_layers_contain_logits_only=False):
  """(gradient multiplier, l2 decay) of a variable by its name, as the reference's trainer sets
  them: variables of a last layer get m = last_layer_gradient_multiplier, its biases 2 m, other
  biases 2, everything else 1 (train_utils.py:84-114); with
  last_layers_contain_logits_only=False, the reference's default, every scope above the backbone
  -- `decoder` among them -- is a last layer, with True the logits only. The l2 regulariser is on
  `weights` alone (model.py:96): gamma, beta and biases carry none."""
  m = float(last_layer_gradient_multiplier)
  scopes = ('logits',) if last_layers_contain_logits_only else LAST_LAYER_SCOPES
  last = any(s in name for s in scopes)
  mult = (m if last else 1.0) * (2.0 if 'biases' in name else 1.0)
  return mult, (float(weight_decay) if name.endswith('/weights') else 0.0)


class Optimizer(object):
  """fp32 master copies on the device of the six logits variables and of the variables of every
  other weights.TRAINABLE_LAYERS layer that has a trainable variable, and momentum accumulators
  of the trainable ones. variables: {checkpoint name: numpy array or tensor} and, optionally,
  the accumulators '<name>/Momentum' as state() and the trainer's checkpoints hold them (absent:
  zeros); other keys are ignored. trainable: the names that step() updates (default: the six
  logits variables) -- --freeze_regex_list filters per variable name (train.py:369-371); a
  frozen variable keeps its bytes and has no accumulator. `layers` are the scopes held;
  step(grads) applies heads_train.momentum_step per trainable variable with gradient_rule's
  multiplier and decay. `params` is what EposNet.set_weights takes."""

  def __init__(self, variables, lr, momentum=0.9, weight_decay=4e-5,
               last_layer_gradient_multiplier=1.0, last_layers_contain_logits_only=False,
               trainable=None, device=None):
    import torch
    if not torch.cuda.is_available():
      raise EposError('the optimiser needs a HIP device (there is no CPU fallback)')
    _lib.load()
    self.device = torch.device(device if device is not None else 'cuda:0')
    self.lr, self.momentum = float(lr), float(momentum)
    if trainable is None:
      trainable = W.trainable_variables(W.LOGITS_LAYERS)
    unknown = sorted(set(trainable) - set(VARIABLES))
    if unknown:
      raise ValueError('not a variable this optimiser holds: %s' % ', '.join(unknown))
    self.trainable = tuple(n for n in VARIABLES if n in trainable)
    self.layers = tuple(s for s in W.TRAINABLE_LAYERS if s in W.LOGITS_LAYERS or
                        any(n in trainable for n in W.trainable_variables((s,))))
    held = W.trainable_variables(self.layers)
    self.rules = {n: gradient_rule(n, last_layer_gradient_multiplier, weight_decay,
                                   last_layers_contain_logits_only) for n in held}
    self.params, self.accums = {}, {}
    for name in held:
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
    """One update of every trainable variable from grads (as net_grads returns them). lr
    overrides the constructor's for this step (the schedules are the caller's)."""
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
    """{variable name: numpy array} for tf_checkpoint.write_checkpoint: the variables held and,
    with_slots, the '<name>/Momentum' accumulators of the trainable ones. Synchronises."""
    out = {name: p.cpu().numpy() for name, p in self.params.items()}
    if with_slots:
      for name, a in self.accums.items():
        out[name + '/Momentum'] = a.cpu().numpy()
    return out


def net_grads(net, gt, variables, trainable_layers=W.LOGITS_LAYERS, weights=(1.0, 1.0, 100.0),
              reduction='pooled', ignore_label=255):
  """From a running network to checkpoint-named gradients: call after net.forward_logits().
  variables: the variables the net currently runs on (Optimizer.params); trainable_layers: the
  scopes whose gradients are wanted (Optimizer.layers), the three logits layers always among
  them. Runs loss_terms -> loss_values once, then heads_weight_grads on net.decoder_out and the
  net's logits, and, only with decoder/decoder_conv1_pointwise among trainable_layers,
  heads_input_grad(relu_of=net.decoder_out) with the logits weights of `variables` and
  pointwise_weight_grads on the net's own A (EposNet.pointwise_operand: fp16 pairs by default)
  with the layer's weights and gamma. Returns (values f64 [4], bad i64 [B], grads): values and
  bad as loss.differentiable_losses returns them, grads = {'<scope>/weights': f32 [1,1,K,N],
  '<scope>/biases' or '<scope>/BatchNorm/gamma', '/BatchNorm/beta': f32 [N]} on the device for
  every variable of trainable_layers. fp32 single-scale nets only. Does not synchronise."""
  layer = DT.LAYER in trainable_layers
  op = net.pointwise_operand(DT.LAYER) if layer else None
  logits, values, bad, scales = HT._net_losses(net, gt, weights, reduction, ignore_label)
  raw = HT.heads_weight_grads(net.decoder_out, logits, gt, scales, ignore_label=ignore_label)
  by_layer = {'logits/' + head: dict(zip(W.layer_variables('logits/' + head), raw[head]))
              for head in HT.HEADS}
  if layer:
    G = HT.heads_input_grad(logits, gt, scales, variables, relu_of=net.decoder_out,
                            ignore_label=ignore_label)
    w, bn = DT._layer_inputs(net, variables)
    a = op['a'].view(-1, op['a'].shape[-1])[:, :op['k']] if op['lda'] != op['k'] else op['a']
    by_layer[DT.LAYER] = DT.pointwise_weight_grads(a, G, w, bn=bn, eps=op['eps'],
                                                   a_h2=op['a_h2'])
  grads = {}
  for scope, by_short in by_layer.items():
    for short, t in by_short.items():            # the checkpoint's layout: matrices as [1,1,K,N]
      grads[scope + '/' + short] = t.view(1, 1, *t.shape) if t.dim() == 2 else t
  return values, bad, grads


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
  """One training step of the variables opt holds, enqueued on the current stream without a
  synchronisation: net.forward_logits(images, use_graph=True), net_grads with opt.params (the
  weights that forward ran on) and opt.layers, opt.step(grads, lr), net.set_weights(opt.params,
  check=False) -- one grouped pack call for all the layers held. With augment (an
  augment.Augmenter) the images are uploaded first (net.set_images), augmented in place on the
  device with the draws of global step `step` (augment.apply(net.images, step)) and the forward
  pass reads them there. Returns (values f64 [4], bad i64 [B], status i32): the losses of THIS
  step's forward (before its update) and the bad-pixel counts as loss.differentiable_losses
  returns them, and set_weights' status words -- non-zero when the packer refused the updated
  weights and the net kept ALL its previous ones. The caller reads them when it chooses."""
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
  values, bad, grads = net_grads(net, gt, opt.params, opt.layers, weights, reduction)
  opt.step(grads, lr)
  status = net.set_weights(opt.params, check=False)
  return values, bad, status
