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
  decoder_conv1_grads  net_grads' nine gradients plus the backward pass through the separable
                  conv decoder_conv1, down to decoder_conv0_pointwise's pre-activation.
  decoder_grads   decoder_conv1_grads plus the backward pass through decoder_conv0, the split of
                  the decoder's concat, feature_projection0 and the decoder's resize, down to
                  concat_projection's pre-activation at the encoder's size.
  aspp_grads      decoder_grads plus the backward pass through concat_projection and ASPP's five
                  branches, joined at the encoder output's pre-activation.
  learning_rate   the reference's schedules (train_utils.py:117-195) in Python floats.

The kernels' wrappers are epos_amd/heads_train.py (the logits layers' weight and input
gradients, the momentum step) and epos_amd/decoder_train.py (the weight and batch-norm
gradients of decoder_conv1_pointwise); the loop itself, its checkpoints and its logging are
train_heads.py; augmentation is epos_amd/augment.py, applied between the upload and the
forward pass. decoder_conv1_grads runs the whole backward pass of the separable conv
decoder_conv1 -- the input gradient of decoder_conv1_pointwise, the weight, batch-norm and input
gradients of decoder_conv1_depthwise -- and returns the gradient at decoder_conv0_pointwise's
pre-activation; decoder_grads goes on through the rest of the decoder ("Losses",
"Backward through the decoder") and returns the gradient at concat_projection's pre-activation;
aspp_grads goes on through ASPP ("Backward through ASPP") and returns the gradient at the
pre-activation of the backbone's last layer.
Not built: the in-place update of any depthwise layer's weights (its folded
weights set the bound gain / bias0 that the plan and its captured graphs hold by value: an
update needs a design for that bound); training the four layers below decoder_conv1, whose
gradients decoder_grads computes (they are rows of weights.POINTWISE_CHAIN_LAYERS and
DEPTHWISE_CHAIN_LAYERS, not of TRAINABLE_LAYERS), or ASPP's (weights.aspp_layers); the
backbone, everything below the encoder output's pre-activation; batch-norm
statistics, bf16 mode, multi-scale nets and more than one device. A
ground truth with the k nearest fragments per pixel (the reference's gt_knn_frags; loss.Batch
reads k from its shapes) goes through every entry here unchanged. A
further trained layer is a row of
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
  values, bad, by_layer, _ = _grads_above(net, gt, variables, DT.LAYER in trainable_layers,
                                         weights, reduction, ignore_label)
  return values, bad, _checkpoint_names(by_layer)


def _grads_above(net, gt, variables, layer, weights, reduction, ignore_label):
  """What net_grads and decoder_conv1_grads share: the losses and the logits layers' weight
  gradients and, with `layer`, heads_input_grad(relu_of=decoder_out) and the weight gradients of
  decoder_conv1_pointwise on the net's own A. Returns (values, bad, {scope: {short name:
  gradient}}, None or (G, A, the layer's operand, its weights, its (gamma, mean, variance)))."""
  op = net.pointwise_operand(DT.LAYER) if layer else None
  logits, values, bad, scales = HT._net_losses(net, gt, weights, reduction, ignore_label)
  raw = HT.heads_weight_grads(net.decoder_out, logits, gt, scales, ignore_label=ignore_label)
  by_layer = {'logits/' + head: dict(zip(W.layer_variables('logits/' + head), raw[head]))
              for head in HT.HEADS}
  if not layer:
    return values, bad, by_layer, None
  G = HT.heads_input_grad(logits, gt, scales, variables, relu_of=net.decoder_out,
                          ignore_label=ignore_label)
  w, bn = DT._layer_inputs(net, variables)
  a = op['a'].view(-1, op['a'].shape[-1])[:, :op['k']] if op['lda'] != op['k'] else op['a']
  by_layer[DT.LAYER] = DT.pointwise_weight_grads(a, G, w, bn=bn, eps=op['eps'],
                                                 a_h2=op['a_h2'])
  return values, bad, by_layer, (G, a, op, w, bn)


def _checkpoint_names(by_layer):
  """{'<scope>/<short name>': gradient} in the checkpoint's layout: matrices as [1,1,K,N]."""
  grads = {}
  for scope, by_short in by_layer.items():
    for short, t in by_short.items():
      grads[scope + '/' + short] = t.view(1, 1, *t.shape) if t.dim() == 2 else t
  return grads


def decoder_conv1_grads(net, gt, variables, weights=(1.0, 1.0, 100.0), reduction='pooled',
                        ignore_label=255):
  """The whole backward pass of the separable conv decoder_conv1: call after
  net.forward_logits(). variables as net_grads takes them, with all four layers of
  weights.TRAINABLE_LAYERS; the depthwise layer's three variables and its statistics come from
  `variables` where given, otherwise from the copy of the net's checkpoint that it keeps on the
  device (EposNet.depthwise_constants). Runs the losses and the logits
  layers' weight gradients as net_grads does, then
    heads_input_grad(relu_of=decoder_out)          G, at decoder_conv1_pointwise's pre-activation
    pointwise_weight_grads                         that layer's dW, dgamma, dbeta
    pointwise_input_grad(relu_of=the net's own A)  D, at decoder_conv1_depthwise's pre-activation
                                                   (the mask: fp16 pairs or fp32, as the plan has it)
    depthwise_weight_grads                         that layer's dw, dgamma, dbeta
    depthwise_input_grad(relu_of=x)                d_in
  Returns (values, bad, grads, d_in): values, bad and the nine gradients as net_grads returns
  them, byte for byte, plus 'decoder/decoder_conv1_depthwise/depthwise_weights' f32 [3,3,C,1],
  '.../BatchNorm/gamma' and '.../BatchNorm/beta' f32 [C]; d_in f32 [B,h,w,C]: the gradient at
  decoder_conv0_pointwise's pre-activation, the G that pointwise_weight_grads takes for that
  layer. The gradients of the depthwise layer are for inspection and for a trainer to come:
  Optimizer and EposNet.set_weights do not take them. fp32 single-scale nets only. Does not
  synchronise."""
  values, bad, by_layer, d_in = _conv1_chain(net, gt, variables, weights, reduction, ignore_label)
  return values, bad, _checkpoint_names(by_layer), d_in


def _conv1_chain(net, gt, variables, weights, reduction, ignore_label):
  """decoder_conv1_grads before the gradients get their checkpoint names: (values, bad, {scope:
  {short name: gradient}}, d_in). decoder_grads goes on from here."""
  dw = net.depthwise_operand(DT.DEPTHWISE_LAYER)
  values, bad, by_layer, (G, a, op, w, bn) = _grads_above(net, gt, variables, True, weights,
                                                          reduction, ignore_label)
  D = DT.pointwise_input_grad(G, w, bn=(bn[0], bn[2]), eps=op['eps'], relu_of=a,
                              relu_of_h2=op['presplit'])
  x = dw['x'][..., :dw['c']]
  D4 = D.view(dw['b'], dw['h'], dw['w'], dw['c'])
  dww, dbn = DT._depthwise_inputs(net, variables)
  by_layer[DT.DEPTHWISE_LAYER] = DT.depthwise_weight_grads(x, D4, dww, dbn, dw['eps'],
                                                           rate=dw['rate'])
  d_in = DT.depthwise_input_grad(D4, dw['w9c'], rate=dw['rate'], relu_of=x)
  return values, bad, by_layer, d_in


def decoder_grads(net, gt, variables, weights=(1.0, 1.0, 100.0), reduction='pooled',
                  ignore_label=255):
  """The backward pass through the whole decoder: call after net.forward_logits(). variables as
  decoder_conv1_grads takes them; the variables and statistics of the four layers below
  (weights.POINTWISE_CHAIN_LAYERS, weights.DEPTHWISE_CHAIN_LAYERS) come from `variables` where
  given, otherwise from the copies of its checkpoint the net keeps on the device
  (EposNet.pointwise_constants, crossed_depthwise_constants). Runs what decoder_conv1_grads runs, then,
  with G0 = its d_in and A0 = the net's own output of decoder_conv0_depthwise (fp16 pairs or
  fp32, as the plan has it),
    pointwise_weight_grads(A0, G0)                 decoder_conv0_pointwise's dW, dgamma, dbeta
    pointwise_input_grad(G0, relu_of=A0)           D0 [M,304], at decoder_conv0_depthwise's
                                                   pre-activation
    depthwise_weight_grads(decoder_concat, D0)     that layer's dw, dgamma, dbeta
    depthwise_input_grad, channels 0:256           the gradient at the resize's output: NO mask,
                                                   behind it lies the resize and not a ReLU
    depthwise_input_grad, channels 256:304,        the gradient at feature_projection0's
      relu_of=decoder_concat[..., 256:]            pre-activation
    pointwise_weight_grads(the low-level tap, that 48-wide slice at row stride 304)
                                                   feature_projection0's dW, dgamma, dbeta
    resize_input_grad(channels 0:256, (eh, ew), relu_of=concat_projection)
                                                   d_proj [B,eh,ew,256]
    pointwise_weight_grads(aspp_concat, d_proj)    concat_projection's dW, dgamma, dbeta (K = 1280)
  Returns (values, bad, grads, d_proj): values, bad and the twelve gradients of
  decoder_conv1_grads byte for byte, plus the twelve new ones under their checkpoint names
  (matrices [1,1,K,N], 'decoder/decoder_conv0_depthwise/depthwise_weights' [3,3,304,1]); d_proj:
  the gradient at concat_projection's pre-activation, at the encoder's size -- the G from which
  ASPP and the backbone start. The new gradients are for inspection and for a trainer to come:
  Optimizer and EposNet.set_weights do not take them. fp32 single-scale nets whose low-level
  features already have the decoder's size. Copies nothing from the host and does not
  synchronise when `variables` holds device tensors, or none of the new names."""
  values, bad, by_layer, d_proj, _ = _decoder_chain(net, gt, variables, weights, reduction,
                                                    ignore_label)
  return values, bad, _checkpoint_names(by_layer), d_proj


def _decoder_chain(net, gt, variables, weights, reduction, ignore_label):
  """decoder_grads before the gradients get their checkpoint names: (values, bad, {scope: {short
  name: gradient}}, d_proj, (concat_projection's record, weights, (gamma, mean, variance))).
  aspp_grads goes on from here."""
  import torch
  ch = net.chain_operands()
  if ch['low_level_hw'] != ch['decoder_hw']:
    raise EposError('decoder_grads: the low-level features (%dx%d) are resized to the decoder\'s '
                    'size (%dx%d); that resize has no backward pass here' % (
                        ch['low_level_hw'] + ch['decoder_hw']))
  op0 = net.crossed_pointwise_operand(W.DECODER_CONV0_POINTWISE)
  opf = net.crossed_pointwise_operand(W.FEATURE_PROJECTION0)
  opc = net.crossed_pointwise_operand(W.CONCAT_PROJECTION)
  dw = net.crossed_depthwise_operand(W.DECODER_CONV0_DEPTHWISE)
  values, bad, by_layer, d_in = _conv1_chain(net, gt, variables, weights, reduction, ignore_label)

  def rows_of(op):
    return op['a'].view(-1, op['a'].shape[-1])[:, :op['k']] if op['lda'] != op['k'] else op['a']

  G0 = d_in.view(-1, d_in.shape[-1])
  a0 = rows_of(op0)
  w0, bn0 = DT._crossed_inputs(net, variables, W.DECODER_CONV0_POINTWISE)
  by_layer[W.DECODER_CONV0_POINTWISE] = DT.pointwise_weight_grads(
      a0, G0, w0, bn=bn0, eps=op0['eps'], a_h2=op0['a_h2'])
  D0 = DT.pointwise_input_grad(G0, w0, bn=(bn0[0], bn0[2]), eps=op0['eps'], relu_of=a0,
                               relu_of_h2=op0['presplit'])
  B, h, w, c = dw['b'], dw['h'], dw['w'], dw['c']
  x = dw['x'][..., :c]
  D4 = D0.view(B, h, w, c)
  dww, dbn = DT._depthwise_inputs(net, variables, W.DECODER_CONV0_DEPTHWISE)
  by_layer[W.DECODER_CONV0_DEPTHWISE] = DT.depthwise_weight_grads(x, D4, dww, dbn, dw['eps'],
                                                                  rate=dw['rate'])
  n = ch['concat_projection'].shape[-1]                # 256: where the concat is split
  d_cat = torch.empty((B, h, w, c), dtype=torch.float32, device=d_in.device)
  DT.depthwise_input_grad(D4[..., :n], dw['w9c'][:, :n].contiguous(), rate=dw['rate'],
                          out=d_cat[..., :n])
  DT.depthwise_input_grad(D4[..., n:], dw['w9c'][:, n:].contiguous(), rate=dw['rate'],
                          relu_of=x[..., n:], out=d_cat[..., n:])
  wf, bnf = DT._crossed_inputs(net, variables, W.FEATURE_PROJECTION0)
  by_layer[W.FEATURE_PROJECTION0] = DT.pointwise_weight_grads(
      rows_of(opf), d_cat[..., n:], wf, bn=bnf, eps=opf['eps'], a_h2=opf['a_h2'])
  d_proj = DT.resize_input_grad(d_cat[..., :n], ch['encoder_hw'],
                                relu_of=ch['concat_projection'])
  wc, bnc = DT._crossed_inputs(net, variables, W.CONCAT_PROJECTION)
  by_layer[W.CONCAT_PROJECTION] = DT.pointwise_weight_grads(
      rows_of(opc), d_proj, wc, bn=bnc, eps=opc['eps'], a_h2=opc['a_h2'])
  return values, bad, by_layer, d_proj, (opc, wc, bnc)


def aspp_grads(net, gt, variables, weights=(1.0, 1.0, 100.0), reduction='pooled',
               ignore_label=255):
  """The backward pass through the decoder and ASPP, down to the encoder output: call after
  net.forward_logits(). variables as decoder_grads takes them; the variables and statistics of
  ASPP's layers (weights.aspp_layers) come from `variables` where given, otherwise from the
  copies of its checkpoint the net keeps on the device (EposNet.aspp_constants). Runs what
  decoder_grads runs, then, with the records of EposNet.aspp_operands, M = B eh ew rows and Wc
  = concat_projection's weights,
    pointwise_input_grad(d_proj, Wc, relu_of=aspp_concat)   D_cat [M, 256 (2 + rates)]: slice s
                                                   is the gradient at branch s's pre-activation
                                                   (slice 0's mask is the broadcast pool_feat)
    pool_broadcast_grad(D_cat[..., 0:256])         g_pool [B,256]
    pointwise_weight_grads(pooled, g_pool)         image_pooling's dW, dgamma, dbeta (B rows)
    pointwise_input_grad(g_pool), no mask          d_pooled [B,ec]
    pointwise_weight_grads(encoder, slice 1)       aspp0's three
    pointwise_input_grad(slice 1), no mask         E0 [M,ec]
    per rate i, with a_i = the net's own output of aspp<i>_depthwise (fp16 pairs or fp32):
      pointwise_weight_grads(a_i, slice i+1)       aspp<i>_pointwise's three
      pointwise_input_grad(slice i+1, relu_of=a_i) D_i [M,ec]
      depthwise_weight_grads(encoder, D_i, rate)   aspp<i>_depthwise's three
    aspp_join_grad(depthwise=[(D_i, w9c_i, r_i)], plain=[E0], pooled=(d_pooled, eh ew),
                   relu_of=encoder where it lies behind a ReLU)        d_enc [B,eh,ew,ec]
  Returns (values, bad, grads, d_enc): values, bad and the 24 gradients of decoder_grads byte
  for byte, plus the 3 (2 + 2 len(rates)) new ones under their checkpoint names (matrices
  [1,1,K,N], depthwise weights [3,3,ec,1]); d_enc: the gradient at the pre-activation of the
  backbone's last layer. The new gradients are for inspection and for a trainer to come:
  Optimizer and EposNet.set_weights do not take them. fp32 single-scale nets only. Copies
  nothing from the host and does not synchronise when `variables` holds device tensors, or
  none of the new names."""
  ap = net.aspp_operands()
  values, bad, by_layer, d_proj, (opc, wc, bnc) = _decoder_chain(net, gt, variables, weights,
                                                                 reduction, ignore_label)
  enc, rates = ap['encoder'], ap['rates']
  B, eh, ew, ec = (int(v) for v in enc.shape)
  cat = ap['aspp_concat']
  D_cat = DT.pointwise_input_grad(d_proj.view(-1, d_proj.shape[-1]), wc, bn=(bnc[0], bnc[2]),
                                  eps=opc['eps'], relu_of=cat, relu_of_h2=opc['presplit'])
  D_cat = D_cat.view(B, eh, ew, -1)

  def inputs(scope, depthwise=False):
    return DT._given_or_kept(net, variables, scope, net.aspp_constants(scope),
                             ('depthwise_weights' if depthwise else 'weights',
                              'BatchNorm/gamma'))

  def rows_of(op):
    return op['a'].view(-1, op['a'].shape[-1])[:, :op['k']] if op['lda'] != op['k'] else op['a']

  def branch(s):                                       # slice s of the concat's gradient
    return D_cat[..., 256 * s:256 * (s + 1)]

  op = ap['pointwise'][W.IMAGE_POOLING]
  w, bn = inputs(W.IMAGE_POOLING)
  g_pool = DT.pool_broadcast_grad(branch(0))
  by_layer[W.IMAGE_POOLING] = DT.pointwise_weight_grads(rows_of(op), g_pool, w, bn=bn,
                                                        eps=op['eps'], a_h2=op['a_h2'])
  d_pooled = DT.pointwise_input_grad(g_pool, w, bn=(bn[0], bn[2]), eps=op['eps'])
  op = ap['pointwise'][W.ASPP0]
  w, bn = inputs(W.ASPP0)
  by_layer[W.ASPP0] = DT.pointwise_weight_grads(rows_of(op), branch(1), w, bn=bn, eps=op['eps'],
                                                a_h2=op['a_h2'])
  E0 = DT.pointwise_input_grad(branch(1), w, bn=(bn[0], bn[2]), eps=op['eps'])
  terms = []
  for i, rate in enumerate(rates, 1):
    pw, dws = 'aspp%d_pointwise' % i, 'aspp%d_depthwise' % i
    op, dw = ap['pointwise'][pw], ap['depthwise'][dws]
    w, bn = inputs(pw)
    a = rows_of(op)
    by_layer[pw] = DT.pointwise_weight_grads(a, branch(i + 1), w, bn=bn, eps=op['eps'],
                                             a_h2=op['a_h2'])
    D = DT.pointwise_input_grad(branch(i + 1), w, bn=(bn[0], bn[2]), eps=op['eps'], relu_of=a,
                                relu_of_h2=op['presplit']).view(B, eh, ew, ec)
    dww, dbn = inputs(dws, depthwise=True)
    by_layer[dws] = DT.depthwise_weight_grads(enc, D, dww, dbn, dw['eps'], rate=dw['rate'])
    terms.append((D, dw['w9c'], dw['rate']))
  d_enc = DT.aspp_join_grad(depthwise=terms, plain=[E0], pooled=(d_pooled, eh * ew),
                            relu_of=enc if ap['encoder_relu'] else None)
  return values, bad, _checkpoint_names(by_layer), d_enc


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
