"""Weight containers for the EPOS network.

A *checkpoint* here is a plain ``dict`` keyed by the reference's TensorFlow
variable names (scopes from net_xception.py:176,181,295,302,
372-376, model.py:20-22,224,237,242,89,97,258,324,352,376,383,440-456) holding
numpy arrays in TF layout (conv ``weights`` HWIO, ``depthwise_weights``
[3,3,C,1], BatchNorm ``gamma/beta/moving_mean/moving_variance``, ``biases``).
It can be stored as an ``.npz``.

``variable_specs`` enumerates every variable of a model; ``random_init`` draws
them with the reference's initialisers (used for synthetic benchmarks and tests
-- there is no network access for the released checkpoints).
"""
import numpy as np

RESNET101_BLOCKS = [  # net_resnet_v1_beta.py:494-505: (scope, base depth, units)
    ('block1', 64, 3), ('block2', 128, 4), ('block3', 256, 23), ('block4', 512, 3),
]

# The other backbones of feature.py:118-129 (networks_map) that share ASPP, decoder and heads.
# Xception tables: (scope, depths, skip, act_in_sep, units, stride) -- net_xception.py:526-590
# (xception_41), :604-648 (xception_65), :660-738 (xception_71); exit_flow/block2 takes the
# multi_grid unit rates.
_XCEPTION_EXIT = [
    ('exit_flow/block1', [728, 1024, 1024], 'conv', False, 1, 2),
    ('exit_flow/block2', [1536, 1536, 2048], 'none', True, 1, 1),
]
XCEPTION_TABLES = {
    'xception_41': [
        ('entry_flow/block1', [128, 128, 128], 'conv', False, 1, 2),
        ('entry_flow/block2', [256, 256, 256], 'conv', False, 1, 2),
        ('entry_flow/block3', [728, 728, 728], 'conv', False, 1, 2),
        ('middle_flow/block1', [728, 728, 728], 'sum', False, 8, 1)] + _XCEPTION_EXIT,
    'xception_65': [
        ('entry_flow/block1', [128, 128, 128], 'conv', False, 1, 2),
        ('entry_flow/block2', [256, 256, 256], 'conv', False, 1, 2),
        ('entry_flow/block3', [728, 728, 728], 'conv', False, 1, 2),
        ('middle_flow/block1', [728, 728, 728], 'sum', False, 16, 1)] + _XCEPTION_EXIT,
    'xception_71': [
        ('entry_flow/block1', [128, 128, 128], 'conv', False, 1, 2),
        ('entry_flow/block2', [256, 256, 256], 'conv', False, 1, 1),
        ('entry_flow/block3', [256, 256, 256], 'conv', False, 1, 2),
        ('entry_flow/block4', [728, 728, 728], 'conv', False, 1, 1),
        ('entry_flow/block5', [728, 728, 728], 'conv', False, 1, 2),
        ('middle_flow/block1', [728, 728, 728], 'sum', False, 16, 1)] + _XCEPTION_EXIT,
}

RESNET50_BLOCKS = [  # net_resnet_v1_beta.py:278-289, :351-362
    ('block1', 64, 3), ('block2', 128, 4), ('block3', 256, 6), ('block4', 512, 3),
]

MEAN_RGB = (123.15, 115.90, 103.06)   # feature.py:154 (_MEAN_RGB)

# model_variant -> how the backbone is built:
#   family      'xception' | 'resnet'
#   scope       the network's variable scope (feature.py:140-149, name_scope)
#   blocks      XCEPTION_TABLES entry | RESNET*_BLOCKS
#   root        xception: 3x3 conv1_1 / conv1_2; resnet 'beta': three 3x3 conv1_1..3
#               (net_resnet_v1_beta.py:96-112), 'conv7': one 7x7 stride-2 conv1 (:168-173)
#   preprocess  'unit_range' (2/255) x - 1 | 'sub_mean' x - MEAN_RGB (feature.py:176-185)
#   tap         the block whose unit_1 separable_conv2_pointwise (xception) / unit_2 conv3
#               (resnet) feeds the decoder (feature.py:29-73)
VARIANTS = {
    'xception_41': dict(family='xception', scope='xception_41', root='xception',
                        preprocess='unit_range', tap='entry_flow/block2'),
    'xception_65': dict(family='xception', scope='xception_65', root='xception',
                        preprocess='unit_range', tap='entry_flow/block2'),
    'xception_71': dict(family='xception', scope='xception_71', root='xception',
                        preprocess='unit_range', tap='entry_flow/block3'),
    'resnet_v1_50': dict(family='resnet', scope='resnet_v1_50', root='conv7',
                         preprocess='sub_mean', tap='block1'),
    'resnet_v1_50_beta': dict(family='resnet', scope='resnet_v1_50', root='beta',
                              preprocess='unit_range', tap='block1'),
    'resnet_v1_101': dict(family='resnet', scope='resnet_v1_101', root='conv7',
                          preprocess='sub_mean', tap='block1'),
    'resnet_v1_101_beta': dict(family='resnet', scope='resnet_v1_101', root='beta',
                               preprocess='unit_range', tap='block1'),
}
for _name, _v in VARIANTS.items():
  _v['blocks'] = (XCEPTION_TABLES[_name] if _v['family'] == 'xception' else
                  RESNET50_BLOCKS if '_50' in _name else RESNET101_BLOCKS)


def variant(model_variant):
  """The VARIANTS entry of a model variant; ValueError for the ones this build lacks."""
  if model_variant not in VARIANTS:
    raise ValueError('Unsupported model variant: %s (supported: %s)' % (
        model_variant, ', '.join(sorted(VARIANTS))))
  return VARIANTS[model_variant]


PRED_OBJ_CONF = 'pred_obj_conf'    # common.py:24-27
PRED_OBJ_LABEL = 'pred_obj_label'
PRED_FRAG_CONF = 'pred_frag_conf'
PRED_FRAG_LOC = 'pred_frag_loc'
DECODER_CONV1_POINTWISE = 'decoder/decoder_conv1_pointwise'
# The 1x1 conv layers whose weights a built net replaces in place (EposNet.set_weights) and the
# trainer holds (epos_amd/trainer.py), in the trainer's order: scope -> None for a layer with
# `biases`, or the eps of its frozen batch norm (gamma and beta trained, the statistics inputs;
# model.py:307-312). A layer with a batch norm is folded before it is packed.
TRAINABLE_LAYERS = {
    'logits/' + PRED_OBJ_CONF: None,
    'logits/' + PRED_FRAG_CONF: None,
    'logits/' + PRED_FRAG_LOC: None,
    DECODER_CONV1_POINTWISE: 1e-5,
}
LOGITS_LAYERS = tuple(s for s in TRAINABLE_LAYERS if s.startswith('logits/'))
DECODER_CONV1_DEPTHWISE = 'decoder/decoder_conv1_depthwise'
# The 3x3 depthwise layers the backward pass crosses (trainer.decoder_conv1_grads): scope -> the
# eps of its frozen batch norm. The plan records their operands (EposNet.depthwise_operand).
# NOT trainable layers: a depthwise layer's folded weights set the bound (gain, bias0) that the
# plan bakes into its launches by value, so an in-place update needs a design of its own.
DEPTHWISE_BACKWARD_LAYERS = {DECODER_CONV1_DEPTHWISE: 1e-5}
DEPTHWISE_VARIABLES = ('depthwise_weights', 'BatchNorm/gamma', 'BatchNorm/beta')
# The layers the backward pass crosses below decoder_conv1 (trainer.decoder_grads), in the order
# it meets them, kept in tables of their own beside the two above: their gradients are for
# inspection and for a trainer to come, and nothing here makes them trainable -- Optimizer,
# EposNet.set_weights and the plan's weight packs (Fp32Mode.packs) hold TRAINABLE_LAYERS only.
# scope -> the eps of its frozen batch norm (net.HEAD_BN_EPS). The plan records the operands of
# the 1x1 layers (EposNet.crossed_pointwise_operand, 'packs' None) and of the depthwise layer
# (EposNet.crossed_depthwise_operand); pointwise_operand and depthwise_operand keep answering for
# the two tables above only. ASPP's layers, which depend on the net's atrous rates, are
# aspp_layers() below (trainer.aspp_grads). Not built: training any of these layers, and the
# backbone below the encoder output's pre-activation.
DECODER_CONV0_POINTWISE = 'decoder/decoder_conv0_pointwise'
DECODER_CONV0_DEPTHWISE = 'decoder/decoder_conv0_depthwise'
FEATURE_PROJECTION0 = 'decoder/feature_projection0'
CONCAT_PROJECTION = 'concat_projection'
POINTWISE_CHAIN_LAYERS = {DECODER_CONV0_POINTWISE: 1e-5, FEATURE_PROJECTION0: 1e-5,
                          CONCAT_PROJECTION: 1e-5}
DEPTHWISE_CHAIN_LAYERS = {DECODER_CONV0_DEPTHWISE: 1e-5}
IMAGE_POOLING = 'image_pooling'
ASPP0 = 'aspp0'


def aspp_layers(atrous_rates):
  """({1x1 scope: eps}, {depthwise scope: eps}) of ASPP for a net's atrous rates, in the order of
  the concat's slices: 'image_pooling', 'aspp0', 'aspp1_pointwise', ... and 'aspp1_depthwise',
  ...; eps: that of the frozen batch norm (net.HEAD_BN_EPS). The layers trainer.aspp_grads
  crosses below concat_projection: the plan records their operands (EposNet.aspp_operands), and
  nothing makes them trainable -- the four tables above stay as they are."""
  n = len(tuple(atrous_rates))
  pointwise = {IMAGE_POOLING: 1e-5, ASPP0: 1e-5}
  pointwise.update(('aspp%d_pointwise' % i, 1e-5) for i in range(1, n + 1))
  return pointwise, {'aspp%d_depthwise' % i: 1e-5 for i in range(1, n + 1)}
# a 1x1 conv layer's trained variables by whether it has a batch norm, `weights` first: what is
# given together to EposNet.set_weights and what a gradient wrapper's result is keyed by
CONV_VARIABLES = {False: ('weights', 'biases'),
                  True: ('weights', 'BatchNorm/gamma', 'BatchNorm/beta')}


def layer_variables(scope):
  """The short names of a TRAINABLE_LAYERS layer's variables."""
  return CONV_VARIABLES[TRAINABLE_LAYERS[scope] is not None]


# checkpoint name -> (scope, short name) of every variable of TRAINABLE_LAYERS
TRAINABLE_VARIABLES = {s + '/' + v: (s, v) for s in TRAINABLE_LAYERS for v in layer_variables(s)}


def trainable_variables(scopes=None):
  """The checkpoint names of the variables of `scopes` (default: every TRAINABLE_LAYERS layer),
  in the table's order."""
  return tuple(n for n, (s, _) in TRAINABLE_VARIABLES.items() if scopes is None or s in scopes)


def variable_shapes(short, k, n):
  """The shapes a variable of a K -> N layer may have."""
  return ((1, 1, k, n), (k, n)) if short == 'weights' else ((n,),)


def outputs_to_num_channels(num_objs, num_frags):
  """common.py:189-203 (frag_cls_agnostic=False)."""
  return {
      PRED_OBJ_CONF: num_objs + 1,
      PRED_FRAG_CONF: num_objs * num_frags,
      PRED_FRAG_LOC: num_objs * num_frags * 3,
  }


def variable_specs(model_variant='xception_65', num_objs=21, num_frags=64,
                   atrous_rates=(12, 24, 36)):
  """Returns a list of (kind, scope, shape-info) for every layer.

  kind: 'conv' (weights HWIO + BN), 'dw' (depthwise_weights + BN),
        'logits' (weights + biases). Each entry carries the initializer family:
        'backbone' (trunc-normal 0.09, net_xception.py:745,782-783),
        'head_dw' (0.33) / 'head_pw' (0.06) (model.py:56-57),
        'xavier' (slim default for plain slim.conv2d in model.py),
        'logits' (trunc-normal 0.01, model.py:437).
  """
  specs = []
  v = variant(model_variant)
  net = v['scope']
  if v['family'] == 'xception':
    specs.append(('conv', net + '/entry_flow/conv1_1', (3, 3, 3, 32), 'backbone'))
    specs.append(('conv', net + '/entry_flow/conv1_2', (3, 3, 32, 64), 'backbone'))
    cin = 64
    for bscope, depths, skip, _, units, _ in v['blocks']:
      for u in range(units):
        scope = '%s/%s/unit_%d/xception_module' % (net, bscope, u + 1)
        c = cin
        for i, d in enumerate(depths):
          sc = '%s/separable_conv%d' % (scope, i + 1)
          specs.append(('dw', sc + '_depthwise', (3, 3, c, 1), 'backbone'))
          specs.append(('conv', sc + '_pointwise', (1, 1, c, d), 'backbone'))
          c = d
        if skip == 'conv':
          specs.append(('conv', scope + '/shortcut', (1, 1, cin, depths[-1]),
                        'backbone'))
        cin = depths[-1]
  else:
    # net_resnet_v1_beta.py:96-112 (beta root) or :168-173 (7x7 root), :38-93 (bottleneck),
    # block tables; variable scope from feature.py:140-149 ('resnet_v1_50_beta' ->
    # 'resnet_v1_50').
    if v['root'] == 'beta':
      cin = 3
      for i, cout in enumerate([64, 64, 128], 1):
        specs.append(('conv', '%s/conv1_%d' % (net, i), (3, 3, cin, cout), 'he'))
        cin = cout
    else:
      specs.append(('conv', net + '/conv1', (7, 7, 3, 64), 'he'))
      cin = 64
    for bscope, base, units in v['blocks']:
      for u in range(units):
        scope = '%s/%s/unit_%d/bottleneck_v1' % (net, bscope, u + 1)
        if cin != base * 4:
          specs.append(('conv', scope + '/shortcut', (1, 1, cin, base * 4), 'he'))
        specs.append(('conv', scope + '/conv1', (1, 1, cin, base), 'he'))
        specs.append(('conv', scope + '/conv2', (3, 3, base, base), 'he'))
        specs.append(('conv', scope + '/conv3', (1, 1, base, base * 4), 'he'))
        cin = base * 4
  specs.append(('conv', 'image_pooling', (1, 1, cin, 256), 'xavier'))
  specs.append(('conv', 'aspp0', (1, 1, cin, 256), 'xavier'))
  for i, _ in enumerate(atrous_rates, 1):
    specs.append(('dw', 'aspp%d_depthwise' % i, (3, 3, cin, 1), 'head_dw'))
    specs.append(('conv', 'aspp%d_pointwise' % i, (1, 1, cin, 256), 'head_pw'))
  specs.append(('conv', 'concat_projection',
                (1, 1, 256 * (2 + len(atrous_rates)), 256), 'xavier'))
  specs.append(('conv', 'decoder/feature_projection0', (1, 1, 256, 48),
                'xavier'))
  specs.append(('dw', 'decoder/decoder_conv0_depthwise', (3, 3, 304, 1),
                'head_dw'))
  specs.append(('conv', 'decoder/decoder_conv0_pointwise', (1, 1, 304, 256),
                'head_pw'))
  specs.append(('dw', 'decoder/decoder_conv1_depthwise', (3, 3, 256, 1),
                'head_dw'))
  specs.append(('conv', 'decoder/decoder_conv1_pointwise', (1, 1, 256, 256),
                'head_pw'))
  for name, ch in sorted(outputs_to_num_channels(num_objs, num_frags).items()):
    specs.append(('logits', 'logits/' + name, (1, 1, 256, ch), 'logits'))
  return specs


def _trunc_normal(rng, shape, std):
  """tf.truncated_normal_initializer: resample outside 2 sigma."""
  x = rng.standard_normal(size=shape)
  bad = np.abs(x) > 2.0
  while bad.any():
    x[bad] = rng.standard_normal(size=int(bad.sum()))
    bad = np.abs(x) > 2.0
  return (x * std).astype(np.float32)


def random_init(model_variant='xception_65', num_objs=21, num_frags=64, seed=0,
                randomize_bn=False, logits_std=0.01, atrous_rates=(12, 24, 36)):
  """Random-init checkpoint with the reference's initialisers.

  randomize_bn=True draws non-trivial BatchNorm statistics (tests use it so that
  BN folding is actually exercised); False gives slim's defaults gamma=1, beta=0,
  mean=0, var=1.
  """
  rng = np.random.RandomState(seed)
  std = {'backbone': 0.09, 'head_dw': 0.33, 'head_pw': 0.06,
         'logits': logits_std}
  w = {}
  for kind, scope, shape, init in variable_specs(
      model_variant, num_objs, num_frags, atrous_rates):
    if init == 'he':      # slim variance_scaling_initializer (resnet_arg_scope)
      fan_in = shape[0] * shape[1] * shape[2]
      arr = _trunc_normal(rng, shape, np.sqrt(2.0 / fan_in) / 0.8796)
    elif init == 'xavier':
      fan_in = shape[0] * shape[1] * shape[2]
      fan_out = shape[0] * shape[1] * shape[3]
      lim = np.sqrt(6.0 / (fan_in + fan_out))
      arr = rng.uniform(-lim, lim, size=shape).astype(np.float32)
    else:
      arr = _trunc_normal(rng, shape, std[init])
    if kind == 'dw':
      w[scope + '/depthwise_weights'] = arr
    else:
      w[scope + '/weights'] = arr
    if kind == 'logits':
      w[scope + '/biases'] = (
          rng.standard_normal(shape[3]).astype(np.float32) * logits_std
          if randomize_bn else np.zeros(shape[3], np.float32))
      continue
    c = shape[2] if kind == 'dw' else shape[3]
    if randomize_bn:
      # The last BN of a ResNet bottleneck gets a small gamma so that 33 stacked
      # residual units keep activations O(1) at random init.
      g_scale = 0.25 if scope.endswith('bottleneck_v1/conv3') else 1.0
      w[scope + '/BatchNorm/gamma'] = (
          rng.uniform(0.5, 1.5, c) * g_scale).astype(np.float32)
      w[scope + '/BatchNorm/beta'] = (
          rng.standard_normal(c) * 0.1).astype(np.float32)
      w[scope + '/BatchNorm/moving_mean'] = (
          rng.standard_normal(c) * 0.1).astype(np.float32)
      w[scope + '/BatchNorm/moving_variance'] = rng.uniform(
          0.5, 1.5, c).astype(np.float32)
    else:
      w[scope + '/BatchNorm/gamma'] = np.ones(c, np.float32)
      w[scope + '/BatchNorm/beta'] = np.zeros(c, np.float32)
      w[scope + '/BatchNorm/moving_mean'] = np.zeros(c, np.float32)
      w[scope + '/BatchNorm/moving_variance'] = np.ones(c, np.float32)
  return w


def heavy_tailed(w, seed=0, tiny_frac=0.01, tiny_scale=1e-10, lognormal_every=4,
                 sigma=3.0):
  """A copy of checkpoint ``w`` whose every conv / logits matrix has the tails of a TRAINED
  network (weight decay drives many weights far below their column's maximum) that the
  reference's initialisers never draw: ``tiny_frac`` of the entries of every matrix are
  scaled by ``tiny_scale``, and every ``lognormal_every``-th output column gets log-normal
  (sigma) magnitudes, renormalised to the column's l2 norm so that activations keep their
  scale. Used by the tests and by ``bench.py --weights heavy-tailed`` to show that such a
  checkpoint stays on the fp16-pair GEMM (until round 5 one such weight moved the whole layer
  to the 20 % slower bf16 x 6 kernel). Depthwise filters and BatchNorm are left alone."""
  rng = np.random.RandomState(seed + 77)
  out = dict(w)
  for key in sorted(w):
    if not key.endswith('/weights'):
      continue
    a = np.asarray(w[key], np.float64)
    shape = a.shape
    m = a.reshape(-1, shape[-1]).copy()
    cols = np.arange(m.shape[1]) % lognormal_every == lognormal_every - 1
    if cols.any() and m.shape[0] > 1:
      norm = np.sqrt((m[:, cols] ** 2).sum(0, keepdims=True))
      h = m[:, cols] * np.exp(sigma * rng.standard_normal((m.shape[0], int(cols.sum()))))
      m[:, cols] = h * (norm / np.maximum(np.sqrt((h ** 2).sum(0, keepdims=True)), 1e-300))
    m[rng.uniform(size=m.shape) < tiny_frac] *= tiny_scale
    out[key] = m.reshape(shape).astype(np.float32)
  return out


def fold_bn(w, scope, eps, kind):
  """Folds inference-mode BatchNorm into a per-output-channel (scale, bias):
  y = scale * conv(x) + bias, scale = gamma / sqrt(var + eps),
  bias = beta - mean * scale. Computed in float64, returned as float32."""
  g = w[scope + '/BatchNorm/gamma'].astype(np.float64)
  b = w[scope + '/BatchNorm/beta'].astype(np.float64)
  m = w[scope + '/BatchNorm/moving_mean'].astype(np.float64)
  v = w[scope + '/BatchNorm/moving_variance'].astype(np.float64)
  scale = g / np.sqrt(v + eps)
  bias = b - m * scale
  return scale.astype(np.float32), bias.astype(np.float32)


def save_npz(path, w):
  np.savez(path, **{k.replace('/', '|'): v for k, v in w.items()})


def load_npz(path):
  with np.load(path) as z:
    return {k.replace('|', '/'): z[k] for k in z.files}
