"""EPOS network (DeepLabv3+ on Xception-41/65/71 or ResNet-v1-50/101[-beta]) executor
for MI355X.

Builds, once per (batch, height, width, num_objs, num_frags), a static plan of
fused HIP launches for the forward pass that the reference builds as a TF graph
in ``model.predict`` (model.py:629-687 -> multi_scale_logits :517 -> get_logits
:461 -> feature.extract_features -> net_xception.xception_65), allocates every
activation buffer in HBM up front (NHWC fp32, the reference's layout and dtype)
and replays the plan on the current HIP stream -- eagerly or as a captured
hipGraph (no tracing compiler: the plan is explicit).

Fusion groups:
  * BatchNorm is folded into the preceding conv at weight-load time;
  * depthwise 3x3 (+BN, ReLU before/after) is one launch;
  * pointwise 1x1 (+BN, +residual add, +ReLU) is one GEMM launch -- the fp16-pair kernel
    where the fp32 A operand has an absmax bound, else the split-operand bf16 x 6 kernel --
    that can read/write channel slices of the ASPP / decoder concat buffers, so no concat
    copy exists;
  * dense 3x3 stem convs: stride 1 with Cin % 32 == 0 (conv1_2) is an implicit GEMM
    inside the LDS-DMA kernel; the 3-channel stride-2 conv1_1 is im2col + the same GEMM.
torch is used for device memory and streams only.

precision='bf16' (opt-in; the default 'fp32' plan is unchanged): the same graph with bf16
activation buffers and bf16 weights (BN folded in fp32, then rounded to nearest even), bf16 x
bf16 products with fp32 accumulation and fp32 epilogues (csrc/bf16.hip), one rounding per
stored activation. The image and its preprocessing, the image-pooling 1x1 and the three
logits / prediction tensors stay fp32; decoder_out is a bf16 tensor. DESIGN.md, "bf16 mode".

The graph walk below is written once for both precisions; every launch decision that
depends on the precision is made by the plan's numeric mode (epos_amd/net_modes.py).
"""
import ctypes
import os

import numpy as np
import torch

from epos_amd import _call as C
from epos_amd import _lib
from epos_amd import weights as W
from epos_amd._call import ptr as _ptr
from epos_amd.net_modes import Bf16Mode, Fp32Mode

XCEPTION_BN_EPS = 1e-3   # feature.py:300-307
HEAD_BN_EPS = 1e-5       # model.py:194-199, 307-312
RESNET_BN_EPS = 1e-5     # feature.py:282-287
MODES = {'fp32': Fp32Mode, 'bf16': Bf16Mode}
PRECISIONS = tuple(MODES)
PREPROCESS = {None: _lib.PREPROCESS_NONE, 'unit_range': _lib.PREPROCESS_UNIT_RANGE,
              'sub_mean': _lib.PREPROCESS_SUB_MEAN}
PREPROCESS_EXPR = {'unit_range': 'preprocess(input)', 'sub_mean': 'submean(input)'}


def scale_dimension(dim, scale):
  """model.py:100-114."""
  return int((float(dim) - 1.0) * scale + 1.0)


_CAPTURE_STREAMS = {}


def _capture_stream(dev):
  """The stream a graph of the plan is captured on: the caller's when it is not the default
  one (the pipeline's own stream) -- every extra HIP stream shifts the stream -> hardware-queue
  mapping (4 queues), and two pipelines sharing a queue serialise against each other --
  else one shared side stream per device."""
  side = torch.cuda.current_stream(dev)
  if side != torch.cuda.default_stream(dev):
    return side
  key = str(dev)
  if key not in _CAPTURE_STREAMS:
    _CAPTURE_STREAMS[key] = torch.cuda.Stream(dev)
  return _CAPTURE_STREAMS[key]


class EposNet(object):
  """Static-shape forward plan. ``forward(images)`` returns the logits buffers;
  ``predict(images)`` the reference's prediction dict (model.py:629-687)."""

  def __init__(self, checkpoint, batch, height, width, num_objs, num_frags=64,
               model_variant='xception_65', encoder_output_stride=8,
               decoder_output_stride=4, atrous_rates=(12, 24, 36),
               multi_grid=None, device='cuda:0', dry_run=False, precision='fp32',
               decoder_hw=None):
    if precision not in PRECISIONS:
      raise ValueError('precision must be one of %s (got %r).' % (PRECISIONS, precision))
    self.precision = precision
    self.variant = W.variant(model_variant)     # ValueError for the variants this build lacks
    self.model_variant = model_variant
    if encoder_output_stride != 8 or decoder_output_stride != 4:
      raise ValueError('Only encoder OS 8 / decoder OS 4 (common.py:127-135).')
    if not 1 <= num_frags <= 256:        # the fragment softmax / correspondence kernels
      raise ValueError('num_frags must be in [1, 256] (got %d).' % num_frags)
    # dry_run: build the plan's STRUCTURE only (tests/test_graph_trace.py) -- buffers are
    # shape-only 'meta' tensors, no weight is packed, nothing can be launched.
    self.dry_run = bool(dry_run)
    if not self.dry_run and not torch.cuda.is_available():
      raise _lib.EposError('EposNet needs a HIP device (no CPU fallback).')
    self.lib = None if self.dry_run else _lib.load()
    self.dev = torch.device('meta' if self.dry_run else device)
    self.B, self.H, self.W = batch, height, width
    self.num_objs, self.num_frags = num_objs, num_frags
    self.atrous_rates = tuple(atrous_rates)
    self.multi_grid = list(multi_grid) if multi_grid else [1, 1, 1]
    # decoder_hw: the size the decoder resizes its two inputs to, (scale_dimension(w, 1/4),
    # scale_dimension(h, 1/4)) of crop_size (model.py:355-356). None: the stride-4 map of the
    # input. Multi-scale inference passes the size the reference's multi_scale_logits gives
    # a scale != 1 (epos_amd/multiscale.py); the low-level features are then resized too.
    self.decoder_hw = tuple(decoder_hw) if decoder_hw is not None else None
    self.ckpt = checkpoint
    self._keep = []          # device tensors owned by the plan
    self.ops = []            # (name, callable(stream))
    self.post_ops = []       # softmax / argmax, in place on the heads
    self.flops = 0           # multiply-add * 2 of the whole plan
    self.op_flops = {}
    self.op_kind = {}        # 'gemm' | 'dw' | 'im2col' | 'other'
    self.op_bytes = {}       # GEMM launches: algorithmic bytes (A + W + out + residual)
    # fusion-group byte model (algorithmic_bytes): per GEMM (A bytes, the rest, id of the A
    # buffer); per depthwise output buffer the bytes its launch READS (input + weights); the
    # stand-alone glue ops' bytes
    self.op_io = {}
    self._dw_reads = {}
    self._glue_bytes = 0
    self._graph = None
    self._graph_sparse = None
    self._graph_logits = None                     # forward_logits(use_graph=True)
    self._graph_alt, self.alt_skip = None, None   # measurement aid: see capture_alt()
    # Structure trace: one record per parametrised layer and a canonical expression per
    # buffer (channel slices of concat buffers separately), in the grammar of
    # tests/golden/tf_recorder.py -- what each launch computes, written down from the very
    # arguments the launch is built from. tests/test_graph_trace.py holds it against the
    # graph the reference's own code builds (tests/golden/graph_*.json).
    self.trace_layers, self.trace_outputs = [], {}
    self._exprs = {}
    self.pad_rows = os.environ.get('EPOS_PAD_ROWS', '1') != '0'
    self._lds = {}
    self._col_ids = set()        # the im2col matrices
    self._images_u8 = None       # device staging for uint8 frames (set_images)
    self.pool_folded = False
    self._n_trunk_ops = 0        # the ops in front of the logits (sparse-head mode)
    self._obj_head_op, self._obj_head_flops = None, 0
    self._sparse_packs = None
    self._layer_consts = {}      # trainable layer -> (moving_mean, moving_variance) on the device
    self._decoder_x = None
    self._dw_operands = {}       # layer of weights.DEPTHWISE_BACKWARD_LAYERS or
    #                              DEPTHWISE_CHAIN_LAYERS -> depthwise_operand
    self._dw_consts = {}         # ... -> its variables and statistics on the device
    self._pw_consts = {}         # layer of weights.POINTWISE_CHAIN_LAYERS -> pointwise_constants
    self._chain = {}             # the buffers trainer.decoder_grads needs: chain_operands
    # ASPP's layers for these rates, whose operands the plan records (aspp_operands): records
    # only, no launch, buffer or argument depends on them
    self._aspp_pw, self._aspp_dw = W.aspp_layers(self.atrous_rates)
    self._aspp = {}
    self.mode = MODES[precision](self)
    self.act_dtype = self.mode.dtype
    self._build_plan()

  # the fp16-pair bookkeeping of the fp32 plan (empty in bf16 mode)
  use_h2 = property(lambda self: self.mode.use_h2)
  h2_layers = property(lambda self: self.mode.h2_layers)
  h2_refused = property(lambda self: self.mode.h2_refused)
  presplit_layers = property(lambda self: self.mode.presplit_layers)
  # the absmax slot table of the fp32 plan (bf16 mode: no slots and no table)
  _n_slots = property(lambda self: self.mode._n_slots)
  _amax_table = property(lambda self: self.mode._amax_table)

  # ------------------------------------------------------------ buffers ---
  def _empty(self, *shape, dtype=torch.float32):
    t = torch.empty(*shape, dtype=dtype, device=self.dev)
    self._keep.append(t)
    return t

  def _act(self, b, h, w, c):
    """Activation buffer [b, h, w, ld] for c channels: rows padded to a multiple of one
    128-byte line (the mode's `line` elements) where c is not one already -- Xception's
    728-channel tensors become 736 floats wide (+1.1 %) -- so that every pixel's channel
    vector starts on a line: the depthwise kernel's per-XCD channel slices then share no
    line (csrc/layers.hip; a dense 728-float row has 7 slice boundaries inside lines and
    ~30 % of the input is fetched by two XCDs), and the GEMMs' A rows and C rows are
    line-aligned. The padding columns are never read or written. EPOS_PAD_ROWS=0: dense
    rows (the A/B switch)."""
    line = self.mode.line
    ld = (c + line - 1) // line * line if (self.pad_rows and c >= 256) else c
    t = self._empty(b, h, w, ld, dtype=self.act_dtype)
    self._lds[id(t)] = ld
    return t

  def _abuf(self, *shape):
    """Dense activation buffer in the plan's activation dtype."""
    return self._empty(*shape, dtype=self.act_dtype)

  def _ld(self, buf):
    """Row pitch (elements) of an activation buffer."""
    return self._lds.get(id(buf), buf.shape[-1])

  def _dev(self, arr):
    t = torch.from_numpy(np.ascontiguousarray(arr)).to(self.dev)
    self._keep.append(t)
    return t

  # ---------------------------------------------------- structure trace ---
  def _set_expr(self, buf, expr, off=0, width=None):
    width = buf.shape[-1] if width is None else width
    ent = [e for e in self._exprs.get(id(buf), []) if e[0] != off]
    ent.append((off, width, expr))
    self._exprs[id(buf)] = sorted(ent)

  def _expr_of(self, buf, off=0, width=None):
    width = buf.shape[-1] if width is None else width
    ent = self._exprs[id(buf)]
    for o, w, e in ent:
      if o == off and w == width:
        return e
    parts, at = [], off
    for o, w, e in ent:                   # a read across the slices of a concat buffer
      if o == at and at < off + width:
        parts.append(e)
        at += w
    assert at == off + width and parts, ('no expression for the slice', off, width, ent)
    return 'concat(%s)' % ','.join(parts)

  @staticmethod
  def _relu_expr(e):
    return e if e.startswith('relu(') else 'relu(%s)' % e

  def _trace_layer(self, scope, op, kernel, stride, rate, padding, cin, cout, bn_eps,
                   bias, expr_in, out_hw):
    self.trace_layers.append({
        'scope': scope, 'op': op, 'kernel': [kernel, kernel], 'stride': stride,
        'rate': rate, 'padding': padding, 'cin': cin, 'cout': cout, 'bn_eps': bn_eps,
        'bias': bias, 'input': expr_in, 'out_hw': [int(out_hw[0]), int(out_hw[1])]})

  # ------------------------------------------------------------ weights ---
  def _conv_params(self, scope, eps):
    """1x1 / dense conv -> (w [K, N], scale, bias): followed by BN (folded with `eps`), or
    eps=None: a conv with biases of its own (the logits)."""
    w = self.ckpt[scope + '/weights']
    w = w.reshape(-1, w.shape[3])
    if eps is None:
      return w, np.ones(w.shape[1], np.float32), self.ckpt[scope + '/biases']
    scale, bias = W.fold_bn(self.ckpt, scope, eps, 'conv')
    return w, scale, bias

  def _dw_params(self, scope, eps):
    """Depthwise 3x3 + BN -> (w9c, bias) on the device and (gain, bias0):
    |depthwise output| <= gain * max|input| + bias0 (the consumer GEMM's A bound)."""
    w = self.ckpt[scope + '/depthwise_weights']          # [3,3,C,1]
    scale, bias = W.fold_bn(self.ckpt, scope, eps, 'dw')
    w9c = (w[:, :, :, 0].reshape(9, -1) * scale[None, :]).astype(np.float32)
    gain = float(np.abs(w9c.astype(np.float64)).sum(0).max())
    bias0 = float(np.abs(np.asarray(bias, np.float64)).max())
    return self._dev(w9c), self._dev(bias), gain, bias0

  # --------------------------------------------------------------- ops ---
  def _fn(self, name):
    """Entry point `name` of the library (None in a dry run, which launches nothing)."""
    return None if self.lib is None else getattr(self.lib, name)

  @staticmethod
  def _call(name, fn, args):
    """callable(stream) running fn(*args, stream). A ctypes struct in `args` is passed by
    reference: fields set after this call still reach the launch."""
    args = tuple(ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in args)

    def run(stream):
      _lib.check(fn(*args, stream), name)
    return run

  def _launch(self, name, fn, args, kind='other', flops=0, nbytes=0):
    """Appends the op `name` = fn(*args, stream) to the plan (see _call)."""
    self.ops.append((name, self._call(name, fn, args)))
    self.op_bytes[name] = nbytes
    self.flops += flops
    self.op_flops[name] = flops
    self.op_kind[name] = kind

  def _conv1x1(self, name, eps, a, a_off, lda, m, k, c, c_off, ldc, relu, res=None,
               res_off=0, ldr=0, sub=1, ho=0, wo=0, hi=0, wi=0, group=None, track_out=True):
    """One 1x1 conv (+BN with `eps`, +residual, +ReLU). With ``group`` (a list) the problem
    is only appended to it; mode.flush later launches the whole list as ONE grouped GEMM."""
    conv = self._conv_params(name, eps)
    n = conv[0].shape[1]
    hw = (ho, wo) if sub > 1 else (c.shape[1:3] if c.dim() == 4 else (1, 1))
    self._trace_layer(name, 'conv2d', 1, sub, 1, 'SAME', k, n, eps, eps is None,
                      self._expr_of(a, a_off, k), hw)
    eout = 'L:' + name
    if res is not None:
      eout = 'add(%s)' % ','.join(sorted([eout, self._expr_of(res, res_off, n)]))
    self._set_expr(c, self._relu_expr(eout) if relu else eout, c_off, n)
    self.mode.pointwise(name, a, a_off, lda, m, k, conv, c, c_off, ldc, relu, res, res_off,
                        ldr, sub, ho, wo, hi, wi, group, track_out)

  def _depthwise(self, name, x, ldx, hi, wi, c, stride, rate, eps, relu_in, relu_out):
    """One depthwise 3x3 launch."""
    B = self.B
    ho, wo = (hi - 1) // stride + 1, (wi - 1) // stride + 1
    w9c, bias, gain, bias0 = self._dw_params(name, eps)
    y = self._act(B, ho, wo, c)
    if name in W.DEPTHWISE_BACKWARD_LAYERS or name in W.DEPTHWISE_CHAIN_LAYERS or \
        name in self._aspp_dw:
      assert stride == 1 and not relu_in and relu_out, name
      self._dw_operands[name] = {'x': x, 'ldx': ldx, 'b': B, 'h': hi, 'w': wi, 'c': c,
                                 'rate': rate, 'w9c': w9c, 'bias': bias, 'eps': eps}
    ein = self._expr_of(x, 0, c)
    if relu_in:
      ein = self._relu_expr(ein)
    if stride > 1:                # fixed_padding (net_xception.py:74-93) + VALID
      ein = 'pad(%s,%d,%d)' % (ein, rate, rate)
    self._trace_layer(name, 'depthwise_conv2d', 3, stride, rate,
                      'SAME' if stride == 1 else 'VALID', c, c, eps, False, ein, (ho, wo))
    self._set_expr(y, self._relu_expr('L:' + name) if relu_out else 'L:' + name, 0, c)
    # algorithmic bytes: the input read once + the output written once, fp32 weights
    e = y.element_size()
    self._dw_reads[id(y)] = e * B * hi * wi * c + 40 * c
    self.mode.depthwise(name, x, y, gain, bias0, 2 * 9 * B * ho * wo * c,
                        e * (B * hi * wi * c + B * ho * wo * c) + 40 * c,
                        X=_ptr(x), ldx=ldx, w9c=_ptr(w9c), bias=_ptr(bias), Y=_ptr(y),
                        ldy=self._ld(y), B=B, Hi=hi, Wi=wi, Ho=ho, Wo=wo, C=c, stride=stride,
                        rate=rate, relu_in=int(relu_in), relu_out=int(relu_out))
    return y, ho, wo

  def _dense_conv(self, name, x, hi, wi, cin, stride, eps, rate=1, preprocess=None):
    """resnet_utils.conv2d_same k x k (+BN+ReLU) (net_xception.py:460-463;
    net_resnet_v1_beta.py:82-83,108-110,168-173). stride 1 -> 'SAME'; stride > 1 ->
    fixed_padding + VALID, rate * (k - 1) // 2 in front and the rest behind. `preprocess`
    ('unit_range' | 'sub_mean'): x is the network input, preprocessed first and padded with
    zeros after (feature.py:157-185 ahead of the network function)."""
    conv = self._conv_params(name, eps)
    kk = self.ckpt[name + '/weights'].shape[0]
    cout = conv[0].shape[1]
    ho, wo = (hi - 1) // stride + 1, (wi - 1) // stride + 1
    pad = rate * (kk - 1) // 2
    ein = self._expr_of(x, 0, cin)
    if preprocess:                # fused into the im2col (feature.py:171-185)
      assert ein == 'input'
      ein = PREPROCESS_EXPR[preprocess]
    if stride > 1:                # conv2d_same: explicit padding + VALID
      ein = 'pad(%s,%d,%d)' % (ein, pad, rate * (kk - 1) - pad)
    self._trace_layer(name, 'conv2d', kk, stride, rate, 'SAME' if stride == 1 else 'VALID',
                      cin, cout, eps, False, ein, (ho, wo))
    y = self._abuf(self.B, ho, wo, cout)
    self.mode.dense_conv(name, x, y, hi, wi, cin, ho, wo, kk, stride, rate, pad,
                         PREPROCESS[preprocess], conv)
    self._set_expr(y, 'relu(L:%s)' % name)
    return y, ho, wo, cout

  # ------------------------------------------------ ResNet-v1-101-beta (C5) ---
  def _bottleneck(self, scope, x, hi, wi, cin, depth, db, stride, rate,
                  keep_conv3=False):
    """net_resnet_v1_beta.py:38-93: 1x1 -> 3x3 (conv2d_same, rate) -> 1x1, plus
    shortcut, ReLU after the add. The add + ReLU is the epilogue of the conv3 GEMM
    unless conv3 itself is an end point (decoder tap, feature.py:50-54)."""
    eps = RESNET_BN_EPS
    B = self.B
    ho = hi if stride == 1 else (hi - 1) // 2 + 1
    wo = wi if stride == 1 else (wi - 1) // 2 + 1
    m_in, m_out = B * hi * wi, B * ho * wo
    if depth == cin:
      if stride == 1:
        shortcut = x
      else:                                    # resnet_utils.subsample (:71-72)
        shortcut = self._abuf(B, ho, wo, depth)
        self._launch(scope + '/shortcut_subsample', self.mode.subsample,
                     (_ptr(x), cin, _ptr(shortcut), depth, B, hi, wi, cin, stride))
        self._glue_bytes += 2 * shortcut.element_size() * B * ho * wo * depth
        self._set_expr(shortcut, 'subsample(%s,%d)' % (self._expr_of(x, 0, cin), stride))
        self.mode.same_bound(shortcut, x)
    else:
      shortcut = self._abuf(B, ho, wo, depth)
      self._conv1x1(scope + '/shortcut', eps, x, 0, cin, m_out, cin, shortcut, 0, depth,
                    relu=False, sub=stride, ho=ho, wo=wo, hi=hi, wi=wi)
    r1 = self._abuf(B, hi, wi, db)
    self._conv1x1(scope + '/conv1', eps, x, 0, cin, m_in, cin, r1, 0, db, relu=True)
    r2, _, _, _ = self._dense_conv(scope + '/conv2', r1, hi, wi, db, stride, eps, rate)
    out = self._abuf(B, ho, wo, depth)
    conv3 = None
    if keep_conv3:
      conv3 = self._abuf(B, ho, wo, depth)
      self._conv1x1(scope + '/conv3', eps, r2, 0, db, m_out, db, conv3, 0, depth, relu=False)
      self._launch(scope + '/add_relu', self.mode.add_relu,
                   (_ptr(conv3), _ptr(shortcut), _ptr(out), m_out * depth))
      self._glue_bytes += 3 * out.element_size() * m_out * depth
      self._set_expr(out, 'relu(add(%s))' % ','.join(sorted(
          [self._expr_of(conv3), self._expr_of(shortcut)])))
      self.mode.track_absmax(scope + '/add_relu/absmax', out, depth, m_out, depth)
    else:
      self._conv1x1(scope + '/conv3', eps, r2, 0, db, m_out, db, out, 0, depth, relu=True,
                    res=shortcut, ldr=depth)
    return out, ho, wo, depth, conv3

  def _backbone_resnet(self):
    """resnet_v1_{50,101}[_beta] (net_resnet_v1_beta.py:233-516) at output_stride 8."""
    B, H, Wd = self.B, self.H, self.W
    net = self.variant['scope']
    x, h, w, c = self.images, H, Wd, 3
    if self.variant['root'] == 'beta':
      for i, stride in enumerate([2, 1, 1], 1):              # :108-110
        x, h, w, c = self._dense_conv('%s/conv1_%d' % (net, i), x, h, w, c, stride,
                                      RESNET_BN_EPS,
                                      preprocess=self.variant['preprocess'] if i == 1 else None)
    else:                                                    # :168-173
      x, h, w, c = self._dense_conv(net + '/conv1', x, h, w, c, 2, RESNET_BN_EPS,
                                    preprocess=self.variant['preprocess'])
    ph, pw = (h + 1) // 2, (w + 1) // 2
    pooled = self._abuf(B, ph, pw, c)
    self._launch(net + '/pool1', self.mode.maxpool,                  # :190
                 (_ptr(x), c, _ptr(pooled), c, B, h, w, c))
    self._glue_bytes += pooled.element_size() * B * (h * w + ph * pw) * c
    self._set_expr(pooled, 'maxpool(%s,3,2,SAME)' % self._expr_of(x, 0, c))
    self.mode.same_bound(pooled, x)           # a max-pool output is bounded by its input
    x, h, w = pooled, ph, pw
    target, current_stride, rate = 2, 1, 1                   # 8 / 4 (:185-188)
    low_level = None
    mg = self.multi_grid
    for bscope, base, units in self.variant['blocks']:
      for u in range(units):
        scope = '%s/%s/unit_%d/bottleneck_v1' % (net, bscope, u + 1)
        stride = 2 if (u == units - 1 and bscope != 'block4') else 1
        unit_rate = mg[u] if bscope == 'block4' else 1
        keep = bscope == self.variant['tap'] and u == 1
        if current_stride == target:
          x, h, w, c, conv3 = self._bottleneck(scope, x, h, w, c, base * 4, base,
                                               1, rate * unit_rate, keep)
          rate *= stride
        else:
          x, h, w, c, conv3 = self._bottleneck(scope, x, h, w, c, base * 4, base,
                                               stride, unit_rate, keep)
          current_stride *= stride
        if keep:
          low_level = (conv3, h, w, base * 4)
    return x, h, w, c, low_level

  def _backbone_xception(self):
    """xception_{41,65,71} (net_xception.py:396-483, block tables in weights.XCEPTION_TABLES)."""
    net = self.variant['scope']
    tap = self.variant['tap']
    x, h, w, c = self._dense_conv(net + '/entry_flow/conv1_1', self.images, self.H, self.W,
                                  3, 2, XCEPTION_BN_EPS, preprocess=self.variant['preprocess'])
    x, h, w, c = self._dense_conv(net + '/entry_flow/conv1_2', x, h, w, c, 1, XCEPTION_BN_EPS)
    # stack_blocks_dense (net_xception.py:326-393) with output_stride 8/2 = 4.
    target, current_stride, rate = 4, 1, 1
    low_level = None
    blocks = [b + ((self.multi_grid if b[0] == 'exit_flow/block2' else [1, 1, 1]),)
              for b in self.variant['blocks']]
    for bscope, depths, skip, act, units, stride, url in blocks:
      for u in range(units):
        scope = '%s/%s/unit_%d/xception_module' % (net, bscope, u + 1)
        # the decoder taps sep-conv 2 of the tap block (entry_flow/block2; xception_71:
        # block3) BEFORE any activation
        linear = (1,) if bscope == tap else ()
        if current_stride == target:
          x, h, w, c, taps = self._xception_module(
              scope, x, h, w, c, depths, skip, act, 1, rate, url, linear)
          rate *= stride
        else:
          x, h, w, c, taps = self._xception_module(
              scope, x, h, w, c, depths, skip, act, stride, 1, url, linear)
          current_stride *= stride
        if bscope == tap:
          low_level = (taps[1], taps[1].shape[1], taps[1].shape[2], depths[1])
    return x, h, w, c, low_level

  def _xception_module(self, scope, x, hi, wi, cin, depths, skip, act_in_sep,
                       stride, rate, unit_rates, linear_taps=()):
    """net_xception.py:197-323 as 3 x (depthwise launch + GEMM launch); the skip
    connection is the residual input of the third GEMM's epilogue.

    In the pre-activation form (ReLU -> depthwise -> pointwise, :272-276) the outputs
    of sep-convs 1 and 2 are read by the next ReLU only, so that ReLU is applied by
    the producing GEMM's epilogue (same values, bit for bit) instead of on every
    tap the depthwise kernel loads -- except for `linear_taps`, which the decoder
    reads before the activation (feature.py:29-73 'entry_flow/block2/unit_1/
    xception_module/separable_conv2_pointwise')."""
    eps = XCEPTION_BN_EPS
    ho = hi if stride == 1 else (hi - 1) // 2 + 1
    wo = wi if stride == 1 else (wi - 1) // 2 + 1
    shortcut = None
    grp = []
    if skip == 'conv':
      # The shortcut GEMM shares a launch with the first pointwise conv.
      shortcut = self._act(self.B, ho, wo, depths[2])
      self._conv1x1(scope + '/shortcut', eps, x, 0, self._ld(x), self.B * ho * wo, cin,
                    shortcut, 0, self._ld(shortcut), relu=False, sub=stride, ho=ho, wo=wo,
                    hi=hi, wi=wi, group=grp)
    r, rh, rw, rc = x, hi, wi, cin
    taps = {}
    r_is_relu = False           # r already holds ReLU(previous sep-conv output)
    for i in range(3):
      sc = '%s/separable_conv%d' % (scope, i + 1)
      s_i = stride if i == 2 else 1
      d, dh, dw_ = self._depthwise(
          sc + '_depthwise', r, self._ld(r), rh, rw, rc, s_i, rate * unit_rates[i], eps,
          relu_in=(not act_in_sep) and not r_is_relu, relu_out=act_in_sep)
      y = self._act(self.B, dh, dw_, depths[i])
      res, ldr = None, 0
      if i == 2 and skip == 'conv':
        res, ldr = shortcut, self._ld(shortcut)
      elif i == 2 and skip == 'sum':
        res, ldr = x, self._ld(x)
      fold_next_relu = (not act_in_sep) and i < 2 and i not in linear_taps
      self._conv1x1(sc + '_pointwise', eps, d, 0, self._ld(d), self.B * dh * dw_, rc, y, 0,
                    self._ld(y), relu=act_in_sep or fold_next_relu, res=res, ldr=ldr,
                    group=grp if i == 0 else None)
      r_is_relu = fold_next_relu
      if i == 0:
        self.mode.flush(grp)
      taps[i] = y
      r, rh, rw, rc = y, dh, dw_, depths[i]
    return r, rh, rw, rc, taps

  # -------------------------------------------------------------- plan ---
  def _build_plan(self):
    B, H, Wd = self.B, self.H, self.W
    mode = self.mode
    self.images = self._empty(B, H, Wd, 3)
    self._set_expr(self.images, 'input')
    mode.begin()
    if self.variant['family'] == 'xception':
      x, h, w, c, low_level = self._backbone_xception()
    else:
      x, h, w, c, low_level = self._backbone_resnet()
    self.encoder = x
    eh, ew, ec = h, w, c

    # ---- ASPP (model.py:213-265): branches write slices of one 1280-wide buffer.
    nb = 2 + len(self.atrous_rates)
    cat = self._abuf(B, eh, ew, 256 * nb)
    ldcat = 256 * nb
    m_enc = B * eh * ew
    # image pooling (model.py:220)
    pooled = self._empty(B, ec)
    self.pool_folded = mode.mean('image_pooling/mean', x, pooled, eh * ew, ec)
    self._set_expr(pooled, 'mean(%s)' % self._expr_of(x, 0, ec))
    pool_feat = self._empty(B, 256)
    self._conv1x1('image_pooling', HEAD_BN_EPS, pooled, 0, ec, B, ec, pool_feat, 0, 256,
                  relu=True)
    mode.resize('image_pooling/resize', pool_feat, 256, cat, ldcat, 1, 1, eh, ew, 256)
    self._set_expr(cat, 'resize(%s,%dx%d)' % (self._expr_of(pool_feat), eh, ew), 0, 256)
    # The four spatial ASPP branches (N = 256 each) share ONE grouped GEMM launch.
    grp = []
    self._conv1x1('aspp0', HEAD_BN_EPS, x, 0, ec, m_enc, ec, cat, 256, ldcat, relu=True,
                  group=grp)
    for i, r in enumerate(self.atrous_rates, 1):
      d, _, _ = self._depthwise('aspp%d_depthwise' % i, x, ec, eh, ew, ec, 1, r,
                                HEAD_BN_EPS, False, True)
      self._conv1x1('aspp%d_pointwise' % i, HEAD_BN_EPS, d, 0, self._ld(d), m_enc, ec, cat,
                    256 * (i + 1), ldcat, relu=True, group=grp)
    mode.flush(grp)
    # the broadcast image-pooling branch is part of `cat` too: its absmax joins the slot
    # the four GEMM problems publish into
    mode.join_absmax('image_pooling/absmax', pool_feat, 256, B, 256, cat)
    proj = self._abuf(B, eh, ew, 256)
    self._conv1x1('concat_projection', HEAD_BN_EPS, cat, 0, ldcat, m_enc, ldcat, proj, 0,
                  256, relu=True)
    self.aspp_concat, self.concat_projection = cat, proj
    # what the backward pass through ASPP reads (aspp_operands): records only
    self._aspp = {'encoder': x, 'eh': eh, 'ew': ew, 'ec': ec, 'pooled': pooled,
                  'pool_feat': pool_feat, 'aspp_concat': cat,
                  'encoder_relu': self._expr_of(x, 0, ec).startswith('relu(')}

    # ---- decoder (model.py:268-393).
    ll, lh, lw, lc = low_level
    dh = scale_dimension(H, 1.0 / 4)
    dw_ = scale_dimension(Wd, 1.0 / 4)
    assert (lh, lw) == (dh, dw_), ((lh, lw), (dh, dw_))
    if self.decoder_hw is not None:
      dh, dw_ = self.decoder_hw
    # (padding the concat's rows 304 -> 320 and the stem's im2col rows 28 -> 32 as well:
    # measured neutral, profiles/r06/ab_pad_level.txt -- left dense)
    dcat = self._abuf(B, dh, dw_, 304)
    ldd = self._ld(dcat)
    mode.resize('decoder/resize', proj, 256, dcat, ldd, eh, ew, dh, dw_, 256)
    self._set_expr(dcat, self._expr_of(proj) if (eh, ew) == (dh, dw_) else
                   'resize(%s,%dx%d)' % (self._expr_of(proj), dh, dw_), 0, 256)
    m_dec = B * dh * dw_
    if (lh, lw) == (dh, dw_):
      self._conv1x1('decoder/feature_projection0', HEAD_BN_EPS, ll, 0, lc, m_dec, lc, dcat,
                    256, ldd, relu=True)
    else:
      # (decoder_hw) the projected low-level features at their own size, resized into the
      # concat's slice (model.py:358-361 resizes both decoder inputs)
      low = self._abuf(B, lh, lw, 48)
      self._conv1x1('decoder/feature_projection0', HEAD_BN_EPS, ll, 0, lc, B * lh * lw, lc,
                    low, 0, 48, relu=True)
      mode.resize('decoder/resize_low_level', low, 48, dcat[..., 256:], ldd, lh, lw, dh, dw_,
                  48)
      self._set_expr(dcat, 'resize(%s,%dx%d)' % (self._expr_of(low), dh, dw_), 256, 48)
      mode.same_bound(dcat, low)
    mode.concat_bound(dcat, proj)
    self.decoder_concat = dcat[..., :304]
    # what the backward pass through the decoder reads (chain_operands): records only
    self._chain = {'decoder_concat': dcat, 'ld_concat': ldd, 'concat_projection': proj,
                   'aspp_concat': cat, 'ld_aspp': ldcat, 'low_level': ll, 'low_level_c': lc,
                   'low_level_hw': (lh, lw), 'encoder_hw': (eh, ew), 'decoder_hw': (dh, dw_)}
    x, c = dcat, 304
    for j in range(2):
      scope = 'decoder/decoder_conv%d' % j
      d, _, _ = self._depthwise(scope + '_depthwise', x, self._ld(x), dh, dw_, c, 1, 1,
                                HEAD_BN_EPS, False, True)
      y = self._abuf(B, dh, dw_, 256)
      self._conv1x1(scope + '_pointwise', HEAD_BN_EPS, d, 0, self._ld(d), m_dec, c, y, 0,
                    256, relu=True)
      x, c = y, 256
    self.decoder_out = x
    self.out_h, self.out_w = dh, dw_

    # ---- logits (model.py:396-458), sorted(name) order (model.py:503).
    self.logits = {}
    grp = []
    self._n_trunk_ops = len(self.ops)      # everything before the logits layers
    for name, ch in sorted(W.outputs_to_num_channels(
        self.num_objs, self.num_frags).items()):
      buf = self._empty(B, dh, dw_, ch)
      self._conv1x1('logits/' + name, None, x, 0, 256, m_dec, 256, buf, 0, ch, relu=False,
                    group=grp, track_out=False)
      self.logits[name] = buf
    # the dense heads (413 MB at C2) are written with streaming stores: nobody re-reads them
    # soon, and as ordinary stores they sweep the 256 MB Infinity Cache clean of the other
    # images' working sets (same box: 424.6 / 422.4 vs 422.0 / 420.4 images/s, prediction of a
    # serial step 3.31 vs 3.35 ms; EPOS_HEAD_NT_STORES=0 turns it off)
    if os.environ.get('EPOS_HEAD_NT_STORES', '1') == '1':
      for g in grp:
        g[1].c_stream = 1
    oname, oargs, oflops = [g for g in grp if g[0].endswith(W.PRED_OBJ_CONF)][0][:3]
    # (Round 4 built the fragment softmax of model.py:678 into this launch's epilogue --
    # identical bits -- and measured it slower than the softmax's own memory-bound launch:
    # 410.6 / 415.6 vs 419.2 / 421.3 images/s, profiles/r04/ab_head_softmax.txt; removed in
    # round 5.)
    # the three heads: one grouped launch; in fp32 mode on the A-stationary heads kernel
    # (csrc/heads_gemm_h2.hip, same bits; EPOS_HEADS_KERNEL=0 keeps the generic grouped GEMM)
    self.heads_group = None      # (argument array, count) of a launch through the heads entry
    mode.flush(grp, heads=os.environ.get('EPOS_HEADS_KERNEL', '1') == '1')
    # Sparse-head mode (pipeline option): only the object head runs densely; the
    # fragment heads are evaluated per (image, target object) -- see
    # run_sparse_heads().
    self._obj_head_op = (oname, mode.obj_head(oname, oargs))
    self._obj_head_flops = oflops
    self._decoder_x = x

    # ---- predict post-ops (model.py:677-683): softmax in place, argmax.
    obj = self.logits[W.PRED_OBJ_CONF]
    frag = self.logits[W.PRED_FRAG_CONF]
    self.obj_label = self._empty(B, dh, dw_, dtype=torch.int64)
    O, F = self.num_objs, self.num_frags
    softmax = self._fn('epos_softmax_groups_f32')
    self.post_ops = [
        ('softmax_obj', self._call('softmax_obj', softmax, (_ptr(obj), m_dec, O + 1))),
        ('softmax_frag', self._call('softmax_frag', softmax, (_ptr(frag), m_dec * O, F))),
        ('argmax', self._call('argmax', self._fn('epos_argmax_i64'),
                              (_ptr(obj), O + 1, _ptr(self.obj_label), m_dec, O + 1)))]
    # model.py:117-147 (reshape), :677-683 (softmax over the last axis, argmax)
    eo = self._expr_of(self.logits[W.PRED_OBJ_CONF])
    ef = self._expr_of(self.logits[W.PRED_FRAG_CONF])
    el = self._expr_of(self.logits[W.PRED_FRAG_LOC])
    self.trace_outputs = {
        W.PRED_OBJ_CONF: {'expr': 'softmax(%s)' % eo, 'shape': [B, dh, dw_, O + 1]},
        W.PRED_OBJ_LABEL: {'expr': 'argmax(softmax(%s))' % eo, 'shape': [B, dh, dw_]},
        W.PRED_FRAG_CONF: {'expr': 'softmax(reshape(%s,%s))' % (ef, [O, F]),
                           'shape': [B, dh, dw_, O, F]},
        W.PRED_FRAG_LOC: {'expr': 'reshape(%s,%s)' % (el, [O, F, 3]),
                          'shape': [B, dh, dw_, O, F, 3]}}
    mode.finish()

  def algorithmic_bytes(self, dense_heads=True):
    """HBM bytes of ONE pass of the plan under the fusion-group rule of SURVEY.md App. A
    (fp32): every separable conv is one group -- the depthwise INPUT is read once, the
    pointwise output written once, weights once, the intermediate never leaves the chip --
    a GEMM reads A and its residual once and writes its output once, the stem's im2col
    matrix does not exist (the input image is read once), and the element-wise ops that
    belong in a producer's epilogue (global mean, decoder resize, softmax, argmax) move
    nothing of their own: the heads are written once. ResNet's max-pool / subsample /
    stand-alone add read and write their tensors once. Reproduces the survey's figures
    (C2: 3.32 vs 3.30 GB, batch 8: 3.17 vs 3.15, C4: 4.40 vs 4.38; C5: 3.64 GB per image at batch 8). What the launches of
    this build actually move is roofline.traffic in bench.py."""
    total = self._glue_bytes
    for a_bytes, rest, a_id in self.op_io.values():
      # A = a depthwise output: the group reads the depthwise input
      total += self._dw_reads.get(a_id, a_bytes) + rest
    if not dense_heads:
      total -= 4 * self.B * self.out_h * self.out_w * (4 * self.num_objs * self.num_frags)
    return total

  # ----------------------------------------------------------- running ---
  def _stream(self):
    return C.stream_handle(self.dev)[1]

  def sync_current(self):
    torch.cuda.current_stream(self.dev).synchronize()

  def run_plan(self, with_post=True, sparse=False, skip_kinds=()):
    """sparse=False: the whole dense plan. sparse=True: trunk + object head +
    object softmax/argmax only (the fragment heads follow per target object).
    skip_kinds: op kinds left out (capture_alt: the plan WITHOUT its GEMM / depthwise
    launches, for the step decomposition of bench.py). 'post' leaves out the in-place
    softmax / argmax post-ops: without the GEMMs the head buffers keep the probabilities
    of the last full run, and softmax applied to them again and again would flatten them
    (the stages downstream would then see no -- or, with one object, all -- pixels)."""
    s = self._stream()
    if not sparse:
      for name, fn in self.ops:
        if self.op_kind.get(name) not in skip_kinds:
          fn(s)
      if with_post and 'post' not in skip_kinds:
        for name, fn in self.post_ops:
          fn(s)
      return
    for name, fn in self.ops[:self._n_trunk_ops]:
      fn(s)
    self._obj_head_op[1](s)
    for name, fn in self.post_ops:
      if name != 'softmax_frag':
        fn(s)

  # ------------------------------------------------------- sparse heads ---
  def _build_sparse_packs(self):
    O, F = self.num_objs, self.num_frags
    wc, bc = self._conv_params('logits/' + W.PRED_FRAG_CONF, None)[::2]
    wl, bl = self._conv_params('logits/' + W.PRED_FRAG_LOC, None)[::2]
    self._sparse_packs = [
        (self.mode.sparse_weights(wc[:, o * F:(o + 1) * F], bc[o * F:(o + 1) * F]),
         self.mode.sparse_weights(wl[:, o * 3 * F:(o + 1) * 3 * F],
                                  bl[o * 3 * F:(o + 1) * 3 * F]))
        for o in range(O)]

  def run_sparse_heads(self, slots, slots_dev):
    """Fragment heads (model.py:449-456) + fragment softmax (model.py:678) for the
    given (image, obj_id) slots only: per slot one 256 -> F and one 256 -> 3F GEMM
    writing the object's channel slice of the dense head buffers, as grouped
    launches. Channels of other objects are left untouched (never read: the
    correspondence stage only visits the slots, corresp.py:42-43).
    slots_dev: int32 [S,2] device copy of ``slots`` for the softmax kernel."""
    if self._sparse_packs is None:
      self._build_sparse_packs()
    O, F = self.num_objs, self.num_frags
    P = self.out_h * self.out_w
    x = self._decoder_x
    s = self._stream()
    flops = 0
    for kind, buf in enumerate((self.logits[W.PRED_FRAG_CONF], self.logits[W.PRED_FRAG_LOC])):
      n = F if kind == 0 else 3 * F
      ldc = O * n
      probs = [self.mode.sparse_problem(self._sparse_packs[obj_id - 1][kind], x, im * P * 256,
                                        buf, im * P * ldc + (obj_id - 1) * n, ldc, P, n)
               for im, obj_id in slots]
      flops += 2 * P * n * 256 * len(slots)
      for i in range(0, len(probs), 8):
        self.mode.sparse_launch(probs[i:i + 8], s)
    if slots:
      _lib.check(self.lib.epos_softmax_slots_f32(_ptr(self.logits[W.PRED_FRAG_CONF]),
                                                 _ptr(slots_dev), len(slots), P, O, F, s),
                 'softmax_slots')
    return flops

  # ------------------------------------------------------ weight update ---
  def _need_fp32_plan(self, what, device=True):
    if self.precision != 'fp32':
      raise NotImplementedError('%s: precision=%r nets are not supported' % (
          what, self.precision))
    if device and self.lib is None:
      raise _lib.EposError('%s needs a HIP device (there is no CPU fallback)' % what)

  def _checked_variables(self, variables):
    """set_weights' argument check against weights.TRAINABLE_LAYERS: [(scope, [the layer's
    variables in weights.layer_variables' order, as given])], the logits layers first, sorted,
    then the others in the table's order. Raises before anything is uploaded or enqueued."""
    given = {}
    for key, v in variables.items():
      if key not in W.TRAINABLE_VARIABLES:
        raise ValueError('%r is not a variable whose weights can be replaced (%s)' % (
            key, ', '.join(W.TRAINABLE_VARIABLES)))
      scope, short = W.TRAINABLE_VARIABLES[key]
      k, n, _ = self.mode.packs[scope]
      shapes = W.variable_shapes(short, k, n)
      if isinstance(v, torch.Tensor):
        if v.dtype != torch.float32:
          raise TypeError('%s must be torch.float32, got %s' % (key, v.dtype))
        if v.device != self.dev:
          raise ValueError('%s is on %s, the net on %s (numpy arrays are uploaded)' % (
              key, v.device, self.dev))
        if not v.is_contiguous():
          raise ValueError('%s must be contiguous' % key)
      else:
        v = np.asarray(v)
        if v.dtype.kind != 'f':
          raise TypeError('%s must be a floating-point array, got %s' % (key, v.dtype))
      if tuple(v.shape) not in shapes:
        raise ValueError('%s must have shape %s, got %s' % (
            key, ' or '.join(str(list(s)) for s in shapes), list(v.shape)))
      given.setdefault(scope, {})[short] = v
    out = []
    for scope in sorted(s for s in given if s in W.LOGITS_LAYERS) + [
        s for s in W.TRAINABLE_LAYERS if s in given and s not in W.LOGITS_LAYERS]:
      shorts = W.layer_variables(scope)
      if len(given[scope]) != len(shorts):
        raise ValueError('%s: %s and %s are set together' % (
            scope, ', '.join(shorts[:-1]), shorts[-1]))
      out.append((scope, [given[scope][short] for short in shorts]))
    return out

  def set_weights(self, variables, check=True):
    """Replaces the weights of layers of weights.TRAINABLE_LAYERS in place, on the device.
    variables: {'<scope>/weights': [1,1,K,N] or [K,N], '<scope>/biases': [N]} for any subset of
    logits/pred_obj_conf, pred_frag_conf and pred_frag_loc, and '<scope>/weights',
    '<scope>/BatchNorm/gamma' and '<scope>/BatchNorm/beta' [N] of decoder/decoder_conv1_pointwise
    (a layer's variables together); values are contiguous fp32 tensors on the net's device
    (trainer.Optimizer.params as it is) or numpy arrays, which are uploaded. A wrong name, shape,
    dtype or device raises ValueError / TypeError before anything is enqueued. The moving
    statistics of a batch norm are the checkpoint's: inputs, never changed.

    A batch norm is folded on the device, bit for bit as weights.fold_bn and the plan's host
    fold do (scale = gamma / sqrt(var + eps) and bias = beta - mean * scale in fp64, each
    operation rounded once, both rounded to fp32; the matrix is weights * scale in fp32). One
    grouped epos_pack_weights_device_f32 call on the current stream then packs every matrix
    into the very tensors the plan's launch arguments point at, together with the per-object
    packs of the sparse heads (built first if they were not): no pointer changes, so forward(),
    forward_logits(), every graph captured before the call, the pipeline's and the stand-alone
    object head use the new weights on their next run. A layer whose fp16-pair weights the host
    packer refused when the plan was built gets its other layouts only. self.ckpt is NOT
    updated (that would take a download): it keeps the weights the net was built from.

    All or nothing, for all the layers given together: when the packer refuses one (a
    non-finite weight, or a column whose fp16-pair scale leaves 2^+-100) nothing is written and
    the net holds its previous weights. check=True reads the status words back (one small
    synchronising copy) and raises EposError naming the layer; check=False does not
    synchronise. Returns the status tensor (int32, on the device, one word per packed matrix:
    the logits layers in sorted order, then per fragment layer its num_objs sparse packs, then
    one word per batch-norm layer; 0 = written).

    Ordering is the caller's: the update is enqueued on the current stream, and a forward in
    flight on ANOTHER stream must be ordered against it by the caller (nothing here records or
    waits for events). fp32 single-scale nets with num_objs <= 126 only."""
    self._need_fp32_plan('set_weights', device=False)
    layers = self._checked_variables(variables)
    self._need_fp32_plan('set_weights')
    if len(W.TRAINABLE_LAYERS) + 2 * self.num_objs > 256:
      raise NotImplementedError('set_weights: more than 126 objects')
    if not layers:
      return torch.zeros(0, dtype=torch.int32, device=self.dev)
    with C.launch(self.dev) as q:
      packed, keep = self._pack_problems(layers)
      q.keep(*keep)                      # uploaded copies outlive the call
      status = torch.empty(len(packed), dtype=torch.int32, device=self.dev)
      self.mode.pack_launch([p[0] for p in packed], status, q.handle)
    if check:
      bad = [packed[i][1:] for i in torch.nonzero(status.cpu()).flatten().tolist()]
      bad = ['%s (sparse pack of object %d)' % b if b[1] else b[0] for b in bad]
      if bad:
        raise _lib.EposError(
            'set_weights: the fp16-pair packer refused %s (a non-finite weight, or '
            'a column whose scale leaves 2^+-100); nothing was written, the net still holds its '
            'previous weights' % ', '.join(bad))
    return status

  def _pack_problems(self, layers):
    """([(problem, scope, object id of a sparse pack or 0)], tensors to keep alive) of the
    device packer for layers as _checked_variables returns them: the logits layers' packs, then
    per fragment layer its num_objs sparse packs, then the folded batch-norm layers' packs."""
    O, F = self.num_objs, self.num_frags
    sparse_n = {'logits/' + W.PRED_FRAG_CONF: (0, F), 'logits/' + W.PRED_FRAG_LOC: (1, 3 * F)}
    if self._sparse_packs is None and any(scope in sparse_n for scope, _ in layers):
      self._build_sparse_packs()         # from self.ckpt, while it still describes the net
    dense, sparse, folded, keep = [], [], [], []
    for scope, values in layers:
      k, n, pack = self.mode.packs[scope]
      w, *rest = (torch.as_tensor(v, dtype=torch.float32).to(self.dev) for v in values)
      w = w.reshape(k, n)
      eps = W.TRAINABLE_LAYERS[scope]
      if eps is None:
        b = rest[0]
      else:
        gamma, beta = rest
        mean, var = self.layer_constants(scope)
        scale = gamma.double() / torch.sqrt(var.double() + eps)
        b = (beta.double() - mean.double() * scale).float()
        w = (w * scale.float()[None, :]).contiguous()
      keep += [w, b]
      (dense if eps is None else folded).append(
          (self.mode.pack_problem(pack, w, b, 0, n), scope, 0))
      if scope in sparse_n:
        kind, width = sparse_n[scope]
        for o in range(O):
          sparse.append((self.mode.pack_problem(self._sparse_packs[o][kind], w, b, o * width,
                                                width), scope, o + 1))
    return dense + sparse + folded, keep

  # ------------------------------------------- the layer below the logits ---
  def pointwise_operand(self, name=W.DECODER_CONV1_POINTWISE):
    """What the backward pass of a trainable 1x1 conv layer needs of the plan, as it was
    recorded while the plan was built: {'a': the layer's input, the depthwise output buffer
    [B,h,w,lda] the net keeps alive; 'lda', 'm', 'k', 'n'; 'presplit': whether that buffer holds
    fp16 pairs (the default; EPOS_H2_PRESPLIT=0, EPOS_GEMM_H2=0 or fp16-pair weights the host
    packer refused give fp32); 'a_h2': None for an fp32 A, else (slot words, second slot's words
    or None, gain, bias), the very values the layer's PointwiseArgs carry; 'packs': the (plain,
    bias, split, fp16-pair) weight tensors its launch points at; 'eps': the batch norm's}."""
    self._need_fp32_plan('pointwise_operand')
    if name not in W.TRAINABLE_LAYERS or name not in self.mode.layer_operands:
      raise ValueError('%r is not a trainable layer (%s)' % (
          name, ', '.join(n for n in self.mode.layer_operands if n in W.TRAINABLE_LAYERS)))
    return self._pointwise_record(name, self.mode.packs[name][2], W.TRAINABLE_LAYERS[name])

  def _pointwise_record(self, name, packs, eps):
    a, lda, m, k, n, args, ab = self.mode.layer_operands[name]
    presplit = bool(args.a_presplit)
    a_h2 = None
    if presplit:
      a_h2 = (self.mode.slot_words(ab[0]), self.mode.slot_words(ab[1]), float(args.a_gain),
              float(args.a_bias))
    return {'a': a, 'lda': lda, 'm': m, 'k': k, 'n': n, 'presplit': presplit, 'a_h2': a_h2,
            'packs': packs, 'eps': eps}

  def crossed_pointwise_operand(self, name):
    """pointwise_operand for a 1x1 conv layer of weights.POINTWISE_CHAIN_LAYERS, which the
    backward pass crosses without training it: the same record, with 'packs' None (nothing
    repacks its weights) and 'eps' from that table. pointwise_operand itself keeps refusing
    these names: it answers for the layers EposNet.set_weights updates."""
    self._need_fp32_plan('crossed_pointwise_operand', device=False)
    if name not in W.POINTWISE_CHAIN_LAYERS or name not in self.mode.layer_operands:
      raise ValueError('%r is not a 1x1 layer the backward pass crosses (%s)' % (
          name, ', '.join(W.POINTWISE_CHAIN_LAYERS)))
    return self._pointwise_record(name, None, W.POINTWISE_CHAIN_LAYERS[name])

  def pointwise_constants(self, name):
    """(weights [1,1,K,N], gamma, moving_mean, moving_variance [N]) of a layer of
    weights.POINTWISE_CHAIN_LAYERS on the device, f32, uploaded from the checkpoint once and
    kept, as depthwise_constants keeps a depthwise layer's: nothing updates these variables."""
    if name not in W.POINTWISE_CHAIN_LAYERS:
      raise ValueError('%r is not a 1x1 layer the backward pass crosses (%s)' % (
          name, ', '.join(W.POINTWISE_CHAIN_LAYERS)))
    if name not in self._pw_consts:
      self._pw_consts[name] = tuple(
          torch.from_numpy(np.ascontiguousarray(self.ckpt[name + '/' + v], np.float32)).to(self.dev)
          for v in ('weights', 'BatchNorm/gamma', 'BatchNorm/moving_mean',
                    'BatchNorm/moving_variance'))
    return self._pw_consts[name]

  def aspp_operands(self):
    """The buffers and launch records the backward pass through ASPP reads (trainer.aspp_grads),
    as they were recorded while the plan was built (a dry run records them too); the net keeps
    them alive. {'encoder': [B,eh,ew,ec] channels of the encoder output, the input of all five
    branches; 'encoder_relu': whether the plan's expression for it is a ReLU (Xception's exit
    flow, the ResNet units) -- only then is it the mask of the gradient at its pre-activation;
    'pooled': [B,ec], its mean, image_pooling's input; 'pool_feat': [B,256], image_pooling's
    output behind its ReLU; 'aspp_concat': [B,eh,ew,256 (2 + rates)]; 'rates'; 'pointwise':
    {scope: the record crossed_pointwise_operand gives, 'packs' None} for image_pooling, aspp0
    and aspp<i>_pointwise; 'depthwise': {scope: the record depthwise_operand gives} for
    aspp<i>_depthwise}."""
    self._need_fp32_plan('aspp_operands', device=False)
    r = self._aspp
    B, eh, ew, ec = self.B, r['eh'], r['ew'], r['ec']
    return {'encoder': r['encoder'].view(B, eh, ew, -1)[..., :ec],
            'encoder_relu': r['encoder_relu'], 'pooled': r['pooled'],
            'pool_feat': r['pool_feat'], 'aspp_concat': r['aspp_concat'],
            'rates': self.atrous_rates,
            'pointwise': {s: self._pointwise_record(s, None, eps)
                          for s, eps in self._aspp_pw.items()},
            'depthwise': {s: dict(self._dw_operands[s]) for s in self._aspp_dw}}

  def aspp_constants(self, scope):
    """(weights [1,1,K,256] or depthwise_weights [3,3,ec,1], gamma, moving_mean,
    moving_variance) of an ASPP layer (weights.aspp_layers) on the device, f32, uploaded from
    the checkpoint once and kept, as pointwise_constants and crossed_depthwise_constants keep
    theirs: nothing updates these variables."""
    if scope not in self._aspp_pw and scope not in self._aspp_dw:
      raise ValueError('%r is not an ASPP layer (%s)' % (
          scope, ', '.join(list(self._aspp_pw) + list(self._aspp_dw))))
    kept = self._pw_consts if scope in self._aspp_pw else self._dw_consts
    if scope not in kept:
      first = 'weights' if scope in self._aspp_pw else 'depthwise_weights'
      kept[scope] = tuple(
          torch.from_numpy(np.ascontiguousarray(self.ckpt[scope + '/' + v], np.float32)).to(self.dev)
          for v in (first, 'BatchNorm/gamma', 'BatchNorm/moving_mean',
                    'BatchNorm/moving_variance'))
    return kept[scope]

  def chain_operands(self):
    """The buffers the backward pass through the decoder reads (trainer.decoder_grads), as they
    were recorded while the plan was built (a dry run records them too); the net keeps them
    alive. {'decoder_concat': [B,h,w,304] = [resize(concat_projection) : 256 |
    feature_projection0 : 48], the input of decoder_conv0_depthwise; 'concat_projection':
    [B,eh,ew,256] behind its ReLU; 'aspp_concat': [B,eh,ew,1280], concat_projection's input;
    'low_level': the backbone's tap, feature_projection0's input, as [B,lh,lw,c] channels;
    'low_level_hw', 'encoder_hw', 'decoder_hw': the three sizes}."""
    self._need_fp32_plan('chain_operands', device=False)
    r = self._chain
    ll, (lh, lw) = r['low_level'], r['low_level_hw']
    return {'decoder_concat': r['decoder_concat'][..., :304],
            'concat_projection': r['concat_projection'], 'aspp_concat': r['aspp_concat'],
            'low_level': ll.view(self.B, lh, lw, -1)[..., :r['low_level_c']],
            'low_level_hw': (lh, lw), 'encoder_hw': r['encoder_hw'],
            'decoder_hw': r['decoder_hw']}

  def depthwise_operand(self, name=W.DECODER_CONV1_DEPTHWISE):
    """What the backward pass through a 3x3 depthwise layer of
    weights.DEPTHWISE_BACKWARD_LAYERS needs of the plan, as it was recorded while the plan was
    built (a dry run records it too): {'x': the layer's input, the buffer [B,h,w,ldx] the layer
    below writes behind its ReLU and the net keeps alive; 'ldx', 'b', 'h', 'w', 'c', 'rate';
    'w9c': the folded weights f32 [9,c] and 'bias': the folded bias f32 [c] its launch reads;
    'eps': the batch norm's}. The layer's output is EposNet.pointwise_operand's 'a'."""
    return self._depthwise_record('depthwise_operand', name, W.DEPTHWISE_BACKWARD_LAYERS)

  def crossed_depthwise_operand(self, name=W.DECODER_CONV0_DEPTHWISE):
    """depthwise_operand for a layer of weights.DEPTHWISE_CHAIN_LAYERS: the same record. For
    decoder_conv0_depthwise 'x' is the decoder's concat buffer, [resize(concat_projection) : 256
    | feature_projection0 : 48], of which only the last 48 channels lie behind a ReLU of their
    own; its output is crossed_pointwise_operand('decoder/decoder_conv0_pointwise')'s 'a'."""
    return self._depthwise_record('crossed_depthwise_operand', name, W.DEPTHWISE_CHAIN_LAYERS)

  def _depthwise_record(self, what, name, table):
    self._need_fp32_plan(what, device=False)
    if name not in table or name not in self._dw_operands:
      raise ValueError('%r is not a depthwise layer the backward pass crosses (%s)' % (
          name, ', '.join(table)))
    return dict(self._dw_operands[name])

  def depthwise_constants(self, name=W.DECODER_CONV1_DEPTHWISE):
    """(depthwise_weights [3,3,C,1], gamma, moving_mean, moving_variance [C]) of a layer of
    weights.DEPTHWISE_BACKWARD_LAYERS on the device, f32, uploaded from the checkpoint once and
    kept: nothing updates that layer's variables, and a backward pass that asks for them enqueues
    no copy and waits for none."""
    return self._depthwise_consts(name, W.DEPTHWISE_BACKWARD_LAYERS)

  def crossed_depthwise_constants(self, name=W.DECODER_CONV0_DEPTHWISE):
    """depthwise_constants for a layer of weights.DEPTHWISE_CHAIN_LAYERS."""
    return self._depthwise_consts(name, W.DEPTHWISE_CHAIN_LAYERS)

  def _depthwise_consts(self, name, table):
    if name not in table:
      raise ValueError('%r is not a depthwise layer the backward pass crosses (%s)' % (
          name, ', '.join(table)))
    if name not in self._dw_consts:
      self._dw_consts[name] = tuple(
          torch.from_numpy(np.ascontiguousarray(self.ckpt[name + '/' + v], np.float32)).to(self.dev)
          for v in ('depthwise_weights', 'BatchNorm/gamma', 'BatchNorm/moving_mean',
                    'BatchNorm/moving_variance'))
    return self._dw_consts[name]

  def layer_constants(self, name=W.DECODER_CONV1_POINTWISE):
    """(moving_mean, moving_variance) of a trainable layer's batch norm on the device, f32 [N],
    uploaded from the checkpoint once: training never changes them."""
    if name not in self._layer_consts:
      self._layer_consts[name] = tuple(
          torch.from_numpy(np.ascontiguousarray(self.ckpt[name + '/BatchNorm/' + v],
                                                np.float32)).to(self.dev)
          for v in ('moving_mean', 'moving_variance'))
    return self._layer_consts[name]

  def set_images(self, images):
    """images: [B,H,W,3] in [0,255] (host numpy or device tensor), float32 -- or uint8 as the
    decoder delivers them (datagen.py:435-436 casts to float32 right behind decode_image; here
    the bytes are uploaded and cast on the device, epos_u8_to_f32). Enqueued on the current
    stream; a pinned host tensor is uploaded without blocking the host."""
    t = torch.as_tensor(images)
    if t.dtype == torch.uint8:
      n = self.B * self.H * self.W * 3
      t = t.reshape(-1)
      if t.numel() != n:
        raise ValueError('images: expected %d values, got %d' % (n, t.numel()))
      if not t.is_cuda and t.is_pinned() and t.is_contiguous() and t.data_ptr() % 16 == 0 and \
          os.environ.get('EPOS_UPLOAD', 'zerocopy') == 'zerocopy':
        # pinned host memory is mapped into the device's address space: the cast kernel reads
        # the bytes over PCIe itself (0.9 MB per 640 x 480 frame) -- no copy engine, no
        # cross-engine dependency in front of the step's first kernel. The caller keeps the
        # buffer untouched until the step has been collected. EPOS_UPLOAD=copy: H2D copy first.
        src = t
      else:
        if self._images_u8 is None:
          self._images_u8 = torch.empty(n, dtype=torch.uint8, device=self.dev)
        self._images_u8.copy_(t, non_blocking=True)
        src = self._images_u8
      _lib.check(self.lib.epos_u8_to_f32(_ptr(src), _ptr(self.images), n, self._stream()),
                 'u8_to_f32')
      return
    if t.dtype != torch.float32:
      if t.is_cuda:
        raise TypeError('device images must be float32 or uint8, got %s' % t.dtype)
      t = t.float()
    self.images.copy_(t.reshape(self.B, self.H, self.W, 3), non_blocking=True)

  def capture_graph(self, sparse=False):
    """Captures the plan (dense, or the sparse-mode trunk) into one hipGraph."""
    torch.cuda.synchronize(self.dev)
    side = _capture_stream(self.dev)
    with torch.cuda.stream(side):
      self.run_plan(sparse=sparse)         # warm-up outside capture
    torch.cuda.synchronize(self.dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
      self.run_plan(sparse=sparse)
    if sparse:
      self._graph_sparse = g
    else:
      self._graph = g
    return g

  def capture_alt(self, skip_kinds):
    """A second hipGraph of the dense plan without the launches of the given kinds
    ('gemm', 'dw'); forward(use_graph=True) replays it while `alt_skip` is set. bench.py
    times the same pipelined steps with it: step time - that time = what the left-out
    kernels cost INSIDE the timed regime (overlap with the other plans included)."""
    if skip_kinds is None:
      self._graph_alt, self.alt_skip = None, None
      return
    torch.cuda.synchronize(self.dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=_capture_stream(self.dev)):
      self.run_plan(skip_kinds=tuple(skip_kinds))
    self._graph_alt, self.alt_skip = g, tuple(skip_kinds)

  def forward(self, images=None, use_graph=False, sparse=False):
    """Runs the plan (logits + softmax/argmax post-ops) on the current stream and
    returns the prediction dict of ``model.predict`` (model.py:629-687) as views
    of the plan's HBM buffers (valid until the next forward)."""
    if images is not None:
      self.set_images(images)
    if use_graph:
      if sparse:
        if self._graph_sparse is None:
          self.capture_graph(sparse=True)
        self._graph_sparse.replay()
      elif self._graph_alt is not None:
        self._graph_alt.replay()
      else:
        if self._graph is None:
          self.capture_graph()
        self._graph.replay()
    else:
      self.run_plan(sparse=sparse)
    return self.outputs()

  def forward_logits(self, images=None, use_graph=False):
    """Runs the dense plan WITHOUT the softmax / argmax post-ops of model.py:677-683 and
    returns the raw logits (model.py:396-458, reshaped as model.py:117-147) as views of the
    head buffers, valid until the next run: {pred_obj_conf [B,h,w,O+1], pred_frag_conf
    [B,h,w,O,F], pred_frag_loc [B,h,w,O,F,3]}. What epos_amd/loss.py computes the training
    losses from: a cross-entropy taken from fp32 probabilities is inf as soon as the target's
    probability underflows. use_graph replays a captured graph of its own; forward(), its graph
    and the pipeline are untouched. The head buffers are shared with forward(): outputs()
    after forward_logits() shows logits (and the label map of the last forward()), and the
    next forward() overwrites them with probabilities again. The three logits layers read
    self.decoder_out ([B,h,w,256], fp32; a bf16 tensor in bf16 mode), valid as long: the tensor to
    put torch's own convolutions on when fine-tuning those layers against
    loss.differentiable_losses."""
    if images is not None:
      self.set_images(images)
    if use_graph:
      if self._graph_logits is None:
        torch.cuda.synchronize(self.dev)
        side = _capture_stream(self.dev)
        with torch.cuda.stream(side):
          self.run_plan(with_post=False)     # warm-up outside capture
        torch.cuda.synchronize(self.dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
          self.run_plan(with_post=False)
        self._graph_logits = g
      self._graph_logits.replay()
    else:
      self.run_plan(with_post=False)
    out = self.outputs()
    del out[W.PRED_OBJ_LABEL]
    return out

  def outputs(self):
    """The prediction dict of the LAST dense run as views of the plan's HBM buffers (no
    launch): what forward() returned, for callers that read the heads after a pipeline
    step (infer.py --vis / --save_corresp). After forward_logits() the three heads hold raw
    logits, not probabilities."""
    B, h, w = self.B, self.out_h, self.out_w
    O, F = self.num_objs, self.num_frags
    return {
        W.PRED_OBJ_CONF: self.logits[W.PRED_OBJ_CONF],
        W.PRED_OBJ_LABEL: self.obj_label,
        W.PRED_FRAG_CONF: self.logits[W.PRED_FRAG_CONF].view(B, h, w, O, F),
        W.PRED_FRAG_LOC: self.logits[W.PRED_FRAG_LOC].view(B, h, w, O, F, 3),
    }

  def time_ops(self, iters=3, warm=0):
    """Per-launch HIP-event timing of the plan (diagnostics). `warm` extra
    untimed launches per op let the core clock ramp (2.06 -> 2.4 GHz)."""
    out = []
    s = self._stream()
    for name, fn in self.ops:
      for _ in range(1 + warm):
        fn(s)
      torch.cuda.synchronize(self.dev)
      e0 = torch.cuda.Event(enable_timing=True)
      e1 = torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(iters):
        fn(s)
      e1.record()
      torch.cuda.synchronize(self.dev)
      out.append((name, e0.elapsed_time(e1) / iters, self.op_flops.get(name, 0)))
    return out
