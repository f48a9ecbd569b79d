"""The numeric modes of the EposNet plan (epos_amd/net.py): every launch decision that depends
on the precision. net.py walks the network graph once, writes the structure trace and calls the
operations below; each mode chooses its kernels, packs its weights and keeps its own
bookkeeping. Entry points are looked up once, when the plan is built.

  * Fp32Mode (precision='fp32', the default): fp32 activations, the split-operand (bf16 x 6)
    and fp16-pair GEMMs, the absmax slots that feed the fp16-pair kernels, presplit depthwise
    outputs, the implicit 3x3 conv, and the pool / amax-clear folds.
  * Bf16Mode (precision='bf16'): bf16 activations and weights on the bf16 kernels
    (csrc/bf16.hip), one shared im2col scratch; the image-pooling 1x1 and the logits stay fp32.
"""
import ctypes
import os

import numpy as np
import torch

from epos_amd import _lib
from epos_amd._call import ptr as _ptr
from epos_amd import weights as W


def _fold(w_kn, scale, kmult):
  """A layer's fp32 weight matrix: the BN scale folded into w_kn [K, N] (TF HWIO with the
  spatial taps flattened into K), K zero-padded to a multiple of kmult."""
  k, n = w_kn.shape
  w = w_kn.astype(np.float32) * scale[None, :].astype(np.float32)
  kpad = -(-k // kmult) * kmult
  if kpad != k:
    w = np.concatenate([w, np.zeros((kpad - k, n), np.float32)], 0)
  return np.ascontiguousarray(w)


def _pack(fn, w, dtype):
  """A packer's size-then-fill call on the folded matrix w; None when it refuses w."""
  src = w.ctypes.data_as(ctypes.c_void_p)
  total = fn(src, w.shape[0], w.shape[1], None)
  if total <= 0:
    return None
  dst = np.empty(total, dtype)
  fn(src, w.shape[0], w.shape[1], dst.ctypes.data_as(ctypes.c_void_p))
  return dst


def _bias(bias, n, mult):
  b = np.zeros(-(-n // mult) * mult, np.float32)
  b[:n] = bias
  return b


class Fp32Mode(object):
  """fp32 activations (NHWC, the reference's dtype), rows padded to 32 floats."""

  dtype, line = torch.float32, 32
  MAX_SLOTS = 512

  def __init__(self, net):
    self.net = net
    fn = net._fn
    self.gemm = fn('epos_pointwise_conv_grouped_f32')
    self.gemm1 = fn('epos_pointwise_conv_f32')
    self.heads = fn('epos_heads_gemm_f32')
    self.dw = fn('epos_depthwise3x3_f32')
    self.conv3x3 = fn('epos_conv3x3_f32')
    self.im2col3x3 = fn('epos_im2col3x3_f32')
    self.im2col_k = fn('epos_im2col_f32')
    self.absmax = fn('epos_absmax_f32')
    self.amax_clear = fn('epos_amax_clear')
    self.avg_pool = fn('epos_global_avg_pool_f32')
    self.avg_pool_partial = fn('epos_global_avg_pool_partial_f32')
    self.resize_fn = fn('epos_resize_bilinear_f32')
    self.subsample = fn('epos_subsample_f32')
    self.add_relu = fn('epos_add_relu_f32')
    self.maxpool = fn('epos_maxpool3x3_s2_f32')
    self.pack_plain = fn('epos_pack_pointwise_weights')
    self.pack_split = fn('epos_pack_pointwise_weights_split')
    self.pack_h2 = fn('epos_pack_pointwise_weights_h2')
    # Absmax slots (include/epos_hip.h): the fp16-pair GEMM scales its fp32 A operand by a
    # power of two taken from an upper bound of max|A|; the producers of every activation
    # tensor keep that bound in a slot (GEMM epilogues by atomic max). `_bounds` maps a
    # buffer to (slot, slot2, gain, bias): bound = gain * max(slot, slot2) + bias. The
    # table is zeroed by the plan's first op, which reads the slot count when it launches.
    self._amax_table = torch.zeros(self.MAX_SLOTS * _lib.AMAX_WORDS, dtype=torch.int32,
                                   device=net.dev)
    self._slot_count = ctypes.c_int64(0)
    self._bounds = {}
    # fp16-pair GEMM switches of the library (A/B runs): with either off no layer gets
    # fp16-pair weights. EPOS_H2_PRESPLIT (default 1 since round 4, 0 = off): the depthwise
    # kernels write their outputs already split (fp16 pairs), so each activation is converted
    # once instead of once per column tile of the GEMM and the GEMM loop carries no
    # conversion. Bit-identical results. Per launch the GEMMs gain 7 % (34.9 vs 37.4 us on
    # average over the plan, profiles/r04/presplit_ab.txt) while the depthwise launches pay
    # most of it back inside the pipelined step (+0.055 ms of depthwise slot time vs -0.02 ms
    # of GEMM and -0.05 ms of the rest): 417.5 / 419.8 vs 415.4 / 417.2 images/s, same box --
    # a small but repeatable gain (round 3 measured it neutral and kept it off).
    self.use_h2 = (os.environ.get('EPOS_GEMM_H2', '1') != '0' and
                   os.environ.get('EPOS_GEMM_SPLIT', '1') != '0')
    self.use_presplit = self.use_h2 and os.environ.get('EPOS_H2_PRESPLIT', '1') == '1'
    self._dw_h2 = {}           # id(depthwise output) -> its (mutable) launch arguments
    self.h2_layers, self.h2_refused, self.presplit_layers = [], [], []
    # layer of weights.TRAINABLE_LAYERS -> (K, N, the (wp, bp, ws, wh) tensors its launch
    # arguments point at): where EposNet.set_weights packs updated weights (references only;
    # wh None = refused)
    self.packs = {}
    # trainable layer below the logits -> what its backward pass needs:
    # (A buffer, lda, M, K, N, the launch's PointwiseArgs, A's bound or None)
    self.layer_operands = {}
    self.pack_device = fn('epos_pack_weights_device_f32')
    self._last_pw = None       # (C, args, foldable): the last stand-alone 1x1 launch
    self._first_im2col = None  # (op name, args, capacity in words): the plan's first im2col

  @property
  def _n_slots(self):
    return self._slot_count.value

  # ------------------------------------------------------- absmax slots ---
  def _new_slot(self):
    i = self._slot_count.value
    if i >= self.MAX_SLOTS:
      raise _lib.EposError('absmax slot table exhausted')
    self._slot_count.value = i + 1
    return i

  def _slot_ptr(self, i):
    return _ptr(self._amax_table, i * _lib.AMAX_WORDS) if i is not None else None

  def _set_bound(self, buf, slot, slot2=None, gain=0.0, bias=0.0):
    self._bounds[id(buf)] = (slot, slot2, float(gain), float(bias))

  def _out_slot(self, buf, n, ldc, off=0):
    """Slot that a GEMM writing `buf` publishes max|out| into, or None when its epilogue
    cannot (rows not float4-able). Writers of one (concat) buffer share the slot."""
    if n % 4 or ldc % 4 or off % 4:
      return None
    b = self._bounds.get(id(buf))
    if b is not None and b[1] is None and b[2] == 0.0:
      return b[0]
    slot = self._new_slot()
    self._set_bound(buf, slot)
    return slot

  def same_bound(self, dst, src):
    """dst is bounded like src (a subsample or max-pool of it)."""
    b = self._bounds.get(id(src))
    if b is not None:
      self._bounds[id(dst)] = b

  def concat_bound(self, cat, left):
    """cat = [bilinear resize of `left` | the GEMM output that owns cat's slot]: an
    interpolation never exceeds its input's absmax, so cat is bounded by the two slots."""
    lb, cb = self._bounds.get(id(left)), self._bounds.get(id(cat))
    if lb is not None and cb is not None:
      self._set_bound(cat, cb[0], lb[0])
    else:
      self._bounds.pop(id(cat), None)

  def track_absmax(self, name, y, ld, rows, n):
    """y (written by a kernel without an absmax epilogue) gets a slot of its own."""
    slot = self._new_slot()
    self._set_bound(y, slot)
    self.net._launch(name, self.absmax, (_ptr(y), ld, rows, n, self._slot_ptr(slot)))

  def join_absmax(self, name, x, ld, rows, n, into):
    """max|x| joins the slot of `into` (x is written into it without a GEMM epilogue)."""
    b = self._bounds.get(id(into))
    if b is not None:
      self.net._launch(name, self.absmax, (_ptr(x), ld, rows, n, self._slot_ptr(b[0])))

  # ------------------------------------------------------ weight packing ---
  def _weights(self, name, conv, h2):
    """(wp, bp, ws, wh, kpad): the layer's folded weights in the plain and the split GEMM
    layouts (epos_pack_pointwise_weights[_split]), its bias, and with `h2` the fp16-pair copy
    with per-column power-of-two scales (epos_pack_pointwise_weights_h2) -- None when the
    packer refuses the matrix (a weight outside the window fp16 pairs represent): the layer
    then stays on the bf16 x 6 kernel. A named layer is listed in h2_layers / h2_refused."""
    w_kn, scale, bias = conv
    k, n = w_kn.shape
    kpad = -(-k // 4) * 4
    net = self.net
    if net.dry_run:
      wp, bp, ws, wh = net._empty(1), net._empty(1), net._empty(1), None
      if h2:
        wh = net._empty(1)
    else:
      w = _fold(w_kn, scale, 4)
      wh = _pack(self.pack_h2, w, np.uint8) if h2 else None
      wh = net._dev(wh) if wh is not None else None
      wp, bp = net._dev(_pack(self.pack_plain, w, np.float32)), net._dev(_bias(bias, n, 128))
      ws = net._dev(_pack(self.pack_split, w, np.uint8))
    if h2 and name is not None:
      (self.h2_layers if wh is not None else self.h2_refused).append(name)
    return wp, bp, ws, wh, kpad

  # --------------------------------------------------------------- ops ---
  def begin(self):
    self.net._launch('amax_clear', self.amax_clear, (_ptr(self._amax_table), self._slot_count))

  def pointwise(self, name, a, a_off, lda, m, k, conv, c, c_off, ldc, relu, res=None, res_off=0,
                ldr=0, sub=1, ho=0, wo=0, hi=0, wi=0, group=None, track_out=True):
    """One 1x1 conv on the split-operand GEMM, or on the fp16-pair GEMM when A has a bound.
    With ``group`` (a list) the problem is only appended to it (see flush)."""
    net = self.net
    ab = self._bounds.get(id(a)) if self.use_h2 else None
    wp, bp, ws, wh, kpad = self._weights(name, conv, ab is not None and m > 8)
    n = conv[0].shape[1]
    assert kpad == k or (kpad > k and lda >= kpad), (name, k, kpad, lda)
    if name in W.TRAINABLE_LAYERS:
      assert kpad == k, name
      self.packs[name] = (k, n, (wp, bp, ws, wh))
    # A = the output of a depthwise conv that was set up to write fp16 pairs: keep that
    # only if this GEMM really runs on the fp16-pair kernel (the packer may have refused
    # the weights); the depthwise arguments are the very struct its launch passes
    dwa = self._dw_h2.pop(id(a), None)
    presplit = False
    if dwa is not None:
      presplit = wh is not None and sub == 1 and a_off == 0
      dwa.y_h2 = int(presplit)
      if presplit:
        self.presplit_layers.append(name)
    track = track_out and m > 8 and (res is None or ldr % 4 == 0)
    cslot = self._out_slot(c, n, ldc, c_off) if track else None
    h = wh is not None
    args = _lib.PointwiseArgs(
        A=_ptr(a, a_off), lda=lda, Wp=_ptr(wp), bias=_ptr(bp),
        R=_ptr(res, res_off) if res is not None else None, ldr=ldr,
        C=_ptr(c, c_off), ldc=ldc, M=m, N=n, K=kpad, relu=int(relu), sub=sub,
        Ho=ho, Wo=wo, Hi=hi, Wi=wi, Ws=_ptr(ws), Wh=_ptr(wh) if h else None,
        a_amax=self._slot_ptr(ab[0]) if h else None,
        a_amax2=self._slot_ptr(ab[1]) if h else None,
        a_gain=ab[2] if h else 0.0, a_bias=ab[3] if h else 0.0,
        a_presplit=int(presplit), c_amax=self._slot_ptr(cslot))
    if (name in W.TRAINABLE_LAYERS and name not in W.LOGITS_LAYERS) or \
        name in W.POINTWISE_CHAIN_LAYERS or name in net._aspp_pw:
      assert a_off == 0 and sub == 1 and res is None, name
      self.layer_operands[name] = (a, lda, m, k, n, args, ab if h else None)
    # fp32 activations in and out, weights once (4 B each: what the layer IS; the
    # split kernel streams 6 B per weight), residual once
    nbytes = 4 * (m * k + k * n + m * n + (m * n if res is not None else 0))
    net.op_io[name] = (4 * m * k, nbytes - 4 * m * k, id(a))
    if group is not None:
      group.append((name, args, 2 * m * n * k, nbytes))
      return
    net._launch(name, self.gemm, (args, 1), 'gemm', 2 * m * n * k, nbytes)
    # the launch passes `args` itself: mean() may still attach the image-pooling block sums
    # to the launch that writes the encoder output
    self._last_pw = (c, args, h and res is None and c_off == 0 and n % 4 == 0)

  def flush(self, group, heads=False):
    """Launches the collected problems as one grouped GEMM -- one per kind: problems whose A
    is already fp16 pairs run on another kernel instantiation than the ones that split
    their fp32 A themselves. heads: the dense logits heads, through epos_heads_gemm_f32 (the
    A-stationary kernel; same bits as the grouped GEMM)."""
    for kind in sorted({g[1].a_presplit for g in group}):
      part = [g for g in group if g[1].a_presplit == kind]
      arr = (_lib.PointwiseArgs * len(part))(*[g[1] for g in part])
      fn = self.heads if heads and not kind else self.gemm
      if fn is self.heads:
        self.net.heads_group = (arr, len(part))    # what epos_heads_gemm_plan is asked about
      self.net._launch('+'.join(g[0] for g in part), fn, (arr, len(part)), 'gemm',
                       sum(g[2] for g in part), sum(g[3] for g in part))
    del group[:]

  def depthwise(self, name, x, y, gain, bias0, flops, nbytes, **fields):
    """One depthwise 3x3 launch; `gain`, `bias0`: |y| <= gain * max|x| + bias0."""
    xb = self._bounds.get(id(x))
    if xb is not None:
      self._set_bound(y, xb[0], xb[1], gain * (xb[2] if xb[2] else 1.0), gain * xb[3] + bias0)
    args = _lib.DepthwiseArgs(**fields)
    yb = self._bounds.get(id(y))
    if yb is not None and self.use_presplit:
      # fp16-pair output, pending the consumer's decision (pointwise): scale from the
      # bound of |Y| = gain * max|X| + max|bias| (the same numbers the GEMM gets)
      args.y_h2 = 1
      args.x_amax, args.x_amax2 = self._slot_ptr(yb[0]), self._slot_ptr(yb[1])
      args.gain, args.bias0 = yb[2], yb[3]
      self._dw_h2[id(y)] = args
    self.net._launch(name, self.dw, (args,), 'dw', flops, nbytes)

  def dense_conv(self, name, x, y, hi, wi, cin, ho, wo, kk, stride, rate, pad, preprocess,
                 conv):
    """A kk x kk conv (+BN+ReLU) into y: an implicit GEMM inside the LDS-DMA kernel for a 3x3
    with Cin % 32 == 0 on an activation, else im2col (epos_im2col3x3_f32, or epos_im2col_f32
    for other kernel sizes) + the GEMM."""
    net, B = self.net, self.net.B
    cout = y.shape[3]
    k = kk * kk * cin
    if kk == 3 and cin % 32 == 0 and preprocess == _lib.PREPROCESS_NONE:
      # implicit GEMM: the LDS-DMA kernel gathers the shifted input pixels itself
      xb = self._bounds.get(id(x))
      wp, bp, ws, wh, _ = self._weights(name, conv, xb is not None and xb[1] is None and
                                        xb[2] == 0.0)     # a plain slot
      yslot = self._out_slot(y, cout, cout)
      args = _lib.Conv3x3Args(X=_ptr(x), ldx=cin, Wp=_ptr(wp), bias=_ptr(bp), Y=_ptr(y),
                              ldy=cout, B=B, H=hi, W=wi, Cin=cin, Cout=cout, stride=stride,
                              rate=rate, relu=1, Ws=_ptr(ws),
                              Wh=_ptr(wh) if wh is not None else None,
                              x_amax=self._slot_ptr(xb[0]) if wh is not None else None,
                              y_amax=self._slot_ptr(yslot))
      net._launch(name, self.conv3x3, (args,), 'gemm', 2 * B * ho * wo * cout * k,
                  4 * (B * hi * wi * cin + k * cout + B * ho * wo * cout))
      net.op_io[name] = (4 * B * hi * wi * cin, 4 * (k * cout + B * ho * wo * cout), id(x))
      return
    ldcol = -(-k // 4) * 4
    m = B * ho * wo
    col = net._empty(m, ldcol)
    net._col_ids.add(id(col))
    geom = dict(X=_ptr(x), ldx=cin, col=_ptr(col), ldcol=ldcol, B=B, Hi=hi, Wi=wi, Ho=ho, Wo=wo,
                C=cin, stride=stride, rate=rate, pad=pad, preprocess=preprocess)
    if kk == 3:
      args, fn, words = _lib.Im2colArgs(**geom), self.im2col3x3, m * ldcol
    else:
      args = _lib.Im2colKArgs(k=kk, mean_rgb=(ctypes.c_float * 3)(*W.MEAN_RGB), **geom)
      fn, words = self.im2col_k, wo * ldcol // 4 * min(B * ho, 65535)
    if self._first_im2col is None:
      self._first_im2col = (name + '/im2col', args, words)
    net._launch(name + '/im2col', fn, (args,), 'im2col')
    # no bound on the col matrix (float inputs outside [0, 255] are legal): fp32 GEMM
    self.pointwise(name, col, 0, ldcol, m, k, conv, y, 0, cout, relu=True)
    # fusion-group bytes: the input is read once, the column matrix does not exist
    net.op_io[name] = (x.element_size() * B * hi * wi * cin, net.op_io[name][1], id(x))

  def mean(self, name, x, pooled, hw, c):
    """Global mean of x [B, hw, c] into pooled. Round 4: when x is written by ONE fp16-pair
    GEMM launch without residual (Xception: exit_flow/block2 separable_conv3), that launch's
    epilogue also writes the column sums of every block of 32 rows and a small kernel
    finishes the mean from 150 x 2048 floats instead of re-reading the 39 MB tensor
    (EPOS_POOL_FOLD=0: the stand-alone reduction, as for ResNet, whose last launch carries a
    residual, and for batches whose images are not a whole number of 32-row blocks).
    Returns whether the mean was folded."""
    net, B = self.net, self.net.B
    lp = self._last_pw
    fold = (not net.dry_run and os.environ.get('EPOS_POOL_FOLD', '1') == '1' and
            lp is not None and lp[0] is x and lp[2] and (hw % 32 == 0 or B == 1))
    if fold:
      blocks = (hw + 31) // 32
      part = net._empty(B * blocks, c)
      lp[1].col_sums = _ptr(part)
      lp[1].col_ld = c
      net._launch(name, self.avg_pool_partial, (_ptr(part), c, _ptr(pooled), B, blocks, c, hw))
    else:
      net._launch(name, self.avg_pool, (_ptr(x), c, _ptr(pooled), B, hw, c))
    return bool(fold)

  def resize(self, name, x, ldx, y, ldy, hi, wi, ho, wo, c):
    self.net._launch(name, self.resize_fn,
                     (_ptr(x), ldx, _ptr(y), ldy, self.net.B, hi, wi, ho, wo, c))

  # ------------------------------------------------------- object heads ---
  def obj_head(self, name, args):
    """The stand-alone launch of the object head's problem (sparse-head mode)."""
    return self.net._call(name, self.gemm1, (args,))

  def sparse_weights(self, w_kn, bias):
    wp, bp, ws, wh, _ = self._weights(None, (w_kn, np.ones(w_kn.shape[1], np.float32), bias),
                                      True)
    return wp, bp, ws, wh

  def sparse_problem(self, pack, x, x_off, c, c_off, ldc, m, n):
    wp, bp, ws, wh = pack
    xb = self._bounds.get(id(x))
    if xb is None:
      wh = None
    h = wh is not None
    return _lib.PointwiseArgs(
        A=_ptr(x, x_off), lda=256, Wp=_ptr(wp), bias=_ptr(bp), R=None, ldr=0,
        C=_ptr(c, c_off), ldc=ldc, M=m, N=n, K=256, relu=0, sub=1, Ws=_ptr(ws),
        Wh=_ptr(wh) if h else None,
        a_amax=self._slot_ptr(xb[0]) if h else None,
        a_amax2=self._slot_ptr(xb[1]) if h else None,
        a_gain=xb[2] if h else 0.0, a_bias=xb[3] if h else 0.0)

  def sparse_launch(self, probs, stream):
    arr = (_lib.PointwiseArgs * len(probs))(*probs)
    _lib.check(self.gemm(arr, len(probs), stream), 'sparse heads')

  # ------------------------------------------------------ weight update ---
  def pack_problem(self, pack, w, bias, col0, n):
    """The device packer's problem that rewrites `pack` = (wp, bp, ws, wh) from the column
    window [col0, col0 + n) of w f32 [256, ldw] and bias f32 [ldw] (device tensors)."""
    wp, bp, ws, wh = pack
    return _lib.WeightPackArgs(W=_ptr(w), ldw=w.shape[-1], col0=col0, bias=_ptr(bias),
                               plain=_ptr(wp), split=_ptr(ws),
                               h2=_ptr(wh) if wh is not None else None, bias_pad=_ptr(bp),
                               K=w.shape[-2], N=n)

  def pack_launch(self, probs, status, stream, what='set_weights'):
    """One grouped epos_pack_weights_device_f32 call: all of probs or none of them."""
    arr = (_lib.WeightPackArgs * len(probs))(*probs)
    _lib.check(self.pack_device(arr, len(probs), _ptr(status), stream), what)

  def slot_words(self, i):
    """The words of absmax slot i as a view of the table (None for None)."""
    if i is None:
      return None
    return self._amax_table[i * _lib.AMAX_WORDS:(i + 1) * _lib.AMAX_WORDS]

  def finish(self):
    """The slot table is zeroed by the plan's first launch. Round 4: that is the im2col of the
    first stem conv itself (EposIm2colArgs.amax_clear) when it directly follows -- one launch
    less per image (EPOS_AMAX_CLEAR_FOLD=0 keeps the separate kernel)."""
    net, fi = self.net, self._first_im2col
    words = self._n_slots * _lib.AMAX_WORDS
    if (not net.dry_run and fi is not None and len(net.ops) > 1 and
        net.ops[0][0] == 'amax_clear' and net.ops[1][0] == fi[0] and words <= fi[2] and
        os.environ.get('EPOS_AMAX_CLEAR_FOLD', '1') == '1'):
      fi[1].amax_clear = _ptr(self._amax_table)
      fi[1].amax_words = words
      del net.ops[0]
      net._n_trunk_ops -= 1


class Bf16Mode(object):
  """bf16 activations, rows padded to 64 elements (128-byte lines), and bf16 weights (BN
  folded in fp32, then rounded to nearest even) on the bf16 kernels."""

  dtype, line = torch.bfloat16, 64
  use_h2 = False             # bf16 has fp32's exponent range: no slot / fp16-pair machinery
  _n_slots = 0

  def __init__(self, net):
    self.net = net
    fn = net._fn
    self.gemm = fn('epos_pointwise_conv_bf16')
    self.gemm_f32 = fn('epos_pointwise_conv_grouped_f32')
    self.dw = fn('epos_depthwise3x3_bf16')
    self.im2col = fn('epos_im2col_bf16')
    self.avg_pool = fn('epos_global_avg_pool_bf16')
    self.resize_fn = fn('epos_resize_bilinear_bf16')
    self.subsample = fn('epos_subsample_bf16')
    self.add_relu = fn('epos_add_relu_bf16')
    self.maxpool = fn('epos_maxpool3x3_s2_bf16')
    self.pack = fn('epos_pack_pointwise_weights_bf16')
    self.pack_plain = fn('epos_pack_pointwise_weights')
    self.pack_split = fn('epos_pack_pointwise_weights_split')
    self.h2_layers, self.h2_refused, self.presplit_layers = [], [], []
    # every im2col of the plan writes one shared scratch matrix, allocated by finish() (the
    # launch arguments that point into it are patched then)
    self._col_users, self._col_elems = [], 0

  def _weights(self, conv):
    """(wp, bp, kpad): folded weights in epos_pack_pointwise_weights_bf16's layout, K
    zero-padded to a multiple of 8, and the fp32 bias."""
    w_kn, scale, bias = conv
    k, n = w_kn.shape
    kpad = -(-k // 8) * 8
    net = self.net
    if net.dry_run:
      return net._empty(1), net._empty(1), kpad
    return (net._dev(_pack(self.pack, _fold(w_kn, scale, 8), np.uint16)),
            net._dev(_bias(bias, n, 4)), kpad)

  # no absmax slots in bf16 mode
  def same_bound(self, dst, src):
    pass

  def concat_bound(self, cat, left):
    pass

  def track_absmax(self, name, y, ld, rows, n):
    pass

  def join_absmax(self, name, x, ld, rows, n, into):
    pass

  def begin(self):
    pass

  # --------------------------------------------------------------- ops ---
  def pointwise(self, name, a, a_off, lda, m, k, conv, c, c_off, ldc, relu, res=None, res_off=0,
                ldr=0, sub=1, ho=0, wo=0, hi=0, wi=0, group=None, track_out=True):
    """One 1x1 conv on the bf16 GEMM (epos_pointwise_conv_bf16): A is bf16 (a=None: the shared
    im2col scratch, patched in by finish()); C is bf16, or fp32 for the logits. An fp32 A
    (the image-pooling 1x1) runs on the fp32 split-operand GEMM. Returns the launch
    arguments."""
    net = self.net
    if a is not None and a.dtype == torch.float32:
      return self._pointwise_f32(name, a, lda, m, k, conv, c, ldc, relu)
    wp, bp, kpad = self._weights(conv)
    n = conv[0].shape[1]
    # a K padded to 8 reads columns k .. kpad of A: only im2col matrices (zero-filled there)
    assert kpad == k or (a is None and lda >= kpad), (name, k, kpad, lda)
    args = _lib.PointwiseBf16Args(
        A=_ptr(a, a_off) if a is not None else None, lda=lda, Wp=_ptr(wp), bias=_ptr(bp),
        R=_ptr(res, res_off) if res is not None else None, ldr=ldr,
        C=_ptr(c, c_off), ldc=ldc, M=m, N=n, K=kpad, relu=int(relu), sub=sub,
        Ho=ho, Wo=wo, Hi=hi, Wi=wi, c_f32=int(c.dtype == torch.float32), c_stream=0)
    # bf16 activations and weights (2 B), the output in its own dtype, residual once
    nbytes = (2 * (m * k + k * n) + c.element_size() * m * n +
              (2 * m * n if res is not None else 0))
    net.op_io[name] = (2 * m * k, nbytes - 2 * m * k, id(a))
    if group is not None:
      group.append((name, args, 2 * m * n * k, nbytes))
      return args
    net._launch(name, self.gemm, (args, 1), 'gemm', 2 * m * n * k, nbytes)
    return args

  def _pointwise_f32(self, name, a, lda, m, k, conv, c, ldc, relu):
    net = self.net
    w_kn, scale, bias = conv
    n = w_kn.shape[1]
    kpad = -(-k // 4) * 4
    assert kpad == k, (name, k)
    if net.dry_run:
      wp, bp, ws = net._empty(1), net._empty(1), net._empty(1)
    else:
      w = _fold(w_kn, scale, 4)
      wp, bp = net._dev(_pack(self.pack_plain, w, np.float32)), net._dev(_bias(bias, n, 128))
      ws = net._dev(_pack(self.pack_split, w, np.uint8))
    args = _lib.PointwiseArgs(A=_ptr(a), lda=lda, Wp=_ptr(wp), bias=_ptr(bp), C=_ptr(c),
                              ldc=ldc, M=m, N=n, K=kpad, relu=int(relu), sub=1, Ws=_ptr(ws))
    nbytes = 4 * (m * k + k * n + m * n)
    net.op_io[name] = (4 * m * k, nbytes - 4 * m * k, id(a))
    net._launch(name, self.gemm_f32, (args, 1), 'gemm', 2 * m * n * k, nbytes)
    return args

  def flush(self, group, heads=False):
    """Launches the collected problems as one grouped GEMM (heads: no kernel of its own in
    this mode)."""
    if group:
      arr = (_lib.PointwiseBf16Args * len(group))(*[g[1] for g in group])
      self.net._launch('+'.join(g[0] for g in group), self.gemm, (arr, len(group)), 'gemm',
                       sum(g[2] for g in group), sum(g[3] for g in group))
    del group[:]

  def depthwise(self, name, x, y, gain, bias0, flops, nbytes, **fields):
    self.net._launch(name, self.dw, (_lib.DepthwiseBf16Args(**fields),), 'dw', flops, nbytes)

  def dense_conv(self, name, x, y, hi, wi, cin, ho, wo, kk, stride, rate, pad, preprocess,
                 conv):
    """A kk x kk conv (+BN+ReLU) into y = epos_im2col_bf16 into the plan's shared column
    scratch + the bf16 GEMM. x is the fp32 image (preprocess = its preprocessing) or a bf16
    activation."""
    net, B = self.net, self.net.B
    k = kk * kk * cin
    ldcol = -(-k // 8) * 8
    m = B * ho * wo
    self._col_elems = max(self._col_elems, m * ldcol)
    args = _lib.Im2colBf16Args(
        X=_ptr(x), ldx=cin, x_bf16=int(x.dtype == torch.bfloat16), col=None, ldcol=ldcol,
        B=B, Hi=hi, Wi=wi, Ho=ho, Wo=wo, C=cin, k=kk, stride=stride, rate=rate, pad=pad,
        preprocess=preprocess, mean_rgb=(ctypes.c_float * 3)(*W.MEAN_RGB))
    self._col_users.append((args, 'col'))
    net._launch(name + '/im2col', self.im2col, (args,), 'im2col')
    gargs = self.pointwise(name, None, 0, ldcol, m, k, conv, y, 0, y.shape[3], relu=True)
    self._col_users.append((gargs, 'A'))
    # fusion-group bytes: the input is read once, the column matrix does not exist
    net.op_io[name] = (x.element_size() * B * hi * wi * cin, net.op_io[name][1], id(x))

  def mean(self, name, x, pooled, hw, c):
    self.net._launch(name, self.avg_pool, (_ptr(x), c, _ptr(pooled), self.net.B, hw, c))
    return False

  def resize(self, name, x, ldx, y, ldy, hi, wi, ho, wo, c):
    """x is bf16, or fp32 (the pooled branch broadcast into the bf16 concat)."""
    self.net._launch(name, self.resize_fn, (_ptr(x), ldx, int(x.dtype == torch.float32),
                                            _ptr(y), ldy, self.net.B, hi, wi, ho, wo, c))

  # ------------------------------------------------------- object heads ---
  def obj_head(self, name, args):
    return self.net._call(name, self.gemm, (args, 1))

  def sparse_weights(self, w_kn, bias):
    return self._weights((w_kn, np.ones(w_kn.shape[1], np.float32), bias))[:2]

  def sparse_problem(self, pack, x, x_off, c, c_off, ldc, m, n):
    wp, bp = pack
    return _lib.PointwiseBf16Args(
        A=_ptr(x, x_off), lda=256, Wp=_ptr(wp), bias=_ptr(bp), R=None, ldr=0,
        C=_ptr(c, c_off), ldc=ldc, M=m, N=n, K=256, relu=0, sub=1, c_f32=1)

  def sparse_launch(self, probs, stream):
    arr = (_lib.PointwiseBf16Args * len(probs))(*probs)
    _lib.check(self.gemm(arr, len(probs), stream), 'sparse heads')

  def finish(self):
    """The shared im2col scratch, sized for the largest column matrix of the plan."""
    if self._col_users:
      net = self.net
      col = net._empty(self._col_elems, dtype=torch.bfloat16)
      net._col_ids.add(id(col))
      for args, field in self._col_users:
        setattr(args, field, _ptr(col))
