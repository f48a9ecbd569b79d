"""Training decoder/decoder_conv1_pointwise, the layer below the logits, on the device
(csrc/pointwise_wgrad.hip; include/epos_hip.h, "Pointwise weight gradient"; DESIGN.md, "Losses",
"Decoder layer gradients"): the first step of backpropagation below the logits layers.

  pointwise_weight_grads  epos_pointwise_wgrad_f32 + epos_pointwise_wgrad_close_f32: dW, dgamma
                          and dbeta of a 1x1 conv layer with a frozen batch norm (or dW and db
                          of one with biases) from its input A -- fp32 or the fp16 pairs the
                          depthwise kernel wrote -- and the gradient G at its pre-activation.

  pointwise_input_grad    epos_pointwise_dgrad_f32: D = mask (.) (G Wf^T), the gradient that
                          crosses the layer, at the pre-activation of decoder_conv1_depthwise
                          (csrc/pointwise_dgrad.hip; "Pointwise input gradient").
  depthwise_weight_grads  epos_depthwise_wgrad_f32 + epos_pointwise_wgrad_close_f32 with K = 9:
                          dw, dgamma and dbeta of a 3x3 depthwise layer with a frozen batch norm
                          (csrc/depthwise_grad.hip; "Depthwise gradients").
  depthwise_input_grad    epos_depthwise_dgrad_f32: the gradient that crosses the depthwise layer,
                          at the pre-activation of decoder_conv0_pointwise.
  resize_input_grad       epos_resize_bilinear_dgrad_f32: the gradient that crosses the decoder's
                          align-corners bilinear resize, at the pre-activation of
                          concat_projection (csrc/resize_grad.hip; "Resize input gradient").
  pool_broadcast_grad     epos_pool_broadcast_dgrad_f32: the adjoint of ASPP's image-pooling
                          broadcast, a per-image column sum in fp64 (csrc/aspp_grad.hip; "ASPP
                          gradients").
  aspp_join_grad          epos_aspp_join_dgrad_f32: the gradient at the encoder output, which
                          feeds ASPP's five branches -- the plain terms, the mirrored taps of the
                          depthwise terms and the per-image term in one fp64 sum per element, one
                          pass over the output.

The nine variables' gradients from a running net, the optimiser and the training step are
epos_amd/trainer.py, and so are the chain of the first five wrappers (trainer.decoder_conv1_grads),
the chain through the whole decoder (trainer.decoder_grads) and the one through ASPP
(trainer.aspp_grads); the in-place weight update is EposNet.set_weights.

The batch-norm statistics are frozen (the reference's fine_tune_batch_norm=False): moving_mean
and moving_variance are inputs. Built: the gradients above ("Losses", "Backward
through decoder_conv1", "Backward through the decoder" and "Backward through ASPP");
pointwise_input_grad at any K (the entry takes K <= 1024: a wider K goes to it in k_blocks).
Not built: the in-place update of
any depthwise layer's weights -- its
folded weights set the bound |Y| <= gain max|X| + bias0 that the plan bakes by value into the
layer's EposDepthwiseArgs and into its consumer's a_gain / a_bias, and captured graphs have
copied those values, so an update needs a design for that bound; training the four layers
below decoder_conv1 and ASPP's (weights.POINTWISE_CHAIN_LAYERS, DEPTHWISE_CHAIN_LAYERS,
weights.aspp_layers: their gradients are computed, the tables of trainable layers do not hold
them); the backbone, everything below the encoder output's pre-activation; batch-norm
statistics, bf16 mode, multi-scale nets and more than one device. Pinned to
tests/helpers/pointwise_wgrad_ref.py, decoder_backward_ref.py, resize_grad_ref.py and
aspp_grad_ref.py and, through them, to torch's fp64 autograd; parity with TensorFlow's gradients
is unpinned, and the formulas for the frozen batch norm are this build's own. There is no CPU fallback.
"""
import ctypes

from epos_amd import _call as C
from epos_amd import _lib
from epos_amd._lib import EposError
from epos_amd import weights as W

LAYER = W.DECODER_CONV1_POINTWISE
LAYER_VARIABLES = W.trainable_variables((LAYER,))
LAYER_CONSTANTS = (LAYER + '/BatchNorm/moving_mean', LAYER + '/BatchNorm/moving_variance')
VARIABLES = W.trainable_variables()
BN_EPS = W.TRAINABLE_LAYERS[LAYER]


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
  C.need_device(g, 'the weight gradients need a HIP device (there is no CPU fallback)')
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
  a2, lda = C.rows(a, K)
  g2, ldg = C.rows(g, N)
  M = int(a2.shape[0])
  if g2.shape[0] != M or M < 1:
    raise ValueError('a holds %d rows, g %d' % (M, g2.shape[0]))
  if a_h2 is not None and a2.data_ptr() != a.data_ptr():
    raise ValueError('a pre-split a must have rows a constant stride apart')
  names = W.CONV_VARIABLES[bn is not None]
  consts = [None, None, None]
  if bn is not None:
    if len(bn) != 3:
      raise ValueError('bn = (gamma, moving_mean, moving_variance)')
    for t, what in zip(bn, ('gamma', 'moving_mean', 'moving_variance')):
      C.dense(t, dev, torch.float32, what, shape=(N,), name='float32')
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
    result[name] = C.out((out or {}).get(name), dev, torch.float32,
                          W.variable_shapes(name, K, N)[0], 'out[%r]' % name, flat=True)
  ws = C.workspace(workspace, dev, 8 * workspace_words(M, K, N), torch.int64)
  S, gsum, slabs = ws[:K * N], ws[K * N:K * N + N], ws[K * N + N:]
  args = _lib.PointwiseWgradArgs(
      A=C.ptr(a2), lda=lda, G=C.ptr(g2), ldg=ldg, M=M, K=K, N=N,
      a_presplit=int(a_h2 is not None), a_amax=C.ptr(slots[0]), a_amax2=C.ptr(slots[1]),
      a_gain=gain, a_bias=bias, S=C.ptr(S), g=C.ptr(gsum),
      workspace=C.ptr(slabs) if slabs.numel() else None)
  with C.launch(dev) as q:
    q.keep(a2, g2, ws)
    _lib.check(lib.epos_pointwise_wgrad_f32(ctypes.byref(args), q.handle),
               'epos_pointwise_wgrad_f32')
    _lib.check(lib.epos_pointwise_wgrad_close_f32(
        C.ptr(S), C.ptr(gsum), C.ptr(weights), K, N, C.ptr(consts[0]), C.ptr(consts[1]),
        C.ptr(consts[2]), float(eps), C.ptr(result['weights']),
        C.ptr(result['BatchNorm/gamma']) if bn is not None else None,
        C.ptr(result[names[-1]]), q.handle), 'epos_pointwise_wgrad_close_f32')
  return result


def _same_device_f32(dev, first, *named):
  import torch
  for t, what in named:
    if t.device != dev:
      raise EposError('%s is on %s, %s on %s' % (what, t.device, first, dev))
    if t.dtype != torch.float32:
      raise TypeError('%s must be torch.float32, got %s' % (what, t.dtype))


def _out_rows(out, dev, n, width, what):
  """(out, its [n, width] view, row stride): a new tensor, or the caller's, whose rows must lie
  a constant stride apart so that the kernel writes into it and not into a copy."""
  import torch
  out = C.out(out, dev, torch.float32, (n, width), what, rows=True)
  out2, ld = C.rows(out, width)
  if out2.data_ptr() != out.data_ptr() or out2.shape[0] != n:
    raise ValueError('%s: %d rows must lie a constant stride apart' % (what, n))
  return out, out2, ld


def pointwise_input_grad(g, weights, bn=None, eps=BN_EPS, relu_of=None, relu_of_h2=False,
                         out=None, workspace=None):
  """epos_pointwise_dgrad_f32: the gradient that crosses the layer y = relu(scale (.) (A W) +
  bias), D = G Wf^T with Wf = the folded weights the forward multiplied by. g: f32 [..., N], the
  gradient at the layer's pre-activation, rows a constant stride apart. weights: f32 [1,1,K,N]
  or [K,N] on the device, contiguous. bn = (gamma, moving_variance), f32 [N] on the device,
  with eps; None: a conv with biases (Wf = W). relu_of: the layer's input A, f32 [..., K], rows
  a constant stride apart -- or, with relu_of_h2, the fp16 pairs the depthwise kernel wrote into
  such a tensor (EposNet.pointwise_operand's 'a'): the result is +0.0 wherever it is <= 0, the
  gradient at the pre-activation of the layer that produced A. Returns D f32 [rows, K], or `out`
  (f32 [..., K], rows a constant stride apart; its padding columns are kept). `workspace`: a
  float64 tensor of at least epos_pointwise_dgrad_workspace_bytes(min(K, 1024), N) / 8 values.
  The entry takes K <= 1024: a wider K (ASPP's 1280 and 2048) goes to it in k_blocks(K), one
  call per block on weights[k0:k1], out[:, k0:k1] and relu_of[:, k0:k1], the same bytes as an
  uncut call would give. N > 1024 stays refused. Every element is written. Enqueues on the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  C.need_device(g, 'the input gradient needs a HIP device (there is no CPU fallback)')
  dev = g.device
  _same_device_f32(dev, 'g', (g, 'g'), (weights, 'weights'))
  N = int(g.shape[-1])
  if weights.dim() < 2 or weights.shape[-1] != N or weights.numel() != weights.shape[-2] * N:
    raise ValueError('weights must be [1, 1, K, %d], got %s' % (N, tuple(weights.shape)))
  if not weights.is_contiguous():
    raise ValueError('weights must be contiguous')
  K = int(weights.shape[-2])
  g2, ldg = C.rows(g, N)
  M = int(g2.shape[0])
  if M < 1:
    raise ValueError('g holds no rows')
  consts = [None, None]
  if bn is not None:
    if len(bn) != 2:
      raise ValueError('bn = (gamma, moving_variance)')
    for t, what in zip(bn, ('gamma', 'moving_variance')):
      C.dense(t, dev, torch.float32, what, shape=(N,), name='float32')
    consts = list(bn)
  m2, ldm = None, K
  if relu_of is not None:
    _same_device_f32(dev, 'g', (relu_of, 'relu_of'))
    if relu_of.shape[-1] != K:
      raise ValueError('relu_of must be [..., %d], got %s' % (K, tuple(relu_of.shape)))
    m2, ldm = C.rows(relu_of, K)
    if m2.shape[0] != M:
      raise ValueError('relu_of holds %d rows, g %d' % (m2.shape[0], M))
    if relu_of_h2 and m2.data_ptr() != relu_of.data_ptr():
      raise ValueError('a pre-split relu_of must have rows a constant stride apart')
  out, out2, ldd = _out_rows(out, dev, M, K, 'out')
  blocks = k_blocks(K)
  nbytes = lib.epos_pointwise_dgrad_workspace_bytes(blocks[0][1], N)
  _lib.check(nbytes, 'epos_pointwise_dgrad_workspace_bytes')
  ws = C.workspace(workspace, dev, nbytes, torch.float64)
  w2 = weights.view(K, N)
  with C.launch(dev) as q:
    q.keep(g2, m2, ws)
    for k0, k1 in blocks:
      args = _lib.PointwiseDgradArgs(
          G=C.ptr(g2), ldg=ldg, W=C.ptr(w2, k0 * N), gamma=C.ptr(consts[0]),
          moving_variance=C.ptr(consts[1]), eps=float(eps), mask=C.ptr(m2, k0), ldm=ldm,
          mask_h2=int(bool(relu_of_h2) and m2 is not None), M=M, K=k1 - k0, N=N,
          D=C.ptr(out2, k0), ldd=ldd, workspace=C.ptr(ws))
      _lib.check(lib.epos_pointwise_dgrad_f32(ctypes.byref(args), q.handle),
                 'epos_pointwise_dgrad_f32')
  return out


DGRAD_MAX_K = 1024     # epos_pointwise_dgrad_f32 refuses a wider K; its tests pin the refusal


def k_blocks(K, width=DGRAD_MAX_K):
  """[(k0, k1), ...]: the K columns of pointwise_input_grad's result cut into consecutive blocks
  of at most `width` (a multiple of 4, so that the quads of a pre-split mask stay whole), one
  call of the entry each. The kernel keeps one accumulator per (row, k) and its reduction runs
  over N, which is never cut: the cut changes no byte. K <= width is one block, the call it
  always was."""
  if K < 1 or width < 4 or width % 4:
    raise ValueError('k_blocks: K >= 1 and a width that is a multiple of 4, got %r, %r' % (
        K, width))
  return [(k0, min(k0 + width, K)) for k0 in range(0, K, width)]


def _nhwc(t, what):
  """(t as [B*H*W, C] rows, pixel stride, (B, H, W, C)) of an NHWC tensor whose pixels lie a
  constant stride apart (a slice of a wider buffer); anything else is made dense."""
  if t.dim() != 4:
    raise ValueError('%s must be [B, H, W, C], got %s' % (what, tuple(t.shape)))
  t2, ld = C.rows(t, int(t.shape[-1]))
  return t2, ld, tuple(int(v) for v in t.shape)


def depthwise_workspace_words(B, H, Wd, Cc):
  """int64 words depthwise_weight_grads needs: T and t in fp64 and the kernel's slabs."""
  nbytes = _lib.load().epos_depthwise_wgrad_workspace_bytes(B, H, Wd, Cc)
  _lib.check(nbytes, 'epos_depthwise_wgrad_workspace_bytes')
  return 10 * Cc + (nbytes + 7) // 8


def depthwise_weight_grads(x, d, depthwise_weights, bn, eps, rate=1, out=None, workspace=None):
  """epos_depthwise_wgrad_f32 + epos_pointwise_wgrad_close_f32 with K = 9: the weight and
  batch-norm gradients of a 3x3 depthwise layer (stride 1, 'SAME') with a frozen batch norm. x:
  the layer's input, f32 [B,H,W,C], pixels a constant stride apart (EposNet.depthwise_operand's
  'x'); d: f32 [B,H,W,C] or [B*H*W,C], the gradient at the layer's pre-activation, as
  pointwise_input_grad(relu_of=...) writes it. depthwise_weights: f32 [3,3,C,1] on the device,
  contiguous; bn = (gamma, moving_mean, moving_variance), f32 [C] on the device, with eps.
  Returns {'depthwise_weights': f32 [3,3,C,1], 'BatchNorm/gamma': f32 [C], 'BatchNorm/beta':
  f32 [C]}. `out` = such a dict of contiguous tensors to write into; `workspace` = an int64
  tensor of at least depthwise_workspace_words(B, H, W, C) values. Every element of every
  output is written. Enqueues on the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  C.need_device(d, 'the depthwise gradients need a HIP device (there is no CPU fallback)')
  dev = d.device
  _same_device_f32(dev, 'd', (x, 'x'), (d, 'd'), (depthwise_weights, 'depthwise_weights'))
  x2, ldx, (B, H, Wd, Cc) = _nhwc(x, 'x')
  d2, ldd = C.rows(d, Cc) if d.shape[-1] == Cc else (None, 0)
  if d2 is None or d2.shape[0] != B * H * Wd:
    raise ValueError('d must hold %d rows of %d values, got %s' % (
        B * H * Wd, Cc, tuple(d.shape)))
  if depthwise_weights.numel() != 9 * Cc or tuple(depthwise_weights.shape[:2]) != (3, 3) or \
      not depthwise_weights.is_contiguous():
    raise ValueError('depthwise_weights must be a contiguous [3, 3, %d, 1] tensor, got %s' % (
        Cc, tuple(depthwise_weights.shape)))
  if bn is None or len(bn) != 3:
    raise ValueError('bn = (gamma, moving_mean, moving_variance)')
  for t, what in zip(bn, ('gamma', 'moving_mean', 'moving_variance')):
    C.dense(t, dev, torch.float32, what, shape=(Cc,), name='float32')
  shapes = {'depthwise_weights': (3, 3, Cc, 1), 'BatchNorm/gamma': (Cc,),
            'BatchNorm/beta': (Cc,)}
  result = {name: C.out((out or {}).get(name), dev, torch.float32, shape, 'out[%r]' % name,
                        flat=True) for name, shape in shapes.items()}
  ws = C.workspace(workspace, dev, 8 * depthwise_workspace_words(B, H, Wd, Cc), torch.int64)
  T, tsum, slabs = ws[:9 * Cc], ws[9 * Cc:10 * Cc], ws[10 * Cc:]
  args = _lib.DepthwiseWgradArgs(
      X=C.ptr(x2), ldx=ldx, D=C.ptr(d2), ldd=ldd, B=B, H=H, W=Wd, C=Cc, stride=1,
      rate=int(rate), T=C.ptr(T), t=C.ptr(tsum),
      workspace=C.ptr(slabs) if slabs.numel() else None)
  with C.launch(dev) as q:
    q.keep(x2, d2, ws)
    _lib.check(lib.epos_depthwise_wgrad_f32(ctypes.byref(args), q.handle),
               'epos_depthwise_wgrad_f32')
    _lib.check(lib.epos_pointwise_wgrad_close_f32(
        C.ptr(T), C.ptr(tsum), C.ptr(depthwise_weights), 9, Cc, C.ptr(bn[0]), C.ptr(bn[1]),
        C.ptr(bn[2]), float(eps), C.ptr(result['depthwise_weights']),
        C.ptr(result['BatchNorm/gamma']), C.ptr(result['BatchNorm/beta']), q.handle),
        'epos_pointwise_wgrad_close_f32')
  return result


def depthwise_input_grad(d, w9c, rate=1, relu_of=None, out=None):
  """epos_depthwise_dgrad_f32: the gradient that crosses a 3x3 depthwise layer (stride 1,
  'SAME'). d: f32 [B,H,W,C], pixels a constant stride apart, the gradient at the layer's
  pre-activation; w9c: f32 [9,C] on the device, contiguous, the FOLDED weights the forward reads
  (EposNet.depthwise_operand's 'w9c'). relu_of: the layer's input x, f32 [B,H,W,C], pixels a
  constant stride apart: the result is +0.0 wherever it is <= 0, the gradient at the
  pre-activation of the layer that produced x. Returns dX f32 [B,H,W,C], or `out` (f32
  [B,H,W,C], pixels a constant stride apart; its padding columns are kept). Every element is
  written. Enqueues on the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  C.need_device(d, 'the depthwise input gradient needs a HIP device (there is no CPU fallback)')
  dev = d.device
  _same_device_f32(dev, 'd', (d, 'd'), (w9c, 'w9c'))
  d2, ldd, (B, H, Wd, Cc) = _nhwc(d, 'd')
  C.dense(w9c, dev, torch.float32, 'w9c', shape=(9, Cc), name='float32')
  y2, ldy = None, Cc
  if relu_of is not None:
    _same_device_f32(dev, 'd', (relu_of, 'relu_of'))
    if tuple(relu_of.shape) != (B, H, Wd, Cc):
      raise ValueError('relu_of must be %s, got %s' % ((B, H, Wd, Cc), tuple(relu_of.shape)))
    y2, ldy = C.rows(relu_of, Cc)
  if out is not None and tuple(out.shape) != (B, H, Wd, Cc):
    raise ValueError('out must be %s, got %s' % ((B, H, Wd, Cc), tuple(out.shape)))
  out, out2, ldx = _out_rows(out, dev, B * H * Wd, Cc, 'out')
  with C.launch(dev) as q:
    q.keep(d2, y2)
    _lib.check(lib.epos_depthwise_dgrad_f32(
        C.ptr(d2), ldd, C.ptr(w9c), C.ptr(y2), ldy, C.ptr(out2), ldx, B, H, Wd, Cc, int(rate),
        q.handle), 'epos_depthwise_dgrad_f32')
  return out.view(B, H, Wd, Cc) if out.dim() == 2 else out


def resize_input_grad(d, in_hw, relu_of=None, out=None):
  """epos_resize_bilinear_dgrad_f32: the gradient that crosses an align-corners bilinear resize
  from in_hw = (Hi, Wi) to d's size, the adjoint of the plan's resize with the forward's own fp32
  coordinates. d: f32 [B,Ho,Wo,C], pixels a constant stride apart (a channel slice of a wider
  buffer goes straight through), the gradient at the resize's output. relu_of: the resize's
  source, f32 [B,Hi,Wi,C], pixels a constant stride apart: the result is +0.0 wherever it is
  <= 0, the gradient at the pre-activation of the layer that produced the source. Returns dX
  f32 [B,Hi,Wi,C], or `out` (f32 [B,Hi,Wi,C], pixels a constant stride apart; its padding
  columns are kept). Every element is written. A source of one row or column under a larger
  output (the image-pooling broadcast) is refused. Enqueues on the current stream; does not
  synchronise."""
  import torch
  lib = _lib.load()
  C.need_device(d, 'the resize input gradient needs a HIP device (there is no CPU fallback)')
  dev = d.device
  _same_device_f32(dev, 'd', (d, 'd'))
  d2, ldd, (B, Ho, Wo, Cc) = _nhwc(d, 'd')
  Hi, Wi = (int(v) for v in in_hw)
  y2, ldy = None, Cc
  if relu_of is not None:
    _same_device_f32(dev, 'd', (relu_of, 'relu_of'))
    if tuple(relu_of.shape) != (B, Hi, Wi, Cc):
      raise ValueError('relu_of must be %s, got %s' % ((B, Hi, Wi, Cc), tuple(relu_of.shape)))
    y2, ldy = C.rows(relu_of, Cc)
  if out is not None and tuple(out.shape) != (B, Hi, Wi, Cc):
    raise ValueError('out must be %s, got %s' % ((B, Hi, Wi, Cc), tuple(out.shape)))
  if Hi < 1 or Wi < 1:
    raise ValueError('in_hw must be positive, got %s' % ((Hi, Wi),))
  out, out2, ldx = _out_rows(out, dev, B * Hi * Wi, Cc, 'out')
  with C.launch(dev) as q:
    q.keep(d2, y2)
    _lib.check(lib.epos_resize_bilinear_dgrad_f32(
        C.ptr(d2), ldd, C.ptr(y2), ldy, C.ptr(out2), ldx, B, Hi, Wi, Ho, Wo, Cc, q.handle),
        'epos_resize_bilinear_dgrad_f32')
  return out.view(B, Hi, Wi, Cc) if out.dim() == 2 else out


def pool_workspace_bytes(B, P, Cc):
  """Bytes of workspace pool_broadcast_grad needs: the ranges' slabs, 0 with one range."""
  nbytes = _lib.load().epos_pool_broadcast_dgrad_workspace_bytes(B, P, Cc)
  _lib.check(nbytes, 'epos_pool_broadcast_dgrad_workspace_bytes')
  return nbytes


def pool_broadcast_grad(d, out=None, workspace=None):
  """epos_pool_broadcast_dgrad_f32: the adjoint of broadcasting a [B,C] tensor over the pixels
  of each image (ASPP's image pooling), g[b,c] = the fp64 sum of d[b,:,c] rounded once. d: f32
  [B,H,W,C] or [B,P,C], pixels a constant stride apart (a column slice of a wider buffer goes
  straight through). Returns g f32 [B,C], or `out` (f32 [B,C], rows a constant stride apart;
  its padding columns are kept). `workspace`: a float64 tensor of at least
  pool_workspace_bytes(B, P, C) / 8 values. Every element is written. Enqueues on the current
  stream; does not synchronise."""
  import torch
  lib = _lib.load()
  C.need_device(d, 'the broadcast\'s adjoint needs a HIP device (there is no CPU fallback)')
  dev = d.device
  _same_device_f32(dev, 'd', (d, 'd'))
  if d.dim() not in (3, 4) or d.numel() < 1:
    raise ValueError('d must be [B, H, W, C] or [B, P, C], got %s' % (tuple(d.shape),))
  B, Cc = int(d.shape[0]), int(d.shape[-1])
  d2, ldd = C.rows(d, Cc)
  P = int(d2.shape[0]) // B
  if out is not None and tuple(out.shape) != (B, Cc):
    raise ValueError('out must be %s, got %s' % ((B, Cc), tuple(out.shape)))
  out, out2, ldg = _out_rows(out, dev, B, Cc, 'out')
  nbytes = lib.epos_pool_broadcast_dgrad_workspace_bytes(B, P, Cc)
  _lib.check(nbytes, 'epos_pool_broadcast_dgrad_workspace_bytes')
  ws = C.workspace(workspace, dev, nbytes, torch.float64) if nbytes else None
  with C.launch(dev) as q:
    q.keep(d2, ws)
    _lib.check(lib.epos_pool_broadcast_dgrad_f32(
        C.ptr(d2), ldd, C.ptr(out2), ldg, B, P, Cc, C.ptr(ws), q.handle),
        'epos_pool_broadcast_dgrad_f32')
  return out


def aspp_join_grad(depthwise=(), plain=(), pooled=None, relu_of=None, out=None,
                   partition='shipped'):
  """epos_aspp_join_dgrad_f32: the gradient at a tensor X [B,H,W,C] that feeds several branches
  (ASPP's encoder output), in one pass: per element one fp64 sum of the plain terms, the
  mirrored taps of the depthwise terms and the per-image term, in that order, rounded once.
  depthwise: up to four (D f32 [B,H,W,C], w9c f32 [9,C] contiguous, rate) -- D the gradient at
  a 3x3 depthwise branch's pre-activation, w9c its FOLDED weights, as depthwise_input_grad
  takes them; plain: up to two f32 [B,H,W,C] or [B*H*W,C], the gradients 1x1 branches sent
  down (pointwise_input_grad's results); pooled = (Pool f32 [B,C], div): the gradient at a mean
  over div pixels, which adds Pool[b,c] / div to every pixel of image b. relu_of: X itself, f32
  [B,H,W,C]: the result is +0.0 wherever it is <= 0. Every tensor may be a slice of a wider
  buffer with pixels a constant stride apart. Returns dX f32 [B,H,W,C], or `out`.
  partition: a key of _lib.ASPP_JOIN_PARTITIONS -- which workgroup computes an element, never
  its value. With one depthwise term alone the bytes are depthwise_input_grad's. Every element
  is written. Enqueues on the current stream; does not synchronise."""
  import torch
  lib = _lib.load()
  depthwise, plain = list(depthwise), list(plain)
  first = (depthwise[0][0] if depthwise else relu_of if relu_of is not None else
           out if out is not None else next((t for t in plain if t.dim() == 4), None))
  if first is None or first.dim() != 4:
    raise ValueError('aspp_join_grad: a [B, H, W, C] tensor among depthwise, relu_of, out or '
                     'plain must give the shape')
  C.need_device(first, 'the ASPP join needs a HIP device (there is no CPU fallback)')
  dev = first.device
  B, H, Wd, Cc = (int(v) for v in first.shape)
  if len(depthwise) > 4 or len(plain) > 2:
    raise ValueError('aspp_join_grad takes at most 4 depthwise and 2 plain terms, got %d and '
                     '%d' % (len(depthwise), len(plain)))
  if not depthwise and not plain and pooled is None:
    raise ValueError('aspp_join_grad: at least one term must be present')
  args = _lib.AsppJoinArgs(B=B, H=H, W=Wd, C=Cc, n_dw=len(depthwise), n_plain=len(plain),
                           partition=_lib.ASPP_JOIN_PARTITIONS[partition])
  kept = []
  for i, (d, w9c, rate) in enumerate(depthwise):
    _same_device_f32(dev, 'the first tensor', (d, 'depthwise[%d] D' % i),
                     (w9c, 'depthwise[%d] w9c' % i))
    if tuple(d.shape) != (B, H, Wd, Cc):
      raise ValueError('depthwise[%d] D must be %s, got %s' % (i, (B, H, Wd, Cc),
                                                               tuple(d.shape)))
    C.dense(w9c, dev, torch.float32, 'depthwise[%d] w9c' % i, shape=(9, Cc), name='float32')
    d2, ldd = C.rows(d, Cc)
    kept += [d2, w9c]
    args.dw[i] = _lib.AsppJoinDw(D=C.ptr(d2), ldd=ldd, w9c=C.ptr(w9c), rate=int(rate))
  for j, e in enumerate(plain):
    _same_device_f32(dev, 'the first tensor', (e, 'plain[%d]' % j))
    if e.shape[-1] != Cc or e.numel() != B * H * Wd * Cc:
      raise ValueError('plain[%d] must hold %d rows of %d values, got %s' % (
          j, B * H * Wd, Cc, tuple(e.shape)))
    e2, lde = C.rows(e, Cc)
    kept.append(e2)
    args.plain[j] = _lib.AsppJoinPlain(E=C.ptr(e2), lde=lde)
  if pooled is not None:
    pool, div = pooled
    _same_device_f32(dev, 'the first tensor', (pool, 'pooled'))
    if tuple(pool.shape) != (B, Cc):
      raise ValueError('pooled must be %s, got %s' % ((B, Cc), tuple(pool.shape)))
    p2, ldp = C.rows(pool, Cc)
    kept.append(p2)
    args.Pool, args.ldp, args.pool_div = C.ptr(p2), ldp, int(div)
  if relu_of is not None:
    _same_device_f32(dev, 'the first tensor', (relu_of, 'relu_of'))
    if tuple(relu_of.shape) != (B, H, Wd, Cc):
      raise ValueError('relu_of must be %s, got %s' % ((B, H, Wd, Cc), tuple(relu_of.shape)))
    y2, ldy = C.rows(relu_of, Cc)
    kept.append(y2)
    args.Y, args.ldy = C.ptr(y2), ldy
  if out is not None and tuple(out.shape) != (B, H, Wd, Cc):
    raise ValueError('out must be %s, got %s' % ((B, H, Wd, Cc), tuple(out.shape)))
  out, out2, ldx = _out_rows(out, dev, B * H * Wd, Cc, 'out')
  args.dX, args.ldx = C.ptr(out2), ldx
  with C.launch(dev) as q:
    q.keep(*kept)
    _lib.check(lib.epos_aspp_join_dgrad_f32(ctypes.byref(args), q.handle),
               'epos_aspp_join_dgrad_f32')
  return out.view(B, H, Wd, Cc) if out.dim() == 2 else out


DEPTHWISE_LAYER = W.DECODER_CONV1_DEPTHWISE
DEPTHWISE_VARIABLES = tuple(DEPTHWISE_LAYER + '/' + v for v in W.DEPTHWISE_VARIABLES)
DEPTHWISE_CONSTANTS = (DEPTHWISE_LAYER + '/BatchNorm/moving_mean',
                       DEPTHWISE_LAYER + '/BatchNorm/moving_variance')


def _depthwise_inputs(net, variables, layer=DEPTHWISE_LAYER):
  """(depthwise_weights, (gamma, moving_mean, moving_variance)) of a depthwise layer the backward
  pass crosses (decoder_conv1_depthwise by default) on the
  net's device: each from `variables` where given, otherwise the copy the net uploaded from its
  checkpoint once (EposNet.depthwise_constants, crossed_depthwise_constants). With tensors on
  the device, or none, given, nothing is copied from the host and nothing waited for."""
  kept = (net.depthwise_constants(layer) if layer in W.DEPTHWISE_BACKWARD_LAYERS else
          net.crossed_depthwise_constants(layer))
  return _given_or_kept(net, variables, layer, kept, ('depthwise_weights', 'BatchNorm/gamma'))


def _crossed_inputs(net, variables, layer):
  """(weights, (gamma, moving_mean, moving_variance)) of a 1x1 layer of
  weights.POINTWISE_CHAIN_LAYERS on the net's device, as _depthwise_inputs gives a depthwise
  layer's: from `variables` where given, otherwise the copy the net keeps
  (EposNet.pointwise_constants)."""
  return _given_or_kept(net, variables, layer, net.pointwise_constants(layer),
                        ('weights', 'BatchNorm/gamma'))


def _given_or_kept(net, variables, layer, kept, shorts):
  import torch
  got = list(kept)
  names = tuple(layer + '/' + v for v in shorts + ('BatchNorm/moving_mean',
                                                   'BatchNorm/moving_variance'))
  for i, n in enumerate(names):
    v = variables.get(n)
    if v is not None:
      got[i] = torch.as_tensor(v, dtype=torch.float32).to(net.dev).contiguous()
  return got[0], tuple(got[1:])


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
