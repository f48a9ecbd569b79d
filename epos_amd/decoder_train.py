"""Training decoder/decoder_conv1_pointwise, the layer below the logits, on the device
(csrc/pointwise_wgrad.hip; include/epos_hip.h, "Pointwise weight gradient"; DESIGN.md, "Losses",
"Decoder layer gradients"): the first step of backpropagation below the logits layers.

  pointwise_weight_grads  epos_pointwise_wgrad_f32 + epos_pointwise_wgrad_close_f32: dW, dgamma
                          and dbeta of a 1x1 conv layer with a frozen batch norm (or dW and db
                          of one with biases) from its input A -- fp32 or the fp16 pairs the
                          depthwise kernel wrote -- and the gradient G at its pre-activation.

The nine variables' gradients from a running net, the optimiser and the training step are
epos_amd/trainer.py; the in-place weight update is EposNet.set_weights.

The batch-norm statistics are frozen (the reference's fine_tune_batch_norm=False): moving_mean
and moving_variance are inputs. Not built: the input gradient of this layer, G W^T, and with it
everything from decoder_conv1_depthwise down; batch-norm statistics, bf16 mode, multi-scale nets
and more than one device. Pinned to tests/helpers/pointwise_wgrad_ref.py and, through it, to
torch's fp64 autograd; parity with TensorFlow's gradients is unpinned. There is no CPU fallback.
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
