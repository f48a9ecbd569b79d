"""The backward pass through the whole decoder from a running net (trainer.decoder_grads) on the
small net of tests/helpers/loss_device.py -- 96 x 128, heads 24 x 32, encoder 12 x 16, B = 2: the
operands the plan recorded against the net's own buffers, the chain against decoder_conv1_grads
and against its wrappers called by hand, every new gradient within its kernel's bound of the
restatements fed the device's own inputs (the depthwise input gradient and the resize adjoint bit
for bit), the masks, the chain without a synchronisation, with an fp32 A0 in a child process, and
against torch's fp64 autograd through a torch.nn restatement of the decoder."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import decoder_backward_ref as ref                     # noqa: E402
from tests.helpers import loss_cases, pointwise_wgrad_ref as wref         # noqa: E402
from tests.helpers import resize_grad_ref                                 # noqa: E402
from tests.helpers.loss_device import (NET_B, NET_F, NET_H, NET_O, NET_W,     # noqa: E402,F401
                                       gt_tensors, small_net)

pytestmark = pytest.mark.gpu

LOSS_WEIGHTS = (0.7, 1.3, 100.0)
EPS = 1e-5
CONV0_PW, CONV0_DW = 'decoder/decoder_conv0_pointwise', 'decoder/decoder_conv0_depthwise'
FEATURE, PROJ = 'decoder/feature_projection0', 'concat_projection'
BN3 = ('BatchNorm/gamma', 'BatchNorm/moving_mean', 'BatchNorm/moving_variance')
NEW = tuple(s + '/' + v for s in (CONV0_PW, FEATURE, PROJ)
            for v in ('weights', 'BatchNorm/gamma', 'BatchNorm/beta')) + tuple(
                CONV0_DW + '/' + v for v in ('depthwise_weights', 'BatchNorm/gamma',
                                             'BatchNorm/beta'))

# The largest |chain - autograd| / max |autograd| per gradient that
# test_the_chain_agrees_with_torch_fp64_autograd measured on the MI355X (profiles/r30/README.md),
# by the layer the gradient belongs to. The restatement runs in fp64 from the net's fp32
# aspp_concat and low-level tap and resizes at the exact positions; the chain reads fp32 (or
# fp16-pair) activations, fp32-folded weights and fp32 coordinates, and a ReLU whose input lies
# within that difference of zero is open on one side and shut on the other. The test allows
# MARGIN times the measured figure; a wrong sign gives 2 and a dropped factor of two 0.5, so
# every allowance must stay below LIMIT.
MEASURED = {
    'logits/pred_obj_conf': 1.37e-07, 'logits/pred_frag_conf': 1.24e-07,
    'logits/pred_frag_loc': 1.72e-07,
    'decoder/decoder_conv1_pointwise': 3.00e-07, 'decoder/decoder_conv1_depthwise': 3.21e-07,
    'decoder/decoder_conv0_pointwise': 3.29e-07, 'decoder/decoder_conv0_depthwise': 1.09e-06,
    'decoder/feature_projection0': 1.95e-07, 'concat_projection': 2.09e-07, 'd_proj': 1.01e-06,
}
# 8 x: the figures are maxima over a few thousand elements of one batch and one set of weights;
# torch's own interpolate backward adds in an order that changes from run to run
MARGIN, LIMIT = 8.0, 0.05


def variables_of(ckpt):
  from epos_amd import decoder_train as DT
  return {n: torch.from_numpy(np.ascontiguousarray(ckpt[n])).cuda() for n in DT.VARIABLES}


def same_bytes(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and \
      a.contiguous().view(torch.uint8).equal(b.contiguous().view(torch.uint8))


def dev(ckpt, name):
  return torch.from_numpy(np.ascontiguousarray(ckpt[name])).cuda()


def a_values(op):
  """fp64 [M,K]: the values the layer's A stands for, from the device's own bytes -- fp16 pairs
  at the plan's scale, or fp32."""
  raw = op['a'].cpu().numpy().reshape(op['m'], op['lda'])
  if not op['presplit']:
    return raw[:, :op['k']].astype(np.float64)
  slot, slot2, gain, bias = op['a_h2']
  words = [None if s is None else s.cpu().numpy().view(np.uint32) for s in (slot, slot2)]
  inv = wref.h2_scale(wref.slot_bound(words[0], words[1], gain, bias))[1]
  return wref.h2_values(raw, op['k'], inv)


def by_hand(net, ckpt, gt, d_in):
  """The new part of the chain, wrapper by wrapper in the documented order, from the d_in of
  decoder_conv1_grads: ({checkpoint name: gradient}, D0, d_cat, d_proj)."""
  from epos_amd import decoder_train as DT
  ch = net.chain_operands()
  op0, opf, opc = (net.crossed_pointwise_operand(s) for s in (CONV0_PW, FEATURE, PROJ))
  dw = net.crossed_depthwise_operand(CONV0_DW)
  B, h, w, c = dw['b'], dw['h'], dw['w'], dw['c']
  out = {}

  def put(scope, result):
    for short, t in result.items():
      out[scope + '/' + short] = t.view(1, 1, *t.shape) if t.dim() == 2 else t

  def bn_of(scope):
    return tuple(dev(ckpt, scope + '/' + v) for v in BN3)
  G0 = d_in.view(-1, 256)
  a0 = op0['a'].view(-1, op0['lda'])[:, :op0['k']]
  w0, bn0 = dev(ckpt, CONV0_PW + '/weights'), bn_of(CONV0_PW)
  put(CONV0_PW, DT.pointwise_weight_grads(a0, G0, w0, bn=bn0, eps=EPS, a_h2=op0['a_h2']))
  D0 = DT.pointwise_input_grad(G0, w0, bn=(bn0[0], bn0[2]), eps=EPS, relu_of=a0,
                               relu_of_h2=op0['presplit'])
  D4 = D0.view(B, h, w, c)
  x = ch['decoder_concat']
  put(CONV0_DW, DT.depthwise_weight_grads(x, D4, dev(ckpt, CONV0_DW + '/depthwise_weights'),
                                          bn_of(CONV0_DW), EPS, rate=1))
  d_cat = torch.full((B, h, w, c), float('nan'), device='cuda')
  w9c = dw['w9c']
  DT.depthwise_input_grad(D4[..., :256], w9c[:, :256].contiguous(), out=d_cat[..., :256])
  DT.depthwise_input_grad(D4[..., 256:], w9c[:, 256:].contiguous(), relu_of=x[..., 256:],
                          out=d_cat[..., 256:])
  put(FEATURE, DT.pointwise_weight_grads(ch['low_level'], d_cat[..., 256:],
                                         dev(ckpt, FEATURE + '/weights'), bn=bn_of(FEATURE),
                                         eps=EPS, a_h2=opf['a_h2']))
  d_proj = DT.resize_input_grad(d_cat[..., :256], ch['encoder_hw'],
                                relu_of=ch['concat_projection'])
  put(PROJ, DT.pointwise_weight_grads(ch['aspp_concat'], d_proj, dev(ckpt, PROJ + '/weights'),
                                      bn=bn_of(PROJ), eps=EPS, a_h2=opc['a_h2']))
  return out, D0, d_cat, d_proj


def check_bytes(net, ckpt, gt, presplit):
  """decoder_grads after a forward_logits: byte-equal, in its twelve shared gradients, values and
  bad, to decoder_conv1_grads, and in everything new to the wrappers called by hand. Returns
  (grads, d_in, D0, d_cat, d_proj)."""
  from epos_amd import decoder_train as DT, trainer
  variables = variables_of(ckpt)
  op0 = net.crossed_pointwise_operand(CONV0_PW)
  assert op0['presplit'] is presplit
  values, bad, grads, d_proj = trainer.decoder_grads(net, gt, variables, LOSS_WEIGHTS)
  values1, bad1, grads1, d_in = trainer.decoder_conv1_grads(net, gt, variables, LOSS_WEIGHTS)
  assert same_bytes(values, values1) and same_bytes(bad, bad1)
  assert sorted(grads1) == sorted(DT.VARIABLES + DT.DEPTHWISE_VARIABLES) and len(grads1) == 12
  assert sorted(grads) == sorted(tuple(grads1) + NEW) and len(grads) == 24
  for n in grads1:
    assert same_bytes(grads[n], grads1[n]), n
  hand, D0, d_cat, d_proj_hand = by_hand(net, ckpt, gt, d_in)
  assert sorted(hand) == sorted(NEW)
  for n in NEW:
    assert same_bytes(grads[n], hand[n]), n
    assert tuple(grads[n].shape) == tuple(ckpt[n].shape), n
    assert torch.isfinite(grads[n]).all() and grads[n].abs().max() > 0, n
  assert same_bytes(d_proj, d_proj_hand)
  eh, ew = net.chain_operands()['encoder_hw']
  assert tuple(d_proj.shape) == (NET_B, eh, ew, 256) and d_proj.dtype == torch.float32
  return grads, d_in, D0, d_cat, d_proj


@pytest.fixture(scope='module')
def chain(small_net):
  """(grads, d_in, D0, d_cat, d_proj) of one checked call, shared and left unchanged."""
  net, ckpt, mo, c, gt = small_net
  return check_bytes(net, ckpt, gt, presplit=True)


def test_the_new_operands_are_the_nets_own_buffers(small_net):
  net = small_net[0]
  from epos_amd import weights as W
  B, h, w = NET_B, net.out_h, net.out_w
  ch = net.chain_operands()
  assert (h, w) == (24, 32) and ch['encoder_hw'] == (12, 16)
  assert ch['decoder_hw'] == ch['low_level_hw'] == (h, w)
  assert tuple(ch['decoder_concat'].shape) == (B, h, w, 304)
  assert ch['decoder_concat'].data_ptr() == net.decoder_concat.data_ptr()
  assert ch['concat_projection'] is net.concat_projection
  assert tuple(ch['concat_projection'].shape) == (B, 12, 16, 256)
  assert ch['aspp_concat'] is net.aspp_concat and tuple(ch['aspp_concat'].shape) == (B, 12, 16, 1280)
  assert tuple(ch['low_level'].shape) == (B, h, w, 256)
  op0 = net.crossed_pointwise_operand(CONV0_PW)
  assert (op0['m'], op0['k'], op0['n'], op0['lda']) == (B * h * w, 304, 256, 320)
  assert op0['presplit'] and op0['packs'] is None and op0['eps'] == EPS
  opf = net.crossed_pointwise_operand(FEATURE)
  assert (opf['m'], opf['k'], opf['n']) == (B * h * w, 256, 48) and not opf['presplit']
  assert opf['a'].data_ptr() == ch['low_level'].data_ptr()
  opc = net.crossed_pointwise_operand(PROJ)
  assert (opc['m'], opc['k'], opc['n'], opc['lda']) == (B * 12 * 16, 1280, 256, 1280)
  assert opc['a'] is net.aspp_concat and not opc['presplit']
  dw = net.crossed_depthwise_operand()
  assert (dw['b'], dw['h'], dw['w'], dw['c'], dw['ldx'], dw['rate']) == (B, h, w, 304, 304, 1)
  assert dw['x'].data_ptr() == net.decoder_concat.data_ptr()
  assert tuple(dw['w9c'].shape) == (9, 304)
  # decoder_conv0_pointwise writes the x of decoder_conv1_depthwise, and the concat's first 256
  # channels are the resize of concat_projection (identical where the sample hits a source)
  assert net.depthwise_operand()['x'].data_ptr() != dw['x'].data_ptr()
  cat, proj = ch['decoder_concat'].cpu().numpy(), ch['concat_projection'].cpu().numpy()
  assert np.array_equal(cat[:, 0, 0, :256], proj[:, 0, 0]) and np.array_equal(
      cat[:, h - 1, w - 1, :256], proj[:, 11, 15])
  assert cat[..., 256:].min() >= 0 and proj.min() >= 0                    # behind their ReLUs
  for scope in (CONV0_PW, FEATURE, PROJ):
    consts = net.pointwise_constants(scope)
    assert all(a is b for a, b in zip(consts, net.pointwise_constants(scope)))
    for t, v in zip(consts, ('weights',) + BN3):
      assert t.is_cuda and np.array_equal(t.cpu().numpy(), small_net[1][scope + '/' + v])
  assert sorted(net.mode.packs) == sorted(W.TRAINABLE_LAYERS)


def test_decoder_grads_equal_decoder_conv1_grads_and_the_wrappers_by_hand(chain):
  assert len(chain[0]) == 24


def wgrad_check(what, A, G, ckpt, scope, grads, shorts=('weights', 'BatchNorm/gamma',
                                                         'BatchNorm/beta')):
  M = A.shape[0]
  S, g, aS, ag = wref.sums(A, G)
  K, N = S.shape
  Wm = ckpt[scope + '/weights'].reshape(K, N)
  bn = [ckpt[scope + '/' + v] for v in BN3]
  want = wref.close(S, g, Wm, *bn, eps=EPS)
  tol = wref.bounds_close(M, S, g, aS, ag, Wm, *bn, eps=EPS)
  for short, wv, tv in zip(shorts, want, tol):
    got = grads[scope + '/' + short].cpu().numpy().reshape(wv.shape)
    ok, worst = wref.within(got, wv, tv)
    print('%s %s (M=%d K=%d N=%d): worst error / bound = %.3g' % (what, short, M, K, N, worst))
    assert ok and np.abs(got).max() > 0, (scope, short, worst)


def test_every_new_gradient_is_within_its_kernels_bound(small_net, chain):
  """The restatements fed the device's own inputs: the widths the gradient kernels had not run
  from a net -- C = 304 in the depthwise sums, N = 48 and K = 1280 in the weight-gradient GEMM."""
  net, ckpt = small_net[0], small_net[1]
  grads, d_in, D0, d_cat, d_proj = chain
  B, h, w = NET_B, net.out_h, net.out_w
  M = B * h * w
  ch = net.chain_operands()
  op0 = net.crossed_pointwise_operand(CONV0_PW)
  A0 = a_values(op0)
  assert A0.shape == (M, 304) and A0.min() >= 0 and 0.05 < (A0 > 0).mean() < 0.95
  G0 = d_in.cpu().numpy().reshape(M, 256)
  wgrad_check('decoder_conv0_pointwise', A0, G0, ckpt, CONV0_PW, grads)
  Wf = ref.fold(ckpt[CONV0_PW + '/weights'].reshape(304, 256), ckpt[CONV0_PW + '/' + BN3[0]],
                ckpt[CONV0_PW + '/' + BN3[2]], EPS)
  want, absum = ref.pointwise_dgrad(G0, Wf, A0)
  D0h = D0.cpu().numpy()
  ok, worst = wref.within(D0h, want, ref.bound_pointwise_dgrad(256, want, absum))
  print('D0 [%d,304]: worst error / bound = %.3g' % (M, worst))
  assert ok and np.abs(D0h).max() > 0 and not D0h.view(np.uint32)[A0 <= 0].any()
  # the depthwise layer at C = 304
  xh = ch['decoder_concat'].cpu().numpy()
  D4 = D0h.reshape(B, h, w, 304)
  T, t, aT, at = ref.depthwise_wgrad(xh, D4, 1)
  w9 = ckpt[CONV0_DW + '/depthwise_weights'].reshape(9, 304)
  bn = [ckpt[CONV0_DW + '/' + v] for v in BN3]
  wantg = wref.close(T, t, w9, *bn, eps=EPS)
  tol = wref.bounds_close(M, T, t, aT, at, w9, *bn, eps=EPS)
  for short, wv, tv in zip(('depthwise_weights', 'BatchNorm/gamma', 'BatchNorm/beta'), wantg, tol):
    got = grads[CONV0_DW + '/' + short].cpu().numpy().reshape(wv.shape)
    ok, worst = wref.within(got, wv, tv)
    print('decoder_conv0_depthwise %s: worst error / bound = %.3g' % (short, worst))
    assert ok and np.abs(got).max() > 0, (short, worst)
  # its input gradient: bit for bit, the first 256 channels without a mask
  w9c = net.crossed_depthwise_operand()['w9c'].cpu().numpy()
  bits = ref.depthwise_dgrad(D4, w9c, 1)
  masked = ref.depthwise_dgrad(D4, w9c, 1, Y=xh)
  cat = d_cat.cpu().numpy()
  assert np.array_equal(cat[..., :256].view(np.uint32), bits[..., :256].view(np.uint32))
  assert np.array_equal(cat[..., 256:].view(np.uint32), masked[..., 256:].view(np.uint32))
  # feature_projection0: N = 48, G at row stride 304
  low = ch['low_level'].cpu().numpy().reshape(M, 256).astype(np.float64)
  wgrad_check('feature_projection0', low, cat[..., 256:].reshape(M, 48), ckpt, FEATURE, grads)
  # the resize adjoint: bit for bit, masked by concat_projection
  proj = ch['concat_projection'].cpu().numpy()
  bits = resize_grad_ref.resize_dgrad(np.ascontiguousarray(cat[..., :256]), 12, 16, Y=proj)
  dp = d_proj.cpu().numpy()
  assert np.array_equal(dp.view(np.uint32), bits.view(np.uint32)) and np.abs(dp).max() > 0
  # concat_projection: K = 1280
  aspp = ch['aspp_concat'].cpu().numpy().reshape(B * 12 * 16, 1280).astype(np.float64)
  wgrad_check('concat_projection', aspp, dp.reshape(-1, 256), ckpt, PROJ, grads)


def test_the_masks(small_net, chain):
  """Channels 0:256 of the concat gradient carry NO mask -- behind them lies the resize, not a
  ReLU; channels 256:304 are +0.0 wherever feature_projection0's output is; d_proj is +0.0
  wherever concat_projection is."""
  net = small_net[0]
  grads, d_in, D0, d_cat, d_proj = chain
  ch = net.chain_operands()
  cat = ch['decoder_concat'].cpu().numpy()
  g = d_cat.cpu().numpy()
  shut = cat[..., :256] <= 0
  assert shut.any(), 'no element of the resized concat_projection is <= 0 in this case'
  n_open = int((g[..., :256][shut] != 0).sum())
  print('concat gradient, channels 0:256: %d of %d elements non-zero where decoder_concat <= 0' % (
      n_open, int(shut.sum())))
  assert n_open > 0
  low_shut = cat[..., 256:] <= 0
  assert low_shut.any() and not g[..., 256:].view(np.uint32)[low_shut].any()
  assert (g[..., 256:][~low_shut] != 0).any()
  proj = ch['concat_projection'].cpu().numpy()
  dp = d_proj.cpu().numpy()
  assert (proj <= 0).any() and not dp.view(np.uint32)[proj <= 0].any()
  assert (dp[proj > 0] != 0).mean() > 0.5


def test_the_chain_copies_nothing_from_the_host_and_does_not_synchronise(small_net, chain):
  net, ckpt, mo, c, gt = small_net
  from epos_amd import trainer
  variables = variables_of(ckpt)
  name = CONV0_DW + '/BatchNorm/gamma'
  given = dict(variables, **{name: dev(ckpt, name) * 2})
  torch.cuda.synchronize()
  torch.cuda.set_sync_debug_mode('error')
  try:
    got = trainer.decoder_grads(net, gt, variables, LOSS_WEIGHTS)
    got2 = trainer.decoder_grads(net, gt, given, LOSS_WEIGHTS)
  finally:
    torch.cuda.set_sync_debug_mode('default')
  torch.cuda.synchronize()
  assert same_bytes(got[3], chain[4])
  for n in chain[0]:
    assert same_bytes(got[2][n], chain[0][n]), n
  # a variable given on the device overrides the net's copy: dw = scale T moves, dbeta = t not
  assert not same_bytes(got2[2][CONV0_DW + '/depthwise_weights'],
                        got[2][CONV0_DW + '/depthwise_weights'])
  assert same_bytes(got2[2][CONV0_DW + '/BatchNorm/beta'], got[2][CONV0_DW + '/BatchNorm/beta'])


def test_an_fp32_a0_in_a_child_process():
  """EPOS_H2_PRESPLIT=0 is read when the plan is built: a child process builds the same net with
  an fp32 A0 and repeats the byte-equalities."""
  env = dict(os.environ, EPOS_H2_PRESPLIT='0')
  done = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT,
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
  text = done.stdout.decode('utf-8', 'replace')
  assert done.returncode == 0 and 'fp32 A0: OK' in text, text[-3000:]


# ----------------------------------------------------------- torch autograd ---
def autograd_grads(net, ckpt, gt):
  """{checkpoint name: gradient} and d_proj from torch's fp64 autograd through a torch.nn
  restatement of the decoder, fed the net's own aspp_concat and low-level tap: 1x1 conv -> BN ->
  ReLU -> interpolate(align_corners=True) -> concat with the projected low-level tap -> two
  separable convs -> logits -> loss.differentiable_losses (the logits pinned to the net's own, so
  that the loss gradient at the logits is the chain's)."""
  from epos_amd import heads_train as HT, loss as L
  Fn = torch.nn.functional
  ch = net.chain_operands()
  B, h, w = NET_B, net.out_h, net.out_w
  leaves = {}

  def leaf(name):
    leaves[name] = dev(ckpt, name).double().requires_grad_()
    return leaves[name]

  def frozen(scope):
    return tuple(dev(ckpt, scope + '/' + v).double() for v in BN3[1:])

  def bn_relu(z, scope):
    mean, var = frozen(scope)
    rstd = 1.0 / torch.sqrt(var + EPS)
    pre = (z - mean) * (leaf(scope + '/BatchNorm/gamma') * rstd) + leaf(scope + '/BatchNorm/beta')
    return torch.relu(pre), pre

  def pointwise(x, scope):
    wt = leaf(scope + '/weights')
    return bn_relu(x @ wt.view(wt.shape[2], wt.shape[3]), scope)

  def depthwise(x, scope):
    wt = leaf(scope + '/depthwise_weights')
    xp = Fn.pad(x, (0, 0, 1, 1, 1, 1))                     # 'SAME': a ring of zeros around H and W
    z = sum(xp[:, ky:ky + h, kx:kx + w, :] * wt[ky, kx, :, 0] for ky in range(3) for kx in range(3))
    return bn_relu(z, scope)[0]

  proj, pre_proj = pointwise(ch['aspp_concat'].double(), PROJ)
  pre_proj.retain_grad()
  up = Fn.interpolate(proj.permute(0, 3, 1, 2), size=(h, w), mode='bilinear',
                      align_corners=True).permute(0, 2, 3, 1)
  low = pointwise(ch['low_level'].double(), FEATURE)[0]
  x = torch.cat([up, low], dim=-1)
  for j in range(2):
    scope = 'decoder/decoder_conv%d' % j
    x = pointwise(depthwise(x, scope + '_depthwise'), scope + '_pointwise')[0]
  with torch.no_grad():                                    # the net's decoder against fp64
    out = net.decoder_out.double()
    assert float((x - out).abs().max()) < 1e-3 * max(1.0, float(out.abs().max()))
  logits = HT.net_logits(net)
  pinned = {}
  for k in logits:
    wt, b = leaf('logits/%s/weights' % k), leaf('logits/%s/biases' % k)
    lin = (x.reshape(-1, 256) @ wt.view(256, -1) + b).view(logits[k].shape)
    pinned[k] = (lin + (logits[k].double() - lin).detach()).float()
  values, _ = L.differentiable_losses(pinned, gt, LOSS_WEIGHTS, 'pooled')
  values[3].backward()
  return {n: t.grad for n, t in leaves.items()}, pre_proj.grad, values.detach()


def layer_of(name):
  return name.split('/BatchNorm/')[0] if '/BatchNorm/' in name else name.rsplit('/', 1)[0]


def test_the_chain_agrees_with_torch_fp64_autograd(small_net, chain):
  net, ckpt, mo, c, gt = small_net
  from epos_amd import trainer
  grads, d_in, D0, d_cat, d_proj = chain
  want, want_proj, values = autograd_grads(net, ckpt, gt)
  assert torch.equal(values, trainer.decoder_grads(net, gt, variables_of(ckpt), LOSS_WEIGHTS)[0])
  assert sorted(want) == sorted(grads)
  figures = {}
  for n in sorted(grads):
    exp = want[n].reshape(grads[n].shape)
    assert float(exp.abs().max()) > 0, n
    figures[n] = float((grads[n].double() - exp).abs().max() / exp.abs().max())
  figures['d_proj'] = float((d_proj.double() - want_proj).abs().max() / want_proj.abs().max())
  worst = {}
  for n, f in figures.items():
    key = 'd_proj' if n == 'd_proj' else layer_of(n)
    worst[key] = max(worst.get(key, 0.0), f)
    print('autograd: %-60s max |chain - autograd| / max |autograd| = %.3g' % (n, f))
  for key in sorted(worst):
    print('autograd, by layer: %-40s %.3g' % (key, worst[key]))
  assert sorted(worst) == sorted(MEASURED)
  failed = []
  for key, f in worst.items():
    allowed = MARGIN * MEASURED[key]
    assert allowed < LIMIT, (key, allowed)                 # a wrong sign or factor cannot pass
    if not f <= allowed:
      failed.append((key, f, allowed))
  assert not failed, failed


if __name__ == '__main__':                    # the child of the fp32-A0 test
  from epos_amd import model, synthetic, weights
  assert os.environ.get('EPOS_H2_PRESPLIT') == '0'
  ckpt_ = weights.random_init('xception_65', num_objs=NET_O, num_frags=NET_F, seed=5,
                              randomize_bn=True)
  mo_ = model.ModelOptions(model.get_outputs_to_num_channels(NET_O, NET_F),
                           crop_size=(NET_W, NET_H))
  net_ = model.get_net(ckpt_, NET_B, NET_H, NET_W, NET_O, NET_F, mo_, 'cuda:0')
  imgs_ = np.stack([synthetic.image(i, NET_H, NET_W) for i in range(NET_B)]).astype(np.float32)
  net_.forward_logits(imgs_)
  torch.cuda.synchronize()
  case_ = loss_cases.make_case(NET_B, net_.out_h * net_.out_w, NET_O, NET_F, seed=33)
  check_bytes(net_, ckpt_, gt_tensors(case_, net_.out_h, net_.out_w), presplit=False)
  print('fp32 A0: OK')
