"""The backward pass through ASPP from a running net (trainer.aspp_grads) on two nets of 96 x 128,
encoder 12 x 16, B = 2: the small net of tests/helpers/loss_device.py with the default rates
(12, 24, 36), where most taps lie in the padding, and one with rates (1, 2, 3), where every tap is
live. The records against the net's own buffers, the chain against decoder_grads and against its
wrappers called by hand, every new weight gradient within its kernel's bound of the restatements
fed the device's own inputs, d_enc bit for bit, the mask, the chain without a synchronisation,
with fp32 A operands in a child process, and against torch's fp64 autograd through a torch.nn
restatement of ASPP and the decoder."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import aspp_grad_ref as aref                           # noqa: E402
from tests.helpers import decoder_backward_ref as ref                     # noqa: E402
from tests.helpers import loss_cases, pointwise_wgrad_ref as wref         # noqa: E402
from tests.helpers.loss_device import (NET_B, NET_F, NET_H, NET_O, NET_W,     # noqa: E402,F401
                                       gt_tensors, small_net)

pytestmark = pytest.mark.gpu

LOSS_WEIGHTS = (0.7, 1.3, 100.0)
EPS = 1e-5
EH, EW, EC = 12, 16, 2048
PROJ = 'concat_projection'
BN3 = ('BatchNorm/gamma', 'BatchNorm/moving_mean', 'BatchNorm/moving_variance')
LIVE_RATES = (1, 2, 3)

# The largest |chain - autograd| / max |autograd| per gradient that
# test_the_chain_agrees_with_torch_fp64_autograd measured on the MI355X (profiles/r31/README.md),
# by the layer the gradient belongs to, the larger of the two nets. The restatement runs in fp64
# from the net's fp32 encoder output and low-level tap; the chain reads fp32 (or fp16-pair)
# activations, fp32-folded weights and fp32 resize coordinates, and a ReLU whose input lies within
# that difference of zero is open on one side and shut on the other. The test allows MARGIN times
# the measured figure; a wrong sign gives 2 and a dropped factor of two 0.5, so every allowance
# must stay below LIMIT.
MEASURED = {
    'logits/pred_obj_conf': 2.74e-07, 'logits/pred_frag_conf': 1.49e-07,
    'logits/pred_frag_loc': 1.95e-07,
    'decoder/decoder_conv1_pointwise': 3.78e-07, 'decoder/decoder_conv1_depthwise': 5.89e-07,
    'decoder/decoder_conv0_pointwise': 4.48e-07, 'decoder/decoder_conv0_depthwise': 1.37e-06,
    'decoder/feature_projection0': 1.95e-07, 'concat_projection': 6.18e-07,
    'image_pooling': 3.81e-07, 'aspp0': 3.26e-07,
    'aspp1_pointwise': 5.92e-07, 'aspp1_depthwise': 2.44e-07,
    'aspp2_pointwise': 2.78e-07, 'aspp2_depthwise': 2.54e-07,
    'aspp3_pointwise': 3.50e-07, 'aspp3_depthwise': 2.81e-07,
    'd_enc': 1.14e-06,
}
# 8 x: the figures are maxima over one batch and one set of weights, and a ReLU within rounding
# of zero opens on one side only
MARGIN, LIMIT = 8.0, 0.05


def pw_scopes(rates):
  return ['image_pooling', 'aspp0'] + ['aspp%d_pointwise' % i for i in range(1, len(rates) + 1)]


def dw_scopes(rates):
  return ['aspp%d_depthwise' % i for i in range(1, len(rates) + 1)]


def new_names(rates):
  return tuple(s + '/' + v for s in pw_scopes(rates)
               for v in ('weights', 'BatchNorm/gamma', 'BatchNorm/beta')) + tuple(
                   s + '/' + v for s in dw_scopes(rates)
                   for v in ('depthwise_weights', 'BatchNorm/gamma', 'BatchNorm/beta'))


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


def by_hand(net, ckpt, d_proj):
  """The new part of the chain, wrapper by wrapper in the documented order, from the d_proj of
  decoder_grads: ({checkpoint name: gradient}, the intermediate tensors, d_enc)."""
  from epos_amd import decoder_train as DT
  ap = net.aspp_operands()
  enc, rates = ap['encoder'], ap['rates']
  B = NET_B
  out, mid = {}, {}

  def put(scope, result):
    for short, t in result.items():
      out[scope + '/' + short] = t.view(1, 1, *t.shape) if t.dim() == 2 else t

  def bn_of(scope):
    return tuple(dev(ckpt, scope + '/' + v) for v in BN3)
  wc, bnc = dev(ckpt, PROJ + '/weights'), bn_of(PROJ)
  D_cat = DT.pointwise_input_grad(d_proj.view(-1, 256), wc, bn=(bnc[0], bnc[2]), eps=EPS,
                                  relu_of=ap['aspp_concat'])
  D_cat = D_cat.view(B, EH, EW, -1)
  branch = lambda s: D_cat[..., 256 * s:256 * (s + 1)]       # noqa: E731
  g_pool = DT.pool_broadcast_grad(branch(0))
  w, bn = dev(ckpt, 'image_pooling/weights'), bn_of('image_pooling')
  put('image_pooling', DT.pointwise_weight_grads(ap['pooled'], g_pool, w, bn=bn, eps=EPS))
  d_pooled = DT.pointwise_input_grad(g_pool, w, bn=(bn[0], bn[2]), eps=EPS)
  w, bn = dev(ckpt, 'aspp0/weights'), bn_of('aspp0')
  op = ap['pointwise']['aspp0']
  put('aspp0', DT.pointwise_weight_grads(enc, branch(1), w, bn=bn, eps=EPS, a_h2=op['a_h2']))
  E0 = DT.pointwise_input_grad(branch(1), w, bn=(bn[0], bn[2]), eps=EPS)
  Ds = []
  for i, r in enumerate(rates, 1):
    pw, dws = 'aspp%d_pointwise' % i, 'aspp%d_depthwise' % i
    op, dw = ap['pointwise'][pw], ap['depthwise'][dws]
    a = op['a'].view(-1, op['lda'])[:, :op['k']]
    w, bn = dev(ckpt, pw + '/weights'), bn_of(pw)
    put(pw, DT.pointwise_weight_grads(a, branch(i + 1), w, bn=bn, eps=EPS, a_h2=op['a_h2']))
    D = DT.pointwise_input_grad(branch(i + 1), w, bn=(bn[0], bn[2]), eps=EPS, relu_of=a,
                                relu_of_h2=op['presplit']).view(B, EH, EW, EC)
    put(dws, DT.depthwise_weight_grads(enc, D, dev(ckpt, dws + '/depthwise_weights'),
                                       bn_of(dws), EPS, rate=r))
    Ds.append((D, dw['w9c'], r))
  d_enc = DT.aspp_join_grad(depthwise=Ds, plain=[E0], pooled=(d_pooled, EH * EW),
                            relu_of=enc if ap['encoder_relu'] else None)
  mid.update(D_cat=D_cat, g_pool=g_pool, d_pooled=d_pooled, E0=E0, Ds=Ds)
  return out, mid, d_enc


def check_bytes(net, ckpt, gt, presplit):
  """aspp_grads after a forward_logits: byte-equal, in its 24 shared gradients, values and bad,
  to decoder_grads, and in everything new to the wrappers called by hand. Returns (grads, the
  intermediate tensors, d_enc)."""
  from epos_amd import trainer
  variables = variables_of(ckpt)
  rates = net.aspp_operands()['rates']
  for s in pw_scopes(rates)[2:]:
    assert net.aspp_operands()['pointwise'][s]['presplit'] is presplit, s
  values, bad, grads, d_enc = trainer.aspp_grads(net, gt, variables, LOSS_WEIGHTS)
  values1, bad1, grads1, d_proj = trainer.decoder_grads(net, gt, variables, LOSS_WEIGHTS)
  assert same_bytes(values, values1) and same_bytes(bad, bad1) and len(grads1) == 24
  new = new_names(rates)
  assert len(new) == 3 * (2 + 2 * len(rates))
  assert sorted(grads) == sorted(tuple(grads1) + new) and len(grads) == 24 + len(new)
  for n in grads1:
    assert same_bytes(grads[n], grads1[n]), n
  hand, mid, d_enc_hand = by_hand(net, ckpt, d_proj)
  assert sorted(hand) == sorted(new)
  for n in new:
    assert same_bytes(grads[n], hand[n]), n
    assert tuple(grads[n].shape) == tuple(ckpt[n].shape), n
    assert torch.isfinite(grads[n]).all() and grads[n].abs().max() > 0, n
  assert same_bytes(d_enc, d_enc_hand)
  assert tuple(d_enc.shape) == (NET_B, EH, EW, EC) and d_enc.dtype == torch.float32
  return grads, mid, d_enc


def live_net():
  """The second net: the small net's size and checkpoint layout with rates (1, 2, 3)."""
  from epos_amd import model, synthetic, weights
  ckpt = weights.random_init('xception_65', num_objs=NET_O, num_frags=NET_F, seed=6,
                             randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(NET_O, NET_F),
                          crop_size=(NET_W, NET_H), atrous_rates=LIVE_RATES)
  net = model.get_net(ckpt, NET_B, NET_H, NET_W, NET_O, NET_F, mo, 'cuda:0')
  imgs = np.stack([synthetic.image(i, NET_H, NET_W) for i in range(NET_B)]).astype(np.float32)
  net.forward_logits(imgs)
  torch.cuda.synchronize()
  c = loss_cases.make_case(NET_B, net.out_h * net.out_w, NET_O, NET_F, seed=33)
  return net, ckpt, gt_tensors(c, net.out_h, net.out_w)


@pytest.fixture(scope='module', params=['padding', 'live'])
def chain(request, small_net):
  """(net, ckpt, gt, (grads, intermediates, d_enc) of one checked call), shared and left
  unchanged, for the net with the default rates and for the one with (1, 2, 3)."""
  if request.param == 'padding':
    net, ckpt, gt = small_net[0], small_net[1], small_net[4]
  else:
    net, ckpt, gt = live_net()
  return net, ckpt, gt, check_bytes(net, ckpt, gt, presplit=True)


def test_the_records_are_the_nets_own_buffers(chain):
  net, ckpt = chain[0], chain[1]
  from epos_amd import weights as W
  B = NET_B
  ap = net.aspp_operands()
  rates = ap['rates']
  assert rates == net.atrous_rates and rates in ((12, 24, 36), LIVE_RATES)
  assert tuple(ap['encoder'].shape) == (B, EH, EW, EC)
  assert ap['encoder'].data_ptr() == net.encoder.data_ptr() and ap['encoder_relu'] is True
  assert ap['aspp_concat'] is net.aspp_concat
  assert tuple(ap['aspp_concat'].shape) == (B, EH, EW, 256 * (2 + len(rates)))
  enc, cat = ap['encoder'].cpu().numpy(), ap['aspp_concat'].cpu().numpy()
  assert enc.min() >= 0 and 0.05 < (enc > 0).mean() < 0.95
  # pooled is the mean of the encoder output, pool_feat what slice 0 of the concat broadcasts
  pooled = ap['pooled'].cpu().numpy()
  assert pooled.shape == (B, EC)
  assert np.abs(pooled - enc.astype(np.float64).mean(axis=(1, 2))).max() <= 1e-5 * pooled.max()
  pf = ap['pool_feat'].cpu().numpy()
  assert pf.shape == (B, 256) and np.array_equal(cat[..., :256], np.broadcast_to(
      pf[:, None, None, :], (B, EH, EW, 256)))
  ip = ap['pointwise']['image_pooling']
  assert ip['a'] is ap['pooled'] and (ip['m'], ip['k'], ip['n']) == (B, EC, 256)
  a0 = ap['pointwise']['aspp0']
  assert a0['a'].data_ptr() == net.encoder.data_ptr() and not a0['presplit']
  assert (a0['m'], a0['k'], a0['n']) == (B * EH * EW, EC, 256)
  for i, r in enumerate(rates, 1):
    d = ap['depthwise']['aspp%d_depthwise' % i]
    assert d['x'].data_ptr() == net.encoder.data_ptr() and d['rate'] == r
    assert (d['b'], d['h'], d['w'], d['c']) == (B, EH, EW, EC)
    p = ap['pointwise']['aspp%d_pointwise' % i]
    assert p['presplit'] and p['packs'] is None and p['eps'] == EPS
    # the layer's A is the depthwise layer's output: its forward on the encoder output
    w9c, bias = d['w9c'].cpu().numpy(), d['bias'].cpu().numpy()
    fwd = ref.depthwise_forward(enc, w9c, bias, r).reshape(-1, EC)
    got = a_values(p)
    assert np.abs(got - fwd).max() <= 2e-3 * max(1.0, np.abs(fwd).max())
  for scope in pw_scopes(rates) + dw_scopes(rates):
    consts = net.aspp_constants(scope)
    assert all(a is b for a, b in zip(consts, net.aspp_constants(scope)))
    first = 'depthwise_weights' if scope.endswith('depthwise') else 'weights'
    for t, v in zip(consts, (first,) + BN3):
      assert t.is_cuda and np.array_equal(t.cpu().numpy(), ckpt[scope + '/' + v])
  assert sorted(net.mode.packs) == sorted(W.TRAINABLE_LAYERS)


def test_aspp_grads_equal_decoder_grads_and_the_wrappers_by_hand(chain):
  grads = chain[3][0]
  assert len(grads) == 24 + 3 * (2 + 2 * len(chain[0].atrous_rates))


def wgrad_check(what, A, G, ckpt, scope, grads):
  M = A.shape[0]
  S, g, aS, ag = wref.sums(A, G)
  K, N = S.shape
  Wm = ckpt[scope + '/weights'].reshape(K, N)
  bn = [ckpt[scope + '/' + v] for v in BN3]
  want = wref.close(S, g, Wm, *bn, eps=EPS)
  tol = wref.bounds_close(M, S, g, aS, ag, Wm, *bn, eps=EPS)
  for short, wv, tv in zip(('weights', 'BatchNorm/gamma', 'BatchNorm/beta'), want, tol):
    got = grads[scope + '/' + short].cpu().numpy().reshape(wv.shape)
    ok, worst = wref.within(got, wv, tv)
    print('%s %s (M=%d K=%d N=%d): worst error / bound = %.3g' % (what, short, M, K, N, worst))
    assert ok and np.abs(got).max() > 0, (scope, short, worst)


def test_every_new_gradient_is_within_its_kernels_bound_and_d_enc_bit_for_bit(chain):
  """The restatements fed the device's own inputs, at the widths the gradient kernels had not
  run from a net: K = 2048 in both GEMMs, M = B, C = 2048 and rates up to 36 in the depthwise
  sums; the broadcast's adjoint to its bound; the join bit for bit."""
  net, ckpt, gt, (grads, mid, d_enc) = chain
  ap = net.aspp_operands()
  rates, B, M = ap['rates'], NET_B, NET_B * EH * EW
  D_cat = mid['D_cat'].cpu().numpy()
  nb = 2 + len(rates)
  # D_cat: K = 1280 (or 256 nb), masked by the concat
  cat = ap['aspp_concat'].cpu().numpy().reshape(M, 256 * nb)
  Wf = ref.fold(ckpt[PROJ + '/weights'].reshape(256 * nb, 256), ckpt[PROJ + '/' + BN3[0]],
                ckpt[PROJ + '/' + BN3[2]], EPS)
  from epos_amd import trainer
  d_proj = trainer.decoder_grads(net, gt, variables_of(ckpt), LOSS_WEIGHTS)[3].cpu().numpy()
  want, absum = ref.pointwise_dgrad(d_proj.reshape(M, 256), Wf, cat)
  ok, worst = wref.within(D_cat.reshape(M, -1), want, ref.bound_pointwise_dgrad(256, want, absum))
  print('D_cat [%d,%d]: worst error / bound = %.3g' % (M, 256 * nb, worst))
  assert ok and not D_cat.reshape(M, -1).view(np.uint32)[cat <= 0].any()
  # the broadcast's adjoint
  g_pool = mid['g_pool'].cpu().numpy()
  want, bound = aref.pool_broadcast_ref(D_cat[..., :256].reshape(B, EH * EW, 256))
  ok, worst = wref.within(g_pool, want, bound)
  print('g_pool [%d,256]: worst error / bound = %.3g' % (B, worst))
  assert ok and np.abs(g_pool).max() > 0
  enc = ap['encoder'].cpu().numpy()
  wgrad_check('image_pooling', ap['pooled'].cpu().numpy().astype(np.float64), g_pool, ckpt,
              'image_pooling', grads)
  wgrad_check('aspp0', enc.reshape(M, EC).astype(np.float64), D_cat[..., 256:512].reshape(M, 256),
              ckpt, 'aspp0', grads)
  terms = []
  for i, r in enumerate(rates, 1):
    pw, dws = 'aspp%d_pointwise' % i, 'aspp%d_depthwise' % i
    A = a_values(ap['pointwise'][pw])
    wgrad_check(pw, A, D_cat[..., 256 * (i + 1):256 * (i + 2)].reshape(M, 256), ckpt, pw, grads)
    D, w9c, _ = mid['Ds'][i - 1]
    Dh = D.cpu().numpy()
    assert not Dh.reshape(M, EC).view(np.uint32)[A <= 0].any() and np.abs(Dh).max() > 0
    T, t, aT, at = ref.depthwise_wgrad(enc, Dh, r)
    w9 = ckpt[dws + '/depthwise_weights'].reshape(9, EC)
    bn = [ckpt[dws + '/' + v] for v in BN3]
    wantg = wref.close(T, t, w9, *bn, eps=EPS)
    tol = wref.bounds_close(M, T, t, aT, at, w9, *bn, eps=EPS)
    for short, wv, tv in zip(('depthwise_weights', 'BatchNorm/gamma', 'BatchNorm/beta'), wantg,
                             tol):
      got = grads[dws + '/' + short].cpu().numpy().reshape(wv.shape)
      ok, worst = wref.within(got, wv, tv)
      print('%s %s (rate %d): worst error / bound = %.3g' % (dws, short, r, worst))
      assert ok and np.abs(got).max() > 0, (dws, short, worst)
    terms.append((Dh, w9c.cpu().numpy(), r))
  # d_enc: bit for bit from the device's own D_i, E0, d_pooled and encoder
  bits = aref.aspp_join_ref((B, EH, EW, EC), terms, [mid['E0'].cpu().numpy()],
                            (mid['d_pooled'].cpu().numpy(), EH * EW), Y=enc)
  got = d_enc.cpu().numpy()
  assert np.array_equal(got.view(np.uint32), bits.view(np.uint32))
  # the mask: +0.0 wherever the encoder output is <= 0, and not identically zero
  assert (enc <= 0).any() and not got.view(np.uint32)[enc <= 0].any()
  assert (got[enc > 0] != 0).mean() > 0.5


def test_the_chain_copies_nothing_from_the_host_and_does_not_synchronise(chain):
  net, ckpt, gt, (grads, mid, d_enc) = chain
  from epos_amd import trainer
  variables = variables_of(ckpt)
  name = 'aspp0/BatchNorm/gamma'
  given = dict(variables, **{name: dev(ckpt, name) * 2})
  torch.cuda.synchronize()
  torch.cuda.set_sync_debug_mode('error')
  try:
    got = trainer.aspp_grads(net, gt, variables, LOSS_WEIGHTS)
    got2 = trainer.aspp_grads(net, gt, given, LOSS_WEIGHTS)
  finally:
    torch.cuda.set_sync_debug_mode('default')
  torch.cuda.synchronize()
  assert same_bytes(got[3], d_enc)
  for n in grads:
    assert same_bytes(got[2][n], grads[n]), n
  # a variable given on the device overrides the net's copy: dW = scale S moves, dbeta = g not
  assert not same_bytes(got2[2]['aspp0/weights'], got[2]['aspp0/weights'])
  assert same_bytes(got2[2]['aspp0/BatchNorm/beta'], got[2]['aspp0/BatchNorm/beta'])
  assert not same_bytes(got2[3], got[3])                   # and E0 with it


def test_fp32_a_operands_in_a_child_process():
  """EPOS_H2_PRESPLIT=0 is read when the plan is built: a fresh child process builds the same
  net with fp32 A operands and repeats the byte-equalities."""
  env = dict(os.environ, EPOS_H2_PRESPLIT='0')
  done = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT,
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
  text = done.stdout.decode('utf-8', 'replace')
  assert done.returncode == 0 and 'fp32 A: OK' in text, text[-3000:]


# ----------------------------------------------------------- torch autograd ---
def autograd_grads(net, ckpt, gt):
  """{checkpoint name: gradient} and d_enc from torch's fp64 autograd through a torch.nn
  restatement of ASPP and the decoder, fed the net's own fp32 encoder output (as the leaf in
  front of its ReLU) and low-level tap."""
  from epos_amd import heads_train as HT, loss as L
  Fn = torch.nn.functional
  ch, ap = net.chain_operands(), net.aspp_operands()
  B, h, w = NET_B, net.out_h, net.out_w
  leaves = {}

  def leaf(name):
    leaves[name] = dev(ckpt, name).double().requires_grad_()
    return leaves[name]

  def bn_relu(z, scope):
    mean, var = (dev(ckpt, scope + '/' + v).double() for v in BN3[1:])
    rstd = 1.0 / torch.sqrt(var + EPS)
    return torch.relu((z - mean) * (leaf(scope + '/BatchNorm/gamma') * rstd) +
                      leaf(scope + '/BatchNorm/beta'))

  def pointwise(x, scope):
    wt = leaf(scope + '/weights')
    return bn_relu(x @ wt.view(wt.shape[2], wt.shape[3]), scope)

  def depthwise(x, scope, rate=1):
    wt = leaf(scope + '/depthwise_weights')
    c = x.shape[-1]
    z = Fn.conv2d(x.permute(0, 3, 1, 2), wt[:, :, :, 0].permute(2, 0, 1).unsqueeze(1),
                  padding=rate, dilation=rate, groups=c).permute(0, 2, 3, 1)
    return bn_relu(z, scope)

  pre = ap['encoder'].double().contiguous().requires_grad_()
  x = torch.relu(pre)
  pf = pointwise(x.mean(dim=(1, 2)), 'image_pooling')
  parts = [pf[:, None, None, :].expand(B, EH, EW, 256), pointwise(x, 'aspp0')]
  for i, r in enumerate(ap['rates'], 1):
    parts.append(pointwise(depthwise(x, 'aspp%d_depthwise' % i, r), 'aspp%d_pointwise' % i))
  proj = pointwise(torch.cat(parts, dim=-1), PROJ)
  up = Fn.interpolate(proj.permute(0, 3, 1, 2), size=(h, w), mode='bilinear',
                      align_corners=True).permute(0, 2, 3, 1)
  low = pointwise(ch['low_level'].double(), 'decoder/feature_projection0')
  y = torch.cat([up, low], dim=-1)
  for j in range(2):
    scope = 'decoder/decoder_conv%d' % j
    y = pointwise(depthwise(y, scope + '_depthwise'), scope + '_pointwise')
  with torch.no_grad():                                    # the net's decoder against fp64
    out = net.decoder_out.double()
    assert float((y - out).abs().max()) < 1e-3 * max(1.0, float(out.abs().max()))
  logits = HT.net_logits(net)
  pinned = {}
  for k in logits:
    wt, b = leaf('logits/%s/weights' % k), leaf('logits/%s/biases' % k)
    lin = (y.reshape(-1, 256) @ wt.view(256, -1) + b).view(logits[k].shape)
    pinned[k] = (lin + (logits[k].double() - lin).detach()).float()
  values, _ = L.differentiable_losses(pinned, gt, LOSS_WEIGHTS, 'pooled')
  values[3].backward()
  return {n: t.grad for n, t in leaves.items()}, pre.grad


def layer_of(name):
  return name.split('/BatchNorm/')[0] if '/BatchNorm/' in name else name.rsplit('/', 1)[0]


def test_the_chain_agrees_with_torch_fp64_autograd(chain):
  net, ckpt, gt, (grads, mid, d_enc) = chain
  want, want_enc = autograd_grads(net, ckpt, gt)
  assert sorted(want) == sorted(grads)
  figures = {}
  for n in sorted(grads):
    exp = want[n].reshape(grads[n].shape)
    assert float(exp.abs().max()) > 0, n
    figures[n] = float((grads[n].double() - exp).abs().max() / exp.abs().max())
  figures['d_enc'] = float((d_enc.double() - want_enc).abs().max() / want_enc.abs().max())
  worst = {}
  for n, f in figures.items():
    key = 'd_enc' if n == 'd_enc' else layer_of(n)
    worst[key] = max(worst.get(key, 0.0), f)
  for key in sorted(worst):
    print('autograd, rates %s, by layer: %-40s %.3g' % (net.atrous_rates, key, worst[key]))
  assert sorted(worst) == sorted(MEASURED)
  failed = []
  for key, f in worst.items():
    allowed = MARGIN * MEASURED[key]
    assert allowed < LIMIT, (key, allowed)                 # a wrong sign or factor cannot pass
    if not f <= allowed:
      failed.append((key, f, allowed))
  assert not failed, failed


if __name__ == '__main__':                    # the child of the fp32-A test
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
  print('fp32 A: OK')
