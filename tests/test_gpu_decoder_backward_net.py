"""The backward pass through decoder_conv1 from a running net (EposNet.depthwise_operand,
trainer.decoder_conv1_grads) on the small net of tests/helpers/loss_device.py: the operand the
plan recorded against the net's own buffers, the chain against its five wrappers called by hand
and against net_grads, the kernels' bounds on the net's own bytes with the mask as fp16 pairs and
-- in a child process, where the switch is read -- as fp32, and the next layer's weight gradients
from the chain's result."""
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
from tests.helpers.loss_device import (NET_B, NET_F, NET_H, NET_O, NET_W,     # noqa: E402,F401
                                       gt_tensors, small_net)

pytestmark = pytest.mark.gpu

LOSS_WEIGHTS = (0.7, 1.3, 100.0)


def variables_of(ckpt):
  from epos_amd import decoder_train as DT
  return {n: torch.from_numpy(np.ascontiguousarray(ckpt[n])).cuda() for n in DT.VARIABLES}


def same_bytes(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and \
      a.contiguous().view(torch.uint8).equal(b.contiguous().view(torch.uint8))


def mask_values(op):
  """fp64 [M,K]: the sign-carrying values of the net's own A, from its bytes."""
  raw = op['a'].cpu().numpy().reshape(op['m'], op['lda'])
  return ref.pair_values(raw, op['k']) if op['presplit'] else raw[:, :op['k']].astype(np.float64)


def check_chain(net, ckpt, gt, presplit):
  """decoder_conv1_grads after a forward_logits: byte-equal to the five wrappers called by hand
  and, in its nine shared gradients, to net_grads; each new kernel within its bound (the
  depthwise input gradient: bit for bit) of the restatement fed the device's own inputs."""
  from epos_amd import decoder_train as DT, heads_train as HT, loss as L, trainer
  from epos_amd import weights as W
  op, dw = net.pointwise_operand(), net.depthwise_operand()
  assert op['presplit'] is presplit
  B, h, w, C = dw['b'], dw['h'], dw['w'], dw['c']
  assert (B, h, w, C, dw['rate']) == (NET_B, net.out_h, net.out_w, 256, 1)
  M = B * h * w
  variables = variables_of(ckpt)
  values, bad, grads, d_in = trainer.decoder_conv1_grads(net, gt, variables, LOSS_WEIGHTS)
  assert sorted(grads) == sorted(DT.VARIABLES + DT.DEPTHWISE_VARIABLES)
  assert tuple(d_in.shape) == (B, h, w, C) and d_in.dtype == torch.float32
  assert tuple(grads[DT.DEPTHWISE_VARIABLES[0]].shape) == (3, 3, C, 1)
  # the nine shared gradients: net_grads with the four layers
  values9, bad9, grads9 = trainer.net_grads(net, gt, variables, tuple(W.TRAINABLE_LAYERS),
                                            LOSS_WEIGHTS, 'pooled')
  assert same_bytes(values, values9) and same_bytes(bad, bad9)
  for n in DT.VARIABLES:
    assert same_bytes(grads[n], grads9[n]), n
  # the five wrappers, by hand
  logits = HT.net_logits(net)
  sums, counts, _ = L.loss_terms(logits, gt)
  _, scales = L.loss_values(sums, counts, LOSS_WEIGHTS, 'pooled')
  G = HT.heads_input_grad(logits, gt, scales, variables, relu_of=net.decoder_out)
  mean, var = net.layer_constants()
  wl, gamma = variables[DT.LAYER + '/weights'], variables[DT.LAYER + '/BatchNorm/gamma']
  layer = DT.pointwise_weight_grads(op['a'], G, wl, bn=(gamma, mean, var), eps=op['eps'],
                                    a_h2=op['a_h2'])
  for short, t in layer.items():
    assert same_bytes(grads[DT.LAYER + '/' + short], t), short
  D = DT.pointwise_input_grad(G, wl, bn=(gamma, var), eps=op['eps'], relu_of=op['a'],
                              relu_of_h2=presplit)
  assert tuple(D.shape) == (M, 256)
  x = dw['x'][..., :C]
  dvars = [torch.from_numpy(np.ascontiguousarray(ckpt[n])).cuda()
           for n in DT.DEPTHWISE_VARIABLES[:2] + DT.DEPTHWISE_CONSTANTS]
  D4 = D.view(B, h, w, C)
  dwg = DT.depthwise_weight_grads(x, D4, dvars[0], tuple(dvars[1:]), dw['eps'], rate=dw['rate'])
  for short, t in dwg.items():
    assert same_bytes(grads[DT.DEPTHWISE_LAYER + '/' + short], t), short
  d_hand = DT.depthwise_input_grad(D4, dw['w9c'], rate=dw['rate'], relu_of=x)
  assert same_bytes(d_in, d_hand)
  # outputs the caller gives are written in place, padding columns kept
  wide = torch.full((M, 260), 7.0, device='cuda')
  assert DT.pointwise_input_grad(G, wl, bn=(gamma, var), eps=op['eps'], relu_of=op['a'],
                                 relu_of_h2=presplit, out=wide[:, :256]).data_ptr() == \
      wide.data_ptr()
  assert same_bytes(wide[:, :256], D) and (wide[:, 256:] == 7.0).all()
  # ---- the kernels' bounds on the device's own inputs
  Gh, Dh = G.cpu().numpy(), D.cpu().numpy()
  Wf = ref.fold(ckpt[DT.LAYER + '/weights'].reshape(256, 256), ckpt[DT.LAYER + '/BatchNorm/gamma'],
                ckpt[DT.LAYER + '/BatchNorm/moving_variance'], op['eps'])
  mask = mask_values(op)
  assert mask.min() >= 0 and 0.05 < (mask > 0).mean() < 0.95      # behind the depthwise ReLU
  want, absum = ref.pointwise_dgrad(Gh, Wf, mask)
  ok, worst = wref.within(Dh, want, ref.bound_pointwise_dgrad(256, want, absum))
  print('D (presplit=%s): worst error / bound = %.3g' % (presplit, worst))
  assert ok and np.abs(Dh).max() > 0 and not Dh.view(np.uint32)[mask <= 0].any()
  xh = x.cpu().numpy()
  T, t, aT, at = ref.depthwise_wgrad(xh, Dh.reshape(B, h, w, C), 1)
  w9 = ckpt[DT.DEPTHWISE_VARIABLES[0]].reshape(9, C)
  bn = [ckpt[n] for n in (DT.DEPTHWISE_VARIABLES[1],) + DT.DEPTHWISE_CONSTANTS]
  wantg = wref.close(T, t, w9, *bn, eps=dw['eps'])
  tol = wref.bounds_close(M, T, t, aT, at, w9, *bn, eps=dw['eps'])
  for short, wv, tv in zip(W.DEPTHWISE_VARIABLES, wantg, tol):
    got = dwg[short].cpu().numpy().reshape(wv.shape)
    ok, worst = wref.within(got, wv, tv)
    print('%s (presplit=%s): worst error / bound = %.3g' % (short, presplit, worst))
    assert ok and np.abs(got).max() > 0, (short, worst)
  w9c = dw['w9c'].cpu().numpy()
  bits = ref.depthwise_dgrad(Dh.reshape(B, h, w, C), w9c, 1, Y=xh)
  assert np.array_equal(d_in.cpu().numpy().view(np.uint32), bits.view(np.uint32))
  assert np.abs(bits).max() > 0 and not bits.view(np.uint32)[xh <= 0].any()
  return d_in


def test_depthwise_operand_reproduces_the_nets_own_a(small_net):
  """x, w9c and bias of the operand, pushed through an fp64 host depthwise + ReLU, against the A
  the net's buffer holds (fp16 pairs at the plan's own scale), to the project's parity tolerance."""
  net, ckpt = small_net[0], small_net[1]
  from epos_amd import decoder_train as DT
  op, dw = net.pointwise_operand(), net.depthwise_operand()
  assert sorted(dw) == sorted(['x', 'ldx', 'b', 'h', 'w', 'c', 'rate', 'w9c', 'bias', 'eps'])
  x = dw['x'][..., :dw['c']].cpu().numpy()
  assert x.min() >= 0 and x.max() > 0                                  # behind conv0's ReLU
  fwd = ref.depthwise_forward(x, dw['w9c'].cpu().numpy(), dw['bias'].cpu().numpy(), dw['rate'])
  raw = op['a'].cpu().numpy().reshape(op['m'], op['lda'])
  assert op['presplit']
  slot, slot2, gain, bias = op['a_h2']
  words = [None if s is None else s.cpu().numpy().view(np.uint32) for s in (slot, slot2)]
  A = wref.h2_values(raw, op['k'], wref.h2_scale(wref.slot_bound(words[0], words[1], gain,
                                                                bias))[1])
  assert np.allclose(A, fwd.reshape(op['m'], op['k']), rtol=1e-4, atol=1e-4)
  assert A.max() > 0.1
  # w9c is the checkpoint's fold
  scale = (ckpt[DT.DEPTHWISE_VARIABLES[1]].astype(np.float64) / np.sqrt(
      ckpt[DT.DEPTHWISE_CONSTANTS[1]].astype(np.float64) + dw['eps'])).astype(np.float32)
  w9c = ckpt[DT.DEPTHWISE_VARIABLES[0]].reshape(9, -1) * scale[None, :]
  assert np.array_equal(dw['w9c'].cpu().numpy(), w9c.astype(np.float32))
  with pytest.raises(ValueError, match='decoder_conv0_depthwise'):
    net.depthwise_operand('decoder/decoder_conv0_depthwise')


def test_decoder_conv1_grads_equal_their_parts_and_the_chain_continues(small_net):
  net, ckpt, mo, c, gt = small_net
  from epos_amd import decoder_train as DT
  d_in = check_chain(net, ckpt, gt, presplit=True)
  # the variables of the depthwise layer are taken from `variables` where given
  from epos_amd import trainer
  variables = variables_of(ckpt)
  name = DT.DEPTHWISE_VARIABLES[1]
  variables[name] = torch.from_numpy(2 * ckpt[name]).cuda()
  grads2 = trainer.decoder_conv1_grads(net, gt, variables, LOSS_WEIGHTS)[2]
  grads1 = trainer.decoder_conv1_grads(net, gt, variables_of(ckpt), LOSS_WEIGHTS)[2]
  assert not same_bytes(grads1[DT.DEPTHWISE_VARIABLES[0]], grads2[DT.DEPTHWISE_VARIABLES[0]])
  assert same_bytes(grads1[DT.DEPTHWISE_VARIABLES[2]], grads2[DT.DEPTHWISE_VARIABLES[2]])
  # the chain continues: d_in is the G of decoder_conv0_pointwise for the existing wrapper
  scope = 'decoder/decoder_conv0_pointwise'
  B, h, w, C = d_in.shape
  # its operand: decoder_conv0_depthwise of the decoder's concat buffer, on the host
  dscope = 'decoder/decoder_conv0_depthwise'
  bn_ = {v: ckpt[dscope + '/BatchNorm/' + v].astype(np.float64)
         for v in ('gamma', 'beta', 'moving_mean', 'moving_variance')}
  sc = bn_['gamma'] / np.sqrt(bn_['moving_variance'] + 1e-5)
  cat = net.decoder_concat.cpu().numpy()
  assert cat.shape == (B, h, w, 304)
  a0 = ref.depthwise_forward(cat, ckpt[dscope + '/depthwise_weights'].reshape(9, 304) * sc,
                             bn_['beta'] - bn_['moving_mean'] * sc, 1)
  a0 = torch.from_numpy(a0.reshape(-1, 304).astype(np.float32)).cuda()
  assert torch.isfinite(a0).all() and a0.max() > 0
  w0 = torch.from_numpy(ckpt[scope + '/weights'].reshape(304, 256)).cuda()
  bn0 = tuple(torch.from_numpy(np.ascontiguousarray(ckpt[scope + '/BatchNorm/' + v])).cuda()
              for v in ('gamma', 'moving_mean', 'moving_variance'))
  out = DT.pointwise_weight_grads(a0, d_in.view(-1, C), w0, bn=bn0, eps=1e-5)
  torch.cuda.synchronize()
  for short, t in out.items():
    assert torch.isfinite(t).all() and t.abs().max() > 0, short


def test_the_chain_copies_nothing_from_the_host_and_does_not_synchronise(small_net):
  """The depthwise layer's variables are uploaded once and kept on the net; with them, or with
  device tensors in `variables`, the chain enqueues only: torch's synchronisation check stays
  silent through a whole call."""
  net, ckpt, mo, c, gt = small_net
  from epos_amd import decoder_train as DT, trainer
  consts = net.depthwise_constants()
  assert all(a is b for a, b in zip(consts, net.depthwise_constants())) and len(consts) == 4
  for t, n in zip(consts, DT.DEPTHWISE_VARIABLES[:2] + DT.DEPTHWISE_CONSTANTS):
    assert t.is_cuda and t.dtype == torch.float32
    assert np.array_equal(t.cpu().numpy(), ckpt[n])
  w, bn = DT._depthwise_inputs(net, {})
  assert w is consts[0] and all(a is b for a, b in zip(bn, consts[1:]))
  variables = variables_of(ckpt)
  given = torch.from_numpy(2 * ckpt[DT.DEPTHWISE_VARIABLES[1]]).cuda()
  w, bn = DT._depthwise_inputs(net, dict(variables, **{DT.DEPTHWISE_VARIABLES[1]: given}))
  assert w is consts[0] and bn[0] is given and bn[1] is consts[2] and bn[2] is consts[3]
  with pytest.raises(ValueError, match='decoder_conv0_depthwise'):
    net.depthwise_constants('decoder/decoder_conv0_depthwise')
  want = trainer.decoder_conv1_grads(net, gt, variables, LOSS_WEIGHTS)
  torch.cuda.synchronize()
  torch.cuda.set_sync_debug_mode('error')
  try:
    got = trainer.decoder_conv1_grads(net, gt, variables, LOSS_WEIGHTS)
  finally:
    torch.cuda.set_sync_debug_mode('default')
  torch.cuda.synchronize()
  assert same_bytes(want[3], got[3])
  for n in want[2]:
    assert same_bytes(want[2][n], got[2][n]), n


def test_the_fp32_mask_route_in_a_child_process():
  """EPOS_H2_PRESPLIT=0 is read when the library's plan is built: a child process builds the same
  net with an fp32 A and runs the same checks."""
  env = dict(os.environ, EPOS_H2_PRESPLIT='0')
  done = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT,
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
  text = done.stdout.decode('utf-8', 'replace')
  assert done.returncode == 0 and 'fp32 mask: OK' in text, text[-3000:]


def test_python_argument_checks():
  from epos_amd import decoder_train as DT
  z = lambda *s: torch.zeros(*s, device='cuda')                            # noqa: E731
  g, wl, bn = z(10, 4), z(8, 4), (z(4) + 1, z(4) + 1)
  assert tuple(DT.pointwise_input_grad(g, wl, bn=bn).shape) == (10, 8)
  assert tuple(DT.pointwise_input_grad(g, wl.view(1, 1, 8, 4), relu_of=z(10, 8)).shape) == (10, 8)
  for kwargs, exc in ((dict(g=g.double()), TypeError), (dict(g=g.cpu()), DT.EposError),
                      (dict(weights=z(8, 5)), ValueError), (dict(weights=z(4, 8).t()), ValueError),
                      (dict(bn=bn + bn[:1]), ValueError), (dict(bn=(bn[0][:3], bn[1])), ValueError),
                      (dict(relu_of=z(10, 7)), ValueError), (dict(relu_of=z(9, 8)), ValueError),
                      (dict(out=z(10, 7)), ValueError), (dict(out=z(9, 8)), ValueError),
                      (dict(workspace=z(3).double()), ValueError)):
    args = dict(g=g, weights=wl, bn=bn)
    args.update(kwargs)
    with pytest.raises(exc):
      DT.pointwise_input_grad(**args)
  x, d, w9 = z(2, 3, 5, 8), z(2, 3, 5, 8), z(3, 3, 8, 1)
  bn3 = (z(8) + 1, z(8), z(8) + 1)
  out = DT.depthwise_weight_grads(x, d, w9, bn3, 1e-5, rate=2)
  assert sorted(out) == ['BatchNorm/beta', 'BatchNorm/gamma', 'depthwise_weights']
  assert tuple(out['depthwise_weights'].shape) == (3, 3, 8, 1)
  assert tuple(DT.depthwise_input_grad(d, z(9, 8), relu_of=x).shape) == (2, 3, 5, 8)
  for kwargs, exc in ((dict(x=x.double()), TypeError), (dict(d=z(2, 3, 4, 8)), ValueError),
                      (dict(x=z(30, 8)), ValueError), (dict(depthwise_weights=z(9, 8)), ValueError),
                      (dict(bn=bn3[:2]), ValueError), (dict(rate=0), DT.EposError),
                      (dict(out={'BatchNorm/beta': z(7)}), ValueError)):
    args = dict(x=x, d=d, depthwise_weights=w9, bn=bn3, eps=1e-5)
    args.update(kwargs)
    with pytest.raises(exc):
      DT.depthwise_weight_grads(**args)
  for kwargs, exc in ((dict(d=z(30, 8)), ValueError), (dict(w9c=z(9, 4)), ValueError),
                      (dict(relu_of=z(2, 3, 5, 4)), ValueError), (dict(out=z(2, 3, 4, 8)), ValueError),
                      (dict(rate=0), DT.EposError)):
    args = dict(d=d, w9c=z(9, 8))
    args.update(kwargs)
    with pytest.raises(exc):
      DT.depthwise_input_grad(**args)


if __name__ == '__main__':                    # the child of the fp32-mask test
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
  check_chain(net_, ckpt_, gt_tensors(case_, net_.out_h, net_.out_w), presplit=False)
  print('fp32 mask: OK')
