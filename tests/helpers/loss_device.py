"""What the GPU tests of the loss family share (test_gpu_loss.py, test_gpu_loss_grad.py,
test_gpu_heads_wgrad.py, test_gpu_heads_dgrad.py, test_gpu_head_update.py): pointers and the
library, device buffers at a chosen offset behind a 16-byte boundary, the constants, host cases
as device tensors, the raw epos_loss_grads call the weight and input gradients are compared
with, and a small real net."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import loss_cases, loss_ref

IGNORE = loss_cases.IGNORE
SENTINEL = 0x7FA55A5A                      # a NaN no kernel produces
WEIGHTS = (0.7, 1.3, 100.0)
UPSTREAM = [0.3, -1.0, 2.0, 0.5]
MEAN, POOLED = 0, 1
KEYS = ('pred_obj_conf', 'pred_frag_conf', 'pred_frag_loc')


def _p(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
  from epos_amd import _lib as binding
  return binding.load()


def _off(a, offset, dtype=torch.float32):
  """The array on the device, `offset` elements behind a 16-byte boundary."""
  a = np.ascontiguousarray(a).reshape(-1)
  flat = torch.empty(a.size + offset, dtype=dtype, device='cuda')
  assert flat.data_ptr() % 16 == 0
  view = flat[offset:]
  view.copy_(torch.from_numpy(a))
  return view


def _out(numel, offset, sentinel=SENTINEL):
  """A sentinel-filled output of `numel` floats, `offset` floats behind a 16-byte boundary."""
  flat = torch.full((numel + offset,), sentinel, dtype=torch.int32, device='cuda')
  assert flat.data_ptr() % 16 == 0
  return flat[offset:].view(torch.float32)


def ref_counts(c, ignore=IGNORE):
  return loss_cases.ref_terms(loss_ref, c, 64, ignore)[1]


def gt_tensors(c, h, w):
  B = c['gt_obj'].shape[0]
  return {'obj_label': torch.from_numpy(c['gt_obj']).cuda().view(B, h, w),
          'frag_label': torch.from_numpy(c['gt_frag']).cuda().view(B, h, w),
          'frag_loc': torch.from_numpy(c['gt_loc']).cuda().view(B, h, w, 3),
          'frag_weight': torch.from_numpy(c['gt_weight']).cuda().view(B, h, w)}


def tensors(c, h, w):
  """(logits, gt) of a host case as loss.loss_terms takes them, images of h x w pixels."""
  B = c['gt_obj'].shape[0]
  O, F = c['frag_logits'].shape[2:4]
  logits = {'pred_obj_conf': torch.from_numpy(c['obj_logits']).cuda().view(B, h, w, O + 1),
            'pred_frag_conf': torch.from_numpy(c['frag_logits']).cuda().view(B, h, w, O, F),
            'pred_frag_loc': torch.from_numpy(c['frag_loc']).cuda().view(B, h, w, O, F, 3)}
  return logits, gt_tensors(c, h, w)


def logit_grads(dev):
  """epos_loss_grads on the buffers of a test's Device (obj with row stride ld_obj, frag, loc,
  g_obj, g_frag, g_loc, g_w, sc, up): the three dense gradients, flat f32 tensors."""
  lib = _lib()
  B, P, O, F = dev.B, dev.P, dev.O, dev.F
  d = [torch.empty(B * P * n, dtype=torch.float32, device='cuda')
       for n in (O + 1, O * F, O * F * 3)]
  rc = lib.epos_loss_grads(_p(dev.obj), dev.ld_obj, _p(dev.frag), _p(dev.loc), _p(dev.g_obj),
                           _p(dev.g_frag), _p(dev.g_loc), _p(dev.g_w), B, P, O, F, dev.ignore,
                           _p(dev.sc), _p(dev.up), _p(d[0]), O + 1, _p(d[1]), _p(d[2]), _stream())
  assert rc == 0, lib.epos_last_error()
  return d


NET_H, NET_W, NET_O, NET_F, NET_B = 96, 128, 3, 8, 2


@pytest.fixture(scope='module')
def small_net():
  """xception_65 at a 128 x 96 crop (the net of test_gpu_loss_net.py), 3 objects x 8
  fragments, after one forward_logits; with labels of a seeded case on its 24 x 32 heads:
  (net, checkpoint, model options, host case, gt tensors)."""
  from epos_amd import model, synthetic, weights
  ckpt = weights.random_init('xception_65', num_objs=NET_O, num_frags=NET_F, seed=5,
                             randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(NET_O, NET_F),
                          crop_size=(NET_W, NET_H))
  net = model.get_net(ckpt, NET_B, NET_H, NET_W, NET_O, NET_F, mo, 'cuda:0')
  imgs = np.stack([synthetic.image(i, NET_H, NET_W) for i in range(NET_B)]).astype(np.float32)
  net.forward_logits(imgs)
  torch.cuda.synchronize()
  h, w = net.out_h, net.out_w
  c = loss_cases.make_case(NET_B, h * w, NET_O, NET_F, seed=33)
  yield net, ckpt, mo, c, gt_tensors(c, h, w)
  model._NETS.clear()


def net_logits(net):
  """The small net's logits as loss.loss_terms takes them, by hand."""
  B, h, w = NET_B, net.out_h, net.out_w
  return {'pred_obj_conf': net.logits['pred_obj_conf'],
          'pred_frag_conf': net.logits['pred_frag_conf'].view(B, h, w, NET_O, NET_F),
          'pred_frag_loc': net.logits['pred_frag_loc'].view(B, h, w, NET_O, NET_F, 3)}
