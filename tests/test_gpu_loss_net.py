"""EposNet.forward_logits: the raw logits of the dense plan, against forward()'s probabilities
and labels; forward() itself unchanged by it; eager and graph runs identical."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

H, W, O, F = 96, 128, 3, 64


@pytest.fixture(scope='module')
def net():
  from epos_amd import model, weights
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), crop_size=(W, H))
  return model.get_net(ckpt, 2, H, W, O, F, mo, 'cuda:0')


@pytest.fixture(scope='module')
def images():
  from epos_amd import synthetic
  return np.stack([synthetic.image(i, H, W) for i in range(2)]).astype(np.float32)


def _host(d):
  torch.cuda.synchronize()
  return {k: v.cpu().numpy().copy() for k, v in d.items()}


def test_forward_logits_against_forward(net, images):
  before = _host(net.forward(images))
  logits = net.forward_logits(images)
  assert sorted(logits) == ['pred_frag_conf', 'pred_frag_loc', 'pred_obj_conf']
  h, w = H // 4, W // 4
  assert logits['pred_obj_conf'].shape == (2, h, w, O + 1)
  assert logits['pred_frag_conf'].shape == (2, h, w, O, F)
  assert logits['pred_frag_loc'].shape == (2, h, w, O, F, 3)
  # views of the head buffers, as forward()'s outputs are
  assert logits['pred_frag_conf'].data_ptr() == net.outputs()['pred_frag_conf'].data_ptr()
  raw = _host(logits)
  # raw logits: not rows that sum to 1
  assert np.abs(raw['pred_obj_conf'].sum(-1) - 1).max() > 1e-3
  assert np.abs(raw['pred_frag_conf'].sum(-1) - 1).max() > 1e-3
  # torch's softmax / argmax on them: forward()'s labels exactly, its confidences to the bound
  # of the softmax kernel's own tests (rtol 2e-6, atol 1e-7 against fp64)
  obj = torch.softmax(torch.from_numpy(raw['pred_obj_conf']).double(), dim=-1)
  frag = torch.softmax(torch.from_numpy(raw['pred_frag_conf']).double(), dim=-1)
  label = torch.argmax(torch.from_numpy(raw['pred_obj_conf']), dim=-1).numpy()
  assert (label == before['pred_obj_label']).all()
  assert len(np.unique(label)) > 1
  np.testing.assert_allclose(before['pred_obj_conf'], obj.numpy(), rtol=2e-6, atol=1e-7)
  np.testing.assert_allclose(before['pred_frag_conf'], frag.numpy(), rtol=2e-6, atol=1e-7)
  assert raw['pred_frag_loc'].tobytes() == before['pred_frag_loc'].tobytes()
  # forward() after forward_logits(): the bytes it returned before, eager and from its graph
  for use_graph in (False, True):
    net.forward_logits(images, use_graph=use_graph)
    after = _host(net.forward(images, use_graph=use_graph))
    assert sorted(after) == sorted(before)
    for k in before:
      assert after[k].tobytes() == before[k].tobytes(), (k, use_graph)


def test_logits_with_and_without_graph_are_identical(net, images):
  eager = _host(net.forward_logits(images))
  graph = _host(net.forward_logits(images, use_graph=True))
  again = _host(net.forward_logits(images, use_graph=True))
  for k in eager:
    assert graph[k].tobytes() == eager[k].tobytes(), k
    assert again[k].tobytes() == eager[k].tobytes(), k
  assert net._graph_logits is not None and net._graph_logits is not net._graph
