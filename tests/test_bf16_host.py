"""bf16 inference mode (EposNet(precision='bf16')), the CPU side: the plan's structure, its
buffer dtypes and bytes, the bf16 weight packer, and the precision option through get_net and
infer.py."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

from helpers.bf16_ref import bf16_round_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'graph_*.json')) +
                glob.glob(os.path.join(ROOT, 'tests', 'golden', 'variant_graph_*.json')) +
                glob.glob(os.path.join(ROOT, 'tests', 'golden', 'f256_graph_*.json')))
IDS = [os.path.basename(p)[:-5] for p in GOLDEN]


def _load(path):
  with open(path) as f:
    return json.load(f)


def _ckpt(cfg):
  from epos_amd import weights
  return weights.random_init(num_objs=cfg['num_objs'], num_frags=cfg['num_frags'], seed=0,
                             model_variant=cfg['model_variant'])


def _plan(cfg, ckpt, precision):
  from epos_amd import net
  return net.EposNet(ckpt, 1, cfg['height'], cfg['width'], cfg['num_objs'],
                     cfg['num_frags'], model_variant=cfg['model_variant'],
                     multi_grid=cfg['multi_grid'], atrous_rates=tuple(cfg['atrous_rates']),
                     dry_run=True, precision=precision)


def test_fixtures_found():
  assert len(GOLDEN) >= 12, IDS


@pytest.mark.parametrize('path', GOLDEN, ids=IDS)
def test_bf16_plan_builds_the_reference_graph(path):
  g = _load(path)
  cfg = g['config']
  ckpt = _ckpt(cfg)
  plan = _plan(cfg, ckpt, 'bf16')
  # the golden list in the reference's order, the plan's in launch order (fused groups)
  key = lambda ls: {l['scope']: l for l in ls}
  assert key(plan.trace_layers) == key(g['layers'])
  assert len(plan.trace_layers) == len(g['layers'])
  assert plan.trace_outputs == g['outputs']
  ref = _plan(cfg, ckpt, 'fp32')
  assert plan.trace_layers == ref.trace_layers
  assert plan.trace_outputs == ref.trace_outputs
  launched = '+'.join(n for n, _ in plan.ops)
  for l in g['layers']:
    assert l['scope'] in launched, l['scope']


def _act_bytes(plan):
  """bytes of the activation buffers: everything the plan allocated except the weights
  (dry run: 1-element stand-ins), the logits, the im2col matrices and the int64 labels"""
  skip = {id(t) for t in plan.logits.values()} | plan._col_ids | {id(plan.obj_label)}
  return sum(t.numel() * t.element_size() for t in plan._keep
             if id(t) not in skip and t.numel() > 1)


def test_bf16_c2_activations_are_bf16_and_half_the_bytes():
  from epos_amd import weights
  cfg = _load(os.path.join(ROOT, 'tests', 'golden', 'graph_c2_xception65_640x480_o21.json'))['config']
  ckpt = _ckpt(cfg)
  bf, fp = _plan(cfg, ckpt, 'bf16'), _plan(cfg, ckpt, 'fp32')
  assert bf.decoder_out.dtype == torch.bfloat16 and bf.encoder.dtype == torch.bfloat16
  assert bf.aspp_concat.dtype == torch.bfloat16 and bf.concat_projection.dtype == torch.bfloat16
  for t in bf.logits.values():
    assert t.dtype == torch.float32
  assert bf.obj_label.dtype == torch.int64
  assert bf.images.dtype == torch.float32
  big = [t for t in bf._keep if t.dim() == 4 and id(t) not in {id(x) for x in bf.logits.values()}
         and t is not bf.images]
  assert big and all(t.dtype == torch.bfloat16 for t in big)
  # 728-channel rows start on 128-byte lines: 768 bf16 elements
  assert any(t.shape[-1] == 768 for t in big) and not any(t.shape[-1] == 736 for t in big)
  ratio = _act_bytes(bf) / _act_bytes(fp)
  assert ratio <= 0.55, ratio
  # one shared im2col scratch in the bf16 plan
  assert len([t for t in bf._keep if id(t) in bf._col_ids]) == 1
  # algorithmic bytes: 2 B per bf16 element, heads 4 B
  assert 0.5 < bf.algorithmic_bytes() / fp.algorithmic_bytes() < 0.65


def test_bf16_plan_has_no_absmax_machinery():
  cfg = _load(os.path.join(ROOT, 'tests', 'golden', 'graph_c2_xception65_640x480_o21.json'))['config']
  bf = _plan(cfg, _ckpt(cfg), 'bf16')
  names = [n for n, _ in bf.ops]
  assert 'amax_clear' not in names and not any('absmax' in n for n in names)
  assert bf._n_slots == 0 and not bf.h2_layers


@pytest.mark.parametrize('bad', ['fp16', 'BF16', 'float32', None, 16])
def test_unknown_precision_raises(bad):
  from epos_amd import net, weights
  ckpt = weights.random_init(num_objs=1, seed=0)
  with pytest.raises(ValueError):
    net.EposNet(ckpt, 1, 64, 64, 1, dry_run=True, precision=bad)


def _pack(lib, w):
  k, n = w.shape
  total = lib.epos_pack_pointwise_weights_bf16(None, k, n, None)
  dst = np.full(total, 0xBEEF, np.uint16)
  w = np.ascontiguousarray(w, np.float32)
  assert lib.epos_pack_pointwise_weights_bf16(w.ctypes.data_as(ctypes.c_void_p), k, n,
                                              dst.ctypes.data_as(ctypes.c_void_p)) == total
  return dst


@pytest.mark.parametrize('k,n', [(8, 5), (27, 64), (32, 130), (152, 64), (304, 256),
                                 (728, 728), (1, 1)])
def test_pack_bf16_matches_numpy_rne(k, n):
  from epos_amd import _lib
  lib = _lib.load()
  rng = np.random.default_rng(k * 1000 + n)
  w = rng.standard_normal((k, n)).astype(np.float32) * np.float32(0.1)
  special = np.array([
      0.0, -0.0, 1.0, -1.0,
      np.float32(1 + 2 ** -8), np.float32(1 + 3 * 2 ** -8),       # ties: to even (down, up)
      np.float32(-(1 + 2 ** -8)), np.float32(1 + 2 ** -8 + 2 ** -20),
      np.float32(2 ** -130), np.float32(-2 ** -140), np.float32(1e-45),   # subnormals
      np.float32(3.3e38), np.float32(-3.4e38), np.float32(65504.0)],   # huge (-> inf on overflow)
      np.float32)
  flat = w.reshape(-1)
  flat[:min(len(special), flat.size)] = special[:flat.size]
  dst = _pack(lib, w)
  k32, npad = (k + 31) // 32 * 32, (n + 127) // 128 * 128
  assert dst.size == k32 * npad
  want = np.zeros((k32, npad), np.uint16)
  want[:k, :n] = bf16_round_bits(w)
  got = dst.reshape(k32 // 8, npad, 8).transpose(0, 2, 1).reshape(k32, npad)
  np.testing.assert_array_equal(got, want)


def test_numpy_rne_reference_itself():
  x = np.array([1 + 2 ** -8, 1 + 3 * 2 ** -8, 3.4e38, np.inf, -0.0, 2 ** -135],
               np.float32)
  b = bf16_round_bits(x)
  assert b[0] == 0x3F80 and b[1] == 0x3F82          # ties to even
  assert b[2] == 0x7F80 and b[3] == 0x7F80          # 3.4e38 rounds up to inf
  assert b[4] == 0x8000 and b[5] == 0x0000          # 2^-135: below half the least subnormal (2^-133)


def test_get_net_caches_precisions_separately(monkeypatch):
  from epos_amd import model, net, weights
  made = []

  class Fake(object):
    def __init__(self, *a, **kw):
      made.append(kw.get('precision'))
  monkeypatch.setattr(net, 'EposNet', Fake)
  monkeypatch.setattr(model, '_NETS', {})
  ckpt = weights.random_init(num_objs=1, seed=0)
  a = model.get_net(ckpt, 1, 64, 64, 1, 64)
  b = model.get_net(ckpt, 1, 64, 64, 1, 64, precision='bf16')
  c = model.get_net(ckpt, 1, 64, 64, 1, 64, precision='fp32')
  d = model.get_net(ckpt, 1, 64, 64, 1, 64, precision='bf16')
  assert a is c and b is d and a is not b
  assert made == ['fp32', 'bf16']


def test_infer_precision_flag():
  import infer
  ap = infer.build_parser()
  assert ap.parse_args(['--model', 'm']).precision == 'fp32'
  assert ap.parse_args(['--model', 'm', '--precision', 'bf16']).precision == 'bf16'
  with pytest.raises(SystemExit):
    ap.parse_args(['--model', 'm', '--precision', 'fp16'])
