"""The bf16 plan (EposNet(precision='bf16')) on the GPU: against the fp32 plan at full C2 size
on the checkpoints of test_gpu_configs.py (label agreement, softmax within 2e-3, SURVEY.md
section 8(d)), every backbone at reduced size against an emulated-bf16 float64 oracle
(tests/helpers/net_ref_bf16.py), 256 fragments, graph replay, batching, sparse
heads, uint8 input, the explicit fp32 default, the pipeline against the oracle chain fed with
the bf16 heads, and infer.py --precision bf16."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ['xception_65', 'xception_41', 'xception_71', 'resnet_v1_101_beta',
            'resnet_v1_50_beta', 'resnet_v1_50', 'resnet_v1_101']
HEADS = ['pred_obj_conf', 'pred_frag_conf', 'pred_frag_loc']


def _net(ckpt, B, H, W_, O, F, precision, variant='xception_65'):
  from epos_amd import net
  return net.EposNet(ckpt, B, H, W_, O, F, model_variant=variant, precision=precision)


def _run(n, img, **kw):
  out = n.forward(torch.from_numpy(img).cuda() if isinstance(img, np.ndarray) else img, **kw)
  torch.cuda.synchronize()
  return {k: v.cpu().numpy() for k, v in out.items()}


def _logits(n):
  return {k: n.logits[k].cpu().numpy() for k in n.logits}


def _rel_rms(a, b):
  a, b = a.astype(np.float64), b.astype(np.float64)
  return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


@pytest.mark.parametrize('tails', ['init', 'heavy_tailed'])
def test_c2_bf16_against_fp32(tails):
  from epos_amd import synthetic, weights
  O, F, H, W_ = 21, 64, 480, 640
  ckpt = weights.random_init(num_objs=O, seed=0, randomize_bn=True, logits_std=0.2)
  if tails == 'heavy_tailed':
    ckpt = weights.heavy_tailed(ckpt, seed=0)
  img = synthetic.image(0, H, W_)[None]
  fp = _net(ckpt, 1, H, W_, O, F, 'fp32')
  ref = _run(fp, img)
  del fp
  torch.cuda.empty_cache()
  bf = _net(ckpt, 1, H, W_, O, F, 'bf16')
  got = _run(bf, img)
  assert bf.decoder_out.dtype == torch.bfloat16
  for k in HEADS:
    assert got[k].dtype == np.float32 and got[k].shape == ref[k].shape, k
    assert np.isfinite(got[k]).all(), k
  assert got['pred_obj_label'].dtype == np.int64
  agree = float((got['pred_obj_label'] == ref['pred_obj_label']).mean())
  d_obj = float(np.abs(got['pred_obj_conf'] - ref['pred_obj_conf']).max())
  d_frag = float(np.abs(got['pred_frag_conf'] - ref['pred_frag_conf']).max())
  loc = _rel_rms(got['pred_frag_loc'], ref['pred_frag_loc'])
  print('\nC2 %s bf16 vs fp32: label agreement %.5f, max|d obj softmax| %.2e, '
        'max|d frag softmax| %.2e, rel rms frag_loc %.3e' % (tails, agree, d_obj, d_frag, loc))
  assert agree >= 0.999, agree
  assert d_obj <= 2e-3, d_obj
  assert d_frag <= 2e-3, d_frag


def _rms(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return float(np.sqrt(np.mean((a - b) ** 2)))


@pytest.mark.parametrize('variant', VARIANTS)
def test_every_backbone_against_emulated_bf16_oracle(variant):
  """Each backbone at reduced size against the float64 oracle: for each head and for the
  decoder output, rms(GPU bf16 - fp64) <= 1.5 x rms(emulated bf16 - fp64), where the emulation
  (tests/helpers/net_ref_bf16.py) rounds at the plan's storage points and uses its bf16
  weights. A rounding point too many or too few, a lost bias or a mis-wired layer moves the GPU
  result away from the emulation's error level."""
  from helpers import net_ref_bf16 as nb
  from helpers import net_ref_variants as nv
  from oracle import net_ref
  from epos_amd import synthetic, weights
  O, F, H, W_ = 2, 8, 96, 128
  ckpt = weights.random_init(variant, num_objs=O, num_frags=F, seed=4, randomize_bn=True)
  img = synthetic.image(1, H, W_)[None]
  with net_ref.precision(torch.float64):
    ref = nv.predict(img, ckpt, num_objs=O, num_frags=F, model_variant=variant)
    with nb.emulate_bf16():
      emu = nv.predict(img, nb.bf16_checkpoint(ckpt), num_objs=O, num_frags=F,
                       model_variant=variant)
  bf = _net(ckpt, 1, H, W_, O, F, 'bf16', variant)
  bf.set_images(torch.from_numpy(img).cuda())
  bf.run_plan(with_post=False)          # the raw logits: no in-place softmax
  torch.cuda.synchronize()
  got = _logits(bf)
  pairs = [(k, got[k], emu['_logits'][k], ref['_logits'][k]) for k in HEADS]
  nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()
  pairs.append(('decoder_out', bf.decoder_out.float().cpu().numpy(),
                nhwc(emu['_end_points']['decoder/decoder_conv1']),
                nhwc(ref['_end_points']['decoder/decoder_conv1'])))
  for name, g, e, r in pairs:
    assert np.isfinite(g).all(), name
    eg, ee = _rms(g, r), _rms(e, r)
    print('\n%s %s: rms(gpu - fp64) %.3e, rms(emulated - fp64) %.3e, ratio %.3f' % (
        variant, name, eg, ee, eg / ee))
    assert ee > 0, name
    assert eg <= 1.5 * ee, (name, eg, ee)


def test_f256_reduced_size():
  from epos_amd import synthetic, weights
  O, F, H, W_ = 2, 256, 96, 128
  ckpt = weights.random_init(num_objs=O, num_frags=F, seed=6, randomize_bn=True)
  img = synthetic.image(2, H, W_)[None]
  fp = _net(ckpt, 1, H, W_, O, F, 'fp32')
  _run(fp, img)
  ref = _logits(fp)
  bf = _net(ckpt, 1, H, W_, O, F, 'bf16')
  out = _run(bf, img)
  assert out['pred_frag_conf'].shape == (1, 24, 32, O, F)
  for k, v in _logits(bf).items():
    assert 0 < _rel_rms(v, ref[k]) <= 5e-2, k


def test_graph_batch_sparse_uint8_and_explicit_fp32():
  from epos_amd import synthetic, weights
  O, F, H, W_ = 4, 64, 96, 128
  ckpt = weights.random_init(num_objs=O, num_frags=F, seed=3, randomize_bn=True)
  imgs = np.stack([synthetic.image(i, H, W_) for i in range(4)])
  b4 = _net(ckpt, 4, H, W_, O, F, 'bf16')
  eager = _run(b4, imgs)
  graph = _run(b4, imgs, use_graph=True)
  for k in eager:
    assert np.array_equal(eager[k], graph[k]), k
  b1 = _net(ckpt, 1, H, W_, O, F, 'bf16')
  for i in (0, 3):
    one = _run(b1, imgs[i:i + 1])
    for k in one:
      assert np.array_equal(one[k][0], eager[k][i]), (k, i)
  # uint8 frames equal float frames of the same values
  u8 = np.round(imgs[:1]).astype(np.uint8)
  a = _run(b1, u8.astype(np.float32))
  b = _run(b1, torch.from_numpy(u8))
  for k in a:
    assert np.array_equal(a[k], b[k]), k
  # sparse heads: the slots' channels equal the dense heads bit for bit
  b1.run_plan()
  torch.cuda.synchronize()
  slots = [(0, 1), (0, 3)]
  sd = torch.tensor(slots, dtype=torch.int32).cuda()
  b1.run_plan(sparse=True)
  from epos_amd import weights as W
  b1.logits[W.PRED_FRAG_CONF].fill_(float('nan'))    # only the sparse launch can fill them
  b1.run_sparse_heads(slots, sd)
  torch.cuda.synchronize()
  conf = b1.logits[W.PRED_FRAG_CONF].view(1, 24, 32, O, F).clone()
  b1.run_plan()     # dense again for the softmax'd reference of the same slots
  torch.cuda.synchronize()
  dconf = b1.logits[W.PRED_FRAG_CONF].view(1, 24, 32, O, F)
  for im, obj in slots:
    assert torch.equal(conf[im, :, :, obj - 1], dconf[im, :, :, obj - 1])
  # explicit precision='fp32' is the default plan, bit for bit
  d = _net(ckpt, 1, H, W_, O, F, 'fp32')
  from epos_amd import net
  e = net.EposNet(ckpt, 1, H, W_, O, F)
  x, y = _run(d, imgs[:1]), _run(e, imgs[:1])
  for k in x:
    assert np.array_equal(x[k], y[k]), k


def _oracle_poses(pipe, store, pred, targets, Ks, seed):
  from oracle import corresp_ref, pnp_ref
  slots, wants = pipe.make_slots(targets)
  exp = []
  for (im, obj_id), want in zip(slots, wants):
    c = corresp_ref.establish_many_to_many(
        pred['pred_obj_conf'][im], pred['pred_frag_conf'][im],
        pred['pred_frag_loc'][im], [obj_id], store.dp_model['obj_ids'],
        store.frag_centers, store.frag_sizes, 0.25, 0.1, 0.5, True)
    if obj_id not in c:
      continue
    s = (seed * 1000003 + im * 1009 + obj_id) & 0x7fffffffffffffff
    rp, _, rs = pnp_ref.find6DPoses(
        c[obj_id]['coord_2d'], c[obj_id]['coord_3d'], Ks[im],
        params=pnp_ref.default_params(max_model_number=want), seed=s, max_k=4)
    if rp is not None:
      for i in range(rp.shape[0] // 3):
        exp.append((im, obj_id, rp[3 * i:3 * i + 3], rs[i]))
  return exp


def test_pipeline_bf16_dense_and_sparse_match_oracle_chain():
  from epos_amd import model, pipeline, synthetic, weights
  O, F, B, H, W_ = 4, 64, 2, 96, 128
  ckpt = weights.random_init(num_objs=O, num_frags=F, seed=8, randomize_bn=True)
  store = synthetic.ModelStore(O, F, seed=0)
  img = np.stack([synthetic.image(i, H, W_) for i in range(B)])
  net0 = model.get_net(ckpt, B, H, W_, O, F, precision='bf16')
  net0.forward(torch.from_numpy(img).cuda())
  torch.cuda.synchronize()
  synthetic.calibrate_logits(ckpt, net0.decoder_out[0].float().cpu().numpy())
  model._NETS.clear()
  Ks = np.tile(np.array([[300., 0, 64], [0, 300., 48], [0, 0, 1]]), (B, 1, 1))
  targets = [{1: 1, 4: 1}, {2: 1}]
  dense = pipeline.EposPipeline(ckpt, B, H, W_, O, F, store, capacity=1 << 16, instance=0,
                                precision='bf16')
  sparse = pipeline.EposPipeline(ckpt, B, H, W_, O, F, store, capacity=1 << 16, instance=1,
                                 sparse_heads=True, precision='bf16')
  assert dense.net.precision == 'bf16' and sparse.net.precision == 'bf16'
  x = torch.from_numpy(img).cuda()
  pd, _ = dense.process_batch(x, Ks, targets, seed=2)
  ps, _ = sparse.process_batch(x, Ks, targets, seed=2)
  assert len(pd) == len(ps) and len(pd) > 0
  for a, b in zip(pd, ps):
    assert a['obj_id'] == b['obj_id'] and a['score'] == b['score']
    assert np.array_equal(a['R'], b['R']) and np.array_equal(a['t'], b['t'])
  pred = {k: v.cpu().numpy() for k, v in dense.net.forward().items()}
  exp = _oracle_poses(dense, store, pred, targets, Ks, 2)
  assert len(pd) == len(exp)
  for p, (im, obj_id, rp, rs) in zip(pd, exp):
    assert (p['im_id'], p['obj_id']) == (im, obj_id)
    np.testing.assert_allclose(np.hstack([p['R'], p['t']]), rp, atol=1e-9)
    np.testing.assert_allclose(p['score'], rs, rtol=1e-12)
  model._NETS.clear()


def test_infer_bf16_synthetic_writes_csv(tmp_path, gpu_children):
  models = tmp_path / 'models'
  (models / 'toy').mkdir(parents=True)
  (models / 'toy' / 'params.yml').write_text('infer_crop_size: "128,96"\n')
  out = subprocess.run(
      ['timeout', '-k', '10', '600', sys.executable, os.path.join(ROOT, 'infer.py'),
       '--model=toy', '--synthetic', '2', '--num_objs', '3', '--precision', 'bf16'],
      env=dict(os.environ, TF_MODELS_PATH=str(models)), capture_output=True, text=True,
      timeout=630)
  assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
  rows = (models / 'toy' / 'infer' / 'estimated-poses.csv').read_text().strip().split('\n')
  assert rows[0].startswith('scene_id')
