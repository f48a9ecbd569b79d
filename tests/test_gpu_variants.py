"""The backbones beyond xception_65 / resnet_v1_101_beta on the GPU: the k x k im2col with fused
preprocessing (epos_im2col_f32) against a float64 numpy restatement, each new variant's network
against the test oracle tests/helpers/net_ref_variants.py at reduced size and two of them at
640x480 with 21 objects, uint8 frames, graph replay, the pipeline (dense and sparse heads)
against the oracle chain, and infer.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['xception_41', 'xception_71', 'resnet_v1_50_beta', 'resnet_v1_50', 'resnet_v1_101']
MEAN_RGB = np.array([123.15, 115.90, 103.06], np.float32)


def _p(t):
  return ctypes.c_void_p(t.data_ptr())


def _im2col_ref(x, C, k, stride, rate, pad, Ho, Wo, ldcol, mode):
  """float64 restatement: preprocess (in float64, from the float32 constants), then zero
  padding; col[m, (ky*k+kx)*C + c]. Returns (col, padded-tap mask)."""
  B, Hi, Wi = x.shape[:3]
  xs = x[..., :C].astype(np.float64)
  if mode == 1:
    xs = (2.0 / 255.0) * xs - 1.0
  elif mode == 2:
    mean = np.zeros(C)
    mean[:min(C, 3)] = MEAN_RGB[:min(C, 3)].astype(np.float64)
    xs = xs - mean
  col = np.zeros((B, Ho, Wo, ldcol))
  padded = np.zeros((B, Ho, Wo, ldcol), bool)
  yo, xo = np.arange(Ho), np.arange(Wo)
  for ky in range(k):
    for kx in range(k):
      yi = yo * stride - pad + ky * rate
      xi = xo * stride - pad + kx * rate
      vy, vx = (yi >= 0) & (yi < Hi), (xi >= 0) & (xi < Wi)
      sl = slice((ky * k + kx) * C, (ky * k + kx + 1) * C)
      g = xs[:, np.clip(yi, 0, Hi - 1)][:, :, np.clip(xi, 0, Wi - 1)]
      ok = (vy[:, None] & vx[None, :])[None, :, :, None]
      col[..., sl] = np.where(ok, g, 0.0)
      padded[..., sl] = ~ok
  return col.reshape(B * Ho * Wo, ldcol), padded.reshape(B * Ho * Wo, ldcol)


CASES = [  # (k, stride, rate, B, Hi, Wi, C, ldx)
    (7, 2, 1, 3, 23, 31, 3, 3),
    (7, 2, 1, 2, 9, 7, 3, 5),        # images smaller than twice the kernel: every tap borders
    (3, 1, 1, 3, 11, 13, 5, 8),
    (3, 2, 1, 3, 15, 17, 3, 3),
    (3, 2, 2, 1, 13, 11, 4, 4),
    (5, 1, 1, 2, 7, 9, 3, 4),
]


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('case', CASES, ids=['k%d_s%d_r%d_b%d_%dx%d_c%d_ld%d' % c for c in CASES])
def test_im2col_k_matches_float64(case, mode):
  from epos_amd import _lib
  lib = _lib.load()
  k, stride, rate, B, Hi, Wi, C, ldx = case
  pad = (k - 1) // 2 * rate
  Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
  ldcol = (k * k * C + 3) // 4 * 4 + (4 if C == 5 else 0)    # also a wider row
  rng = np.random.RandomState(k * 100 + Hi)
  # values outside [0, 255] are legal float input
  x = rng.uniform(-40, 300, (B, Hi, Wi, ldx)).astype(np.float32)
  X = torch.from_numpy(x).cuda()
  col = torch.full((B * Ho * Wo, ldcol), float('nan'), device='cuda')
  words = 3 * _lib.AMAX_WORDS
  table = torch.full((words + 64,), -1, dtype=torch.int32, device='cuda')
  args = _lib.Im2colKArgs(X=_p(X), ldx=ldx, col=_p(col), ldcol=ldcol, B=B, Hi=Hi, Wi=Wi,
                          Ho=Ho, Wo=Wo, C=C, k=k, stride=stride, rate=rate, pad=pad,
                          preprocess=mode, mean_rgb=(ctypes.c_float * 3)(*MEAN_RGB),
                          amax_clear=_p(table), amax_words=words)
  _lib.check(lib.epos_im2col_f32(ctypes.byref(args), None))
  got = col.cpu().numpy()
  ref, padded = _im2col_ref(x, C, k, stride, rate, pad, Ho, Wo, ldcol, mode)
  np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-5)
  # padded taps are exactly 0 -- not -mean, not -1 -- at every border, and so is the tail
  assert (got[padded] == 0.0).all()
  taps = padded[:, :k * k * C].reshape(B, Ho, Wo, k, k, C)
  assert taps[:, 0, :, 0].any() and taps[:, -1, :, -1].any()          # top, bottom
  assert taps[:, :, 0, :, 0].any() and taps[:, :, -1, :, -1].any()    # left, right
  assert (got[:, k * k * C:] == 0.0).all()
  t = table.cpu().numpy()
  assert (t[:words] == 0).all() and (t[words:] == -1).all()


@pytest.mark.parametrize('stride', [1, 2])
def test_im2col_k3_unit_range_is_bit_identical_to_im2col3x3(stride):
  from epos_amd import _lib
  lib = _lib.load()
  B, Hi, Wi, C = 2, 33, 47, 3
  Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
  ldcol = 28
  x = np.random.RandomState(stride).uniform(0, 255, (B, Hi, Wi, C)).astype(np.float32)
  X = torch.from_numpy(x).cuda()
  outs = []
  for fn in ('3x3', 'k'):
    col = torch.full((B * Ho * Wo, ldcol), float('nan'), device='cuda')
    if fn == '3x3':
      a = _lib.Im2colArgs(X=_p(X), ldx=C, col=_p(col), ldcol=ldcol, B=B, Hi=Hi, Wi=Wi, Ho=Ho,
                          Wo=Wo, C=C, stride=stride, rate=1, pad=1, preprocess=1)
      _lib.check(lib.epos_im2col3x3_f32(ctypes.byref(a), None))
    else:
      a = _lib.Im2colKArgs(X=_p(X), ldx=C, col=_p(col), ldcol=ldcol, B=B, Hi=Hi, Wi=Wi,
                           Ho=Ho, Wo=Wo, C=C, k=3, stride=stride, rate=1, pad=1, preprocess=1)
      _lib.check(lib.epos_im2col_f32(ctypes.byref(a), None))
    outs.append(col.cpu().numpy())
  assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


def test_im2col_k_refuses_bad_arguments():
  from epos_amd import _lib
  lib = _lib.load()
  X = torch.zeros(1, 8, 8, 3, device='cuda')
  col = torch.zeros(16 * 148 + 4, device='cuda')     # room for the base shape
  base = dict(X=_p(X), ldx=3, col=_p(col), ldcol=148, B=1, Hi=8, Wi=8, Ho=4, Wo=4, C=3, k=7,
              stride=2, rate=1, pad=3, preprocess=2)
  for bad in (dict(ldcol=146), dict(ldcol=144), dict(preprocess=3), dict(k=0),
              dict(col=ctypes.c_void_p(col.data_ptr() + 4)),
              dict(amax_clear=_p(col), amax_words=16 * 37 + 1)):
    a = _lib.Im2colKArgs(**dict(base, **bad))
    assert lib.epos_im2col_f32(ctypes.byref(a), None) < 0, bad
  torch.cuda.synchronize()


def _ckpt(variant, num_objs, seed):
  """Random-init weights. The reference's initialiser draws the 7x7 root of resnet_v1_50 /
  resnet_v1_101 for inputs of unit scale, but those two see the mean-subtracted image (about
  127.5 times the [-1, 1] range of the other variants): every activation and head then grows
  ~100-fold (logits to ~400), and at that scale the oracle's own fp32 and fp64 heads already
  differ by 1e-3. The root is scaled by 1 / 127.5, as a network trained on that input range
  would be, so that the heads have the scale of the other variants and the bar of the existing
  parity tests applies."""
  from epos_amd import weights
  w = weights.random_init(variant, num_objs=num_objs, seed=seed, randomize_bn=True,
                          logits_std=0.2)
  if weights.VARIANTS[variant]['root'] == 'conv7':
    key = weights.VARIANTS[variant]['scope'] + '/conv1/weights'
    w[key] = (w[key] / np.float32(127.5)).astype(np.float32)
  return w


def _close(a, b, what):
  scale = max(1.0, float(np.abs(b).max()))
  np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4 * scale, err_msg=what)


def _check_against_oracle(net, out, ref):
  ep = ref['_end_points']

  def nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()
  _close(net.encoder.cpu().numpy(), nhwc(ep['encoder']), 'encoder')
  _close(net.decoder_concat.cpu().numpy(), nhwc(ep['decoder_concat']), 'decoder_concat')
  for k in ['pred_obj_conf', 'pred_frag_conf', 'pred_frag_loc']:
    a = out[k].cpu().numpy()
    assert a.shape == ref[k].shape and a.dtype == ref[k].dtype, k
    np.testing.assert_allclose(a, ref[k], rtol=1e-4, atol=1e-4, err_msg=k)
  lab = out['pred_obj_label'].cpu().numpy()
  conf = np.sort(ref['pred_obj_conf'], axis=-1)
  clear = (conf[..., -1] - conf[..., -2]) > 1e-3
  assert np.array_equal(lab[clear], ref['pred_obj_label'][clear])


@pytest.mark.parametrize('variant', NEW)
def test_variant_matches_oracle_and_replays(variant):
  from epos_amd import model
  from helpers import net_ref_variants as nv
  num_objs, B, h, w = 2, 2, 96, 128
  mg = [1, 2, 4] if variant == 'resnet_v1_50' else None
  ckpt = _ckpt(variant, num_objs, 5)
  img = np.random.RandomState(1).randint(0, 256, (B, h, w, 3)).astype('f')
  ref = nv.predict(img, ckpt, num_objs=num_objs, num_frags=64, model_variant=variant,
                   multi_grid=mg)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(num_objs, 64),
                          model_variant=variant, multi_grid=mg)
  net = model.get_net(ckpt, B, h, w, num_objs, 64, mo)
  out = net.forward(torch.from_numpy(img).cuda())
  torch.cuda.synchronize()
  _check_against_oracle(net, out, ref)
  if variant in ('resnet_v1_50', 'resnet_v1_101'):
    # the 7x7 root's im2col opens the plan and clears the slot table itself
    assert net.ops[0][0] == variant + '/conv1/im2col'
  # graph replay gives the same bits as eager
  a0 = {k: v.clone() for k, v in out.items()}
  out2 = net.forward(torch.from_numpy(img).cuda(), use_graph=True)
  torch.cuda.synchronize()
  for k in a0:
    assert torch.equal(a0[k], out2[k]), k


def test_uint8_frames_equal_float_frames_with_mean_subtraction():
  from epos_amd import model
  variant, num_objs, B, h, w = 'resnet_v1_101', 2, 2, 64, 96
  ckpt = _ckpt(variant, num_objs, 6)
  u8 = np.random.RandomState(3).randint(0, 256, (B, h, w, 3)).astype(np.uint8)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(num_objs, 64),
                          model_variant=variant)
  net = model.get_net(ckpt, B, h, w, num_objs, 64, mo)
  a = {k: v.clone() for k, v in net.forward(torch.from_numpy(u8.astype(np.float32))).items()}
  b = net.forward(torch.from_numpy(u8))
  torch.cuda.synchronize()
  for k in a:
    assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('variant', ['xception_71', 'resnet_v1_101'])
def test_variant_full_size_21_objects(variant):
  from epos_amd import model, synthetic
  from helpers import net_ref_variants as nv
  O, F, H, W_ = 21, 64, 480, 640
  ckpt = _ckpt(variant, O, 7)
  img = synthetic.image(4, H, W_)[None]
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), model_variant=variant)
  net = model.get_net(ckpt, 1, H, W_, O, F, mo)
  out = net.forward(torch.from_numpy(img).cuda())
  torch.cuda.synchronize()
  assert (net.out_h, net.out_w) == (120, 160)
  ref = nv.predict(img, ckpt, num_objs=O, num_frags=F, model_variant=variant)
  _check_against_oracle(net, out, ref)
  model._NETS.clear()


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


def test_pipeline_resnet_v1_50_dense_and_sparse_match_oracle_chain():
  from epos_amd import model, pipeline, synthetic, weights
  variant, O, F, B, H, W_ = 'resnet_v1_50', 4, 64, 2, 96, 128
  ckpt = weights.random_init(variant, num_objs=O, num_frags=F, seed=8, randomize_bn=True)
  store = synthetic.ModelStore(O, F, seed=0)
  img = np.stack([synthetic.image(i, H, W_) for i in range(B)])
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), model_variant=variant)
  net0 = model.get_net(ckpt, B, H, W_, O, F, mo)
  net0.forward(torch.from_numpy(img).cuda())
  torch.cuda.synchronize()
  synthetic.calibrate_logits(ckpt, net0.decoder_out[0].cpu().numpy())
  model._NETS.clear()
  Ks = np.tile(np.array([[300., 0, 64], [0, 300., 48], [0, 0, 1]]), (B, 1, 1))
  targets = [{1: 1, 4: 1}, {2: 1}]
  dense = pipeline.EposPipeline(ckpt, B, H, W_, O, F, store, capacity=1 << 16, instance=0,
                                model_options=mo)
  sparse = pipeline.EposPipeline(ckpt, B, H, W_, O, F, store, capacity=1 << 16, instance=1,
                                 sparse_heads=True, model_options=mo)
  assert dense.net.model_variant == variant and sparse.net.model_variant == variant
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


def test_infer_xception_71_synthetic_writes_csv(tmp_path, gpu_children):
  models = tmp_path / 'models'
  (models / 'toy').mkdir(parents=True)
  (models / 'toy' / 'params.yml').write_text('infer_crop_size: "128,96"\n')
  out = subprocess.run(
      ['timeout', '-k', '10', '600', sys.executable, os.path.join(ROOT, 'infer.py'),
       '--model=toy', '--model_variant', 'xception_71', '--synthetic', '2', '--num_objs', '3'],
      env=dict(os.environ, TF_MODELS_PATH=str(models)), capture_output=True, text=True,
      timeout=630)
  assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
  rows = (models / 'toy' / 'infer' / 'estimated-poses.csv').read_text().strip().split('\n')
  assert rows[0].startswith('scene_id')
