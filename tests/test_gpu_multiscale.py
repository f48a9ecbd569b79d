"""Multi-scale inference on the GPU (image_pyramid + merge_method, model.py:515-626):
epos_resize_merge_f32 bit for bit against the numpy float32 statement
(tests/helpers/multiscale_ref.py), model.predict(image_pyramid=...) against the composite of
the oracle per scale + resize + merge (reduced size, full C2 size, ResNet-101-beta, bf16), and
the pipeline on the merged heads: the oracle chain, planted poses at the merged stride, four
pipelines in flight, graph replay against eager."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import multiscale_ref as msr

pytestmark = pytest.mark.gpu

HEADS = ['pred_obj_conf', 'pred_frag_conf', 'pred_frag_loc']
E_INVALID = -1


def _p(t, off=0):
  return ctypes.c_void_p(t.data_ptr() + 4 * off)


def _dev_src(rng, B, hi, wi, C, ld, off):
  """A source [B,hi,wi,C] stored at channel offset `off` of rows `ld` floats wide."""
  x = rng.standard_normal((B, hi, wi, C)).astype(np.float32)
  buf = np.full((B, hi, wi, ld), np.nan, np.float32)
  buf[..., off:off + C] = x
  return x, torch.from_numpy(buf).cuda()


LAYOUTS = {'dense': lambda C: (C, 0), 'pitched': lambda C: (C + 8, 0),
           'unaligned': lambda C: (C + 3, 1)}
SRC_SIZES = [(5, 7), (9, 13), (17, 25), (1, 1)]      # up, identity, down, one pixel


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
@pytest.mark.parametrize('merge', ['max', 'avg'])
@pytest.mark.parametrize('C', [1, 3, 22, 64, 1344, 1347])
def test_resize_merge_bit_exact(C, merge, layout):
  from epos_amd import _lib
  lib = _lib.load()
  rng = np.random.RandomState(C * 7 + len(layout))
  ld, off = LAYOUTS[layout](C)
  mcode = _lib.MERGE_MAX if merge == 'max' else _lib.MERGE_MEAN
  cases = [(S, (9, 13)) for S in (1, 2, 3, 4)] + [(2, (1, 1)), (3, (4, 1)), (1, (17, 25))]
  for i, (S, (ho, wo)) in enumerate(cases):
    B = 1 if i % 2 == 0 else 3
    sizes = [SRC_SIZES[(i + s) % len(SRC_SIZES)] for s in range(S)]
    host, keep = [], []
    arr = (_lib.ResizeSrc * S)()
    for s, (hi, wi) in enumerate(sizes):
      x, t = _dev_src(rng, B, hi, wi, C, ld, off)
      host.append(x)
      keep.append(t)
      arr[s] = _lib.ResizeSrc(_p(t, off), ld, hi, wi)
    Y = torch.full((B, ho, wo, ld), float('nan'), device='cuda')
    _lib.check(lib.epos_resize_merge_f32(arr, S, _p(Y, off), ld, B, ho, wo, C, mcode, None))
    torch.cuda.synchronize()
    got = Y.cpu().numpy()
    want = msr.resize_merge(host, ho, wo, merge)
    assert np.array_equal(got[..., off:off + C], want), (C, merge, layout, S, sizes, ho, wo)
    assert np.isnan(got[..., :off]).all() and np.isnan(got[..., off + C:]).all()
  # a same-size single source is an exact copy
  x, t = _dev_src(rng, 2, 6, 10, C, ld, off)
  arr = (_lib.ResizeSrc * 1)(_lib.ResizeSrc(_p(t, off), ld, 6, 10))
  Y = torch.zeros((2, 6, 10, C), device='cuda')
  _lib.check(lib.epos_resize_merge_f32(arr, 1, _p(Y), C, 2, 6, 10, C, mcode, None))
  torch.cuda.synchronize()
  assert np.array_equal(Y.cpu().numpy(), x)


def test_resize_merge_invalid_arguments():
  from epos_amd import _lib
  lib = _lib.load()
  X = torch.zeros(4 * 4 * 8, device='cuda')
  Y = torch.zeros(4 * 4 * 8, device='cuda')
  good = _lib.ResizeSrc(_p(X), 8, 4, 4)
  arr9 = (_lib.ResizeSrc * 9)(*([good] * 9))
  null = (_lib.ResizeSrc * 1)(_lib.ResizeSrc(None, 8, 4, 4))
  f = lib.epos_resize_merge_f32
  assert f(arr9, 0, _p(Y), 8, 1, 4, 4, 8, 0, None) == E_INVALID          # S = 0
  assert f(arr9, 9, _p(Y), 8, 1, 4, 4, 8, 0, None) == E_INVALID          # S > 8
  assert f(None, 1, _p(Y), 8, 1, 4, 4, 8, 0, None) == E_INVALID          # no sources
  assert f(arr9, 1, None, 8, 1, 4, 4, 8, 0, None) == E_INVALID           # no output
  assert f(null, 1, _p(Y), 8, 1, 4, 4, 8, 0, None) == E_INVALID          # null source
  assert f(arr9, 1, _p(Y), 8, 1, 4, 4, 0, 0, None) == E_INVALID          # C < 1
  assert f(arr9, 1, _p(Y), 4, 1, 4, 4, 8, 0, None) == E_INVALID          # ldy < C
  assert f(arr9, 1, _p(Y), 8, 1, 4, 4, 8, 2, None) == E_INVALID          # unknown merge
  assert f(arr9, 8, _p(Y), 8, 1, 4, 4, 8, 1, None) == 0                  # S = 8 is fine
  torch.cuda.synchronize()


def _check_heads(got, ref, bar, what=''):
  for k in HEADS:
    a = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
    assert a.shape == ref[k].shape and a.dtype == ref[k].dtype, (what, k)
    np.testing.assert_allclose(a, ref[k], rtol=bar, atol=bar, err_msg='%s %s' % (what, k))
  lab = got['pred_obj_label'].cpu().numpy()
  assert lab.dtype == np.int64 and lab.shape == ref['pred_obj_label'].shape
  conf = np.sort(ref['pred_obj_conf'], axis=-1)
  clear = (conf[..., -1] - conf[..., -2]) > 1e-3
  assert np.array_equal(lab[clear], ref['pred_obj_label'][clear]), what


@pytest.mark.parametrize('pyr,merge,batch,u8', [
    ([0.5, 1.0, 1.25], 'max', 1, False),     # per-scale sizes 32x48, 64x96, 79x119 (odd)
    ([0.5, 1.0], 'avg', 2, False),
    ([0.5], 'max', 1, False),                # one scale != 1: still resized to stride 4
    ([0.5, 0.75], 'avg', 1, True),           # no 1.0 plan: own image buffer, uint8 frames
    ([1.0, 1.0], 'max', 1, False),           # one merge entry 'logits_1.00' (model.py:606)
    ([1.0, 0.5, 1.0, 0.501], 'avg', 1, False),   # entries 1.00 and 0.50: the last of each
])
def test_predict_matches_composite(pyr, merge, batch, u8):
  from epos_amd import model, weights
  O, F, H, W_ = 2, 64, 64, 96
  ckpt = weights.random_init(num_objs=O, seed=3, randomize_bn=True, logits_std=0.2)
  img = np.random.RandomState(len(pyr)).randint(0, 256, (batch, H, W_, 3)).astype('f')
  ref = msr.predict(img, ckpt, O, F, pyr, merge)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), merge_method=merge)
  x = torch.from_numpy(img.astype(np.uint8) if u8 else img).cuda()
  out = model.predict(x, mo, ckpt, image_pyramid=pyr, num_objs=O, num_frags=F)
  torch.cuda.synchronize()
  lh, lw = msr.merged_size(H, W_, pyr)
  assert tuple(out['pred_frag_loc'].shape) == (batch, lh, lw, O, F, 3)
  _check_heads(out, ref, 2e-4, str(pyr))
  # the plan is cached per pyramid and merge method; graph replay = eager, bit for bit
  net = model.get_net(ckpt, batch, H, W_, O, F, mo, image_pyramid=pyr)
  assert model.get_net(ckpt, batch, H, W_, O, F, mo, image_pyramid=list(pyr)) is net
  eager = {k: v.clone() for k, v in out.items()}
  graph = net.forward(x, use_graph=True)
  torch.cuda.synchronize()
  for k in eager:
    assert torch.equal(eager[k], graph[k]), k


def test_single_scale_pyramid_is_the_plain_plan():
  from epos_amd import model, net, weights
  ckpt = weights.random_init(num_objs=1, seed=0)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(1, 64))
  for pyr in (None, [1.0]):
    assert type(model.get_net(ckpt, 1, 64, 64, 1, 64, mo, image_pyramid=pyr)) is net.EposNet
  img = np.zeros((1, 64, 64, 3), np.float32)
  with pytest.raises(ValueError):
    model.predict(img, mo, ckpt, image_pyramid=[], num_objs=1, num_frags=64)


def test_resnet_v1_101_beta_pyramid():
  from epos_amd import model, weights
  O, F, H, W_, pyr = 2, 64, 64, 96, [0.75, 1.0]
  v = 'resnet_v1_101_beta'
  ckpt = weights.random_init(v, num_objs=O, seed=4, randomize_bn=True, logits_std=0.2)
  img = np.random.RandomState(2).randint(0, 256, (1, H, W_, 3)).astype('f')
  ref = msr.predict(img, ckpt, O, F, pyr, 'max', model_variant=v)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), model_variant=v)
  out = model.predict(img, mo, ckpt, image_pyramid=pyr, num_objs=O, num_frags=F)
  torch.cuda.synchronize()
  _check_heads(out, ref, 2e-4, v)


def test_bf16_pyramid_against_emulated_oracle():
  """precision='bf16' composes: the merged raw logits against the float64 composite, at the
  bf16 mode's bar (rms(GPU - fp64) <= 1.5 x rms(emulated bf16 - fp64), as
  tests/test_gpu_bf16_net.py holds the single-scale plan)."""
  from helpers import net_ref_bf16 as nb
  from oracle import net_ref
  from epos_amd import multiscale, synthetic, weights
  O, F, H, W_, pyr = 2, 8, 64, 96, [0.5, 1.0, 1.25]
  ckpt = weights.random_init(num_objs=O, num_frags=F, seed=4, randomize_bn=True)
  img = synthetic.image(1, H, W_)[None]
  with net_ref.precision(torch.float64):
    ref = msr.logits(img, ckpt, O, F, pyr, 'max')
    with nb.emulate_bf16():
      emu = msr.logits(img, nb.bf16_checkpoint(ckpt), O, F, pyr, 'max')
  n = multiscale.MultiScaleNet(ckpt, 1, H, W_, O, F, image_pyramid=pyr, precision='bf16')
  assert all(p.precision == 'bf16' for p in n.nets)
  n.set_images(torch.from_numpy(img).cuda())
  n.run_plan(with_post=False)           # the merged raw logits: no in-place softmax
  torch.cuda.synchronize()
  for k in HEADS:
    g = n.logits[k].cpu().numpy()
    assert np.isfinite(g).all(), k
    eg = np.sqrt(np.mean((g.astype(np.float64) - ref[k]) ** 2))
    ee = np.sqrt(np.mean((emu[k] - ref[k]) ** 2))
    assert 0 < ee and eg <= 1.5 * ee, (k, eg, ee)


def test_c2_full_size_two_scales():
  """C2: 640x480, 21 objects, [0.75, 1.0], against the composite at the survey bar."""
  from epos_amd import model, synthetic, weights
  O, F, H, W_, pyr = 21, 64, 480, 640, [0.75, 1.0]
  ckpt = weights.random_init(num_objs=O, seed=0, randomize_bn=True, logits_std=0.2)
  img = synthetic.image(0, H, W_)[None]
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F))
  out = model.predict(img, mo, ckpt, image_pyramid=pyr, num_objs=O, num_frags=F)
  torch.cuda.synchronize()
  got = {k: v.cpu().numpy() for k, v in out.items()}
  ref = msr.predict(img, ckpt, O, F, pyr, 'max')
  for k in HEADS:
    np.testing.assert_allclose(got[k], ref[k], rtol=1e-4, atol=1e-4, err_msg=k)


class Store(object):
  def __init__(self, num_objs, num_frags, seed=0):
    rng = np.random.RandomState(seed)
    self.dp_model = {'obj_ids': list(range(1, num_objs + 1))}
    self.frag_centers = {o: rng.uniform(-80, 80, (num_frags, 3))
                         for o in self.dp_model['obj_ids']}
    self.frag_sizes = {o: rng.uniform(5, 40, num_frags)
                       for o in self.dp_model['obj_ids']}


def test_pipeline_matches_oracle_chain_at_the_merged_stride():
  from epos_amd import pipeline, weights
  from oracle import corresp_ref, pnp_ref
  O, F, B, H, W_, pyr = 3, 64, 2, 96, 128, [0.75, 1.0, 1.25]
  ckpt = weights.random_init(num_objs=O, seed=5, randomize_bn=True, logits_std=0.6)
  store = Store(O, F)
  pipe = pipeline.EposPipeline(ckpt, B, H, W_, O, F, store, capacity=1 << 18,
                               image_pyramid=pyr)
  assert pipe.output_scale == 1.25 / 4 and pipe.net.out_h == msr.merged_size(H, W_, pyr)[0]
  img = np.random.RandomState(1).randint(0, 256, (B, H, W_, 3)).astype('f')
  Ks = np.tile(np.array([[300., 0, 64], [0, 300., 48], [0, 0, 1]]), (B, 1, 1))
  targets = [{1: 1, 3: 1}, {2: 1}]
  poses, _ = pipe.process_batch(torch.from_numpy(img).cuda(), Ks, targets, seed=7)
  pred = {k: v.cpu().numpy() for k, v in pipe.net.outputs().items()}
  slots, wants = pipe.make_slots(targets)
  exp = []
  for (im, obj_id), want in zip(slots, wants):
    c = corresp_ref.establish_many_to_many(
        pred['pred_obj_conf'][im], pred['pred_frag_conf'][im],
        pred['pred_frag_loc'][im], [obj_id], store.dp_model['obj_ids'],
        store.frag_centers, store.frag_sizes, 1.25 / 4, 0.1, 0.5, True)
    if obj_id not in c:
      continue
    seed = (7 * 1000003 + im * 1009 + obj_id) & 0x7fffffffffffffff
    rp, rl, rs = pnp_ref.find6DPoses(
        c[obj_id]['coord_2d'], c[obj_id]['coord_3d'], Ks[im],
        params=pnp_ref.default_params(max_model_number=want), seed=seed)
    if rp is not None:
      exp.append((im, obj_id, rp, rs))
  assert exp and len(poses) == len(exp)
  for p, (im, obj_id, rp, rs) in zip(poses, exp):
    assert (p['im_id'], p['obj_id']) == (im, obj_id)
    np.testing.assert_allclose(np.hstack([p['R'], p['t']]), rp[:3], atol=1e-9)
    np.testing.assert_allclose(p['score'], rs[0], rtol=1e-12)


def test_planted_poses_at_the_merged_stride():
  """Heads rendered from known poses at the merged map's stride 4 / 1.25 (the scatter of
  bench.py --planted-poses): the poses come back only if the correspondences are placed with
  the merged output scale."""
  from epos_amd import _lib, pipeline, synthetic, weights
  lib = _lib.load()
  O, F, H, W, pyr = 6, 64, 240, 320, [0.75, 1.0, 1.25]
  K = synthetic.YCBV_K.copy()
  K[:2] *= 0.5
  store = synthetic.ModelStore(O, F, seed=0)
  ckpt = weights.random_init(num_objs=O, seed=1, randomize_bn=True, logits_std=0.6)
  pipe = pipeline.EposPipeline(ckpt, 1, H, W, O, F, store, capacity=1 << 16,
                               image_pyramid=pyr)
  tgs = [{2: 1, 5: 1}]
  sc = synthetic.planted_scene(10, store, tgs[0], K, pipe.net.out_h, pipe.net.out_w, O, F,
                               stride=4 / 1.25, outlier_frac=0.5, depth_mm=(300.0, 500.0))
  dv = {k: (torch.from_numpy(sc[k][0]).cuda(),
            torch.from_numpy(np.ascontiguousarray(sc[k][1].reshape(len(sc[k][0]), -1))).cuda())
        for k in ('obj', 'frag', 'loc')}

  def plant(p):
    st = ctypes.c_void_p(p.stream.cuda_stream)
    for key, name in (('obj', weights.PRED_OBJ_CONF), ('frag', weights.PRED_FRAG_CONF),
                      ('loc', weights.PRED_FRAG_LOC)):
      off, val = dv[key]
      _lib.check(lib.epos_scatter_blocks_f32(
          ctypes.c_void_p(p.net.logits[name].data_ptr()), ctypes.c_void_p(off.data_ptr()),
          ctypes.c_void_p(val.data_ptr()), off.numel(), int(val.shape[1]), st), 'scatter')
  img = synthetic.image(0, H, W)[None]
  poses, _ = pipe.process_batch(torch.from_numpy(img).cuda(), K[None], tgs, image_ids=[0],
                                seed=5, after_net=plant)
  for obj_id, R, t in sc['poses']:
    cand = [synthetic.pose_errors(p['R'], p['t'], R, t) for p in poses
            if p['obj_id'] == obj_id]
    assert cand and min(c[0] for c in cand) < 1.0 and min(c[1] for c in cand) < 5.0, (
        obj_id, cand)


def test_four_multiscale_pipelines_in_flight_repeat_bit_for_bit():
  from epos_amd import pipeline, weights
  O, F, B, H, W_, pyr = 3, 64, 1, 96, 128, [0.75, 1.0, 1.25]
  ckpt = weights.random_init(num_objs=O, seed=9, randomize_bn=True, logits_std=0.6)
  store = Store(O, F)
  pipes = [pipeline.EposPipeline(ckpt, B, H, W_, O, F, store, capacity=1 << 18, instance=j,
                                 image_pyramid=pyr) for j in range(4)]
  rng = np.random.RandomState(3)
  frames = [torch.from_numpy(rng.randint(0, 256, (B, H, W_, 3)).astype('f')).cuda()
            for _ in range(2)]
  Ks = np.tile(np.array([[300., 0, 64], [0, 300., 48], [0, 0, 1]]), (B, 1, 1))
  targets = [{1: 1, 2: 1, 3: 1}]
  ref = {}
  for rnd in range(3):
    for f, img in enumerate(frames):
      for p in pipes:
        p.launch(img, Ks, targets, seed=11)
      for p in pipes:
        poses, _ = p.collect()
        heads = {k: p.net.logits[k].cpu() for k in HEADS}
        if f not in ref:
          ref[f] = (poses, heads)
        rp, rh = ref[f]
        for k in HEADS:
          assert torch.equal(heads[k], rh[k]), k
        assert len(poses) == len(rp)
        for a, b in zip(poses, rp):
          assert a['obj_id'] == b['obj_id'] and a['score'] == b['score']
          assert np.array_equal(a['R'], b['R']) and np.array_equal(a['t'], b['t'])


def test_infer_multi_scale_synthetic_writes_csv(tmp_path, gpu_children):
  import os
  import subprocess
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  models = tmp_path / 'models'
  (models / 'toy').mkdir(parents=True)
  (models / 'toy' / 'params.yml').write_text('infer_crop_size: "128,96"\n')
  cmd = ['timeout', '-k', '10', '600', sys.executable, os.path.join(root, 'infer.py'),
         '--model=toy', '--synthetic', '4', '--num_objs', '3', '--image_pyramid',
         '0.75,1.0,1.25']
  env = dict(os.environ, TF_MODELS_PATH=str(models))
  out = subprocess.run(cmd + ['--multi_scale_inference', 'true'], env=env,
                       capture_output=True, text=True, timeout=630)
  assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
  assert 'image pyramid [0.75, 1.0, 1.25]' in out.stdout and 'NOTE --image_pyramid' in out.stdout
  rows = (models / 'toy' / 'infer' / 'estimated-poses.csv').read_text().strip().split('\n')
  assert rows[0].startswith('scene_id')
  # without the flag the same pyramid is refused
  out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=630)
  assert out.returncode != 0 and 'NotImplementedError' in out.stderr, out.stderr[-2000:]
