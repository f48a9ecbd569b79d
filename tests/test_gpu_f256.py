"""256 fragments per object on the GPU (the reference's "-f256" models): the correspondence
kernels bit-exact against the f256_* fixtures recorded from the imported reference and against
the numpy oracle at the C2 head size, the fragment softmax for 64 < F <= 256 against fp64 (the
sparse-head kernel bit-identical to the dense one), the network against the torch-CPU oracle
at reduced and at full C2 size, the pipeline against the oracle chain (dense and sparse heads)
and on a planted scene, and infer.py / bench.py at --num_frags 256."""
import ctypes
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
KEYS = ['px_id', 'frag_id', 'coord_2d', 'coord_3d', 'conf', 'conf_obj', 'conf_frag']
CASES = sorted(glob.glob(os.path.join(GOLDEN, 'f256_corresp_*.npz')))


class Store(object):
  def __init__(self, centers, sizes):
    n = centers.shape[0]
    self.dp_model = {'obj_ids': list(range(1, n + 1))}
    self.frag_centers = {o + 1: centers[o] for o in range(n)}
    self.frag_sizes = {o + 1: sizes[o] for o in range(n)}


def _p(t, off=0):
  return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


# ------------------------------------------------------------- correspondences ---
@pytest.mark.parametrize('path', CASES, ids=[os.path.basename(p) for p in CASES])
def test_corresp_bit_exact_vs_f256_reference_golden(path):
  from epos_amd import corresp
  z = np.load(path)
  out = corresp.establish_many_to_many(
      z['obj_confs'], z['frag_confs'], z['frag_coords'],
      gt_obj_ids=list(z['gt_obj_ids']),
      model_store=Store(z['frag_centers'], z['frag_sizes']),
      output_scale=float(z['output_scale']),
      min_obj_conf=float(z['min_obj_conf']),
      min_frag_rel_conf=float(z['min_frag_rel_conf']),
      project_to_surface=False, only_annotated_objs=bool(z['only_annotated']))
  assert sorted(out.keys()) == sorted(int(o) for o in z['out_obj_ids'])
  for oid in out:
    for k in KEYS:
      exp = z['out_%d_%s' % (oid, k)]
      assert out[oid][k].dtype == exp.dtype, (oid, k)
      assert np.array_equal(out[oid][k], exp), (oid, k)


def test_corresp_f256_matches_oracle_at_full_size():
  """C2 head map (120x160, 21 objects, 256 fragments): HIP vs the numpy oracle, bit-exact,
  plus raster / ascending-fragment order across the four mask words."""
  from epos_amd import corresp
  from oracle import corresp_ref
  rng = np.random.default_rng(11)
  h, w, O, F = 120, 160, 21, 256
  obj = rng.standard_normal((h, w, O + 1), dtype=np.float32) * 3
  obj = (np.exp(obj) / np.exp(obj).sum(-1, keepdims=True)).astype('f')
  frag = rng.standard_normal((h, w, O, F), dtype=np.float32) * 3
  frag = np.exp(frag)
  frag /= frag.sum(-1, keepdims=True)
  loc = rng.standard_normal((h, w, O, F, 3), dtype=np.float32)
  store = Store(rng.uniform(-80, 80, (O, F, 3)), rng.uniform(5, 40, (O, F)))
  gt = [1, 7, 21]
  out = corresp.establish_many_to_many(obj, frag, loc, gt, store, 0.25, 0.1, 0.5, False,
                                       True)
  ref = corresp_ref.establish_many_to_many(
      obj, frag, loc, gt, store.dp_model['obj_ids'], store.frag_centers, store.frag_sizes,
      0.25, 0.1, 0.5, True)
  assert sorted(out) == sorted(ref) == gt
  for oid in gt:
    for k in KEYS:
      assert np.array_equal(out[oid][k], ref[oid][k]), (oid, k)
    px, fr = out[oid]['px_id'], out[oid]['frag_id']
    assert (np.diff(px) >= 0).all()
    assert (np.diff(fr)[np.diff(px) == 0] > 0).all()
    assert fr.max() >= 192                             # the last mask word is used


def test_corresp_refuses_more_than_256_fragments():
  from epos_amd import _lib
  lib = _lib.load()
  S, P, O, F = 1, 64, 1, 257
  oc = torch.zeros(P * (O + 1), device='cuda')
  fc = torch.zeros(P * O * F, device='cuda')
  slots = torch.tensor([[0, 1]], dtype=torch.int32, device='cuda')
  i32 = torch.zeros(S * P, dtype=torch.int32, device='cuda')
  mask = torch.zeros(S * P * 5, dtype=torch.int64, device='cuda')
  tot = torch.zeros(2 * S, dtype=torch.int32, device='cuda')
  rc = lib.epos_corr_count(_p(oc), _p(fc), _p(slots), S, 1, P, O, F, 0.1, 0.5, _p(i32),
                           _p(i32), _p(mask), _p(tot), None)
  assert rc == -1                                     # EPOS_E_INVALID
  assert b'[1, 256]' in lib.epos_last_error()


def test_fragmentation_fps_f256_matches_reference_golden():
  from epos_amd import fragment
  z = np.load(os.path.join(GOLDEN, 'f256_fragment_ellipsoid_s2.npz'))
  centers, ids = fragment.fragmentation_fps(z['vertices'], 256)
  assert np.array_equal(centers, z['frag_centers'])
  assert np.array_equal(ids, z['vertex_frag_ids'])


# --------------------------------------------------------------------- softmax ---
def _softmax_case(G, off):
  rng = np.random.RandomState(G * 10 + off)
  n = 301
  x = (rng.standard_normal((n, G)) * 3).astype(np.float32)
  x[3] = np.where(np.arange(G) % 2, 80.0, -80.0)
  x[4] = 1.25                                          # all tied
  x[5, :G // 2] = 2.5                                  # a tied maximum
  x[6, [63, 64, G - 1]] = 40.0                         # maxima across the lane blocks
  return x


@pytest.mark.parametrize('G,off', [(65, 0), (128, 0), (200, 0), (255, 0), (256, 0),
                                   (256, 1)],
                         ids=['G65', 'G128', 'G200', 'G255', 'G256', 'G256-off1'])
def test_softmax_wide_against_fp64_and_slots_bit_identical(G, off):
  """epos_softmax_groups_f32 for 64 < G <= 256 (G = 256 on an aligned buffer: the float4
  kernel; otherwise the generic one) against fp64; epos_softmax_slots_f32 on the same data,
  laid out as [B, P, O, F], gives the dense kernel's bits on the slots and leaves the other
  groups alone."""
  from epos_amd import _lib
  lib = _lib.load()
  x = _softmax_case(G, off)
  n = x.shape[0]
  buf = torch.full((x.size + G,), 123.0, device='cuda')
  buf[off:off + x.size] = torch.from_numpy(x.ravel()).cuda()
  _lib.check(lib.epos_softmax_groups_f32(_p(buf, off), n, G, None), 'softmax_groups')
  torch.cuda.synchronize()
  got = buf.cpu().numpy()
  assert (got[:off] == 123.0).all() and (got[off + x.size:] == 123.0).all()
  dense = got[off:off + x.size].reshape(n, G)
  ref = torch.softmax(torch.from_numpy(x).double(), dim=-1).numpy()
  np.testing.assert_allclose(dense, ref, rtol=2e-6, atol=1e-7)
  assert (np.abs(dense.astype(np.float64).sum(-1) - 1) <= G * 2.0 ** -24).all()
  # the same groups as [B=2, P, O=3, F]: slots (0, 2), (1, 1), (1, 3)
  B, O, P = 2, 3, n // 6
  xs = x[:B * P * O].reshape(B, P, O, G)
  slots = [(0, 2), (1, 1), (1, 3)]
  buf2 = torch.full((xs.size + G,), 123.0, device='cuda')
  buf2[off:off + xs.size] = torch.from_numpy(xs.ravel()).cuda()
  sl = torch.tensor(slots, dtype=torch.int32, device='cuda')
  _lib.check(lib.epos_softmax_slots_f32(_p(buf2, off), _p(sl), len(slots), P, O, G, None),
             'softmax_slots')
  torch.cuda.synchronize()
  got2 = buf2.cpu().numpy()[off:off + xs.size].reshape(B, P, O, G)
  dense4 = dense[:B * P * O].reshape(B, P, O, G)
  for im in range(B):
    for obj in range(1, O + 1):
      if (im, obj) in slots:
        assert np.array_equal(got2[im, :, obj - 1].view(np.uint32),
                              dense4[im, :, obj - 1].view(np.uint32)), (im, obj)
      else:
        assert np.array_equal(got2[im, :, obj - 1], xs[im, :, obj - 1]), (im, obj)


def test_softmax_refuses_more_than_256():
  from epos_amd import _lib
  lib = _lib.load()
  buf = torch.zeros(257 * 4, device='cuda')
  sl = torch.tensor([[0, 1]], dtype=torch.int32, device='cuda')
  assert lib.epos_softmax_groups_f32(_p(buf), 4, 257, None) < 0
  assert lib.epos_softmax_slots_f32(_p(buf), _p(sl), 1, 4, 1, 257, None) < 0
  torch.cuda.synchronize()
  assert (buf.cpu() == 0).all()


# --------------------------------------------------------------------- network ---
def test_net_f256_matches_oracle_reduced_size():
  from epos_amd import model, weights
  from oracle import net_ref
  O, F, h, w = 2, 256, 96, 128
  ckpt = weights.random_init(num_objs=O, num_frags=F, seed=3, randomize_bn=True,
                             logits_std=0.2)
  img = np.random.RandomState(0).randint(0, 256, (1, h, w, 3)).astype('f')
  ref = net_ref.predict(img, ckpt, num_objs=O, num_frags=F)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F))
  net = model.get_net(ckpt, 1, h, w, O, F, mo)
  out = net.forward(torch.from_numpy(img).cuda())
  torch.cuda.synchronize()
  for k in ['pred_obj_conf', 'pred_frag_conf', 'pred_frag_loc']:
    a = out[k].cpu().numpy()
    assert a.shape == ref[k].shape and a.dtype == ref[k].dtype, k
    np.testing.assert_allclose(a, ref[k], rtol=1e-4, atol=1e-4, err_msg=k)
  a0 = out['pred_frag_conf'].clone()
  l0 = out['pred_frag_loc'].clone()
  out2 = net.forward(torch.from_numpy(img).cuda(), use_graph=True)
  torch.cuda.synchronize()
  assert torch.equal(a0, out2['pred_frag_conf'])
  assert torch.equal(l0, out2['pred_frag_loc'])


def test_c2_f256_full_size_heads_match_oracle():
  """C2 at 640x480 with 21 objects x 256 fragments (heads of 5376 / 16128 channels): the
  object head and the target objects' fragment heads against the torch-CPU oracle."""
  from epos_amd import model, synthetic, weights
  from oracle import net_ref
  O, F, H, W_ = 21, 256, 480, 640
  ckpt = weights.random_init(num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  img = synthetic.image(7, H, W_)[None]
  net = model.get_net(ckpt, 1, H, W_, O, F)
  out = net.forward(torch.from_numpy(img).cuda())
  torch.cuda.synchronize()
  objs = [o - 1 for o in synthetic.targets(7, O, 5)]
  got = {'pred_obj_conf': out['pred_obj_conf'].cpu().numpy(),
         'pred_frag_conf': out['pred_frag_conf'][:, :, :, objs].cpu().numpy(),
         'pred_frag_loc': out['pred_frag_loc'][:, :, :, objs].cpu().numpy()}
  model._NETS.clear()
  del net, out
  ref = net_ref.predict(img, ckpt, num_objs=O, num_frags=F)
  want = {'pred_obj_conf': ref['pred_obj_conf'],
          'pred_frag_conf': ref['pred_frag_conf'][:, :, :, objs],
          'pred_frag_loc': ref['pred_frag_loc'][:, :, :, objs]}
  del ref
  for k in want:
    assert got[k].shape == want[k].shape, k
    np.testing.assert_allclose(got[k], want[k], rtol=1e-4, atol=1e-4, err_msg=k)
  np.testing.assert_allclose(got['pred_frag_conf'].sum(-1), 1.0, atol=1e-5)


# -------------------------------------------------------------------- pipeline ---
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


def test_pipeline_f256_dense_and_sparse_match_oracle_chain():
  """EposPipeline at F = 256 with dense and with sparse heads: the target objects' fragment
  channels are bit-identical between the two, and the poses equal the oracle chain run on
  the HIP heads."""
  from epos_amd import model, pipeline, synthetic, weights
  O, F, B, H, W_ = 4, 256, 2, 96, 128
  ckpt = weights.random_init(num_objs=O, num_frags=F, seed=8, randomize_bn=True)
  store = synthetic.ModelStore(O, F, seed=0)
  img = np.stack([synthetic.image(i, H, W_) for i in range(B)])
  net0 = model.get_net(ckpt, B, H, W_, O, F)
  net0.forward(torch.from_numpy(img).cuda())
  torch.cuda.synchronize()
  synthetic.calibrate_logits(ckpt, net0.decoder_out[0].cpu().numpy())
  model._NETS.clear()
  Ks = np.tile(np.array([[300., 0, 64], [0, 300., 48], [0, 0, 1]]), (B, 1, 1))
  targets = [{1: 1, 4: 1}, {2: 1}]
  dense = pipeline.EposPipeline(ckpt, B, H, W_, O, F, store, capacity=1 << 16, instance=0)
  sparse = pipeline.EposPipeline(ckpt, B, H, W_, O, F, store, capacity=1 << 16, instance=1,
                                 sparse_heads=True)
  assert dense.capacity == 4 << 16
  x = torch.from_numpy(img).cuda()
  pd, _ = dense.process_batch(x, Ks, targets, seed=2)
  ps, _ = sparse.process_batch(x, Ks, targets, seed=2)
  dc = dense.net.logits['pred_frag_conf'].view(B, -1, O, F)
  sc = sparse.net.logits['pred_frag_conf'].view(B, -1, O, F)
  dl = dense.net.logits['pred_frag_loc'].view(B, -1, O, F * 3)
  sl = sparse.net.logits['pred_frag_loc'].view(B, -1, O, F * 3)
  for im, t in enumerate(targets):
    for obj in t:
      assert torch.equal(dc[im, :, obj - 1], sc[im, :, obj - 1])
      assert torch.equal(dl[im, :, obj - 1], sl[im, :, obj - 1])
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


def test_planted_scene_f256_recovered_through_the_hip_pipeline():
  """A planted scene rendered into the F = 256 heads between the network and the
  correspondence stage: the planted counts come through and every pose is recovered within
  1 degree / 5 mm."""
  from epos_amd import _lib, pipeline, synthetic, weights
  lib = _lib.load()
  O, F, H, W = 6, 256, 240, 320
  K = synthetic.YCBV_K.copy()
  K[:2] *= 0.5
  store = synthetic.ModelStore(O, F, seed=0)
  ckpt = weights.random_init(num_objs=O, num_frags=F, seed=1, randomize_bn=True,
                             logits_std=0.6)
  pipe = pipeline.EposPipeline(ckpt, 2, H, W, O, F, store, capacity=1 << 16)
  tgs = [{2: 1, 5: 1}, {1: 2}]
  scenes = [synthetic.planted_scene(10 + b, store, tgs[b], K, pipe.net.out_h, pipe.net.out_w,
                                    O, F, outlier_frac=0.5, image_in_batch=b,
                                    depth_mm=(300.0, 500.0)) for b in range(2)]
  dv = {}
  for key in ('obj', 'frag', 'loc'):
    off = np.concatenate([sc[key][0] for sc in scenes])
    val = np.concatenate([sc[key][1].reshape(len(sc[key][0]), -1) for sc in scenes])
    dv[key] = (torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(val)).cuda(),
               int(val.shape[1]))

  def plant(p):
    st = ctypes.c_void_p(p.stream.cuda_stream)
    for key, name in (('obj', weights.PRED_OBJ_CONF), ('frag', weights.PRED_FRAG_CONF),
                      ('loc', weights.PRED_FRAG_LOC)):
      off, val, width = dv[key]
      _lib.check(lib.epos_scatter_blocks_f32(
          ctypes.c_void_p(p.net.logits[name].data_ptr()), ctypes.c_void_p(off.data_ptr()),
          ctypes.c_void_p(val.data_ptr()), off.numel(), width, st), 'scatter')
  imgs = np.stack([synthetic.image(b, H, W) for b in range(2)])
  poses, _ = pipe.process_batch(torch.from_numpy(imgs).cuda(), np.stack([K, K]), tgs,
                                image_ids=[0, 1], seed=5, after_net=plant)
  totals = pipe.last_totals
  want = [scenes[0]['stats'][2][0], scenes[0]['stats'][5][0], scenes[1]['stats'][1][0]]
  assert [int(x) for x in totals[:, 0]] == want
  assert [int(x) for x in totals[:, 1]] == [2 * x for x in want]
  for b, sc in enumerate(scenes):
    for obj_id, R, t in sc['poses']:
      cand = [synthetic.pose_errors(p['R'], p['t'], R, t) for p in poses
              if p['im_id'] == b and p['obj_id'] == obj_id]
      assert cand and min(c[0] for c in cand) < 1.0 and min(c[1] for c in cand) < 5.0, \
          (b, obj_id, cand)


# ------------------------------------------------------------------------- CLI ---
def _infer(models, extra, timeout=600):
  out = subprocess.run(
      ['timeout', '-k', '10', str(timeout), sys.executable, os.path.join(ROOT, 'infer.py'),
       '--model=toy', '--synthetic', '3', '--num_objs', '3', '--num_frags', '256'] + extra,
      env=dict(os.environ, TF_MODELS_PATH=str(models)), capture_output=True, text=True,
      timeout=timeout + 30)
  assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
  txt = (models / 'toy' / 'infer' / 'estimated-poses.csv').read_text().strip().split('\n')
  return out.stdout, [','.join(r.split(',')[:-1]) for r in txt]


def test_infer_f256_sparse_and_dense_give_the_same_poses(tmp_path, gpu_children):
  rows = {}
  for name, extra in (('auto', []), ('dense', ['--sparse_heads', 'false'])):
    models = tmp_path / name
    (models / 'toy').mkdir(parents=True)
    (models / 'toy' / 'params.yml').write_text('infer_crop_size: "128,96"\n')
    stdout, rows[name] = _infer(models, extra)
    plan = [l for l in stdout.split('\n') if l.startswith('plan:')][0]
    assert (', sparse' in plan) == (name == 'auto'), plan
  assert rows['dense'][0].startswith('scene_id')
  assert rows['auto'] == rows['dense']


def test_infer_f256_with_fragments_from_ply_models(tmp_path, gpu_children):
  """fragments.pkl made on the GPU (256 FPS fragments of PLY models) drives the run."""
  from epos_amd import fragment, ply
  rng = np.random.RandomState(0)
  mdir = tmp_path / 'ply'
  mdir.mkdir()
  pts = {}
  for o in (1, 2, 3):
    d = rng.standard_normal((2000, 3))
    path = str(mdir / ('obj_%06d.ply' % o))
    ply.save_ply(path, d / np.linalg.norm(d, axis=1, keepdims=True) * (30 + 10 * o))
    pts[o] = ply.load_ply(path)['pts']
  centers, sizes = fragment.fragment_models(pts, 256)
  models = tmp_path / 'models'
  (models / 'toy').mkdir(parents=True)
  (models / 'toy' / 'params.yml').write_text('infer_crop_size: "128,96"\n')
  fragment.save_fragments(str(models / 'toy' / 'fragments.pkl'), centers, sizes)
  _, rows = _infer(models, [])
  assert rows[0].startswith('scene_id')


@pytest.mark.parametrize('sparse', [False, True], ids=['dense', 'sparse'])
def test_bench_f256_prints_its_json_line(sparse, gpu_children):
  cmd = ['timeout', '-k', '10', '900', sys.executable, os.path.join(ROOT, 'bench.py'),
         '--num-frags', '256', '--steps', '3', '--warmup', '1', '--full', '--no-cpu-baseline',
         '--traffic', 'off'] + (['--sparse-heads'] if sparse else [])
  out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=930)
  assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
  lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
  assert len(lines) == 1
  d = json.loads(lines[0])
  assert d['value'] > 0 and d['config']['poses_per_step'] > 0
